"""The row-deferred Adam scheme without a GPU: the NumPy restatement (tests/sparse_update_reference.py) flushed equals dense Adam bit
for bit; a replay written as `m *= b1` does not (so the GPU tests' strictness is not vacuous); the `"sparse_update": true` key of
`sampled_batches`: what it requires, and that checkpoint metadata keeps it."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import sparse_update_reference as U  # noqa: E402

F, N, K, STEPS = 37, 4, 4, 40


def _run(seed, replay=U.adam_element, steps=STEPS):
    rng = np.random.default_rng([11, seed])
    p, m, v = U.special_values(rng, F, N)
    dense, deferred = U.Dense(p, m, v), U.Deferred(p, m, v, K, replay=replay)
    pending_seen = 0
    for step in range(1, steps + 1):
        # a touch pattern of its own every step: ~30 % of the rows, none at all every seventh step, all every eleventh
        named = rng.random(F) < 0.3
        if step % 7 == 0:
            named[:] = False
        if step % 11 == 0:
            named[:] = True
        g = np.where(named[:, None], rng.standard_normal((F, N)), 0.0).astype(np.float32)
        lr_t = U.step_size(1e-3 * (0.5 + rng.random()), step)                    # a varying lr_scale
        scale = U.clip_scale(np.sqrt((g.astype(np.float64) ** 2).sum()), 1.0 if step % 2 else 1e9)      # active and inactive clipping
        dense.step(g, lr_t, scale)
        deferred.catch_up(named)
        deferred.step(named, g, lr_t, scale)
        pending_seen = max(pending_seen, deferred.pending_rows())
    return dense, deferred, pending_seen


@pytest.mark.parametrize("seed", range(5))
def test_the_deferred_scheme_flushed_is_dense_adam_bit_for_bit(seed):
    dense, deferred, pending_seen = _run(seed)
    assert pending_seen > F // 2 and deferred.forced_flushes >= STEPS // K - 1       # rows really fell behind; the table really filled
    assert deferred.pending_rows() > 0
    stale = deferred.stamps < deferred.t
    assert not np.array_equal(U.bits(deferred.p[stale]), U.bits(dense.p[stale]))     # before the flush the stale rows differ
    deferred.flush()
    assert deferred.pending_rows() == 0 and deferred.base == deferred.t == dense.t == STEPS
    for name in ("p", "m", "v"):
        assert np.array_equal(U.bits(getattr(deferred, name)), U.bits(getattr(dense, name))), name
    assert np.isfinite(dense.p).all()


def test_a_replay_that_only_decays_the_slots_is_caught_by_a_negative_zero():
    """Row 0 starts at m = -0, p = -0 and is never touched: dense Adam turns m into +0 in its first step (b1 * -0 + (1-b1) * +0) and
    p = -0 - lr_t * (+0 / ...) stays -0; `m *= b1` keeps m = -0, and p = -0 - lr_t * (-0 / ...) = -0 + 0 becomes +0."""
    rng = np.random.default_rng(3)
    p, m, v = U.special_values(rng, F, N)
    assert np.signbit(p[0]).all() and np.signbit(m[0]).all()
    named = np.zeros(F, bool)
    named[5] = True
    g = np.where(named[:, None], 1.0, 0.0).astype(np.float32) * np.ones((F, N), np.float32)
    results = {}
    for which, replay in (("element", U.adam_element), ("shortcut", U.shortcut_element)):
        dense, deferred = U.Dense(p, m, v), U.Deferred(p, m, v, K, replay=replay)
        for step in (1, 2, 3):
            lr_t = U.step_size(1e-3, step)
            dense.step(g, lr_t)
            deferred.catch_up(named)
            deferred.step(named, g, lr_t)
        deferred.flush()
        results[which] = (dense, deferred)
    dense, good = results["element"]
    assert all(np.array_equal(U.bits(getattr(good, a)), U.bits(getattr(dense, a))) for a in "pmv")
    assert not np.signbit(dense.m[0]).any() and np.signbit(dense.p[0]).all()
    _, bad = results["shortcut"]
    assert np.array_equal(bad.m[0], dense.m[0]) and np.array_equal(bad.p[0], dense.p[0])        # equal as numbers ...
    assert not np.array_equal(U.bits(bad.m[0]), U.bits(dense.m[0]))                            # ... and different bits
    assert np.signbit(bad.m[0]).all()
    assert not np.array_equal(U.bits(bad.p), U.bits(dense.p)) or not np.array_equal(U.bits(bad.m), U.bits(dense.m))


def test_step_sizes_and_clip_scale_restate_the_launch_arguments():
    assert U.step_size(1e-3, 1) == np.float32(1e-3 * (1 - 0.999) ** 0.5 / (1 - 0.9))
    assert U.clip_scale(0.5, 1.0) == 1 and U.clip_scale(4.0, 1.0) == np.float32(0.25) and U.clip_scale(np.nan, 1.0) == 1
    assert U.clip_scale(np.inf, 1.0) == 0 and U.clip_scale(123.0, 0.0) == 1
    rowptr = U.rowptr_of(U.touch_patterns(F)["first and last"])
    assert rowptr.dtype == np.int32 and len(rowptr) == F + 1 and np.flatnonzero(np.diff(rowptr)).tolist() == [0, F - 1]


# ---- the task parameter ---------------------------------------------------------------------------------------------------------------
PLAIN = {"fanouts": [3, 2], "seeds_per_batch": 16, "seed": 1}
BOTH = dict(PLAIN, sparse_features=True)
ON = dict(BOTH, sparse_update=True)


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


def _cpu_model(task, **params):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(dict(dict(hidden_size=16, graph_num_layers=1, random_seed=1), **params))
    return RGCN_Model(p, task, device="cpu")


def test_the_key_requires_sparse_features():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import parse_sampled_batches
    task = _task(sampled_batches=ON, sparse_node_features=True)
    assert task.sampled_batches == ON and task.sparse_update is True
    assert _task(sampled_batches=BOTH, sparse_node_features=True).sparse_update is False and _task().sparse_update is False
    assert _task(sampled_batches=dict(BOTH, sparse_update=False), sparse_node_features=True).sparse_update is False
    with pytest.raises(ValueError, match="sparse_features"):
        _task(sampled_batches=dict(PLAIN, sparse_update=True))                             # the key without "sparse_features"
    with pytest.raises(ValueError, match="sparse_features"):
        _task(sampled_batches=dict(PLAIN, sparse_features=False, sparse_update=True))
    with pytest.raises(ValueError, match="sparse_node_features"):
        _task(sampled_batches=ON)                                                          # ... and without the task's sparse mode
    for value in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match="sparse_update"):
            parse_sampled_batches(dict(BOTH, sparse_update=value))
    assert "sparse_update" not in parse_sampled_batches(BOTH)
    assert "sampled_batches" not in _task().default_params()


def _loaded(task, num_features=10):
    task.load_synthetic(num_nodes=120, num_features=num_features, num_classes=4, num_train=30, num_valid=30, num_test=30)
    return task


def test_the_key_requires_adam_and_the_input_projection():
    with pytest.raises(ValueError, match="Adam"):
        _cpu_model(_loaded(_task(sampled_batches=ON, sparse_node_features=True)), optimizer="RMSProp")
    with pytest.raises(ValueError, match="Adam"):
        _cpu_model(_loaded(_task(sampled_batches=ON, sparse_node_features=True)), optimizer="SGD")
    with pytest.raises(ValueError, match="graph_model/dense/kernel"):
        _cpu_model(_loaded(_task(sampled_batches=ON, sparse_node_features=True), num_features=16))      # feature size == hidden size
    model = _cpu_model(_loaded(_task(sampled_batches=ON, sparse_node_features=True)))
    opt = model.optimizer
    assert opt._deferred is not None and model.optimizer.params[opt._deferred.index] is model.variables["graph_model/dense/kernel"]
    assert opt._deferred.capacity == 1024 and opt.pending_rows() == 0
    assert _cpu_model(_loaded(_task(sampled_batches=BOTH, sparse_node_features=True))).optimizer._deferred is None


def test_defer_rows_refuses_what_it_cannot_update():
    import torch
    from tf_gnn_samples_amd.models.optimizer import TFStyleOptimizer
    table, vector, odd = (torch.nn.Parameter(torch.zeros(s)) for s in ((6, 8), (8,), (6, 6)))
    for name in ("rmsprop", "sgd"):
        with pytest.raises(ValueError, match="Adam"):
            TFStyleOptimizer([table], name, 1e-3, 1.0).defer_rows(table)
    opt = TFStyleOptimizer([table, vector, odd], "adam", 1e-3, 1.0)
    for bad in (vector, odd, torch.nn.Parameter(torch.zeros((6, 8)))):
        with pytest.raises(ValueError):
            opt.defer_rows(bad)
    for capacity in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="capacity"):
            opt.defer_rows(table, capacity=capacity)
    with pytest.raises(RuntimeError, match="defer_rows"):
        opt.pending_rows()
    opt.defer_rows(table, capacity=4)
    assert opt.pending_rows() == 0 and opt._deferred.step_sizes.shape == (4,) and opt._deferred.stamps.tolist() == [0] * 6
    with pytest.raises(ValueError, match="one already is"):
        opt.defer_rows(table)
    opt.flush_deferred()                                   # nothing behind: no launch, also on the CPU
    with pytest.raises(ValueError, match="row pointer"):
        opt.rows_touched(torch.zeros(6, dtype=torch.int32))
    table.grad = torch.ones_like(table)
    with pytest.raises(RuntimeError, match="fused update"):
        opt.clip_and_step()                                # a CPU parameter: the row kernels are HIP, there is no fallback
    with pytest.raises(RuntimeError):
        opt.clip_and_step(device_step_count=True)


def test_checkpoint_metadata_keeps_the_key(tmp_path):
    from tf_gnn_samples_amd import models
    task = _loaded(_task(sampled_batches=ON, sparse_node_features=True))
    assert task.get_metadata()["params"]["sampled_batches"] == ON
    model = _cpu_model(task)
    path = str(tmp_path / "model.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.sampled_batches == ON and restored.task.sparse_update is True
    assert restored.task.get_metadata() == task.get_metadata()
    assert restored.optimizer._deferred is not None and restored.optimizer._deferred.base == restored.optimizer.t
    plain = _task()
    plain.restore_from_metadata(task.get_metadata())
    assert plain.sparse_update is True
