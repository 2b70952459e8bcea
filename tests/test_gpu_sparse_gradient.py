"""The compact row gradient on the GPU (csrc/sparse_gradient.hip, include/relgnn_sparse_gradient.h, TFStyleOptimizer.compact_row_gradient,
the citation task's `"sparse_gradient": true`): the named rows and the compact structure against tests/sparse_gradient_reference.py
element for element; the compact gradient against the rows of the dense one; the norm against relgnn_mt_l2norm over to_dense(), the
32 partials included; the row step on compact rows against the one on the dense gradient; two models from one seed, key on and off."""
import ctypes
import pickle
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sparse_gradient_reference as G  # noqa: E402
import sparse_update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu

V_MIXED = 1200


# ---- named rows and the compact structure ---------------------------------------------------------------------------------------------
def _named_cases():
    """name -> (held_words arguments, node list): F = 300 throughout."""
    every = np.arange(V_MIXED, dtype=np.int32)
    single, full = np.zeros(300, np.int64), 1 + np.arange(300) % 3
    single[17] = 5
    return {"mixed lengths": ((G.mixed_lengths(), V_MIXED), every),
            "a node twice": ((G.mixed_lengths(), V_MIXED), np.concatenate([every[::-1], every[40:41]]).astype(np.int32)),
            "T = 0": ((single, 64), np.zeros(0, np.int32)),
            "T = 0 of nodes without words": ((np.zeros(300, np.int64), 64), np.arange(9, dtype=np.int32)),
            "T = 1": ((single, 64), np.arange(64, dtype=np.int32)),
            "T = F": ((full, 64), np.arange(64, dtype=np.int32))}


def _source(args):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    return SparseRows(*G.held_words(*args))


def _arrays(named):
    s = named.structure
    return {"words": named.words, "slot": named.slot, "rowptr": s.rowptr, "slabs": s.slabs, "combos": s.combos}


@pytest.mark.parametrize("name", list(_named_cases()))
def test_named_rows_equal_the_reference(gpu_device, name):
    args, nodes = _named_cases()[name]
    host = _source(args)
    taken = host.to(gpu_device).take_rows(torch.as_tensor(nodes, device=gpu_device), named_rows=True)
    on_host = host.take_rows(nodes, named_rows=True)                       # the host constructor, NumPy named rows
    assert taken.has_named_rows and on_host.has_named_rows and taken.is_cuda and not on_host.is_cuda
    t = taken.transposed
    want = G.compact_structure(t.rowptr.cpu().numpy(), t.slabs.cpu().numpy(), t.combos.cpu().numpy())
    T = len(want["words"])
    assert T == {"T = 0": 0, "T = 0 of nodes without words": 0, "T = 1": 1, "T = F": 300}.get(name, 7)
    got, got_host = _arrays(taken.named_rows()), _arrays(on_host.named_rows())
    for key in want:
        assert got[key].dtype == torch.int32 and got[key].is_cuda
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
        assert np.array_equal(got_host[key].numpy(), want[key]), key + " (host)"
    s = taken.named_rows().structure
    assert s.col is t.col and s.val is t.val and s.ws_rows == t.ws_rows and s.num_rows == T and s.num_cols == len(nodes)
    if name == "mixed lengths":
        assert np.diff(want["rowptr"]).tolist() == [1, 128, 129, 512, 513, 1100, 2]
        per_row = np.bincount(want["slabs"][:, 0], minlength=T).tolist()
        assert per_row == [0, 0, 1, 1, 2, 3, 0] and want["combos"][:, 0].tolist() == [4, 5]
    # a container that was not asked builds the same arrays when it is (one more read-back), once
    lazy = host.to(gpu_device).take_rows(torch.as_tensor(nodes, device=gpu_device))
    assert not lazy.has_named_rows
    again = _arrays(lazy.named_rows())
    assert lazy.named_rows() is lazy.named_rows() and all(np.array_equal(again[k].cpu().numpy(), want[k]) for k in want)


def test_nothing_is_written_behind_the_stated_sizes(gpu_device):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    args, nodes = _named_cases()["mixed lengths"]
    t = _source(args).to(gpu_device).take_rows(torch.as_tensor(nodes, device=gpu_device)).transposed
    want = G.compact_structure(t.rowptr.cpu().numpy(), t.slabs.cpu().numpy(), t.combos.cpu().numpy())
    F, T, S, C, pad = 300, 7, int(t.slabs.shape[0]), int(t.combos.shape[0]), 37
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=gpu_device)
    slot, sizes = i32(F + 1 + pad), i32(9 + pad)
    nbytes = lib.relgnn_named_rows_workspace_bytes(F)
    ws = _lib.scratch(nbytes, gpu_device)
    _lib.launch("relgnn_named_rows_count", _lib.ptr(t.rowptr), F, _lib.ptr(slot), sizes[8:].data_ptr(), _lib.ptr(ws), nbytes)
    out = {"words": i32(T + pad), "rowptr": i32(T + 1 + pad), "slabs": i32(S + pad, 4), "combos": i32(C + pad, 3)}
    _lib.launch("relgnn_named_rows_fill", _lib.ptr(t.rowptr), F, _lib.ptr(slot), T, _lib.ptr(out["words"]), _lib.ptr(out["rowptr"]),
                _lib.ptr(t.slabs), _lib.ptr(out["slabs"]), S, _lib.ptr(t.combos), _lib.ptr(out["combos"]), C)
    sizes = sizes.cpu().numpy()
    assert sizes[8] == T and (np.delete(sizes, 8) == -7).all()            # the count, one int behind the eight sizes, and nothing else
    out = dict(out, slot=slot)
    for key, size in (("words", T), ("rowptr", T + 1), ("slabs", S), ("combos", C), ("slot", F + 1)):
        host = out[key].cpu().numpy()
        assert np.array_equal(host[:size], want[key]), key
        assert len(host[size:]) == pad and (host[size:] == -7).all(), key + ": written behind the stated size"
    # a capacity below the count: the stores stop at it (a caller's mistake costs rows, never memory)
    short = {"words": i32(T + pad), "rowptr": i32(T + 1 + pad)}
    _lib.launch("relgnn_named_rows_fill", _lib.ptr(t.rowptr), F, _lib.ptr(slot), 3, _lib.ptr(short["words"]), _lib.ptr(short["rowptr"]),
                None, None, 0, None, None, 0)
    assert short["words"].cpu().numpy()[:3].tolist() == want["words"][:3].tolist() and (short["words"].cpu().numpy()[3:] == -7).all()
    assert (short["rowptr"].cpu().numpy()[4:] == -7).all()


# ---- the compact gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["tanh", "linear"])
@pytest.mark.parametrize("n", [4, 12, 64, 256, 1024])
def test_compact_gradient_is_the_named_rows_of_the_dense_one(gpu_device, n, act):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.models.optimizer import RowGradientSink
    args, nodes = _named_cases()["a node twice"]
    rows = _source(args).to(gpu_device).take_rows(torch.as_tensor(nodes, device=gpu_device), named_rows=True)
    act_id = ops.activation_id(None if act == "linear" else act)
    rng = np.random.default_rng([9, n])
    weight = (rng.standard_normal((300, n)) * 0.05).astype(np.float32)
    gout = torch.as_tensor(G.spread_values(rng, np.arange(len(nodes)), n), device=gpu_device)
    sink = RowGradientSink(300, n)
    results = []
    for use in (None, sink):
        W = torch.as_tensor(weight, device=gpu_device).clone().requires_grad_(True)
        out = ops.csr_rows_project(rows, W, act_id, row_gradient_sink=use)
        assert ops.ROUTES["csr_project"] == "hip"
        out.backward(gout)
        results.append((out.detach(), W.grad))
    (out_dense, dense), (out_compact, none) = results
    assert none is None and torch.equal(out_dense, out_compact)
    gradient = sink.gradient
    words = gradient.words.cpu().numpy()
    assert words.tolist() == sorted(G.MIXED_LENGTHS) and tuple(gradient.values.shape) == (7, n)
    dense_bits = U.bits(dense.cpu().numpy())
    assert np.array_equal(U.bits(gradient.values.cpu().numpy()), dense_bits[words])
    rest = np.ones(300, bool)
    rest[words] = False
    assert not dense_bits[rest].any() and dense_bits[words].any(axis=1).all()            # +0 outside the named rows
    assert np.array_equal(U.bits(gradient.to_dense().cpu().numpy()), dense_bits)
    with pytest.raises(RuntimeError, match="second deposit"):                            # the sink still holds this step's rows
        ops.csr_rows_project(rows, torch.as_tensor(weight, device=gpu_device).requires_grad_(True), act_id, row_gradient_sink=sink).backward(gout)
    sink.clear()
    bare = _source(args).to(gpu_device).take_rows(torch.as_tensor(nodes, device=gpu_device))
    with pytest.raises(RuntimeError, match="named rows"):
        ops.csr_rows_project(bare, torch.as_tensor(weight, device=gpu_device).requires_grad_(True), act_id, row_gradient_sink=sink).backward(gout)


# ---- the norm -------------------------------------------------------------------------------------------------------------------------
def _dense_norm(dense: torch.Tensor):
    """relgnn_mt_l2norm over one tensor -> (its 32 partials, the float), as bits."""
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    nbytes = lib.relgnn_mt_l2norm_workspace_bytes()
    ws = torch.full((nbytes // 8,), -1.0, dtype=torch.float64, device=dense.device)
    norm = torch.full((1,), -1.0, dtype=torch.float32, device=dense.device)
    _lib.launch("relgnn_mt_l2norm", (ctypes.c_void_p * 1)(dense.data_ptr()), (ctypes.c_int64 * 1)(dense.numel()), 1, _lib.ptr(norm), _lib.ptr(ws),
                nbytes)
    return G.bits64(ws[:32].cpu().numpy()), G.bits32(norm.cpu().numpy())


def _compact_norm(words: torch.Tensor, values: torch.Tensor, F: int):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    assert lib.relgnn_rows_l2norm_workspace_bytes() == 256
    ws = torch.full((32 + 5,), -1.0, dtype=torch.float64, device=values.device)
    norm = torch.full((1 + 5,), -1.0, dtype=torch.float32, device=values.device)
    T, n = int(values.shape[0]), int(values.shape[1])
    _lib.launch("relgnn_rows_l2norm", _lib.ptr(words) if T else None, T, _lib.ptr(values, rows_strided=True) if T else None,
                values.stride(0) if T else n, n, F, _lib.ptr(norm), _lib.ptr(ws), 256)
    assert (ws[32:] == -1).all() and (norm[1:] == -1).all()
    return G.bits64(ws[:32].cpu().numpy()), G.bits32(norm[:1].cpu().numpy())


@pytest.mark.parametrize("F,n", G.NORM_SHAPES)
def test_norm_has_the_dense_launch_s_partials_and_float(gpu_device, F, n):
    from tf_gnn_samples_amd.models.optimizer import RowGradient
    assert F * n > G.SLOTS
    for name in ("one", "all", "one residue", "ends", "tenth"):
        words, values = G.norm_case(F, n, name)
        gradient = RowGradient(torch.as_tensor(words, device=gpu_device), None, torch.as_tensor(values, device=gpu_device), F)
        want = _dense_norm(gradient.to_dense())
        got = _compact_norm(gradient.words, gradient.values, F)
        reference = G.compact_norm(words, values)
        assert np.array_equal(got[0], want[0]), (name, "partials", int((got[0] != want[0]).sum()))
        assert np.array_equal(got[1], want[1]), (name, "norm")
        assert np.array_equal(got[0], G.bits64(reference[0])) and got[1][0] == G.bits32(reference[1]), (name, "against the restatement")
    # rows with a leading dimension above n
    words, values = G.norm_case(F, n, "tenth")
    wide = torch.full((len(words), n + 8), 3.0, dtype=torch.float32, device=gpu_device)
    wide[:, :n] = torch.as_tensor(values, device=gpu_device)
    got = _compact_norm(torch.as_tensor(words, device=gpu_device), wide[:, :n], F)
    assert np.array_equal(got[0], G.bits64(G.compact_norm(words, values)[0]))


@pytest.mark.parametrize("F,n", [(5000, 12), (300, 256)])
def test_norm_non_finite_empty_and_on_a_side_stream(gpu_device, F, n):
    from tf_gnn_samples_amd.models.optimizer import RowGradient
    words, values = G.norm_case(F, n, "tenth")
    for poison in (np.inf, -np.inf, np.nan):
        bad = values.copy()
        bad[len(words) // 2, n - 3] = poison
        gradient = RowGradient(torch.as_tensor(words, device=gpu_device), None, torch.as_tensor(bad, device=gpu_device), F)
        want, got = _dense_norm(gradient.to_dense()), _compact_norm(gradient.words, gradient.values, F)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), poison
        assert not np.isfinite(got[1].view(np.float32)[0])
    empty = _compact_norm(torch.zeros(0, dtype=torch.int32, device=gpu_device), torch.zeros((0, n), device=gpu_device), F)
    assert not empty[0].any() and not empty[1].any()                                    # T = 0: +0, every partial too
    w, v = torch.as_tensor(words, device=gpu_device), torch.as_tensor(values, device=gpu_device)
    main = _compact_norm(w, v, F)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        on_side = _compact_norm(w, v, F)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert np.array_equal(main[0], on_side[0]) and np.array_equal(main[1], on_side[1])
    assert np.array_equal(main[0], G.bits64(G.compact_norm(words, values)[0]))


# ---- the row step ---------------------------------------------------------------------------------------------------------------------
def _optimizer_pair(device, rows, width, clip, seed):
    """Two TFStyleOptimizers over equal copies of (vector, [rows, width] table, matrix), the table row-deferred with capacity 4 in
    both; the second takes its gradient compact."""
    from tf_gnn_samples_amd.models.optimizer import TFStyleOptimizer
    rng = np.random.default_rng([41, seed])
    p, m, v = U.special_values(rng, rows, width)
    others = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in ((5,), (3, 7))]
    made = []
    for compact in (False, True):
        params = [torch.nn.Parameter(torch.as_tensor(a, device=device).clone()) for a in (others[0], p, others[1])]
        opt = TFStyleOptimizer(params, "adam", 1e-3, clip)
        opt.m[1].copy_(torch.as_tensor(m, device=device))
        opt.v[1].copy_(torch.as_tensor(v, device=device))
        opt.defer_rows(params[1], capacity=4)
        if compact:
            opt.compact_row_gradient()
        made.append((opt, params))
    return made


def _raw_state(opt):
    d = opt._deferred
    tensors = list(opt.params) + opt.m + opt.v + [d.step_sizes]
    return [U.bits(t.detach().cpu().numpy()).copy() for t in tensors] + [d.stamps.cpu().numpy().copy(), np.array([d.base, opt.t])]


@pytest.mark.parametrize("clip", [0.05, 1e9], ids=["clip active", "clip inactive"])
def test_six_steps_on_compact_rows_equal_the_steps_on_the_dense_gradient(gpu_device, clip):
    rows, width = 300, 32
    (dense, dense_params), (compact, compact_params) = _optimizer_pair(gpu_device, rows, width, clip, seed=int(clip > 1))
    sink = compact.row_gradient_sink
    rng = np.random.default_rng([42, int(clip > 1)])
    flushes = 0
    for step in range(1, 7):
        named = rng.random(rows) < (0.0 if step == 4 else 0.3)                           # step 4 names nothing: T = 0
        words = np.flatnonzero(named).astype(np.int32)
        values = rng.standard_normal((len(words), width)).astype(np.float32)
        g = G.to_dense(words, values, rows)
        small = [rng.standard_normal(tuple(q.shape)).astype(np.float32) for q in (dense_params[0], dense_params[2])]
        rowptr = torch.as_tensor(U.rowptr_of(named), device=gpu_device)
        slot = torch.as_tensor(np.concatenate([[0], np.cumsum(named)]).astype(np.int32), device=gpu_device)
        lr_scale = 0.5 + rng.random()
        for opt, params in ((dense, dense_params), (compact, compact_params)):
            opt.zero_grad()
            params[0].grad, params[2].grad = (torch.as_tensor(a, device=gpu_device).clone() for a in small)
            opt.rows_touched(rowptr)
            if opt is dense:
                params[1].grad = torch.as_tensor(g, device=gpu_device)
            else:
                sink.deposit(SimpleNamespace(words=torch.as_tensor(words, device=gpu_device), slot=slot, count=len(words)),
                             torch.as_tensor(values, device=gpu_device))
            base = opt._deferred.base
            opt.clip_and_step(lr_scale)
            flushes += int(opt is compact and opt._deferred.base != base)
        assert dense.t == compact.t == step and sink.gradient is None and compact_params[1].grad is None
        for a, b in zip(_raw_state(dense), _raw_state(compact)):                         # raw: stale rows and all
            assert np.array_equal(a, b), step
        assert compact.pending_rows() == dense.pending_rows()
    assert flushes == 1 and compact.pending_rows() > 0                                   # the table of four step sizes filled up once
    compact.flush_deferred(), dense.flush_deferred()
    assert all(np.array_equal(a, b) for a, b in zip(_raw_state(dense), _raw_state(compact)))
    # the refusals of a step
    compact.zero_grad()
    compact_params[0].grad = torch.zeros_like(compact_params[0])
    with pytest.raises(RuntimeError, match="no gradient"):                               # other variables step, the sink is empty
        compact.clip_and_step()
    compact_params[1].grad = torch.zeros_like(compact_params[1])
    with pytest.raises(RuntimeError, match="dense gradient"):
        compact.clip_and_step()
    compact.zero_grad()
    compact.clip_and_step()                                                              # nothing to do: no step
    assert compact.t == 6


# ---- the model ------------------------------------------------------------------------------------------------------------------------
UPDATE = {"fanouts": [3, 2], "seeds_per_batch": 16, "seed": 2, "sparse_features": True, "sparse_update": True}
ON = dict(UPDATE, sparse_gradient=True)
KERNEL = "graph_model/dense/kernel"
SYNTHETIC = dict(num_nodes=300, num_features=200, num_classes=3, feature_density=0.008, seed=5, num_train=60, num_valid=60, num_test=60)


def _task(sampled, **synthetic):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True, sampled_batches=sampled))
    task.load_synthetic(**dict(SYNTHETIC, **synthetic))
    return task


def _model(name, task, device, result_dir, run_id, hidden=64):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(hidden_size=hidden, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=6)
    return cls(p, task, run_id=run_id, result_dir=str(result_dir), device=str(device))


@pytest.mark.parametrize("model_name", ["RGCN_Model", "GGNN_Model"])
def test_two_models_from_one_seed_key_on_and_key_off(gpu_device, tmp_path, model_name):
    from tf_gnn_samples_amd.tasks import DataFold
    on, off = (_model(model_name, _task(s), gpu_device, tmp_path, run_id) for s, run_id in ((ON, "on"), (UPDATE, "off")))
    assert on.task.sparse_gradient and not off.task.sparse_gradient
    assert on.optimizer.row_gradient_sink is not None and off.optimizer.row_gradient_sink is None and off.optimizer._deferred is not None
    steps = 0
    for epoch in range(2):
        pairs = zip(on._batches(on.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN), off._batches(off.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN))
        for batch_on, batch_off in pairs:
            assert torch.equal(batch_on.extra["sampled_nodes"], batch_off.extra["sampled_nodes"])
            rows_on, rows_off = batch_on.extra["sparse_node_features"], batch_off.extra["sparse_node_features"]
            assert rows_on.has_named_rows and not rows_off.has_named_rows
            assert 0 < rows_on.named_rows().count <= 200
            loss_on = np.float32(float(on.train_step(batch_on)["loss"].detach()))
            loss_off = np.float32(float(off.train_step(batch_off)["loss"].detach()))
            steps += 1
            assert np.isfinite(loss_on) and loss_on.view(np.uint32) == loss_off.view(np.uint32), (steps, loss_on, loss_off)
            assert on.variables[KERNEL].grad is None and off.variables[KERNEL].grad is not None
            assert on.optimizer.row_gradient_sink.gradient is None
            assert all(on.variables[k].grad is not None for k in on.variables.names() if k != KERNEL)
        valid = [m._run_epoch("valid", m.task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, quiet=True) for m in (on, off)]
        assert valid[0][0] == valid[1][0] and np.isfinite(valid[0][0])
    assert steps == 8 and on.optimizer.t == off.optimizer.t == 8
    batch_on, batch_off = (next(iter(m._batches(m.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN))) for m in (on, off))
    on.train_step(batch_on), off.train_step(batch_off)
    assert on.optimizer.pending_rows() == off.optimizer.pending_rows() > 0
    saved = {}
    for name, model in (("on", on), ("off", off)):
        model.save_model(str(tmp_path / (name + ".pickle")))
        with open(tmp_path / (name + ".pickle"), "rb") as f:
            saved[name] = pickle.load(f)
    assert saved["on"]["task_params"]["sampled_batches"] == ON and saved["off"]["task_params"]["sampled_batches"] == UPDATE
    w_on, w_off = saved["on"]["weights"], saved["off"]["weights"]
    assert sorted(w_on) == sorted(w_off) and KERNEL + "/Adam_1:0" in w_on
    for key in w_on:
        assert np.array_equal(U.bits(np.asarray(w_on[key], np.float32)), U.bits(np.asarray(w_off[key], np.float32))), key


def test_a_full_graph_sparse_batch_builds_its_named_rows_when_asked(gpu_device, tmp_path):
    """A training step on the fold's own container (no per-batch take_rows): the model asks it for its named rows."""
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    on, off = (_model("RGCN_Model", _task(s), gpu_device, tmp_path, run_id) for s, run_id in ((ON, "on"), (UPDATE, "off")))
    losses = []
    for model in (on, off):
        (mb,) = model.task.make_minibatch_iterator(model.task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, 10 ** 6)
        losses.append([float(model.train_step(DeviceBatch(mb, gpu_device))["loss"].detach()) for _ in range(2)])
        model.optimizer.flush_deferred()
    assert losses[0] == losses[1] and on.variables[KERNEL].grad is None
    assert all(torch.equal(on.variables[k], off.variables[k]) for k in on.variables.names())


def test_a_step_allocates_no_dense_gradient(gpu_device, tmp_path):
    """F = V = 2^16 identity features, hidden 256: the step's peak with the key lies below the peak without it by at least
    0.9 (F - T) n 4 bytes, T the batches' largest named count — the dense [F, n] gradient is gone, [T, n] took its place."""
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    F, n = 2 ** 16, 256
    peaks, named = {}, []
    for which, sampled in (("off", UPDATE), ("on", ON)):
        task = _task(dict(sampled, seeds_per_batch=64), num_nodes=F, num_features=F, feature_density=0.0, num_train=512, num_valid=64,
                     num_test=64)
        host = SparseRows(np.arange(F + 1), np.arange(F), np.ones(F, np.float32), (F, F))
        for fold in (DataFold.TRAIN, DataFold.VALIDATION):
            task._loaded_data[fold] = [f._replace(node_features=host) for f in task._loaded_data[fold]]
        model = _model("RGCN_Model", task, gpu_device, tmp_path, which, hidden=n)
        batches = iter(model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN))
        model.train_step(next(batches))                                                  # warm: plans, scratch, the library's handles
        model.optimizer.zero_grad()                                                      # (a step leaves its gradients behind: not part of `before`)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(gpu_device)
        before = torch.cuda.memory_allocated(gpu_device)
        for _ in range(2):
            batch = next(batches)
            named.append(int((torch.diff(batch.extra["sparse_node_features"].transposed.rowptr) > 0).sum()))
            model.train_step(batch)
            assert (model.variables[KERNEL].grad is None) == (which == "on")
            model.optimizer.zero_grad()
            del batch
        torch.cuda.synchronize()
        peaks[which] = torch.cuda.max_memory_allocated(gpu_device) - before
        del model, batches, task
    T = max(named)
    margin = 0.9 * (F - T) * n * 4
    print("peak %.1f MiB with the key, %.1f MiB without; T = %d of %d, margin asked %.1f MiB"
          % (peaks["on"] / 2 ** 20, peaks["off"] / 2 ** 20, T, F, margin / 2 ** 20))
    assert 0 < T < F // 4 and peaks["on"] <= peaks["off"] - margin
