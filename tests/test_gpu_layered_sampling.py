"""Layered sampled batches on the GPU (csrc/neighbour_sample.hip: the hop-ordered relabel and degree kernels; tasks/neighbour_sampling.py:
NeighbourSampler.sample_by_hop, HopSubgraph.device_batch; models/sparse_graph_model.py: the level graphs): the kernels against
tests/layered_sampling_reference.py bit for bit, a layered step against the un-layered step on the same HopSubgraph with a float64 run
of the un-layered model between them, the key together with the three sparse keys, and train() with the key."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import layered_sampling_reference as LR  # noqa: E402

pytestmark = pytest.mark.gpu

V = LR.V


def device_graph(L, device):
    from tf_gnn_samples_amd.graph import RelGraph
    adjacency, (rowptr, col, _) = LR.graph(L)
    g = RelGraph([torch.as_tensor(a, device=device) for a in adjacency], V)
    assert np.array_equal(g.rowptr_t.cpu().numpy(), rowptr) and np.array_equal(g.col_t.cpu().numpy(), col)
    return g


def check_against_reference(sub, want, what):
    assert sub.num_nodes == len(want.nodes) and sub.num_edges == sum(len(a) for a in want.adjacency_lists), what
    assert sub.nodes.dtype == torch.int32 and np.array_equal(sub.nodes.cpu().numpy(), want.nodes), what
    assert len(sub.adjacency_lists) == len(want.adjacency_lists)
    for l, (got, ref) in enumerate(zip(sub.adjacency_lists, want.adjacency_lists)):
        assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape and np.array_equal(got.cpu().numpy(), ref), (what, l)
    got = sub.type_to_num_incoming_edges
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.degrees.view(np.uint32)), what
    assert np.array_equal(sub.seed_mask.cpu().numpy().view(np.uint32), want.seed_mask.view(np.uint32)), what
    if hasattr(want, "hop_nodes"):
        assert sub.hop_nodes == want.hop_nodes and sub.hop_edges == want.hop_edges, what
        assert all(type(x) is int for x in sub.hop_nodes) and all(type(x) is int for e in sub.hop_edges for x in e)


@pytest.mark.parametrize("fanouts", [[3, 2], [2, 2, 2], [0, 4]])
@pytest.mark.parametrize("L", [2, 3])
def test_kernels_reproduce_the_reference_bit_for_bit(gpu_device, L, fanouts):
    """Every output array, hop_nodes and hop_edges; the same draws as sample(); the level graphs' views and degree tables; stamps all
    zero after every call and after a refused seed list."""
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    _, (rowptr, col, _) = LR.graph(L)
    sampler = NeighbourSampler(device_graph(L, gpu_device), fanouts, seed=11, replica=2)
    H = len(fanouts)
    for name, seeds in LR.seed_lists(L).items():
        for draw in (0, 7):
            want = LR.sample_by_hop(rowptr, col, V, L, seeds, fanouts, draw, seed=11, replica=2)
            sub = sampler.sample_by_hop(torch.as_tensor(seeds, device=gpu_device), draw)
            check_against_reference(sub, want, (L, fanouts, name, draw))
            assert not sampler.stamp.any()                            # all zero after every call
            check_against_reference(sampler.sample(seeds, draw), want.by_id, (L, fanouts, name, draw, "by id"))
            assert not sampler.stamp.any()
            levels = sub.level_graphs()
            assert len(levels) == H
            for level, (lists, sources, targets, table) in zip(levels, LR.levels(want)):
                assert (level.num_sources, level.num_targets) == (sources, targets)
                assert np.array_equal(level.type_to_num_incoming_edges.cpu().numpy().view(np.uint32), table.view(np.uint32))
                for got, base, ref in zip(level.adjacency_lists, sub.adjacency_lists, lists):
                    assert got.data_ptr() == base.data_ptr() or got.numel() == 0              # a prefix view, no copy
                    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), ref)
    # a host array in any order is the same seed list
    seeds = LR.seed_lists(L)["mixed"]
    check_against_reference(sampler.sample_by_hop(seeds[::-1].copy(), 7),
                            LR.sample_by_hop(rowptr, col, V, L, seeds, fanouts, 7, seed=11, replica=2), "host seeds")
    for bad in (np.array([1, 1], np.int32), np.array([-1], np.int32), np.array([V], np.int32), np.zeros(0, np.int32), np.array([1], np.int64)):
        with pytest.raises(ValueError):
            sampler.sample_by_hop(bad, 0)
    assert not sampler.stamp.any()


def test_state_and_streams(gpu_device):
    """The two numberings in turn on one sampler: the stamps are clean in between.  The same bits on a stream that is not the default
    one.  A call that raises behind the hops leaves the stamps zero."""
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    L, fanouts = 2, [3, 2]
    _, (rowptr, col, _) = LR.graph(L)
    sampler = NeighbourSampler(device_graph(L, gpu_device), fanouts, seed=5)
    lists = LR.seed_lists(L)
    want = {name: LR.sample_by_hop(rowptr, col, V, L, seeds, fanouts, 3, seed=5) for name, seeds in lists.items()}
    for name in ("mixed", "mixed", "single", "all", "isolated", "mixed"):
        check_against_reference(sampler.sample_by_hop(torch.as_tensor(lists[name], device=gpu_device), 3), want[name], name)
        assert not sampler.stamp.any()
        check_against_reference(sampler.sample(lists[name], 3), want[name].by_id, name)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        for name in ("mixed", "all"):
            sub = sampler.sample_by_hop(torch.as_tensor(lists[name], device=gpu_device), 3)
            side.synchronize()
            check_against_reference(sub, want[name], name + " on a side stream")
            assert not sampler.stamp.any()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    # a call that raises after the hops stamped their nodes (the host refuses the relabel before anything is launched)
    real = _lib.launch

    def refusing(name, *args):
        if name == "relgnn_neighbour_sample_relabel_by_hop":
            raise _lib.RelGnnLibraryError("refused for the test")
        return real(name, *args)
    _lib.launch = refusing
    try:
        with pytest.raises(_lib.RelGnnLibraryError):
            sampler.sample_by_hop(lists["mixed"], 3)
    finally:
        _lib.launch = real
    assert not sampler.stamp.any()
    check_against_reference(sampler.sample_by_hop(lists["mixed"], 3), want["mixed"], "after a call that raised")


def test_bucketing_with_long_runs_of_empty_buckets(gpu_device):
    """A hop-ordered subgraph ends in its leaves, which are nobody's target: the by-target row pointer ends in one run of
    (n_H - n_{H-1}) * L equal entries.  csrc/plan.hip writes a run of 16 empty buckets or more with a whole wave: runs of 0 .. 17, 63,
    64, 65, 127, 128, 129 and 5000 buckets in front of a key, at the head, in the middle (also two long runs owned by one wave) and
    at the tail, by target and by source, against the NumPy bucketing."""
    import neighbour_sampling_reference as R
    from tf_gnn_samples_amd.graph import RelGraph
    L = 2
    runs = list(range(18)) + [63, 64, 65, 127, 128, 129, 5000, 3, 700, 900, 1]
    rng = np.random.default_rng(0)
    for head, tail in ((0, 0), (40, 9000), (17, 15), (5000, 16)):
        keys = head + np.cumsum(np.array(runs) + 1) - 1                  # bucket ids (node * L + type) that hold edges
        num_nodes = int(keys[-1] // L + 1 + tail)
        adjacency = []
        for l in range(L):
            tgt = np.repeat(keys[keys % L == l] // L, 3)
            src = (keys[rng.integers(0, len(keys), size=len(tgt))] // L)          # sources with the same gaps
            e = np.stack([src, tgt], axis=1)[rng.permutation(len(tgt))]
            adjacency.append(np.ascontiguousarray(e, dtype=np.int32))
        g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adjacency], num_nodes)
        rowptr, col, perm = R.bucketing(adjacency, num_nodes)
        assert np.array_equal(g.rowptr_t.cpu().numpy(), rowptr) and np.array_equal(g.col_t.cpu().numpy(), col), (head, tail)
        assert np.array_equal(g.perm_t.cpu().numpy(), perm)
        rowptr_s, _, perm_s = R.bucketing([a[:, ::-1] for a in adjacency], num_nodes)
        assert np.array_equal(g.rowptr_s.cpu().numpy(), rowptr_s) and np.array_equal(g.perm_s.cpu().numpy(), perm_s), (head, tail)


# ---- layered against un-layered on the same HopSubgraph ------------------------------------------------------------------------------
MODELS = ["RGCN_Model", "GGNN_Model", "RGAT_Model", "GNN_FiLM_Model"]          # the models tests/test_gpu_citation.py covers
FLOOR = 2.0 ** -22
_TASKS = {}


def _citation_task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    key = tuple(sorted((k, repr(v)) for k, v in params.items()))
    if key not in _TASKS:
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
        task.load_synthetic(num_nodes=600, num_features=48, num_classes=5, num_train=140, num_valid=150, num_test=150, feature_density=0.1,
                            seed=3)
        _TASKS[key] = task
    return _TASKS[key]


def _model(name, task, device, num_layers, **params):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(dict(dict(hidden_size=32, graph_num_layers=num_layers, graph_layer_input_dropout_keep_prob=1.0, random_seed=6), **params))
    return cls(p, task, device=str(device))


def _hop_subgraph(task, device, fanouts, num_seeds=32, draw=4):
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler, epoch_seed_batches
    fold = task._loaded_data[DataFold.TRAIN][0]
    g = RelGraph([torch.as_tensor(a, device=device) for a in fold.adjacency_lists], len(fold.labels))
    seeds = epoch_seed_batches(fold.mask, num_seeds, 0, 0)[0]
    return fold, NeighbourSampler(g, fanouts, seed=9).sample_by_hop(seeds, draw)


def _forward_and_gradients(model, batch, num_seeds):
    """-> {tensor name: float32 array} of the seed states, the seeds' logits, loss, num_correct and every variable's gradient."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.dense import dense
    for p in model.variables.parameters():
        p.grad = None
    final = model._final_node_states(batch, training=False)
    head = model.variables.scope(model._task_scope)
    metrics = model.task.compute_task_metrics(final, batch, head)
    metrics["loss"].backward()
    ops.join_deferred()
    with torch.no_grad():
        logits = dense(final.detach(), head["kernel"].detach())
    torch.cuda.synchronize()
    out = {"seed_states": final.detach()[:num_seeds], "logits": logits[:num_seeds], "loss": metrics["loss"].detach().reshape(1),
           "num_correct": metrics["num_correct"].reshape(1)}
    for n in model.variables.names():
        assert model.variables[n].grad is not None, n
        out["grad " + n] = model.variables[n].grad
    return {k: v.cpu().numpy().astype(np.float32).copy() for k, v in out.items()}, int(final.shape[0])


def _float64_run(model, model_name, fold, sub, dense_features=None):
    """The un-layered model on the union batch in float64: oracle/torch_model.py's driver over oracle/torch_ref.py's layers, the
    citation head (tasks/citation_network_task.py:133-148) on top."""
    from oracle import torch_model as TM, torch_ref as TR
    from tf_gnn_samples_amd.models.adapters import SPECS
    spec = next(s for s in SPECS if s.class_name == model_name)
    layer = getattr(TR, spec.layer_fn.__name__)
    p = model.params
    names = list(model.variables.names())
    W = {n[len("graph_model/"):]: model.variables[n].detach().cpu().double().requires_grad_(True) for n in names if n.startswith("graph_model/")}
    head = {n: model.variables[n].detach().cpu().double().requires_grad_(True) for n in names if not n.startswith("graph_model/")}

    def apply(layer_idx, h, adj, deg, timesteps, lw):
        kwargs = {kw: p[key] for kw, key in spec.layer_kwargs.items()}
        state_dim = kwargs.pop("state_dim")
        args = (h, adj, deg, state_dim) if spec.takes_in_degrees else (h, adj, state_dim)
        return layer(*args, num_timesteps=timesteps, weights=lw, **kwargs)
    nodes = sub.nodes.cpu().numpy().astype(np.int64)
    features = fold.node_features if dense_features is None else dense_features
    x = torch.as_tensor(np.asarray(features)[nodes]).double()
    adj = [a.cpu().long() for a in sub.adjacency_lists]
    deg = sub.type_to_num_incoming_edges.cpu().double()
    final = TM.graph_propagation(x, adj, deg, p, W, apply)
    (kernel,) = [v for k, v in head.items() if k.endswith("kernel")]
    logits = final @ kernel
    labels = torch.as_tensor(fold.labels[nodes]).long()
    mask = (sub.seed_mask.cpu().double() * torch.as_tensor(fold.mask[nodes]).double())
    losses = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    loss = (losses * mask).sum() / mask.sum()
    loss.backward()
    n0 = sub.hop_nodes[0]
    correct = ((logits.detach().argmax(1) == labels).double() * mask).sum()
    out = {"seed_states": final.detach()[:n0], "logits": logits.detach()[:n0], "loss": loss.detach().reshape(1), "num_correct": correct.reshape(1)}
    for n in names:
        out["grad " + n] = (W[n[len("graph_model/"):]] if n.startswith("graph_model/") else head[n]).grad
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def deviation(x, x64):
    return float(np.abs(x.astype(np.float64) - x64).max() / max(float(np.abs(x64).max()), 1e-300))


def check_relation(layered, plain, want, what):
    """Per tensor: the layered run's deviation from float64 is at most twice the un-layered run's, plus 2^-22.  The two runs add the same
    non-zero terms and differ by dropped zero terms, by the tile grouping of the weight-gradient sums and by a Dense route chosen from the
    row count, so their errors are of one size; the floor covers an un-layered run that happens to be exact.  Every figure is printed
    before anything is asserted."""
    rows = []
    for name in want:
        a, b = deviation(layered[name], want[name]), deviation(plain[name], want[name])
        same = np.array_equal(layered[name].view(np.uint32), plain[name].view(np.uint32))
        rows.append((name, a, b, same))
        print("%s %s: layered %.3g  un-layered %.3g  bound %.3g  identical bits: %s" % (what, name, a, b, 2 * b + FLOOR, same))
    for name, a, b, _ in rows:
        assert math.isfinite(a) and a <= 2 * b + FLOOR, (what, name, a, b)
    return rows


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("fanouts", [[3, 2], [3, 2, 2]])
@pytest.mark.parametrize("model_name", MODELS)
def test_layered_step_against_the_unlayered_step(gpu_device, model_name, fanouts, norm):
    """device_batch(layered=True) against device_batch(layered=False) on one HopSubgraph, keep-probabilities 1.0, default switches:
    seed states, logits, loss, num_correct and every variable's gradient, each against a float64 run of the un-layered model.  H = 3
    runs with a residual every 2 layers, so the kept tensor of layer 0 (n_3 rows) is cut to the n_1 rows layer 2 takes.

    A gradient that lost an activation derivative: the driver vouches for nothing in layered mode, and the row cut itself is a view,
    which carries no activation tag (activation_tags.py), so no consumer behind a cut can fold anything.  Were a tanh' lost all the
    same, every gradient below that Dense would be off by the factor 1 / (1 - y^2) per unit, O(1) of its size with |y| up to 1, against
    an un-layered deviation of some 1e-6: the relation fails by five orders of magnitude.  The GGNN, RGAT and the projection's tanh
    are on that path in every case here."""
    H = len(fanouts)
    task = _citation_task()
    fold, sub = _hop_subgraph(task, gpu_device, fanouts)
    n0 = sub.hop_nodes[0]
    assert n0 == 32 and n0 < sub.hop_nodes[1] < sub.hop_nodes[-1] == sub.num_nodes < len(fold.labels)
    model = _model(model_name, task, gpu_device, H, graph_inter_layer_norm=norm, graph_residual_connection_every_num_layers=2)
    tables = (torch.as_tensor(fold.node_features, device=gpu_device), torch.as_tensor(fold.labels, device=gpu_device),
              torch.as_tensor(fold.mask, device=gpu_device))
    layered_batch = sub.device_batch(*tables, 1.0, layered=True)
    plain_batch = sub.device_batch(*tables, 1.0, layered=False)
    assert "layer_graphs" not in plain_batch.extra and len(layered_batch.extra["layer_graphs"]) == H
    assert layered_batch.extra["labels"].shape == (n0,) and float(layered_batch.extra["mask"].sum()) == float(plain_batch.extra["mask"].sum()) == n0
    layered, rows_layered = _forward_and_gradients(model, layered_batch, n0)
    plain, rows_plain = _forward_and_gradients(model, plain_batch, n0)
    assert (rows_layered, rows_plain) == (n0, sub.num_nodes)
    want = _float64_run(model, model_name, fold, sub)
    assert float(np.abs(want["grad graph_model/dense/kernel"]).max()) > 0
    assert layered["num_correct"][0] == plain["num_correct"][0]
    rows = check_relation(layered, plain, want, "%s H=%d norm=%s" % (model_name, H, norm))
    forward = [same for name, _, _, same in rows if name in ("seed_states", "logits", "loss")]
    print("%s H=%d norm=%s: forward bit-identical at the seeds: %s; gradients bit-identical: %d of %d"
          % (model_name, H, norm, all(forward), sum(same for name, _, _, same in rows if name.startswith("grad ")),
             sum(1 for name, _, _, _ in rows if name.startswith("grad "))))


KERNEL = "graph_model/dense/kernel"
EVERY_KEY = {"fanouts": [3, 2], "seeds_per_batch": 32, "seed": 1, "sparse_features": True, "sparse_update": True, "sparse_gradient": True,
             "layered": True}


def test_the_key_composes_with_the_sparse_keys(gpu_device):
    """One training step with sparse_features, sparse_update, sparse_gradient and layered, against the same keys without layered on the
    same HopSubgraph, two models from one seed: the loss and the rows of the projection's weight the step updated obey the relation of
    check_relation against a float64 step (float64 gradient of the un-layered model, tf.clip_by_norm, Adam's first step)."""
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, resident_copy
    task = _citation_task(sparse_node_features=True, sampled_batches=EVERY_KEY)
    fold, sub = _hop_subgraph(task, gpu_device, EVERY_KEY["fanouts"])
    assert isinstance(fold.node_features, SparseRows)
    features = resident_copy(task._device_rows, fold.node_features, gpu_device)
    labels, mask = torch.as_tensor(fold.labels, device=gpu_device), torch.as_tensor(fold.mask, device=gpu_device)
    dense_features = fold.node_features.to_dense().cpu().numpy()       # (for the float64 run alone: [600, 48])
    results = {}
    for which in ("layered", "plain"):
        model = _model("RGCN_Model", task, gpu_device, 2)
        assert model.optimizer.row_gradient_sink is not None
        before = model.variables[KERNEL].detach().cpu().numpy().copy()
        if which == "layered":
            want = _float64_run(model, "RGCN_Model", fold, sub, dense_features=dense_features)
        batch = sub.device_batch(features, labels, mask, 1.0, named_rows=True, layered=which == "layered")
        assert ("layer_graphs" in batch.extra) == (which == "layered") and batch.extra["sparse_node_features"].has_named_rows
        metrics = model.train_step(batch)
        assert model.variables[KERNEL].grad is None                  # the compact gradient: no dense one
        model.optimizer.flush_deferred()
        torch.cuda.synchronize()
        after = model.variables[KERNEL].detach().cpu().numpy().copy()
        results[which] = (np.float32(float(metrics["loss"].detach())).reshape(1), before, after)
    assert np.array_equal(results["layered"][1], results["plain"][1])
    before = results["plain"][1].astype(np.float64)
    g = want["grad " + KERNEL]
    clip = float(model.params["clamp_gradient_norm"])
    g = g * clip / max(float(np.linalg.norm(g)), clip)
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, float(model.params["learning_rate"])
    lr_t = lr * (1 - b2) ** 0.5 / (1 - b1)
    after64 = before - lr_t * ((1 - b1) * g) / (np.sqrt((1 - b2) * g * g) + eps)
    touched = np.flatnonzero(np.abs(want["grad " + KERNEL]).max(axis=1) > 0)
    assert len(touched) > 0
    for which in results:                                            # the rows no word of the batch names did not move
        untouched = np.setdiff1d(np.arange(before.shape[0]), touched)
        assert np.array_equal(results[which][2][untouched], results[which][1][untouched]), which
    check_relation({"loss": results["layered"][0], "updated rows": results["layered"][2][touched]},
                   {"loss": results["plain"][0], "updated rows": results["plain"][2][touched]},
                   {"loss": want["loss"], "updated rows": after64[touched]}, "all keys")


# ---- training -----------------------------------------------------------------------------------------------------------------------
def _train_two_epochs(device, result_dir, sampled, **model_params):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sampled_batches=sampled))
    task.load_synthetic(seed=2)                                       # synthetic Cora: 2708 nodes, 140 of them in the train fold
    p = RGCN_Model.default_params()
    p.update(dict(dict(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3), **model_params))
    result_dir.mkdir()
    model = RGCN_Model(p, task, run_id="layered", result_dir=str(result_dir), device=str(device))
    record, run_epoch = [], model._run_epoch

    def recording(epoch_name, data, fold, quiet=False):
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, len(out[1]), out[2], [m.get("num_masked") for m in out[1]], [float(m["loss"]) for m in out[1]]))
        return out
    model._run_epoch = recording
    model.train(quiet=True, max_epochs=2)
    model._run_epoch = run_epoch
    torch.cuda.synchronize()
    return task, model, record


SAMPLED = {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1, "layered": True}


@pytest.mark.parametrize("native_batching", [True, False])
def test_train_with_the_key(gpu_device, tmp_path, native_batching):
    from tf_gnn_samples_amd import models
    task, model, record = _train_two_epochs(gpu_device, tmp_path / "a", SAMPLED, native_batching=native_batching)
    # ceil(140 / 32) = 5 steps per training epoch, one full-graph validation pass behind each
    assert [(r[1], r[2]) for r in record] == [(5, 5), (1, 1), (5, 5), (1, 1)], record
    assert record[0][3] == [32.0, 32.0, 32.0, 32.0, 12.0] and record[1][3] == [None]              # validation: no sampled batch
    assert all(math.isfinite(x) for r in record for x in r[4])
    assert (task.batches.epoch, task.batches.draw) == (2, 10)
    log = open(model.log_file).read()
    assert log.count(" Train: loss:") == 2 and log.count(" Valid: loss:") == 2 and "Acc:" in log
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.sampled_batches == SAMPLED and restored.task.layered
    (prediction,) = restored.predict(task.synthetic_test_data)         # the full graph
    assert prediction["classes"].shape == (2708,) and prediction["probabilities"].shape == (2708, 7)


@pytest.mark.parametrize("route", ["torch", "fused"])
def test_layer_input_dropout_runs_on_both_routes(gpu_device, tmp_path, monkeypatch, route):
    """keep-probability 0.8: the masks differ from the un-layered run's (torch draws by shape, the fused route by element index over
    another row count), so nothing is compared with it: the steps run, on hop-ordered batches with level graphs, and the losses are
    finite."""
    from tf_gnn_samples_amd import config, ops
    from tf_gnn_samples_amd.tasks import DataFold
    if route == "fused":
        monkeypatch.setattr(config.settings, "layer_dropout", "fused")
    calls = []
    for name in ("dropout", "dropout_residual"):
        monkeypatch.setattr(ops, name, lambda *args, _real=getattr(ops, name), _name=name: (calls.append(_name), _real(*args))[1])
    task, model, record = _train_two_epochs(gpu_device, tmp_path / route, dict(SAMPLED, fanouts=[5, 5, 5]), graph_num_layers=3,
                                            graph_layer_input_dropout_keep_prob=0.8, graph_residual_connection_every_num_layers=2)
    assert [(r[1], r[2]) for r in record] == [(5, 5), (1, 1), (5, 5), (1, 1)] and all(math.isfinite(x) for r in record for x in r[4])
    batch = next(iter(model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)))
    assert len(batch.extra["layer_graphs"]) == 3 and batch.extra["labels"].shape[0] == 32
    a = float(model.forward_batch(batch, training=True)["loss"].detach())
    b = float(model.forward_batch(batch, training=True)["loss"].detach())
    assert math.isfinite(a) and math.isfinite(b) and a != b            # two passes, two draws
    assert ("dropout" in calls and "dropout_residual" in calls) if route == "fused" else not calls


def test_a_layered_step_peaks_no_higher(gpu_device):
    """The peak device memory of a training step on device_batch(layered=True) is at most the peak of the step on
    device_batch(layered=False) of the same HopSubgraph (both measured from the same resting state, after a warming step each)."""
    task = _citation_task()
    fold, sub = _hop_subgraph(task, gpu_device, [5, 5], num_seeds=64)
    tables = (torch.as_tensor(fold.node_features, device=gpu_device), torch.as_tensor(fold.labels, device=gpu_device),
              torch.as_tensor(fold.mask, device=gpu_device))
    peaks = {}
    for which in ("plain", "layered"):
        model = _model("RGCN_Model", task, gpu_device, 2, hidden_size=128)
        batch = sub.device_batch(*tables, 1.0, layered=which == "layered")
        model.train_step(batch)                                        # warm: plans, scratch, the bucketing of every level
        model.optimizer.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(gpu_device)
        before = torch.cuda.memory_allocated(gpu_device)
        model.train_step(batch)
        model.optimizer.zero_grad()
        torch.cuda.synchronize()
        peaks[which] = torch.cuda.max_memory_allocated(gpu_device) - before
        del model, batch
    print("peak of a step above the resting state: un-layered %d bytes, layered %d bytes (%d nodes, %d one hop out, %d seeds)"
          % (peaks["plain"], peaks["layered"], sub.hop_nodes[2], sub.hop_nodes[1], sub.hop_nodes[0]))
    assert 0 < peaks["layered"] <= peaks["plain"], peaks
