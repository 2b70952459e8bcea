"""The node, edge and partition samplers of `subgraph_batches` (the key "sampler") on the GPU.  No kernel is new: a batch is
relgnn_neighbour_sample_begin or relgnn_subgraph_walk in front of the induced path, so what is held to tests/subgraph_samplers_reference.py
bit for bit here is the host plan's way onto the device: every batch's nodes, lists, degrees and per-edge weights, the visit counts of the
pre-sampling, the stamps left behind; then the task: a batch without a TRAIN node, train() and restore() per sampler, sparse features, and
two ranks over gloo against a one-process replay (tests/test_gpu_single_graph_dp.py's, over the cases of tests/subgraph_samplers_dp_cases.py)."""
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import subgraph_samplers_dp_cases as D  # noqa: E402
import subgraph_samplers_reference as P  # noqa: E402
from subgraph_samplers_reference import N, S  # noqa: E402

pytestmark = pytest.mark.gpu

V, SEED, WALK, EPOCHS, CAP = P.V, 5, 2, 2, 1e4
CASES = [("walk", 16), ("walk", 64), ("node", 16), ("node", 64), ("edge", 16), ("edge", 64), ("parts", 1), ("parts", 5)]
NORM = {"presample_epochs": EPOCHS}


def _value(sampler, per_batch, parts_path=None, **more):
    value = {"sampler": sampler, "seed": SEED, "normalisation": dict(NORM)}
    if sampler == "parts":
        value.update(parts_path=str(parts_path), parts_per_batch=per_batch)
    else:
        value.update(roots_per_batch=per_batch)
    if sampler == "walk":
        value.update(walk_length=WALK)
    return dict(value, **more)


def _device_graph(graph, device):
    from tf_gnn_samples_amd.graph import RelGraph
    g = RelGraph([torch.as_tensor(a, device=device) for a in graph.adjacency], graph.num_nodes)
    assert np.array_equal(g.rowptr_t.cpu().numpy(), graph.rowptr_t) and np.array_equal(g.col_t.cpu().numpy(), graph.col_t)
    return g


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.uint32)


def _sampler_and_plan(graph, device, sampler, per_batch, tmp_path):
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, parse_subgraph_batches, sampler_plan
    np.save(tmp_path / "parts.npy", graph.parts)
    plan = sampler_plan(parse_subgraph_batches(_value(sampler, per_batch, tmp_path / "parts.npy")), graph.mask, graph.adjacency, graph.num_nodes)
    steps = WALK if sampler == "walk" else plan.walk_steps
    assert steps == {"walk": WALK, "edge": 1, "node": 0, "parts": 0}[sampler]
    return SubgraphSampler(_device_graph(graph, device), steps, seed=SEED), plan


# ---- 1. every batch and the pre-sampling against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("sampler, per_batch", CASES)
def test_batches_weights_and_visit_counts_equal_the_reference(gpu_device, tmp_path, sampler, per_batch, L):
    from tf_gnn_samples_amd.tasks.subgraph_sampling import epoch_node_lists
    from test_gpu_subgraph_batches import check_against_reference
    graph = P.sampler_graph(L)
    rowptr, col = graph.rowptr_t, graph.col_t
    device_sampler, plan = _sampler_and_plan(graph, gpu_device, sampler, per_batch, tmp_path)
    # the pre-sampling: E = 2 epochs of the plan's lists, stamped by the sampler's own front, counted without a read-back
    counts = device_sampler.presample_lists(lambda epoch: epoch_node_lists(plan, epoch), EPOCHS, plan.longest(), plan.walked)
    sets = P.presampled_node_sets(sampler, graph, per_batch, SEED, EPOCHS, WALK)
    node_visits, edge_visits = N.visit_counts(rowptr, col, V, L, sets)
    assert counts.num_subgraphs == len(sets) == EPOCHS * P.batches_per_epoch(sampler, graph, per_batch)
    assert counts.node_visits.dtype == counts.edge_visits.dtype == torch.int32
    assert np.array_equal(counts.node_visits.cpu().numpy(), node_visits) and np.array_equal(counts.edge_visits.cpu().numpy(), edge_visits)
    assert not device_sampler.stamp.any()
    # the batches of epoch 0: batch j is drawn with draw = j
    lists = epoch_node_lists(plan, 0)
    want_lists = P.epoch_lists(sampler, graph, per_batch, SEED, 0)
    assert len(lists) == len(want_lists) == P.batches_per_epoch(sampler, graph, per_batch)
    hub_entries = 0
    for j, (ids, want_ids) in enumerate(zip(lists, want_lists)):
        what = (sampler, per_batch, L, j)
        nodes = P.node_set(sampler, graph, want_ids, j, SEED, 0, WALK)
        want = S.induced(rowptr, col, V, L, nodes)
        weighted = device_sampler.sample(ids, j, (counts, CAP)) if plan.walked else device_sampler.sample_nodes(ids, (counts, CAP))
        check_against_reference(weighted, want, what)
        assert not device_sampler.stamp.any(), what
        want_weights = N.edge_weights(rowptr, col, V, L, nodes, node_visits, edge_visits, CAP)
        got = weighted.message_weights
        assert got.dtype == torch.float32 and tuple(got.shape) == (weighted.num_edges,) == want_weights.shape, what
        assert np.array_equal(_bits(got), want_weights.view(np.uint32)), what
        plain = device_sampler.sample(ids, j) if plan.walked else device_sampler.sample_nodes(ids)
        check_against_reference(plain, want, what)
        assert plain.message_weights is None and not device_sampler.stamp.any(), what
        hub_entries = max(hub_entries, int(want.degrees[0][np.searchsorted(nodes, P.HUB)]) if P.HUB in nodes else 0)
    if sampler == "node":                                         # a degree-proportional draw meets the hub, and keeps a long bucket of it
        assert hub_entries > 64, hub_entries
    if sampler == "parts":
        assert hub_entries > 64 * per_batch // 5, hub_entries


def test_a_bad_node_list_is_a_value_error_and_the_stamps_stay_zero(gpu_device, tmp_path, monkeypatch):
    graph = P.sampler_graph(3)
    device_sampler, _ = _sampler_and_plan(graph, gpu_device, "node", 16, tmp_path)
    good = np.array([3, 4, 250], np.int32)
    for bad, message in ((np.array([3, V], np.int32), "node outside"), (np.array([-1, 3], np.int32), "node outside"),
                         (np.array([3, 4, 3], np.int32), "names a node twice"), (np.zeros(0, np.int32), "list is empty"),
                         (np.array([3, 4], np.int64), "int32")):
        with pytest.raises(ValueError, match=message):
            device_sampler.sample_nodes(bad)
        assert not device_sampler.stamp.any()
    # a call that fails behind the stamping: the guard zeroes what it stamped
    monkeypatch.setattr(device_sampler, "_node_list", lambda *a: (_ for _ in ()).throw(RuntimeError("behind the stamps")))
    with pytest.raises(RuntimeError, match="behind the stamps"):
        device_sampler.sample_nodes(good)
    assert not device_sampler.stamp.any()
    monkeypatch.undo()
    sub = device_sampler.sample_nodes(torch.as_tensor(good[::-1].copy(), device=gpu_device))         # any order, from the device too
    assert sub.nodes.cpu().tolist() == good.tolist() and not device_sampler.stamp.any()


# ---- 2. the task ----------------------------------------------------------------------------------------------------------------------
def _graph_task(L, value, train_mask=None, **params):
    """The citation task over P.sampler_graph(L) (V = 300): load_synthetic's features and labels, the reference graph's edges and fold."""
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    graph = P.sampler_graph(L)
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), out_layer_dropout_keep_prob=1.0, subgraph_batches=value, **params))
    task.load_synthetic(num_nodes=V, num_features=24, num_classes=5, num_train=100, num_valid=80, num_test=80, feature_density=0.2, seed=3)
    adjacency = [np.ascontiguousarray(a) for a in graph.adjacency]
    degrees = np.stack([np.bincount(a[:, 1], minlength=V) for a in adjacency]).astype(np.int32)
    for folds in (task._loaded_data[DataFold.TRAIN], task._loaded_data[DataFold.VALIDATION], task.synthetic_test_data):
        folds[0] = folds[0]._replace(adjacency_lists=adjacency, type_to_node_to_num_incoming_edges=degrees)
    train = task._loaded_data[DataFold.TRAIN]
    train[0] = train[0]._replace(mask=np.ascontiguousarray(graph.mask if train_mask is None else train_mask, dtype=np.float32))
    task._Citation_Network_Task__num_edge_types = L
    return task


def _rgcn(task, device, result_dir=None, run_id="samplers", **params):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(dict(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=6), **params)
    if result_dir is None:
        return RGCN_Model(p, task, device=str(device))
    return RGCN_Model(p, task, run_id=run_id, result_dir=str(result_dir), device=str(device))


@pytest.mark.parametrize("normalised", [False, True], ids=["plain", "normalised"])
def test_the_walk_sampler_named_is_the_batch_without_the_key(gpu_device, normalised):
    from tf_gnn_samples_amd.tasks import DataFold
    from test_gpu_single_graph_dp import _assert_same_batch
    absent = {"roots_per_batch": 16, "walk_length": WALK, "seed": SEED}
    if normalised:
        absent["normalisation"] = dict(NORM)
    tasks = [_graph_task(3, absent), _graph_task(3, dict(absent, sampler="walk"))]
    assert "sampler" not in tasks[0].subgraph_batches and tasks[1].subgraph_batches["sampler"] == "walk"
    for task in tasks:
        task.bind_sampling_device(gpu_device)
    for epoch in range(2):
        without, named = (list(task.batches.train_batches(task._loaded_data[DataFold.TRAIN][0])) for task in tasks)
        assert len(without) == len(named) == 7                    # ceil(100 / 16)
        for j, (a, b) in enumerate(zip(named, without)):
            _assert_same_batch(a, b, "epoch %d, batch %d" % (epoch, j))
            assert ("loss_normalisation" in a.extra) == normalised
    assert all((task.batches.epoch, task.batches.draw) == (2, 14) for task in tasks)


def test_a_node_batch_without_a_train_node_has_loss_zero_and_zero_gradients(gpu_device):
    """The TRAIN fold is the isolated node alone: a node batch draws targets of by-target entries and never holds it."""
    from tf_gnn_samples_amd.tasks import DataFold
    from test_gpu_subgraph_batches import _metrics_and_gradients
    only = np.zeros(V, np.float32)
    only[P.ISOLATED] = 1.0
    task = _graph_task(3, _value("node", 16), train_mask=only)
    model = _rgcn(task, gpu_device)
    train = task._loaded_data[DataFold.TRAIN]
    (batch,) = list(model._batches(train, DataFold.TRAIN))        # ceil(1 / 16) batches an epoch
    assert P.ISOLATED not in batch.extra["sampled_nodes"].cpu().tolist() and float(batch.extra["mask"].sum()) == 0.0
    weights, denominator = batch.extra["loss_normalisation"]
    assert denominator == 1.0 and bool(torch.isfinite(weights).all())
    metrics, grads = _metrics_and_gradients(model, batch)
    assert metrics["loss"] == 0.0 and metrics["total_loss"] == 0.0 and metrics["num_masked"] == 0.0 and metrics["num_correct"] == 0.0
    held = [g for g in grads.values() if g is not None]
    assert held and all(np.isfinite(g).all() and not g.any() for g in held)
    # an epoch of such batches: a finite loss, a finite early-stopping metric, an accuracy that prints; the step changed nothing
    before = {n: model.variables[n].detach().clone() for n in model.variables.names()}
    loss, results, graphs, *_ = model._run_epoch("train", train, DataFold.TRAIN, quiet=True)
    assert len(results) == 1 and loss == 0.0 and np.isfinite(task.early_stopping_metric(results, graphs))
    assert task.pretty_print_epoch_task_metrics(results + results, graphs) == "Acc: 0.00%"
    assert all(bool(torch.isfinite(model.variables[n]).all()) and torch.equal(before[n], model.variables[n]) for n in before)


SYNTHETIC = dict(num_nodes=200, num_features=24, num_classes=4, num_train=60, num_valid=50, num_test=50, feature_density=0.2, seed=2)


def _synthetic_value(sampler, tmp_path, **more):
    """R = 16: ceil(60 / 16) = 4 batches an epoch; 12 parts, 3 a batch: 4 batches an epoch."""
    path = tmp_path / "parts200.npy"
    if sampler == "parts" and not path.exists():
        np.save(path, (np.random.default_rng(7).permutation(SYNTHETIC["num_nodes"]) % 12).astype(np.int32))
    return _value(sampler, 3 if sampler == "parts" else 16, path, **more)


def _train_two_epochs(device, result_dir, value):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), subgraph_batches=value))
    task.load_synthetic(**SYNTHETIC)
    result_dir.mkdir()
    model = _rgcn(task, device, result_dir, random_seed=3)
    record, run_epoch = [], model._run_epoch

    def recording(epoch_name, data, fold, quiet=False):
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, [np.float32(float(m["loss"])).tobytes() for m in out[1]]))
        return out
    model._run_epoch = recording
    try:
        model.train(quiet=True, max_epochs=2)
    finally:
        model._run_epoch = run_epoch
    torch.cuda.synchronize()
    with open(model.best_model_file, "rb") as f:
        saved = {k: np.asarray(v).tobytes() for k, v in pickle.load(f)["weights"].items()}
    return task, model, record, saved


@pytest.mark.parametrize("sampler", P.SAMPLERS)
def test_two_epochs_train_alike_twice_and_restore_continues_with_the_same_batches(gpu_device, tmp_path, sampler):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold
    from test_gpu_single_graph_dp import _assert_same_batch
    value = _synthetic_value(sampler, tmp_path)
    task, model, record, saved = _train_two_epochs(gpu_device, tmp_path / "a", value)
    assert [len(r[1]) for r in record] == [4, 1, 4, 1] and (task.batches.epoch, task.batches.draw) == (2, 8)
    losses = [np.frombuffer(b, np.float32)[0] for r in record for b in r[1]]
    assert np.isfinite(losses).all() and any(x > 0 for x in losses)
    (state,) = [s for s in task.batches.fold_states.values() if s.visit_counts is not None]
    assert state.visit_counts.num_subgraphs == EPOCHS * 4
    _, _, again_record, again_saved = _train_two_epochs(gpu_device, tmp_path / "b", value)
    assert again_record == record and again_saved == saved        # the same losses and the same checkpoint, bit for bit
    # restore(): the key (and the partition's path) comes back; from the counters of the run the next epoch's batches are the run's
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.subgraph_batches == task.subgraph_batches and restored.task.subgraph_batches["sampler"] == sampler
    restored.task.load_synthetic(**SYNTHETIC)
    restored.task.bind_sampling_device(gpu_device)
    restored.task.batches.epoch, restored.task.batches.draw = task.batches.epoch, task.batches.draw
    want = list(task.batches.train_batches(task._loaded_data[DataFold.TRAIN][0]))
    got = list(restored.task.batches.train_batches(restored.task._loaded_data[DataFold.TRAIN][0]))
    assert len(got) == len(want) == 4
    for j, (a, b) in enumerate(zip(got, want)):
        assert len(a.adjacency_lists) == 2 and all(torch.equal(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists))
        assert torch.equal(a.extra["sampled_nodes"], b.extra["sampled_nodes"]) and torch.equal(a.extra["mask"], b.extra["mask"]), j
        assert np.array_equal(_bits(a.extra["loss_normalisation"][0]), _bits(b.extra["loss_normalisation"][0])), j
        assert np.array_equal(_bits(a.graph.degree_scale(a.type_to_num_incoming_edges)), _bits(b.graph.degree_scale(b.type_to_num_incoming_edges))), j
    loss, results, *_ = restored._run_epoch("train", restored.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, quiet=True)
    assert len(results) == 4 and np.isfinite(loss)


@pytest.mark.parametrize("sampler", ["node", "edge", "parts"])
def test_one_step_over_sparse_features_is_finite_and_the_same_twice(gpu_device, tmp_path, sampler):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    value = _synthetic_value(sampler, tmp_path, sparse_features=True)
    steps = []
    for _ in range(2):
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), subgraph_batches=value, sparse_node_features=True))
        task.load_synthetic(**SYNTHETIC)
        model = _rgcn(task, gpu_device)
        batch = next(iter(model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)))
        assert isinstance(batch.extra["sparse_node_features"], SparseRows) and tuple(batch.initial_node_features.shape) == (batch.num_nodes, 1)
        metrics = model.train_step(batch)
        torch.cuda.synchronize()
        steps.append((np.float32(float(metrics["loss"].detach())), {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}))
    (loss_a, vars_a), (loss_b, vars_b) = steps
    assert np.isfinite(loss_a) and loss_a.tobytes() == loss_b.tobytes()
    assert all(np.isfinite(vars_a[n]).all() and np.array_equal(vars_a[n].view(np.uint32), vars_b[n].view(np.uint32)) for n in vars_a)


# ---- 3. two ranks on one card over gloo -----------------------------------------------------------------------------------------------
def _run_two_ranks(kind, num_train, tmp_path, refusals=False):
    """tests/test_gpu_single_graph_dp.py's, with the worker that knows this file's cases."""
    import test_gpu_single_graph_dp as T
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = T._free_port()
    procs = [ctx.Process(target=D.worker, args=(r, 2, port, q, kind, num_train, str(tmp_path), refusals)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=240) for _ in range(2)), key=lambda d: d["rank"])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return results


@pytest.mark.timeout(300)
@pytest.mark.parametrize("sampler", ["node", "edge", "parts"])
def test_two_ranks_equal_a_one_process_replay(gpu_device, tmp_path, monkeypatch, sampler):
    """Two epochs of train(group=WORLD) and a test(group=WORLD) on the sampler's batches, four an epoch, dealt out in turn; replayed by
    this process alone: the bits of every reduced gradient, variable, optimizer slot and reported loss."""
    import test_gpu_single_graph_dp as T
    D.write_parts(tmp_path)
    D.register(tmp_path)
    monkeypatch.setattr(T, "_run_two_ranks", _run_two_ranks)
    try:
        results = T._check_two_ranks(sampler, D.NUM_TRAIN, gpu_device, tmp_path, batches=D.BATCHES[sampler], evaluation_batches=1)
    finally:
        for kind in D.BATCHES:
            T.C.TASK_PARAMS.pop(kind, None)
    assert all(r["counters"] == (2, 2 * D.BATCHES[sampler]) for r in results)
