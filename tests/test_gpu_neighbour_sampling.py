"""Neighbour sampling on the GPU (csrc/neighbour_sample.hip, tasks/neighbour_sampling.py): the kernels against
tests/neighbour_sampling_reference.py bit for bit, the stamp array and streams, the full graph as a sample of itself, a sampled batch
against the same batch fed through the NumPy path, and train() on sampled batches."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import neighbour_sampling_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

V = 300
# (target, type 0) buckets of these lengths at targets 0, 1, 2, ...: empty, one entry, k and k + 1 for k = 2, 3, 4, the wave width and
# its neighbours, more than two waves, and a hub far longer than a wave
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 5000]
HUB = LENGTHS.index(5000)
_GRAPHS = {}


def graph(L):
    """adjacency lists (host), the reference's bucketing of them, and the RelGraph on the device; built once per L."""
    if L not in _GRAPHS:
        rng = np.random.default_rng(L)
        adjacency = []
        for l in range(L):
            lengths = rng.integers(0, 9, size=V)
            if l == 0:
                lengths[:len(LENGTHS)] = LENGTHS
            tgt = np.repeat(np.arange(V), lengths)
            src = rng.integers(0, V, size=len(tgt))                   # (5000 draws from 300 nodes: duplicate edges throughout)
            src[tgt == 20] = 21                                       # one bucket of one edge repeated
            e = np.stack([src, tgt], axis=1)[rng.permutation(len(tgt))]
            adjacency.append(np.ascontiguousarray(e, dtype=np.int32))
        _GRAPHS[L] = (adjacency, R.bucketing(adjacency, V))
    return _GRAPHS[L]


def device_graph(L, device):
    from tf_gnn_samples_amd.graph import RelGraph
    adjacency, (rowptr, col, _) = graph(L)
    g = RelGraph([torch.as_tensor(a, device=device) for a in adjacency], V)
    assert np.array_equal(g.rowptr_t.cpu().numpy(), rowptr) and np.array_equal(g.col_t.cpu().numpy(), col)
    return g


def seed_lists(L):
    adjacency, (rowptr, col, _) = graph(L)
    neighbour = int(col[rowptr[7 * L]] // L)                          # a source of target 7: a seed that is another seed's neighbour
    mixed = np.unique(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, HUB, 20, 150, 299, neighbour]))
    return {"mixed": mixed.astype(np.int32), "single": np.array([HUB], np.int32), "all": np.arange(V, dtype=np.int32)}


def check_against_reference(sub, want, what):
    assert sub.num_nodes == len(want.nodes) and sub.num_edges == sum(len(a) for a in want.adjacency_lists), what
    assert sub.nodes.dtype == torch.int32 and np.array_equal(sub.nodes.cpu().numpy(), want.nodes), what
    assert len(sub.adjacency_lists) == len(want.adjacency_lists)
    for l, (got, ref) in enumerate(zip(sub.adjacency_lists, want.adjacency_lists)):
        assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape and np.array_equal(got.cpu().numpy(), ref), (what, l)
    got = sub.type_to_num_incoming_edges
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.degrees.view(np.uint32)), what
    assert np.array_equal(sub.seed_mask.cpu().numpy().view(np.uint32), want.seed_mask.view(np.uint32)), what


@pytest.mark.parametrize("fanouts", [[3], [3, 2], [0, 4]])
@pytest.mark.parametrize("L", [2, 3])
def test_kernels_reproduce_the_reference_bit_for_bit(gpu_device, L, fanouts):
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.neighbour_sampling import MAX_FANOUT, MAX_HOPS, NeighbourSampler
    lib = _lib.load_library()
    assert (lib.relgnn_neighbour_sample_max_fanout(), lib.relgnn_neighbour_sample_max_hops()) == (MAX_FANOUT, MAX_HOPS)
    _, (rowptr, col, _) = graph(L)
    sampler = NeighbourSampler(device_graph(L, gpu_device), fanouts, seed=11, replica=2)
    assert sampler.synced_hops == [h for h, k in enumerate(fanouts) if k == 0]
    for name, seeds in seed_lists(L).items():
        for draw in (0, 7):
            want = R.sample(rowptr, col, V, L, seeds, fanouts, draw, seed=11, replica=2)
            sub = sampler.sample(torch.as_tensor(seeds, device=gpu_device), draw)
            check_against_reference(sub, want, (L, fanouts, name, draw))
            assert not sampler.stamp.any()                            # all zero after every call
    # a host array in any order is the same seed list
    seeds = seed_lists(L)["mixed"]
    check_against_reference(sampler.sample(seeds[::-1].copy(), 7), R.sample(rowptr, col, V, L, seeds, fanouts, 7, seed=11, replica=2), "host seeds")
    for bad in (np.array([1, 1], np.int32), np.array([-1], np.int32), np.array([V], np.int32), np.zeros(0, np.int32), np.array([1], np.int64)):
        with pytest.raises(ValueError):
            sampler.sample(bad, 0)
    assert not sampler.stamp.any()


def test_state_and_streams(gpu_device):
    """The same call twice, then another seed list, on one sampler: the stamps are clean in between.  The same bits on a stream
    that is not the default one."""
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    L, fanouts = 2, [3, 2]
    _, (rowptr, col, _) = graph(L)
    sampler = NeighbourSampler(device_graph(L, gpu_device), fanouts, seed=5)
    lists = seed_lists(L)
    want = {name: R.sample(rowptr, col, V, L, seeds, fanouts, 3, seed=5) for name, seeds in lists.items()}
    for name in ("mixed", "mixed", "single", "all", "mixed"):
        check_against_reference(sampler.sample(torch.as_tensor(lists[name], device=gpu_device), 3), want[name], name)
        assert not sampler.stamp.any()
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        for name in ("mixed", "all"):
            sub = sampler.sample(torch.as_tensor(lists[name], device=gpu_device), 3)
            side.synchronize()
            check_against_reference(sub, want[name], name + " on a side stream")
            assert not sampler.stamp.any()
    torch.cuda.current_stream(gpu_device).wait_stream(side)


def test_unsupported_shapes_are_value_errors(gpu_device):
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    g = device_graph(2, gpu_device)
    for fanouts in ([65], [], [1] * 9, [-1]):
        with pytest.raises(ValueError):
            NeighbourSampler(g, fanouts)


def _citation_task(num_nodes=600, **params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
    task.load_synthetic(num_nodes=num_nodes, num_features=48, num_classes=5, num_train=140, num_valid=150, num_test=150, feature_density=0.1, seed=3)
    return task


def _model(name, task, device, **params):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=6, **params)
    return cls(p, task, device=str(device))


def _loss_and_gradients(model, batch):
    from tf_gnn_samples_amd import ops
    for p in model.variables.parameters():
        p.grad = None
    metrics = model.forward_batch(batch, training=False)
    metrics["loss"].backward()
    ops.join_deferred()
    torch.cuda.synchronize()
    grads = {n: (None if model.variables[n].grad is None else model.variables[n].grad.cpu().numpy().copy()) for n in model.variables.names()}
    loss = float(metrics["loss"].detach())
    return loss, np.float32(loss), grads


def _fold_tables(fold, device):
    return (torch.as_tensor(fold.node_features, device=device), torch.as_tensor(fold.labels, device=device),
            torch.as_tensor(fold.mask, device=device))


def test_the_full_graph_is_a_sample_of_itself(gpu_device):
    """All nodes as seeds, fanouts [0]: nodes = arange(V), the graph's degree table, every bucket's edges in the graph's order; one RGCN
    step on it gives the full-graph batch's loss (1e-5) and every variable's gradient at the bars tests/test_gpu_citation.py holds the
    models to (2e-5 of the gradient's largest entry element-wise, 2e-5 in the Frobenius norm)."""
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    task = _citation_task()
    fold = task._loaded_data[DataFold.TRAIN][0]
    n = len(fold.labels)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in fold.adjacency_lists], n)
    sub = NeighbourSampler(g, [0]).sample(torch.arange(n, dtype=torch.int32, device=gpu_device), 0)
    assert np.array_equal(sub.nodes.cpu().numpy(), np.arange(n)) and sub.seed_mask.cpu().numpy().all()
    assert np.array_equal(sub.type_to_num_incoming_edges.cpu().numpy(), fold.type_to_node_to_num_incoming_edges.astype(np.float32))
    for got, full in zip(sub.adjacency_lists, fold.adjacency_lists):
        assert np.array_equal(got.cpu().numpy(), full[np.argsort(full[:, 1], kind="stable")])       # per-bucket order preserved
    model = _model("RGCN_Model", task, gpu_device)
    (mb,) = task.make_minibatch_iterator([fold], DataFold.TRAIN, 10 ** 6)
    want_loss, _, want = _loss_and_gradients(model, DeviceBatch(mb, gpu_device))
    got_loss, _, got = _loss_and_gradients(model, sub.device_batch(*_fold_tables(fold, gpu_device), 1.0))
    print("loss: full graph %.9g, as a sample %.9g" % (want_loss, got_loss))
    assert abs(got_loss - want_loss) <= 1e-5
    identical = got_loss == want_loss
    for name in want:
        a, b = want[name].astype(np.float64), got[name].astype(np.float64)
        scale = max(1e-6, float(np.abs(a).max()))
        err, fro = float(np.abs(a - b).max()), float(np.linalg.norm(a - b) / max(1e-12, np.linalg.norm(a)))
        same = np.array_equal(want[name].view(np.uint32), got[name].view(np.uint32))
        identical = identical and same
        print("%s: err / scale %.3g  fro %.3g  identical bits: %s" % (name, err / scale, fro, same))
        assert err <= 2e-5 * scale and fro <= 2e-5, (name, err, scale, fro)
    print("full graph as a sample: bit-identical step: %s" % identical)


@pytest.mark.parametrize("model_name", ["RGCN_Model", "GGNN_Model"])
def test_sampled_batch_equals_the_numpy_path(gpu_device, model_name):
    """device_batch() against the reference's subgraph fed through DeviceBatch(MinibatchData): the same loss and gradients bit for
    bit, with mean aggregation (RGCN also divides by the sampled in-degree table)."""
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, MinibatchData
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler, epoch_seed_batches
    task = _citation_task()
    fold = task._loaded_data[DataFold.TRAIN][0]
    n, L = len(fold.labels), len(fold.adjacency_lists)
    seeds = epoch_seed_batches(fold.mask, 32, 0, 0)[0]
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in fold.adjacency_lists], n)
    sub = NeighbourSampler(g, [3, 2], seed=9).sample(seeds, 4)
    rowptr, col, _ = R.bucketing(fold.adjacency_lists, n)
    want = R.sample(rowptr, col, n, L, seeds, [3, 2], 4, seed=9)
    check_against_reference(sub, want, model_name)
    assert 32 < sub.num_nodes < n and (want.degrees.max(axis=1) == [1, 3]).all()
    model = _model(model_name, task, gpu_device, message_aggregation_function="mean")
    device_side = sub.device_batch(*_fold_tables(fold, gpu_device), 1.0)
    assert device_side.num_graphs == 1 and torch.equal(device_side.extra["sampled_nodes"], sub.nodes)
    assert float(device_side.extra["mask"].sum()) == 32.0
    nodes = want.nodes
    feed = {"initial_node_features": fold.node_features[nodes], "adjacency_lists": want.adjacency_lists,
            "type_to_num_incoming_edges": want.degrees, "num_graphs": 1, "labels": fold.labels[nodes],
            "mask": want.seed_mask * fold.mask[nodes], "out_layer_dropout_keep_prob": 1.0}
    host_side = DeviceBatch(MinibatchData(feed, 1, len(nodes), sum(len(a) for a in want.adjacency_lists)), gpu_device)
    _, loss_a, grads_a = _loss_and_gradients(model, device_side)
    _, loss_b, grads_b = _loss_and_gradients(model, host_side)
    assert np.isfinite(loss_a) and loss_a.view(np.uint32) == loss_b.view(np.uint32)
    for name in grads_a:
        assert grads_a[name] is not None and np.abs(grads_a[name]).max() > 0, name
        assert np.array_equal(grads_a[name].view(np.uint32), grads_b[name].view(np.uint32)), name


def _train_two_epochs(device, result_dir, params, **model_params):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
    task.load_synthetic(seed=2)                                       # synthetic Cora: 2708 nodes, 140 of them in the train fold
    p = RGCN_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3, **model_params)
    result_dir.mkdir()
    model = RGCN_Model(p, task, run_id="sampled", result_dir=str(result_dir), device=str(device))
    record, run_epoch = [], model._run_epoch

    def recording(epoch_name, data, fold, quiet=False):
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, len(out[1]), out[2], [m.get("num_masked") for m in out[1]]))
        return out
    model._run_epoch = recording
    model.train(quiet=True, max_epochs=2)
    model._run_epoch = run_epoch
    torch.cuda.synchronize()
    return task, model, record, {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}


def test_train_on_sampled_batches(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    sampled = {"sampled_batches": {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1}}
    task, model, record, first = _train_two_epochs(gpu_device, tmp_path / "a", sampled)
    # 5 steps per training epoch (140 seeds: four batches of 32 and one of 12), one full-graph validation pass
    assert [(r[1], r[2]) for r in record] == [(5, 5), (1, 1), (5, 5), (1, 1)], record
    assert record[0][3] == [32.0, 32.0, 32.0, 32.0, 12.0] and record[1][3] == [None]
    assert (task.batches.epoch, task.batches.draw) == (2, 10)
    log = open(model.log_file).read()
    assert log.count(" Train: loss:") == 2 and log.count(" Valid: loss:") == 2 and "Acc:" in log
    for pipeline in ({}, {"native_batching": False}):                 # either iterator, and again: identical weights
        _, _, again_record, again = _train_two_epochs(gpu_device, tmp_path / ("b%d" % len(pipeline)), sampled, **pipeline)
        assert again_record == record
        for n in first:
            assert np.array_equal(first[n].view(np.uint32), again[n].view(np.uint32)), n
    # without the parameter, and with None: the single-batch loop, step for step
    _, _, absent_record, absent = _train_two_epochs(gpu_device, tmp_path / "c", {})
    plain_task, plain_model, none_record, none = _train_two_epochs(gpu_device, tmp_path / "d", {"sampled_batches": None})
    assert absent_record == none_record and [(r[1], r[2]) for r in none_record] == [(1, 1)] * 4
    from tf_gnn_samples_amd.models import RGCN_Model
    p = dict(plain_model.params)
    by_hand = RGCN_Model(p, plain_task, run_id="by_hand", result_dir=str(tmp_path / "d"), device=str(gpu_device))
    for _ in range(2):
        (mb,) = plain_task.make_minibatch_iterator(plain_task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, p["max_nodes_in_batch"])
        by_hand.train_step(DeviceBatch(mb, gpu_device))
    torch.cuda.synchronize()
    for n in none:
        assert np.array_equal(absent[n].view(np.uint32), none[n].view(np.uint32)), n
        assert np.array_equal(none[n], by_hand.variables[n].detach().cpu().numpy()), n
        assert not np.array_equal(none[n], first[n]), n               # the sampled run did train on something else
    # the native iterator, asked directly, yields the same kind of epoch (the model routes both settings to one generator)
    train = task._loaded_data[DataFold.TRAIN]
    native = list(task.make_native_minibatch_iterator(model._native_pipeline(train), DataFold.TRAIN, 10 ** 6))
    numpy_side = list(task.make_minibatch_iterator(train, DataFold.TRAIN, 10 ** 6))
    for batches in (native, numpy_side):
        assert len(batches) == 5 and all(isinstance(b, DeviceBatch) and "sampled_nodes" in b.extra for b in batches)
        assert [float(b.extra["mask"].sum()) for b in batches] == [32.0, 32.0, 32.0, 32.0, 12.0]
    assert (task.batches.epoch, task.batches.draw) == (4, 20)
    # restore() of the sampled run's best model: the parameter comes back, predict() is the full graph
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.sampled_batches == sampled["sampled_batches"]
    (prediction,) = restored.predict(task.synthetic_test_data)
    assert prediction["classes"].shape == (2708,) and prediction["probabilities"].shape == (2708, 7)
    # a sampled batch cannot be captured
    restored.task.bind_sampling_device(gpu_device)
    batch = next(iter(restored.task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, 0)))
    assert isinstance(batch, DeviceBatch) and "sampled_nodes" in batch.extra
    with pytest.raises(RuntimeError, match="sampled batch"):
        restored.capture_train_step(batch)
