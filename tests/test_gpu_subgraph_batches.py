"""Random-walk subgraph batches on the GPU (csrc/subgraph_sample.hip, tasks/subgraph_sampling.py, the citation task's
`subgraph_batches`): the walks and the induced subgraph against tests/subgraph_reference.py bit for bit, the stamp array and streams,
one read-back per call, a training step on a subgraph batch against the same subgraph fed through the NumPy path, train() on
subgraph batches, and the peak memory of a deep model's step."""
import math
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import sparse_subset_reference as SS  # noqa: E402
import subgraph_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

V = 300
DEAD_ENDS = [290, 291, 292]            # no in-edge of any type
LOOP_ONLY = [293, 294]                 # the only in-edge is a self loop
EVERYONES = 299                        # (L = 3) an in-neighbour of every other node
# (target, type 0) buckets of these lengths at targets 0, 1, 2, ...: empty, one entry, the wave width and its neighbours, two waves,
# and a hub far longer than a wave
LENGTHS = [0, 1, 63, 64, 65, 128, 5000]
HUB = LENGTHS.index(5000)
OUTSIDE = np.arange(200, 264)          # the 64 sources of target 3's bucket, in this order: a set without them keeps none of it
_GRAPHS = {}
MODELS = ["RGCN_Model", "GGNN_Model", "RGAT_Model", "GNN_FiLM_Model"]


def walk_graph(L):
    """V = 300.  Random buckets of 0 .. 8 entries per (target, type), duplicates included; DEAD_ENDS have no in-edge, LOOP_ONLY only
    their self loop (type 0); with L = 3, type 2 holds the edge EVERYONES -> v for every other v that may have an in-edge."""
    if ("walk", L) not in _GRAPHS:
        rng = np.random.default_rng(L)
        special = np.array(DEAD_ENDS + LOOP_ONLY)
        adjacency = []
        for l in range(L):
            if l == 2:
                tgt = np.setdiff1d(np.arange(V), np.append(special, EVERYONES))
                e = np.stack([np.full(len(tgt), EVERYONES), tgt], axis=1)
            else:
                lengths = rng.integers(0, 9, size=V)
                lengths[special] = 0
                tgt = np.repeat(np.arange(V), lengths)
                e = np.stack([rng.integers(0, V, size=len(tgt)), tgt], axis=1)
                if l == 0:
                    e = np.concatenate([e, np.stack([LOOP_ONLY, LOOP_ONLY], axis=1)])
            adjacency.append(np.ascontiguousarray(e[rng.permutation(len(e))], dtype=np.int32))
        _GRAPHS[("walk", L)] = (adjacency, S.bucketing(adjacency, V))
    return _GRAPHS[("walk", L)]


def bucket_graph():
    """V = 300, L = 3.  Type 0: buckets of LENGTHS entries at targets 0 .. 6, 0 .. 8 entries elsewhere, random sources (5 000 draws
    from 300 nodes: a node set keeps a mixed part of every 64-entry pass); target 3's 64 sources are OUTSIDE, one each; the edge
    290 -> 291.  Type 1: random, and nodes 290 .. 294 are never a source of it.  Type 2: no edge at all."""
    if "bucket" not in _GRAPHS:
        rng = np.random.default_rng(17)
        lengths = rng.integers(0, 9, size=V)
        lengths[:len(LENGTHS)] = LENGTHS
        lengths[290:295] = 0
        tgt = np.repeat(np.arange(V), lengths)
        src = rng.integers(0, V, size=len(tgt))
        src[tgt == 3] = OUTSIDE
        e0 = np.concatenate([np.stack([src, tgt], axis=1), [[290, 291]]])
        e0 = e0[rng.permutation(len(e0))]
        e0 = np.concatenate([e0[e0[:, 1] != 3], np.stack([OUTSIDE, np.full(64, 3)], axis=1)])     # target 3's entries in OUTSIDE's order
        e1 = np.stack([rng.integers(0, 290, size=900), rng.integers(0, V, size=900)], axis=1)
        adjacency = [np.ascontiguousarray(e0, dtype=np.int32), np.ascontiguousarray(e1, dtype=np.int32), np.zeros((0, 2), np.int32)]
        _GRAPHS["bucket"] = (adjacency, S.bucketing(adjacency, V))
    return _GRAPHS["bucket"]


def device_graph(which, device):
    from tf_gnn_samples_amd.graph import RelGraph
    adjacency, (rowptr, col, _) = which
    g = RelGraph([torch.as_tensor(a, device=device) for a in adjacency], V)
    assert np.array_equal(g.rowptr_t.cpu().numpy(), rowptr) and np.array_equal(g.col_t.cpu().numpy(), col)
    return g


def check_against_reference(sub, want, what):
    assert sub.num_nodes == len(want.nodes) and sub.num_edges == sum(len(a) for a in want.adjacency_lists), what
    assert sub.nodes.dtype == torch.int32 and np.array_equal(sub.nodes.cpu().numpy(), want.nodes), what
    assert len(sub.adjacency_lists) == len(want.adjacency_lists)
    for l, (got, ref) in enumerate(zip(sub.adjacency_lists, want.adjacency_lists)):
        assert got.dtype == torch.int32 and got.is_contiguous() and tuple(got.shape) == ref.shape, (what, l)
        assert np.array_equal(got.cpu().numpy(), ref), (what, l)
    got = sub.type_to_num_incoming_edges
    assert got.dtype == torch.float32 and tuple(got.shape) == want.degrees.shape, what
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.degrees.view(np.uint32)), what
    assert np.array_equal(sub.seed_mask.cpu().numpy().view(np.uint32), want.seed_mask.view(np.uint32)), what


def root_list(R):
    """R distinct roots that hold the special nodes first (as far as R allows), ascending."""
    first = [EVERYONES, DEAD_ENDS[0], LOOP_ONLY[0], 0, LOOP_ONLY[1], DEAD_ENDS[1], 7]
    rest = [v for v in np.random.default_rng(R).permutation(V).tolist() if v not in first]
    return np.sort(np.array((first + rest)[:R], np.int32))


# ---- 1. walks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0, 1, 3, 8, 64])
@pytest.mark.parametrize("L", [2, 3])
def test_walks_visit_the_reference_s_node_sets(gpu_device, L, h):
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.subgraph_sampling import MAX_WALK_LENGTH, SubgraphSampler
    assert _lib.load_library().relgnn_subgraph_max_walk_length() == MAX_WALK_LENGTH
    which = walk_graph(L)
    _, (rowptr, col, _) = which
    sampler = SubgraphSampler(device_graph(which, gpu_device), h, seed=11, replica=2)
    for R in (1, 7, 64, 65):
        roots = root_list(R)
        for draw in (0, 7):
            want = S.sample(rowptr, col, V, L, roots, h, draw, seed=11, replica=2)
            sub = sampler.sample(torch.as_tensor(roots, device=gpu_device), draw)
            check_against_reference(sub, want, (L, h, R, draw))
            assert set(roots.tolist()) <= set(want.nodes.tolist()) and len(want.nodes) <= min(V, R * (h + 1))
            assert not sampler.stamp.any()                            # all zero after every call
    # the walks of dead ends and of nodes whose only in-edge is their self loop stay where they are
    stay = np.array(sorted(DEAD_ENDS + LOOP_ONLY), np.int32)
    assert np.array_equal(sampler.sample(stay, 3).nodes.cpu().numpy(), stay)
    if L == 3 and h >= 1:                                             # EVERYONES is not a root here: the walks find it
        others = np.arange(100, 164, dtype=np.int32)
        assert EVERYONES in sampler.sample(others, 0).nodes.cpu().numpy().tolist()


def test_walks_are_the_same_on_any_stream_and_run_and_differ_by_draw_seed_and_replica(gpu_device):
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler
    L, h = 2, 3
    which = walk_graph(L)
    _, (rowptr, col, _) = which
    g = device_graph(which, gpu_device)
    roots = root_list(64)
    sampler = SubgraphSampler(g, h, seed=5)
    want = S.sample(rowptr, col, V, L, roots, h, 3, seed=5)
    for _ in range(2):
        check_against_reference(sampler.sample(torch.as_tensor(roots, device=gpu_device), 3), want, "again")
    check_against_reference(sampler.sample(roots[::-1].copy(), 3), want, "a host array in any order")
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        sub = sampler.sample(torch.as_tensor(roots, device=gpu_device), 3)
        side.synchronize()
        check_against_reference(sub, want, "on a side stream")
        assert not sampler.stamp.any()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    base = want.nodes
    for what, other, ref in (("draw", SubgraphSampler(g, h, seed=5).sample(roots, 4), S.sample(rowptr, col, V, L, roots, h, 4, seed=5)),
                             ("seed", SubgraphSampler(g, h, seed=6).sample(roots, 3), S.sample(rowptr, col, V, L, roots, h, 3, seed=6)),
                             ("replica", SubgraphSampler(g, h, seed=5, replica=1).sample(roots, 3),
                              S.sample(rowptr, col, V, L, roots, h, 3, seed=5, replica=1))):
        check_against_reference(other, ref, what)
        assert not np.array_equal(other.nodes.cpu().numpy(), base), what


def test_unsupported_shapes_and_bad_root_lists_are_value_errors(gpu_device):
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, induced_subgraph
    g = device_graph(walk_graph(2), gpu_device)
    for walk_length in (65, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            SubgraphSampler(g, walk_length)
    with pytest.raises(ValueError):
        SubgraphSampler(g, 2, replica=2 ** 31)
    sampler = SubgraphSampler(g, 2)
    for bad in (np.array([1, 1], np.int32), np.array([-1], np.int32), np.array([V], np.int32), np.zeros(0, np.int32), np.array([1], np.int64),
                np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError):
            sampler.sample(bad, 0)
        with pytest.raises(ValueError):
            induced_subgraph(g, bad)
    assert not sampler.stamp.any()
    # a call that raised half-way leaves the stamps clean too
    from tf_gnn_samples_amd import _lib
    launch = _lib.launch

    def failing(name, *args):
        if name == "relgnn_subgraph_induced_count":
            raise RuntimeError("stop here")
        launch(name, *args)
    _lib.launch = failing
    try:
        with pytest.raises(RuntimeError, match="stop here"):
            sampler.sample(root_list(7), 0)
    finally:
        _lib.launch = launch
    assert not sampler.stamp.any()
    assert sampler.sample(root_list(7), 0).num_nodes >= 7


# ---- 2. induced edges -----------------------------------------------------------------------------------------------------------------
def node_sets():
    rng = np.random.default_rng(3)
    head = np.arange(len(LENGTHS))
    half = np.union1d(head, rng.choice(V, size=V // 2, replace=False))
    return {
        "mixed": half,                                                                    # a part of every pass of the hub's bucket
        "none of a pass": np.setdiff1d(np.union1d(half, [3]), OUTSIDE),                   # target 3 keeps 0 of its 64 entries
        "all of a pass": np.union1d(head, OUTSIDE),                                       # ... and all 64 of them
        "type 1 keeps nothing": np.array([290, 291, 292]),                                # 290 -> 291 of type 0 is all there is
        "one node": np.array([HUB]),
        "all": np.arange(V),
    }


def test_induced_subgraphs_equal_the_reference_array_for_array(gpu_device):
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks.subgraph_sampling import induced_subgraph
    which = bucket_graph()
    adjacency, (rowptr, col, _) = which
    g = device_graph(which, gpu_device)
    lengths = np.diff(rowptr.astype(np.int64))[np.arange(len(LENGTHS)) * 3]
    assert lengths.tolist() == LENGTHS and len(adjacency[2]) == 0
    subs = {}
    for name, nodes in node_sets().items():
        want = S.induced(rowptr, col, V, 3, nodes)
        order = np.random.default_rng(5).permutation(len(nodes))
        subs[name] = sub = induced_subgraph(g, torch.as_tensor(nodes[order].astype(np.int32), device=gpu_device))
        check_against_reference(sub, want, name)
        assert len(want.adjacency_lists[2]) == 0
        print("%s: %d nodes, edges per type %s" % (name, len(want.nodes), [len(a) for a in want.adjacency_lists]))
    local = lambda name, v: int(np.searchsorted(node_sets()[name], v))
    assert float(subs["none of a pass"].type_to_num_incoming_edges[0, local("none of a pass", 3)]) == 0.0
    assert float(subs["all of a pass"].type_to_num_incoming_edges[0, local("all of a pass", 3)]) == 64.0
    hub_kept = float(subs["mixed"].type_to_num_incoming_edges[0, local("mixed", HUB)])
    assert 64 < hub_kept < 5000 - 64
    assert [int(a.shape[0]) for a in subs["type 1 keeps nothing"].adjacency_lists] == [1, 0, 0]
    assert subs["one node"].num_nodes == 1
    # all V nodes: every edge of the full graph, and a RelGraph built from the lists is the full graph's bucketing
    everything = subs["all"]
    assert everything.num_edges == sum(len(a) for a in adjacency)
    assert np.array_equal(everything.type_to_num_incoming_edges.cpu().numpy(),
                          np.stack([np.bincount(a[:, 1], minlength=V) for a in adjacency]).astype(np.float32))
    rebuilt = RelGraph(everything.adjacency_lists, V)
    assert torch.equal(rebuilt.rowptr_t, g.rowptr_t) and torch.equal(rebuilt.col_t, g.col_t)


@pytest.mark.parametrize("L", [2, 3])
def test_induced_subgraph_agrees_with_the_sampler_on_the_sampler_s_node_set(gpu_device, L):
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, induced_subgraph
    g = device_graph(walk_graph(L), gpu_device)
    sampler = SubgraphSampler(g, 3, seed=4)
    for R in (7, 65):
        sub = sampler.sample(root_list(R), 1)
        again = induced_subgraph(g, sub.nodes)
        assert again.num_nodes == sub.num_nodes and again.num_edges == sub.num_edges and torch.equal(again.nodes, sub.nodes)
        assert all(torch.equal(a, b) for a, b in zip(again.adjacency_lists, sub.adjacency_lists))
        assert torch.equal(again.type_to_num_incoming_edges, sub.type_to_num_incoming_edges) and torch.equal(again.seed_mask, sub.seed_mask)
        assert not sampler.stamp.any()
    # the hub graph through the sampler: h = 0 is the subgraph induced on the roots alone
    which = bucket_graph()
    _, (rowptr, col, _) = which
    roots = node_sets()["mixed"].astype(np.int32)
    hub_sampler = SubgraphSampler(device_graph(which, gpu_device), 0)
    check_against_reference(hub_sampler.sample(roots, 0), S.induced(rowptr, col, V, 3, roots), "h = 0 on the hub graph")
    assert not hub_sampler.stamp.any()


# ---- 3. one read-back per call --------------------------------------------------------------------------------------------------------
def test_a_call_reads_back_once(gpu_device, monkeypatch):
    """Every Tensor.tolist / .item / .cpu of a device tensor is counted while sample() and induced_subgraph() run on a host root list
    (nothing of the validation is then on the device): one per call, the [L + 2] sizes."""
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, induced_subgraph
    which = walk_graph(3)
    g = device_graph(which, gpu_device)
    sampler = SubgraphSampler(g, 8, seed=1)              # (the graph is checked here, once per graph: not part of a call)
    sampler.sample(root_list(7), 0)
    reads = []
    for name in ("tolist", "item", "cpu"):
        original = getattr(torch.Tensor, name)

        def counting(self, *args, _name=name, _original=original, **kwargs):
            if self.is_cuda:
                reads.append((_name, tuple(self.shape)))
            return _original(self, *args, **kwargs)
        monkeypatch.setattr(torch.Tensor, name, counting)
    sub = sampler.sample(root_list(65), 3)
    assert reads == [("tolist", (5,))], reads
    del reads[:]
    induced_subgraph(g, root_list(64))
    assert reads == [("tolist", (5,))], reads
    monkeypatch.undo()
    assert sub.num_nodes >= 65


# ---- 4. a training step on a subgraph batch -------------------------------------------------------------------------------------------
def _citation_task(sparse=False, num_nodes=600, **params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    if sparse:
        params["sparse_node_features"] = True
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
    task.load_synthetic(num_nodes=num_nodes, num_features=48, num_classes=5, num_train=140, num_valid=150, num_test=150, feature_density=0.1,
                        seed=3)
    return task


def _model(name, task, device, num_layers=2, **params):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(dict(dict(hidden_size=32, graph_num_layers=num_layers, graph_layer_input_dropout_keep_prob=1.0, random_seed=6,
                       graph_residual_connection_every_num_layers=2), **params))
    return cls(p, task, device=str(device))


def _metrics_and_gradients(model, batch):
    from tf_gnn_samples_amd import ops
    for p in model.variables.parameters():
        p.grad = None
    metrics = model.forward_batch(batch, training=False)
    metrics["loss"].backward()
    ops.join_deferred()
    torch.cuda.synchronize()
    grads = {n: (None if model.variables[n].grad is None else model.variables[n].grad.cpu().numpy().copy()) for n in model.variables.names()}
    values = {k: np.float32(float(metrics[k].detach())) for k in ("loss", "total_loss", "accuracy", "num_masked", "num_correct") if k in metrics}
    return values, grads


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("num_layers", [2, 8])
@pytest.mark.parametrize("model_name", MODELS)
def test_a_subgraph_batch_equals_the_numpy_path(gpu_device, model_name, num_layers, norm, sparse):
    """The task's first subgraph batch against the reference's subgraph fed through DeviceBatch(MinibatchData): the loss, the metrics
    and every variable's gradient bit for bit.  140 nodes at the most: far below the 4 096 rows at which a product changes route."""
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, MinibatchData
    from tf_gnn_samples_amd.tasks.neighbour_sampling import epoch_seed_batches
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, node_stand_in
    value = {"roots_per_batch": 32, "walk_length": 3, "seed": 9}
    if sparse:
        value["sparse_features"] = True
    task = _citation_task(sparse, subgraph_batches=value)
    train = task._loaded_data[DataFold.TRAIN]
    fold = train[0]
    n, L = len(fold.labels), len(fold.adjacency_lists)
    model = _model(model_name, task, gpu_device, num_layers, graph_inter_layer_norm=norm)
    device_side = next(iter(model._batches(train, DataFold.TRAIN)))
    roots = epoch_seed_batches(fold.mask, 32, 9, 0)[0]
    rowptr, col, _ = S.bucketing(fold.adjacency_lists, n)
    want = S.sample(rowptr, col, n, L, roots, 3, 0, seed=9)
    nodes = want.nodes
    assert isinstance(device_side, DeviceBatch) and device_side.num_graphs == 1 and 32 < len(nodes) <= 128 < 4096
    assert np.array_equal(device_side.extra["sampled_nodes"].cpu().numpy(), nodes)
    for got, ref in zip(device_side.adjacency_lists, want.adjacency_lists):
        assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(device_side.type_to_num_incoming_edges.cpu().numpy(), want.degrees)
    assert want.degrees[1].max() >= 1 and (want.degrees[0] == 1).all()                    # self loops stay, neighbours as far as induced
    mask = fold.mask[nodes]
    assert float(device_side.extra["mask"].sum()) == float(mask.sum()) >= 32.0            # every TRAIN node of the subgraph counts
    feed = {"adjacency_lists": want.adjacency_lists, "type_to_num_incoming_edges": want.degrees, "num_graphs": 1,
            "labels": fold.labels[nodes], "mask": want.seed_mask * mask, "out_layer_dropout_keep_prob": 1.0}
    if sparse:
        full = fold.node_features
        taken = SS.take_rows(*(a.numpy() for a in (full.rows.rowptr, full.rows.col, full.rows.val)), full.shape, nodes)
        assert tuple(device_side.initial_node_features.shape) == (len(nodes), 1)
        SS.compare(device_side.extra["sparse_node_features"], taken, "the batch's rows")
        feed["initial_node_features"] = node_stand_in(len(nodes))
        feed["sparse_node_features"] = SparseRows(taken.rows.rowptr, taken.rows.col, taken.rows.val, taken.shape)
    else:
        feed["initial_node_features"] = fold.node_features[nodes]
    host_side = DeviceBatch(MinibatchData(feed, 1, len(nodes), sum(len(a) for a in want.adjacency_lists)), gpu_device)
    host_side.extra["sampled_nodes"] = device_side.extra["sampled_nodes"]                 # (the counts of the epoch's accuracy too)
    metrics_a, grads_a = _metrics_and_gradients(model, device_side)
    metrics_b, grads_b = _metrics_and_gradients(model, host_side)
    assert sorted(metrics_a) == ["accuracy", "loss", "num_correct", "num_masked", "total_loss"] and np.isfinite(metrics_a["loss"])
    assert metrics_a["num_masked"] == float(mask.sum())
    for k in metrics_a:
        assert metrics_a[k].view(np.uint32) == metrics_b[k].view(np.uint32), k
    assert any(g is not None and np.abs(g).max() > 0 for g in grads_a.values())
    for name in grads_a:
        assert (grads_a[name] is None) == (grads_b[name] is None), name
        if grads_a[name] is not None:
            assert np.array_equal(grads_a[name].view(np.uint32), grads_b[name].view(np.uint32)), name


# ---- 5. train() -----------------------------------------------------------------------------------------------------------------------
SUBGRAPH = {"subgraph_batches": {"roots_per_batch": 32, "walk_length": 4, "seed": 1}}


def _train_two_epochs(device, result_dir, params, **model_params):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    from tf_gnn_samples_amd.tasks import subgraph_sampling
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
    task.load_synthetic(seed=2)                                       # synthetic Cora: 2708 nodes, 140 of them in the train fold
    p = RGCN_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3, **model_params)
    result_dir.mkdir()
    model = RGCN_Model(p, task, run_id="subgraph", result_dir=str(result_dir), device=str(device))
    record, roots_seen, run_epoch, sample = [], [], model._run_epoch, subgraph_sampling.SubgraphSampler.sample

    def recording(epoch_name, data, fold, quiet=False):
        del roots_seen[:]
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, len(out[1]), out[2], [m.get("num_masked") for m in out[1]], [float(m["loss"]) for m in out[1]],
                       [list(r) for r in roots_seen]))
        return out

    def sampling(self, roots, draw):
        roots_seen.append(np.asarray(roots).tolist())
        return sample(self, roots, draw)
    model._run_epoch = recording
    subgraph_sampling.SubgraphSampler.sample = sampling
    try:
        model.train(quiet=True, max_epochs=2)
    finally:
        subgraph_sampling.SubgraphSampler.sample = sample
        model._run_epoch = run_epoch
    torch.cuda.synchronize()
    return task, model, record, {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}


def test_train_on_subgraph_batches(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold, DeviceBatch
    task, model, record, first = _train_two_epochs(gpu_device, tmp_path / "a", SUBGRAPH)
    steps = math.ceil(140 / 32)
    # ceil(n_train / R) steps per training epoch, one full-graph validation pass
    assert [(r[1], r[2]) for r in record] == [(steps, steps), (1, 1), (steps, steps), (1, 1)], record
    train_nodes = np.flatnonzero(task._loaded_data[DataFold.TRAIN][0].mask).tolist()
    for epoch in (record[0], record[2]):
        assert [len(r) for r in epoch[5]] == [32, 32, 32, 32, 12]
        assert sorted(v for r in epoch[5] for v in r) == train_nodes                    # every train node is a root once per epoch
        assert all(masked >= len(r) for masked, r in zip(epoch[3], epoch[5]))           # all TRAIN nodes of the subgraph count
        assert np.isfinite(epoch[4]).all()
    assert record[0][5] != record[2][5] and record[1][3] == [None] and record[1][5] == []
    assert any(masked > len(r) for epoch in (record[0], record[2]) for masked, r in zip(epoch[3], epoch[5]))
    assert (task.batches.epoch, task.batches.draw) == (2, 2 * steps)
    with open(model.best_model_file, "rb") as f:
        saved_bits = {k: np.asarray(v).tobytes() for k, v in pickle.load(f)["weights"].items()}
    for pipeline in ({}, {"native_batching": False}):                 # either iterator, and again: the same losses, the same checkpoint
        _, other, again_record, again = _train_two_epochs(gpu_device, tmp_path / ("b%d" % len(pipeline)), SUBGRAPH, **pipeline)
        assert again_record == record
        for n in first:
            assert np.array_equal(first[n].view(np.uint32), again[n].view(np.uint32)), n
        with open(other.best_model_file, "rb") as f:
            assert {k: np.asarray(v).tobytes() for k, v in pickle.load(f)["weights"].items()} == saved_bits
    # the native iterator, asked directly, yields the same kind of epoch (the model routes both settings to one generator)
    train = task._loaded_data[DataFold.TRAIN]
    native = list(task.make_native_minibatch_iterator(model._native_pipeline(train), DataFold.TRAIN, 10 ** 6))
    numpy_side = list(task.make_minibatch_iterator(train, DataFold.TRAIN, 10 ** 6))
    for batches in (native, numpy_side):
        assert len(batches) == steps and all(isinstance(b, DeviceBatch) and "sampled_nodes" in b.extra for b in batches)
    assert (task.batches.epoch, task.batches.draw) == (4, 4 * steps)
    assert len(task.batches.graph_states) == 1                                # one device RelGraph and one feature table
    # restore(): the parameter comes back and the restored model trains on with it
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.subgraph_batches == SUBGRAPH["subgraph_batches"] and restored.task.get_metadata() == task.get_metadata()
    restored.task.load_synthetic(seed=2)
    before = {n: restored.variables[n].detach().clone() for n in restored.variables.names()}
    loss, results, *_ = restored._run_epoch("train", restored.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, quiet=True)
    assert len(results) == steps and np.isfinite(loss) and all("num_masked" in m for m in results)
    assert any(not torch.equal(before[n], restored.variables[n]) for n in before)
    # evaluation is untouched: VALIDATION and TEST metrics of the checkpoint under a task with and without the parameter
    with open(model.best_model_file, "rb") as f:
        saved = pickle.load(f)
    metrics = {}
    for which, params in (("with", SUBGRAPH), ("without", {})):
        t = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
        t.load_synthetic(seed=2)
        m = RGCN_Model(dict(saved["model_params"]), t, run_id=which, result_dir=str(tmp_path), device=str(gpu_device))
        m.load_weights(saved["weights"])
        valid = m._run_epoch("valid", t._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, quiet=True)
        test = m._run_epoch("test", t.synthetic_test_data, DataFold.TEST, quiet=True)
        metrics[which] = [(out[0], out[2], [{k: float(v) for k, v in r.items()} for r in out[1]]) for out in (valid, test)]
        (prediction,) = m.predict(t.synthetic_test_data)
        assert prediction["classes"].shape == (2708,) and prediction["probabilities"].shape == (2708, 7)
        named = m.predict(t.synthetic_test_data, nodes=[5, 2000, 5])                               # without an "evaluation" key, as ever
        assert np.array_equal(named["classes"], prediction["classes"][[5, 2000, 5]])
    assert metrics["with"] == metrics["without"] and len(metrics["with"][0][2]) == 1
    # a subgraph batch cannot be captured
    with pytest.raises(RuntimeError, match="sampled batch"):
        restored.capture_train_step(numpy_side[0])


# ---- 6. peak memory of an 8-layer step ------------------------------------------------------------------------------------------------
def test_an_eight_layer_step_on_a_subgraph_batch_peaks_below_the_full_graph_step(gpu_device):
    """V = 60 000, average in-degree 8 (4 neighbour-list entries per node, both directions) and a self loop, RGCN 8 x 64: a TRAIN epoch of
    subgraph batches (R = 256, h = 4: at most 1 280 nodes a step) against the one full-graph step of the same model on the same graph."""
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    peaks = {}
    for which, params in (("full", {}), ("subgraph", {"subgraph_batches": {"roots_per_batch": 256, "walk_length": 4}})):
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
        task.load_synthetic(num_nodes=60000, num_features=32, num_classes=5, num_train=1024, num_valid=500, num_test=500,
                            neighbours_per_node=4.0, feature_density=0.2, seed=1)
        train = task._loaded_data[DataFold.TRAIN]
        edges = sum(len(a) for a in train[0].adjacency_lists[1:])
        assert 7.5 < edges / 60000 < 8.5
        model = _model("RGCN_Model", task, gpu_device, 8, hidden_size=64)
        model._run_epoch("warm", train, DataFold.TRAIN, quiet=True)               # tables, plans and scratch are in place
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(gpu_device)
        before = torch.cuda.memory_allocated(gpu_device)
        _, res, steps, _, _, _ = model._run_epoch("measured", train, DataFold.TRAIN, quiet=True)
        torch.cuda.synchronize()
        peaks[which] = torch.cuda.max_memory_allocated(gpu_device) - before
        assert steps == len(res) == (1 if which == "full" else 4) and np.isfinite([float(m["loss"]) for m in res]).all()
        del model, task, train
    print("peak of a training epoch above the resting state: full graph %d bytes, subgraph batches %d bytes" % (peaks["full"], peaks["subgraph"]))
    assert 0 < peaks["subgraph"] < peaks["full"], peaks
