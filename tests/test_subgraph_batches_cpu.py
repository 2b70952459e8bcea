"""Random-walk subgraph batches without a GPU: the rules as tests/subgraph_reference.py states them (against a brute-force edge filter,
and shown to notice five plausible mistakes), the task parameter's validation and refusals, checkpoint metadata, the header."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import philox_reference as P  # noqa: E402
import subgraph_reference as S  # noqa: E402


def small_graph(V=60, L=2, seed=0, hub=200):
    """Random typed graph with duplicate edges, self loops, empty buckets, nodes without an in-edge (the last five) and one hub
    bucket (node 0, type L - 1) of `hub` entries."""
    rng = np.random.default_rng(seed)
    adjacency = []
    for l in range(L):
        e = rng.integers(0, V, size=(4 * V, 2))
        e[:10] = e[10:20]                                               # duplicates
        e[20:25, 0] = e[20:25, 1]                                       # self loops
        e = e[(e[:, 1] % 7 != l) & (e[:, 1] < V - 5)]                   # some empty buckets; five nodes nobody points at
        if l == L - 1:
            e = np.concatenate([e, np.stack([rng.integers(0, V, size=hub), np.zeros(hub, np.int64)], axis=1)])
        adjacency.append(e.astype(np.int32))
    return adjacency


def same(a: S.Induced, b: S.Induced) -> bool:
    return (np.array_equal(a.nodes, b.nodes) and len(a.adjacency_lists) == len(b.adjacency_lists)
            and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists))
            and np.array_equal(a.degrees.view(np.uint32), b.degrees.view(np.uint32)) and np.array_equal(a.seed_mask, b.seed_mask))


@pytest.mark.parametrize("L", [1, 2, 3])
def test_induced_reference_equals_a_brute_force_edge_filter(L):
    V = 60
    for seed in range(4):
        adjacency = small_graph(V, L, seed)
        rowptr, col, _ = S.bucketing(adjacency, V)
        rng = np.random.default_rng([seed, L])
        for nodes in (rng.choice(V, size=25, replace=False), np.array([0]), np.arange(V), np.array([V - 1, 0, 7])):
            got, want = S.induced(rowptr, col, V, L, nodes), S.brute_force(adjacency, V, nodes)
            assert same(got, want), (seed, L, len(nodes))
            assert got.nodes.dtype == np.int32 and got.degrees.dtype == np.float32 and all(a.dtype == np.int32 for a in got.adjacency_lists)
            for l, a in enumerate(got.adjacency_lists):
                assert (np.diff(a[:, 1]) >= 0).all()                    # targets ascend within a type
                assert np.array_equal(np.bincount(a[:, 1], minlength=len(got.nodes)), got.degrees[l])
    # all V nodes: the lists hold every edge of the full graph, in the by-target order
    everything = S.induced(rowptr, col, V, L, np.arange(V))
    for a, full in zip(everything.adjacency_lists, adjacency):
        assert np.array_equal(a, full[np.argsort(full[:, 1], kind="stable")])


def test_walk_reference_properties():
    V, L, h = 60, 2, 5
    adjacency = small_graph(V, L)
    rowptr, col, _ = S.bucketing(adjacency, V)
    roots = np.array([0, 5, 17, 18, 57, 59], np.int32)                  # 57 and 59 have no in-edge: their walks stay
    nodes = S.walk_nodes(rowptr, col, V, L, roots, h, draw=2, seed=3)
    assert nodes.dtype == np.int32 and (np.diff(nodes) > 0).all() and set(roots) <= set(nodes) and len(nodes) <= len(roots) * (h + 1)
    assert np.array_equal(S.walk_nodes(rowptr, col, V, L, roots, 0, 2, 3), np.sort(roots))              # h = 0: the roots alone
    assert np.array_equal(S.walk_nodes(rowptr, col, V, L, np.array([57, 59]), 8, 2, 3), [57, 59])       # dead ends
    # walk by walk, by hand: every step goes to an in-neighbour of the node it leaves, the one the multiply-high picks
    r64, c64 = rowptr.astype(np.int64), col.astype(np.int64)
    visited = set()
    for w, root in enumerate(roots):
        v = int(root)
        visited.add(v)
        for step in range(h):
            b, e = r64[v * L], r64[(v + 1) * L]
            if e == b:
                continue
            word = int(P.philox4x32_10((w, step, 2, 0), (3, 0))[0])
            v = int(c64[b + ((word * int(e - b)) >> 32)] // L)
            visited.add(v)
    assert sorted(visited) == nodes.tolist()
    # the same arguments give the same set; another draw, seed or replica gives another
    assert np.array_equal(nodes, S.walk_nodes(rowptr, col, V, L, roots, h, draw=2, seed=3))
    for other in (dict(draw=3, seed=3), dict(draw=2, seed=4), dict(draw=2, seed=3, replica=1)):
        assert not np.array_equal(nodes, S.walk_nodes(rowptr, col, V, L, roots, h, **other))
    sub = S.sample(rowptr, col, V, L, roots, h, 2, 3)
    assert same(sub, S.induced(rowptr, col, V, L, nodes)) and sub.seed_mask.all()


@pytest.mark.parametrize("mistake", ["drop_edge", "source_order", "full_degrees"])
def test_the_comparison_notices_a_wrong_induced_subgraph(mistake):
    V, L = 60, 2
    adjacency = small_graph(V, L)
    rowptr, col, _ = S.bucketing(adjacency, V)
    nodes = np.random.default_rng(1).choice(V, size=30, replace=False)
    assert not same(S.induced(rowptr, col, V, L, nodes, mistake=mistake), S.brute_force(adjacency, V, nodes))


@pytest.mark.parametrize("mistake", ["out_edges", "modulo"])
def test_the_comparison_notices_a_wrong_walk(mistake):
    V, L = 60, 2
    adjacency = small_graph(V, L)
    rowptr, col, _ = S.bucketing(adjacency, V)
    roots = np.arange(0, 40, 3)
    right = S.walk_nodes(rowptr, col, V, L, roots, 4, draw=0, seed=1)
    assert not np.array_equal(right, S.walk_nodes(rowptr, col, V, L, roots, 4, draw=0, seed=1, mistake=mistake))


# ---- the task parameter -------------------------------------------------------------------------------------------------------------
def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


GOOD = {"roots_per_batch": 32, "walk_length": 4, "seed": 1}


def test_good_forms():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    from tf_gnn_samples_amd.tasks.subgraph_sampling import MAX_WALK_LENGTH, parse_subgraph_batches
    assert "subgraph_batches" not in Citation_Network_Task.default_params()
    assert _task().subgraph_batches is None and _task(subgraph_batches=None).subgraph_batches is None
    assert parse_subgraph_batches(None) is None
    assert _task(subgraph_batches=GOOD).subgraph_batches == GOOD and _task(subgraph_batches=GOOD).sampled_batches is None
    assert _task(subgraph_batches={"roots_per_batch": 7, "walk_length": 0}).subgraph_batches == {"roots_per_batch": 7, "walk_length": 0, "seed": 0}
    assert parse_subgraph_batches({"roots_per_batch": np.int64(3), "walk_length": np.int32(64)}) == {"roots_per_batch": 3, "walk_length": 64, "seed": 0}
    assert MAX_WALK_LENGTH == S.MAX_WALK_LENGTH == 64
    sparse = dict(GOOD, sparse_features=True)
    assert _task(subgraph_batches=sparse, sparse_node_features=True).subgraph_batches == sparse
    assert _task(subgraph_batches=dict(GOOD, sparse_features=False)).subgraph_batches == dict(GOOD, sparse_features=False)


@pytest.mark.parametrize("bad, message", [
    ([32, 4], "subgraph_batches must be"), ("walks", "subgraph_batches must be"),
    ({"roots_per_batch": 32}, "subgraph_batches must be"), ({"walk_length": 4}, "subgraph_batches must be"),
    ({"roots_per_batch": 32, "walk_length": 4, "fanouts": [3]}, "unknown key 'fanouts'"),
    ({"roots_per_batch": 0, "walk_length": 4}, "roots_per_batch must be a positive integer"),
    ({"roots_per_batch": 2.0, "walk_length": 4}, "roots_per_batch must be a positive integer"),
    ({"roots_per_batch": True, "walk_length": 4}, "roots_per_batch must be a positive integer"),
    ({"roots_per_batch": 32, "walk_length": -1}, r"subgraph_batches: walk_length must be an integer in \[0, 64\]"),
    ({"roots_per_batch": 32, "walk_length": 65}, r"subgraph_batches: walk_length must be an integer in \[0, 64\]"),
    ({"roots_per_batch": 32, "walk_length": 2.0}, "walk_length must be an integer"),
    ({"roots_per_batch": 32, "walk_length": False}, "walk_length must be an integer"),
    ({"roots_per_batch": 32, "walk_length": 4, "seed": "1"}, "seed must be an integer"),
    ({"roots_per_batch": 32, "walk_length": 4, "sparse_features": 1}, "sparse_features must be true or false"),
])
def test_malformed_values_are_value_errors_when_the_task_is_made(bad, message):
    with pytest.raises(ValueError, match=message):
        _task(subgraph_batches=bad)


@pytest.mark.parametrize("key", ["sparse_update", "sparse_gradient", "layered", "evaluation"])
def test_keys_of_sampled_batches_are_unknown_keys_here(key):
    with pytest.raises(ValueError, match="subgraph_batches must be .* unknown key '%s'" % key):
        _task(subgraph_batches=dict(GOOD, **{key: True}))


def test_refusals_name_the_parameter():
    with pytest.raises(ValueError, match="subgraph_batches cannot be combined with sampled_batches"):
        _task(subgraph_batches=GOOD, sampled_batches={"fanouts": [5, 5], "seeds_per_batch": 32})
    with pytest.raises(ValueError, match="subgraph_batches cannot be combined with sparse_node_features unless"):
        _task(subgraph_batches=GOOD, sparse_node_features=True)
    with pytest.raises(ValueError, match='subgraph_batches: "sparse_features": true requires the task parameter sparse_node_features'):
        _task(subgraph_batches=dict(GOOD, sparse_features=True))


def _cpu_model(task):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, random_seed=1)
    return RGCN_Model(p, task, device="cpu")


def test_a_cpu_model_is_refused_and_so_is_a_captured_step():
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    task = _task(subgraph_batches=GOOD)
    task.load_synthetic(num_nodes=200, num_features=12, num_classes=3, num_train=40, num_valid=50, num_test=50)
    model = _cpu_model(task)
    train = task._loaded_data[DataFold.TRAIN]
    with pytest.raises(RuntimeError, match="GPU"):
        model._batches(train, DataFold.TRAIN)
    with pytest.raises(RuntimeError, match="no device bound"):              # the iterators alone, without a model
        next(iter(task.make_minibatch_iterator(train, DataFold.TRAIN, 100)))
    # the other folds are the full graph, as ever
    (mb,) = model._batches(task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION)
    assert mb.num_nodes == 200 and "sampled_nodes" not in mb.feed_dict
    batch = DeviceBatch(mb, "cpu")
    batch.extra["sampled_nodes"] = torch.arange(200, dtype=torch.int32)     # (what every subgraph batch carries)
    with pytest.raises(RuntimeError, match="sampled batch"):
        model.capture_train_step(batch)


def test_process_groups_stay_refused(monkeypatch):
    import torch.distributed as dist
    from tf_gnn_samples_amd.tasks import DataFold
    task = _task(subgraph_batches=GOOD)
    task.load_synthetic(num_nodes=100, num_features=8, num_classes=3, num_train=20, num_valid=20, num_test=20)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="cannot be split by graph"):
        list(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, 100))


def test_checkpoint_metadata_keeps_the_parameter(tmp_path):
    from tf_gnn_samples_amd import models
    task = _task(subgraph_batches=GOOD)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    assert task.get_metadata()["params"]["subgraph_batches"] == GOOD
    model = _cpu_model(task)
    path = str(tmp_path / "model.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.subgraph_batches == GOOD and restored.task.get_metadata() == task.get_metadata()
    plain = _task()
    plain.restore_from_metadata(task.get_metadata())
    assert plain.subgraph_batches == GOOD and plain.sampled_batches is None


def test_a_graph_on_the_cpu_is_refused():
    """The sampler is a HIP kernel: no CPU fallback."""
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, check_walk_length
    with pytest.raises(ValueError, match="walk_length"):
        check_walk_length(65)

    class OnTheHost:
        rowptr_t = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.RelGnnLibraryError, match="GPU only"):
        SubgraphSampler(OnTheHost(), 2)


# ---- include/relgnn_subgraph.h: its limits and host-side refusals (tests/test_abi.py holds the header against the binding) ----------
def test_header_binding_and_library_agree():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = _lib.load_library()
    assert lib.relgnn_subgraph_max_walk_length() == 64
    assert lib.relgnn_subgraph_supported(1024, 8, 1 << 20, 2) == 1 and lib.relgnn_subgraph_supported(1, 0, 300, 3) == 1
    assert lib.relgnn_subgraph_supported(1, 64, 300, 3) == 1 and lib.relgnn_subgraph_supported(1, 65, 300, 3) == 0
    assert lib.relgnn_subgraph_supported(0, 2, 300, 3) == 0 and lib.relgnn_subgraph_supported(1, -1, 300, 3) == 0
    assert lib.relgnn_subgraph_supported(1, 1, 1 << 30, 2) == 0                          # V * L = 2^31
    assert lib.relgnn_subgraph_supported(1, 1, (1 << 30) - 1, 2) == 1
    # argument checks run on the host in front of the launch
    assert lib.relgnn_subgraph_walk(None, None, 300, 2, None, 4, 65, 0, 0, 0, None, None) == _lib.EUNSUPPORTED
    assert lib.relgnn_subgraph_walk(None, None, 300, 2, None, 4, 2, 0, 0, 0, None, None) == _lib.EINVAL
    assert lib.relgnn_subgraph_induced_emit(None, None, 300, 2, None, 5, 4, None, None, 0, None, None, None) == _lib.EINVAL   # n > bound
    assert lib.relgnn_subgraph_clear(None, 0, None, 300, None) == _lib.OK
