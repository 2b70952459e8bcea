"""Layered sampled batches without a GPU: the hop-ordered numbering is a relabelling of the id-ordered subgraph, hop_nodes / hop_edges
are cumulative and describe prefixes, integer propagation over the level graphs equals propagation over the union graph at every seed
(and a wrong level rule does not), the `"layered"` key is parsed, refused and kept in the metadata, and include/relgnn_layered_sampling.h's
entry points refuse bad arguments before any launch."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import layered_sampling_reference as LR  # noqa: E402

CASES = [(2, [3, 2]), (2, [0, 4]), (3, [2, 2, 2])]
_SAMPLES = {}


def hop_sample(L, fanouts, name):
    key = (L, tuple(fanouts), name)
    if key not in _SAMPLES:
        _, (rowptr, col, _) = LR.graph(L)
        _SAMPLES[key] = LR.sample_by_hop(rowptr, col, LR.V, L, LR.seed_lists(L)[name], fanouts, 7, seed=11, replica=2)
    return _SAMPLES[key]


def global_edges(nodes, adjacency_lists):
    rows = [np.stack([nodes[a[:, 0]], nodes[a[:, 1]], np.full(len(a), l)], axis=1) for l, a in enumerate(adjacency_lists)]
    rows = np.concatenate(rows).astype(np.int64)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("L,fanouts", CASES)
@pytest.mark.parametrize("name", ["mixed", "single", "all", "dead_end", "isolated"])
def test_hop_order_is_a_relabelling_and_the_levels_are_prefixes(L, fanouts, name):
    s = hop_sample(L, fanouts, name)
    base, H = s.by_id, len(fanouts)
    seeds = np.sort(LR.seed_lists(L)[name])
    # the same nodes, the same multiset of global (source, target, type) edges, the same degree of every global node, the same seeds
    assert np.array_equal(np.sort(s.nodes), base.nodes) and np.array_equal(s.nodes[s.new_of_old], base.nodes)
    assert np.array_equal(global_edges(s.nodes, s.adjacency_lists), global_edges(base.nodes, base.adjacency_lists))
    assert np.array_equal(s.degrees[:, s.new_of_old], base.degrees)
    assert np.array_equal(s.nodes[s.seed_mask == 1], seeds) and np.array_equal(base.nodes[base.seed_mask == 1], seeds)
    # node order: seeds first and ascending, every hop's group ascending, the groups' bounds cumulative
    assert len(s.hop_nodes) == H + 1 and s.hop_nodes[0] == len(seeds) and s.hop_nodes[-1] == len(s.nodes)
    assert all(a <= b for a, b in zip(s.hop_nodes, s.hop_nodes[1:]))
    assert np.array_equal(s.nodes[:len(seeds)], seeds) and np.array_equal(s.seed_mask, (np.arange(len(s.nodes)) < len(seeds)).astype(np.float32))
    for lo, hi in zip([0] + s.hop_nodes, s.hop_nodes):
        assert (np.diff(s.nodes[lo:hi]) > 0).all()
    # the lists: hop_edges cumulative, the edges hop d emitted have their targets in hop d's group, in ascending order; so the edges
    # whose target is below n_d are exactly the prefix hop_edges[l][d]
    for l, (a, cumulative) in enumerate(zip(s.adjacency_lists, s.hop_edges)):
        assert len(cumulative) == H and cumulative[-1] == len(a) and all(x <= y for x, y in zip(cumulative, cumulative[1:]))
        for d, (lo, hi) in enumerate(zip([0] + cumulative, cumulative)):
            targets = a[lo:hi, 1]
            assert (s.node_hop[targets] == d).all() and (np.diff(targets) >= 0).all()
            assert (s.node_hop[a[lo:hi, 0]] <= d + 1).all()
            assert np.array_equal(np.flatnonzero(a[:, 1] < s.hop_nodes[d]), np.arange(hi))
        assert np.array_equal(np.bincount(a[:, 1], minlength=len(s.nodes)), s.degrees[l])
    # the levels: every edge of level l has its target below n_{H-l} and its source below n_{H-l+1}; level 1 is the union graph
    levels = LR.levels(s)
    assert len(levels) == H
    for layer, (lists, sources, targets, table) in enumerate(levels, start=1):
        assert (sources, targets) == (s.hop_nodes[H - layer + 1], s.hop_nodes[H - layer]) and table.shape == (L, sources)
        for l, a in enumerate(lists):
            assert (a[:, 1] < targets).all() and (a[:, 0] < sources).all()
            assert np.array_equal(np.bincount(a[:, 1], minlength=sources), table[l])
    assert all(np.array_equal(a, b) for a, b in zip(levels[0][0], s.adjacency_lists)) and np.array_equal(levels[0][3], s.degrees)


def test_the_seed_lists_hold_the_cases_the_numbering_can_get_wrong():
    # a seed that is another seed's neighbour stays at level 0
    s = hop_sample(2, [3, 2], "mixed")
    n0 = s.hop_nodes[0]
    assert any(((a[:, 0] < n0) & (a[:, 1] < n0) & (a[:, 0] != a[:, 1])).any() for a in s.adjacency_lists)
    # a node reached in hop 1 and again in hop 2 stays at level 1: a hop-1 edge (target at level 1) whose source is at level 1 too,
    # and that source is also the source of a hop-0 edge
    s = hop_sample(2, [0, 4], "single")
    a, cumulative = s.adjacency_lists[0], s.hop_edges[0]
    again = a[cumulative[0]:cumulative[1]]
    again = again[s.node_hop[again[:, 0]] == 1][:, 0]
    assert len(again) and np.isin(again, a[:cumulative[0], 0]).all()
    # a hop that finds no new node; a hop that emits no edge
    s = hop_sample(2, [3, 2], "all")
    assert s.hop_nodes == [LR.V] * 3 and s.hop_edges[0][0] > 0 and all(e[1] == e[0] for e in s.hop_edges)
    assert [sources for _, sources, _, _ in LR.levels(s)] == [LR.V, LR.V]
    s = hop_sample(2, [3, 2], "dead_end")
    assert s.hop_nodes == [1, 2, 2] and s.hop_edges == [[1, 1], [0, 0]] and s.nodes.tolist() == [LR.DEAD_END, LR.ISOLATED]
    s = hop_sample(2, [3, 2], "isolated")
    assert s.hop_nodes == [1, 1, 1] and s.hop_edges == [[0, 0], [0, 0]]


@pytest.mark.parametrize("L,fanouts,residual_every", [(2, [3, 2], 10 ** 9), (2, [0, 4], 10 ** 9), (3, [2, 2, 2], 10 ** 9),
                                                       (3, [2, 2, 2], 2), (2, [3, 2], 1)])
@pytest.mark.parametrize("name", ["mixed", "single", "all", "dead_end"])
def test_propagation_over_the_levels_is_propagation_over_the_union_at_the_seeds(L, fanouts, residual_every, name):
    s = hop_sample(L, fanouts, name)
    H, n0 = len(fanouts), s.hop_nodes[0]
    states = np.random.default_rng(5).integers(1, LR.MODULUS, size=(len(s.nodes), 3))
    union = LR.propagate(states, s.adjacency_lists, H, residual_every)
    layered = LR.propagate_levels(states, LR.levels(s), residual_every)
    assert layered.shape == (n0, 3) and np.array_equal(layered, union[:n0])
    # the id-ordered subgraph is the same graph: the same states at the same global nodes
    by_id = LR.propagate(states[s.new_of_old], s.by_id.adjacency_lists, H, residual_every)
    assert np.array_equal(by_id, union[s.new_of_old])


@pytest.mark.parametrize("rule", ["one_hop_short", "per_hop"])
def test_a_wrong_level_rule_is_seen(rule):
    """The rule can be seen to break: with the prefix one hop too short, or with one hop's edges in place of the cumulative prefix,
    some seed's state differs from the union graph's."""
    for L, fanouts, name in [(2, [3, 2], "mixed"), (3, [2, 2, 2], "mixed")]:
        s = hop_sample(L, fanouts, name)
        H, n0 = len(fanouts), s.hop_nodes[0]
        states = np.random.default_rng(5).integers(1, LR.MODULUS, size=(len(s.nodes), 3))
        union = LR.propagate(states, s.adjacency_lists, H)
        assert np.array_equal(LR.propagate_levels(states, LR.levels(s), 10 ** 9), union[:n0])
        assert not np.array_equal(LR.propagate_levels(states, LR.levels(s, rule), 10 ** 9), union[:n0]), (rule, L, fanouts)


# ---- the parameter ------------------------------------------------------------------------------------------------------------------
GOOD = {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1, "layered": True}


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


def _cpu_model(task, **params):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(dict(dict(hidden_size=16, graph_num_layers=2, random_seed=1), **params))
    return RGCN_Model(p, task, device="cpu")


def test_the_key_is_parsed_refused_and_kept(tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks.neighbour_sampling import parse_sampled_batches
    plain = {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1}
    assert parse_sampled_batches(GOOD) == GOOD and parse_sampled_batches(dict(plain, layered=False)) == dict(plain, layered=False)
    assert parse_sampled_batches(plain) == plain and "layered" not in parse_sampled_batches(plain)        # absent by default
    assert _task(sampled_batches=GOOD).layered and not _task(sampled_batches=plain).layered and not _task().layered
    assert not _task(sampled_batches=dict(plain, layered=False)).layered
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match="layered"):
            _task(sampled_batches=dict(plain, layered=bad))
    with pytest.raises(ValueError, match="sampled_batches must be"):                 # an unknown key is still refused
        _task(sampled_batches=dict(GOOD, layerd=True))
    # it composes with the other optional keys
    every = dict(GOOD, sparse_features=True, sparse_update=True, sparse_gradient=True)
    assert _task(sampled_batches=every, sparse_node_features=True).sampled_batches == every
    # messages that other tests pin are as they were
    with pytest.raises(ValueError, match="sparse_node_features"):
        _task(sampled_batches=GOOD, sparse_node_features=True)
    with pytest.raises(ValueError, match='"sparse_update": true requires "sparse_features": true'):
        _task(sampled_batches=dict(GOOD, sparse_update=True))
    with pytest.raises(ValueError, match='"sparse_gradient": true requires "sparse_update": true'):
        _task(sampled_batches=dict(GOOD, sparse_gradient=True))
    # the metadata round trip
    task = _task(sampled_batches=GOOD)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    assert task.get_metadata()["params"]["sampled_batches"] == GOOD
    path = str(tmp_path / "model.pickle")
    _cpu_model(task).save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.sampled_batches == GOOD and restored.task.layered
    other = _task()
    other.restore_from_metadata(task.get_metadata())
    assert other.sampled_batches == GOOD


def test_the_model_refuses_what_the_levels_cannot_do():
    from tf_gnn_samples_amd.tasks import DataFold
    task = _task(sampled_batches=GOOD)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    with pytest.raises(ValueError, match='"layered".*graph_num_layers'):
        _cpu_model(task, graph_num_layers=3)
    with pytest.raises(ValueError, match='"layered".*graph_num_timesteps_per_layer'):
        _cpu_model(task, graph_num_timesteps_per_layer=2)
    # without the key neither is asked
    plain = _task(sampled_batches={k: v for k, v in GOOD.items() if k != "layered"})
    plain.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    _cpu_model(plain, graph_num_layers=3, graph_num_timesteps_per_layer=2)
    # the existing refusals stay: a CPU model, a captured step
    model = _cpu_model(task)
    with pytest.raises(RuntimeError, match="GPU"):
        model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)
    with pytest.raises(RuntimeError, match="no device bound"):
        next(iter(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, 100)))
    # the other folds are the full graph
    (mb,) = model._batches(task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION)
    assert mb.num_nodes == 120 and "layer_graphs" not in mb.feed_dict


def test_header_binding_and_library_agree():
    """include/relgnn_layered_sampling.h: the refusals that return before anything is launched (tests/test_abi.py holds the header
    against the binding)."""
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = _lib.load_library()
    fake = 4096                                            # an aligned non-null "pointer": every call below returns before it is read
    starts = lambda *v: (ctypes.c_int64 * len(v))(*v)
    relabel = lambda first=0, count=4, V=10, hs=starts(0, 2, 5), levels=2, edges=fake, out=fake, stamp=fake, nodes=fake: \
        lib.relgnn_neighbour_sample_relabel_by_hop(edges, first, count, stamp, V, nodes, hs, levels, out, None)
    assert relabel(count=0) == _lib.OK                     # nothing to relabel: nothing launched
    for bad in (dict(first=-1), dict(count=-1), dict(V=0), dict(hs=None), dict(hs=starts(1, 2, 5)), dict(hs=starts(0, 3, 2)),
                dict(hs=starts(0, 0, 0)), dict(edges=None), dict(out=None), dict(stamp=None), dict(nodes=None), dict(out=fake + 4)):
        assert relabel(**bad) == _lib.EINVAL, bad
    assert relabel(levels=0) == _lib.EUNSUPPORTED and relabel(levels=10, hs=starts(*range(11))) == _lib.EUNSUPPORTED
    assert relabel(hs=starts(0, 2, 1 << 31)) == _lib.EUNSUPPORTED
    degrees = lambda B=8, nf=4, L=2, base=0, n=8, counts=fake, out=fake: lib.relgnn_neighbour_sample_degrees_by_hop(counts, B, nf, L, base, n,
                                                                                                             out, None)
    assert degrees(nf=0) == _lib.OK
    for bad in (dict(nf=-1), dict(nf=9), dict(L=0), dict(base=-1), dict(base=5), dict(n=3), dict(counts=None), dict(out=None)):
        assert degrees(**bad) == _lib.EINVAL, bad
