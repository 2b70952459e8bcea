"""`"blocks": true` without a GPU: the derivation of a level's bucketing from the union graph's (tests/block_levels_reference.py) equals
the constructor's bucketing of the level's prefix lists, array for array, and four plausible mistakes do not; the arena layout that
relgnn_level_plan is told; the key is parsed, refused and kept in the metadata; csrc/level_plan.h is held to the binding and the
library, and its entry point refuses bad arguments before any launch."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import block_levels_reference as BR  # noqa: E402
import layered_sampling_reference as LR  # noqa: E402
from abi_reference import declared_names, declared_signatures  # noqa: E402

HEADER = "../tf_gnn_samples_amd/csrc/level_plan.h"
FANOUTS = [[3, 2], [2, 2, 2], [0, 4]]
TYPES = [1, 2, 3]
NAMES = ["mixed", "single", "all", "dead_end", "isolated"]
_SAMPLES = {}


def hop_sample(L, fanouts, name):
    key = (L, tuple(fanouts), name)
    if key not in _SAMPLES:
        _, (rowptr, col, _) = LR.graph(L)
        sample = LR.sample_by_hop(rowptr, col, LR.V, L, LR.seed_lists(L)[name], fanouts, 7, seed=11, replica=2)
        _SAMPLES[key] = (sample, BR.constructor(sample.adjacency_lists, len(sample.nodes)))
    return _SAMPLES[key]


@pytest.mark.parametrize("fanouts", FANOUTS, ids=str)
@pytest.mark.parametrize("L", TYPES)
def test_the_derivation_is_the_constructor(L, fanouts):
    H = len(fanouts)
    for name in NAMES:
        s, union = hop_sample(L, fanouts, name)
        for d in range(H - 1):
            want = BR.constructor(BR.level_lists(s.adjacency_lists, s.hop_edges, d), s.hop_nodes[d + 1])
            got = BR.derive(union, s.hop_nodes, s.hop_edges, d)
            for k in BR.ARRAYS:
                assert got[k].dtype == want[k].dtype == np.int32 and got[k].shape == want[k].shape, (name, d, k)
                assert np.array_equal(got[k], want[k]), (name, d, k)
            # the claims the kernels stand on: the by-target arrays are a prefix, col_t keeps its values
            P = len(want["col_t"])
            assert np.array_equal(want["col_t"], union["col_t"][:P])
            assert np.array_equal(want["rowptr_t"][:s.hop_nodes[d] * L + 1], union["rowptr_t"][:s.hop_nodes[d] * L + 1])
            assert (want["rowptr_t"][s.hop_nodes[d] * L:] == P).all()
            assert P == 0 or want["tgt_s"].max() < s.hop_nodes[d]
        # level H - 1 is the union graph itself: the leaves have no incoming edge
        assert union["rowptr_t"][s.hop_nodes[H - 1] * L] == len(union["col_t"])
        assert len(union["tgt_s"]) == 0 or union["tgt_s"].max() < s.hop_nodes[H - 1]


def test_the_cases_hold_what_the_derivation_can_get_wrong():
    s, _ = hop_sample(2, [3, 2], "all")                                # a hop that reached nothing new: T == S
    assert s.hop_nodes[0] == s.hop_nodes[1]
    s, _ = hop_sample(2, [3, 2], "isolated")                           # M == 0
    assert sum(len(a) for a in s.adjacency_lists) == 0
    s, _ = hop_sample(2, [3, 2], "dead_end")                           # an edge type with no edges, a level whose deeper hop adds none
    assert len(s.adjacency_lists[1]) == 0 and s.hop_edges[0][0] == s.hop_edges[0][1] == 1
    s, _ = hop_sample(2, [2, 2, 2], "isolated")                        # levels with no edges
    assert all(e[0] == 0 for e in s.hop_edges)
    s, union = hop_sample(2, [0, 4], "single")                         # source buckets that the filter thins out, none to nothing
    kept = np.diff(BR.derive(union, s.hop_nodes, s.hop_edges, 0)["rowptr_s"])
    assert ((kept > 1) & (kept < np.diff(union["rowptr_s"])[:len(kept)])).any()


@pytest.mark.parametrize("mistake", BR.MISTAKES)
def test_every_named_mistake_is_seen(mistake):
    """Over the cases of the test above a derivation that made this mistake differs from the constructor in at least one level (and
    with more than one edge type where the mistake needs one: a re-basing by zero is right for L = 1)."""
    differing, total = [], 0
    for L in TYPES:
        for fanouts in FANOUTS:
            for name in NAMES:
                s, union = hop_sample(L, fanouts, name)
                for d in range(len(fanouts) - 1):
                    want = BR.constructor(BR.level_lists(s.adjacency_lists, s.hop_edges, d), s.hop_nodes[d + 1])
                    assert BR.equal(BR.derive(union, s.hop_nodes, s.hop_edges, d), want)
                    total += 1
                    if not BR.equal(BR.derive(union, s.hop_nodes, s.hop_edges, d, mistake), want):
                        differing.append((L, fanouts, name, d))
    print(mistake, len(differing), "of", total)
    assert differing
    assert any(L == 2 for L, *_ in differing) and any(L == 3 for L, *_ in differing)
    if mistake != "perm_not_rebased":
        assert any(L == 1 for L, *_ in differing)


def test_the_layout_of_the_output_arena():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import LEVEL_PLAN_ARRAYS, LEVEL_PLAN_FIXED, level_plan_layout
    s, _ = hop_sample(3, [2, 2, 2], "mixed")
    L, H = 3, 3
    desc, length, max_rows, max_messages = level_plan_layout(s.hop_nodes, s.hop_edges, L)
    assert desc.dtype == np.int64 and desc.shape == (H - 1, LEVEL_PLAN_FIXED + 2 * L + 1) and LEVEL_PLAN_FIXED == 3 + len(LEVEL_PLAN_ARRAYS)
    regions = []
    for d in range(H - 1):
        T, S, P = desc[d, :3]
        assert (T, S) == (s.hop_nodes[d], s.hop_nodes[d + 1]) and P == sum(e[d] for e in s.hop_edges)
        offsets = desc[d, LEVEL_PLAN_FIXED + L:]
        assert offsets[0] == 0 and offsets[-1] == P and np.array_equal(np.diff(offsets), [e[d] for e in s.hop_edges])
        union_offsets = np.concatenate([[0], np.cumsum([e[H - 1] for e in s.hop_edges])])
        assert np.array_equal(desc[d, LEVEL_PLAN_FIXED:LEVEL_PLAN_FIXED + L], union_offsets[:L] - offsets[:L])
        for k, name in enumerate(LEVEL_PLAN_ARRAYS):
            regions.append((int(desc[d, 3 + k]), S * L + 1 if name.startswith("rowptr") else P))
    regions.sort()
    assert regions[0][0] == 0 and all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))       # no overlap
    assert regions[-1][0] + regions[-1][1] <= length and all(a % 4 == 0 for a, _ in regions)
    assert max_rows == max(desc[:, 1]) * L + 1 and max_messages == max(desc[:, 2])
    # H = 1: no level below the union graph
    desc, length, max_rows, max_messages = level_plan_layout([4, 9], [[5], [2]], 2)
    assert desc.shape[0] == 0 and (length, max_rows, max_messages) == (0, 0, 0)


# ---- the parameter ------------------------------------------------------------------------------------------------------------------
PLAIN = {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1}
LAYERED = dict(PLAIN, layered=True)
GOOD = dict(LAYERED, blocks=True)
EVALUATION = {"fanouts": [0, 0], "seeds_per_batch": 64}


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
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    from tf_gnn_samples_amd.tasks.neighbour_sampling import parse_sampled_batches
    from tf_gnn_samples_amd.tasks.subgraph_sampling import parse_subgraph_batches
    assert Citation_Network_Task.default_params().get("sampled_batches") is None
    assert parse_sampled_batches(GOOD) == GOOD and list(parse_sampled_batches(GOOD))[-1] == "blocks"
    assert parse_sampled_batches(dict(LAYERED, blocks=False)) == dict(LAYERED, blocks=False)
    assert parse_sampled_batches(dict(PLAIN, blocks=False)) == dict(PLAIN, blocks=False)          # false needs nothing
    # absent by default: every parsed dict is the one it was
    for value in (PLAIN, LAYERED, dict(PLAIN, evaluation=EVALUATION), dict(LAYERED, data_parallel=True)):
        assert parse_sampled_batches(value) == value and "blocks" not in parse_sampled_batches(value)
    assert _task(sampled_batches=GOOD).blocks and not _task(sampled_batches=LAYERED).blocks and not _task().blocks
    assert not _task(sampled_batches=dict(LAYERED, blocks=False)).blocks
    # with "evaluation" alone, and with both
    with_evaluation = dict(PLAIN, evaluation=EVALUATION, blocks=True)
    assert parse_sampled_batches(with_evaluation) == with_evaluation and _task(sampled_batches=with_evaluation).blocks
    assert parse_sampled_batches(dict(GOOD, evaluation=dict(EVALUATION, keep=True)))["blocks"] is True
    # neither "layered" nor "evaluation": the refusal names all three
    for value in (dict(PLAIN, blocks=True), dict(PLAIN, layered=False, blocks=True)):
        with pytest.raises(ValueError, match='"blocks".*"layered".*"evaluation"'):
            _task(sampled_batches=value).sampled_batches
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match="blocks"):
            _task(sampled_batches=dict(LAYERED, blocks=bad)).sampled_batches
    with pytest.raises(ValueError, match="sampled_batches must be"):                 # an unknown key is still refused
        _task(sampled_batches=dict(GOOD, block=True)).sampled_batches
    with pytest.raises(ValueError, match="subgraph_batches"):                        # no levels there: the key is unknown
        parse_subgraph_batches({"roots_per_batch": 8, "walk_length": 2, "blocks": True})
    # it composes with the other optional keys
    every = dict(GOOD, sparse_features=True, sparse_update=True, sparse_gradient=True)
    assert _task(sampled_batches=every, sparse_node_features=True).sampled_batches == every
    parallel = dict(GOOD, data_parallel=True, evaluation=EVALUATION)
    assert _task(sampled_batches=parallel).sampled_batches == parallel
    # messages that other tests pin are as they were
    with pytest.raises(ValueError, match="sparse_node_features"):
        _task(sampled_batches=GOOD, sparse_node_features=True).sampled_batches
    with pytest.raises(ValueError, match='"sparse_update": true requires "sparse_features": true'):
        _task(sampled_batches=dict(GOOD, sparse_update=True)).sampled_batches
    with pytest.raises(ValueError, match='"data_parallel": true cannot be combined with "sparse_update": true'):
        _task(sampled_batches=dict(every, data_parallel=True), sparse_node_features=True).sampled_batches
    # the metadata round trip, and the data-parallel fingerprint
    task = _task(sampled_batches=GOOD)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    assert task.get_metadata()["params"]["sampled_batches"] == GOOD
    from tf_gnn_samples_amd.tasks import DataFold
    folds = {"train": task._loaded_data[DataFold.TRAIN][0]}
    assert task.batches.fingerprint(folds)["sampled_batches"] == GOOD
    path = str(tmp_path / "model.pickle")
    _cpu_model(task).save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.sampled_batches == GOOD and restored.task.blocks and restored.task.layered
    other = _task()
    other.restore_from_metadata(task.get_metadata())
    assert other.sampled_batches == GOOD


def test_a_graph_knows_its_target_rows():
    """num_targets is V for everything built without the key; from_arrays takes another and refuses one outside [0, V]."""
    import torch
    from tf_gnn_samples_amd.graph import RelGraph
    rowptr = torch.zeros(7, dtype=torch.int32)
    empty = torch.zeros(0, dtype=torch.int32)
    arrays = dict(rowptr_t=rowptr, rowptr_s=rowptr, tgt_s=empty, perm_t=empty, col_t=empty, inv_perm_t=empty, perm_s=empty, frow_s=empty,
                  pos_t_of_s=empty)
    lists = [torch.zeros((0, 2), dtype=torch.int32)] * 2
    assert RelGraph.from_arrays(lists, 3, **arrays).num_targets == 3
    assert RelGraph.from_arrays(lists, 3, num_targets=1, **arrays).num_targets == 1
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="num_targets"):
            RelGraph.from_arrays(lists, 3, num_targets=bad, **arrays)


# ---- the package-internal header ----------------------------------------------------------------------------------------------------
def _library():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    return _lib, _lib.load_library()


def test_the_internal_header_is_held_to_the_binding_and_the_library():
    _lib, lib = _library()
    table = _lib.INTERNAL["level_plan.h"]
    names = declared_names(HEADER)
    declared = declared_signatures(HEADER)
    assert names == sorted(declared) == sorted(table)
    assert {"relgnn_level_plan", "relgnn_level_plan_workspace_bytes"} <= set(names)
    wrong = {n: (table[n], declared[n]) for n in declared if (table[n][0], list(table[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert not [n for n in names if not hasattr(raw, n)]
    for name, (restype, argtypes) in table.items():               # load_library() types this table too
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # not public ABI: no header under include/ speaks of it
    assert not set(table) & set(_lib.signatures())
    for p in (HERE.parent / "include").iterdir():
        assert "level_plan" not in p.name and "relgnn_level_plan" not in p.read_text(), p.name


def test_the_host_checks_its_arguments_in_front_of_a_launch():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import LEVEL_PLAN_FIXED, MAX_HOPS
    _lib, lib = _library()
    assert lib.relgnn_level_plan_max_levels() == MAX_HOPS - 1 == 7 and lib.relgnn_level_plan_tile() == 1024
    assert [lib.relgnn_level_plan_desc_stride(L) for L in (1, 2, 23)] == [LEVEL_PLAN_FIXED + 2 * L + 1 for L in (1, 2, 23)]
    assert lib.relgnn_level_plan_desc_stride(0) == 0
    size = lib.relgnn_level_plan_workspace_bytes
    assert size(0, 3) == 0 and size(100, 0) == 0 and size(100, 8) == 0 and size(-1, 1) == 0
    # per tile of 1024 entries and level: 16 masks of 8 bytes, 16 wave offsets and one tile offset of 4
    assert size(1, 1) >= 16 * 12 + 4 and size(1025, 7) >= 2 * 7 * (16 * 12 + 4) and size(1024, 1) == size(1, 1)
    assert 7 * 1024 * (16 * 12 + 4) <= size(1 << 20, 7) < 7 * 1024 * (16 * 12 + 4) + 3 * 256 and size(1 << 20, 7) < size((1 << 20) + 1, 7)
    plan = lib.relgnn_level_plan

    def args(V=10, L=2, M=0, levels=1, rows=5, messages=0, length=64, pointers=1, desc=1, out=1, ws=0):
        p = ctypes.c_void_p(256) if pointers else None             # (never dereferenced: every call here returns in front of a launch)
        return (p, p, p, p, p, p, p, p, p, V, L, M, ctypes.c_void_p(256) if desc else None, levels, rows, messages,
                ctypes.c_void_p(256) if out else None, length, None, ws, None)
    assert plan(*args(levels=0, pointers=0, desc=0, out=0)) == _lib.OK            # no level: no launch, nothing is read
    for bad in (dict(V=-1), dict(M=-1), dict(L=0), dict(levels=-1), dict(levels=8), dict(length=-1), dict(rows=-1), dict(messages=-1),
                dict(rows=22), dict(messages=1), dict(V=1 << 30, L=2), dict(desc=0), dict(pointers=0), dict(out=0),
                dict(M=5, messages=5, ws=0)):
        assert plan(*args(**bad)) == _lib.EINVAL, bad
