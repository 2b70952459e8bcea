"""The graph partitioner without a GPU: the key "partition" of `subgraph_batches` (its forms, refusals and way through the checkpoint
metadata), the rule itself on its NumPy restatement (tests/graph_partition_reference.py: invariants, a hand-worked case, the locality it
finds, the mistakes the tests must be able to see), the package-internal header against the binding and the library, and the host
argument checks."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import graph_partition_reference as R  # noqa: E402
from abi_reference import declared_names, declared_signatures  # noqa: E402

NORM = {"presample_epochs": 2}
PARSED_NORM = {"presample_epochs": 2, "aggregation": True, "max_edge_weight": 1e4}
HEADER = "../tf_gnn_samples_amd/csrc/graph_partition.h"
PLANTED = [(512, 8, 8), (512, 8, 16), (300, 5, 7)]          # (V, communities, P)
SEEDS = (0, 1, 2)


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


def _value(partition, **more):
    return dict({"partition": partition, "parts_per_batch": 2, "sampler": "parts", "normalisation": NORM}, **more)


# ---- the parameter --------------------------------------------------------------------------------------------------------------------
def test_partition_takes_the_place_of_parts_path():
    from tf_gnn_samples_amd.tasks.subgraph_sampling import parse_subgraph_batches
    full = {"num_parts": 8, "imbalance_percent": 10, "refine_rounds": 8}
    assert parse_subgraph_batches(_value({"num_parts": 8}, seed=3)) == {"partition": full, "parts_per_batch": 2, "seed": 3, "sampler": "parts",
                                                                       "normalisation": PARSED_NORM}
    asked = {"num_parts": np.int64(5), "imbalance_percent": 0, "refine_rounds": 64}
    assert parse_subgraph_batches(_value(asked))["partition"] == {"num_parts": 5, "imbalance_percent": 0, "refine_rounds": 64}
    assert parse_subgraph_batches(_value({"num_parts": 8192, "imbalance_percent": 100, "refine_rounds": 0}))["partition"]["num_parts"] == 8192
    # a parsed dict without the key is the dict it was
    with_file = {"parts_path": "parts.npy", "parts_per_batch": 5, "sampler": "parts", "normalisation": NORM, "seed": 2}
    assert parse_subgraph_batches(with_file) == dict(with_file, normalisation=PARSED_NORM)
    walk = {"roots_per_batch": 32, "walk_length": 4, "seed": 1}
    assert parse_subgraph_batches(walk) == walk
    # it composes with its siblings
    parsed = _task(subgraph_batches=_value({"num_parts": 4}, data_parallel=True, sparse_features=True), sparse_node_features=True).subgraph_batches
    assert parsed["partition"]["num_parts"] == 4 and parsed["data_parallel"] is True and parsed["sparse_features"] is True


@pytest.mark.parametrize("bad, message", [
    (_value({"num_parts": 4}, parts_path="p.npy"), "exactly one of parts_path .* and partition"),
    ({"parts_per_batch": 2, "sampler": "parts", "normalisation": NORM}, '"sampler": "parts" requires parts_path'),
    ({"partition": {"num_parts": 4}, "sampler": "parts", "normalisation": NORM}, '"sampler": "parts" requires parts_per_batch'),
    ({"partition": {"num_parts": 4}, "parts_per_batch": 2, "sampler": "parts"}, '"sampler": "parts" requires the key "normalisation"'),
    ({"roots_per_batch": 32, "walk_length": 4, "partition": {"num_parts": 4}}, '"sampler": "walk" takes no partition'),
    ({"roots_per_batch": 8, "sampler": "node", "normalisation": NORM, "partition": {"num_parts": 4}}, '"sampler": "node" takes no partition'),
    ({"roots_per_batch": 8, "sampler": "edge", "normalisation": NORM, "partition": {"num_parts": 4}}, '"sampler": "edge" takes no partition'),
    (_value(8), "subgraph_batches: partition must be"),
    (_value([8]), "subgraph_batches: partition must be"),
    (_value({}), "subgraph_batches: partition: num_parts is required"),
    (_value({"imbalance_percent": 5}), "subgraph_batches: partition: num_parts is required"),
    (_value({"num_parts": 4, "seed": 1}), "subgraph_batches: partition: unknown key 'seed'"),
    (_value({"num_parts": 0}), "subgraph_batches: partition: num_parts must be an integer in"),
    (_value({"num_parts": True}), "subgraph_batches: partition: num_parts must be an integer in"),
    (_value({"num_parts": 4.0}), "subgraph_batches: partition: num_parts must be an integer in"),
    (_value({"num_parts": 8193}), r"subgraph_batches: partition: num_parts must be an integer in \[1, 8192\]"),
    (_value({"num_parts": 4, "imbalance_percent": 101}), r"subgraph_batches: partition: imbalance_percent must be an integer in \[0, 100\]"),
    (_value({"num_parts": 4, "imbalance_percent": -1}), "subgraph_batches: partition: imbalance_percent must be"),
    (_value({"num_parts": 4, "imbalance_percent": 2.5}), "subgraph_batches: partition: imbalance_percent must be"),
    (_value({"num_parts": 4, "refine_rounds": 65}), r"subgraph_batches: partition: refine_rounds must be an integer in \[0, 64\]"),
    (_value({"num_parts": 4, "refine_rounds": -1}), "subgraph_batches: partition: refine_rounds must be"),
    (_value({"num_parts": 4, "refine_rounds": False}), "subgraph_batches: partition: refine_rounds must be"),
])
def test_refusals(bad, message):
    with pytest.raises(ValueError, match=message):
        _task(subgraph_batches=bad)


def test_the_refusal_of_both_names_the_two_keys():
    with pytest.raises(ValueError) as refusal:
        _task(subgraph_batches=_value({"num_parts": 4}, parts_path="p.npy"))
    assert "parts_path" in str(refusal.value) and "partition" in str(refusal.value)


def test_the_key_travels_in_the_checkpoint_and_a_cpu_model_is_a_value_error(tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold
    value = _value({"num_parts": 6, "refine_rounds": 2}, seed=4)
    task = _task(subgraph_batches=value)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    parsed = task.subgraph_batches
    assert parsed["partition"] == {"num_parts": 6, "imbalance_percent": 10, "refine_rounds": 2}
    assert task.get_metadata()["params"]["subgraph_batches"] == value
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, random_seed=1)
    model = RGCN_Model(p, task, device="cpu")
    path = str(tmp_path / "model.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.subgraph_batches == parsed and restored.task.get_metadata() == task.get_metadata()
    assert "parts_path" not in restored.task.subgraph_batches                  # the key travels; no array, no file
    with pytest.raises(ValueError, match="partition is GPU only"):
        model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)


def test_the_plan_of_a_computed_partition_goes_through_the_files_validation():
    from tf_gnn_samples_amd.tasks.subgraph_sampling import load_parts, parse_subgraph_batches, sampler_plan, validated_parts
    V = 40
    parsed = parse_subgraph_batches(_value({"num_parts": 4}))
    mask, adjacency = np.ones(V, dtype=np.float32), [np.zeros((0, 2), dtype=np.int32)]
    good = (np.arange(V) % 4).astype(np.int32)
    plan = sampler_plan(parsed, mask, adjacency, V, partition=lambda: good)
    assert np.array_equal(plan.parts, good) and [n.tolist() for n in plan.part_nodes] == [list(range(p, V, 4)) for p in range(4)]
    assert plan.batches_per_epoch() == 2 and plan.longest() == 20
    with pytest.raises(ValueError, match="partition .* part 2 has no node"):
        sampler_plan(parsed, mask, adjacency, V, partition=lambda: np.where(good == 2, 3, good).astype(np.int32))
    with pytest.raises(ValueError, match="partition .* must hold an int32 array"):
        sampler_plan(parsed, mask, adjacency, V, partition=lambda: good.astype(np.int64))
    with pytest.raises(ValueError, match="subgraph_batches: partition"):                # the positional signature: no graph to compute it from
        sampler_plan(parsed, mask, adjacency, V)
    assert validated_parts(good, V, "x") is good and load_parts.__doc__


def test_anchors_and_cap():
    from tf_gnn_samples_amd.tasks.graph_partition import partition_anchors, partition_cap
    for V, P, seed in ((512, 8, 0), (300, 7, 2), (5, 5, 1), (9, 1, 2 ** 32 + 3)):
        anchors = partition_anchors(V, P, seed)
        assert anchors.dtype == np.int32 and np.array_equal(anchors, R.anchors_of(V, P, seed))
        assert len(np.unique(anchors)) == P and (np.diff(anchors) > 0).all() and 0 <= anchors[0] and anchors[-1] < V
    assert np.array_equal(partition_anchors(9, 3, 2 ** 32 + 3), partition_anchors(9, 3, 3))         # the seed's low 32 bits
    assert [partition_cap(512, 8, 10), partition_cap(512, 16, 10), partition_cap(300, 7, 10), partition_cap(6, 2, 0)] == [71, 36, 48, 3]
    assert all(partition_cap(V, P, b) == R.cap_of(V, P, b) for V, P, b in ((1000, 3, 7), (1, 1, 100), (8300, 8192, 0)))
    with pytest.raises(ValueError, match="num_parts"):
        partition_anchors(4, 5, 0)


# ---- the rule, on its restatement ---------------------------------------------------------------------------------------------------------
_GRAPHS = {}


def _planted(V, C, seed, L=1):
    if (V, C, seed, L) not in _GRAPHS:
        _GRAPHS[V, C, seed, L] = R.bucketing(R.planted_graph(V, C, seed, L), V)
    return _GRAPHS[V, C, seed, L]


_PARTS = {}


def _reference(V, C, P, seed, variant=(), b=10):
    key = (V, C, P, seed, tuple(variant), b)
    if key not in _PARTS:
        rowptr, col = _planted(V, C, seed)
        _PARTS[key] = R.partition(rowptr, col, 1, P, seed=seed, b=b, variant=variant)
    return _PARTS[key]


@pytest.mark.parametrize("V, C, P", PLANTED)
@pytest.mark.parametrize("seed", SEEDS)
def test_invariants_on_planted_graphs(V, C, P, seed):
    rowptr, col = _planted(V, C, seed)
    cap, anchors = R.cap_of(V, P, 10), R.anchors_of(V, P, seed)
    seen = []

    def after_round(phase, part):
        seen.append(phase)
        assert R.sizes_of(part, P).max() <= cap, phase                      # no part above cap after ANY round
        assert np.array_equal(part[anchors], np.arange(P)), phase           # the anchors keep their parts
    part = R.partition(rowptr, col, 1, P, seed=seed, after_round=after_round)
    assert seen.count("refine") == 8 and seen.count("fill") == 1 and seen.count("grow") >= 2
    assert part.dtype == np.int32 and part.min() == 0 and part.max() == P - 1
    sizes = np.bincount(part, minlength=P)
    assert sizes.min() >= 1 and sizes.max() <= cap
    assert np.array_equal(part, _reference(V, C, P, seed))                  # two runs, the same array
    assert not np.array_equal(part, R.partition(rowptr, col, 1, P, seed=seed + 10))     # another seed, another array


@pytest.mark.parametrize("V, C, P", PLANTED)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_partition_keeps_at_least_twice_the_entries_of_a_random_one(V, C, P, seed):
    rowptr, col = _planted(V, C, seed)
    kept, entries = R.kept_entries(rowptr, col, 1, _reference(V, C, P, seed))
    kept_random, entries_random = R.kept_entries(rowptr, col, 1, R.random_partition(V, P, seed))
    assert entries == entries_random > 0
    print("V %d C %d P %d seed %d: kept %.3f, random %.3f" % (V, C, P, seed, kept / entries, kept_random / entries))
    assert kept / entries >= 2 * kept_random / entries


def _path_graph(V=6):
    forward = np.stack([np.arange(V - 1), np.arange(1, V)], axis=1)
    return R.bucketing([np.concatenate([forward, forward[:, ::-1]]).astype(np.int32)], V)


def test_a_path_of_six_nodes_worked_by_hand():
    """The path 0 - 1 - 2 - 3 - 4 - 5, both directions stored, P = 2, seed 0.  RandomState([0, 4]).choice(6, 2) sorted is [0, 3]:
    part = [0 . . 1 . .] (a dot: unassigned).  Philox's low bits for seed 0: round 0 makes node 5 eligible, round 1 the nodes 1, 2, 4.

    b = 10, cap = ceil(6 * 110 / 200) = 4.
      grow 1: sizes (1, 1), room (3, 3).  1 sees {0, 2}: c(0) = 1, wishes 0.  2 sees {1, 3}: c(1) = 1, wishes 1.  4 sees {3, 5}: wishes
              1.  5 sees {4}: nothing.  Part 0 admits 1; part 1 admits 2 and 4 (room 3).      -> [0 0 1 1 1 .]
      grow 2: sizes (2, 3), room (2, 1).  5 sees {4}: c(1) = 1, room 1: wishes 1, admitted.     -> [0 0 1 1 1 1]
      grow 3: nobody is unassigned, nobody moves: the phase ends.  Fill: nobody is left.
      refine 0: sizes (2, 4), room (2, 0).  5 (part 1) sees {4}: only its own label.  Stays.
      refine 1: 1 (part 0) sees {0, 2}: c(0) = 1 = base, c(1) = 1 is not > base (and part 1 has no room).  2 (part 1) sees {1, 3}:
              c(0) = 1 is not > base = c(1) = 1.  4 (part 1) sees {3, 5}: its own label only.       -> [0 0 1 1 1 1]
    b = 0, cap = 3.
      grow 1: as above (room (2, 2): part 1 admits both 2 and 4)                                 -> [0 0 1 1 1 .]
      grow 2: sizes (2, 3), room (1, 0).  5 sees {4}: part 1 has no room, no wish.  Nobody moves: the phase ends.
      fill:   5 is leftover k = 0; cumsum(room) = (1, 1); searchsorted((1, 1), 0, "right") = 0     -> [0 0 1 1 1 0]
      refine 0: sizes (3, 3), room (0, 0): nobody can wish anything, here and in round 1."""
    rowptr, col = _path_graph()
    assert rowptr.tolist() == [0, 1, 3, 5, 7, 9, 10] and col.tolist() == [1, 0, 2, 1, 3, 2, 4, 3, 5, 4]
    assert R.anchors_of(6, 2, 0).tolist() == [0, 3]
    assert R.refine_eligible(6, 0, 0, [0, 3]).tolist() == [False, False, False, False, False, True]
    assert R.refine_eligible(6, 1, 0, [0, 3]).tolist() == [False, True, True, False, True, False]
    seen = []
    assert R.partition(rowptr, col, 1, 2, seed=0, b=10, T=2, after_round=lambda phase, part: seen.append((phase, part.tolist()))).tolist() \
        == [0, 0, 1, 1, 1, 1]
    assert seen == [("grow", [0, 0, 1, 1, 1, -1]), ("grow", [0, 0, 1, 1, 1, 1]), ("grow", [0, 0, 1, 1, 1, 1]), ("fill", [0, 0, 1, 1, 1, 1]),
                    ("refine", [0, 0, 1, 1, 1, 1]), ("refine", [0, 0, 1, 1, 1, 1])]
    seen = []
    assert R.partition(rowptr, col, 1, 2, seed=0, b=0, T=2, after_round=lambda phase, part: seen.append((phase, part.tolist()))).tolist() \
        == [0, 0, 1, 1, 1, 0]
    assert seen[:3] == [("grow", [0, 0, 1, 1, 1, -1]), ("grow", [0, 0, 1, 1, 1, -1]), ("fill", [0, 0, 1, 1, 1, 0])]


def test_one_round_by_hand_ties_rooms_self_entries_and_multiplicity():
    """Node 0 holds the entries [1, 1, 2, 0, 0, 0, 3, 4] (sources; L = 1): 1 twice, itself three times.  part = [0, 1, 1, 2, 2, -1],
    cap 3: c(1) = 3 (1 twice and 2), c(2) = 2, the three self entries count nowhere (else base would be 3).  Sizes (1, 2, 2), room
    (2, 1, 1): node 0 wishes 1.  Node 5 holds [3, 1]: c(2) = c(1) = 1, a tie: the lowest, 1.  Two nodes wish part 1 with room 1: the
    lower id, 0, moves and 5 stays unassigned.  With part 1 full (cap 2: room (1, 0, 0)) nobody can wish anything."""
    edges = np.array([[1, 0], [1, 0], [2, 0], [0, 0], [0, 0], [0, 0], [3, 0], [4, 0], [3, 5], [1, 5]], dtype=np.int32)
    rowptr, col = R.bucketing([edges], 6)
    part = np.array([0, 1, 1, 2, 2, -1], dtype=np.int32)
    everyone = np.ones(6, dtype=bool)
    wish = R.wishes(rowptr, col, 1, part, np.array([2, 1, 1]), everyone)
    assert wish.tolist() == [1, -1, -1, -1, -1, 1]
    new, moved = R.one_round(rowptr, col, 1, part, everyone, 3, 3)
    assert new.tolist() == [1, 1, 1, 2, 2, -1] and moved.tolist() == [True, False, False, False, False, False]
    assert R.wishes(rowptr, col, 1, part, np.array([1, 0, 0]), everyone).tolist() == [-1] * 6
    assert R.wishes(rowptr, col, 1, part, np.array([2, 0, 1]), everyone).tolist() == [2, -1, -1, -1, -1, 2]      # part 1 full: the next best
    only_five = np.arange(6) == 5
    assert R.wishes(rowptr, col, 1, part, np.array([2, 1, 1]), only_five).tolist() == [-1, -1, -1, -1, -1, 1]
    # the variants on this round
    assert R.wishes(rowptr, col, 1, part, np.array([2, 1, 1]), everyone, ("ties_highest",)).tolist() == [1, -1, -1, -1, -1, 2]
    assert R.wishes(rowptr, col, 1, part, np.array([2, 1, 1]), everyone, ("count_self",)).tolist() == [-1, -1, -1, -1, -1, 1]
    assert R.one_round(rowptr, col, 1, part, everyone, 3, 3, ("admit_descending",))[0].tolist() == [0, 1, 1, 2, 2, 1]


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_named_mistake_changes_the_result_on_a_test_graph(variant):
    """The planted graphs of the other tests (b = 10 and the tight b = 0): a GPU result that made one of these mistakes would differ
    from the reference on at least the graphs counted here."""
    differing = [(V, C, P, seed, b) for V, C, P in PLANTED for seed in SEEDS for b in (10, 0)
                 if not np.array_equal(_reference(V, C, P, seed, b=b), _reference(V, C, P, seed, (variant,), b=b))]
    print(variant, len(differing), "of", 2 * len(PLANTED) * len(SEEDS))
    assert differing


# ---- the package-internal header ----------------------------------------------------------------------------------------------------------
def _library():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    return _lib, _lib.load_library()


def test_the_internal_header_is_held_to_the_binding_and_the_library():
    _lib, lib = _library()
    table = _lib.INTERNAL["graph_partition.h"]
    names = declared_names(HEADER)
    assert names == sorted(declared_signatures(HEADER)) == sorted(table)
    assert {"relgnn_partition_supported", "relgnn_partition_wish"} <= set(names)
    declared = declared_signatures(HEADER)
    wrong = {n: (table[n], declared[n]) for n in declared if (table[n][0], list(table[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert not [n for n in names if not hasattr(raw, n)]
    for name, (restype, argtypes) in table.items():               # load_library() types this table too
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_no_internal_name_is_public_abi():
    _lib, _ = _library()
    internal = {n for table in _lib.INTERNAL.values() for n in table}
    assert internal and not internal & set(_lib.signatures())
    assert not any(internal & set(_lib.signatures(h)) for h in _lib.ABI)
    assert not [p.name for p in (HERE.parent / "include").iterdir() if "partition" in p.name]
    for p in (HERE.parent / "include").iterdir():
        assert "relgnn_partition" not in p.read_text(), p.name
    assert "not public ABI" in (HERE.parent / "INTEGRATION.md").read_text()


def test_the_host_checks_its_arguments_in_front_of_a_launch():
    _lib, lib = _library()
    supported = lib.relgnn_partition_supported
    assert supported(512, 1, 8, 10, 8) == 1 and supported(8300, 3, 8192, 0, 0) == 1 and supported(5, 2, 5, 100, 64) == 1
    assert supported(8300, 1, 8193, 10, 8) == 0 and supported(4, 1, 5, 10, 8) == 0 and supported(4, 1, 0, 10, 8) == 0
    assert supported(0, 1, 1, 10, 8) == 0 and supported(4, 0, 1, 10, 8) == 0 and supported(1 << 30, 2, 8, 10, 8) == 0
    assert supported(512, 1, 8, 101, 8) == 0 and supported(512, 1, 8, -1, 8) == 0
    assert supported(512, 1, 8, 10, 65) == 0 and supported(512, 1, 8, 10, -1) == 0
    assert lib.relgnn_partition_wave_row_max() == 64
    wish = lib.relgnn_partition_wish
    args = lambda V=300, L=3, M=10, P=8, refine=0, rnd=0, bound=0, classes=3: (None, None, V, L, M, None, None, P, None, refine, rnd, 0,
                                                                              None, None, bound, classes, None, None)
    assert wish(*args(V=0)) == _lib.OK                              # no node: no launch
    assert wish(*args(V=-1)) == _lib.EINVAL and wish(*args(M=-1)) == _lib.EINVAL
    assert wish(*args(bound=301)) == _lib.EINVAL and wish(*args(bound=-1)) == _lib.EINVAL
    assert wish(*args(classes=0)) == _lib.EINVAL and wish(*args(classes=4)) == _lib.EINVAL
    assert wish(*args(P=8193)) == _lib.EUNSUPPORTED and wish(*args(P=0)) == _lib.EUNSUPPORTED and wish(*args(P=301)) == _lib.EUNSUPPORTED
    assert wish(*args(V=1 << 30, L=2)) == _lib.EUNSUPPORTED and wish(*args(M=1 << 31)) == _lib.EUNSUPPORTED
    assert wish(*args(refine=1, rnd=65)) == _lib.EUNSUPPORTED
    assert wish(*args()) == _lib.EINVAL                             # null pointers


def test_partition_graph_is_gpu_only_and_checks_before_it_launches():
    import torch
    from tf_gnn_samples_amd.tasks.graph_partition import partition_graph

    class HostGraph:
        device, V, L, M = torch.device("cpu"), 10, 1, 0
    with pytest.raises(ValueError, match="GPU only"):
        partition_graph(HostGraph(), 2)
