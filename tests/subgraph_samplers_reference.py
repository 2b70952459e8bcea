"""NumPy restatement of the four node-set samplers of `subgraph_batches` (the key "sampler") on top of tests/subgraph_reference.py and
tests/subgraph_norm_reference.py: the lists of an epoch and the node set each list stands for.  A helper, not a test:
tests/test_subgraph_samplers_cpu.py checks its properties (and that they notice plausible mistakes) and holds the package's host plan to
it, the GPU tests hold the batches to it bit for bit.  Nothing here touches the GPU or the package under test.

    node_draws(rowptr_t, V, L, R, seed, epoch, j)         -> the R drawn nodes of batch j, before they are made distinct
    edge_roots(V, R, seed, epoch, j)                      -> the root list of batch j
    part_lists(parts, q, seed, epoch)                     -> the node sets of an epoch of partition batches
    epoch_lists(sampler, graph, per_batch, seed, epoch)   -> the epoch's lists, int32 ascending distinct
    node_set(sampler, graph, ids, draw, seed, replica)    -> the node set a list stands for (a walk for "walk" and "edge")
    presampled_node_sets(sampler, graph, per_batch, seed, E, h) -> the sets of E pre-sampling epochs, in draw order

The rules: "node" draws R positions among the M by-target entries, RandomState([seed, epoch, j, 1]).randint(0, M, R, int64), and takes each
entry's TARGET, a node in proportion to its in-degree; "edge" draws R roots, RandomState([seed, epoch, j, 2]).randint(0, V, R), and walks ONE
step from each distinct root: entry (u <- v) is taken with probability 1 / (V deg u); "parts" cuts RandomState([seed, epoch, 3]).permutation(P)
into runs of q parts.  "node" and "edge" have ceil(n_train / R) batches an epoch, "parts" ceil(P / q).

`mistake` switches ONE deliberate error on: "uniform_nodes" for node_draws(), "uniform_entry" for edge_pair().
"""
import sys
from pathlib import Path
from typing import List, NamedTuple

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import subgraph_norm_reference as N  # noqa: E402
import subgraph_reference as S  # noqa: E402

SAMPLERS = ("walk", "node", "edge", "parts")
PRESAMPLE_REPLICA, PRESAMPLE_EPOCH = N.PRESAMPLE_REPLICA, N.PRESAMPLE_EPOCH


class Graph(NamedTuple):
    adjacency: List[np.ndarray]             # per type int32 [E_l, 2]
    rowptr_t: np.ndarray                    # S.bucketing's
    col_t: np.ndarray
    num_nodes: int
    num_edge_types: int
    mask: np.ndarray                        # float32 [V], the TRAIN fold
    parts: np.ndarray                       # int32 [V], values 0 .. P - 1


# ---- the test graphs (V = 300; L = 2 and 3), shared by the CPU and the GPU tests ------------------------------------------------------
V, P = 300, 12
HUB, HUB_ENTRIES = 4, 5000                  # target 4's type-0 bucket: far more than a wave and than the 4 096 at which a bucket is split
ISOLATED = 299                              # no edge of any type, in either direction
NUM_TRAIN = 100
_GRAPHS = {}


def sampler_graph(L: int) -> Graph:
    """Type 0: 0 .. 8 entries per target and HUB_ENTRIES at HUB, random sources (300 nodes in 5 000 draws: many duplicate edges);
    type 1: 900 random edges, the first 60 of them twice; type 2 (L = 3): a self loop per node.  ISOLATED is in none of them.  The TRAIN
    fold: 100 random nodes, HUB and ISOLATED among them.  The partition: 12 parts of 25 random nodes."""
    if L not in _GRAPHS:
        rng = np.random.default_rng(40 + L)
        others = V - 1
        lengths = rng.integers(0, 9, size=others)
        lengths[HUB] = HUB_ENTRIES
        tgt = np.repeat(np.arange(others), lengths)
        adjacency = [np.stack([rng.integers(0, others, size=len(tgt)), tgt], axis=1)]
        random_edges = rng.integers(0, others, size=(900, 2))
        adjacency.append(np.concatenate([random_edges, random_edges[:60]]))
        if L == 3:
            adjacency.append(np.stack([np.arange(others), np.arange(others)], axis=1))
        adjacency = [np.ascontiguousarray(e[rng.permutation(len(e))], dtype=np.int32) for e in adjacency[:L]]
        assert not any((e == ISOLATED).any() for e in adjacency)
        mask = np.zeros(V, np.float32)
        rest = np.setdiff1d(np.arange(V), [HUB, ISOLATED])
        mask[np.concatenate([[HUB, ISOLATED], rng.choice(rest, size=NUM_TRAIN - 2, replace=False)])] = 1.0
        parts = (rng.permutation(V) % P).astype(np.int32)
        rowptr_t, col_t, _ = S.bucketing(adjacency, V)
        _GRAPHS[L] = Graph(adjacency, rowptr_t, col_t, V, L, mask, parts)
    return _GRAPHS[L]


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def _rng(*words):
    return np.random.RandomState([int(w) & 0xffffffff for w in words])


def node_draws(rowptr_t, num_nodes: int, num_edge_types: int, per_batch: int, seed: int, epoch: int, j: int, mistake: str = "") -> np.ndarray:
    """R positions among the by-target entries, each mapped to the target whose bucket holds it."""
    rowptr_t = np.asarray(rowptr_t, np.int64)
    M = int(rowptr_t[-1])
    at = _rng(seed, epoch, j, 1).randint(0, M, size=int(per_batch), dtype=np.int64)
    if mistake == "uniform_nodes":
        return _rng(seed, epoch, j, 1).randint(0, int(num_nodes), size=int(per_batch))
    row = np.searchsorted(rowptr_t, at, side="right") - 1         # the last (target, type) row that starts at or before the position
    return row // int(num_edge_types)


def edge_roots(num_nodes: int, per_batch: int, seed: int, epoch: int, j: int) -> np.ndarray:
    return np.unique(_rng(seed, epoch, j, 2).randint(0, int(num_nodes), size=int(per_batch))).astype(np.int32)


def edge_pair(rowptr_t, col_t, num_nodes: int, num_edge_types: int, seed: int, epoch: int, j: int, mistake: str = ""):
    """The edge rule with R = 1: batch j's one root and where its one step leads, as an unordered pair (a root without an in-edge stays:
    (u, u)).  "uniform_entry": a uniformly drawn by-target entry instead (every stored entry alike: proportional to 1)."""
    if mistake == "uniform_entry":
        rowptr = np.asarray(rowptr_t, np.int64)
        at = int(_rng(seed, epoch, j, 2).randint(0, int(rowptr[-1])))
        u = (int(np.searchsorted(rowptr, at, side="right")) - 1) // int(num_edge_types)
        return tuple(sorted((u, int(col_t[at]) // int(num_edge_types))))
    (u,) = edge_roots(num_nodes, 1, seed, epoch, j)
    nodes = S.walk_nodes(rowptr_t, col_t, num_nodes, num_edge_types, [u], 1, j, seed)
    return (int(nodes[0]), int(nodes[-1]))


def part_lists(parts, per_batch: int, seed: int, epoch: int) -> List[np.ndarray]:
    parts = np.asarray(parts)
    order = _rng(seed, epoch, 3).permutation(int(parts.max()) + 1)
    return [np.flatnonzero(np.isin(parts, order[i:i + per_batch])).astype(np.int32) for i in range(0, len(order), int(per_batch))]


def batches_per_epoch(sampler: str, graph: Graph, per_batch: int) -> int:
    items = int(graph.parts.max()) + 1 if sampler == "parts" else int(np.count_nonzero(graph.mask))
    return -(-items // int(per_batch))


def epoch_lists(sampler: str, graph: Graph, per_batch: int, seed: int, epoch: int) -> List[np.ndarray]:
    if sampler == "walk":
        return N.seed_batches(graph.mask, per_batch, seed, epoch)
    if sampler == "parts":
        return part_lists(graph.parts, per_batch, seed, epoch)
    count = batches_per_epoch(sampler, graph, per_batch)
    if sampler == "node":
        return [np.unique(node_draws(graph.rowptr_t, graph.num_nodes, graph.num_edge_types, per_batch, seed, epoch, j)).astype(np.int32)
                for j in range(count)]
    return [edge_roots(graph.num_nodes, per_batch, seed, epoch, j) for j in range(count)]


def node_set(sampler: str, graph: Graph, ids, draw: int, seed: int, replica: int = 0, walk_length: int = 0) -> np.ndarray:
    """"walk": walk_length steps from every id; "edge": one step; "node" and "parts": the list is the set."""
    if sampler in ("walk", "edge"):
        steps = walk_length if sampler == "walk" else 1
        return S.walk_nodes(graph.rowptr_t, graph.col_t, graph.num_nodes, graph.num_edge_types, ids, steps, draw, seed, replica)
    return np.unique(np.asarray(ids)).astype(np.int32)


def presampled_node_sets(sampler: str, graph: Graph, per_batch: int, seed: int, epochs: int, walk_length: int = 0) -> List[np.ndarray]:
    """Epochs 0x80000000 + e of the sampler's lists, each with replica 0x20000000 and draw = the running index."""
    sets = []
    for e in range(int(epochs)):
        for ids in epoch_lists(sampler, graph, per_batch, seed, PRESAMPLE_EPOCH + e):
            sets.append(node_set(sampler, graph, ids, len(sets), seed, PRESAMPLE_REPLICA, walk_length))
    return sets


# ---- the 12-node graph of the distribution checks -------------------------------------------------------------------------------------
DEGREES = [8, 7, 6, 5, 4, 3, 2, 1, 4, 3, 2, 1]


def small_undirected_graph():
    """12 nodes with DEGREES (Havel-Hakimi: the node with the most stubs left is joined to the next most), simple, stored in both
    directions as one edge type.  -> (adjacency [46, 2], rowptr_t, col_t, the 23 pairs)."""
    left, pairs = list(DEGREES), []
    while any(left):
        order = sorted(range(len(left)), key=lambda v: (-left[v], v))
        u, take = order[0], left[order[0]]
        for v in order[1:1 + take]:
            assert left[v] > 0
            pairs.append((min(u, v), max(u, v)))
            left[v] -= 1
        left[u] = 0
    assert len(set(pairs)) == len(pairs) == sum(DEGREES) // 2
    edges = np.asarray(pairs + [(b, a) for a, b in pairs], np.int32)
    assert np.array_equal(np.bincount(edges[:, 1], minlength=len(DEGREES)), DEGREES)
    rowptr_t, col_t, _ = S.bucketing([edges], len(DEGREES))
    return [edges], rowptr_t, col_t, sorted(pairs)
