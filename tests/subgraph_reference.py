"""NumPy restatement of the rules of include/relgnn_subgraph.h over tests/philox_reference.py: the random walks and the node-induced
subgraph.  A helper, not a test: tests/test_subgraph_batches_cpu.py checks its properties (and that it notices plausible mistakes),
the GPU tests hold the kernels to it bit for bit.  Nothing here touches the GPU or the package under test.

    walk_nodes(rowptr_t, col_t, V, L, roots, h, draw, seed, replica)  -> the visited nodes, ascending
    induced(rowptr_t, col_t, V, L, nodes)                             -> Induced(nodes, adjacency_lists, degrees, seed_mask)
    sample(...)                                                       -> induced(walk_nodes(...))

`mistake` switches ONE deliberate error on (the CPU tests show that the comparison they make notices each): "drop_edge",
"source_order", "full_degrees" for induced(), "out_edges", "modulo" for walk_nodes().
"""
import sys
from pathlib import Path
from typing import List, NamedTuple

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

from neighbour_sampling_reference import bucketing  # noqa: E402,F401  (the by-target bucketing of graph.RelGraph)
from philox_reference import philox4x32_10  # noqa: E402

MAX_WALK_LENGTH = 64


class Induced(NamedTuple):
    nodes: np.ndarray                       # int32 [n], ascending global ids
    adjacency_lists: List[np.ndarray]       # per type int32 [E_l, 2] = (source, target) in local ids
    degrees: np.ndarray                     # float32 [L, n], the induced in-degrees
    seed_mask: np.ndarray                   # float32 [n], ones


def walk_words(num_walks: int, step: int, draw: int, seed: int, replica: int) -> np.ndarray:
    """Output word 0 of Philox4x32-10 with counter (w, step, draw, 0), key (seed, replica), for w in [0, num_walks)."""
    w = np.arange(num_walks, dtype=np.uint64)
    return philox4x32_10((w, int(step), int(draw) & 0xffffffff, 0), (int(seed) & 0xffffffff, int(replica)))[0]


def walk_nodes(rowptr_t, col_t, num_nodes: int, num_edge_types: int, roots, walk_length: int, draw: int, seed: int = 0,
               replica: int = 0, mistake: str = "") -> np.ndarray:
    V, L, h = int(num_nodes), int(num_edge_types), int(walk_length)
    rowptr_t, col_t = np.asarray(rowptr_t, np.int64), np.asarray(col_t, np.int64)
    roots = np.asarray(roots, np.int64)
    assert len(roots) >= 1 and roots.min() >= 0 and roots.max() < V and 0 <= h <= MAX_WALK_LENGTH and V * L < 2 ** 31
    if mistake == "out_edges":                          # the by-SOURCE bucketing: the walk follows the edges instead
        tgt = np.repeat(np.arange(V * L) // L, np.diff(rowptr_t))
        order = np.argsort(col_t // L, kind="stable")
        begin = np.zeros(V + 1, np.int64)
        np.cumsum(np.bincount(col_t // L, minlength=V), out=begin[1:])
        end, neighbour = begin[1:], tgt[order]
    else:
        begin, end, neighbour = rowptr_t[np.arange(V) * L], rowptr_t[(np.arange(V) + 1) * L], col_t // L
    at = roots.copy()
    visited = np.zeros(V, bool)
    visited[at] = True
    for step in range(h if len(neighbour) else 0):              # (an edge-free graph: every walk stays)
        b, deg = begin[at], end[at] - begin[at]
        word = walk_words(len(roots), step, draw, seed, replica).astype(np.uint64)
        if mistake == "modulo":
            j = (word % np.maximum(deg, 1).astype(np.uint64)).astype(np.int64)
        else:
            j = ((word * deg.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)       # 32 x 32 -> 64: no overflow in uint64
        moves = deg > 0
        at = np.where(moves, neighbour[np.where(moves, b + j, 0)], at)
        visited[at] = True
    return np.flatnonzero(visited).astype(np.int32)


def induced(rowptr_t, col_t, num_nodes: int, num_edge_types: int, nodes, mistake: str = "") -> Induced:
    """Every type's list filtered by membership of both ends, ordered by (target, position in the full graph's bucket), relabelled by
    rank in the ascending node list."""
    V, L = int(num_nodes), int(num_edge_types)
    rowptr_t, col_t = np.asarray(rowptr_t, np.int64), np.asarray(col_t, np.int64)
    nodes = np.unique(np.asarray(nodes, np.int64))
    member = np.zeros(V, bool)
    member[nodes] = True
    local = np.full(V, -1, np.int64)
    local[nodes] = np.arange(len(nodes))
    row = np.repeat(np.arange(V * L), np.diff(rowptr_t))         # by-target position -> its (target, type) row
    target, typ, source = row // L, row % L, col_t // L
    keep = member[target] & member[source]
    adjacency, degrees = [], np.zeros((L, len(nodes)), np.float32)
    for l in range(L):
        at = np.flatnonzero(keep & (typ == l))                   # ascending position = (target, position in the bucket)
        if mistake == "drop_edge" and len(at):
            at = at[:-1]
        if mistake == "source_order":
            at = at[np.lexsort((source[at], target[at]))]
        adjacency.append(np.stack([local[source[at]], local[target[at]]], axis=1).astype(np.int32).reshape(-1, 2))
        if mistake == "full_degrees":
            degrees[l] = (rowptr_t[nodes * L + l + 1] - rowptr_t[nodes * L + l]).astype(np.float32)
        else:
            degrees[l] = np.bincount(local[target[at]], minlength=len(nodes)).astype(np.float32)
    return Induced(nodes.astype(np.int32), adjacency, degrees, np.ones(len(nodes), np.float32))


def sample(rowptr_t, col_t, num_nodes: int, num_edge_types: int, roots, walk_length: int, draw: int, seed: int = 0,
           replica: int = 0) -> Induced:
    return induced(rowptr_t, col_t, num_nodes, num_edge_types,
                   walk_nodes(rowptr_t, col_t, num_nodes, num_edge_types, roots, walk_length, draw, seed, replica))


def brute_force(adjacency_lists, num_nodes: int, nodes) -> Induced:
    """The induced subgraph straight from the edge lists, without the bucketing: per type the edges with both ends in the set, stably
    sorted by target (the order of a by-target bucket is the list's own order), relabelled by rank."""
    nodes = np.unique(np.asarray(nodes, np.int64))
    rank = {int(v): i for i, v in enumerate(nodes)}
    adjacency, degrees = [], np.zeros((len(adjacency_lists), len(nodes)), np.float32)
    for l, edges in enumerate(adjacency_lists):
        kept = [(rank[int(s)], rank[int(t)]) for s, t in np.asarray(edges).reshape(-1, 2) if int(s) in rank and int(t) in rank]
        kept.sort(key=lambda st: st[1])                          # (stable)
        adjacency.append(np.asarray(kept, np.int32).reshape(-1, 2))
        for _, t in kept:
            degrees[l, t] += 1
    return Induced(nodes.astype(np.int32), adjacency, degrees, np.ones(len(nodes), np.float32))
