"""NumPy statement of the block of a window of target rows (tf_gnn_samples_amd/csrc/window_block.h; tasks/layerwise.py), from adjacency
lists, and a brute-force statement of the same that loops over edges; the graphs the GPU tests cut windows from.

The block of [a, b): nodes = a .. b - 1, then every source outside [a, b) of an edge whose target is inside, ascending; per edge type
the (source, target) pairs in local ids, ascending target and, under one target, in the order of the type's list (what the stable sort
of the by-target bucketing leaves: "the bucket's own order"), duplicates kept; degrees float32 [L, n] = the in-degrees of the targets by
type, 0 behind them."""
from typing import List, NamedTuple

import numpy as np


class Block(NamedTuple):
    nodes: np.ndarray                           # int32 [n]
    adjacency_lists: List[np.ndarray]           # per type int32 [E_l, 2] in local ids
    degrees: np.ndarray                         # float32 [L, n]
    sizes: tuple                                # (E_0, ..., E_{L-1}, n - T)


def target_windows(num_nodes, rows_per_batch):
    return [(a, min(a + rows_per_batch, num_nodes)) for a in range(0, num_nodes, rows_per_batch)]


def window_block(adjacency, num_nodes, a, b) -> Block:
    """Vectorised: a stable sort by target of every type's edges inside the window."""
    assert 0 <= a < b <= num_nodes
    T = b - a
    kept = []
    for edges in adjacency:
        edges = np.asarray(edges).reshape(-1, 2)
        inside = edges[(edges[:, 1] >= a) & (edges[:, 1] < b)]
        kept.append(inside[np.argsort(inside[:, 1], kind="stable")])
    sources = np.concatenate([k[:, 0] for k in kept]) if kept else np.zeros(0, np.int64)
    outside = np.unique(sources[(sources < a) | (sources >= b)])
    nodes = np.concatenate([np.arange(a, b), outside]).astype(np.int32)
    n = len(nodes)
    lists, degrees = [], np.zeros((len(adjacency), n), dtype=np.float32)
    for l, k in enumerate(kept):
        src, tgt = k[:, 0], k[:, 1]
        local = np.where((src >= a) & (src < b), src - a, T + np.searchsorted(outside, src))
        lists.append(np.stack([local, tgt - a], axis=1).astype(np.int32).reshape(-1, 2))
        degrees[l, :T] = np.bincount(tgt - a, minlength=T)
    return Block(nodes, lists, degrees, tuple(len(k) for k in kept) + (n - T,))


def window_block_brute_force(adjacency, num_nodes, a, b) -> Block:
    """Loops over targets and edges; shares no line with window_block."""
    T = b - a
    outside = set()
    for edges in adjacency:
        for s, t in np.asarray(edges).reshape(-1, 2).tolist():
            if a <= t < b and not a <= s < b:
                outside.add(s)
    listed = sorted(outside)
    local_of = {v: i for i, v in enumerate(list(range(a, b)) + listed)}
    n = T + len(listed)
    lists, degrees = [], np.zeros((len(adjacency), n), dtype=np.float32)
    for l, edges in enumerate(adjacency):
        pairs = np.asarray(edges).reshape(-1, 2).tolist()
        out = []
        for target in range(a, b):
            for s, t in pairs:
                if t == target:
                    out.append((local_of[s], target - a))
                    degrees[l, target - a] += 1
        lists.append(np.asarray(out, dtype=np.int32).reshape(-1, 2))
    return Block(np.asarray(list(range(a, b)) + listed, dtype=np.int32), lists, degrees, tuple(len(x) for x in lists) + (len(listed),))


def same_block(x: Block, y: Block) -> bool:
    return (np.array_equal(x.nodes, y.nodes) and x.nodes.dtype == y.nodes.dtype and len(x.adjacency_lists) == len(y.adjacency_lists)
            and all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(x.adjacency_lists, y.adjacency_lists))
            and x.degrees.shape == y.degrees.shape and np.array_equal(x.degrees.view(np.uint32), y.degrees.view(np.uint32))
            and tuple(x.sizes) == tuple(y.sizes))


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------
HUB_V = 300
HUB = 16
HUB_BUCKETS = {10: 0, 11: 1, 12: 63, 13: 64, 14: 65, 15: 129, HUB: 5000}       # node -> entries of its (node, type 1) bucket
_HUB_GRAPHS = {}


def hub_graph(L):
    """The hub graph of the sampled-evaluation tests, restated: V = 300; type 0 one self loop per node; type 1 buckets of 0, 1, 63, 64, 65,
    129 and 5 000 entries at nodes 10 .. 16, three at every other node, random sources (duplicates and self loops included), the list
    shuffled; type 2 (L = 3) 150 random edges, so most of its buckets are empty.  -> (adjacency, degrees int32 [L, V])."""
    if L not in _HUB_GRAPHS:
        V = HUB_V
        rng = np.random.default_rng(L)
        nodes = np.arange(V)
        counts = np.full(V, 3)
        for node, n in HUB_BUCKETS.items():
            counts[node] = n
        tgt = np.repeat(nodes, counts)
        src = rng.integers(0, V, size=len(tgt))
        src[np.flatnonzero(tgt == 11)[0]] = HUB
        src[np.flatnonzero(tgt == 12)[0]] = 17
        edges = np.stack([src, tgt], axis=1)[rng.permutation(len(tgt))]
        adjacency = [np.stack([nodes, nodes], axis=1).astype(np.int32), np.ascontiguousarray(edges, dtype=np.int32)]
        if L == 3:
            adjacency.append(np.ascontiguousarray(rng.integers(0, V, size=(150, 2)), dtype=np.int32))
        degrees = np.stack([np.bincount(a[:, 1], minlength=V) for a in adjacency]).astype(np.int32)
        _HUB_GRAPHS[L] = (adjacency, degrees)
    return _HUB_GRAPHS[L]


EDGE_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)      # the tile (1 024) and wave (64) edges of the flat passes


def tile_edge_graph(L=3, rows_per_window=8, seed=11):
    """A graph whose window i = [8 i, 8 i + 8) holds exactly EDGE_COUNTS[i] entries, spread unevenly over its targets and the types
    0 .. L - 2 (a target may hold most of a window's entries); then one window whose every entry has type L - 1 (37 of them), and a
    last window of 5 entries.  Sources are random over all nodes; node V - 1 is a source of the first non-empty window and of the last.
    -> (adjacency, V, [(window, its entry count)])."""
    rng = np.random.default_rng(seed)
    counts = list(EDGE_COUNTS) + [37, 5]
    V = rows_per_window * len(counts)
    lists = [[] for _ in range(L)]
    windows = []
    for i, count in enumerate(counts):
        a, b = rows_per_window * i, rows_per_window * (i + 1)
        windows.append(((a, b), count))
        if count == 0:
            continue
        weights = rng.random(rows_per_window) ** 4
        targets = rng.choice(np.arange(a, b), size=count, p=weights / weights.sum())
        sources = rng.integers(0, V, size=count)
        if i in (1, len(counts) - 1):
            sources[0] = V - 1
        types = np.full(count, L - 1) if i == len(EDGE_COUNTS) else rng.integers(0, max(L - 1, 1), size=count)
        for s, t, l in zip(sources.tolist(), targets.tolist(), types.tolist()):
            lists[l].append((s, t))
    adjacency = []
    for pairs in lists:
        edges = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        adjacency.append(np.ascontiguousarray(edges[rng.permutation(len(edges))]))
    return adjacency, V, windows


def banded_graph(num_nodes, L=3, offsets=(1, 2, 5)):
    """source = target +- offsets[l] (mod V is NOT taken: the ends of the band have fewer edges), type l: a window's sources are its
    targets and at most 2 max(offsets) more.  -> (adjacency, degrees int32 [L, V])."""
    nodes = np.arange(num_nodes)
    adjacency = []
    for l in range(L):
        d = offsets[l]
        pairs = np.concatenate([np.stack([nodes[d:], nodes[:-d]], axis=1), np.stack([nodes[:-d], nodes[d:]], axis=1)])
        adjacency.append(np.ascontiguousarray(pairs, dtype=np.int32))
    degrees = np.stack([np.bincount(a[:, 1], minlength=num_nodes) for a in adjacency]).astype(np.int32)
    return adjacency, degrees
