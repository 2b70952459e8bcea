"""NumPy restatement of the neighbour-sampling rule of include/relgnn_sampling.h over tests/philox_reference.py.  A helper, not a
test: tests/test_neighbour_sampling_cpu.py checks its properties, the GPU tests hold the kernels to it bit for bit.  Nothing here
touches the GPU or the package under test.

    bucketing(adjacency_lists, V)                      -> (rowptr_t, col_t, perm_t) as a RelGraph holds them
    take(deg, k, row, hop, draw, seed, replica)        -> the positions taken from one bucket, ascending
    sample(rowptr_t, col_t, V, L, seeds, fanouts, ...) -> Sample(nodes, adjacency_lists, degrees, seed_mask, ...)
"""
import sys
from pathlib import Path
from typing import List, NamedTuple

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

from philox_reference import philox4x32_10  # noqa: E402

MAX_FANOUT, MAX_HOPS = 64, 8


class Sample(NamedTuple):
    nodes: np.ndarray                       # int32 [n], ascending global ids
    adjacency_lists: List[np.ndarray]       # per type int32 [E_l, 2] = (source, target) in local ids
    degrees: np.ndarray                     # float32 [L, n], the sampled in-degrees
    seed_mask: np.ndarray                   # float32 [n]
    positions: List[np.ndarray]             # per type int64 [E_l]: the by-target position (index into col_t) of every edge
    frontiers: List[np.ndarray]             # the frontier of every hop (global ids, ascending)


def bucketing(adjacency_lists, num_nodes: int):
    """The by-target bucketing of graph.RelGraph: messages type-major, stably sorted by (target, type)."""
    L = len(adjacency_lists)
    src = np.concatenate([np.asarray(a, np.int64).reshape(-1, 2)[:, 0] for a in adjacency_lists])
    tgt = np.concatenate([np.asarray(a, np.int64).reshape(-1, 2)[:, 1] for a in adjacency_lists])
    typ = np.concatenate([np.full(len(np.asarray(a).reshape(-1, 2)), l, np.int64) for l, a in enumerate(adjacency_lists)])
    key = tgt * L + typ
    perm = np.argsort(key, kind="stable")
    rowptr = np.zeros(num_nodes * L + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=num_nodes * L), out=rowptr[1:])
    return rowptr.astype(np.int32), (src * L + typ)[perm].astype(np.int32), perm.astype(np.int32)


def words(deg: int, row: int, hop: int, draw: int, seed: int, replica: int) -> np.ndarray:
    """word_j for j in [0, deg): output word j % 4 of Philox4x32-10, counter (j // 4, row, hop, draw), key (seed, 0x80000000 | replica)."""
    j = np.arange(deg, dtype=np.uint64)
    out = philox4x32_10((j >> np.uint64(2), row, hop, int(draw) & 0xffffffff), (int(seed) & 0xffffffff, 0x80000000 | int(replica)))
    return np.choose((j & np.uint64(3)).astype(np.int64), [np.broadcast_to(w, j.shape) for w in out])


def take(deg: int, k: int, row: int, hop: int, draw: int, seed: int, replica: int) -> np.ndarray:
    if k == 0 or deg <= k:
        return np.arange(deg, dtype=np.int64)
    w = words(deg, row, hop, draw, seed, replica)
    order = np.lexsort((np.arange(deg), w))             # by (word, j)
    return np.sort(order[:k]).astype(np.int64)


def sample(rowptr_t, col_t, num_nodes: int, num_edge_types: int, seeds, fanouts, draw: int, seed: int = 0, replica: int = 0) -> Sample:
    V, L = int(num_nodes), int(num_edge_types)
    rowptr_t, col_t = np.asarray(rowptr_t, np.int64), np.asarray(col_t, np.int64)
    seeds = np.asarray(seeds, np.int64)
    assert len(np.unique(seeds)) == len(seeds) and (len(seeds) == 0 or (seeds.min() >= 0 and seeds.max() < V))
    assert 1 <= len(fanouts) <= MAX_HOPS and all(0 <= k <= MAX_FANOUT for k in fanouts) and V * L < 2 ** 31
    stamp = np.zeros(V, np.int32)
    stamp[seeds] = -1
    frontier = np.sort(seeds)
    frontiers, hops = [], []                            # hops: per hop and type (sources, targets, positions, counts per frontier node)
    for h, k in enumerate(fanouts):
        frontiers.append(frontier)
        per_type = []
        for l in range(L):
            src, tgt, pos, cnt = [], [], [], []
            for t in frontier:
                b, e = rowptr_t[t * L + l], rowptr_t[t * L + l + 1]
                js = take(int(e - b), k, int(t * L + l), h, draw, seed, replica)
                cnt.append(len(js))
                pos.extend(b + js)
                src.extend(col_t[b + js] // L)
                tgt.extend([t] * len(js))
            per_type.append((np.asarray(src, np.int64), np.asarray(tgt, np.int64), np.asarray(pos, np.int64), np.asarray(cnt, np.int64)))
        hops.append(per_type)
        new = np.unique(np.concatenate([p[0] for p in per_type])) if L else np.zeros(0, np.int64)
        new = new[stamp[new] == 0]
        stamp[new] = h + 1
        frontier = new                                   # ascending (np.unique sorts)
    nodes = np.flatnonzero(stamp != 0)
    local = np.full(V, -1, np.int64)
    local[nodes] = np.arange(len(nodes))
    degrees = np.zeros((L, len(nodes)), np.float32)
    adjacency, positions = [], []
    for l in range(L):
        parts, where = [], []
        for h in range(len(fanouts)):
            src, tgt, pos, cnt = hops[h][l]
            parts.append(np.stack([local[src], local[tgt]], axis=1).reshape(-1, 2))
            where.append(pos)
            degrees[l, local[frontiers[h]]] = cnt
        adjacency.append(np.concatenate(parts).astype(np.int32).reshape(-1, 2))
        positions.append(np.concatenate(where))
    return Sample(nodes.astype(np.int32), adjacency, degrees, (stamp[nodes] == -1).astype(np.float32), positions, frontiers)
