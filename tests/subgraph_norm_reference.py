"""NumPy restatement of the rules of include/relgnn_subgraph_norm.h on top of tests/subgraph_reference.py: GraphSAINT's visit counts
over pre-sampled subgraphs, the float32 per-edge and per-node weights, and the weighted masked softmax cross-entropy with its gradient in
float64.  A helper, not a test: tests/test_subgraph_norm_cpu.py checks its identities (and that they notice plausible mistakes), the GPU
tests hold the kernels to it.  Nothing here touches the GPU or the package under test.

    seed_batches(fold_mask, R, seed, epoch)                          -> the root lists of one epoch (the task's epoch_seed_batches)
    presampled_node_sets(rowptr_t, col_t, V, L, fold_mask, R, h, seed, E) -> the N = E * ceil(n / R) node sets, in draw order
    visit_counts(rowptr_t, col_t, V, L, node_sets)                   -> (node_visits int32 [V], edge_visits int32 [M])
    kept_positions(rowptr_t, col_t, V, L, nodes)                     -> per type the by-target positions of the induced list's entries
    edge_weights(rowptr_t, col_t, V, L, nodes, node_visits, edge_visits, cap) -> float32 [edges], the lists one behind the other
    node_weights(node_visits, nodes, N)                              -> float32 [n]
    weighted_stats / weighted_gradient                               -> float64

`mistake` switches ONE deliberate error on: "induced_degree" and "inverted" for edge_weights(), "from_edge_visits" for node_weights().
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import subgraph_reference as S  # noqa: E402

PRESAMPLE_REPLICA = 0x20000000
PRESAMPLE_EPOCH = 0x80000000


# ---- the two test graphs (V = 300, L = 3), shared by the CPU and the GPU tests ------------------------------------------------------------
V, L = 300, 3
# (target, type 0) buckets of these lengths at targets 0, 1, 2, ...: empty, one entry, the wave width and its neighbours, eight passes
# of 64 entries (the loads a wave issues together) and one more, and a hub far longer than that
LENGTHS = [0, 1, 63, 64, 65, 512, 513, 5000]
HUB = LENGTHS.index(5000)
NO_IN_EDGE = [290, 291, 292, 293, 294]
_GRAPHS = {}


def norm_graph(which: str):
    """-> (adjacency lists int32 [E_l, 2], (rowptr_t, col_t, perm_t) of S.bucketing, fold mask float32 [V] with 128 nodes).
    "bucket": type 0 holds buckets of LENGTHS entries at targets 0 .. 7 and 0 .. 8 entries elsewhere, random sources; type 1 is random;
    type 2 is one self loop per node.  "walk": 0 .. 8 entries per (target, type) bucket, and NO_IN_EDGE have no in-edge of any type."""
    if which not in _GRAPHS:
        rng = np.random.default_rng(23 if which == "bucket" else 29)
        adjacency = []
        for l in range(L):
            if which == "bucket" and l == 2:
                e = np.stack([np.arange(V), np.arange(V)], axis=1)
            elif which == "bucket" and l == 1:
                e = np.stack([rng.integers(0, V, size=900), rng.integers(0, V, size=900)], axis=1)
            else:
                lengths = rng.integers(0, 9, size=V)
                if which == "bucket":
                    lengths[:len(LENGTHS)] = LENGTHS
                else:
                    lengths[NO_IN_EDGE] = 0
                tgt = np.repeat(np.arange(V), lengths)
                e = np.stack([rng.integers(0, V, size=len(tgt)), tgt], axis=1)
            adjacency.append(np.ascontiguousarray(e[rng.permutation(len(e))], dtype=np.int32))
        mask = np.zeros(V, np.float32)
        head = np.arange(len(LENGTHS)) if which == "bucket" else np.array(NO_IN_EDGE)
        rest = np.setdiff1d(np.arange(V), head)
        mask[np.concatenate([head, rng.choice(rest, size=128 - len(head), replace=False)])] = 1.0
        _GRAPHS[which] = (adjacency, S.bucketing(adjacency, V), mask)
    return _GRAPHS[which]


def seed_batches(fold_mask, per_batch: int, seed: int, epoch: int):
    """A permutation of the fold's nodes from RandomState([seed, epoch]) cut into ascending int32 lists of per_batch."""
    nodes = np.flatnonzero(np.asarray(fold_mask) != 0)
    order = np.random.RandomState([int(seed) & 0xffffffff, int(epoch) & 0xffffffff]).permutation(len(nodes))
    shuffled = nodes[order]
    return [np.sort(shuffled[i:i + per_batch]).astype(np.int32) for i in range(0, len(shuffled), per_batch)]


def presampled_node_sets(rowptr_t, col_t, num_nodes, num_edge_types, fold_mask, roots_per_batch, walk_length, seed, epochs):
    """Epochs 0x80000000 + e of root lists, every list walked with replica 0x20000000 and draw = the running index."""
    sets = []
    for e in range(int(epochs)):
        for roots in seed_batches(fold_mask, roots_per_batch, seed, PRESAMPLE_EPOCH + e):
            sets.append(S.walk_nodes(rowptr_t, col_t, num_nodes, num_edge_types, roots, walk_length, len(sets), seed, PRESAMPLE_REPLICA))
    return sets


def _positions(rowptr_t, col_t, num_nodes, num_edge_types):
    """target, type and source of every by-target position"""
    row = np.repeat(np.arange(num_nodes * num_edge_types), np.diff(np.asarray(rowptr_t, np.int64)))
    return row // num_edge_types, row % num_edge_types, np.asarray(col_t, np.int64) // num_edge_types


def visit_counts(rowptr_t, col_t, num_nodes, num_edge_types, node_sets):
    target, _, source = _positions(rowptr_t, col_t, num_nodes, num_edge_types)
    node_visits, edge_visits = np.zeros(num_nodes, np.int32), np.zeros(len(target), np.int32)
    for nodes in node_sets:
        member = np.zeros(num_nodes, bool)
        member[np.asarray(nodes, np.int64)] = True
        node_visits += member
        edge_visits += member[target] & member[source]
    return node_visits, edge_visits


def kept_positions(rowptr_t, col_t, num_nodes, num_edge_types, nodes):
    """Per type the by-target positions of the entries the induced subgraph keeps, ascending: the order of S.induced()'s lists."""
    target, typ, source = _positions(rowptr_t, col_t, num_nodes, num_edge_types)
    member = np.zeros(num_nodes, bool)
    member[np.asarray(nodes, np.int64)] = True
    keep = member[target] & member[source]
    return [np.flatnonzero(keep & (typ == l)) for l in range(num_edge_types)]


def edge_weights(rowptr_t, col_t, num_nodes, num_edge_types, nodes, node_visits, edge_visits, max_edge_weight=1e4, mistake=""):
    """float32, step for step as the header states it: a = max(C_t, 1) / max(C_p, 1); a = min(a, cap); a * (1 / (deg + 1e-7))."""
    rowptr = np.asarray(rowptr_t, np.int64)
    target, typ, _ = _positions(rowptr_t, col_t, num_nodes, num_edge_types)
    at = np.concatenate(kept_positions(rowptr_t, col_t, num_nodes, num_edge_types, nodes))
    row = target[at] * num_edge_types + typ[at]
    deg = rowptr[row + 1] - rowptr[row]
    if mistake == "induced_degree":
        kept = np.zeros(num_nodes * num_edge_types, np.int64)
        np.add.at(kept, row, 1)
        deg = kept[row]
    c_v = np.maximum(np.asarray(node_visits)[target[at]], 1).astype(np.float32)
    c_e = np.maximum(np.asarray(edge_visits)[at], 1).astype(np.float32)
    a = c_e / c_v if mistake == "inverted" else c_v / c_e
    a = np.minimum(a, np.float32(max_edge_weight))
    return (a * (np.float32(1.0) / (deg.astype(np.float32) + np.float32(1e-7)))).astype(np.float32)


def node_weights(node_visits, nodes, num_subgraphs, mistake="", rowptr_t=None, edge_visits=None, num_edge_types=None):
    """float32 N / max(C_v, 1).  "from_edge_visits": the count of the node's first incoming entry in the node count's place."""
    nodes = np.asarray(nodes, np.int64)
    visits = np.asarray(node_visits)[nodes]
    if mistake == "from_edge_visits":
        rowptr = np.asarray(rowptr_t, np.int64)
        first, end = rowptr[nodes * num_edge_types], rowptr[(nodes + 1) * num_edge_types]
        visits = np.where(end > first, np.asarray(edge_visits)[np.minimum(first, len(edge_visits) - 1)], 0)
    return np.float32(num_subgraphs) / np.maximum(visits, 1).astype(np.float32)


def row_losses(x32, labels):
    """float64 softmax cross-entropy of every row of float32 logits (a -inf column counts as exp(-inf) = 0)."""
    x = np.asarray(x32).astype(np.float64)
    if not x.shape[0]:
        return np.zeros(0)
    m = x.max(axis=1)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(x), 0.0, np.exp(x - m[:, None]))
    return np.log(e.sum(axis=1)) + (m - x[np.arange(x.shape[0]), labels])


def weighted_stats(x32, labels, mask, weights, denominator):
    """(sum mask w loss, sum mask, sum mask [argmax == label], [0] / denominator, [2] / [1], sum mask w) in float64, and
    sum mask w |loss|, which the tolerance is applied to."""
    losses = row_losses(x32, labels)
    mw = np.asarray(mask, np.float64) * np.asarray(weights, np.float64)
    total = float((losses * mw).sum())
    nmask = float(np.asarray(mask, np.float64).sum())
    correct = float(((np.argmax(x32, axis=1) == labels) * np.asarray(mask, np.float64)).sum()) if len(labels) else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        accuracy = np.float64(correct) / np.float64(nmask)
    return (total, nmask, correct, total / float(denominator), float(accuracy), float(mw.sum())), float((np.abs(losses) * mw).sum())


def weighted_gradient(x32, labels, mask, weights, denominator, g_loss, g_total):
    x = np.asarray(x32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(x), 0.0, np.exp(x - x.max(axis=1, keepdims=True)))
    soft = e / e.sum(axis=1, keepdims=True)
    soft[np.arange(x.shape[0]), labels] -= 1.0
    return (np.asarray(mask, np.float64) * np.asarray(weights, np.float64))[:, None] * soft * (g_total + g_loss / float(denominator))
