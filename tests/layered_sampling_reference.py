"""NumPy restatement of the hop-ordered numbering and of the level graphs of a layered sampled batch (include/relgnn_sampling.h,
"The hop-ordered numbering"; tasks/neighbour_sampling.py, HopSubgraph / LevelGraph) over tests/neighbour_sampling_reference.py, and
an integer-valued sum propagation that shows the rule: H layers over the levels give, at every seed, what H layers over the union
graph give.  A helper, not a test: tests/test_layered_sampling_cpu.py checks its properties, tests/test_gpu_layered_sampling.py holds
the kernels to it bit for bit.  Nothing here touches the GPU or the package under test.

    graph(L)                                    -> (adjacency lists, (rowptr_t, col_t, perm_t)) of the test graph, V nodes
    seed_lists(L)                               -> the seed lists of the test graph by name
    sample_by_hop(rowptr_t, col_t, V, L, ...)   -> HopSample: the Sample of the same arguments under the hop-ordered numbering
    levels(sample, rule)                        -> per layer (adjacency lists, num_sources, num_targets, degrees)
    propagate(...) / propagate_levels(...)      -> int64 node states after H layers over the union graph / over the levels
"""
import sys
from pathlib import Path
from typing import List, NamedTuple

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import neighbour_sampling_reference as R  # noqa: E402

# the graph of tests/test_gpu_neighbour_sampling.py (type-0 buckets of these lengths at targets 0, 1, 2, ...: empty, one entry, k and
# k + 1 for k = 2, 3, 4, the wave width and its neighbours, more than two waves, a hub far longer than a wave; duplicate edges
# throughout) and two more nodes: ISOLATED has no incoming edge of any type, DEAD_END has one, from ISOLATED
CORE = 300
ISOLATED, DEAD_END = CORE, CORE + 1
V = CORE + 2
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 5000]
HUB = LENGTHS.index(5000)
_GRAPHS = {}


def graph(L):
    if L not in _GRAPHS:
        rng = np.random.default_rng(100 + L)
        adjacency = []
        for l in range(L):
            lengths = rng.integers(0, 9, size=CORE)
            if l == 0:
                lengths[:len(LENGTHS)] = LENGTHS
            tgt = np.repeat(np.arange(CORE), lengths)
            src = rng.integers(0, CORE, size=len(tgt))
            src[tgt == 20] = 21                                       # one bucket of one edge repeated
            if l == 0:
                src, tgt = np.append(src, ISOLATED), np.append(tgt, DEAD_END)
            e = np.stack([src, tgt], axis=1)[rng.permutation(len(tgt))]
            adjacency.append(np.ascontiguousarray(e, dtype=np.int32))
        _GRAPHS[L] = (adjacency, R.bucketing(adjacency, V))
    return _GRAPHS[L]


def seed_lists(L):
    _, (rowptr, col, _) = graph(L)
    neighbour = int(col[rowptr[7 * L]] // L)                          # a source of target 7: a seed that is another seed's neighbour
    mixed = np.unique(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, HUB, 20, 150, 299, neighbour]))
    return {"mixed": mixed.astype(np.int32), "single": np.array([HUB], np.int32), "all": np.arange(V, dtype=np.int32),
            "dead_end": np.array([DEAD_END], np.int32),               # hop 0 emits one edge, hop 1 none, and finds no new node
            "isolated": np.array([ISOLATED], np.int32)}               # no hop emits an edge: the subgraph is the seed


class HopSample(NamedTuple):
    nodes: np.ndarray                       # int32 [n]: seeds ascending, then the nodes first reached in hop 1 ascending, ...
    adjacency_lists: List[np.ndarray]       # per type int32 [E_l, 2] in these local ids; hops ascending, as Sample's
    degrees: np.ndarray                     # float32 [L, n]
    seed_mask: np.ndarray                   # float32 [n]
    hop_nodes: List[int]                    # [n_0, ..., n_H], cumulative
    hop_edges: List[List[int]]              # per type [E_{l,0}, ..., E_{l,H-1}], cumulative
    node_hop: np.ndarray                    # int64 [n]: the hop that first reached each node (0: a seed)
    by_id: R.Sample                         # the id-ordered sample this one relabels
    new_of_old: np.ndarray                  # int64 [n]: hop-ordered local id of every id-ordered local id


def sample_by_hop(rowptr_t, col_t, num_nodes, num_edge_types, seeds, fanouts, draw, seed=0, replica=0) -> HopSample:
    base = R.sample(rowptr_t, col_t, num_nodes, num_edge_types, seeds, fanouts, draw, seed=seed, replica=replica)
    L, H = int(num_edge_types), len(fanouts)
    in_a_frontier = np.concatenate(base.frontiers).astype(np.int64)
    leaves = np.setdiff1d(base.nodes.astype(np.int64), in_a_frontier)             # first reached in hop H, ascending
    groups = [np.asarray(f, np.int64) for f in base.frontiers] + [leaves]
    nodes = np.concatenate(groups)
    assert len(nodes) == len(base.nodes) and len(np.unique(nodes)) == len(nodes)
    hop_nodes = np.cumsum([len(g) for g in groups]).tolist()
    node_hop = np.repeat(np.arange(H + 1), [len(g) for g in groups])
    new_of_global = np.full(int(num_nodes), -1, np.int64)
    new_of_global[nodes] = np.arange(len(nodes))
    new_of_old = new_of_global[base.nodes]
    adjacency = [new_of_old[a.astype(np.int64)].astype(np.int32).reshape(-1, 2) for a in base.adjacency_lists]
    degrees = np.zeros_like(base.degrees)
    degrees[:, new_of_old] = base.degrees
    seed_mask = np.zeros(len(nodes), np.float32)
    seed_mask[new_of_old] = base.seed_mask
    # a node is expanded once, in the hop whose frontier holds it: its sampled in-degree is what that hop emitted for it
    hop_edges = [np.cumsum([int(degrees[l, new_of_global[g]].sum()) for g in groups[:H]]).tolist() for l in range(L)]
    return HopSample(nodes.astype(np.int32), adjacency, degrees, seed_mask, hop_nodes, hop_edges, node_hop, base, new_of_old)


def levels(sample: HopSample, rule: str = "right"):
    """Per layer l = 1 .. H: (adjacency lists, num_sources, num_targets, degrees [L, num_sources]).  rule "right": the edges whose
    targets are among the first n_{H-l} nodes, the prefix E_{l,H-l} of every list.  Two deliberately wrong rules: "one_hop_short"
    stops the prefix one hop early; "per_hop" takes the edges the hop H - l emitted alone instead of the cumulative prefix."""
    H = len(sample.hop_nodes) - 1
    out = []
    for layer in range(1, H + 1):
        d = H - layer
        sources, targets = sample.hop_nodes[d + 1], sample.hop_nodes[d]
        lists = []
        for a, cumulative in zip(sample.adjacency_lists, sample.hop_edges):
            if rule == "right":
                lists.append(a[:cumulative[d]])
            elif rule == "one_hop_short":
                lists.append(a[:cumulative[d - 1] if d > 0 else 0])
            elif rule == "per_hop":
                lists.append(a[(cumulative[d - 1] if d > 0 else 0):cumulative[d]])
            else:
                raise ValueError(rule)
        table = np.zeros((sample.degrees.shape[0], sources), np.float32)
        table[:, :targets] = sample.degrees[:, :targets]
        out.append((lists, sources, targets, table))
    return out


MODULUS = 1_000_003


def _layer(states, adjacency_lists, layer_idx):
    """One integer 'RGCN' layer: out[t] = sum over types l and edges (s, t) of type l of (3 + 2 l + layer) * states[s], squared and
    reduced: not linear, exact in int64."""
    out = np.zeros_like(states)
    for l, a in enumerate(adjacency_lists):
        a = np.asarray(a, np.int64).reshape(-1, 2)
        np.add.at(out, a[:, 1], (3 + 2 * l + layer_idx) * states[a[:, 0]])
    out %= MODULUS
    return (out * out + out + 1) % MODULUS


def propagate(states, adjacency_lists, num_layers, residual_every=10 ** 9):
    """num_layers layers over one graph, with the driver's residual rule (models/sparse_graph_model.py): at layer index i > 0 with
    i % residual_every == 0 the input becomes input + the input of the last residual step (the mean's division left out: integers)."""
    cur, last = np.asarray(states, np.int64), None
    for i in range(num_layers):
        if i % residual_every == 0:
            kept = cur
            if i > 0:
                cur = (cur + last) % MODULUS
            last = kept
        cur = _layer(cur, adjacency_lists, i)
    return cur


def propagate_levels(states, level_list, residual_every=10 ** 9):
    """The same over level graphs: layer i takes num_sources rows, its output is cut to num_targets rows, the kept residual tensor is
    cut to the current row count."""
    cur, last = np.asarray(states, np.int64), None
    for i, (lists, sources, targets, _) in enumerate(level_list):
        assert cur.shape[0] == sources, (i, cur.shape, sources)
        if i % residual_every == 0:
            kept = cur
            if i > 0:
                cur = (cur + last[:sources]) % MODULUS
            last = kept
        cur = _layer(cur, lists, i)[:targets]
    return cur
