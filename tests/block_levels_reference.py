"""NumPy restatement of RelGraph's bucketing (tf_gnn_samples_amd/graph.py: two stable sorts over the type-major message list) and of the
derivation of a level graph's bucketing from the union graph's (csrc/level_plan.h; tasks/neighbour_sampling.py, derived_level_graphs;
the citation task's `"blocks": true`).  A helper, not a test: tests/test_block_levels_cpu.py holds the two against each other and shows
that the plausible mistakes differ; tests/test_gpu_block_levels.py holds the kernels to the constructor.  Nothing here touches the GPU
or the package under test.

    constructor(adjacency_lists, num_nodes)           -> the nine arrays of a RelGraph over these lists
    derive(union, hop_nodes, hop_edges, d, mistake)   -> the nine arrays of level d, from the union graph's alone
    level_lists(adjacency_lists, hop_edges, d)        -> the prefix lists of level d
"""
import numpy as np

ARRAYS = ("rowptr_t", "perm_t", "col_t", "inv_perm_t", "rowptr_s", "perm_s", "frow_s", "tgt_s", "pos_t_of_s")
MISTAKES = ("unstable_filter", "rowptr_t_not_filled", "perm_not_rebased", "bound_le")


def constructor(adjacency_lists, num_nodes):
    """Messages type-major (list 0's edges, then list 1's, ...); by target: a stable sort by tgt * L + l; by source: by src * L + l."""
    L, V = len(adjacency_lists), int(num_nodes)
    lists = [np.asarray(a, np.int64).reshape(-1, 2) for a in adjacency_lists]
    src = np.concatenate([a[:, 0] for a in lists])
    tgt = np.concatenate([a[:, 1] for a in lists])
    typ = np.concatenate([np.full(len(a), l, np.int64) for l, a in enumerate(lists)])
    key_t, key_s = tgt * L + typ, src * L + typ
    perm_t = np.argsort(key_t, kind="stable")
    perm_s = np.argsort(key_s, kind="stable")
    inv_perm_t = np.empty_like(perm_t)
    inv_perm_t[perm_t] = np.arange(len(perm_t))
    rowptr = lambda keys: np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=V * L))])
    out = dict(rowptr_t=rowptr(key_t), perm_t=perm_t, col_t=key_s[perm_t], inv_perm_t=inv_perm_t, rowptr_s=rowptr(key_s), perm_s=perm_s,
               frow_s=key_t[perm_s], tgt_s=tgt[perm_s], pos_t_of_s=inv_perm_t[perm_s])
    return {k: v.astype(np.int32) for k, v in out.items()}


def level_lists(adjacency_lists, hop_edges, d):
    return [a[:edges[d]] for a, edges in zip(adjacency_lists, hop_edges)]


def derive(union, hop_nodes, hop_edges, d, mistake=None):
    """Level d < H - 1 (targets: the first T = n_d nodes, sources: the first S = n_{d+1}) from the union graph's arrays and the hop
    sizes; no sort.  mistake: one of MISTAKES, a plausible wrong derivation."""
    assert mistake is None or mistake in MISTAKES
    H, L = len(hop_nodes) - 1, len(hop_edges)
    T, S = int(hop_nodes[d]), int(hop_nodes[d + 1])
    u = {k: np.asarray(v, np.int64) for k, v in union.items()}
    offsets = np.concatenate([[0], np.cumsum([edges[d] for edges in hop_edges])]).astype(np.int64)          # the level's type offsets
    union_offsets = np.concatenate([[0], np.cumsum([edges[H - 1] for edges in hop_edges])]).astype(np.int64)
    delta = (union_offsets - offsets)[:L]                              # message m' of type l of the level is the union's m' + delta[l]
    if mistake == "perm_not_rebased":
        delta = np.zeros_like(delta)
    P = int(offsets[-1])
    # by target: the first P positions of the union's order ARE the level's (its keys are the keys below T * L)
    col_t = u["col_t"][:P]
    fill = u["rowptr_t"][T * L + 1:S * L + 1] if mistake == "rowptr_t_not_filled" else np.full((S - T) * L, P, np.int64)
    rowptr_t = np.concatenate([u["rowptr_t"][:T * L + 1], fill])
    perm_t = u["perm_t"][:P] - delta[col_t % L]
    type_of = np.searchsorted(offsets, np.arange(P), side="right") - 1
    inv_perm_t = u["inv_perm_t"][np.arange(P) + delta[type_of]] if P else np.zeros(0, np.int64)
    # by source: the stable compaction of the union's entries whose target is among the level's
    keep = u["tgt_s"] <= T if mistake == "bound_le" else u["tgt_s"] < T
    kept = np.flatnonzero(keep)
    if mistake == "unstable_filter":                                   # the kept entries of every source bucket in reverse
        bucket = np.searchsorted(u["rowptr_s"], kept, side="right") - 1
        kept = kept[np.lexsort((-kept, bucket))]
    in_front = np.concatenate([[0], np.cumsum(keep)])                  # kept entries in front of position q, q = 0 .. M
    rowptr_s = in_front[u["rowptr_s"][:S * L + 1]]
    frow_s = u["frow_s"][kept]
    out = dict(rowptr_t=rowptr_t, perm_t=perm_t, col_t=col_t, inv_perm_t=inv_perm_t, rowptr_s=rowptr_s,
               perm_s=u["perm_s"][kept] - delta[frow_s % L], frow_s=frow_s, tgt_s=u["tgt_s"][kept], pos_t_of_s=u["pos_t_of_s"][kept])
    return {k: v.astype(np.int32) for k, v in out.items()}


def equal(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ARRAYS)
