"""NumPy restatement of the graph partitioner's rule (csrc/graph_partition.h, tasks/graph_partition.py), with
Philox through tests/philox_reference.py, and the graphs its tests run on.  A helper, not a test.

The rule, for rowptr_t int32 [V * L + 1], col_t int32 [M] = source * L + type (a RelGraph's), P parts, a 32-bit seed, imbalance_percent b
and refine_rounds T:
  cap = ceil(V (100 + b) / (100 P)).  N(v) = col_t[j] // L over j in [rowptr_t[v L], rowptr_t[(v + 1) L]), with multiplicity, without
  the entries whose source is v.  part int32 [V], -1 unassigned.  The anchors, ascending, are
  sort(RandomState([seed & 0xffffffff, 4]).choice(V, P, replace=False)); anchor i starts in part i and never moves.
  A round over an eligible set reads the round's start only: size[l] = nodes in part l, room[l] = cap - size[l]; for an eligible v,
  c(l) = |{u in N(v): part[u] = l}|, base = c(part[v]) (0 for an unassigned v), and v wishes the lowest l among those that maximise
  c(l) over the labels with l != part[v], room[l] > 0 and c(l) > base (nothing if there is none).  Per label the wishing nodes are
  taken in ascending id and the first room[l] of them move; departures are not credited within the round.
  Grow: rounds over the unassigned nodes until one moves nobody.  Fill: the k-th node still unassigned, ascending, goes to part
  searchsorted(cumsum(room), k, side="right").  Refine, rounds r = 0 .. T - 1: eligible are the non-anchor v with
  philox4x32_10((v, r, 0, 0), (seed, 0x10000000))[0] & 1 == 1.

VARIANTS names the mistakes the tests must be able to see: each changes the result on at least one test graph."""
import numpy as np

from philox_reference import philox4x32_10

ELIGIBLE_KEY = 0x10000000
VARIANTS = ("ties_highest", "count_self", "credit_departures", "admit_descending", "at_least_base", "all_eligible")


def cap_of(V, P, b):
    return -(-V * (100 + b) // (100 * P))


def anchors_of(V, P, seed):
    return np.sort(np.random.RandomState([seed & 0xffffffff, 4]).choice(V, P, replace=False)).astype(np.int32)


def refine_eligible(V, r, seed, anchors):
    """bool [V]: who may move in refine round r."""
    word = philox4x32_10((np.arange(V), r, 0, 0), (seed & 0xffffffff, ELIGIBLE_KEY))[0]
    eligible = (word & np.uint64(1)) == np.uint64(1)
    eligible[anchors] = False
    return eligible


def sizes_of(part, P):
    return np.bincount(part[part >= 0], minlength=P)[:P]


def wishes(rowptr, col, L, part, room, eligible, variant=()):
    """int32 [V]: the wish of every eligible node, -1 for none and for everyone else."""
    V, P = len(part), len(room)
    ends = np.asarray(rowptr, dtype=np.int64)[::L]
    target = np.repeat(np.arange(V), np.diff(ends))
    source = np.asarray(col, dtype=np.int64) // L
    label = part[source].astype(np.int64)
    counted = (label >= 0) & eligible[target]
    if "count_self" not in variant:
        counted &= source != target
    pairs, count = np.unique(target[counted] * P + label[counted], return_counts=True)       # every (v, l) with c(l) >= 1
    v, l = pairs // P, pairs % P
    own = l == part[v]
    base = np.zeros(V, dtype=np.int64)
    base[v[own]] = count[own]
    beats = count >= base[v] if "at_least_base" in variant else count > base[v]
    candidate = ~own & (room[l] > 0) & beats
    v, l, count = v[candidate], l[candidate], count[candidate]
    order = np.lexsort((-l if "ties_highest" in variant else l, -count, v))      # per node: the largest count first, then the lowest label
    v, l = v[order], l[order]
    first = np.ones(len(v), dtype=bool)
    first[1:] = v[1:] != v[:-1]
    wish = np.full(V, -1, dtype=np.int32)
    wish[v[first]] = l[first]
    return wish


def admitted(wish, room, part=None, variant=()):
    """bool [V]: per label the nodes that wish it in ascending id, the first room[label] of them."""
    moved = np.zeros(len(wish), dtype=bool)
    room = np.asarray(room).copy()
    if "credit_departures" in variant:                      # (a node that wishes to leave frees its place at once)
        room += np.bincount(part[(wish >= 0) & (part >= 0)], minlength=len(room))
    for l in np.unique(wish[wish >= 0]):
        ids = np.flatnonzero(wish == l)
        if "admit_descending" in variant:
            ids = ids[::-1]
        moved[ids[:max(int(room[l]), 0)]] = True
    return moved


def one_round(rowptr, col, L, part, eligible, P, cap, variant=()):
    """-> (the new part array, who moved)."""
    room = cap - sizes_of(part, P)
    wish = wishes(rowptr, col, L, part, room, eligible, variant)
    moved = admitted(wish, room, part, variant)
    return np.where(moved, wish, part).astype(np.int32), moved


def partition(rowptr, col, L, P, seed=0, b=10, T=8, variant=(), after_round=None):
    """The whole rule -> part int32 [V].  after_round(phase, part) sees the array after every round and after the fill."""
    V = (len(rowptr) - 1) // L
    cap, anchors = cap_of(V, P, b), anchors_of(V, P, seed)
    part = np.full(V, -1, dtype=np.int32)
    part[anchors] = np.arange(P, dtype=np.int32)
    see = after_round or (lambda phase, part: None)
    while True:
        part, moved = one_round(rowptr, col, L, part, part < 0, P, cap, variant)
        see("grow", part)
        if not moved.any():
            break
    left = np.flatnonzero(part < 0)
    room = cap - sizes_of(part, P)
    part[left] = np.searchsorted(np.cumsum(room), np.arange(len(left)), side="right")
    see("fill", part)
    for r in range(T):
        eligible = refine_eligible(V, r, seed, anchors)
        if "all_eligible" in variant:
            eligible[:] = True
            eligible[anchors] = False
        part, _ = one_round(rowptr, col, L, part, eligible, P, cap, variant)
        see("refine", part)
    return part


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
def bucketing(adjacency_lists, V):
    """rowptr_t int32 [V * L + 1] and col_t int32 [M] of adjacency lists ([E, 2] arrays of (source, target), one per type): rows
    target * L + type, a row's entries in the order of the lists (what RelGraph builds on the device)."""
    L = len(adjacency_lists)
    rows = np.concatenate([np.asarray(e).reshape(-1, 2)[:, 1].astype(np.int64) * L + l for l, e in enumerate(adjacency_lists)])
    cols = np.concatenate([np.asarray(e).reshape(-1, 2)[:, 0].astype(np.int64) * L + l for l, e in enumerate(adjacency_lists)])
    order = np.argsort(rows, kind="stable")
    rowptr = np.zeros(V * L + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=V * L), out=rowptr[1:])
    return rowptr.astype(np.int32), cols[order].astype(np.int32)


def planted_graph(V, C, seed, L=1):
    """C communities interleaved by id (node v is in community v % C, so id blocks are useless); every node makes 6 draws inside its
    community and 1 outside, each stored in both directions and dealt to one of L types -> adjacency lists, [E, 2] int32 each."""
    rng = np.random.RandomState([seed, V, C])
    nodes = np.arange(V)
    inside = (rng.randint(0, -(-V // C), size=(V, 6)) * C + (nodes % C)[:, None]) % V
    inside = np.where(inside % C == (nodes % C)[:, None], inside, nodes[:, None])          # (V no multiple of C: the wrapped draws)
    outside = rng.randint(0, V, size=(V, 1))
    drawn = np.concatenate([inside, outside], axis=1)
    pairs = np.stack([np.repeat(nodes, 7), drawn.reshape(-1)], axis=1)
    edges = np.concatenate([pairs, pairs[:, ::-1]])
    types = rng.randint(0, L, size=len(edges))
    return [edges[types == l].astype(np.int32) for l in range(L)]


def kept_entries(rowptr, col, L, part):
    """(the entries whose two ends share a part, the non-self entries)."""
    V = len(part)
    target = np.repeat(np.arange(V), np.diff(np.asarray(rowptr, dtype=np.int64)[::L]))
    source = np.asarray(col, dtype=np.int64) // L
    apart = source != target
    return int((apart & (part[source] == part[target])).sum()), int(apart.sum())


def random_partition(V, P, seed):
    """An equal-size random partition: RandomState(seed).permutation(V) * P // V."""
    return (np.random.RandomState(seed).permutation(V) * P // V).astype(np.int32)
