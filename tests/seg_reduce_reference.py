"""Plain NumPy references for the segment-reduce kernel family (csrc/seg_reduce.hip) and the seeded inputs its tests share.

Nothing here touches the GPU or the package under test.  A message list is the reference's own: type-major over the adjacency
lists (gnns/rgcn.py:78,108), message m of type l going from adj[l][e, 0] to adj[l][e, 1].  Per-message weights arrive in the
BY-TARGET order the kernels read them in (stable sort of the messages on target * L + type) and are mapped back here.

Every float64 reference returns, next to its value, for every output element
    k        the number of terms of its sum,
    sum_abs  the sum of their magnitudes,
    min_abs  the smallest of their magnitudes (inf where k == 0),
so that a test can hold a float32 kernel to bound(k, sum_abs) and test_seg_reduce_reference_cpu.py can show that this bound
is tight enough to see ONE dropped term (min_abs > 4 * bound)."""
import functools
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24                        # unit round-off of float32, round to nearest
F32_LOWEST = np.float32(-3.4028235e38)
SELU_SCALE = 1.0507009873554804934193349852946
SELU_SCALE_ALPHA = 1.7580993408473768599402175208123
ACT_ALLOWANCE = 3e-7                  # per evaluated activation: what tests/test_gpu_activations.py holds the kernels to
SUM_MODES = ("sum", "mean", "sqrt_n")
MODES = SUM_MODES + ("max",)
KINDS = ("transformed", "untransformed", "messages", "target_rows")   # RelGraph.plan_<kind>


def bound(k, sum_abs):
    """(k + 3) * 2^-24 * sum|term|: a sequential float32 sum of k terms rounds at most k times in its adds; three more
    roundings cover w * f(n), the product with the gathered value and the division or cast at the end."""
    return (np.asarray(k, np.float64) + 3.0) * U * np.asarray(sum_abs, np.float64)


# ---- message lists ------------------------------------------------------------------------------------------------------
Messages = namedtuple("Messages", "rows tgt typ order num_out num_rows V L")


def messages(adj, V, kind="transformed"):
    """rows[m]: the row of X that message m gathers; tgt[m]: the output row it is reduced into; order[p]: the message at
    by-target position p."""
    L = len(adj)
    src = np.concatenate([a[:, 0] for a in adj]).astype(np.int64)
    tgt = np.concatenate([a[:, 1] for a in adj]).astype(np.int64)
    typ = np.concatenate([np.full(len(a), l, np.int64) for l, a in enumerate(adj)])
    M = len(src)
    rows, num_rows = {"transformed": (src * L + typ, V * L), "untransformed": (src, V),
                      "messages": (np.arange(M, dtype=np.int64), M), "target_rows": (tgt, V)}[kind]
    order = np.argsort(tgt * L + typ, kind="stable")
    return Messages(rows, tgt, typ, order, V, num_rows, V, L)


def weights_by_message(msgs, w_t):
    """float32 per-message weights in message order from the by-target array (None: all ones)."""
    if w_t is None:
        return np.ones(len(msgs.tgt), np.float32)
    w = np.empty(len(msgs.tgt), np.float32)
    w[msgs.order] = np.asarray(w_t, np.float32)
    return w


def degree_scale_by_target(adj, V):
    """1 / (in-degree of (type, target) + 1e-7) in float32 (gnns/rgcn.py:100-104), one per message, by-target order."""
    msgs = messages(adj, V)
    deg = np.zeros((len(adj), V), np.float32)
    np.add.at(deg, (msgs.typ, msgs.tgt), np.float32(1.0))
    w = (np.float32(1.0) / (deg[msgs.typ, msgs.tgt] + np.float32(1e-7))).astype(np.float32)
    return w[msgs.order], deg


def mode_factor(msgs, mode):
    """f(n) per output row in float64: 1, 1 / max(n, 1), 1 / sqrt(max(n, 1))."""
    n = np.maximum(np.bincount(msgs.tgt, minlength=msgs.num_out), 1).astype(np.float64)
    return {"sum": np.ones_like(n), "mean": 1.0 / n, "sqrt_n": 1.0 / np.sqrt(n), "max": np.ones_like(n)}[mode]


Sum64 = namedtuple("Sum64", "value k sum_abs min_abs")


def _sum_terms(index, terms, n_out):
    """out[i] = sum of terms[m] over the messages m with index[m] == i, with k, sum|term| and min|term| per element."""
    D = terms.shape[1]
    value, sum_abs = np.zeros((n_out, D)), np.zeros((n_out, D))
    min_abs = np.full((n_out, D), np.inf)
    k = np.broadcast_to(np.bincount(index, minlength=n_out)[:, None], (n_out, D))
    if len(index):
        by = np.argsort(index, kind="stable")
        rows, starts = np.unique(index[by], return_index=True)
        t = terms[by]
        value[rows] = np.add.reduceat(t, starts, axis=0)
        sum_abs[rows] = np.add.reduceat(np.abs(t), starts, axis=0)
        min_abs[rows] = np.minimum.reduceat(np.abs(t), starts, axis=0)
    return Sum64(value, k, sum_abs, min_abs)


def reduce_fwd64(msgs, X, w_t, mode):
    """out[v] = f(n_v) * sum over the messages m into v of w[m] * X[rows[m]]   (sum / mean / sqrt_n), float64."""
    assert mode in SUM_MODES
    w = weights_by_message(msgs, w_t).astype(np.float64)
    f = mode_factor(msgs, mode)
    terms = (w * f[msgs.tgt])[:, None] * np.asarray(X, np.float64)[msgs.rows]
    return _sum_terms(msgs.tgt, terms, msgs.num_out)


def reduce_bwd64(msgs, w_t, gout, mode):
    """gX[r] = sum over the messages m gathered from row r of w[m] * f(n_tgt(m)) * gout[tgt(m)], float64."""
    assert mode in SUM_MODES
    w = weights_by_message(msgs, w_t).astype(np.float64)
    f = mode_factor(msgs, mode)
    terms = (w * f[msgs.tgt])[:, None] * np.asarray(gout, np.float64)[msgs.tgt]
    return _sum_terms(msgs.rows, terms, msgs.num_rows)


Max32 = namedtuple("Max32", "out count win grad")


def max_fwd_bwd32(msgs, X, w_t, gout):
    """unsorted_segment_max and its gradient with the winners decided as the kernels decide them: the product w * x is ONE
    float32 multiply, the maximum is taken over those products (float32 lowest for an empty segment), a message wins where
    its product equals the maximum (-0.0 == +0.0), and gsel = gout / count is ONE float32 division.  The gradient is then
    the float64 sum of w * gsel over the winning messages gathered from a row (a Sum64)."""
    X, gout = np.asarray(X, np.float32), np.asarray(gout, np.float32)
    w = weights_by_message(msgs, w_t)
    prod = (w[:, None] * X[msgs.rows]).astype(np.float32)
    V, D = msgs.num_out, X.shape[1]
    out = np.full((V, D), F32_LOWEST, np.float32)
    count = np.zeros((V, D), np.float32)
    if len(msgs.tgt):
        by = np.argsort(msgs.tgt, kind="stable")
        rows, starts = np.unique(msgs.tgt[by], return_index=True)
        out[rows] = np.maximum(np.maximum.reduceat(prod[by], starts, axis=0), F32_LOWEST)
        win = prod == out[msgs.tgt]
        count[rows] = np.add.reduceat(win[by].astype(np.float32), starts, axis=0)
    else:
        win = np.zeros((0, D), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        gsel = np.where(count > 0, (gout / count).astype(np.float32), np.float32(0.0)).astype(np.float32)
    terms = np.where(win, w.astype(np.float64)[:, None] * gsel.astype(np.float64)[msgs.tgt], 0.0)
    # only the winners are terms of the sum: count, magnitude and minimum over them alone
    value = _sum_terms(msgs.rows, terms, msgs.num_rows).value
    k = np.zeros((msgs.num_rows, D))
    np.add.at(k, msgs.rows, win.astype(np.float64))
    sum_abs = _sum_terms(msgs.rows, np.abs(terms), msgs.num_rows).value
    min_abs = _sum_terms(msgs.rows, np.where(win, np.abs(terms), np.inf), msgs.num_rows).min_abs
    return Max32(out, count, win, Sum64(value, k, sum_abs, min_abs))


# ---- activations --------------------------------------------------------------------------------------------------------
ACTIVATIONS = ("tanh", "relu", "leaky_relu", "elu", "selu", "gelu")
EPILOGUE_ACTIVATIONS = ACTIVATIONS[:5]           # those whose derivative the output determines
LIPSCHITZ = {"tanh": 1.0, "relu": 1.0, "leaky_relu": 1.0, "elu": 1.0, "selu": SELU_SCALE_ALPHA, "gelu": 1.13}


def act64(name, x):
    """(act(x), act'(x)) in float64: utils/utils.py:36-58 of the reference."""
    x = np.asarray(x, np.float64)
    e = np.exp(np.minimum(x, 0.0))
    if name == "tanh":
        t = np.tanh(x)
        return t, 1.0 - t * t
    if name == "relu":
        return np.maximum(x, 0.0), (x > 0).astype(np.float64)
    if name == "leaky_relu":
        return np.where(x > 0, x, 0.2 * x), np.where(x > 0, 1.0, 0.2)
    if name == "elu":
        return np.where(x > 0, x, e - 1.0), np.where(x > 0, 1.0, e)
    if name == "selu":
        return np.where(x > 0, SELU_SCALE * x, SELU_SCALE_ALPHA * (e - 1.0)), np.where(x > 0, SELU_SCALE, SELU_SCALE_ALPHA * e)
    if name == "gelu":
        cdf = 0.5 * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(x / math.sqrt(2.0)))
        return x * cdf, cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    raise KeyError(name)


def dact_from_output64(name, y):
    """act'(x) written in terms of y = act(x), float64 (exact for the five epilogue activations)."""
    y = np.asarray(y, np.float64)
    if name == "tanh":
        return 1.0 - y * y
    if name == "relu":
        return (y > 0).astype(np.float64)
    if name == "leaky_relu":
        return np.where(y > 0, 1.0, 0.2)
    if name == "elu":
        return np.where(y > 0, 1.0, y + 1.0)
    if name == "selu":
        return np.where(y > 0, SELU_SCALE, y + SELU_SCALE_ALPHA)
    raise KeyError(name)


def act_bwd_from_output32(name, y, g):
    """act_bwd_from_output_kernel restated in float32: one multiply for y * y, one subtract (or add), one multiply by g."""
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    one = np.float32(1.0)
    if name == "tanh":
        d = one - (y * y).astype(np.float32)
    elif name == "relu":
        d = np.where(y > 0, one, np.float32(0.0))
    elif name == "leaky_relu":
        d = np.where(y > 0, one, np.float32(0.2))
    elif name == "elu":
        d = np.where(y > 0, one, y + one)
    elif name == "selu":
        d = np.where(y > 0, np.float32(SELU_SCALE), y + np.float32(SELU_SCALE_ALPHA))
    else:
        raise KeyError(name)
    return (g * d.astype(np.float32)).astype(np.float32)


def msgact_fwd64(msgs, X, w_t, mode, name):
    """out[v] = f(n_v) * sum_m act(w[m] * X[rows[m]]) (the Edge-MLP per-message activation inside the reduce): a Sum64 of the
    terms f * act(w x), and the activation allowance of every output element: sum_m f * 3e-7 * max(1, |act(w x)|)."""
    w = weights_by_message(msgs, w_t).astype(np.float64)
    f = mode_factor(msgs, mode)[msgs.tgt][:, None]
    a, _ = act64(name, w[:, None] * np.asarray(X, np.float64)[msgs.rows])
    allowance = _sum_terms(msgs.tgt, f * ACT_ALLOWANCE * np.maximum(1.0, np.abs(a)), msgs.num_out).value
    return _sum_terms(msgs.tgt, f * a, msgs.num_out), allowance


def msgact_bwd64(msgs, X, w_t, gout, mode, name):
    """gX[m] = w[m] * act'(w[m] * X[m]) * f(n) * gout[tgt(m)] for a materialised message tensor X [M, D] (rows[m] == m), and
    the tolerance of every element: 3e-7 * max(1, |act'|) * |w f gout| plus three float32 ulps of the result."""
    w = weights_by_message(msgs, w_t).astype(np.float64)[:, None]
    f = mode_factor(msgs, mode)[msgs.tgt][:, None]
    _, d = act64(name, w * np.asarray(X, np.float64)[msgs.rows])
    wfg = w * f * np.asarray(gout, np.float64)[msgs.tgt]
    ref = d * wfg
    tol = ACT_ALLOWANCE * np.maximum(1.0, np.abs(d)) * np.abs(wfg) + 3.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return ref, tol


# ---- the graphs and inputs the GPU tests use ----------------------------------------------------------------------------
V, L = 97, 3                                     # V = 97: the last workgroup of every group size is ragged; type 1 is empty
D_MAX = 1028
IN_DEGREES = (0, 1, 3, 4, 5, 8, 9, 15, 16, 17)   # per target over all types; 15 / 16 / 17: the unroll-16 tail
OUT_DEGREES = (0, 1, 3, 4, 5)                    # per (source, type) row
HUB_LENGTHS = (63, 63, 64, 64, 65, 65, 130)      # the 64-message index batch, the unroll-8 tail, three batches
HUB_SOURCE_ROWS = (20, 40)                       # two long by-source buckets, so that the hub route chunks the gradient too

Graph = namedtuple("Graph", "name adj V L")


def _assemble(rng, indeg, outdeg, spread=()):
    """Adjacency lists with the given in-degree per target and out-degree per (source, type) row (type 1 stays empty).
    spread: rows whose messages go to distinct targets of in-degree <= 17 (a long by-source bucket must not mix the tiny terms
    of a hub target with terms of order one: no bound could see one of the former next to the latter)."""
    need = indeg.copy()
    edges = []
    for r in spread:
        pool = np.flatnonzero((need > 0) & (indeg <= 17))
        for t in rng.choice(pool, size=outdeg[r], replace=False):
            edges.append((r // L, r % L, t))
            need[t] -= 1
    slots = np.repeat(np.arange(V * L), [0 if r in spread else outdeg[r] for r in range(V * L)])
    rng.shuffle(slots)
    assert len(slots) == need.sum(), (len(slots), need.sum())
    edges += [(r // L, r % L, t) for r, t in zip(slots, np.repeat(np.arange(V), need))]
    edges = [edges[i] for i in rng.permutation(len(edges))]
    return [np.array([(s, t) for s, l, t in edges if l == typ], np.int32).reshape(-1, 2) for typ in range(L)]


def _out_degrees(rng, total, pattern, skip=()):
    """One out-degree per (source, type) row from `pattern` in turn (type 1: none), then single steps up or down on the rows that
    hold the pattern's largest value until the sum is `total`."""
    rows = [r for r in range(V * L) if r % L != 1 and r not in skip]
    out = np.zeros(V * L, np.int64)
    out[rows] = [pattern[i % len(pattern)] for i in rng.permutation(len(rows))]
    top = max(pattern)
    adjustable = [r for r in rows if out[r] == top][1:]
    i = 0
    while out.sum() != total:
        out[adjustable[i % len(adjustable)]] += 1 if out.sum() < total else -1
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def graph(name):
    """'main': in-degrees 0 .. 17 and out-degrees 0 .. 5, so that one dropped term shows in every sum (the sensitivity check);
    'hub': the same degrees plus targets of 63 .. 65 and 130 messages and two long by-source buckets."""
    rng = np.random.default_rng({"main": 1, "hub": 2}[name])
    indeg = np.array([IN_DEGREES[i % len(IN_DEGREES)] for i in range(V)], np.int64)
    rng.shuffle(indeg)
    if name == "main":
        outdeg = _out_degrees(rng, indeg.sum(), OUT_DEGREES + (5, 5, 4, 5, 5))
        return Graph(name, _assemble(rng, indeg, outdeg), V, L)
    indeg[np.flatnonzero(indeg == 0)[:len(HUB_LENGTHS)]] = HUB_LENGTHS
    spread = (5 * L, 11 * L + 2)
    outdeg = _out_degrees(rng, indeg.sum() - sum(HUB_SOURCE_ROWS), (4, 5, 6, 7, 8, 7), skip=spread)
    outdeg[list(spread)] = HUB_SOURCE_ROWS
    return Graph(name, _assemble(rng, indeg, outdeg, spread), V, L)


def _signed(rng, shape):
    """magnitudes in [0.5, 2] with random signs: no term of a sum is small next to the others"""
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


Inputs = namedtuple("Inputs", "graph msgs X gout w_t")


@functools.lru_cache(maxsize=None)
def _master(name, kind, halves):
    g = graph(name)
    msgs = messages(g.adj, g.V, kind)
    rng = np.random.default_rng([{"main": 1, "hub": 2}[name], KINDS.index(kind), int(halves)])
    X = _signed(rng, (msgs.num_rows, D_MAX))
    gout = _signed(rng, (g.V, D_MAX))
    if halves:
        # max: values on a grid of halves and weights that hit the same products from different factors (0.5 * 2 == 1 * 1 ==
        # 2 * 0.5, 1.5 * 1 == 1 * 1.5), one that rounds (1/3): two-way, three-way and mixed-weight ties all occur
        X = (np.round(X * 2) / 2).astype(np.float32)
        w_t = rng.choice(np.array([0.5, 1.0, 2.0, 1.5, 1.0 / 3.0], np.float32), size=len(msgs.tgt)).astype(np.float32)
    else:
        w_t, _ = degree_scale_by_target(g.adj, g.V)
    for a in (X, gout, w_t):
        a.setflags(write=False)
    return g, msgs, X, gout, w_t


def inputs(name, D, kind="transformed", halves=False):
    """The seeded inputs of one GPU case: the first D columns of the master arrays of (graph, plan kind).  halves=True: the max
    inputs (ties).  Columns are independent draws, so a property shown at D_MAX columns holds at every width."""
    g, msgs, X, gout, w_t = _master(name, kind, bool(halves))
    return Inputs(g, msgs, np.array(X[:, :D]), np.array(gout[:, :D]), np.array(w_t))      # copies: the masters stay as they are


def preactivation_margin(res):
    """How far a float32 sum may sit from the float64 one plus four float32 steps at the size of its terms: an element whose
    float64 pre-activation is farther than this from 0 cannot land within four ulps of a ReLU-type kink."""
    return bound(res.k, res.sum_abs) + 4.0 * np.spacing(np.maximum(res.sum_abs, 1e-30).astype(np.float32)).astype(np.float64)
