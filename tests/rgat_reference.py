"""Plain NumPy references for the RGAT attention kernels (csrc/rgat_fast.hip, csrc/rgat.hip, csrc/rgat_scores.hip) and the seeded
inputs their tests share.  Nothing here touches the GPU or the package under test.

The operation (gnns/rgat.py:98-136 of the reference), on the by-target message list of seg_reduce_reference.messages(adj, V,
"transformed") — position p gathers row col[p] = src * L + type of T and belongs to target v(p), bucket trow(p) = v * L + type:
    z[p,k]      = s_src[col p, k] + s_tgt[trow p, k]
    e           = z if z > 0 else slope * z                       lrelu'(0) = slope: the kernels' convention and torch's
    alpha[p,k]  = exp(e - max) / sum exp(e - max)                 over ALL messages of the target, per head
    out[v, k:]  = sum_p alpha[p,k] * T[col p, head k]
    dz[p,k]     = alpha * (<gout_vk, T_k[col p]> - <gout_vk, out_vk>) * lrelu'(z)
    gT[r, k:]   = sum over the messages gathered from r of alpha[p,k] * gout[v(p), head k]
    gs_src[r,k] = sum of dz over the messages gathered from row r;  gs_tgt[(v,l),k] = sum of dz over bucket (v, l)
and for the score kernels, with att [L, 2D] read as [L, K, 2 Dh] (first Dh entries of a head: the source half):
    s_src[r,k]  = <T[r, head k], att[l, k, :Dh]>,  s_tgt[r,k] = <T[r, head k], att[l, k, Dh:]>       (l = r % L)
    d att[l,k]  = sum_v gs_src[v L + l, k] * T[v L + l, head k]  ||  the same with gs_tgt
    gT         += gs_src * att[.., :Dh] + gs_tgt * att[.., Dh:]   (the in-place fold)
Every float64 sum comes with the bookkeeping of seg_reduce_reference.Sum64 (k, sum_abs, min_abs) per output element.

The bounds a float32 kernel is held to, with u = 2^-24 and A = ACT_ALLOWANCE = 3e-7 (what tests/test_gpu_activations.py holds the
project's transcendental kernels to, taken per expf / logf evaluation).  All of it is first order in u, evaluated at the float64
values, and derived here, not tuned:

  alpha.  The kernels compute expf(w), w = fl(fl(e^ - max) - logf(S)), S = the float32 sum of expf(fl(e^ - max)), e^ the float32 e.
    * e^ differs from e by at most dz_in + 2 u |z| (the score tables' own error dz_in, 0 for given tables; the add; the product with
      slope).  A softmax whose logits all move by at most d moves by at most the factor exp(2 d): 2 * max over the target.
    * fl(e^ - max) rounds once: u |d|, d = e - max, an absolute error of the exponent.
    * S: every term has the relative error A + u |d_q| (the latter weighs alpha_q in the total), the n-term sum (n + 2) u whatever its
      order — the terms are positive; logf adds A * max(1, |log S|) absolute; all of it enters the exponent as an absolute error.
    * the second subtraction rounds once: u |log alpha|;  the final expf: A.
    The sum of these, r, gives |alpha^ - alpha| <= alpha * expm1(r) + FLT_MIN; the floor (the smallest normal float32) is for an
    alpha that underflows, where expf may flush or return a denormal of few bits.
  plain sums (out, gT, gs_src, gs_tgt, score tables): seg_reduce_reference.bound(k, sum_abs) = (k + 3) u sum|term| plus the error of
    the computed factor carried through: sum |term's other factor| * tol(alpha or dz).
  dz = alpha * (a - c) * lrelu'.  a and c are dot products of Dh terms, (Dh + 3) u sum|g t| each; c is taken with the kernel's OWN
    float32 out, so sum |g| tol(out) more; the difference rounds once, the two products twice and one to spare: 3 u |dz|; and
    tol(alpha) |a - c|.  The absolute terms matter: a target with one message has a - c == 0 in float64 and rounding residue in
    float32.
  the composition from segment ops takes c as sum_q alpha_q a_q: dz_composed, added to tol(dz) there, is that sum's bound
    (n + 3) u sum alpha |a| plus the dot products' (Dh + 3) u sum alpha sum|g t|.
  d att: group partials, then column_sum — one sum of V terms plus two roundings, bound(V + 2, sum_abs), plus sum |T| tol(gs).
  the fold: a sum of three terms, bound(3, .), plus tol(gT) + |att| tol(gs).
lrelu' is a step: with given score tables (multiples of 2^-6, |s| <= 60) z is exact in float32 and no branch can differ from
float64; with computed tables fused_inputs() asserts that every float64 z is farther from 0 than z's own error bound.

restate32() states every quantity again in float32 in the kernels' evaluation order (sequential sums in message order; the
wave-wide xor tree over 64-message chunks where the fast kernels use one), so that tests/test_rgat_reference_cpu.py can show that
honest float32 arithmetic lies inside every bound and that the bounds see each of a list of plausible mistakes."""
import functools
from collections import namedtuple

import numpy as np

import seg_reduce_reference as S
from seg_reduce_reference import ACT_ALLOWANCE, Sum64, U, bound

FLT_MIN = float(np.finfo(np.float32).tiny)
SLOPE = 0.2
D_MAX, K_MAX = 1024, 16

# ---- graphs -------------------------------------------------------------------------------------------------------------
# chunks: per target the bucket lengths (type 0 .. 3).  The fast kernels walk a target in chunks of 64 messages:
CHUNK_TARGETS = (
    (40, 50, 0, 7),      # 97 = 64 + 33: the chunk boundary falls inside bucket 1; tail 33 % 8 == 1
    (64, 10, 0, 0),      # exactly between buckets 0 and 1; tail 10 % 8 == 2
    (30, 34, 6, 0),      # exactly between buckets 1 and 2; tail 6
    (0, 0, 70, 5),       # two empty leading buckets, then the boundary inside bucket 2; tail 11 % 8 == 3
    (0, 70, 0, 0),       # 70 messages from ONE source row (SAME_ROW_TARGET)
    (0, 0, 0, 1),        # one message
    (0, 0, 0, 0),        # none
    (3, 0, 5, 0), (3, 0, 6, 0), (0, 4, 0, 6), (1, 1, 1, 8), (12, 0, 0, 0), (0, 13, 0, 0), (7, 0, 0, 7), (5, 5, 5, 0),   # n = 8 .. 15
    (20, 20, 20, 8),     # 68 = 64 + 4: tail 4; the boundary inside bucket 3
    (0, 0, 0, 133),      # three chunks of one bucket, tail 5
)
SAME_ROW_TARGET, SAME_ROW_SOURCE = 4, 9
CHUNKS_V, CHUNKS_L = 23, 4                       # V = 23: not a multiple of 4, the last workgroup is ragged
TYPED = {"many_types": (61, 23, 5), "sixteen_types": (59, 16, 6)}      # V, L, seed
TYPED_DEGREES = (0, 1, 2, 3, 5, 8, 9, 12, 17)

GRAPHS = ("main", "hub", "many_types", "sixteen_types", "chunks")


@functools.lru_cache(maxsize=None)
def graph(name):
    """'main' / 'hub': the seg-reduce graphs.  'many_types' (L = 23) / 'sixteen_types' (L = 16): about 60 nodes, at most 17 messages
    per target, so most types of a target are empty.  'chunks': the hand-built targets of CHUNK_TARGETS."""
    if name in ("main", "hub"):
        return S.graph(name)
    if name in TYPED:
        V, L, seed = TYPED[name]
        rng = np.random.default_rng(seed)
        edges = [[] for _ in range(L)]
        for v in rng.permutation(V):
            for _ in range(TYPED_DEGREES[v % len(TYPED_DEGREES)]):
                edges[rng.integers(L)].append((rng.integers(V), v))
    else:
        V, L = CHUNKS_V, CHUNKS_L
        rng = np.random.default_rng(7)
        edges = [[] for _ in range(L)]
        for v, lengths in enumerate(CHUNK_TARGETS):
            for l, n in enumerate(lengths):
                src = np.full(n, SAME_ROW_SOURCE) if v == SAME_ROW_TARGET else rng.integers(V, size=n)
                edges[l] += [(s, v) for s in src]
        edges = [[e[i] for i in rng.permutation(len(e))] for e in edges]
    return S.Graph(name, [np.array(e, np.int32).reshape(-1, 2) for e in edges], V, L)


Positions = namedtuple("Positions", "col v l trow V L M")


def positions(msgs, order=None):
    """The by-target message list: position p gathers row col[p] of T for target v[p] through type l[p].  order: the by-target
    permutation (default: the reference's stable sort; a test passes the graph's own, which may order a bucket differently)."""
    order = msgs.order if order is None else np.asarray(order, np.int64)
    v, l = msgs.tgt[order], msgs.typ[order]
    assert np.all(np.diff(v * msgs.L + l) >= 0), "not a by-target order"
    return Positions(msgs.rows[order], v, l, v * msgs.L + l, msgs.V, msgs.L, len(order))


# ---- float64 ------------------------------------------------------------------------------------------------------------
def _seg_sum(index, x, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, index, x)
    return out


def _seg_max(index, x, n, empty=-np.inf):
    out = np.full((n,) + x.shape[1:], empty)
    np.maximum.at(out, index, x)
    return out


def _heads(D, K):
    assert D % K == 0
    return np.arange(D) // (D // K)


Attention64 = namedtuple("Attention64", "z n alpha alpha_tol out out_tol dz dz_tol dz_composed gT gT_tol gs_src gs_src_tol gs_tgt gs_tgt_tol")


def attention64(pos, T, s_src, s_tgt, K, slope, gout, z_err=None):
    """Every quantity of the attention op in float64 with its tolerance (see the module docstring).  s_src / s_tgt: float32 tables,
    or float64 ones with z_err [M, K], the bound on the error of the kernel's own z = s_src + s_tgt before its add."""
    V, L, M = pos.V, pos.L, pos.M
    D = T.shape[1]
    Dh, hcol = D // K, _heads(D, K)
    slope = float(np.float32(slope))
    T, gout = np.asarray(T, np.float64), np.asarray(gout, np.float64)
    z = np.asarray(s_src, np.float64)[pos.col] + np.asarray(s_tgt, np.float64)[pos.trow]
    e = np.where(z > 0, z, slope * z)
    d = e - _seg_max(pos.v, e, V)[pos.v]
    ex = np.exp(d)
    den = _seg_sum(pos.v, ex, V)
    alpha = ex / den[pos.v]
    n = np.bincount(pos.v, minlength=V)
    z_in = (0.0 if z_err is None else z_err) + 2 * U * np.abs(z)
    with np.errstate(divide="ignore"):
        log_den = np.where(den > 0, np.log(np.maximum(den, 1e-300)), 0.0)
    r = (2 * _seg_max(pos.v, z_in, V, 0.0)[pos.v] + U * np.abs(d)
         + U * _seg_sum(pos.v, np.abs(d) * alpha, V)[pos.v] + ACT_ALLOWANCE + (n[pos.v, None] + 2) * U
         + ACT_ALLOWANCE * np.maximum(1.0, np.abs(log_den))[pos.v]
         + U * np.abs(d - log_den[pos.v]) + ACT_ALLOWANCE)
    alpha_tol = alpha * np.expm1(r) + FLT_MIN

    a_cols, at_cols = alpha[:, hcol], alpha_tol[:, hcol]
    Tc, gv = T[pos.col], gout[pos.v]
    out = S._sum_terms(pos.v, a_cols * Tc, V)
    out_tol = bound(out.k, out.sum_abs) + _seg_sum(pos.v, at_cols * np.abs(Tc), V)

    def per_head(x):
        return x.reshape(x.shape[0], K, Dh).sum(-1)
    a, a_abs = per_head(gv * Tc), per_head(np.abs(gv * Tc))
    c, c_abs = per_head(gout * out.value), per_head(np.abs(gout * out.value))
    c_extra = per_head(np.abs(gout) * out_tol)
    dprime = np.where(z > 0, 1.0, slope)
    diff = a - c[pos.v]
    dz = alpha * diff * dprime
    dz_tol = dprime * (alpha_tol * np.abs(diff) + (alpha + alpha_tol) * (
        (Dh + 3) * U * (a_abs + c_abs[pos.v]) + c_extra[pos.v] + U * np.abs(diff))) + 3 * U * np.abs(dz)

    # the composition from segment ops (gnns.rgat._attention_from_segment_ops) takes c as sum_q alpha_q a_q through autograd instead
    # of <gout, out>: an n-term sum of terms that each carry a dot product's error
    dz_composed = dprime * (alpha + alpha_tol) * ((n[:, None] + 3) * U * _seg_sum(pos.v, alpha * np.abs(a), V)
                                                  + (Dh + 3) * U * _seg_sum(pos.v, alpha * a_abs, V))[pos.v]
    gT = S._sum_terms(pos.col, a_cols * gv, V * L)
    gT_tol = bound(gT.k, gT.sum_abs) + _seg_sum(pos.col, at_cols * np.abs(gv), V * L)
    gs_src = S._sum_terms(pos.col, dz, V * L)
    gs_src_tol = bound(gs_src.k, gs_src.sum_abs) + _seg_sum(pos.col, dz_tol, V * L)
    gs_tgt = S._sum_terms(pos.trow, dz, V * L)
    gs_tgt_tol = bound(gs_tgt.k, gs_tgt.sum_abs) + _seg_sum(pos.trow, dz_tol, V * L)
    return Attention64(z, n, alpha, alpha_tol, out, out_tol, dz, dz_tol, dz_composed, gT, gT_tol, gs_src, gs_src_tol, gs_tgt, gs_tgt_tol)


def _att_halves(att, L, K):
    """att [L, 2D] -> (source half, target half), each [L, D] with head k at columns k Dh .. (k + 1) Dh"""
    a = np.asarray(att).reshape(L, K, 2, -1)
    return a[:, :, 0, :].reshape(L, -1), a[:, :, 1, :].reshape(L, -1)


def _sum_last(terms):
    """Sum64 of the sum over the last axis"""
    k = np.full(terms.shape[:-1], terms.shape[-1])
    return Sum64(terms.sum(-1), k, np.abs(terms).sum(-1), np.abs(terms).min(-1))


def scores64(T, att, L, K):
    """(s_src, s_tgt): Sum64 each, [V L, K], k = Dh"""
    T = np.asarray(T, np.float64)
    R, D = T.shape
    lrow = np.arange(R) % L
    return tuple(_sum_last((T * np.asarray(h, np.float64)[lrow]).reshape(R, K, D // K)) for h in _att_halves(att, L, K))


def datt64(T, gs_src, gs_tgt, L, K, gs_src_tol=0.0, gs_tgt_tol=0.0):
    """(d att [L, 2D] as a Sum64 with k = V, its tolerance)"""
    T = np.asarray(T, np.float64)
    R, D = T.shape
    V, hcol = R // L, _heads(D, K)
    parts, tols = [], []
    for gs, gtol in ((gs_src, gs_src_tol), (gs_tgt, gs_tgt_tol)):
        terms = (np.asarray(gs, np.float64)[:, hcol] * T).reshape(V, L, K, D // K)
        parts.append(_sum_last(np.moveaxis(terms, 0, -1)))
        tols.append(((np.zeros((R, K)) + gtol)[:, hcol] * np.abs(T)).reshape(V, L, K, D // K).sum(0))
    res = Sum64(*[np.stack([p[i] for p in parts], axis=2).reshape(L, 2 * D) for i in range(4)])
    return res, bound(res.k + 2, res.sum_abs) + np.stack(tols, axis=2).reshape(L, 2 * D)


def fold64(gT, gs_src, gs_tgt, att, L, K, gT_tol=0.0, gs_src_tol=0.0, gs_tgt_tol=0.0):
    """(gT + gs_src * att_src + gs_tgt * att_tgt as a Sum64 with k = 3, its tolerance)"""
    gT = np.asarray(gT, np.float64)
    R, D = gT.shape
    hcol, lrow = _heads(D, K), np.arange(R) % L
    a_s, a_t = (np.asarray(h, np.float64)[lrow] for h in _att_halves(att, L, K))
    terms = np.stack([gT, np.asarray(gs_src, np.float64)[:, hcol] * a_s, np.asarray(gs_tgt, np.float64)[:, hcol] * a_t], axis=-1)
    res = _sum_last(terms)
    tol = bound(res.k, res.sum_abs) + gT_tol + (np.zeros((R, K)) + gs_src_tol)[:, hcol] * np.abs(a_s) \
        + (np.zeros((R, K)) + gs_tgt_tol)[:, hcol] * np.abs(a_t)
    return res, tol


# ---- float32, in the kernels' order -------------------------------------------------------------------------------------
F = np.float32


def _ranks(seg):
    """position of every element inside its run of equal `seg` values (seg sorted)"""
    start = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]]) if len(seg) else np.zeros(0, np.int64)
    return np.arange(len(seg)) - np.repeat(start, np.diff(np.r_[start, len(seg)]))


def _seq_sum32(seg, terms, nseg):
    """out[s] = ((t0 + t1) + t2) + ... over the elements of segment s in the order given, float32 (seg sorted)"""
    acc = np.zeros((nseg,) + terms.shape[1:], F)
    rank = _ranks(seg)
    by = np.argsort(rank, kind="stable")
    cuts = np.cumsum(np.bincount(rank)) if len(rank) else []
    lo = 0
    for hi in cuts:
        sel = by[lo:hi]
        acc[seg[sel]] = acc[seg[sel]] + terms[sel]
        lo = hi
    return acc


def _tree_sum32(seg, terms, nseg, lane=None, chunk=None):
    """The fast kernels' order: 64 elements at a time, one per lane (idle lanes hold 0), the xor butterfly of wave_sum (every lane
    ends with the same total), the chunk totals added up in turn.  lane / chunk: where an element sits (default: its rank)."""
    rank = _ranks(seg)
    lane = rank % 64 if lane is None else lane
    chunk = rank // 64 if chunk is None else chunk
    key = seg * (int(chunk.max(initial=0)) + 1) + chunk
    ids, inv = np.unique(key, return_inverse=True)
    wave = np.zeros((len(ids), 64) + terms.shape[1:], F)
    wave[inv, lane] = terms
    for off in (32, 16, 8, 4, 2, 1):
        wave = wave + wave[:, np.arange(64) ^ off]
    return _seq_sum32(ids // (int(chunk.max(initial=0)) + 1), wave[:, 0], nseg)


def _dot32(a, b, K):
    """per-head dot product [N, D] x [N, D] -> [N, K]: a float4's four products in turn, then the float4s of the head in turn"""
    p = (a.astype(F) * b.astype(F)).reshape(a.shape[0], K, -1, 4)
    s = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    acc = s[..., 0]
    for j in range(1, s.shape[-1]):
        acc = acc + s[..., j]
    return acc


MUTATIONS = ("drop_message", "bucket_softmax", "head0_alpha", "no_cdot", "lrelu_branch", "chunk_neighbour_type")


def restate32(pos, T, s_src, s_tgt, K, slope, gout, tree=True, chunked=True, mutate=None):
    """Every quantity in float32.  tree: rgat_alpha_kernel's wave-wide sums; chunked: gs_tgt as rgat_dz_kernel keeps it, a wave total
    per 64-message chunk and type; otherwise in message order (csrc/rgat.hip).  mutate: one of MUTATIONS or 'no_shift' — the same
    arithmetic with one plausible mistake."""
    assert mutate in (None, "no_shift") + MUTATIONS
    V, L, M = pos.V, pos.L, pos.M
    D = T.shape[1]
    hcol = _heads(D, K)
    T, gout, slope = np.asarray(T, F), np.asarray(gout, F), F(slope)
    seg_sum = _tree_sum32 if tree else _seq_sum32
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        z = np.asarray(s_src, F)[pos.col] + np.asarray(s_tgt, F)[pos.trow]
        e = np.where(z > 0, z, slope * z).astype(F)
        seg, nseg = (pos.trow, V * L) if mutate == "bucket_softmax" else (pos.v, V)
        keep = np.ones(M, bool)
        if mutate == "drop_message":
            keep[np.flatnonzero(np.bincount(pos.v, minlength=V)[pos.v] >= 2)[0]] = False
        mx = _seg_max(seg[keep], e[keep], nseg).astype(F)
        d = e if mutate == "no_shift" else (e - mx[seg]).astype(F)
        ex = np.where(keep[:, None], np.exp(d), F(0)).astype(F)
        den = seg_sum(seg, ex, nseg)
        alpha = np.where(keep[:, None], np.exp((d - np.log(den)[seg]).astype(F)), F(0)).astype(F)
        if mutate == "head0_alpha":
            alpha = np.repeat(alpha[:, :1], K, axis=1)
        a_cols = alpha[:, hcol]
        out = _seq_sum32(pos.v, a_cols * T[pos.col], V)
        a = _dot32(gout[pos.v], T[pos.col], K)
        c = _dot32(gout, out, K)
        diff = a if mutate == "no_cdot" else a - c[pos.v]
        dprime = np.where(z > 0, F(1), F(1) if mutate == "lrelu_branch" else slope).astype(F)
        dz = ((alpha * diff) * dprime).astype(F)
        if chunked:
            rank = _ranks(pos.v)
            credit = pos.l.copy()
            if mutate == "chunk_neighbour_type":          # the first chunk of the first target with two messages or more
                v0 = np.flatnonzero(np.bincount(pos.v, minlength=V) >= 2)[0]
                hit = (pos.v == v0) & (rank < 64)
                credit[hit] = (credit[hit] + 1) % L
            by = np.argsort(pos.v * L + credit, kind="stable")
            gs_tgt = _tree_sum32((pos.v * L + credit)[by], dz[by], V * L, lane=(rank % 64)[by], chunk=(rank // 64)[by])
        else:
            gs_tgt = _seq_sum32(pos.trow, dz, V * L)
        by = np.argsort(pos.col, kind="stable")
        gT = _seq_sum32(pos.col[by], (a_cols * gout[pos.v])[by], V * L)
        gs_src = _seq_sum32(pos.col[by], dz[by], V * L)
    return dict(z=z, den=den, alpha=alpha, out=out, dz=dz, gT=gT, gs_src=gs_src, gs_tgt=gs_tgt)


def scores32(T, att, L, K, swap=False):
    T = np.asarray(T, F)
    lrow = np.arange(T.shape[0]) % L
    a_s, a_t = _att_halves(np.asarray(att, F), L, K)
    if swap:
        a_s, a_t = a_t, a_s
    return _dot32(T, a_s[lrow], K), _dot32(T, a_t[lrow], K)


def datt32(T, gs_src, gs_tgt, L, K):
    T = np.asarray(T, F)
    R, D = T.shape
    hcol = _heads(D, K)
    halves = []
    for gs in (gs_src, gs_tgt):
        terms = (np.asarray(gs, F)[:, hcol] * T).reshape(R // L, L, K, D // K)
        acc = np.zeros(terms.shape[1:], F)
        for v in range(R // L):
            acc = acc + terms[v]
        halves.append(acc)
    return np.stack(halves, axis=2).reshape(L, 2 * D)


def fold32(gT, gs_src, gs_tgt, att, L, K):
    gT = np.asarray(gT, F)
    hcol, lrow = _heads(gT.shape[1], K), np.arange(gT.shape[0]) % L
    a_s, a_t = _att_halves(np.asarray(att, F), L, K)
    return gT + (np.asarray(gs_src, F)[:, hcol] * a_s[lrow] + np.asarray(gs_tgt, F)[:, hcol] * a_t[lrow])


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
SCORES = ("plain", "extreme")
Inputs = namedtuple("Inputs", "graph msgs T gout s_src s_tgt equal_target zero_target")


def _special_targets(g, msgs):
    """(a target of three messages or more, a target of two or more) whose source rows are disjoint and which share none with a
    one-message target; the second one's first two messages come from different rows"""
    by_target = [np.flatnonzero(msgs.tgt == v) for v in range(g.V)]
    rows = [set(msgs.rows[m].tolist()) for m in by_target]
    single = set().union(*[rows[v] for v in range(g.V) if len(by_target[v]) == 1])
    for a in range(g.V):
        if len(by_target[a]) < 3 or rows[a] & single:
            continue
        for b in range(g.V):
            if b != a and 2 <= len(by_target[b]) <= 17 and len(rows[b]) >= 2 and not rows[b] & (rows[a] | single):
                return a, b
    raise AssertionError("no pair of targets with disjoint source rows in " + g.name)


@functools.lru_cache(maxsize=None)
def _master(name, scores):
    g = graph(name)
    msgs = S.messages(g.adj, g.V, "transformed")
    rng = np.random.default_rng([GRAPHS.index(name), 31])
    T = S._signed(rng, (g.V * g.L, D_MAX))
    gout = S._signed(rng, (g.V, D_MAX))
    rng = np.random.default_rng([GRAPHS.index(name), 32, SCORES.index(scores)])
    top = 64 if scores == "plain" else 60 * 64                        # multiples of 2^-6 in [-1, 1] or [-60, 60]
    s_src, s_tgt = ((rng.integers(-top, top + 1, size=(g.V * g.L, K_MAX)) / 64.0).astype(np.float32) for _ in range(2))
    equal = zero = -1
    if scores == "extreme":
        equal, zero = _special_targets(g, msgs)
        pos = positions(msgs)
        # all logits of `equal` are the same number; `zero` sees z == -0.0 (-0 + -0) from its first source row and +0.0 (+0 + -0)
        # from its second
        of = pos.v == equal
        s_src[pos.col[of]] = np.float32(-17.25)
        s_tgt[pos.trow[of]] = np.float32(3.5)
        of = np.flatnonzero(pos.v == zero)
        first = pos.col[of[0]]
        second = pos.col[of][pos.col[of] != first][0]
        s_tgt[pos.trow[of]] = np.float32(-0.0)
        s_src[first], s_src[second] = np.float32(-0.0), np.float32(0.0)
    for a in (T, gout, s_src, s_tgt):
        a.setflags(write=False)
    return g, msgs, T, gout, s_src, s_tgt, equal, zero


def inputs(name, D, K, scores="plain"):
    """The seeded inputs of one case: the first D columns of T and gout and the first K columns of the score tables of (graph,
    value set).  Columns are independent draws."""
    assert D <= D_MAX and K <= K_MAX
    g, msgs, T, gout, s_src, s_tgt, equal, zero = _master(name, scores)
    return Inputs(g, msgs, np.array(T[:, :D]), np.array(gout[:, :D]), np.array(s_src[:, :K]), np.array(s_tgt[:, :K]), equal, zero)


# (D, K) -> the seed of att for which every z of the fused-score cases clears its margin (found by trying 0, 1, 2, ...)
FUSED_CASES = ((32, 8), (32, 2), (64, 16), (64, 4), (128, 32), (128, 8), (256, 16), (256, 4))
FUSED_SEEDS = {}
Fused = namedtuple("Fused", "graph msgs T gout att s_src s_tgt z_err")


@functools.lru_cache(maxsize=None)
def fused_inputs(name, D, K):
    """The inputs of a fused-score case: att [L, 2D] with magnitudes in [1/32, 1/8]; the float64 score tables (Sum64) and z_err [M, K],
    the bound on the error of the kernel's z before its own add.  Asserts that every float64 z is farther from 0 than the bound on
    the float32 z's error (preactivation_margin-style), so that lrelu' cannot take another branch than float64's."""
    g, msgs, T, gout = _master(name, "plain")[:4]
    T, gout = np.array(T[:, :D]), np.array(gout[:, :D])
    rng = np.random.default_rng([GRAPHS.index(name), 33, D, K, FUSED_SEEDS.get((name, D, K), 0)])
    att = (S._signed(rng, (g.L, 2 * D)) / np.float32(16.0)).astype(np.float32)
    s_src, s_tgt = scores64(T, att, g.L, K)
    pos = positions(msgs)
    z_err = bound(s_src.k, s_src.sum_abs)[pos.col] + bound(s_tgt.k, s_tgt.sum_abs)[pos.trow]
    z = s_src.value[pos.col] + s_tgt.value[pos.trow]
    margin = z_err + U * np.abs(z) + 4.0 * np.spacing(np.maximum(np.abs(z), 1e-30).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(z) > margin), "%s D=%d K=%d: a z within its float32 error of 0; take another seed" % (name, D, K)
    return Fused(g, msgs, T, gout, att, s_src, s_tgt, z_err)


# ---- the cases of tests/test_gpu_rgat_kernels.py (tests/test_rgat_reference_cpu.py restates each) ------------------------
# (graph, D, K, route); route: "dz" fast forward + rgat_dz_kernel, "logits" fast forward + rgat_bwd_logits_kernel, "generic"
DZ_WIDTHS = ((16, 4), (64, 8), (64, 4), (32, 1), (256, 4), (256, 2), (256, 1))              # Dh4 = 1, 2, 4, 8, 16, 32, 64
LOGITS_WIDTHS = ((320, 4), (96, 2), (48, 1), (512, 2), (1024, 8))
GENERIC_WIDTHS = ((96, 3), (64, 16), (256, 16), (20, 5), (120, 6), (384, 3), (1024, 16))
CASES = tuple(
    [("main", D, K, "dz") for D, K in DZ_WIDTHS]
    + [(name, D, 4, "dz") for name in ("hub", "chunks") for D in (64, 256)]
    + [(name, D, K, "logits") for name in ("main", "hub") for D, K in LOGITS_WIDTHS]
    + [("main", D, K, "generic") for D, K in GENERIC_WIDTHS]
    + [(name, D, K, "generic") for name in ("hub", "chunks") for D, K in ((96, 3), (120, 6))]
    + [("sixteen_types", 64, 4, "dz"), ("many_types", 64, 4, "dz"), ("many_types", 128, 8, "dz"), ("many_types", 64, 2, "dz")])
EXTREME_CASES = tuple((name, D, K, route) for name in ("main", "hub") for D, K, route in ((64, 4, "dz"), (96, 2, "logits"), (96, 3, "generic")))


@functools.lru_cache(maxsize=4)
def reference(name, D, K, scores="plain", order=None):
    """(inputs, positions, Attention64) of a case; order: the graph's own by-target permutation as a tuple"""
    case = inputs(name, D, K, scores)
    pos = positions(case.msgs, None if order is None else np.array(order))
    return case, pos, attention64(pos, case.T, case.s_src, case.s_tgt, K, SLOPE, case.gout)
