"""Keeps tests/rgat_reference.py honest without a GPU, on the very inputs tests/test_gpu_rgat_kernels.py uses: its float64 values
against float64 autograd; its float32 restatement inside every bound for every element of every quantity (nothing excluded); each
of a list of plausible mistakes, made in that restatement, beyond 4x the bound (hub graph: 2x) somewhere; and the extreme logits
overflowing a softmax without the max shift.  The mistakes are what makes the bounds a test rather than a formality."""
import numpy as np
import pytest
import torch

import rgat_reference as R

QUANTITIES = ("alpha", "out", "dz", "gT", "gs_src", "gs_tgt")


def _value(x):
    return x.value if isinstance(x, R.Sum64) else x


def _worst(got, want, tol):
    """the largest error / bound; inf where an element with bound 0 is not exact or a value is not finite"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - _value(want))
    if (err[tol == 0] > 0).any():
        return np.inf
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def _ratios(ref, got):
    return {q: _worst(got[q], getattr(ref, q), getattr(ref, q + "_tol")) for q in QUANTITIES}


def _restate(name, D, K, route, scores="plain", mutate=None):
    case, pos, ref = R.reference(name, D, K, scores)
    got = R.restate32(pos, case.T, case.s_src, case.s_tgt, K, R.SLOPE, case.gout, tree=route != "generic",
                      chunked=route == "dz" and pos.L * K <= 64, mutate=mutate)
    return case, pos, ref, got


# ---- the float64 formulas -----------------------------------------------------------------------------------------------
def test_references_match_float64_autograd():
    """the op written with torch's own leaky_relu / exp / index_add in float64, through the fused scores: every value of
    attention64, scores64, datt64 and fold64 (dz: the gradient of the retained z)"""
    D, K = 24, 3
    g = R.graph("chunks")
    L = g.L
    pos = R.positions(R.S.messages(g.adj, g.V))
    rng = np.random.default_rng(5)
    T = rng.standard_normal((g.V * L, D))
    att = rng.standard_normal((L, 2 * D))
    gout = rng.standard_normal((g.V, D))
    Tt, at = torch.as_tensor(T).requires_grad_(True), torch.as_tensor(att).requires_grad_(True)
    a4 = at.view(L, K, 2, D // K)
    t4 = Tt.view(g.V, L, K, D // K)
    s_src = (t4 * a4[:, :, 0]).sum(-1).reshape(g.V * L, K)
    s_tgt = (t4 * a4[:, :, 1]).sum(-1).reshape(g.V * L, K)
    col, v, trow = (torch.as_tensor(x) for x in (pos.col, pos.v, pos.trow))
    z = s_src[col] + s_tgt[trow]
    z.retain_grad()
    e = torch.nn.functional.leaky_relu(z, float(np.float32(R.SLOPE)))
    ex = torch.exp(e - e.max())                                     # any shift common to a target cancels; so does a global one
    alpha = ex / torch.zeros(g.V, K, dtype=torch.float64).index_add(0, v, ex)[v]
    msg = (alpha.unsqueeze(2) * Tt[col].view(-1, K, D // K)).reshape(-1, D)
    out = torch.zeros(g.V, D, dtype=torch.float64).index_add(0, v, msg)
    out.backward(torch.as_tensor(gout))

    def close(a, b):
        return np.all(np.abs(_value(a) - b.detach().numpy()) <= 1e-11 * np.maximum(1.0, np.abs(b.detach().numpy())))
    s64 = R.scores64(T, att, L, K)
    assert close(s64[0], s_src) and close(s64[1], s_tgt)
    ref = R.attention64(pos, T, s64[0].value, s64[1].value, K, R.SLOPE, gout, z_err=np.zeros((pos.M, K)))
    assert close(ref.z, z) and close(ref.alpha, alpha) and close(ref.out, out) and close(ref.dz, z.grad)
    assert close(R.datt64(T, ref.gs_src.value, ref.gs_tgt.value, L, K)[0], at.grad)
    assert close(R.fold64(ref.gT.value, ref.gs_src.value, ref.gs_tgt.value, att, L, K)[0], Tt.grad)
    n = np.bincount(pos.v, minlength=g.V)
    assert np.array_equal(ref.n, n) and np.array_equal(ref.out.k[:, 0], n) and np.array_equal(ref.gs_tgt.k[:, 0], np.bincount(pos.trow, minlength=g.V * L))
    assert np.all(np.abs(_seg(pos.v, ref.alpha, g.V)[n > 0] - 1.0) < 1e-12)


def _seg(index, x, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, index, x)
    return out


# ---- the graphs and value sets ------------------------------------------------------------------------------------------
def test_graphs_hold_what_the_cases_need():
    for name in ("many_types", "sixteen_types"):
        g = R.graph(name)
        pos = R.positions(R.S.messages(g.adj, g.V))
        assert (g.V, g.L) == R.TYPED[name][:2] and 55 <= g.V <= 65 and g.V % 4 != 0
        used = np.array([len(set(pos.l[pos.v == v])) for v in range(g.V)])
        assert (g.L - used >= 3).all() and used.max() >= 8              # several empty types per target, and many used ones
        assert {0, 1} <= set(np.bincount(pos.v, minlength=g.V).tolist())
    assert R.graph("many_types").L * 4 == 92 and R.graph("sixteen_types").L * 4 == 64 and R.graph("many_types").L * 2 == 46
    g = R.graph("chunks")
    pos = R.positions(R.S.messages(g.adj, g.V))
    assert g.V % 4 != 0 and g.L == 4 and pos.M <= 2000
    lengths = np.bincount(pos.trow, minlength=g.V * g.L).reshape(g.V, g.L)
    assert np.array_equal(lengths[:len(R.CHUNK_TARGETS)], R.CHUNK_TARGETS) and not lengths[len(R.CHUNK_TARGETS):].any()
    total, cum = lengths.sum(1), np.cumsum(lengths, 1)
    inside = [v for v in range(g.V) if total[v] > 64 and 64 not in cum[v]]
    between = [v for v in range(g.V) if total[v] > 64 and 64 in cum[v]]
    after_empty = [v for v in range(g.V) if total[v] > 64 and not lengths[v, :2].any()]
    assert inside and between and after_empty
    assert {n % 64 % 8 for n in total} == set(range(8)) and {0, 1} <= set(total.tolist())       # the unroll-8 loop and its tail
    same = pos.v == R.SAME_ROW_TARGET
    assert same.sum() == 70 and len(set(pos.col[same])) == 1
    for name in ("main", "hub"):
        n = np.bincount(R.S.messages(R.graph(name).adj, 97).tgt, minlength=97)
        assert {0, 1} <= set(n.tolist())


@pytest.mark.parametrize("name", ["main", "hub"])
def test_value_sets(name):
    plain, extreme = R.inputs(name, 64, R.K_MAX), R.inputs(name, 64, R.K_MAX, "extreme")
    for case, top in ((plain, 1.0), (extreme, 60.0)):
        for s in (case.s_src, case.s_tgt):
            assert np.array_equal(s * 64, np.round(s * 64)) and np.abs(s).max() <= top
    assert np.abs(plain.T).min() >= 0.5 and np.abs(plain.T).max() <= 2.0 and np.abs(plain.gout).min() >= 0.5
    pos = R.positions(extreme.msgs)
    z = extreme.s_src[pos.col] + extreme.s_tgt[pos.trow]                          # float32, and exact
    assert np.array_equal(z.astype(np.float64), extreme.s_src.astype(np.float64)[pos.col] + extreme.s_tgt.astype(np.float64)[pos.trow])
    assert z.max() > 100 and z.min() < -100
    eq = z[pos.v == extreme.equal_target]
    assert len(eq) >= 3 and (eq == eq[0, 0]).all()
    zz = z[pos.v == extreme.zero_target]
    assert ((zz == 0) & np.signbit(zz)).any() and ((zz == 0) & ~np.signbit(zz)).any()
    ref = R.reference(name, 64, 4, "extreme")[2]
    assert ((ref.alpha < R.FLT_MIN) & (ref.alpha > 0)).any() and (ref.alpha[ref.n[pos.v] == 1] == 1.0).all()


# ---- honest float32 lies inside every bound -----------------------------------------------------------------------------
ALL_CASES = [c + ("plain",) for c in R.CASES] + [c + ("extreme",) for c in R.EXTREME_CASES]


@pytest.mark.parametrize("name,D,K,route,scores", ALL_CASES, ids=lambda x: str(x))
def test_restatement_lies_inside_every_bound(name, D, K, route, scores):
    case, pos, ref, got = _restate(name, D, K, route, scores)
    ratios = _ratios(ref, got)
    assert max(ratios.values()) <= 1.0, ratios
    n = ref.n[pos.v]
    assert (got["alpha"][n == 1] == 1.0).all()                       # one message: exp(0 - log 1)
    assert (got["out"][ref.n == 0] == 0).all()


@pytest.mark.parametrize("D,K", R.FUSED_CASES)
@pytest.mark.parametrize("name", ["main", "chunks"])
def test_fused_restatement_lies_inside_every_bound(name, D, K):
    f = R.fused_inputs(name, D, K)
    L = f.graph.L
    pos = R.positions(f.msgs)
    s32 = R.scores32(f.T, f.att, L, K)
    for got, want in zip(s32, (f.s_src, f.s_tgt)):
        assert _worst(got, want, R.bound(want.k, want.sum_abs)) <= 1.0
    ref = R.attention64(pos, f.T, f.s_src.value, f.s_tgt.value, K, R.SLOPE, f.gout, z_err=f.z_err)
    got = R.restate32(pos, f.T, s32[0], s32[1], K, R.SLOPE, f.gout, tree=K in (1, 2, 4, 8), chunked=K in (1, 2, 4, 8))
    ratios = _ratios(ref, got)
    datt, datt_tol = R.datt64(f.T, ref.gs_src.value, ref.gs_tgt.value, L, K, ref.gs_src_tol, ref.gs_tgt_tol)
    ratios["d att"] = _worst(R.datt32(f.T, got["gs_src"], got["gs_tgt"], L, K), datt, datt_tol)
    fold, fold_tol = R.fold64(ref.gT.value, ref.gs_src.value, ref.gs_tgt.value, f.att, L, K, ref.gT_tol, ref.gs_src_tol, ref.gs_tgt_tol)
    ratios["fold"] = _worst(R.fold32(got["gT"], got["gs_src"], got["gs_tgt"], f.att, L, K), fold, fold_tol)
    assert max(ratios.values()) <= 1.0, ratios


# ---- the bounds see mistakes --------------------------------------------------------------------------------------------
# mutation -> the quantity it must show in
SHOWS_IN = {"drop_message": "out", "bucket_softmax": "alpha", "head0_alpha": "out", "no_cdot": "dz", "lrelu_branch": "dz",
            "chunk_neighbour_type": "gs_tgt"}


@pytest.mark.parametrize("mutate", R.MUTATIONS)
@pytest.mark.parametrize("name,factor", [("main", 4.0), ("hub", 2.0)])
def test_mutations_exceed_the_bound(name, factor, mutate):
    assert set(SHOWS_IN) == set(R.MUTATIONS)
    case, pos, ref, got = _restate(name, 64, 4, "dz", mutate=mutate)
    assert (case.s_src + case.s_tgt < 0).any()
    ratio = _ratios(ref, got)[SHOWS_IN[mutate]]
    assert ratio > factor, "%s on %s: only %.2f x the bound in %s" % (mutate, name, ratio, SHOWS_IN[mutate])


@pytest.mark.parametrize("name,factor", [("main", 4.0), ("hub", 2.0)])
def test_swapped_att_halves_exceed_the_bound(name, factor):
    f = R.fused_inputs(name, 64, 4)
    got = R.scores32(f.T, f.att, f.graph.L, 4, swap=True)
    for g32, want in zip(got, (f.s_src, f.s_tgt)):
        assert _worst(g32, want, R.bound(want.k, want.sum_abs)) > factor


@pytest.mark.parametrize("name,D,K,route", R.EXTREME_CASES, ids=lambda x: str(x))
def test_extreme_logits_see_a_missing_max_shift(name, D, K, route):
    case, pos, ref, got = _restate(name, D, K, route, "extreme", mutate="no_shift")
    assert not np.isfinite(got["den"][ref.n > 0]).all()
    assert _ratios(ref, got)["alpha"] > 4.0


@pytest.mark.parametrize("D,K", R.FUSED_CASES)
def test_one_dropped_term_exceeds_the_score_bounds(D, K):
    """the inputs of test_score_kernels_on_their_own: one node's term missing from d att, or one of the fold's three, is beyond 4x
    the bound of every element (the kernels stay far inside: a sequential sum of 97 signed terms rarely comes near its bound)"""
    f = R.fused_inputs("main", D, K)
    V, L = f.graph.V, f.graph.L
    rng = np.random.default_rng([D, K])
    gs, gt, g0 = R.S._signed(rng, (V * L, K)), R.S._signed(rng, (V * L, K)), R.S._signed(rng, (V * L, D))
    for res, tol in (R.datt64(f.T, gs, gt, L, K), R.fold64(g0, gs, gt, f.att, L, K)):
        assert (res.min_abs / tol).min() > 4.0
    for res in (f.s_src, f.s_tgt):
        assert (res.min_abs / R.bound(res.k, res.sum_abs)).min() > 4.0
