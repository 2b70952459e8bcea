"""The RGAT attention kernels (csrc/rgat_fast.hip, csrc/rgat.hip, csrc/rgat_scores.hip) at the op level, one case per route and
kernel class, against plain float64 (tests/rgat_reference.py).

Every quantity — alpha, out, dz, gT, gs_src, gs_tgt, the score tables, d att and the folded gT — is compared element by element
with float64 under the bound rgat_reference derives for it; tests/test_rgat_reference_cpu.py shows on these very inputs that honest
float32 arithmetic lies inside those bounds and that a list of plausible mistakes does not.  alpha and dz never leave the op, so
_pieces() launches the kernels with the arguments of ops/rgat.py into NaN-filled buffers, and the op itself (run twice: there are
no atomics in these files, so bit-identical) must give the very bits of those launches.  Every case asserts the route it is meant
to take from the predicates of ops/rgat.py, so that a change to the gates cannot silently empty a row of this table.

Which case reaches which kernel ((D, K) on the `main` graph unless said):
  rgat_alpha_kernel<1|2|4|8>                 every "dz" and "logits" case: (32,1) (256,2) (64,4) (64,8); targets over 64 messages on
                                             `hub` / `chunks` (the three-pass loop); the extreme logits
  headw_reduce_kernel<NCH,K,HAS_Z=false>     forward of the same cases: NCH = 1 up to D = 256, 2 at (320,4) (512,2), 4 at (1024,8);
                                             as the gT pass under RELGNN_RGAT_FUSED_SUMS=0
  headw_reduce_kernel<NCH,K,HAS_Z=true>      their gT pass with gs_src riding along; by-source buckets of 20 / 40 on `hub`, 70 on `chunks`
  rgat_dz_kernel<K>, fused gs_tgt            head_sum at Dh4 = 1 (16,4), 2 (64,8), 4 (64,4), 8 (32,1), 16 (256,4), 32 (256,2), 64 (256,1);
                                             the chunk walk on `hub` and `chunks`; L K == 64: `sixteen_types` (64,4); empty types:
                                             `many_types` (64,2)
  rgat_dz_kernel<K>, gs_tgt = NULL           L K > 64: `many_types` (64,4) = 92, (128,8) = 184, gs_tgt from the segment reduce;
                                             RELGNN_RGAT_FUSED_SUMS=0
  rgat_bwd_logits_kernel<G,NCH,POW2=false>   "logits": G = 16 (48,1), 32 (96,2), 64 x 2 (320,4) (512,2), 64 x 4 (1024,8); "generic":
                                             32 (120,6), 64 x 2 (384,3), 64 x 4 (1024,16)
  rgat_bwd_logits_kernel<G,1,POW2=true>      "generic": G = 8 (20,5), 16 (64,16), 32 (96,3), 64 (256,16)
  rgat_fwd_kernel / rgat_bwd_msg_kernel      "generic": <8,1> (20,5), <16,1> (64,16), <32,1> (96,3) (120,6), <64,1> (256,16),
                                             <64,2> (384,3), <64,4> (1024,16); (96,3) (120,6) on `hub` and `chunks` too
  rgat_scores_fwd / bwd_rows / bwd_att<G>    G = 8 (32,8) (32,2), 16 (64,16) (64,4), 32 (128,32) (128,8), 64 (256,16) (256,4); K == G:
                                             one lane per head; V = 97 and 23: no multiple of 256 / G lane groups per workgroup
  gnns.rgat._attention_from_segment_ops      test_hub_safe_composition
  sparse_rgat_layer -> the generic route     test_layer_reaches_the_generic_route

Each test prints the largest error / bound per quantity it saw (pytest -s, or -rP)."""
import numpy as np
import pytest
import torch

import rgat_reference as R
from helpers import rgcn_weights, set_switch

pytestmark = pytest.mark.gpu

SLOPE = R.SLOPE
_GRAPHS = {}


def _graph(name, device, split=False):
    """(RelGraph, Positions in the graph's own by-target order, that order as a tuple) of a reference graph, built once"""
    from tf_gnn_samples_amd.graph import RelGraph
    key = (name, str(device), split)
    if key not in _GRAPHS:
        ref = R.graph(name)
        g = RelGraph([torch.as_tensor(a, device=device) for a in ref.adj], ref.V)
        assert not g.has_long_buckets
        if split:
            assert g.split_long_segments(threshold=16) and g.has_long_buckets
        order = g.perm_t.cpu().numpy().astype(np.int64)
        pos = R.positions(R.S.messages(ref.adj, ref.V), order)
        np.testing.assert_array_equal(g.col_t.cpu().numpy(), pos.col)
        np.testing.assert_array_equal(g.rowptr_t.cpu().numpy(), np.r_[0, np.cumsum(np.bincount(pos.trow, minlength=ref.V * ref.L))])
        _GRAPHS[key] = (g, pos, tuple(order.tolist()))
    return _GRAPHS[key]


def _route(D, K):
    from tf_gnn_samples_amd.ops import rgat
    if not rgat._rgat_fast_ok(D, K):
        return "generic"
    return "dz" if rgat._rgat_dz_fast_ok(D, K) else "logits"


def _assert_within(got, want, tol, what):
    """|got - want| <= tol element-wise; a miss is reported with its element, the reference value and the ratio to the bound.
    Returns the largest error / bound."""
    got = np.asarray(got, np.float64)
    want = want.value if isinstance(want, R.Sum64) else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite values" % (what, (~np.isfinite(got)).sum())
    err = np.abs(got - want)
    bad = err > tol
    if bad.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bad, err / tol, 0.0)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %.9g, reference %.17g, error %.3g = %.2f x bound"
                             % (what, bad.sum(), bad.size, at, got[at], want[at], err[at], ratio[at]))
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


QUANTITIES = ("alpha", "out", "dz", "gT", "gs_src", "gs_tgt")


def _assert_attention(got, ref, what, only=QUANTITIES):
    ratios = {q: _assert_within(got[q], getattr(ref, q), getattr(ref, q + "_tol"), "%s %s" % (what, q)) for q in only}
    print("error / bound  %-44s %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    return ratios


def _nan(shape, device):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=device)


def _pieces(T, s_src, s_tgt, g, K, gout, fuse=True):
    """The launches of ops.rgat._RgatAttention with its arguments, every output starting as NaN: alpha and dz next to what the op
    returns.  Returns the tensors and the route taken."""
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.ops.segment import _seg_reduce_raw
    V, L, M, D, dev, p = g.V, g.L, g.M, T.shape[1], T.device, _lib.ptr
    out, alpha, dz = _nan((V, D), dev), _nan((M, K), dev), _nan((M, K), dev)
    gT, gs_src, gs_tgt = _nan((V * L, D), dev), _nan((V * L, K), dev), _nan((V * L, K), dev)
    route = _route(D, K)
    if route != "generic":
        _lib.launch("relgnn_rgat_alpha", p(s_src), p(s_tgt), K, p(g.rowptr_t), V, L, p(g.col_t), SLOPE, p(alpha))
        _lib.launch("relgnn_headw_reduce", p(T), V * L, D, D, K, p(g.rowptr_t), V, L, p(g.col_t), p(alpha), None, p(out), D, None, None)
    else:
        _lib.launch("relgnn_rgat_fwd", p(T), D, D, K, p(s_src), p(s_tgt), p(g.rowptr_t), V, L, p(g.col_t), SLOPE, p(out), D, p(alpha))
    if route == "dz":
        fuse_t = fuse and L * K <= 64
        _lib.launch("relgnn_rgat_dz", p(T), V * L, D, D, K, p(s_src), p(s_tgt), p(g.rowptr_t), V, L, p(g.col_t), SLOPE, p(alpha), p(out),
                    p(gout), D, p(dz), p(gs_tgt) if fuse_t else None)
        if not fuse_t:
            gs_tgt = _seg_reduce_raw(_lib.AGG_SUM, dz, g.rowptr_t, 1, g.iota, None, V * L)
    else:
        _lib.launch("relgnn_rgat_bwd_logits", p(T), D, D, K, p(s_src), p(s_tgt), p(g.rowptr_t), V, L, p(g.col_t), SLOPE, p(alpha), p(out),
                    p(gout), D, p(dz), p(gs_tgt))
    if route != "generic":
        _lib.launch("relgnn_headw_reduce", p(gout), V, D, D, K, p(g.rowptr_s), V * L, 1, p(g.tgt_s), p(alpha), p(g.pos_t_of_s), p(gT), D,
                    p(dz) if fuse else None, p(gs_src) if fuse else None)
        if not fuse:
            gs_src = _seg_reduce_raw(_lib.AGG_SUM, dz, g.rowptr_s, 1, g.pos_t_of_s, None, V * L)
    else:
        _lib.launch("relgnn_rgat_bwd_msg", D, K, p(g.rowptr_s), V * L, p(g.tgt_s), p(g.pos_t_of_s), p(alpha), p(dz), p(gout), D, p(gT), D,
                    p(gs_src))
    return dict(alpha=alpha, out=out, dz=dz, gT=gT, gs_src=gs_src, gs_tgt=gs_tgt)


def _twice(fn, leaves, gout):
    """out = fn(*leaves) and its gradients, twice: bit-identical, or the test fails here.  Before each pass NaN-filled blocks of the
    outputs' sizes go back to the allocator (best effort: the allocator decides), so that an element a kernel does not write would
    show as NaN instead of a lucky zero."""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        poison = [torch.full(tuple(t.shape), float("nan"), device=t.device) for t in leaves] + [torch.full_like(gout, float("nan"))]
        del poison
        out = fn(*leaves)
        poison = [torch.full(tuple(t.shape), float("nan"), device=t.device) for t in leaves]
        del poison
        out.backward(gout)
        runs.append([out.detach().clone()] + [t.grad.clone() for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs of the same op differ"
    return runs[0]


def _run_attention(device, name, D, K, scores="plain", fuse=True):
    """The op twice, the launches once, the same bits from both; returns (inputs, positions, reference, the launches' results)"""
    from tf_gnn_samples_amd import ops
    g, pos, order = _graph(name, device)
    case, pos, ref = R.reference(name, D, K, scores, order)
    T, s_src, s_tgt, gout = (torch.as_tensor(x, device=device) for x in (case.T, case.s_src, case.s_tgt, case.gout))
    got = _pieces(T, s_src, s_tgt, g, K, gout, fuse)
    leaves = [t.clone().requires_grad_(True) for t in (T, s_src, s_tgt)]
    op = _twice(lambda a, b, c: ops.rgat_attention(a, b, c, g, K, SLOPE), leaves, gout)
    for q, t in zip(("out", "gT", "gs_src", "gs_tgt"), op):
        assert torch.equal(t, got[q]), "%s: the op and the launches with its arguments differ" % q
    return case, pos, ref, {q: t.cpu().numpy() for q, t in got.items()}


# ---- every route, every kernel class ------------------------------------------------------------------------------------
# (D, K) -> (G, NCH, POW2) of csrc/rgat.hip, as the table above states them
GEOMETRY = {(320, 4): (64, 2, False), (96, 2): (32, 1, False), (48, 1): (16, 1, False), (512, 2): (64, 2, False), (1024, 8): (64, 4, False),
            (96, 3): (32, 1, True), (64, 16): (16, 1, True), (256, 16): (64, 1, True), (20, 5): (8, 1, True), (120, 6): (32, 1, False),
            (384, 3): (64, 2, False), (1024, 16): (64, 4, False)}


def _geometry(D, K):
    """pick_geo and the POW2 gate of relgnn_rgat_bwd_logits (csrc/rgat.hip), restated"""
    d4, dh4 = D // 4, D // K // 4
    G, nch = next((g, n) for top, g, n in ((8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (256, 64, 4)) if d4 <= top)
    assert K <= G
    return G, nch, nch == 1 and dh4 & (dh4 - 1) == 0 and G % dh4 == 0


@pytest.mark.parametrize("name,D,K,route", R.CASES, ids=lambda x: str(x))
def test_attention_routes(gpu_device, name, D, K, route):
    L = R.graph(name).L
    assert _route(D, K) == route
    if route == "dz":
        dh4 = D // K // 4
        assert D <= 256 and dh4 & (dh4 - 1) == 0
        assert (L * K <= 64) == ((name, D, K) not in (("many_types", 64, 4), ("many_types", 128, 8)))       # fused gs_tgt or not
    else:
        assert _geometry(D, K) == GEOMETRY[(D, K)]
    case, pos, ref, got = _run_attention(gpu_device, name, D, K)
    _assert_attention(got, ref, "%s (%d,%d) %s" % (name, D, K, route))
    assert (ref.n == 0).any() and (got["out"][ref.n == 0] == 0).all()                       # no message: exactly zero
    assert (got["gs_tgt"][np.bincount(pos.trow, minlength=pos.V * pos.L) == 0] == 0).all()    # an empty bucket: exactly zero
    assert (got["gT"][np.bincount(pos.col, minlength=pos.V * pos.L) == 0] == 0).all()
    assert (got["alpha"][ref.n[pos.v] == 1] == 1.0).all()


@pytest.mark.parametrize("flag", ["0", "1"])
def test_fused_sums_switch_each_against_float64(gpu_device, monkeypatch, flag):
    """RELGNN_RGAT_FUSED_SUMS: gs_tgt inside the dz pass and gs_src inside the gT pass (1), or two segment reduces over dz (0);
    each held to float64 on its own"""
    from tf_gnn_samples_amd import config
    set_switch(monkeypatch, "RELGNN_RGAT_FUSED_SUMS", flag)
    assert config.settings.rgat_fused_sums == flag and _route(256, 4) == "dz"
    case, pos, ref, got = _run_attention(gpu_device, "hub", 256, 4, fuse=flag == "1")
    _assert_attention(got, ref, "hub (256,4) RELGNN_RGAT_FUSED_SUMS=" + flag)


# ---- the softmax at the edge of float32 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,K,route", R.EXTREME_CASES, ids=lambda x: str(x))
def test_extreme_logits(gpu_device, name, D, K, route):
    assert _route(D, K) == route
    case, pos, ref, got = _run_attention(gpu_device, name, D, K, "extreme")
    what = "%s (%d,%d) %s extreme" % (name, D, K, route)
    _assert_attention(got, ref, what)                                                       # (asserts that everything is finite)
    alpha, n = got["alpha"], ref.n[pos.v]
    assert (n == 1).any() and (alpha[n == 1] == 1.0).all()                                   # one message: exactly 1
    eq = pos.v == case.equal_target
    assert eq.sum() >= 3
    _assert_within(alpha[eq], np.full((eq.sum(), K), 1.0 / eq.sum()), ref.alpha_tol[eq], what + " all-equal logits")
    under = ref.alpha < R.FLT_MIN
    assert under.any() and (np.abs(alpha[under] - ref.alpha[under]) <= R.FLT_MIN * 1.001).all()   # underflow: the absolute floor
    total = np.zeros((pos.V, K))
    np.add.at(total, pos.v, alpha.astype(np.float64))
    has = ref.n > 0
    # whatever the logits, the alphas of a target add up to 1: the n-term sum, and A per expf (terms), logf and expf (result)
    tol = (ref.n[has, None] + 2) * R.U + R.ACT_ALLOWANCE * (2 + np.maximum(1.0, np.log(ref.n[has, None]))) + np.zeros((1, K))
    print("error / bound  %-44s sum of alpha %.3f" % (what, _assert_within(total[has], np.ones((has.sum(), K)), tol, what + " sum of alpha")))
    assert (got["out"][~has] == 0).all() and (got["gs_tgt"].reshape(pos.V, -1)[~has] == 0).all()
    zero = pos.v == case.zero_target
    z32 = (case.s_src[pos.col] + case.s_tgt[pos.trow])[zero]
    assert ((z32 == 0) & np.signbit(z32)).any() and ((z32 == 0) & ~np.signbit(z32)).any()


# ---- score kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", R.FUSED_CASES)
def test_score_kernels_on_their_own(gpu_device, D, K):
    """relgnn_rgat_scores_fwd and relgnn_rgat_scores_bwd with given gs_src / gs_tgt / gT: the tables, d att (group partials, then
    column_sum) and the in-place fold, each against float64 with nothing propagated"""
    from tf_gnn_samples_amd import _lib, ops
    from tf_gnn_samples_amd.dense import column_sum
    assert ops.rgat_scores_supported(D, K)
    f = R.fused_inputs("main", D, K)
    V, L = f.graph.V, f.graph.L
    assert V % (256 // (D // 4)) != 0
    T, att = torch.as_tensor(f.T, device=gpu_device), torch.as_tensor(f.att, device=gpu_device)
    s_src, s_tgt = _nan((V * L, K), gpu_device), _nan((V * L, K), gpu_device)
    _lib.launch("relgnn_rgat_scores_fwd", _lib.ptr(T), D, D, K, _lib.ptr(att), L, V, _lib.ptr(s_src), _lib.ptr(s_tgt))
    ratios = {}
    for q, got, want in (("s_src", s_src, f.s_src), ("s_tgt", s_tgt, f.s_tgt)):
        ratios[q] = _assert_within(got.cpu().numpy(), want, R.bound(want.k, want.sum_abs), "scores (%d,%d) %s" % (D, K, q))
    rng = np.random.default_rng([D, K])
    gs, gt, g0 = R.S._signed(rng, (V * L, K)), R.S._signed(rng, (V * L, K)), R.S._signed(rng, (V * L, D))
    gs_d, gt_d, gT = (torch.as_tensor(x, device=gpu_device) for x in (gs, gt, g0))
    groups = int(_lib.load_library().relgnn_rgat_scores_groups(V))
    partial = _nan((groups, L * 2 * D), gpu_device)
    _lib.launch("relgnn_rgat_scores_bwd", _lib.ptr(T), D, D, K, _lib.ptr(att), L, V, _lib.ptr(gs_d), _lib.ptr(gt_d), _lib.ptr(gT), D,
                _lib.ptr(partial), groups)
    gatt = column_sum(partial).view(L, 2 * D)
    want, tol = R.datt64(f.T, gs, gt, L, K)
    ratios["d att"] = _assert_within(gatt.cpu().numpy(), want, tol, "scores (%d,%d) d att" % (D, K))
    want, tol = R.fold64(g0, gs, gt, f.att, L, K)
    ratios["fold"] = _assert_within(gT.cpu().numpy(), want, tol, "scores (%d,%d) fold" % (D, K))
    print("error / bound  scores (%d,%d) %s" % (D, K, "  ".join("%s %.3f" % kv for kv in ratios.items())))


@pytest.mark.parametrize("D,K", R.FUSED_CASES)
@pytest.mark.parametrize("name", ["main", "chunks"])
def test_layer_attention_with_fused_scores(gpu_device, name, D, K):
    """ops.rgat_layer_attention: tables, softmax, weighted sum and their gradients as one node; the errors of the computed tables
    carried into alpha's bound, those of gs_src / gs_tgt into d att and the folded gT"""
    from tf_gnn_samples_amd import ops
    assert ops.rgat_scores_supported(D, K)
    f = R.fused_inputs(name, D, K)
    g, pos, _ = _graph(name, gpu_device)
    L = g.L
    z_err = R.bound(f.s_src.k, f.s_src.sum_abs)[pos.col] + R.bound(f.s_tgt.k, f.s_tgt.sum_abs)[pos.trow]
    ref = R.attention64(pos, f.T, f.s_src.value, f.s_tgt.value, K, SLOPE, f.gout, z_err=z_err)
    leaves = [torch.as_tensor(x, device=gpu_device).requires_grad_(True) for x in (f.T, f.att)]
    out, gT, gatt = _twice(lambda a, b: ops.rgat_layer_attention(a, b, g, K, SLOPE), leaves, torch.as_tensor(f.gout, device=gpu_device))
    what = "%s (%d,%d) %s fused scores" % (name, D, K, _route(D, K))
    ratios = {"out": _assert_within(out.cpu().numpy(), ref.out, ref.out_tol, what + " out")}
    want, tol = R.fold64(ref.gT.value, ref.gs_src.value, ref.gs_tgt.value, f.att, L, K, ref.gT_tol, ref.gs_src_tol, ref.gs_tgt_tol)
    ratios["gT"] = _assert_within(gT.cpu().numpy(), want, tol, what + " folded gT")
    want, tol = R.datt64(f.T, ref.gs_src.value, ref.gs_tgt.value, L, K, ref.gs_src_tol, ref.gs_tgt_tol)
    ratios["d att"] = _assert_within(gatt.cpu().numpy(), want, tol, what + " d att")
    print("error / bound  %-44s %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))


# ---- the hub-safe composition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(64, 4), (96, 3)])
def test_hub_safe_composition(gpu_device, D, K):
    """gnns.rgat._attention_from_segment_ops on the hub graph with its long buckets split (threshold 16): the same float64 values,
    forward and — through autograd — gradients.  Its index_add gradients use atomics: no bit-identity is asked of it; and it takes
    <gout, out> as a sum over messages, which rgat_reference allows for in dz_composed."""
    from tf_gnn_samples_amd.gnns.rgat import _attention_from_segment_ops
    g, pos, order = _graph("hub", gpu_device, split=True)
    case, pos, ref = R.reference("hub", D, K, "plain", order)
    leaves = [torch.as_tensor(x, device=gpu_device).requires_grad_(True) for x in (case.T, case.s_src, case.s_tgt)]
    out = _attention_from_segment_ops(*leaves, g, K, SLOPE)
    out.backward(torch.as_tensor(case.gout, device=gpu_device))
    got = dict(out=out.detach().cpu().numpy(), gT=leaves[0].grad.cpu().numpy(), gs_src=leaves[1].grad.cpu().numpy(),
               gs_tgt=leaves[2].grad.cpu().numpy())
    rows = pos.V * pos.L
    composed = ref._replace(gs_src_tol=ref.gs_src_tol + R._seg_sum(pos.col, ref.dz_composed, rows),
                            gs_tgt_tol=ref.gs_tgt_tol + R._seg_sum(pos.trow, ref.dz_composed, rows))
    _assert_attention(got, composed, "hub (%d,%d) from segment ops" % (D, K), only=("out", "gT", "gs_src", "gs_tgt"))


# ---- the public API reaches the generic route ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(96, 3), (256, 16)])
def test_layer_reaches_the_generic_route(gpu_device, D, K):
    from oracle import torch_ref
    from test_gpu_layers import _dev, _grad_check, _graph as _layer_graph
    from tf_gnn_samples_amd.gnns import sparse_rgat_layer
    from tf_gnn_samples_amd.graph import as_rel_graph
    assert _route(D, K) == "generic"
    rng, adj, deg = _layer_graph(11)
    V, L = 150, 3
    w = rgcn_weights(rng, L, D, D)
    for l in range(L):
        w["Edge_%i_Attention_Parameters" % l] = (rng.standard_normal(2 * D) * 0.3).astype(np.float32)
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    adj_d, adj_c = _dev(adj, gpu_device), [torch.as_tensor(a) for a in adj]
    assert not as_rel_graph(adj_d, V).has_long_buckets                  # the attention kernels, not the composition
    _grad_check(lambda x, ww: sparse_rgat_layer(x, adj_d, D, K, 1, "tanh", weights=ww),
                lambda x, ww: torch_ref.sparse_rgat_layer(x, adj_c, D, K, 1, "tanh", weights=ww), h, w, gpu_device)


# ---- shapes the C side rejects ------------------------------------------------------------------------------------------
def test_more_heads_than_lanes_is_refused(gpu_device):
    """K = 128 at D = 512 is legal for the layer (Dh = 4) but the generic kernels keep one lane per head (K <= G = 64): the binding's
    error, not uninitialised output"""
    from tf_gnn_samples_amd import ops
    D, K = 512, 128
    g, pos, _ = _graph("main", gpu_device)
    assert _route(D, K) == "generic"
    T = torch.zeros((g.V * g.L, D), device=gpu_device)
    s = torch.zeros((g.V * g.L, K), device=gpu_device)
    with pytest.raises(ValueError, match="relgnn_rgat_fwd"):
        ops.rgat_attention(T, s, s.clone(), g, K, SLOPE)
