"""Keeps tests/seg_reduce_reference.py honest without a GPU: its float64 sums and its float32 max rule against float64 autograd
through oracle.torch_ref.unsorted_segment, and — on every graph and input set tests/test_gpu_seg_reduce_backward.py uses —
that dropping any ONE term of any reference sum moves the result by more than 4x (hub graph: 2x) the bound the kernels are
held to.  The second property is what makes `bound` a test rather than a formality."""
import numpy as np
import pytest
import torch

import seg_reduce_reference as R
from helpers import random_relational_graph
from oracle import torch_ref

WEIGHTED = [False, True]


def _autograd64(msgs, X, w_t, gout, mode):
    Xr = torch.as_tensor(np.asarray(X, np.float64)).requires_grad_(True)
    w = torch.as_tensor(R.weights_by_message(msgs, w_t).astype(np.float64))
    data = w.unsqueeze(1) * Xr.index_select(0, torch.as_tensor(msgs.rows))
    out = torch_ref.unsorted_segment(mode, data, torch.as_tensor(msgs.tgt), msgs.num_out)
    out.backward(torch.as_tensor(np.asarray(gout, np.float64)))
    return out.detach().numpy(), Xr.grad.numpy()


def _close(a, b):
    return np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("mode", R.MODES)
def test_references_match_float64_autograd(mode, weighted, kind):
    rng = np.random.default_rng(3)
    V, L, D = 40, 3, 6
    # (target_rows: every message of a target carries the same row, so the whole segment ties: keep the segments short)
    adj = random_relational_graph(rng, V, L, [150, 0, 60]) if kind != "target_rows" else \
        random_relational_graph(rng, V, L, [50, 0, 20], heavy_tail=False)
    msgs = R.messages(adj, V, kind)
    if mode == "max":
        # products, counts and quotients that are exact in float32, so that the float32 rule and float64 autograd must agree:
        # halves times {0.5, 1, 1.5, 2}, and gradients that are multiples of 840/1024 (divisible by every tie count up to 8)
        X = (rng.integers(1, 5, size=(msgs.num_rows, D)) * rng.choice([-0.5, 0.5], size=(msgs.num_rows, D))).astype(np.float32)
        w_t = rng.choice(np.array([0.5, 1.0, 1.5, 2.0], np.float32), size=len(msgs.tgt)) if weighted else None
        gout = (rng.integers(1, 20, size=(V, D)) * rng.choice([-1.0, 1.0], size=(V, D)) * 840.0 / 1024.0).astype(np.float32)
        got = R.max_fwd_bwd32(msgs, X, w_t, gout)
        assert 2 <= got.count.max() <= 8                      # forced ties, the exact division holds
        out, grad = _autograd64(msgs, X, w_t, gout, mode)
        nonempty = np.bincount(msgs.tgt, minlength=V) > 0                         # (an empty segment is the dtype's lowest)
        assert np.array_equal(got.out[nonempty].astype(np.float64), out[nonempty])
        assert (got.out[~nonempty] == R.F32_LOWEST).all() and (got.count[~nonempty] == 0).all()
        assert _close(got.grad.value, grad)
        assert np.array_equal(got.grad.k > 0, got.grad.sum_abs > 0)
        return
    X = rng.standard_normal((msgs.num_rows, D)).astype(np.float32)
    gout = rng.standard_normal((V, D)).astype(np.float32)
    w_t = R.degree_scale_by_target(adj, V)[0] if weighted else None
    out, grad = _autograd64(msgs, X, w_t, gout, mode)
    fwd, bwd = R.reduce_fwd64(msgs, X, w_t, mode), R.reduce_bwd64(msgs, w_t, gout, mode)
    assert _close(fwd.value, out) and _close(bwd.value, grad)
    assert np.all(np.abs(fwd.value) <= fwd.sum_abs * (1 + 1e-12)) and np.all(fwd.min_abs[fwd.k > 0] * fwd.k[fwd.k > 0] <= fwd.sum_abs[fwd.k > 0] * (1 + 1e-12))
    assert np.array_equal(fwd.k[:, 0], np.bincount(msgs.tgt, minlength=V)) and np.array_equal(bwd.k[:, 0], np.bincount(msgs.rows, minlength=msgs.num_rows))


def test_degree_scale_is_the_reference_formula():
    from oracle import bookkeeping
    g = R.graph("main")
    w_t, deg = R.degree_scale_by_target(g.adj, g.V)
    assert np.array_equal(deg, bookkeeping.in_degree_table(g.adj, g.V).astype(np.float32))
    msgs = R.messages(g.adj, g.V)
    assert np.array_equal(R.weights_by_message(msgs, w_t), np.float32(1.0) / (deg[msgs.typ, msgs.tgt] + np.float32(1e-7)))


@pytest.mark.parametrize("name", ["tanh", "relu", "leaky_relu", "elu", "selu", "gelu"])
def test_activation_references(name):
    x = np.concatenate([np.linspace(-6, 6, 1201), [1e-30, -1e-30, 30.0, -30.0]])
    xr = torch.as_tensor(x).requires_grad_(True)
    y = torch_ref.activation(name)(xr)
    y.sum().backward()
    a, d = R.act64(name, x)
    assert _close(a, y.detach().numpy()) and _close(d, xr.grad.numpy())
    assert np.all(np.abs(d) <= R.LIPSCHITZ[name])
    if name in R.EPILOGUE_ACTIVATIONS:
        nz = x != 0
        assert np.all(np.abs(R.dact_from_output64(name, a) - d)[nz] <= 1e-12)
        # the float32 restatement is the float64 formula rounded: y * y, the subtraction and the product with g, half an ulp each
        y32 = a.astype(np.float32)
        g32 = np.linspace(-2, 2, len(x)).astype(np.float32)
        want = R.dact_from_output64(name, y32) * g32.astype(np.float64)
        got = R.act_bwd_from_output32(name, y32, g32).astype(np.float64)
        assert np.all(np.abs(got - want) <= 3 * R.U * np.maximum(np.abs(g32), np.abs(want)))


def test_bound_is_the_stated_formula():
    assert R.bound(1, 1.0) == 4 * 2.0 ** -24 and R.bound(65, 2.0) == 68 * 2.0 ** -23
    assert np.array_equal(R.bound(np.array([0, 5]), np.array([3.0, 0.0])), [9 * 2.0 ** -24, 0.0])


# ---- the graphs ---------------------------------------------------------------------------------------------------------
def _degrees(g):
    msgs = R.messages(g.adj, g.V)
    return np.bincount(msgs.tgt, minlength=g.V), np.bincount(msgs.rows, minlength=g.V * g.L)


def test_main_graph_covers_the_stated_degrees():
    g = R.graph("main")
    assert (g.V, g.L) == (97, 3) and len(g.adj[1]) == 0 and len(g.adj[0]) > 0 and len(g.adj[2]) > 0
    indeg, outdeg = _degrees(g)
    assert indeg.sum() <= 2000
    assert set(R.IN_DEGREES) <= set(indeg.tolist()) and indeg.max() == 17       # capped: the sensitivity check needs it
    assert set(R.OUT_DEGREES) <= set(outdeg.tolist()) and outdeg.max() <= 6
    assert all(a.dtype == np.int32 and a.min(initial=0) >= 0 and a.max(initial=0) < g.V for a in g.adj)


def test_hub_graph_has_the_long_buckets():
    g = R.graph("hub")
    assert (g.V, g.L) == (97, 3) and len(g.adj[1]) == 0
    indeg, outdeg = _degrees(g)
    assert indeg.sum() <= 2000
    for n in (63, 64, 65):
        assert (indeg == n).sum() == 2
    assert (indeg == 130).sum() == 1 and (indeg == 0).sum() >= 1
    assert {15, 16, 17} <= set(indeg.tolist())
    assert sorted(outdeg[outdeg > 16].tolist()) == list(R.HUB_SOURCE_ROWS)       # two by-source buckets the hub route chunks


# ---- one dropped term must show -----------------------------------------------------------------------------------------
def _assert_sensitive(res, factor, what):
    has = res.k > 0
    assert has.any(), what
    ratio = res.min_abs[has] / R.bound(res.k[has], res.sum_abs[has])
    assert ratio.min() > factor, "%s: a single term moves the sum by only %.2f x its bound" % (what, ratio.min())


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind,weighted", [("transformed", False), ("transformed", True), ("untransformed", False),
                                           ("untransformed", True), ("messages", False), ("target_rows", False)])
@pytest.mark.parametrize("name,factor", [("main", 4.0), ("hub", 2.0)])
def test_one_dropped_term_exceeds_the_bound(name, factor, kind, weighted, mode):
    """At D_MAX columns, of which every GPU case takes a prefix.  (plan_messages / plan_target_rows carry no weights.)"""
    case = R.inputs(name, R.D_MAX, kind, halves=(mode == "max"))
    w_t = case.w_t if weighted else None
    what = "%s/%s/%s/%s" % (name, kind, mode, "w" if weighted else "-")
    if mode == "max":
        _assert_sensitive(R.max_fwd_bwd32(case.msgs, case.X, w_t, case.gout).grad, factor, what + " gradient")
        return
    _assert_sensitive(R.reduce_fwd64(case.msgs, case.X, w_t, mode), factor, what + " forward")
    _assert_sensitive(R.reduce_bwd64(case.msgs, w_t, case.gout, mode), factor, what + " gradient")


@pytest.mark.parametrize("weighted", WEIGHTED)
def test_max_inputs_hold_every_kind_of_tie(weighted):
    case = R.inputs("main", 64, halves=True)
    w_t = case.w_t if weighted else None
    got = R.max_fwd_bwd32(case.msgs, case.X, w_t, case.gout)
    assert (got.count == 2).any() and (got.count == 3).any() and (got.count[np.bincount(case.msgs.tgt, minlength=97) == 0] == 0).all()
    if weighted:
        w = R.weights_by_message(case.msgs, w_t)
        mixed = 0
        for v in range(case.graph.V):
            m = np.flatnonzero(case.msgs.tgt == v)
            for d in range(64):
                ws = w[m][got.win[m, d]]
                mixed += len(ws) > 1 and ws.min() != ws.max()
        assert mixed > 10                                         # ties between messages of different weight
        # and a product that rounds (w = float32(1/3)) wins somewhere: the compare sees a rounded product
        assert got.win[w == np.float32(1.0 / 3.0)].any()


@pytest.mark.parametrize("mode", R.SUM_MODES)
def test_epilogue_preactivations_stay_clear_of_the_kink(mode):
    """The activation-epilogue cases (D = 50, 64, 256: the first 256 columns): no float64 pre-activation is so close to 0 that
    the float32 sum could land within four ulps of it, so the GPU test's excluded share is 0 for these inputs."""
    case = R.inputs("main", 256)
    res = R.reduce_fwd64(case.msgs, case.X, case.w_t, mode)
    has = res.k > 0
    assert np.all(np.abs(res.value[has]) > R.preactivation_margin(res)[has])
