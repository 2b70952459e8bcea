"""The gradient side of csrc/seg_reduce.hip, one case per kernel class, against plain float64 (tests/seg_reduce_reference.py).

Every comparison with float64 is held to bound(k, sum|term|) = (k + 3) * 2^-24 * sum|term| of the element's own sum — derived,
not tuned; tests/test_seg_reduce_reference_cpu.py shows on these very inputs that one dropped term exceeds it four times (hub
graph: twice).  Where an activation is evaluated, 3e-7 * max(1, |value|) per evaluation is added (the figure of
tests/test_gpu_activations.py), scaled by what multiplies the activation downstream.  Every gradient is computed twice and must
be bit-identical: there are no atomics anywhere in the file under test.

Which case reaches which kernel:
  seg_max_count_kernel / seg_max_bwd_kernel (scalar)        test_max_gradient at D = 7, 50, 70, 130
  seg_max_count_vec_kernel<G> / seg_max_bwd_vec_kernel<G>   test_max_gradient: G = 8 at D = 4, 16, 32; 16 at 36, 64; 32 at 68, 128;
                                                            64 at 132 .. 1028 (1028: the chunk loop runs five times, ragged)
  seg_reduce_scalar_kernel                                  forward of D = 7, 50, 70, 130 and of the misaligned view, all four modes,
                                                            weighted and not; its gradient use (weighted) at the same widths;
                                                            with the epilogue: test_activation_epilogue at D = 50
  seg_reduce_group_kernel<8|16|32> / wave_kernel<1|2|4>     the other widths, forward and (over the transposed plan) gradient; with
                                                            segments of 63 .. 65 and 130: test_long_segments_in_every_kernel_class
  msg_act_bwd_kernel, MSGACT group / wave kernels           test_message_activation_inside_the_reduce
  act_bwd_from_output_kernel                                test_act_bwd_from_output_bit_for_bit, test_activation_epilogue
  the eight RELGNN_SEG_VARIANT instantiations               test_seg_variants_never_change_results"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import seg_reduce_reference as R
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
VECTOR_WIDTHS = [4, 32, 36, 64, 68, 128, 132, 256, 260, 1028]
SCALAR_WIDTHS = [7, 50, 70, 130]
# "64@misaligned": D = 64 as the column view wide[:, 1:65] (data_ptr() % 16 != 0: the scalar forward kernel by alignment);
# "16@strided":    D = 16 as wide[:, :16] of a 24-column tensor (the vector kernels with a row stride)
WIDTHS = VECTOR_WIDTHS + SCALAR_WIDTHS + ["64@misaligned", "16@strided"]

_GRAPHS = {}


def _graph(name, device, split=False):
    """(RelGraph, degree-scale weights by target) of a reference graph, built once; split: with chunked long buckets."""
    from tf_gnn_samples_amd.graph import RelGraph
    key = (name, str(device), split)
    if key not in _GRAPHS:
        ref = R.graph(name)
        g = RelGraph([torch.as_tensor(a, device=device) for a in ref.adj], ref.V)
        w_t, deg = R.degree_scale_by_target(ref.adj, ref.V)
        w = g.degree_scale(torch.as_tensor(deg, device=device))
        np.testing.assert_array_equal(w.cpu().numpy(), w_t)            # same values in the same by-target order
        if split:
            assert g.split_long_segments(threshold=16)
        _GRAPHS[key] = (g, w)
    return _GRAPHS[key]


def _plan(g, kind, w):
    if kind in ("transformed", "untransformed"):
        return getattr(g, "plan_" + kind)(w)
    assert w is None
    return getattr(g, "plan_" + kind)()


def _place(X, width, device):
    """(leaf, operand, columns): the tensor that receives the gradient, the view handed to the op, the leaf's columns it covers.
    The columns of `wide` outside the view hold NaN: a kernel that read them would show it."""
    if not isinstance(width, str):
        leaf = torch.as_tensor(X, device=device).requires_grad_(True)
        return leaf, leaf, slice(None)
    D, layout = int(width.split("@")[0]), width.split("@")[1]
    cols, total = (slice(1, D + 1), D + 4) if layout == "misaligned" else (slice(0, D), 24)
    wide = np.full((X.shape[0], total), np.nan, np.float32)
    wide[:, cols] = X
    leaf = torch.as_tensor(wide, device=device).requires_grad_(True)
    view = leaf[:, cols]
    assert view.stride(0) % 4 == 0 and (view.data_ptr() % 16 != 0) == (layout == "misaligned")
    return leaf, view, cols


def _width(width):
    return width if not isinstance(width, str) else int(width.split("@")[0])


def _fwd_bwd(fn, leaf, gout):
    """out = fn(), then its gradient into `leaf` twice: bit-identical, or the test fails here."""
    grads = []
    for _ in range(2):
        leaf.grad = None
        out = fn()
        # gX comes from torch.empty: poison what the allocator is likely to hand out next (best effort: the allocator decides),
        # so that a row the kernel does not write would show as NaN instead of a lucky zero
        poison = torch.full(tuple(leaf.shape), float("nan"), device=leaf.device)
        del poison
        out.backward(gout)
        grads.append(leaf.grad.clone())
    assert torch.equal(grads[0], grads[1]), "two runs of the same gradient differ"
    return out.detach().cpu().numpy(), grads[0].cpu().numpy()


def _assert_within(got, want, tol, what):
    """|got - want| <= tol element-wise; a miss is reported with its element, the reference value and the ratio to the bound."""
    got = np.asarray(got, np.float64)
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


def _assert_sum(got, res, what, extra=0.0):
    return _assert_within(got, res.value, R.bound(res.k, res.sum_abs) + extra, what)


def _oracle_fold(case, X, w_t, mode):
    """the oracle's sequential float32 fold in the reference's message order (tf.unsorted_segment_* on CPU)"""
    data = X[case.msgs.rows]
    if w_t is not None:
        data = R.weights_by_message(case.msgs, w_t)[:, None] * data
    return T.get_aggregation_function(mode)(data.astype(np.float32), case.msgs.tgt.astype(np.int32), case.graph.V)


# ---- sum / mean / sqrt_n ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.SUM_MODES)
@pytest.mark.parametrize("width", WIDTHS, ids=str)
def test_sum_like_gradient(gpu_device, width, mode):
    from tf_gnn_samples_amd import ops
    D = _width(width)
    case = R.inputs("main", D)
    g, w = _graph("main", gpu_device)
    gout = torch.as_tensor(case.gout, device=gpu_device)
    no_edge = np.bincount(case.msgs.rows, minlength=case.msgs.num_rows) == 0
    assert no_edge.any()
    for w_dev, w_t in ((None, None), (w, case.w_t)):
        what = "D=%s %s %s" % (width, mode, "weighted" if w_t is not None else "unweighted")
        leaf, view, cols = _place(case.X, width, gpu_device)
        out, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, g.plan_transformed(w_dev), mode), leaf, gout)
        fwd = R.reduce_fwd64(case.msgs, case.X, w_t, mode)
        if D % 4 == 0 and width != "64@misaligned":
            np.testing.assert_array_equal(out, _oracle_fold(case, case.X, w_t, mode), err_msg=what)   # bit for bit
        _assert_sum(out, fwd, what + " forward")
        _assert_sum(grad[:, cols], R.reduce_bwd64(case.msgs, w_t, case.gout, mode), what + " gradient")
        assert (grad[:, cols][no_edge] == 0.0).all()                  # rows without an outgoing edge: exactly 0.0
        if isinstance(width, str):                                    # the columns outside the view receive no gradient
            outside = np.ones(grad.shape[1], bool)
            outside[cols] = False
            assert (grad[:, outside] == 0.0).all()


# ---- max ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("width", WIDTHS, ids=str)
def test_max_gradient(gpu_device, width, weighted):
    from tf_gnn_samples_amd import ops
    D = _width(width)
    case = R.inputs("main", D, halves=True)
    g, _ = _graph("main", gpu_device)
    w_t = case.w_t if weighted else None
    w_dev = torch.as_tensor(case.w_t, device=gpu_device) if weighted else None
    what = "D=%s max %s" % (width, "weighted" if weighted else "unweighted")
    leaf, view, cols = _place(case.X, width, gpu_device)
    out, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, g.plan_transformed(w_dev), "max"), leaf,
                         torch.as_tensor(case.gout, device=gpu_device))
    grad = grad[:, cols]
    ref = R.max_fwd_bwd32(case.msgs, case.X, w_t, case.gout)
    np.testing.assert_array_equal(out, ref.out, err_msg=what)                       # the float32 maxima, bit for bit
    _assert_sum(grad, ref.grad, what + " gradient")
    # an empty segment: float32 lowest forward, and no gradient comes out of it
    empty = np.bincount(case.msgs.tgt, minlength=case.graph.V) == 0
    assert empty.any() and (out[empty] == R.F32_LOWEST).all() and (ref.count[empty] == 0).all()
    # a k-way tie splits gout / k equally: where a row wins exactly once, its gradient IS w * (gout / k), the one float32 product
    w_msg = R.weights_by_message(case.msgs, w_t)
    gsel = np.where(ref.count > 0, case.gout / np.maximum(ref.count, 1), 0).astype(np.float32)
    for k in (1, 2, 3):
        m, d = np.nonzero(ref.win & (ref.count[case.msgs.tgt] == k) & (ref.grad.k[case.msgs.rows] == 1))
        assert len(m) > 0, "no %d-way tie with a single-winner row at %s" % (k, what)
        np.testing.assert_array_equal(grad[case.msgs.rows[m], d], (w_msg[m] * gsel[case.msgs.tgt[m], d]).astype(np.float32))
    # a row that wins nowhere, and a row with no outgoing edge at all: exactly 0.0
    assert (grad[ref.grad.k == 0] == 0.0).all()
    no_edge = np.bincount(case.msgs.rows, minlength=case.msgs.num_rows) == 0
    assert no_edge.any() and (grad[no_edge] == 0.0).all()


@pytest.mark.parametrize("D", [64, 50], ids=["vector", "scalar"])
def test_max_count_pass_on_its_own(gpu_device, D):
    """relgnn_seg_max_count: gsel = gout / #winners as ONE float32 division, 0 for an empty segment."""
    from tf_gnn_samples_amd import _lib, ops
    case = R.inputs("main", D, halves=True)
    g, _ = _graph("main", gpu_device)
    w = torch.as_tensor(case.w_t, device=gpu_device)
    plan = g.plan_transformed(w)
    X, gout = torch.as_tensor(case.X, device=gpu_device), torch.as_tensor(case.gout, device=gpu_device)
    out = ops.seg_gather_reduce(X, plan, "max")
    gsel = torch.full_like(gout, float("nan"))
    _lib.launch("relgnn_seg_max_count", _lib.ptr(X), D, D, _lib.ptr(plan.rowptr), plan.num_out, plan.stride, _lib.ptr(plan.col),
                _lib.ptr(plan.w), _lib.ptr(out), _lib.ptr(gout), D, _lib.ptr(gsel))
    ref = R.max_fwd_bwd32(case.msgs, case.X, case.w_t, case.gout)
    want = np.where(ref.count > 0, case.gout / np.maximum(ref.count, 1), 0).astype(np.float32)
    np.testing.assert_array_equal(gsel.cpu().numpy(), want)
    assert (want[np.bincount(case.msgs.tgt, minlength=case.graph.V) == 0] == 0).all()


# ---- the other plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 132])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind,weighted", [("untransformed", False), ("untransformed", True), ("messages", False), ("target_rows", False)])
def test_other_plans_forward_and_gradient(gpu_device, kind, weighted, mode, D):
    from tf_gnn_samples_amd import ops
    is_max = mode == "max"
    case = R.inputs("main", D, kind, halves=is_max)
    g, w = _graph("main", gpu_device)
    w_t = case.w_t if weighted else None
    w_dev = None if not weighted else (torch.as_tensor(case.w_t, device=gpu_device) if is_max else w)
    plan = _plan(g, kind, w_dev)
    assert plan.num_rows_x == case.msgs.num_rows and plan.num_out == case.graph.V
    what = "plan_%s %s D=%d%s" % (kind, mode, D, " weighted" if weighted else "")
    leaf, view, _ = _place(case.X, D, gpu_device)
    out, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, plan, mode), leaf, torch.as_tensor(case.gout, device=gpu_device))
    if is_max:
        ref = R.max_fwd_bwd32(case.msgs, case.X, w_t, case.gout)
        np.testing.assert_array_equal(out, ref.out, err_msg=what)
        _assert_sum(grad, ref.grad, what + " gradient")
    else:
        _assert_sum(out, R.reduce_fwd64(case.msgs, case.X, w_t, mode), what + " forward")
        _assert_sum(grad, R.reduce_bwd64(case.msgs, w_t, case.gout, mode), what + " gradient")


# ---- long segments, one wave each ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("width", [4, 64, 128, 256, 260, 1028, 50])
def test_long_segments_in_every_kernel_class(gpu_device, width, mode):
    """The hub graph without the split: targets of 63, 64, 65 and 130 messages (the 64-message index batch of the wave kernels and
    their unroll-8 tail, several index batches of every group size, the four-at-a-time tail of the max passes) and by-source
    buckets of 20 and 40 for the gradient, in each forward class: group 8 / 16 / 32, wave 1 / 2 / 4 chunks, scalar."""
    from tf_gnn_samples_amd import ops
    is_max = mode == "max"
    case = R.inputs("hub", width, halves=is_max)
    g, w = _graph("hub", gpu_device)
    w_dev = torch.as_tensor(case.w_t, device=gpu_device) if is_max else w
    what = "hub graph D=%d %s" % (width, mode)
    leaf, view, _ = _place(case.X, width, gpu_device)
    out, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, g.plan_transformed(w_dev), mode), leaf,
                         torch.as_tensor(case.gout, device=gpu_device))
    if is_max:
        ref = R.max_fwd_bwd32(case.msgs, case.X, case.w_t, case.gout)
        np.testing.assert_array_equal(out, ref.out, err_msg=what)
        _assert_sum(grad, ref.grad, what + " gradient")
        return
    if width % 4 == 0:
        np.testing.assert_array_equal(out, _oracle_fold(case, case.X, case.w_t, mode), err_msg=what)
    _assert_sum(out, R.reduce_fwd64(case.msgs, case.X, case.w_t, mode), what + " forward")
    _assert_sum(grad, R.reduce_bwd64(case.msgs, case.w_t, case.gout, mode), what + " gradient")


# ---- hub route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("mode", R.MODES)
def test_hub_route_gradient(gpu_device, mode, D):
    """split_long_segments(threshold=16): chunks as virtual rows, then the chunks of a bucket combined — still a sum of the same
    terms, so the same bound holds; and the chunked and the one-wave order agree within twice that bound."""
    from tf_gnn_samples_amd import ops
    is_max = mode == "max"
    case = R.inputs("hub", D, halves=is_max)
    grads = []
    for split in (True, False):
        g, w = _graph("hub", gpu_device, split=split)
        by_t, by_s = getattr(g.rowptr_t, "_relgnn_split", {}), getattr(g.rowptr_s, "_relgnn_split", {})
        assert (g.L in by_t and 1 in by_s) == split                      # the forward's and the gradient's bucketing both chunk
        w_dev = torch.as_tensor(case.w_t, device=gpu_device) if is_max else w
        what = "hub %s D=%d %s" % (mode, D, "split" if split else "one wave")
        leaf, view, _ = _place(case.X, D, gpu_device)
        out, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, g.plan_transformed(w_dev), mode), leaf,
                             torch.as_tensor(case.gout, device=gpu_device))
        if is_max:
            ref = R.max_fwd_bwd32(case.msgs, case.X, case.w_t, case.gout)
            np.testing.assert_array_equal(out, ref.out, err_msg=what)
            bwd = ref.grad
        else:
            _assert_sum(out, R.reduce_fwd64(case.msgs, case.X, case.w_t, mode), what + " forward")
            bwd = R.reduce_bwd64(case.msgs, case.w_t, case.gout, mode)
        _assert_sum(grad, bwd, what + " gradient")
        grads.append(grad)
    _assert_within(grads[0], grads[1].astype(np.float64), 2 * R.bound(bwd.k, bwd.sum_abs), "hub %s D=%d split vs one wave" % (mode, D))


# ---- activation epilogue ------------------------------------------------------------------------------------------------
RELU_TYPE = ("relu", "leaky_relu", "elu", "selu")      # a kink (or a jump of the derivative) at 0


@pytest.mark.parametrize("D", [64, 256, 50], ids=["group", "wave", "scalar"])
@pytest.mark.parametrize("mode", R.SUM_MODES)
@pytest.mark.parametrize("act", R.EPILOGUE_ACTIVATIONS)
def test_activation_epilogue(gpu_device, act, mode, D):
    from tf_gnn_samples_amd import ops
    case = R.inputs("main", D)
    g, w = _graph("main", gpu_device)
    what = "epilogue %s %s D=%d" % (act, mode, D)
    leaf, view, _ = _place(case.X, D, gpu_device)
    y, grad = _fwd_bwd(lambda: ops.seg_gather_reduce(view, g.plan_transformed(w), mode, act), leaf,
                       torch.as_tensor(case.gout, device=gpu_device))
    pre = R.reduce_fwd64(case.msgs, case.X, case.w_t, mode)
    want, _ = R.act64(act, pre.value)
    # the sum's own bound, carried through the activation (its largest slope), plus the allowance of the one evaluation
    tol = R.LIPSCHITZ[act] * R.bound(pre.k, pre.sum_abs) + R.ACT_ALLOWANCE * np.maximum(1.0, np.abs(want))
    _assert_within(y, want, tol, what + " forward")
    # gradient: float64 at the kernel's own output y, which is what the kernel differentiates from
    d = R.dact_from_output64(act, y)
    bwd = R.reduce_bwd64(case.msgs, case.w_t, case.gout.astype(np.float64) * d, mode)
    allowance = R.reduce_bwd64(case.msgs, case.w_t, R.ACT_ALLOWANCE * np.maximum(1.0, np.abs(d)) * np.abs(case.gout), mode).sum_abs
    # within four ulps of the kink: the float64 pre-activation is so close to 0 that the float32 sum may sit on either side of it
    # (a ReLU output of exactly 0 far on the negative side is not near the kink)
    near_kink = (np.abs(pre.value) <= R.preactivation_margin(pre)) & (pre.k > 0) & (act in RELU_TYPE)
    share = near_kink.mean()
    assert share < 0.01, "%s: %.2f %% of the outputs within four ulps of the kink" % (what, 100 * share)
    touched = np.zeros(grad.shape, bool)
    np.logical_or.at(touched, case.msgs.rows, near_kink[case.msgs.tgt])
    tol = np.where(touched, np.inf, R.bound(bwd.k, bwd.sum_abs) + allowance)
    _assert_within(grad, bwd.value, tol, what + " gradient")


@pytest.mark.parametrize("act", R.EPILOGUE_ACTIVATIONS)
def test_act_bwd_from_output_bit_for_bit(gpu_device, act):
    """4097 elements (a ragged end of the grid-stride loop), the special outputs, against the float32 restatement."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.dense import act_bwd_from_output
    rng = np.random.default_rng(11)
    n = 4097
    y = rng.uniform(-1.0, 1.0, size=n).astype(np.float32) if act == "tanh" else rng.standard_normal(n).astype(np.float32)
    special = [0.0, -0.0, 1.0, -1.0, 1e-30]
    if act == "elu":
        special.append(-1.0)                                         # -alpha
    if act == "selu":
        special.append(-R.SELU_SCALE_ALPHA / R.SELU_SCALE)           # -alpha
        special.append(-R.SELU_SCALE_ALPHA)                          # the output's own lower limit, -scale * alpha
    y[:len(special)] = np.array(special, np.float32)
    y[-1] = np.float32(0.5)                                          # the last, ragged element is a known one
    gvals = rng.standard_normal(n).astype(np.float32)
    got = act_bwd_from_output(ops.activation_id(act), torch.as_tensor(y, device=gpu_device), torch.as_tensor(gvals, device=gpu_device))
    np.testing.assert_array_equal(got.cpu().numpy(), R.act_bwd_from_output32(act, y, gvals))


def test_epilogue_refusals(gpu_device):
    from tf_gnn_samples_amd import _lib, ops
    case = R.inputs("main", 64)
    g, w = _graph("main", gpu_device)
    X = torch.as_tensor(case.X, device=gpu_device)
    with pytest.raises(ValueError):
        ops.seg_gather_reduce(X, g.plan_transformed(w), "sum", "gelu")
    for act in R.EPILOGUE_ACTIVATIONS:
        with pytest.raises(ValueError):
            ops.seg_gather_reduce(X, g.plan_transformed(w), "max", act)
    y = torch.zeros(16, device=gpu_device)
    rc = _lib.load_library().relgnn_act_bwd_from_output(_lib.ACT_GELU, _lib.ptr(y), _lib.ptr(y), 16, _lib.ptr(torch.empty_like(y)),
                                                        _lib.current_stream())
    assert rc == _lib.EUNSUPPORTED


# ---- per-message activation inside the reduce ---------------------------------------------------------------------------
def _check_message_activation(gpu_device, graph_name, split, act, D, modes=R.SUM_MODES):
    from tf_gnn_samples_amd import ops
    case = R.inputs(graph_name, D, "messages")
    g, w = _graph(graph_name, gpu_device, split=split)
    w_full, _ = R.degree_scale_by_target(case.graph.adj, case.graph.V)
    gout = torch.as_tensor(case.gout, device=gpu_device)
    outs = {}
    for mode in modes:
        for w_dev, w_t in ((None, None), (w, w_full)):
            what = "message %s %s D=%d %s%s" % (act, mode, D, "weighted" if w_t is not None else "unweighted", " hub" if split else "")
            leaf, view, _ = _place(case.X, D, gpu_device)
            out, grad = _fwd_bwd(lambda: ops.message_act_reduce(view, g, w_dev, mode, act), leaf, gout)
            fwd, allowance = R.msgact_fwd64(case.msgs, case.X, w_t, mode, act)
            _assert_sum(out, fwd, what + " forward", extra=allowance)
            ref, tol = R.msgact_bwd64(case.msgs, case.X, w_t, case.gout, mode, act)
            _assert_within(grad, ref, tol, what + " gradient")
            outs[(mode, w_t is not None)] = out
    return case, g, w, outs


@pytest.mark.parametrize("D", [32, 64, 128, 132, 260])
@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_message_activation_inside_the_reduce(gpu_device, act, D):
    """ops.message_act_reduce on the fused pair relgnn_seg_reduce_msgact_fwd / relgnn_msg_act_bwd: the group kernels at
    D = 32, 64, 128 and the wave kernels at 132, 260; six activations x sum / mean / sqrt_n x weighted and not."""
    _check_message_activation(gpu_device, "main", False, act, D)


@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_message_activation_composed_routes(gpu_device, act):
    """The routes around the fused pair hold the same bounds: D % 4 != 0 (D = 50: the scalar kernel over plan_messages, weighted
    in its gradient use) and a graph with hub buckets (chunked)."""
    from tf_gnn_samples_amd import _lib
    _check_message_activation(gpu_device, "main", False, act, 50)
    _check_message_activation(gpu_device, "hub", True, act, 64, modes=("mean",))
    t = torch.zeros((8, 50), device=gpu_device)
    tgt = torch.zeros(8, dtype=torch.int32, device=gpu_device)
    rc = _lib.load_library().relgnn_msg_act_bwd(_lib.ACT_TANH, _lib.ptr(t), 50, None, _lib.ptr(tgt), _lib.ptr(t), 8,
                                                _lib.ptr(torch.empty_like(t)), _lib.current_stream())
    assert rc == _lib.EUNSUPPORTED


@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_message_activation_max_route(gpu_device, act):
    """max takes the composed route (activation, then the max reduce over plan_messages).  max is 1-Lipschitz in every message, so
    the forward is within the largest per-message error of its segment: the activation allowance plus the rounding of w * x carried
    through the activation's largest slope.  The gradient goes to the winner alone; it is compared where the float64 winner leads
    the runner-up by more than twice that error (elsewhere float32 may rightly pick another message)."""
    from tf_gnn_samples_amd import ops
    D = 64
    case = R.inputs("main", D, "messages")
    g, w = _graph("main", gpu_device)
    msgs = case.msgs
    wm = R.weights_by_message(msgs, case.w_t).astype(np.float64)[:, None]
    a, d = R.act64(act, wm * case.X.astype(np.float64))
    err = R.ACT_ALLOWANCE * np.maximum(1.0, np.abs(a)) + R.LIPSCHITZ[act] * R.U * np.abs(wm * case.X)
    V = case.graph.V
    want, tol = np.full((V, D), float(R.F32_LOWEST)), np.zeros((V, D))
    np.maximum.at(want, msgs.tgt, a)
    np.maximum.at(tol, msgs.tgt, err)
    leaf, view, _ = _place(case.X, D, gpu_device)
    out, grad = _fwd_bwd(lambda: ops.message_act_reduce(view, g, w, "max", act), leaf, torch.as_tensor(case.gout, device=gpu_device))
    _assert_within(out, want, tol, "message %s max forward" % act)
    lead = a >= want[msgs.tgt] - 2 * tol[msgs.tgt]                    # messages that could win in float32
    contenders = np.zeros((V, D))
    np.add.at(contenders, msgs.tgt, lead.astype(np.float64))
    clear = contenders[msgs.tgt] == 1
    assert clear.mean() > 0.3
    wfg = wm * case.gout.astype(np.float64)[msgs.tgt]
    ref = np.where(lead, d * wfg, 0.0)
    gtol = R.ACT_ALLOWANCE * np.maximum(1.0, np.abs(d)) * np.abs(wfg) + 3.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    _assert_within(grad, ref, np.where(clear, np.where(lead, gtol, 0.0), np.inf), "message %s max gradient" % act)


def test_message_activation_c_entries(gpu_device):
    """The two C entries called directly give the bits ops.message_act_reduce gives (it adds nothing of its own)."""
    from tf_gnn_samples_amd import _lib, ops
    D, act, mode = 132, "elu", "sqrt_n"
    case, g, w, outs = _check_message_activation(gpu_device, "main", False, act, D, modes=(mode,))
    plan = g.plan_messages()
    X, gout = torch.as_tensor(case.X, device=gpu_device), torch.as_tensor(case.gout, device=gpu_device)
    M = X.shape[0]
    out = torch.empty((case.graph.V, D), device=gpu_device)
    _lib.launch("relgnn_seg_reduce_msgact_fwd", _lib.AGG_SQRT_N, _lib.ACT_ELU, _lib.ptr(X), M, D, D, _lib.ptr(plan.rowptr), case.graph.V,
                plan.stride, _lib.ptr(plan.col), _lib.ptr(w), _lib.ptr(out), D)
    np.testing.assert_array_equal(out.cpu().numpy(), outs[(mode, True)])
    n = torch.as_tensor(np.maximum(np.bincount(case.msgs.tgt, minlength=case.graph.V), 1).astype(np.float32), device=gpu_device)
    gagg = (gout * (1.0 / torch.sqrt(n)).unsqueeze(1)).contiguous()
    w_orig = torch.as_tensor(R.weights_by_message(case.msgs, case.w_t), device=gpu_device)
    tgt = torch.as_tensor(case.msgs.tgt.astype(np.int32), device=gpu_device)
    gX = torch.empty_like(X)
    _lib.launch("relgnn_msg_act_bwd", _lib.ACT_ELU, _lib.ptr(X), D, _lib.ptr(w_orig), _lib.ptr(tgt), _lib.ptr(gagg), M, _lib.ptr(gX))
    leaf = X.clone().requires_grad_(True)
    ops.message_act_reduce(leaf, g, w, mode, act).backward(gout)
    assert torch.equal(gX, leaf.grad)


# ---- RELGNN_SEG_VARIANT -------------------------------------------------------------------------------------------------
_VARIANT_CHILD = r"""
import os, sys
import numpy as np, torch
assert os.environ["RELGNN_SEG_VARIANT"] == sys.argv[2]
from tf_gnn_samples_amd import ops
from tf_gnn_samples_amd.graph import RelGraph
z = np.load(sys.argv[1])
dev = torch.device("cuda:0")
L = int(z["L"])
g = RelGraph([torch.as_tensor(z["adj%d" % l], device=dev) for l in range(L)], int(z["V"]))
plan = g.plan_transformed(torch.as_tensor(z["w"], device=dev))
bad = 0
for D in (132, 256):
    X = torch.as_tensor(z["X%d" % D], device=dev)
    for mode in ("sum", "mean", "sqrt_n"):
        out = ops.seg_gather_reduce(X, plan, mode).cpu().numpy()
        want = z["out_%s_%d" % (mode, D)]
        if not (out.view(np.uint32) == want.view(np.uint32)).all():
            bad += 1
            print("variant", sys.argv[2], mode, D, "differs in", int((out != want).sum()), "elements")
sys.exit(1 if bad else 0)
"""


def _write_variant_baseline(gpu_device, tmp_path):
    """Weighted sum / mean / sqrt_n at D = 132 and 256 (the one-chunk wave kernel, the only one the variants replace) on the
    default instantiation, on the hub graph: segment lengths 15, 16, 17 (unroll-16 tail), 63, 64, 65 and 130."""
    from tf_gnn_samples_amd import ops
    assert os.environ.get("RELGNN_SEG_VARIANT", "0") in ("", "0")
    g, w = _graph("hub", gpu_device)
    ref = R.graph("hub")
    blobs = {"V": ref.V, "L": ref.L, "w": w.cpu().numpy()}
    blobs.update({"adj%d" % l: a for l, a in enumerate(ref.adj)})
    for D in (132, 256):
        case = R.inputs("hub", D)
        blobs["X%d" % D] = case.X
        X = torch.as_tensor(case.X, device=gpu_device)
        for mode in R.SUM_MODES:
            out = ops.seg_gather_reduce(X, g.plan_transformed(w), mode).cpu().numpy()
            np.testing.assert_array_equal(out, _oracle_fold(case, case.X, case.w_t, mode))
            blobs["out_%s_%d" % (mode, D)] = out
    path = tmp_path / "baseline.npz"
    np.savez(path, **blobs)
    return path


@pytest.mark.parametrize("variant", range(1, 9))
def test_seg_variants_never_change_results(gpu_device, tmp_path, variant):
    """unroll 4 / 16, non-temporal streams, no XCD swizzle: a fresh process per value (the library reads the variable once)."""
    variant_baseline = _write_variant_baseline(gpu_device, tmp_path)
    env = dict(os.environ, RELGNN_SEG_VARIANT=str(variant))
    done = subprocess.run([sys.executable, "-c", _VARIANT_CHILD, str(variant_baseline), str(variant)], env=env, cwd=str(ROOT),
                          timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "RELGNN_SEG_VARIANT=%d: exit %d\n%s\n%s" % (variant, done.returncode, done.stdout[-2000:], done.stderr[-2000:])
