"""The aggregate-first RGCN layer: gather from the SMALL table, then one K = L*Din product (two kernels, or the fused one of
csrc/rgcn_fused.hip)."""
from typing import Optional

import torch

from .. import _lib, dense as DN
from ..activations import FUSABLE_ACTS as _FUSABLE_ACTS, activation_id, apply_activation, get_activation
from ..config import settings as _cfg
from ..graph import split_plan_of
from ..handover import handover_word
from ..weight_grad_stream import fork
from .segment import ROUTES, _mode_factor, _raw_sum_gradient, _seg_reduce_raw, aggregation_mode_id, rowmax_supported


def aggregate_acc64() -> bool:
    """RELGNN_AGG_ACC=f32|f64: accumulator width of the bucket sums that feed the K = L*D GEMM of the aggregate-first order.
    Measured at the full C2 batch (profiles/r03_parity_margin.json): float64 accumulators change the distance to the oracle from
    6.2e-6 to 6.0e-6 and the distance to the float64 truth from 4.8e-6 to 5.1e-6 — the bucket sums are NOT where the
    aggregate-first order spends its error budget (the K = 768 dot products are), so the default stays the float32 kernel."""
    return _cfg.agg_acc == "f64"


def _weight_gradient(agg, gsc, amax, L: int):
    """agg^T @ gsc (agg [V, L*Din]: the bucket sums, gsc [V, Dout]).  On the two-fp16-limb route (RELGNN_LIMB=pair: `amax`, the
    forward gather's per-bucket magnitudes [V*L], says the layer took it) the operands go behind exact power-of-two scales that
    factor out of the product: gsc one per COLUMN (gradient columns differ by decades and Adam normalises every weight by its own
    history: relgnn_col_absmax_f32, one streaming pass over [V, Dout]), agg one per EDGE TYPE — the largest of that type's bucket
    magnitudes, a reduction over the [V, L] table the gather already wrote.  (One magnitude per column of agg as well would cost a
    pass over the [V, L*Din] sums — 110 MB at C2, measured +50 us per layer even on a side stream, more than the two-limb
    arithmetic gains; within an edge type an element keeps all 22 bits down to 4e-6 of the type's largest bucket entry, and the
    columns of one type's bucket sums are sums of the same post-activation states.  The kernel and the C ABI take any grouping:
    tests/test_gpu_limb_gemm.py measures per-column scales on both sides.)"""
    if (amax is not None and _cfg.limb_pair and _cfg.pair_part("tn") and DN.limb_tn_supported(agg, gsc)
            and agg.shape[1] * gsc.shape[1] > 256 * 256):
        return DN.limb_gemm_tn(agg, gsc, DN.col_absmax(amax.view(-1, L)), DN.col_absmax(gsc))
    return DN.matmul_tn_splitk(agg, gsc)


def _pair_products(X, rowptr, stride, V, k, n, kernels, kind) -> bool:
    """The two-fp16-limb form for this gather + product pair (dense.RELGNN_LIMB=pair): the gather can write the per-bucket
    magnitudes and the product takes the limb route."""
    if not (_cfg.limb_pair and X.is_cuda and DN.limb_shape_ok(V, n, k)):
        return False
    if not _cfg.pair_part(kind):                         # (diagnostics: which products take the form)
        return False
    return (rowmax_supported(X, rowptr, stride, aggregate_acc64())
            and DN.weight_image_ok(list(kernels), DN.WEIGHT_NN if kind == "nn" else DN.WEIGHT_NT))


def _target_rows(graph) -> int:
    """The rows aggregate_then_transform computes for this graph: its num_targets (graph.RelGraph; V for every graph but a level of
    a "blocks" batch)."""
    T = int(getattr(graph, "num_targets", graph.V))
    return T if 0 <= T < graph.V else graph.V


def _fused_layer_ok(H, graph, w, kernels) -> bool:
    """relgnn_rgcn_fused_fwd applies: switch on, exact-split limb route, 256 -> 256, no hub plan on the by-target buckets."""
    if _cfg.rgcn_fused != "1" or not _cfg.limb_gemm or aggregate_acc64():
        return False
    if not (H.is_cuda and DN.rows_aligned(H) and kernels[0].shape == (256, 256) and H.shape[1] == 256 and DN.weight_image_ok(kernels, DN.WEIGHT_NN)):
        return False
    if split_plan_of(graph.rowptr_t, 1) is not None or graph.V <= 0 or len(kernels) > 64:
        return False
    return w is None or (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous())


def _rgcn_fused(H, graph, w, kernels, relu: bool, want_sums: bool):
    V, L = graph.V, len(kernels)
    out = torch.empty((V, 256), dtype=torch.float32, device=H.device)
    agg = torch.empty((V, L * 256), dtype=torch.float32, device=H.device) if want_sums else None
    buf = DN.weight_limbs(list(kernels), DN.WEIGHT_NN)
    _lib.launch("relgnn_rgcn_fused_fwd", _lib.ptr(H, rows_strided=True), H.shape[0], H.stride(0), _lib.ptr(graph.rowptr_t), V, L,
                _lib.ptr(graph.src_t), _lib.ptr(w), buf.data_ptr(), None, _lib.ACT_RELU if relu else _lib.ACT_LINEAR, _lib.ptr(agg),
                L * 256, _lib.ptr(out), 256, 256, 256, handover_word(H.device).data_ptr())
    return agg, out


class _AggregateThenTransform(torch.autograd.Function):
    """out = act(f_mode(sum_l A_l @ W_l)),  A_l[v] = sum_{p in (v,l)} w_p H[src_p]   (W: [L, Din, Dout]).

    Same function as transform-then-aggregate (gnns/rgcn.py:84-114: sum / mean / sqrt_n commute with the per-type linear
    map), different memory behaviour: the gather reads the [V, Din] state table (C2: 33 MB, one graph's slab fits the 4 MiB
    L2 of its XCD) instead of the L-times larger table of transformed states, and the GEMM gets K = L*Din.  Measured on
    MI355X, C2, one layer forward: 86.6 + 107.5 us vs 120.8 + 107.4 us (scripts/exp_agg_first.py).
    Backward: dH through the by-source buckets exactly as before (gather dOut rows, GEMM with the stacked W_l^T),
    dW_l = A_l^T @ dOut from the saved aggregated rows.

    Target rows only: a graph whose messages all arrive among its first graph.num_targets nodes (a level of a sampled batch under
    the citation task's "blocks") gets bucket sums, a product, `out` and a weight gradient over those T rows alone: the by-target
    bucketing of rows [0, T) is a prefix of the arrays, so the same gather runs with num_out = T * L on the same rowptr_t object (a
    hub's SplitPlan stays attached to it).  The by-source gather and the input-gradient product stay over all V sources and read
    dOut [T, Dout]: no by-source entry names a target >= T.  The fused kernel and the RELGNN_LIMB=pair route (per-bucket magnitudes
    over V * L rows) keep all V rows; the caller cuts what it gets (ROUTES["rgcn_rows"] says which ran last)."""

    @staticmethod
    def forward(ctx, H, graph, w, mode: int, act: int, act_name, h_act: int, *kernels):
        H = H.contiguous()
        L = len(kernels)                                # kernels[l]: [Din, Dout], the per-edge-type variables themselves
        d_in, d_out = kernels[0].shape
        V = graph.V
        # RELGNN_LIMB=pair: the gather also writes every bucket's largest magnitude — the row scales of the two-fp16-limb product
        amax = None
        if _pair_products(H, graph.rowptr_t, 1, V, L * d_in, d_out, kernels, "nn"):
            amax = torch.empty(V * L, dtype=torch.float32, device=H.device)
        want_w = any(ctx.needs_input_grad[7:])
        fused = amax is None and _fused_layer_ok(H, graph, w, kernels)
        # the rows computed: the graph's targets alone, unless a route that needs the square graph serves this call
        T = V if (amax is not None or fused) else _target_rows(graph)
        ROUTES["rgcn_rows"] = "targets" if T < V else "all"
        f = _mode_factor(graph, mode)
        if f is not None and T < V:
            f = f[:T]
        fused_relu = act == _lib.ACT_RELU and f is None       # sum aggregation: ReLU rides in the product's epilogue
        if fused:
            # one kernel: the gather waves hand the bucket sums to the matrix waves through LDS (csrc/rgcn_fused.hip); the sums are
            # also stored as fp32 when the weight gradient will read them.  Same bits as the two launches below.
            agg, out = _rgcn_fused(H, graph, w, kernels, fused_relu, want_w)
        else:
            agg = _seg_reduce_raw(_lib.AGG_SUM, H, graph.rowptr_t, 1, graph.src_t, w, T * L,
                                  acc64=aggregate_acc64(), rowmax=amax).view(T, L * d_in)
            out = DN.grouped_nn_gemm(agg, kernels, relu=fused_relu, xmax=amax, xgroups=L)
        if f is not None:
            out.mul_(f.unsqueeze(1))
        if act == _lib.ACT_RELU:
            if not fused_relu:
                out.relu_()
        elif act == _lib.ACT_TANH:
            out.tanh_()
        elif act != _lib.ACT_LINEAR:
            out = apply_activation(get_activation(act_name), out)
        ctx.graph, ctx.w, ctx.mode, ctx.act, ctx.L, ctx.T = graph, w, mode, act, L, T
        # h_act: H is itself the output of that activation and its gradient factor may ride in the input-gradient product's
        # epilogue (dense.fusable_activation_of; needs d_in == the product's N, i.e. H's own rows as the epilogue operand)
        ctx.h_act = h_act if ctx.needs_input_grad[0] else 0
        ctx.save_for_backward(agg if want_w else None, out if act != _lib.ACT_LINEAR else None,
                              amax if want_w else None, H if ctx.h_act else None, *kernels)
        ctx.leaf_params = tuple(kernels) if all(k.is_leaf for k in kernels) else None
        return out

    @staticmethod
    def backward(ctx, gout):
        graph, w, mode, act, L = ctx.graph, ctx.w, ctx.mode, ctx.act, ctx.L
        agg, out, amax, H_in, *kernels = ctx.saved_tensors
        d_in, d_out = kernels[0].shape
        V, T = graph.V, ctx.T
        if gout.shape[0] != T:
            raise ValueError("aggregate_then_transform: the gradient has %d rows, the layer gave %d" % (gout.shape[0], T))
        # g * act'(out) — unless the consumer of `out` folded that factor into the product that made this gradient (the tag is on
        # the tensor object: look before anything copies it)
        premasked = act != _lib.ACT_LINEAR and DN.is_premasked(gout, out, act)
        gout = gout.contiguous()
        if act != _lib.ACT_LINEAR and not premasked:
            gout = DN.act_bwd_from_output(act, out, gout)
        need = ctx.needs_input_grad[7:]
        want_w = any(need)

        def weight_side():
            gsc = _raw_sum_gradient(gout, graph, mode, T)  # agg holds the raw sums: the factor multiplies dOut
            gW = _weight_gradient(agg, gsc, amax, L)    # dW_l = A_l^T @ dOut: row block l of [L*Din, Dout]
            return tuple(gW[l * d_in:(l + 1) * d_in] if need[l] else None for l in range(L))

        # The weight gradient (matrix-pipe bound, one workgroup per CU, 147 KB of LDS, no L2 pressure) does not depend on the input
        # gradient's gather (L2-latency bound, no LDS, few registers): it runs on a side stream next to it (fork / join by events,
        # capturable in a hipGraph; the result is the same bits, the kernels are the same).
        aside = fork(weight_side, (gout, agg) + ((amax,) if amax is not None else ()), ctx.leaf_params,
                     want=want_w and ctx.needs_input_grad[0], join_in_backward=True, contributes=want_w)
        gH = None
        if ctx.needs_input_grad[0]:
            plan = graph.plan_transformed(w)            # by-source buckets; weights carry the mean / sqrt_n factor
            gmax = None
            if (plan.num_rows_x == V * L and
                    _pair_products(gout, plan.rowptr_b, plan.stride_b, V, L * d_out, d_in, kernels, "nt")):
                gmax = torch.empty(V * L, dtype=torch.float32, device=gout.device)
            gT = _seg_reduce_raw(_lib.AGG_SUM, gout, plan.rowptr_b, plan.stride_b, plan.col_b, plan.w_bwd(mode),
                                 plan.num_rows_x, acc64=aggregate_acc64(), rowmax=gmax).view(V, L * d_out)   # row u: [dT_0 | .. | dT_{L-1}]
            if ctx.h_act and H_in is not None:                               # dH = sum_l dT_l @ W_l^T (* act'(H): H's producer skips its pass)
                gH = DN.mark_premasked(DN.grouped_nt_gemm(gT, kernels, xmax=gmax, xgroups=L, premask=(ctx.h_act, H_in)), H_in, ctx.h_act)
            else:
                gH = DN.grouped_nt_gemm(gT, kernels, xmax=gmax, xgroups=L)
        gWs = aside.join() if aside is not None else (weight_side() if want_w else (None,) * L)
        return (gH, None, None, None, None, None, None) + gWs


def aggregate_then_transform(H, W, graph, w, aggregation: str, activation: Optional[str], sole_reader: bool = False):
    """sole_reader: this call is the only reader of H (activation_tags.py, "activation gradients folded into the product that feeds them")."""
    mode, act = aggregation_mode_id(aggregation), activation_id(activation)
    if mode == _lib.AGG_MAX or act not in _FUSABLE_ACTS:
        raise ValueError("aggregate_then_transform: max aggregation / %r do not apply" % activation)
    # W: the per-edge-type kernels [Din, Dout] (a sequence: the variables themselves — nothing is stacked) or one [L, Din, Dout] tensor
    kernels = W.unbind(0) if torch.is_tensor(W) else tuple(W)
    h_act = DN.fusable_activation_of(H, sole_reader) if (H.requires_grad and H.is_contiguous() and H.shape[1] == kernels[0].shape[0]) else 0
    out = _AggregateThenTransform.apply(H, graph, w, mode, act, activation, h_act, *kernels)
    return DN.mark_activation_output(out, act)     # (ReLU: any consumer may fold its gradient; the others need a caller's word that it is the only one)

