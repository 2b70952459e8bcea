"""Fused edge-wise message kernels (csrc/edge_fused.hip), the materialised pair messages, and the per-edge-type Dense layers of an
edge MLP on the type-major message list: blocked_linear and its fusion with the pair messages (csrc/edge_mlp_fused.hip)."""
from typing import Optional

import torch

from .. import _lib
from ..activations import FUSABLE_ACTS as _FUSABLE_ACTS, activation_id
from ..config import settings as _cfg
from ..dense import GEMM_NN, GEMM_NT, act_bwd_from_output, matmul_tn_splitk, mm_into, sel_image
from .segment import _check_f32, _raw_sum_gradient, _seg_reduce_raw, aggregation_mode_id


class _FusedEdgeMessages(torch.autograd.Function):
    """kind 'film': out[v] = AGG act(gamma[v,l] * (w * T[src,l]) + beta[v,l]),  A = film [V*L, 2D]
       kind 'pair': out[v] = AGG act(w * (T[src,l] + A[v,l])),                  A = Q    [V*L, D]"""

    @staticmethod
    def forward(ctx, T, A, graph, w, mode: int, act: int, kind: str, pairs=None):
        """pairs (graph.PairTables, FiLM only): T / A hold rows for the non-empty (node,type) buckets only."""
        _check_f32(T, "T"); _check_f32(A, "A")
        T, A = T.contiguous(), A.contiguous()
        V, L = graph.V, graph.L
        D = T.shape[1]
        rows_t, rows_a = (V * L, V * L) if pairs is None else (pairs.P_s, pairs.P_t)
        if pairs is not None and kind != "film":
            raise ValueError("compact pair tables are only wired into the FiLM kernels")
        if T.shape[0] != rows_t or A.shape[0] != rows_a or A.shape[1] != (2 * D if kind == "film" else D):
            raise ValueError("bad operand shapes for fused %s messages" % kind)
        out = torch.empty((V, D), dtype=torch.float32, device=T.device)
        if kind == "film":
            col = graph.col_t if pairs is None else pairs.col_t
            brow = None if pairs is None else pairs.tgt.bucket_row
            _lib.launch("relgnn_film_fwd", mode, act, _lib.ptr(T), D, _lib.ptr(A), A.shape[1], D, _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(col), _lib.ptr(w), _lib.ptr(out), D, _lib.ptr(brow))
        else:
            _lib.launch("relgnn_pair_fwd", mode, act, _lib.ptr(T), D, _lib.ptr(A), A.shape[1], D, _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(graph.col_t), _lib.ptr(w), _lib.ptr(out), D)
        ctx.graph, ctx.w, ctx.mode, ctx.act, ctx.kind, ctx.pairs = graph, w, mode, act, kind, pairs
        ctx.save_for_backward(T, A)
        return out

    @staticmethod
    def backward(ctx, gout):
        graph, w, mode, act, kind, pairs = ctx.graph, ctx.w, ctx.mode, ctx.act, ctx.kind, ctx.pairs
        if mode == _lib.AGG_MAX:
            raise RuntimeError("fused %s messages have no max-aggregation backward; the layer uses the unfused path" % kind)
        T, A = ctx.saved_tensors
        V, L = graph.V, graph.L
        D = T.shape[1]
        gagg = _raw_sum_gradient(gout, graph, mode)
        gA = torch.empty_like(A)
        if pairs is not None:
            # compact tables: every real row is written by the kernels; the few padding rows are not and feed the
            # batched weight-gradient GEMM (against all-zero inputs, but 0 * NaN garbage would still poison it)
            _fill_rows(gA, pairs.tgt.pad_rows, 0.0)
        # Two ways to the gradient of the gathered rows (RELGNN_EDGE_BWD=emit|regather overrides the choice):
        #  emit:     pass A (by target) also writes every message's gradient w.r.t. its gathered row ([M, D]); gT is then
        #            one plain gather-reduce of those rows over the by-source buckets;
        #  regather: pass B walks the by-source buckets and re-gathers the per-bucket row (8D bytes for FiLM) and the
        #            target's gradient row once per MESSAGE, recomputing the pre-activation: nothing [M, D] is written.
        # Measured on MI355X (scripts/bench_configs.py): the wave kernels (D > 128) on dense tables win with regather
        # (FiLM on the C2 batch: 833 + 426 us -> 330 + 536 us per layer, step 9.06 -> 7.66 ms); the lane-group kernels on
        # compact pair tables (C5: D = 128, 23 types) with emit (47.4 vs 52.9 ms).
        choice = _cfg.edge_bwd if _cfg.edge_bwd != "auto" else ("emit" if (pairs is not None or D <= 128) else "regather")
        emit = choice == "emit"
        dmsg = torch.empty((graph.M, D), dtype=torch.float32, device=T.device) if emit else None
        # RELGNN_EDGE_SIGN_MASK=1 (opt-in; regather + piecewise-linear activation + wave kernels with one float4 per lane):
        # pass A leaves one sign bit per feature and message, pass B then gathers gamma and the target's gradient row only.
        # Measured on the C2 batch: pass B 536 -> 419 us, but the four ballots + the mask store cost pass A 330 -> 402 us and
        # the step does not get faster (7.31 / 7.27 ms without, 7.43 / 7.41 ms with, one A/B call) -> off by default.
        smask = None
        if (not emit and kind == "film" and pairs is None and act in (_lib.ACT_LINEAR, _lib.ACT_RELU, _lib.ACT_LEAKY_RELU)
                and 128 < D <= 256 and L <= 63 and V * L * (D // 4) < 2 ** 32 and graph.M > 0
                and _cfg.edge_sign_mask == "1"):
            smask = torch.empty((graph.M, 4), dtype=torch.int64, device=T.device)
        if kind == "film":
            col = graph.col_t if pairs is None else pairs.col_t
            brow_t = None if pairs is None else pairs.tgt.bucket_row
            _lib.launch("relgnn_film_bwd_film", act, _lib.ptr(T), D, _lib.ptr(A), A.shape[1], D, _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(col), _lib.ptr(w), _lib.ptr(gagg), D, _lib.ptr(gA), A.shape[1], _lib.ptr(brow_t), _lib.ptr(dmsg),
                        _lib.ptr(smask))
        else:
            _lib.launch("relgnn_pair_bwd_q", act, _lib.ptr(T), D, _lib.ptr(A), D, D, _lib.ptr(graph.rowptr_t), V, L, _lib.ptr(graph.col_t),
                        _lib.ptr(w), _lib.ptr(gagg), D, _lib.ptr(gA), D, _lib.ptr(dmsg))
        if emit:
            if pairs is None:
                gT = _seg_reduce_raw(_lib.AGG_SUM, dmsg, graph.rowptr_s, 1, graph.pos_t_of_s, None, V * L)
            else:
                rowptr_c, _, pos_c = pairs._messages_by_source_row()
                gT = _seg_reduce_raw(_lib.AGG_SUM, dmsg, rowptr_c, 1, pos_c, None, pairs.P_s)   # padding rows: zero
        elif smask is not None:
            gT = torch.empty_like(T)
            _lib.launch("relgnn_film_bwd_msg_masked", act, _lib.ptr(A), A.shape[1], D, _lib.ptr(graph.rowptr_s), V * L,
                        _lib.ptr(graph.tgt_s), _lib.ptr(graph.frow_s), _lib.ptr(graph.w_by_source(w)), _lib.ptr(graph.pos_t_of_s),
                        _lib.ptr(smask), _lib.ptr(gagg), D, _lib.ptr(gT), D)
        elif kind == "film":
            gT = torch.empty_like(T)
            if pairs is not None:
                _fill_rows(gT, pairs.src.pad_rows, 0.0)
            frow = graph.frow_s if pairs is None else pairs.frow_s
            brow_s = None if pairs is None else pairs.src.bucket_row
            _lib.launch("relgnn_film_bwd_msg", act, _lib.ptr(T), D, _lib.ptr(A), A.shape[1], D, _lib.ptr(graph.rowptr_s), V * L,
                        _lib.ptr(graph.tgt_s), _lib.ptr(frow), _lib.ptr(graph.w_by_source(w)), _lib.ptr(gagg), D, _lib.ptr(gT), D,
                        _lib.ptr(brow_s))
        else:
            gT = torch.empty_like(T)
            _lib.launch("relgnn_pair_bwd_p", act, _lib.ptr(T), D, _lib.ptr(A), D, D, _lib.ptr(graph.rowptr_s), V * L, _lib.ptr(graph.tgt_s),
                        _lib.ptr(graph.frow_s), _lib.ptr(graph.w_by_source(w)), _lib.ptr(gagg), D, _lib.ptr(gT), D)
        return gT, gA, None, None, None, None, None, None


def film_messages_reduce(T, film, graph, w, aggregation: str, activation: Optional[str], pairs=None):
    """gnns/gnn_film.py:92-116 in one kernel (sum / mean / sqrt_n; max forward only).  With `pairs`
    (graph.PairTables) T is [P_s, D] and film [P_t, 2D]: rows for the non-empty (node,type) buckets only."""
    return _on_padded_columns(_FusedEdgeMessages, (T, film), graph, w, aggregation_mode_id(aggregation), activation_id(activation),
                              "film", pairs)


class _BlockedLinear(torch.autograd.Function):
    """Y[a_l:b_l] = X[a_l:b_l] @ W_l for consecutive row blocks (the per-edge-type Dense layers of an edge MLP on the
    type-major message list, utils/utils.py:120-126 via gnns/gnn_edge_mlp.py:102).  One autograd node instead of L
    slices + L GEMM nodes + cat: outputs and input gradients are written straight into their row blocks (no concat,
    no zero-filled accumulation buffer), weight gradients use the split-K reduction over the block's rows."""

    @staticmethod
    def forward(ctx, X, offsets, *weights):
        X = X.contiguous()
        Y = torch.empty((X.shape[0], weights[0].shape[1]), dtype=X.dtype, device=X.device)
        for l, W in enumerate(weights):
            a, b = offsets[l], offsets[l + 1]
            if b > a:
                mm_into(GEMM_NN, X[a:b], W, Y[a:b])
        ctx.offsets = offsets
        ctx.save_for_backward(X, *weights)
        return Y

    @staticmethod
    def backward(ctx, gY):
        X, *weights = ctx.saved_tensors
        gX, gW = _blocked_backward(X, gY.contiguous(), ctx.offsets, weights, ctx.needs_input_grad[0], ctx.needs_input_grad[2:])
        return (gX, None, *gW)


def _blocked_backward(left, gY, offsets, weights, need_x: bool, need_w):
    """(gX, [gW_l]) of Y[a_l:b_l] = left[a_l:b_l] @ W_l: per non-empty row block gX[a:b] = gY[a:b] @ W_l^T written in place and
    gW_l = left[a:b]^T @ gY[a:b] (split-K over the block's rows); an empty block's weight gradient is zero.  need_w: one flag per
    block; `left` is read for the weight gradients only."""
    gX = torch.empty((gY.shape[0], weights[0].shape[0]), dtype=torch.float32, device=gY.device) if need_x else None
    gW = []
    for l, W in enumerate(weights):
        a, b = offsets[l], offsets[l + 1]
        if b > a:
            if need_x:
                mm_into(GEMM_NT, gY[a:b], W, gX[a:b])
            gW.append(matmul_tn_splitk(left[a:b], gY[a:b]) if need_w[l] else None)
        else:
            gW.append(torch.zeros_like(W) if need_w[l] else None)
    return gX, gW


def blocked_linear(X, offsets, weights):
    """X [M, Din] in consecutive row blocks offsets[l]:offsets[l+1]; weights: one [Din, Dout] kernel per block."""
    _check_f32(X, "X")
    return _BlockedLinear.apply(X, [int(o) for o in offsets], *weights)


def _fill_rows(X: torch.Tensor, rows: torch.Tensor, value: float) -> None:
    """X[rows] = value (rows: int64 ids on the device) — relgnn_fill_rows_f32; torch's index_fill_ took 30 us for a few thousand rows."""
    if rows.numel() == 0:
        return
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1 and rows.dtype == torch.int64 and rows.is_contiguous()):
        X.index_fill_(0, rows, value)
        return
    _lib.launch("relgnn_fill_rows_f32", X.data_ptr(), X.stride(0), X.shape[1], rows.data_ptr(), rows.numel(), float(value))


def pair_messages_reduce_fused(P, Q, graph, w, aggregation: str, activation: Optional[str]):
    return _on_padded_columns(_FusedEdgeMessages, (P, Q), graph, w, aggregation_mode_id(aggregation), activation_id(activation), "pair")


class _PairMaterialize(torch.autograd.Function):
    """hidden[m] = act(P[src_m*L+l_m] + Q[tgt_m*L+l_m]) in the reference's type-major message order."""

    @staticmethod
    def forward(ctx, P, Q, graph, act: int):
        P = P.contiguous()
        Q = Q.contiguous() if Q is not None else None
        M, D = graph.M, P.shape[1]
        out = torch.empty((M, D), dtype=torch.float32, device=P.device)
        _lib.launch("relgnn_pair_materialize", act, _lib.ptr(P), D, _lib.ptr(Q), D, D, _lib.ptr(graph.key_by_source),
                    _lib.ptr(graph.key_by_target), M, None, _lib.ptr(out), D)
        ctx.graph, ctx.act, ctx.has_q = graph, act, Q is not None
        ctx.save_for_backward(P, Q)
        return out

    @staticmethod
    def backward(ctx, ghidden):
        P, Q = ctx.saved_tensors
        gP, gQ = _pair_hidden_backward(P, Q if ctx.has_q else None, ctx.graph, ctx.act, ghidden)
        return gP, gQ, None, None


def _pair_hidden_backward(P, Q, graph, act: int, ghidden):
    """(gP, gQ) from the gradient of hidden[m] = act(P[src_m*L+l_m] + Q[tgt_m*L+l_m]) (Q may be None: gQ is None then) — the
    backward of _PairMaterialize and the tail of _EdgeMlpFirstProduct's."""
    has_q = Q is not None
    M, D = graph.M, P.shape[1]
    ghidden = ghidden.contiguous()
    S = graph.V * graph.L
    if (has_q and _cfg.edge_bwd != "emit" and D % 4 == 0 and 128 < D <= 1024
            and M * (D // 4) < 2 ** 32 and S > 0):
        # No [M, D] gradient of the pre-activation is written and re-read twice: the by-(source,type) pass of the pair
        # kernels sums g_m * act'(P[r] + Q[f_m]) per bucket r straight from ghidden's rows (its "target gradient row" is
        # the message's own row here), once over the by-source buckets for gP and once over the by-target buckets with
        # the roles of P and Q swapped for gQ.  C2 shape, elu: 959 + 2 x 423 us -> 2 x ~500 us per layer.
        gP, gQ = torch.empty_like(P), torch.empty_like(Q)
        _lib.launch("relgnn_pair_bwd_p", act, _lib.ptr(P), D, _lib.ptr(Q), D, D, _lib.ptr(graph.rowptr_s), S, _lib.ptr(graph.perm_s),
                    _lib.ptr(graph.frow_s), None, _lib.ptr(ghidden), D, _lib.ptr(gP), D)
        _lib.launch("relgnn_pair_bwd_p", act, _lib.ptr(Q), D, _lib.ptr(P), D, D, _lib.ptr(graph.rowptr_t), S, _lib.ptr(graph.perm_t),
                    _lib.ptr(graph.col_t), None, _lib.ptr(ghidden), D, _lib.ptr(gQ), D)
        return gP, gQ
    gpre = torch.empty_like(ghidden)
    _lib.launch("relgnn_pair_materialize", act, _lib.ptr(P), D, _lib.ptr(Q), D, D, _lib.ptr(graph.key_by_source),
                _lib.ptr(graph.key_by_target), M, _lib.ptr(ghidden), _lib.ptr(gpre), D)
    # gP[r] = sum of gpre over the messages whose source row is r; gQ[f] likewise by target row
    gP = _seg_reduce_raw(_lib.AGG_SUM, gpre, graph.rowptr_s, 1, graph.perm_s, None, S)
    gQ = _seg_reduce_raw(_lib.AGG_SUM, gpre, graph.rowptr_t, 1, graph.perm_t, None, S) if has_q else None
    return gP, gQ


def _on_padded_columns(node, tables, *rest):
    """node.apply(*tables, *rest) for tables [rows, D] (or [rows, k * D]: k blocks of D columns, FiLM's [gamma | beta]; or None).  The
    edge kernels move 16-byte pieces of a row (D % 4 == 0).  A width the reference accepts and they do not (hidden_size 15) runs on
    tables whose every block has zero columns behind it: every message activation maps 0 to 0, so the padded columns stay 0 through
    product, scale, activation and every aggregation, and are cut off again (differentiable: F.pad / slice)."""
    D = tables[0].shape[1]
    pad = (-D) % 4
    if not pad:
        return node.apply(*tables, *rest)

    def padded(X):
        if X is None or X.shape[1] == D:
            return torch.nn.functional.pad(X, (0, pad)) if X is not None else None
        return torch.nn.functional.pad(X.reshape(X.shape[0], -1, D), (0, pad)).reshape(X.shape[0], -1)

    return node.apply(*map(padded, tables), *rest)[:, :D]


def pair_materialize(P, Q, graph, activation: Optional[str]):
    return _on_padded_columns(_PairMaterialize, (P, Q), graph, activation_id(activation))


class _EdgeMlpFirstProduct(torch.autograd.Function):
    """C[m] = out_act(in_act(P[src_m*L+l_m] + Q[tgt_m*L+l_m]) @ W_{l_m}) in ONE launch (csrc/edge_mlp_fused.hip): pair_materialize
    and the first blocked_linear of an edge MLP without the [M, Dh] hidden tensor between them — neither written in the forward
    nor kept for the backward, which recomputes it into a transient buffer (relgnn_pair_materialize) for the weight gradients.
      backward  gC *= out_act'(C)                      (when out_act was fused: act_bwd_from_output)
                hidden = in_act(P[..] + Q[..])          transient
                gH[a:b] = gC[a:b] @ W_l^T, gW_l = hidden[a:b]^T @ gC[a:b]      per non-empty type block (as _BlockedLinear)
                gP, gQ from gH                          (_pair_hidden_backward: as _PairMaterialize)"""

    @staticmethod
    def forward(ctx, P, Q, graph, in_act: int, out_act: int, *weights):
        P = P.contiguous()
        Q = Q.contiguous() if Q is not None else None
        M, (K, N) = graph.M, weights[0].shape
        im = sel_image(weights, GEMM_NN)
        if im is None:
            raise ValueError("edge_mlp_first_product: the weights have no cached limb image (dense.sel_weights_cacheable)")
        panels = graph.edge_mlp_panels()
        C = torch.empty((M, N), dtype=torch.float32, device=P.device)
        _lib.launch("relgnn_edge_mlp_fwd_xf32", in_act, out_act, _lib.ptr(P), P.stride(0), _lib.ptr(Q), Q.stride(0) if Q is not None else 0,
                    _lib.ptr(graph.key_by_source), _lib.ptr(graph.key_by_target), im.buf.data_ptr(), len(weights), _lib.ptr(panels),
                    panels.shape[0], _lib.ptr(C), N, M, N, K)
        ctx.graph, ctx.acts, ctx.has_q = graph, (in_act, out_act), Q is not None
        ctx.save_for_backward(P, Q, C if out_act != _lib.ACT_LINEAR else None, *weights)
        return C

    @staticmethod
    def backward(ctx, gC):
        P, Q, C, *weights = ctx.saved_tensors
        graph, (in_act, out_act) = ctx.graph, ctx.acts
        M, K = graph.M, P.shape[1]
        gC = gC.contiguous()
        if C is not None:
            gC = act_bwd_from_output(out_act, C, gC)
        need_w = ctx.needs_input_grad[5:]
        need_h = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        hidden = None
        if any(need_w) and M > 0:
            # (the one pass through HBM that a gathered-operand weight-gradient kernel would remove: everything below reads
            #  `hidden` as the left operand of a TN product only)
            hidden = torch.empty((M, K), dtype=torch.float32, device=P.device)
            _lib.launch("relgnn_pair_materialize", in_act, _lib.ptr(P), K, _lib.ptr(Q), K, K, _lib.ptr(graph.key_by_source),
                        _lib.ptr(graph.key_by_target), M, None, _lib.ptr(hidden), K)
        gH, gW = _blocked_backward(hidden, gC, graph.type_offsets, weights, need_h, need_w)
        del hidden
        gP = gQ = None
        if need_h:
            gP, gQ = _pair_hidden_backward(P, Q if ctx.has_q else None, graph, in_act, gH)
        return (gP, gQ, None, None, None, *gW)


def edge_mlp_first_product(P, Q, graph, in_activation: Optional[str], weights, out_activation: Optional[str] = None):
    """out_act(in_act(P[src_m*L+l_m] + Q[tgt_m*L+l_m]) @ weights[l_m]) for every message m, [M, N] in the type-major message
    order: ops.pair_materialize + ops.blocked_linear (+ the activation) in one launch, bit for bit.  P, Q ([V*L, K]; Q may be
    None), weights: one [K, N] kernel per edge type whose limb images the step's cache holds (dense.sel_weights_cacheable).
    out_activation must be one whose gradient follows from the output (anything but gelu): apply another one outside.
    Raises where relgnn_edge_mlp_fwd_xf32 does not take the operands — gnns/pair.py asks first (_edge_mlp_fused_ok)."""
    _check_f32(P, "P")
    out_act = activation_id(out_activation)
    if out_act not in _FUSABLE_ACTS:
        raise ValueError("edge_mlp_first_product: out_activation %r cannot be fused (its gradient needs the pre-activation)"
                         % out_activation)
    return _EdgeMlpFirstProduct.apply(P, Q, graph, activation_id(in_activation), out_act, *list(weights))

