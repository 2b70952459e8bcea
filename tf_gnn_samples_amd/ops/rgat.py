"""RGAT attention (csrc/rgat_fast.hip, generic fallback csrc/rgat.hip; score tables csrc/rgat_scores.hip)."""
import torch

from .. import _lib
from ..config import settings as _cfg
from ..dense import column_sum
from .segment import _seg_reduce_raw


def _rgat_fast_ok(D: int, K: int) -> bool:
    return K in (1, 2, 4, 8) and D % K == 0 and (D // K) % 4 == 0 and D <= 1024


def _rgat_dz_fast_ok(D: int, K: int) -> bool:
    dh4 = D // K // 4 if K and D % (4 * K) == 0 else 0
    return _rgat_fast_ok(D, K) and D <= 256 and dh4 > 0 and (dh4 & (dh4 - 1)) == 0


class _RgatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, s_src, s_tgt, graph, num_heads: int, slope: float):
        T, s_src, s_tgt = T.contiguous(), s_src.contiguous(), s_tgt.contiguous()
        V, L, M = graph.V, graph.L, graph.M
        D = T.shape[1]
        out = torch.empty((V, D), dtype=torch.float32, device=T.device)
        alpha = torch.empty((M, num_heads), dtype=torch.float32, device=T.device)
        fast = _rgat_fast_ok(D, num_heads)
        if fast:
            _lib.launch("relgnn_rgat_alpha", _lib.ptr(s_src), _lib.ptr(s_tgt), num_heads, _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(graph.col_t), slope, _lib.ptr(alpha))
            _lib.launch("relgnn_headw_reduce", _lib.ptr(T), V * L, D, D, num_heads, _lib.ptr(graph.rowptr_t), V, L, _lib.ptr(graph.col_t),
                        _lib.ptr(alpha), None, _lib.ptr(out), D, None, None)
        else:
            _lib.launch("relgnn_rgat_fwd", _lib.ptr(T), D, D, num_heads, _lib.ptr(s_src), _lib.ptr(s_tgt), _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(graph.col_t), slope, _lib.ptr(out), D, _lib.ptr(alpha))
        ctx.graph, ctx.K, ctx.slope, ctx.fast = graph, num_heads, slope, fast
        ctx.save_for_backward(T, s_src, s_tgt, alpha, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        graph, K, slope = ctx.graph, ctx.K, ctx.slope
        T, s_src, s_tgt, alpha, out = ctx.saved_tensors
        V, L, M = graph.V, graph.L, graph.M
        D = T.shape[1]
        gout = gout.contiguous()
        dz = torch.empty((M, K), dtype=torch.float32, device=T.device)
        # the two score-table gradients are sums of dz over the (target, type) and the (source, type) buckets: the dz
        # pass keeps the first in registers and the by-source gather of the gT pass carries the second along
        # (RELGNN_RGAT_FUSED_SUMS=0: two separate gather-reduces over dz, 70 + 60 us per layer at the C2 shape)
        fuse = _cfg.rgat_fused_sums != "0"
        if ctx.fast and _rgat_dz_fast_ok(D, K):
            fuse_t = fuse and L * K <= 64
            gs_tgt = torch.empty((V * L, K), dtype=torch.float32, device=T.device) if fuse_t else None
            _lib.launch("relgnn_rgat_dz", _lib.ptr(T), V * L, D, D, K, _lib.ptr(s_src), _lib.ptr(s_tgt), _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(graph.col_t), slope, _lib.ptr(alpha), _lib.ptr(out), _lib.ptr(gout), D, _lib.ptr(dz), _lib.ptr(gs_tgt))
            if not fuse_t:
                gs_tgt = _seg_reduce_raw(_lib.AGG_SUM, dz, graph.rowptr_t, 1, graph.iota, None, V * L)
        else:
            gs_tgt = torch.empty((V * L, K), dtype=torch.float32, device=T.device)
            _lib.launch("relgnn_rgat_bwd_logits", _lib.ptr(T), D, D, K, _lib.ptr(s_src), _lib.ptr(s_tgt), _lib.ptr(graph.rowptr_t), V, L,
                        _lib.ptr(graph.col_t), slope, _lib.ptr(alpha), _lib.ptr(out), _lib.ptr(gout), D, _lib.ptr(dz), _lib.ptr(gs_tgt))
        if ctx.fast:
            gT = torch.empty_like(T)
            gs_src = torch.empty((V * L, K), dtype=torch.float32, device=T.device) if fuse else None
            _lib.launch("relgnn_headw_reduce", _lib.ptr(gout), V, D, D, K, _lib.ptr(graph.rowptr_s), V * L, 1, _lib.ptr(graph.tgt_s),
                        _lib.ptr(alpha), _lib.ptr(graph.pos_t_of_s), _lib.ptr(gT), D, _lib.ptr(dz) if fuse else None, _lib.ptr(gs_src))
            if not fuse:
                gs_src = _seg_reduce_raw(_lib.AGG_SUM, dz, graph.rowptr_s, 1, graph.pos_t_of_s, None, V * L)
        else:
            gT = torch.empty_like(T)
            gs_src = torch.empty((V * L, K), dtype=torch.float32, device=T.device)
            _lib.launch("relgnn_rgat_bwd_msg", D, K, _lib.ptr(graph.rowptr_s), V * L, _lib.ptr(graph.tgt_s), _lib.ptr(graph.pos_t_of_s),
                        _lib.ptr(alpha), _lib.ptr(dz), _lib.ptr(gout), D, _lib.ptr(gT), D, _lib.ptr(gs_src))
        return gT, gs_src, gs_tgt, None, None, None


def rgat_scores_supported(D: int, K: int) -> bool:
    g = D // 4
    return D % 4 == 0 and g in (8, 16, 32, 64) and K > 0 and g % K == 0 and ((g // K) & (g // K - 1)) == 0


class _RgatLayerAttention(torch.autograd.Function):
    """rgat.py:103-136 from the transformed rows T [V*L, D] and the stacked attention parameters att [L, 2D]:
    score tables (csrc/rgat_scores.hip) -> segmented softmax -> attention-weighted sum, one autograd node; the
    backward folds the score-table gradients into gT in place and reduces d att without atomics."""

    @staticmethod
    def forward(ctx, T, att, graph, num_heads: int, slope: float):
        T, att = T.contiguous(), att.contiguous()
        V, L = graph.V, graph.L
        D = T.shape[1]
        s_src = torch.empty((V * L, num_heads), dtype=torch.float32, device=T.device)
        s_tgt = torch.empty_like(s_src)
        _lib.launch("relgnn_rgat_scores_fwd", _lib.ptr(T), D, D, num_heads, _lib.ptr(att), L, V, _lib.ptr(s_src), _lib.ptr(s_tgt))
        out = _RgatAttention.forward(ctx, T, s_src, s_tgt, graph, num_heads, slope)   # saves T, s_*, alpha, out
        ctx.att = att
        return out

    @staticmethod
    def backward(ctx, gout):
        T = ctx.saved_tensors[0]
        att, graph, K = ctx.att, ctx.graph, ctx.K
        V, L = graph.V, graph.L
        D = T.shape[1]
        gT, gs_src, gs_tgt = _RgatAttention.backward(ctx, gout)[:3]
        groups = int(_lib.load_library().relgnn_rgat_scores_groups(V))
        partial = torch.empty((groups, L * 2 * D), dtype=torch.float32, device=T.device)
        _lib.launch("relgnn_rgat_scores_bwd", _lib.ptr(T), D, D, K, _lib.ptr(att), L, V, _lib.ptr(gs_src), _lib.ptr(gs_tgt), _lib.ptr(gT),
                    D, _lib.ptr(partial), groups)
        gatt = column_sum(partial).view(L, 2 * D)
        return gT, gatt, None, None, None


def rgat_layer_attention(T, att, graph, num_heads: int, slope: float = 0.2):
    """T [V*L, D] (row v*L+l = h_v W_l), att [L, 2D] = the stacked Edge_%i_Attention_Parameters."""
    return _RgatLayerAttention.apply(T, att, graph, int(num_heads), float(slope))


def rgat_attention(T, s_src, s_tgt, graph, num_heads: int, slope: float = 0.2):
    """gnns/rgat.py:98-136: segmented softmax over all incoming messages + attention-weighted sum."""
    return _RgatAttention.apply(T, s_src, s_tgt, graph, int(num_heads), float(slope))

