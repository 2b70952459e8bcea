"""RGDCN dynamic kernels applied node-side (csrc/rgdcn.hip)."""
from typing import Optional

import torch

from .. import _lib
from ..activations import FUSABLE_ACTS as _FUSABLE_ACTS, activation_id
from ..dense import act_bwd_from_output
from .segment import _raw_sum_gradient, aggregation_mode_id


class _RgdcnApply(torch.autograd.Function):
    """out[v,c,:] = out_act(f_mode(sum_l A[v,l,c,:] @ weight_act(P[v,l,c]))); A [V*L, C*K] (bucket-aggregated source
    states), P pre-activation dynamic weights in either GEMM layout ([V, L, C, K*K] or [C, V, L, K*K])."""

    @staticmethod
    def forward(ctx, A, P, graph, C: int, K: int, mode: int, weight_act: int, out_act: int, channel_major: bool):
        A, P = A.contiguous(), P.contiguous()
        V, L = graph.V, graph.L
        KK = K * K
        strides = (L * KK, KK, V * L * KK) if channel_major else (L * C * KK, C * KK, KK)
        out = torch.empty((V, C * K), dtype=torch.float32, device=A.device)
        _lib.launch("relgnn_rgdcn_apply_fwd", mode, weight_act, out_act, _lib.ptr(A), _lib.ptr(P), *strides, V, L, C, K,
                    _lib.ptr(graph.rowptr_t), _lib.ptr(out))
        ctx.graph, ctx.geom, ctx.strides = graph, (C, K, mode, weight_act, out_act), strides
        ctx.save_for_backward(A, P, out if out_act != _lib.ACT_LINEAR else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        A, P, out = ctx.saved_tensors
        graph = ctx.graph
        C, K, mode, weight_act, out_act = ctx.geom
        V, L = graph.V, graph.L
        g = gout.contiguous()
        if out_act != _lib.ACT_LINEAR:
            g = act_bwd_from_output(out_act, out, g)
        g = _raw_sum_gradient(g, graph, mode)
        gA, gP = torch.empty_like(A), torch.empty_like(P)
        _lib.launch("relgnn_rgdcn_apply_bwd", weight_act, _lib.ptr(A), _lib.ptr(P), *ctx.strides, V, L, C, K, _lib.ptr(g), _lib.ptr(gA),
                    _lib.ptr(gP))
        return gA, gP, None, None, None, None, None, None, None


def rgdcn_apply_supported(K: int, out_act: int) -> bool:
    return 0 < K <= 64 and (K & (K - 1)) == 0 and out_act in _FUSABLE_ACTS


def rgdcn_apply(A, P, graph, num_channels: int, channel_dim: int, aggregation: str, weight_activation: Optional[str],
                output_activation: Optional[str], channel_major: bool):
    return _RgdcnApply.apply(A, P, graph, int(num_channels), int(channel_dim), aggregation_mode_id(aggregation),
                             activation_id(weight_activation), activation_id(output_activation), bool(channel_major))

