"""Layer-input dropout (include/relgnn_dropout.h, csrc/dropout.hip; config.settings.layer_dropout == "fused")."""
import torch

from .. import _lib
from ..config import settings as _cfg
from .segment import _check_f32


def dropout_threshold(keep_prob: float) -> int:
    """T of the keep rule (word >> 8) < T: round(keep_prob * 2^24), in double on the host."""
    return int(round(float(keep_prob) * float(1 << 24)))


def dropout_state(device, seed: int = 0, replica: int = 0, step: int = 0) -> torch.Tensor:
    """The int64[3] state block {seed, replica, step} of csrc/dropout.hip in device memory."""
    return torch.tensor([int(seed) & 0xffffffff, int(replica) & 0xffffffff, int(step)], dtype=torch.int64, device=device)


def fused_dropout_on(keep_prob: float) -> bool:
    """The switch, asked once per pass: layer_dropout == "fused" and something is dropped at all."""
    return _cfg.layer_dropout == "fused" and keep_prob < 1.0


def dropout_tensor_ok(x: torch.Tensor) -> bool:
    """A layer input the kernels take: a contiguous fp32 GPU tensor (anything else is the torch call's)."""
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()


def _dropout_args(x, keep_prob, state, stream_id, what):
    _check_f32(x, what)
    if state.dtype != torch.int64 or state.numel() != 3:
        raise ValueError("%s: the state block is int64[3] = {seed, replica, step}" % what)
    if not 0.0 < keep_prob <= 1.0:
        raise ValueError("%s: keep_prob must be in (0, 1], got %r" % (what, keep_prob))
    return x.numel(), 0, _lib.ptr(state), int(stream_id), dropout_threshold(keep_prob), float(keep_prob)


def _dropout_backward(gy, ctx, state, what):
    """g_x = (g_y / keep_prob) * m with m regenerated from the saved state (relgnn_dropout_bwd)."""
    gy = gy.contiguous()
    gx = torch.empty_like(gy)
    _lib.launch("relgnn_dropout_bwd", _lib.ptr(gy), *_dropout_args(gy, ctx.keep_prob, state, ctx.stream_id, what), _lib.ptr(gx))
    return gx


class _DropoutFn(torch.autograd.Function):
    """csrc/dropout.hip: y = (x / keep_prob) * m, one read + one write; the backward regenerates m from the saved 24-byte state."""

    @staticmethod
    def forward(ctx, x, keep_prob: float, state, stream_id: int):
        args = _dropout_args(x, keep_prob, state, stream_id, "dropout")
        y = torch.empty_like(x)
        _lib.launch("relgnn_dropout_fwd", _lib.ptr(x), *args, _lib.ptr(y))
        ctx.keep_prob, ctx.stream_id = keep_prob, stream_id
        ctx.save_for_backward(state)
        return y

    @staticmethod
    def backward(ctx, gy):
        (state,) = ctx.saved_tensors
        return _dropout_backward(gy, ctx, state, "dropout"), None, None, None


class _DropoutResidualFn(torch.autograd.Function):
    """csrc/dropout.hip, residual layers after the first: t = drop(x) and cur = (t + last) / 2 in one pass over x and last; the
    backward is one pass too: g_last = g_cur / 2, g_x = ((g_t + g_cur / 2) / keep_prob) * m (the composition's order of operations:
    on the same mask the same bits)."""

    @staticmethod
    def forward(ctx, x, last, keep_prob: float, state, stream_id: int):
        args = _dropout_args(x, keep_prob, state, stream_id, "dropout_residual")
        _check_f32(last, "dropout_residual")
        if last.shape != x.shape:
            raise ValueError("dropout_residual: x %s and last %s differ in shape" % (tuple(x.shape), tuple(last.shape)))
        t, cur = torch.empty_like(x), torch.empty_like(x)
        _lib.launch("relgnn_dropout_residual_fwd", _lib.ptr(x), _lib.ptr(last), *args, _lib.ptr(t), _lib.ptr(cur))
        ctx.keep_prob, ctx.stream_id = keep_prob, stream_id
        ctx.set_materialize_grads(False)          # (g_t is absent at the last residual layer: no zeros filled, no 0 added)
        ctx.save_for_backward(state)
        return t, cur

    @staticmethod
    def backward(ctx, g_t, g_cur):
        (state,) = ctx.saved_tensors
        if g_cur is None:                         # only t was used: the plain dropout's backward
            return _dropout_backward(g_t, ctx, state, "dropout_residual"), None, None, None, None
        g_cur = g_cur.contiguous()
        g_t = g_t.contiguous() if g_t is not None else None
        g_x, g_last = torch.empty_like(g_cur), torch.empty_like(g_cur)
        _lib.launch("relgnn_dropout_residual_bwd", _lib.ptr(g_t), _lib.ptr(g_cur),
                    *_dropout_args(g_cur, ctx.keep_prob, state, ctx.stream_id, "dropout_residual"), _lib.ptr(g_x), _lib.ptr(g_last))
        return g_x, g_last, None, None, None


def dropout(x: torch.Tensor, keep_prob: float, state: torch.Tensor, stream_id: int) -> torch.Tensor:
    """tf.nn.dropout(x, rate = 1 - keep_prob) with the mask of (state = {seed, replica, step}, stream_id): a contiguous fp32 GPU
    tensor of any shape (no CPU fallback here: the caller picks the route, dropout_tensor_ok)."""
    return _DropoutFn.apply(x.contiguous(), float(keep_prob), state, int(stream_id))


def dropout_residual(x: torch.Tensor, last: torch.Tensor, keep_prob: float, state: torch.Tensor, stream_id: int):
    """(t, cur) = (dropout(x), (t + last) / 2): the layer-input stage of a residual layer after the first
    (models/sparse_graph_model.py:178-185) in one kernel."""
    return _DropoutResidualFn.apply(x.contiguous(), last.contiguous(), float(keep_prob), state, int(stream_id))
