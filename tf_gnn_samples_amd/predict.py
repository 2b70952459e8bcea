"""Probabilities and predicted labels out of the task heads' logits (include/relgnn_predict.h, csrc/predict.hip).

A predicted label is decided by the device code that counts it in the task's metric: the three rules below have one definition each
in csrc/common.h, called by the metric kernel and by the prediction kernel.
  sigmoid     PPI          round(sigmoid(x)) half-even == x > 0 and 1 / (1 + exp(-x)) > 0.5 in float32 (a logit of 1e-8 is a 0)
  softmax     Citation     the lowest index of the maximum LOGIT
  candidates  VarMisuse    the lowest index of the maximum float32 softmax PROBABILITY (two logits one ulp apart can share it)
Float32 GPU logits take the kernels; anything else (CPU tensors, other dtypes) takes the torch compositions below, which state the
same rules, as the heads' metric code does.  The optional `out` tensors (views of a packed arena: models/sparse_graph_model.py) are
written in place by the kernels, at their own leading dimensions.
"""
from typing import Optional, Tuple

import torch

from . import _lib


def _rows_ok(t: torch.Tensor) -> bool:
    return t.dim() == 2 and (t.shape[0] <= 1 or t.shape[1] == 0 or (t.stride(1) == 1 and t.stride(0) >= t.shape[1]))


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _out(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError("prediction output: expected %s %s on %s, got %s %s on %s"
                         % (tuple(shape), dtype, device, tuple(out.shape), out.dtype, out.device))
    return out


def _kernel_route(logits: torch.Tensor) -> bool:
    return logits.is_cuda and logits.dtype == torch.float32


def _as_rows(logits: torch.Tensor) -> torch.Tensor:
    if logits.dim() != 2:
        raise ValueError("logits must be [rows, cols], got %s" % (tuple(logits.shape),))
    return logits if _rows_ok(logits) and (not logits.is_cuda or logits.data_ptr() % 4 == 0) else logits.contiguous()


def _first_max(values: torch.Tensor) -> torch.Tensor:
    """int32 [rows]: the lowest column holding the row's maximum (tf.argmax's tie rule)."""
    cols = values.shape[1]
    top = values.max(dim=1, keepdim=True).values
    columns = torch.arange(cols, device=values.device).expand_as(values)
    return torch.where(values == top, columns, cols).min(dim=1).values.clamp(max=cols - 1).to(torch.int32)


def predict_sigmoid(logits: torch.Tensor, out_probs: Optional[torch.Tensor] = None,
                    out_labels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (probabilities float32 [rows, cols], labels uint8 [rows, cols]) of PPI-style logits."""
    logits = _as_rows(logits.detach())
    rows, cols = logits.shape
    probs = _out(out_probs, (rows, cols), logits.dtype if logits.is_floating_point() else torch.float32, logits.device)
    labels = _out(out_labels, (rows, cols), torch.uint8, logits.device)
    if rows == 0 or cols == 0:
        return probs, labels
    if _kernel_route(logits) and _rows_ok(probs) and _rows_ok(labels):
        _lib.launch("relgnn_predict_sigmoid_f32", _lib.ptr(logits, rows_strided=True), _ld(logits), rows, cols,
                    _lib.ptr(probs, rows_strided=True), _ld(probs), _lib.ptr(labels, rows_strided=True), _ld(labels))
        return probs, labels
    e = torch.exp(-logits.abs())
    upper = 1.0 / (1.0 + e)                                  # the quotient the label rule compares, and the probability for x >= 0
    probs.copy_(torch.where(logits >= 0, upper, e / (1.0 + e)))
    labels.copy_(((logits > 0) & (upper > 0.5)).to(torch.uint8))
    return probs, labels


def predict_softmax(logits: torch.Tensor, out_probs: Optional[torch.Tensor] = None,
                    out_classes: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (probabilities float32 [rows, cols], classes int32 [rows]) of citation-style logits."""
    logits = _as_rows(logits.detach())
    rows, cols = logits.shape
    if cols < 1:
        raise ValueError("softmax over zero classes")
    probs = _out(out_probs, (rows, cols), logits.dtype, logits.device)
    classes = _out(out_classes, (rows,), torch.int32, logits.device)
    if rows == 0:
        return probs, classes
    if _kernel_route(logits) and _rows_ok(probs) and classes.is_contiguous():
        _lib.launch("relgnn_predict_softmax_f32", _lib.ptr(logits, rows_strided=True), _ld(logits), rows, cols,
                    _lib.ptr(probs, rows_strided=True), _ld(probs), _lib.ptr(classes))
        return probs, classes
    probs.copy_(torch.softmax(logits, dim=1))
    classes.copy_(_first_max(logits))
    return probs, classes


MAX_CANDIDATES = 8          # csrc/common.h: kMaxCandidates


def predict_candidates(logits: torch.Tensor, out_probs: Optional[torch.Tensor] = None,
                       out_predicted: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (probabilities float32 [rows, cols], predicted int32 [rows]) of VarMisuse-style logits: the head kernel's arithmetic
    (maximum; e = exp(x - m); sum = 1 + the other columns' e in index order; p = e / sum; the first largest p)."""
    logits = logits.detach()
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be [rows, cols >= 1], got %s" % (tuple(logits.shape),))
    logits = logits.contiguous()
    rows, cols = logits.shape
    probs = _out(out_probs, (rows, cols), logits.dtype, logits.device)
    predicted = _out(out_predicted, (rows,), torch.int32, logits.device)
    if rows == 0:
        return probs, predicted
    if _kernel_route(logits) and cols <= MAX_CANDIDATES and probs.is_contiguous() and predicted.is_contiguous():
        _lib.launch("relgnn_predict_candidates_f32", _lib.ptr(logits), rows, cols, _lib.ptr(probs), _lib.ptr(predicted))
        return probs, predicted
    top, first = logits.max(dim=1, keepdim=True).values, _first_max(logits).long().unsqueeze(1)
    e = torch.exp(logits - top)
    rest = torch.zeros_like(top)
    for c in range(cols):                                     # index order; the maximum's own 1 is added last
        rest = rest + torch.where(first == c, torch.zeros_like(top), e[:, c:c + 1])
    p = e / (1.0 + rest)
    probs.copy_(p)
    predicted.copy_(_first_max(p))
    return probs, predicted
