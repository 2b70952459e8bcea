"""Segment reduce (csrc/seg_reduce.hip): the gather-reduce launch with its hub-split route, and its autograd wrappers.

`unsorted_segment_{sum,mean,max,sqrt_n}` mirror the TF ops returned by the reference's
get_aggregation_function (utils/utils.py:23-33), same argument names and meaning.
`seg_gather_reduce` is the fused form the layer functions use: the gather
(tf.nn.embedding_lookup), the per-message scale and the segment reduction in ONE kernel.
"""
import warnings
from typing import Optional

import torch

from .. import _lib
from ..activations import FUSABLE_ACTS as _FUSABLE_ACTS, activation_id, activation_of_id, apply_activation, get_activation
from ..dense import act_bwd_from_output, dense_act
from ..graph import GatherReducePlan, SplitPlan, build_segment_plan, split_plan_of

_MODE_IDS = {
    "sum": _lib.AGG_SUM, "unsorted_segment_sum": _lib.AGG_SUM,
    "max": _lib.AGG_MAX, "unsorted_segment_max": _lib.AGG_MAX,
    "mean": _lib.AGG_MEAN, "unsorted_segment_mean": _lib.AGG_MEAN,
    "sqrt_n": _lib.AGG_SQRT_N, "unsorted_segment_sqrt_n": _lib.AGG_SQRT_N,
}


def aggregation_mode_id(aggregation_fun: Optional[str]) -> int:
    """Same accepted strings and error as get_aggregation_function (utils/utils.py:23-33)."""
    if aggregation_fun not in _MODE_IDS:
        raise ValueError("Unknown aggregation function '%s'!" % aggregation_fun)
    return _MODE_IDS[aggregation_fun]


def _check_f32(x: torch.Tensor, what: str):
    if x.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (what, x.dtype))


def _seg_reduce_split(mode, X, sp: SplitPlan, col, w, num_out, act):
    first = _lib.AGG_MAX if mode == _lib.AGG_MAX else _lib.AGG_SUM
    parts = _seg_reduce_raw(first, X, sp.virtual_rowptr, 1, col, w, sp.num_virtual)
    out = _seg_reduce_raw(first, parts, sp.combine_rowptr, 1, sp.iota, None, num_out)
    if mode in (_lib.AGG_MEAN, _lib.AGG_SQRT_N):
        n = sp.lengths.clamp(min=1).to(torch.float32).unsqueeze(1)
        out = out / (n if mode == _lib.AGG_MEAN else torch.sqrt(n))
    return apply_activation(activation_of_id(act), out)


def acc64_supported(D: int) -> bool:
    """Row widths relgnn_seg_reduce_acc64_fwd takes (the one-wave-per-row kernels)."""
    return D % 4 == 0 and 128 < D <= 1024


def _float4_rows(X) -> bool:
    """Every row of X starts on a 16-byte boundary (the one-wave-per-row kernels read float4 pieces)."""
    return X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0


def rowmax_supported(X, rowptr, stride, acc64: bool = False) -> bool:
    """relgnn_seg_reduce_fwd_rowmax takes this gather (one wave holds a whole output row; not the hub-split route)."""
    D = X.shape[1]
    return (not acc64 and split_plan_of(rowptr, stride) is None and X.is_cuda and D % 4 == 0 and 128 < D <= 1024
            and _float4_rows(X))


def _seg_reduce_raw(mode, X, rowptr, stride, col, w, num_out, act=_lib.ACT_LINEAR, acc64: bool = False, rowmax=None):
    """acc64: float64 bucket accumulators (relgnn_seg_reduce_acc64_fwd) — for sums that feed a GEMM, never for values that
    stand for the reference's own segment sums.  Split (hub) plans keep the float32 two-pass route.
    rowmax: a [num_out] float32 tensor that receives the largest magnitude of every output row (rowmax_supported)."""
    split = split_plan_of(rowptr, stride)
    if split is not None:
        return _seg_reduce_split(mode, X, split, col, w, num_out, act)
    D = X.shape[1]
    out = torch.empty((num_out, D), dtype=torch.float32, device=X.device)
    args = (mode, _lib.ptr(X, rows_strided=True), X.shape[0], X.stride(0), D, _lib.ptr(rowptr), num_out, stride, _lib.ptr(col), _lib.ptr(w),
            act, _lib.ptr(out), D)
    if rowmax is not None:
        _lib.launch("relgnn_seg_reduce_fwd_rowmax", *args, _lib.ptr(rowmax))
    elif acc64 and mode != _lib.AGG_MAX and acc64_supported(D) and _float4_rows(X):
        _lib.launch("relgnn_seg_reduce_acc64_fwd", *args)
    else:
        _lib.launch("relgnn_seg_reduce_fwd", *args)
    return out


class _SegGatherReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, plan: GatherReducePlan, mode: int, act: int):
        _check_f32(X, "X")
        if X.dim() != 2 or X.shape[0] != plan.num_rows_x:
            raise ValueError("X must be [%d, D], got %s" % (plan.num_rows_x, tuple(X.shape)))
        if X.stride(1) != 1 or (mode == _lib.AGG_MAX and not X.is_contiguous()):
            X = X.contiguous()
        out = _seg_reduce_raw(mode, X, plan.rowptr, plan.stride, plan.col, plan.w, plan.num_out, act)
        ctx.plan, ctx.mode, ctx.act = plan, mode, act
        need_x = mode == _lib.AGG_MAX
        need_out = need_x or act != _lib.ACT_LINEAR
        ctx.save_for_backward(X if need_x else None, out if need_out else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        plan, mode, act = ctx.plan, ctx.mode, ctx.act
        X, out = ctx.saved_tensors
        gout = gout.contiguous()
        D = gout.shape[1]
        if act != _lib.ACT_LINEAR:
            gout = act_bwd_from_output(act, out, gout)
        if mode == _lib.AGG_MAX:
            if act != _lib.ACT_LINEAR:
                raise RuntimeError("max aggregation is never fused with an activation epilogue")
            gsel = torch.empty_like(gout)
            _lib.launch("relgnn_seg_max_count", _lib.ptr(X), X.stride(0), D, _lib.ptr(plan.rowptr), plan.num_out, plan.stride,
                        _lib.ptr(plan.col), _lib.ptr(plan.w), _lib.ptr(out), _lib.ptr(gout), D, _lib.ptr(gsel))
            gX = torch.empty((plan.num_rows_x, D), dtype=torch.float32, device=gout.device)
            _lib.launch("relgnn_seg_max_bwd", _lib.ptr(X), X.stride(0), D, _lib.ptr(plan.rowptr_b), plan.num_rows_x, plan.stride_b,
                        _lib.ptr(plan.col_b), _lib.ptr(plan.w_bwd(_lib.AGG_SUM)), _lib.ptr(out), _lib.ptr(gsel), D, _lib.ptr(gX), D)
            return gX, None, None, None
        # sum / mean / sqrt_n: the gradient is the same gather-reduce over the transposed buckets
        gX = _seg_reduce_raw(_lib.AGG_SUM, gout, plan.rowptr_b, plan.stride_b, plan.col_b,
                             plan.w_bwd(mode), plan.num_rows_x)
        return gX, None, None, None


def seg_gather_reduce(X: torch.Tensor, plan: GatherReducePlan, aggregation: str = "sum",
                      activation: Optional[str] = None) -> torch.Tensor:
    """out[s] = act( AGG_{p in segment s} w[p] * X[col[p]] )  — one fused HIP kernel.

    `activation` is fused as an epilogue when its derivative is recoverable from the output
    (everything in get_activation except gelu); gelu is applied by the caller."""
    mode = aggregation_mode_id(aggregation)
    act = activation_id(activation)
    if act not in _FUSABLE_ACTS or mode == _lib.AGG_MAX and act != _lib.ACT_LINEAR:
        raise ValueError("activation %r cannot be fused into the reduce epilogue" % activation)
    return _SegGatherReduce.apply(X, plan, mode, act)


# ---- drop-in tf.unsorted_segment_* --------------------------------------------------------
class SegmentPlanCache:
    """Plans for raw (segment_ids, num_segments) pairs, keyed by tensor identity."""

    def __init__(self, size=8):
        self._d = {}
        self._order = []
        self._size = size

    def get(self, segment_ids: torch.Tensor, num_segments: int) -> GatherReducePlan:
        key = (segment_ids.data_ptr(), segment_ids._version, segment_ids.numel(), int(num_segments))
        hit = self._d.get(key)
        if hit is not None:
            return hit[1]
        ids = segment_ids.to(torch.int32).contiguous()
        M = ids.numel()
        segments = int(num_segments)
        if M > 0:
            lo, hi = int(ids.min()), int(ids.max())
            if hi >= num_segments:  # TF-CPU: InvalidArgumentError
                raise ValueError("segment id out of range [0, %d)" % num_segments)
            if lo < 0:
                # tf.unsorted_segment_*: "if the given segment ID is negative, the value is dropped".  Dropped rows go
                # to one extra bucket behind the real ones; the caller slices it off (and autograd's slice backward
                # hands those rows a zero gradient).
                ids = torch.where(ids < 0, torch.full_like(ids, segments), ids)
                segments += 1
        num_segments = segments
        rowptr, perm, _ = build_segment_plan(ids, num_segments)
        inv = torch.empty_like(perm)
        _lib.launch("relgnn_invert_perm", _lib.ptr(perm), M, _lib.ptr(inv))
        plan = GatherReducePlan(
            rowptr=rowptr, stride=1, col=perm, w=None, num_out=num_segments, num_rows_x=M,
            rowptr_b=torch.arange(M + 1, dtype=torch.int32, device=ids.device), stride_b=1, col_b=ids,
            pos_b=inv, num_messages=M)
        self._d[key] = (segment_ids, plan)
        self._order.append(key)
        while len(self._order) > self._size:
            self._d.pop(self._order.pop(0), None)
        return plan


_SEGMENT_PLANS = SegmentPlanCache()


def _unsorted_segment(mode_name, data, segment_ids, num_segments):
    if data.dim() == 1:
        return _unsorted_segment(mode_name, data.unsqueeze(1), segment_ids, num_segments).squeeze(1)
    lead = data.shape[0]
    flat = data.reshape(lead, -1)
    plan = _SEGMENT_PLANS.get(segment_ids, int(num_segments))
    out = _SegGatherReduce.apply(flat, plan, aggregation_mode_id(mode_name), _lib.ACT_LINEAR)
    if plan.num_out > int(num_segments):          # the bucket of rows with negative ids (dropped, like TF)
        out = out[:int(num_segments)]
    return out.reshape((int(num_segments),) + tuple(data.shape[1:]))


def unsorted_segment_sum(data, segment_ids, num_segments):
    """tf.unsorted_segment_sum(data, segment_ids, num_segments) on the HIP path."""
    return _unsorted_segment("sum", data, segment_ids, num_segments)


def unsorted_segment_mean(data, segment_ids, num_segments):
    return _unsorted_segment("mean", data, segment_ids, num_segments)


def unsorted_segment_sqrt_n(data, segment_ids, num_segments):
    return _unsorted_segment("sqrt_n", data, segment_ids, num_segments)


def unsorted_segment_max(data, segment_ids, num_segments):
    """Empty segments yield float32 lowest (-3.4028235e38), as TF does."""
    return _unsorted_segment("max", data, segment_ids, num_segments)


# ---- CSR rows times a row table: sparse node features through the input projection (csrc/csr_project.hip) --------------------
ROUTES = {"csr_project": None,       # which implementation the last csr_rows_project took: "hip", "composition" or "dense"
          "rgcn_rows": None}         # the rows the last aggregate_then_transform computed: "targets" (num_targets of them) or "all"
_WARNED = set()


def csr_project_supported(n: int) -> bool:
    """Row widths relgnn_csr_project_f32 takes (relgnn_csr_project_supported, restated: asked before the library is loaded)."""
    return n % 4 == 0 and 4 <= n <= 1024


def _csr_project_raw(structure, table, act: int, y=None):
    """One launch of relgnn_csr_project_f32 over `structure` (rowptr / col / val / slabs / combos of one device): the forward with
    the epilogue `act` (y None), or the gradient form that scales every gathered row of `table` by act'(y row)."""
    n = table.shape[1]
    def float4_rows(t):                   # dense rows on 16-byte boundaries, any leading dimension; anything else is copied
        ok = t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0
        return t if ok else t.contiguous()
    table = float4_rows(table)
    y = float4_rows(y) if y is not None else None
    out = torch.empty((structure.num_rows, n), dtype=torch.float32, device=table.device)
    ws = torch.empty((structure.ws_rows, n), dtype=torch.float32, device=table.device) if structure.ws_rows else None
    _lib.launch("relgnn_csr_project_f32", act, _lib.ptr(structure.rowptr), structure.num_rows, _lib.ptr(structure.col),
                _lib.ptr(structure.val), structure.nnz, _lib.ptr(table, rows_strided=True), table.shape[0], max(table.stride(0), n),
                _lib.ptr(y, rows_strided=True), max(y.stride(0), n) if y is not None else 0, n,
                _lib.ptr(structure.slabs) if structure.slabs.shape[0] else None, structure.slabs.shape[0],
                _lib.ptr(structure.combos) if structure.combos.shape[0] else None, structure.combos.shape[0], _lib.ptr(ws),
                structure.ws_rows, _lib.ptr(out), n)
    return out


class _CsrRowsProject(torch.autograd.Function):
    """out = act(rows @ weight) for a CSR container: one launch forward, one launch over the transposed structure backward
    (dW[f] = sum_v X[v, f] * dOut[v] * act'(out[v])).  No gradient towards the container: the features are data.
    With a `sink` the backward's launch runs over the container's named rows (a CSR of T rows, tasks/sparse_features.py NamedRows):
    the [T, n] result goes to the sink with the words it belongs to, and the weight receives no gradient tensor at all."""

    @staticmethod
    def forward(ctx, weight, rows, act: int, sink=None):
        out = _csr_project_raw(rows.rows, weight, act)
        ctx.rows, ctx.act, ctx.sink = rows, act, sink
        ctx.save_for_backward(out if act != _lib.ACT_LINEAR else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        (out,) = ctx.saved_tensors
        if ctx.sink is None:
            return _csr_project_raw(ctx.rows.transposed, gout, ctx.act, out), None, None, None
        ctx.sink.check(ctx.rows)              # (RuntimeError: a second deposit in one step, a container without named rows)
        named = ctx.rows.named_rows()
        if named.count:
            values = _csr_project_raw(named.structure, gout, ctx.act, out)
        else:                                 # no word named: nothing to launch
            values = torch.empty((0, gout.shape[1]), dtype=torch.float32, device=gout.device)
        ctx.sink.deposit(named, values)
        return None, None, None, None


def _csr_rows_composition(rows, weight, act: int):
    """The same sum in torch: index_select, scale, index_add_ in ascending entry order (any device and dtype)."""
    s = rows.rows
    terms = weight.index_select(0, s.col.long()) * s.val.to(weight.dtype).unsqueeze(1)
    out = torch.zeros((s.num_rows, weight.shape[1]), dtype=weight.dtype, device=weight.device).index_add_(0, s.row_ids(), terms)
    return apply_activation(activation_of_id(act), out)


def csr_rows_project(rows, weight: torch.Tensor, act_id: int = _lib.ACT_LINEAR, row_gradient_sink=None) -> torch.Tensor:
    """act(X @ weight) [V, n] for sparse features `rows` (tasks.sparse_features.SparseRows, [V, F]) and weight [F, n].

    float32 GPU operands of a width the kernel takes run csrc/csr_project.hip (gelu: the linear kernel, then the torch activation,
    as the Dense route); any other GPU shape densifies the container on the device and takes the Dense route, with one warning;
    CPU tensors and other dtypes take the torch composition.  ROUTES["csr_project"] says which.  A column that is not stored
    contributes nothing, even against a non-finite weight (the dense product gives 0 * inf = NaN).

    row_gradient_sink (models.optimizer.RowGradientSink, owned by the optimizer that registered `weight` as row-deferred with a
    compact gradient): the backward deposits (words, slot, values [T, n]) there — the rows of the weight gradient that the
    container names, bit for bit — and weight.grad stays None; no [F, n] tensor is allocated.  Only the kernel route takes a sink
    (anything else is a ValueError), and the container must carry its named rows (SparseRows.named_rows) before the backward."""
    if getattr(rows, "requires_grad", False) or rows.rows.val.requires_grad:
        raise ValueError("csr_rows_project: the feature container requires grad, but the features are data: no gradient towards "
                         "them exists")
    if weight.dim() != 2 or weight.shape[0] != rows.shape[1]:
        raise ValueError("weight must be [%d, n], got %s" % (rows.shape[1], tuple(weight.shape)))
    if rows.device != weight.device:
        raise ValueError("csr_rows_project: the features live on %s, the weight on %s" % (rows.device, weight.device))
    n = weight.shape[1]
    if row_gradient_sink is not None and not (weight.is_cuda and weight.dtype == torch.float32 and csr_project_supported(n)):
        raise ValueError("csr_rows_project: a row gradient sink needs the CSR kernel (a float32 GPU weight with rows of a multiple of "
                         "4 up to 1024 floats); got %s %s rows of %d" % (weight.device, weight.dtype, n))
    if not (weight.is_cuda and weight.dtype == torch.float32):
        ROUTES["csr_project"] = "composition"
        return _csr_rows_composition(rows, weight, act_id)
    if not csr_project_supported(n):
        if n not in _WARNED:
            _WARNED.add(n)
            warnings.warn("csr_rows_project: rows of %d floats are not taken by the CSR kernel (a multiple of 4 up to 1024 is); "
                          "the features are densified on the device for the Dense route" % n)
        ROUTES["csr_project"] = "dense"
        return dense_act(rows.to_dense(), weight, None, act_id)
    ROUTES["csr_project"] = "hip"
    if act_id in _FUSABLE_ACTS:
        return _CsrRowsProject.apply(weight, rows, act_id, row_gradient_sink)
    return apply_activation(activation_of_id(act_id), _CsrRowsProject.apply(weight, rows, _lib.ACT_LINEAR, row_gradient_sink))


def _mode_factor(graph, mode: int):
    """d(finalised aggregate)/d(raw sum) per target node: 1, 1/max(n,1) or 1/sqrt(max(n,1))."""
    if mode == _lib.AGG_SUM:
        return None
    n = graph.messages_per_target()
    return (1.0 / n) if mode == _lib.AGG_MEAN else (1.0 / torch.sqrt(n))


def _raw_sum_gradient(gout, graph, mode: int, rows: int = None):
    """The gradient of the raw bucket sums from that of the finalised aggregate: gout * _mode_factor per row, contiguous.  rows: gout
    holds the first `rows` nodes only (ops/rgcn.py, target rows only)."""
    f = _mode_factor(graph, mode)
    if f is not None and rows is not None and rows < f.shape[0]:
        f = f[:rows]
    return (gout * f.unsqueeze(1)).contiguous() if f is not None else gout.contiguous()


# ---- materialised messages: scale + activation fused into the segment reduce ------------------------------------
class _MessageActReduce(torch.autograd.Function):
    """out[v] = f_mode( sum_{m -> v} act( w_m * msgs[m] ) ) for a message tensor [M, D] in the reference's type-major
    order (gnns/gnn_edge_mlp.py:104-116): no elementwise pass over [M, D] forward, one fused pass backward."""

    @staticmethod
    def forward(ctx, msgs, graph, w, mode: int, act: int):
        msgs = msgs.contiguous()
        M, D = msgs.shape
        plan = graph.plan_messages()
        out = torch.empty((graph.V, D), dtype=torch.float32, device=msgs.device)
        _lib.launch("relgnn_seg_reduce_msgact_fwd", mode, act, _lib.ptr(msgs), M, D, D, _lib.ptr(plan.rowptr), graph.V, plan.stride,
                    _lib.ptr(plan.col), _lib.ptr(w), _lib.ptr(out), D)
        ctx.graph, ctx.w, ctx.mode, ctx.act = graph, w, mode, act
        ctx.save_for_backward(msgs)
        return out

    @staticmethod
    def backward(ctx, gout):
        graph, w, mode, act = ctx.graph, ctx.w, ctx.mode, ctx.act
        (msgs,) = ctx.saved_tensors
        M, D = msgs.shape
        gagg = _raw_sum_gradient(gout, graph, mode)
        plan = graph.plan_messages()
        w_orig = graph.w_original_order(w) if w is not None else None
        gX = torch.empty_like(msgs)
        _lib.launch("relgnn_msg_act_bwd", act, _lib.ptr(msgs), D, _lib.ptr(w_orig), _lib.ptr(plan.col_b), _lib.ptr(gagg), M, _lib.ptr(gX))
        return gX, None, None, None, None


def message_act_reduce(msgs, graph, w, aggregation: str, activation: Optional[str]):
    """Sum-like aggregations only (max: apply the activation, then seg_gather_reduce over plan_messages()); graphs with hub
    buckets take that route too (its gather-reduce splits long buckets into chunked virtual rows)."""
    mode = aggregation_mode_id(aggregation)
    if mode == _lib.AGG_MAX or msgs.shape[1] % 4 != 0 or graph.has_long_buckets:
        if w is not None:
            msgs = graph.w_original_order(w).unsqueeze(1) * msgs
        msgs = apply_activation(get_activation(activation), msgs)
        return seg_gather_reduce(msgs, graph.plan_messages(), aggregation, None)
    return _MessageActReduce.apply(msgs, graph, w, mode, activation_id(activation))

