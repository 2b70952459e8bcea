"""One wrapper per librelgnn entry point (or family of entry points) behind the node-side Dense products: what an operand has to look
like for it, its scratch buffers, its argument list.  WHICH of them a product runs on is decided in dense.py (_route), which also
re-exports every name here under dense.X — callers keep saying dense.limb_gemm_tn, dense.column_sum, ...
"""
import ctypes

import torch

from . import _lib
from .config import settings as _cfg
from .handover import handover_word
from .weight_images import (GEMM_NN, GEMM_NT, GEMM_TN, WEIGHT_NN, WEIGHT_NT, _PerStream, _weight_image_shape, _weight_matrices,
                            weight_image, weight_limbs)

_LIMB_MIN_ROWS, _LIMB_MAX_K = 4096, 1024


# ---- what an operand must look like: one predicate per question ---------------------------------------------------------------------
def rows_aligned(t: torch.Tensor) -> bool:
    """fp32 device matrix, unit column stride, rows that do not overlap, every row 16-byte aligned: the limb and panel kernels
    (relgnn_limb_*, relgnn_panel_gemm_f32, relgnn_rgcn_fused_fwd) read float4."""
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0
            and (t.stride(0) >= t.shape[1] or t.shape[0] == 1)
            and t.data_ptr() % 16 == 0 and t.shape[0] < 2 ** 31 and t.shape[1] < 2 ** 31)


def rows_dense(t: torch.Tensor) -> bool:
    """Non-empty fp32 device matrix, unit column stride, rows that do not overlap (an expand()-backed gradient, strides (0, 1), would
    be read with ld = 0): relgnn_blaslt_gemm_f32 and relgnn_gemm_tn_stream_*_f32 take any leading dimension and alignment."""
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] > 0
            and t.shape[1] > 0 and (t.stride(0) >= t.shape[1] or t.shape[0] == 1))


def premask_ok(y: torch.Tensor, rows: int, cols: int) -> bool:
    """y [rows, cols] may be the activation output of a dact epilogue (relgnn_limb*_gemm_xf32_dact, _pc): aligned rows of that shape."""
    return y is not None and rows_aligned(y) and tuple(y.shape) == (rows, cols) and y.stride(0) >= cols


def bias_ok(bias, aligned: bool = False) -> bool:
    """No bias, or a contiguous fp32 device vector; aligned: at a 16-byte boundary (the limb and panel epilogues read float4)."""
    return bias is None or (bias.is_cuda and bias.is_contiguous() and bias.dtype == torch.float32
                            and (not aligned or bias.data_ptr() % 16 == 0))


def limb_shape_ok(rows, n: int, k: int, columns: int = 256) -> bool:
    """THE shape rule of the limb products: tall (rows = None: the caller's rows are gathered, any number), whole column chunks of
    `columns` (256, or the 128 of the panel kernels), whole k-tiles, and K <= 1024 — the error of the six-product sum grows faster
    with K than an fmaf chain's (2.2 x the fp32 product's at K = 1040 .. 4096)."""
    return (rows is None or rows >= _LIMB_MIN_ROWS) and n % columns == 0 and k % 16 == 0 and 16 <= k <= _LIMB_MAX_K


# ---- scratch --------------------------------------------------------------------------------------------------------------------------
_LIMB_WS = _PerStream()
_WORKSPACE = _PerStream()
_ZEROS = {}


def _per_stream(cache: _PerStream, device, numel: int, dtype, floor: int) -> torch.Tensor:
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.lookup(key)
    if ws is None or ws.numel() < numel:
        ws = cache.store(key, torch.empty(max(numel, floor), dtype=dtype, device=device))
    return ws


def _workspace(device) -> torch.Tensor:
    """hipBLASLt scratch (split-K / stream-K solutions write partial products there), one buffer per (device, stream):
    GEMMs issued on different streams may run concurrently and must not share it.  The library checks the size it is handed
    against the solution's need on every call (a cached solution that wants more fails and is re-queried, blaslt_gemm.hip)."""
    return _per_stream(_WORKSPACE, device, 64 << 20, torch.uint8, 0)


def _limb_ws(device, need: int) -> torch.Tensor:
    return _per_stream(_LIMB_WS, device, need, torch.bfloat16, 1 << 20)


def _zeros(device) -> torch.Tensor:
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(int(_lib.load_library().relgnn_panel_gemm_zeros_floats()), dtype=torch.float32, device=device)
    return z


# ---- passes -------------------------------------------------------------------------------------------------------------------------
def act_bwd_from_output(act: int, y: torch.Tensor, g: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """g * act'(y) with the derivative taken from the activation's output (relgnn_act_bwd_from_output); out may be g itself."""
    g = g if g.is_contiguous() else g.contiguous()
    if out is None:
        out = torch.empty_like(g)
    _lib.launch("relgnn_act_bwd_from_output", act, _lib.ptr(y), _lib.ptr(g), g.numel(), _lib.ptr(out))
    return out


def column_sum(g: torch.Tensor) -> torch.Tensor:
    """sum over rows of a [V, N] tensor (bias gradient).  torch's strided reduction took 330 us and rocBLAS gemv
    230 us for [32k, 121] on MI355X; the two-stage HIP kernel (csrc/dense_utils.hip) is bandwidth-bound."""
    if not g.is_cuda:
        return g.sum(0)
    V, N = g.shape
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    nbytes = _lib.load_library().relgnn_column_sum_workspace_bytes(V, N)
    ws = _lib.scratch(nbytes, g.device)
    _lib.launch("relgnn_column_sum", _lib.ptr(g, rows_strided=True), V, N, g.stride(0), _lib.ptr(out), _lib.ptr(ws), nbytes)
    return out


def col_absmax(x: torch.Tensor) -> torch.Tensor:
    """[cols] float32 on the device: the largest finite magnitude of every column of x [rows, cols] (relgnn_col_absmax_f32)."""
    cols = x.shape[1]
    if cols > 16 and cols % 4:
        # the kernel's wide form reads float4 columns: pad to the next multiple of 4 with zeros (a zero never is a column's largest
        # magnitude unless the column is zero) — e.g. the [V, L] bucket magnitudes of an 18-type aggregate-first layer
        return col_absmax(torch.nn.functional.pad(x, (0, (-cols) % 4)))[:cols]
    if not (rows_aligned(x) if cols > 16 else (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1)):
        x = x.contiguous()
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    nbytes = int(_lib.load_library().relgnn_col_absmax_workspace_bytes(x.shape[0], cols))
    ws = _lib.scratch(nbytes, x.device) if nbytes else None
    _lib.launch("relgnn_col_absmax_f32", _lib.ptr(x, rows_strided=True), x.stride(0) if x.shape[0] > 1 else cols, x.shape[0], cols,
            out.data_ptr(), _lib.ptr(ws), nbytes)
    return out


def absmax(x: torch.Tensor) -> torch.Tensor:
    """[1] float32 on the device: max |x| over the finite elements (relgnn_absmax_f32; no host round trip)."""
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.launch("relgnn_absmax_f32", _lib.ptr(x), x.numel(), out.data_ptr())
    return out


# ---- the exact-fp32 row-panel kernel ------------------------------------------------------------------------------------------------
def panel_gemm_supported(layout: int, a: torch.Tensor, b: torch.Tensor, n_out: int = None) -> bool:
    """Shapes relgnn_panel_gemm_f32 takes: fp32 device operands with 16-byte aligned dense rows, N % 64 == 0, K % 4 == 0
    (TN: M % 4 == 0 instead)."""
    if not (rows_aligned(a) and rows_aligned(b)):
        return False
    if layout == GEMM_NN:
        K, N = a.shape[1], b.shape[1]
    elif layout == GEMM_NT:
        K, N = a.shape[1], b.shape[0]
    else:
        K, N = a.shape[0], b.shape[1]
        if a.shape[1] % 4 != 0:
            return False
    if n_out is not None:
        N = n_out
    return N % 64 == 0 and (K % 4 == 0 or layout == GEMM_TN) and K > 0


def panel_gemm(layout: int, a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor = None, act: int = 0, *,
               a_rows: torch.Tensor = None, num_rows: int = None, b_select: torch.Tensor = None, rows_per_select: int = 0,
               batch: int = 1, strides=(0, 0, 0), split_k_rows: int = 0, dims=None, out: torch.Tensor = None) -> torch.Tensor:
    """relgnn_panel_gemm_f32 (csrc/panel_gemm.hip).  NN a @ b | NT a @ b^T | TN a^T @ b on the exact-fp32 matrix pipe.
      a_rows / num_rows : gathered left rows (NN / NT: output row r uses a[a_rows[r]], < 0 = zeros) or gathered reduction
                          rows of `a` (TN)
      b_select          : [num_rows / rows_per_select] int32, b is then [num_select, ...] and block p of rows_per_select output
                          rows multiplies b[b_select[p]]
      batch / strides   : independent products (element strides of a, b, out) or, with split_k_rows, K chunks -> out [batch, M, N]
      dims              : (M, N, K) when they do not follow from the operand shapes (batched / typed operands)"""
    if dims is not None:
        M, N, K = dims
    elif layout == GEMM_NN:
        M, K, N = (num_rows if a_rows is not None else a.shape[0]), a.shape[1], b.shape[-1]
    elif layout == GEMM_NT:
        M, K, N = (num_rows if a_rows is not None else a.shape[0]), a.shape[1], b.shape[-2]
    else:
        K, M, N = (num_rows if a_rows is not None else a.shape[0]), a.shape[1], b.shape[-1]
    if out is None:
        out = torch.empty((batch, M, N) if batch > 1 else (M, N), dtype=torch.float32, device=a.device)
    ldc = out.stride(-2)
    _lib.launch("relgnn_panel_gemm_f32", layout, act, a.data_ptr(), a.stride(-2), _lib.ptr(a_rows), b.data_ptr(), b.stride(-2),
            _lib.ptr(b_select), int(rows_per_select), b.stride(0) if b_select is not None else 0, _lib.ptr(bias),
            _lib.ptr(_zeros(a.device)), out.data_ptr(), ldc, M, N, K, batch, strides[0], strides[1],
            strides[2] if batch > 1 and strides[2] else (M * ldc if batch > 1 else 0), int(split_k_rows))
    return out


# ---- limb products: explicit limbs --------------------------------------------------------------------------------------------------
class Limbs:
    """An fp32 [rows, cols] matrix as three bf16 limbs per element in the tiled layout of csrc/limb_gemm.hip (include/relgnn.h:
    "limb tiles").  `data` is the flat bf16 buffer."""
    __slots__ = ("data", "rows", "cols")

    def __init__(self, data: torch.Tensor, rows: int, cols: int):
        self.data, self.rows, self.cols = data, int(rows), int(cols)

    def to_float64(self) -> torch.Tensor:
        """hi + mid + lo as float64 [rows, cols] (tests)."""
        RB, KT = (self.rows + 31) // 32, self.cols // 16
        t = self.data.view(RB, KT, 3, 2, 32, 8).double().sum(2)              # [RB, KT, h, i, 8]
        return t.permute(0, 3, 1, 2, 4).reshape(RB * 32, self.cols)[:self.rows]


def limb_split(x: torch.Tensor, transpose: bool = False, out: "Limbs" = None) -> "Limbs":
    """fp32 [R, C] -> the three bf16 limbs of x (or of x^T), x = hi + mid + lo exactly (relgnn_limb_split_f32)."""
    if not rows_aligned(x):
        x = x.contiguous()
    R, C = x.shape
    rows, cols = (C, R) if transpose else (R, C)
    if out is None:
        out = Limbs(torch.empty(int(_lib.load_library().relgnn_limb_elements(rows, cols)), dtype=torch.bfloat16, device=x.device), rows, cols)
    elif (out.rows, out.cols) != (rows, cols):
        raise ValueError("limb_split: out holds a [%d, %d] matrix, not [%d, %d]" % (out.rows, out.cols, rows, cols))
    _lib.launch("relgnn_limb_split_f32", x.data_ptr(), x.stride(0), R, C, 1 if transpose else 0, out.data.data_ptr())
    return out


def limb_gemm(a: "Limbs", b: "Limbs", bias: torch.Tensor = None, act: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """act(bias + A @ B^T) in fp32 from the limbs of A [M, K] and B [N, K] (relgnn_limb_gemm_f32): six bf16 MFMA products per
    fp32 product, fp32 accumulation — fp32-class accuracy at up to 2.7x the fp32-input MFMA rate."""
    if a.cols != b.cols:
        raise ValueError("limb_gemm: reduction lengths differ (%d, %d)" % (a.cols, b.cols))
    dev = a.data.device
    if out is None:
        out = torch.empty((a.rows, b.rows), dtype=torch.float32, device=dev)
    _lib.launch("relgnn_limb_gemm_f32", act, a.data.data_ptr(), b.data.data_ptr(), _lib.ptr(bias), _lib.ptr(_zeros(dev)), out.data_ptr(),
            out.stride(0), a.rows, b.rows, a.cols)
    return out


def limb_gemm_xf32(a: torch.Tensor, b: "Limbs", bias: torch.Tensor = None, act: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """act(bias + a @ B^T) with a fp32 [M, K] (dense rows) split inside the kernel and B [N, K] as limbs (relgnn_limb_gemm_xf32)."""
    if not rows_aligned(a):
        a = a.contiguous()
    M, K = a.shape
    if K != b.cols:
        raise ValueError("limb_gemm_xf32: reduction lengths differ (%d, %d)" % (K, b.cols))
    if out is None:
        out = torch.empty((M, b.rows), dtype=torch.float32, device=a.device)
    _lib.launch("relgnn_limb_gemm_xf32", act, a.data_ptr(), a.stride(0), b.data.data_ptr(), _lib.ptr(bias), _lib.ptr(_zeros(a.device)),
            out.data_ptr(), out.stride(0), M, b.rows, K)
    return out


# ---- limb products: a fp32 left operand against the limb image of weights -----------------------------------------------------------
def _handover(device) -> int:
    return handover_word(device).data_ptr()


def limb_gemm_weight(a: torch.Tensor, w, kind: str, bias: torch.Tensor = None, act: int = 0,
                     out: torch.Tensor = None, xmax: torch.Tensor = None, xgroups: int = 0, dact: int = 0,
                     dy: torch.Tensor = None) -> torch.Tensor:
    """act(bias + a @ B^T) (times dact'(dy) with dy [M, n], an activation's output) with B = the cached limb image of the weight
    operand w, a fp32 [M, K] split inside the kernel.  Five entry points, one product:
      xmax [M * xgroups] (per-row magnitudes of `a` from its producer, ops.segment._seg_reduce_raw(rowmax=)): the two-fp16-limb form,
                         relgnn_limb16_gemm_xf32 / _dact
      _limb_pc_ok        wave roles instead of k-loop phases (csrc/limb_gemm_pc.hip): the same bits, the matrix waves at their
                         MFMA-only time — relgnn_limb_gemm_xf32_pc, which carries dact itself
      otherwise          relgnn_limb_gemm_xf32 / _dact"""
    n, k = _weight_image_shape(_weight_matrices(w), kind)
    M = a.shape[0]
    if a.shape[1] != k:
        raise ValueError("limb_gemm_weight: a is [%d, %d], the weight operand has K = %d" % (M, a.shape[1], k))
    if out is None:
        out = torch.empty((M, n), dtype=torch.float32, device=a.device)
    left = (act, a.data_ptr(), a.stride(0))
    factor = (int(dact), dy.data_ptr(), dy.stride(0)) if dy is not None else ()
    result = (out.data_ptr(), out.stride(0), M, n, k)
    if xmax is not None:
        if xmax.numel() != M * xgroups or xmax.dtype != torch.float32 or not xmax.is_contiguous():
            raise ValueError("limb_gemm_weight: xmax must be a contiguous float32 [%d * %d]" % (M, xgroups))
        im = weight_image(w, kind, pair=True)
        _lib.launch("relgnn_limb16_gemm_xf32_dact" if factor else "relgnn_limb16_gemm_xf32", *left, xmax.data_ptr(), int(xgroups),
                im.buf.data_ptr(), im.wmax.data_ptr(), _lib.ptr(bias), _lib.ptr(_zeros(a.device)), *factor, *result)
        return out
    buf = weight_limbs(w, kind)
    if _limb_pc_ok(a, n, k, bias, act, dy, out, kind):
        _lib.launch("relgnn_limb_gemm_xf32_pc", *left, buf.data_ptr(), _lib.ptr(bias), *(factor or (int(dact), None, 0)), *result,
                _handover(a.device))
    else:
        _lib.launch("relgnn_limb_gemm_xf32_dact" if factor else "relgnn_limb_gemm_xf32", *left, buf.data_ptr(), _lib.ptr(bias),
                _lib.ptr(_zeros(a.device)), *factor, *result)
    return out


def _limb_pc_ok(a, n: int, k: int, bias, act: int, dy, out, kind: str) -> bool:
    """Shapes relgnn_limb_gemm_xf32_pc takes (config limb_pc): K % 128 == 0 (<= 1024), N % 256 == 0, N == 256 or K <= 256; ReLU / no
    activation.  limb_pc = fwd (the default): forward products only (WEIGHT_NN).  The kernel holds every CU for its whole run
    (one persistent 16-wave workgroup each); an input-gradient product runs next to the weight gradient on the side stream, whose
    workgroups then wait for CUs: measured in the C2 step, forward products 106 -> 87 us, input-gradient products 116 -> 128 us
    and the side stream's kernels twice as long (profiles/r05_g_limb_pc_step_timelines.txt)."""
    mode = _cfg.limb_pc
    if mode == "0" or (mode == "fwd" and kind != WEIGHT_NN):     # (the small input-gradient products, K <= 256 and N = 256, on it too: no
        return False                                              #  difference, 1.8115 vs 1.8101 ms over three alternations)
    if a.shape[0] < _LIMB_MIN_ROWS or not _lib.load_library().relgnn_limb_gemm_xf32_pc_supported(int(act), a.shape[0], n, k):
        return False                                              # (the shape list lives in the library: csrc/limb_gemm_pc.hip)
    return (a.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0
            and bias_ok(bias, aligned=True) and (dy is None or (dy.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0)))


def limb_dense(layout: int, a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor = None, act: int = 0,
               out: torch.Tensor = None, weight: bool = False) -> torch.Tensor:
    """NN act(bias + a @ b) | NT a @ b^T through relgnn_limb_dense_f32: b split into limbs in a per-(device, stream) scratch buffer, a
    split inside the product kernel.  weight: b is a parameter (or a view of one) — limb_gemm_weight, its limbs are kept across the
    products of a step."""
    if weight:
        return limb_gemm_weight(a, b, WEIGHT_NN if layout == GEMM_NN else WEIGHT_NT, bias, act, out)
    M, K = a.shape
    N = b.shape[1] if layout == GEMM_NN else b.shape[0]
    ws = _limb_ws(a.device, int(_lib.load_library().relgnn_limb_elements(N, K)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.launch("relgnn_limb_dense_f32", layout, act, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), _lib.ptr(bias),
            _lib.ptr(_zeros(a.device)), ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0), M, N, K)
    return out


def limb_dense_sel(layout: int, a: torch.Tensor, b, bias: torch.Tensor = None, act: int = 0, *,
                   a_rows: torch.Tensor = None, num_rows: int = None, b_select: torch.Tensor = None, rows_per_select: int = 0,
                   cached: bool = False, as_one: bool = False, image=None, out: torch.Tensor = None) -> torch.Tensor:
    """The limb product in 128 x 128 panels.  b: [K, N] / [N, K] (NN / NT) or, with b_select, [num_b, K, N] / [num_b, N, K];
    a_rows: int32 row ids of `a` per output row (< 0: zeros), num_rows output rows.  Three entry points:
      image (sel_image(b, layout), looked up by the caller) or cached=True (sel_weights_cacheable(b, layout)): b is the weight matrix /
               the LIST of per-type weight matrices themselves and their limbs come from the step's image cache — no split launch, no
               stacked copy of the weights: relgnn_limb_gemm_sel_xf32, or under config typed_pc the wave-role kernel
               relgnn_limb_gemm_sel_pc_xf32 (csrc/limb_gemm_pc_typed.hip: the same bits, every gathered row read once);
               as_one: the images one behind the other = the image of [w_0 | w_1 | ..] stacked along N: ONE product, L * N columns
      else     b is split into the per-(device, stream) scratch in front of the product: relgnn_limb_dense_sel_f32"""
    lib = _lib.load_library()
    K = a.shape[1]
    M = int(num_rows) if a_rows is not None else a.shape[0]
    if cached or image is not None:
        ws = _weight_matrices(b)
        N = ws[0].shape[1] if layout == GEMM_NN else ws[0].shape[0]
        im = image if image is not None else weight_image(ws, WEIGHT_NN if layout == GEMM_NN else WEIGHT_NT, separate=True)
        if as_one:
            return _sel_with_image(a, im, len(ws) * N, K, act, bias)
        if out is not None and (out.shape != (M, N) or out.dtype != torch.float32 or out.stride(1) != 1):
            raise ValueError("limb_dense_sel: out must be a float32 [%d, %d] matrix with dense rows" % (M, N))
        roles = ((_cfg.typed_pc == "1" or (_cfg.typed_pc == "fwd" and a_rows is not None and N == 256)) and b_select is not None
                 and bias is None and act == 0 and lib.relgnn_limb_gemm_sel_pc_supported(M, N, K, int(rows_per_select))
                 and (a_rows is None or a_rows.data_ptr() % 16 == 0))
        return _sel_with_image(a, im, N, K, act, bias, len(ws), a_rows, M, b_select, rows_per_select, out, roles)
    num_b = b.shape[0] if b.dim() == 3 else 1
    N = b.shape[-1] if layout == GEMM_NN else b.shape[-2]
    ws = _limb_ws(a.device, int(lib.relgnn_limb_elements((N + 127) // 128 * 128, K)) * num_b)
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.launch("relgnn_limb_dense_sel_f32", layout, act, a.data_ptr(), a.stride(0), _lib.ptr(a_rows), b.data_ptr(), b.stride(-2), num_b,
            b.stride(0) if b.dim() == 3 else 0, _lib.ptr(b_select), int(rows_per_select), _lib.ptr(bias), _lib.ptr(_zeros(a.device)),
            ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0), M, N, K)
    return out


def _sel_with_image(a: torch.Tensor, im, n: int, k: int, act: int = 0, bias: torch.Tensor = None, count: int = 1,
                    a_rows: torch.Tensor = None, m: int = None, b_select: torch.Tensor = None, rows_per_select: int = 0,
                    out: torch.Tensor = None, roles: bool = False) -> torch.Tensor:
    """act(bias + a @ B^T) on the 128-column panels, B [n, k] = the limb image im — or `count` images one behind the other, block p of
    rows_per_select output rows against image b_select[p].  roles: relgnn_limb_gemm_sel_pc_xf32 (no bias, no activation)."""
    m = a.shape[0] if m is None else m
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    left = (a.data_ptr(), a.stride(0), _lib.ptr(a_rows), im.buf.data_ptr(), count, _lib.ptr(b_select), int(rows_per_select))
    result = (_lib.ptr(_zeros(a.device)), out.data_ptr(), out.stride(0), m, n, k)
    if roles:
        _lib.launch("relgnn_limb_gemm_sel_pc_xf32", *left, *result, _handover(a.device))
    else:
        _lib.launch("relgnn_limb_gemm_sel_xf32", act, *left, _lib.ptr(bias), *result)
    return out


# ---- limb products: weight gradients ------------------------------------------------------------------------------------------------
def limb_tn_supported(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (rows_aligned(a) and rows_aligned(b) and a.shape[0] == b.shape[0] and a.shape[0] >= _LIMB_MIN_ROWS and a.shape[1] % 32 == 0
            and b.shape[1] % 256 == 0)


def limb_gemm_tn(a: torch.Tensor, b: torch.Tensor, amax: torch.Tensor = None, bmax: torch.Tensor = None) -> torch.Tensor:
    """a^T @ b for a [V, J], b [V, C] (weight gradient) through relgnn_limb_gemm_tn_f32 + the in-order slab sum.
    amax, bmax (device floats): the two-fp16-limb form — [J] / [C] magnitudes per column (col_absmax(): one power-of-two scale
    per column of each operand), [1] / [1] (absmax(): one scale per operand), or any count that divides the operand's width (one
    per group of consecutive columns)."""
    V, J = a.shape
    C = b.shape[1]
    Z = int(_lib.load_library().relgnn_limb_gemm_tn_chunks(V, J, C))
    if Z <= 0:
        raise ValueError("limb_gemm_tn: unsupported shape [%d, %d]^T @ [%d, %d]" % (V, J, V, C))
    parts = torch.empty((Z, J, C), dtype=torch.float32, device=a.device)
    operands = (a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0))
    if amax is not None:
        na, nb = amax.numel(), bmax.numel()
        if na < 1 or nb < 1 or J % na or C % nb or amax.dtype != torch.float32 or bmax.dtype != torch.float32:
            raise ValueError("limb_gemm_tn: the magnitude counts (%d, %d) must divide the operand widths (%d, %d)" % (na, nb, J, C))
        _lib.launch("relgnn_limb16_gemm_tn_f32", *operands, amax.data_ptr(), J // na, bmax.data_ptr(), C // nb, parts.data_ptr(), V, J, C)
    else:
        _lib.launch("relgnn_limb_gemm_tn_f32", *operands, parts.data_ptr(), V, J, C)
    return sum_slabs_tail(parts, a, b, V - V % 32)


def sum_slabs_tail(parts: torch.Tensor, a: torch.Tensor, b: torch.Tensor, head: int) -> torch.Tensor:
    """sum_z parts[z] in slab order + a[head:]^T @ b[head:] (the rows the slabs left out, exact fp32), one pass
    (relgnn_sum_slabs_tail_f32): torch.sum + a second product + an accumulate were three launches, and the library's pick for a
    [16, 128]^T @ [16, 640] leftover took 191 us (C3 timeline)."""
    Z, M, N = parts.shape
    R = a.shape[0] - head
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.launch("relgnn_sum_slabs_tail_f32", _lib.ptr(parts), Z, M, N, a[head:].data_ptr() if R else None, a.stride(0),
            b[head:].data_ptr() if R else None, b.stride(0), R, _lib.ptr(out))
    return out


def limb_tn_tiles_supported(a: torch.Tensor, g: torch.Tensor, a_rows: torch.Tensor, rows_per_tile: int) -> bool:
    """Shapes relgnn_limb_gemm_tn_tiles_f32 takes (the typed weight-gradient partials of ops.typed_linear)."""
    return (_cfg.limb_gemm and rows_aligned(a) and rows_aligned(g) and a_rows.is_cuda and a_rows.dtype == torch.int32
            and a_rows.is_contiguous() and a_rows.data_ptr() % 16 == 0 and a_rows.numel() == g.shape[0] and rows_per_tile % 32 == 0
            and g.shape[0] % rows_per_tile == 0 and a.shape[1] % 64 == 0 and g.shape[1] % 128 == 0)


def limb_gemm_tn_tiles(a: torch.Tensor, g: torch.Tensor, a_rows: torch.Tensor, rows_per_tile: int) -> torch.Tensor:
    """part[z] = a[a_rows[tile z]]^T @ g[tile z] for the P / rows_per_tile tiles of a compact pair table (a [*, J] node table, g [P, C]
    the table's gradient, a_rows [P] int32, < 0 = padding): [tiles, J, C], three bf16 limbs per value, gathered / transposed /
    split in flight (relgnn_limb_gemm_tn_tiles_f32)."""
    P, C = g.shape
    J = a.shape[1]
    part = torch.empty((P // rows_per_tile, J, C), dtype=torch.float32, device=g.device)
    _lib.launch("relgnn_limb_gemm_tn_tiles_f32", a.data_ptr(), a.stride(0), a_rows.data_ptr(), g.data_ptr(), g.stride(0),
            _lib.ptr(_zeros(g.device)), part.data_ptr(), P, int(rows_per_tile), J, C)
    return part


# ---- the streaming weight-gradient kernel (csrc/gemm_tn_stream.hip) -------------------------------------------------------------------
_TN_BLOCKS_MAX_OUT = 128 * 1024      # outputs of the block form (measured up to [128, 640]; its partial sums are chunks * M * N floats)
_TN_MAX_ROWS = 1 << 18


def _tn_stream(name: str, a: torch.Tensor, b: torch.Tensor, *result) -> None:
    V, M = a.shape
    N = b.shape[1]
    nbytes = _lib.load_library().relgnn_gemm_tn_stream_workspace_bytes(M, N, V)
    ws = _lib.scratch(nbytes, a.device)
    _lib.launch(name, _lib.ptr(a, rows_strided=True), a.stride(0), _lib.ptr(b, rows_strided=True), b.stride(0), *result, _lib.ptr(ws), nbytes)


def tn_stream_gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """a^T @ b for a [V, M], b [V, N] through the streaming weight-gradient kernel; with `out` (contiguous [M, N]): out += a^T @ b."""
    (V, M), N = a.shape, b.shape[1]
    accumulate = out is not None
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _tn_stream("relgnn_gemm_tn_stream_f32", a, b, _lib.ptr(out), N, M, N, V, 1 if accumulate else 0)
    return out


def tn_stream_into(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> None:
    """out[:] = a^T @ b through the streaming weight-gradient kernel, `out` a [M, N] block of a wider row-major matrix (dense rows,
    any row stride): the two column blocks of a GRU's recurrent-kernel gradient are written in place, no zeros + copies + add."""
    (V, M), N = a.shape, b.shape[1]
    if out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise ValueError("tn_stream_into: out must be a float32 [%d, %d] block with dense rows" % (M, N))
    _tn_stream("relgnn_gemm_tn_stream_f32", a, b, out.data_ptr(), out.stride(0), M, N, V, 0)


def tn_stream_blocks_ok(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (_cfg.tn == "stream" and a.is_cuda and a.shape[1] * b.shape[1] <= _TN_BLOCKS_MAX_OUT and 0 < a.shape[0] <= _TN_MAX_ROWS
            and rows_dense(a) and rows_dense(b))


def tn_stream_blocks(a: torch.Tensor, b: torch.Tensor, L: int) -> torch.Tensor:
    """[L, M, N / L]: block l = a^T @ b[:, l * N / L : (l + 1) * N / L] for a [V, M], b [V, N] — ONE pass of the streaming
    weight-gradient kernel over a, every block a dense matrix of its own (relgnn_gemm_tn_stream_blocks_f32)."""
    (V, M), N = a.shape, b.shape[1]
    bc = N // L
    out = torch.empty((L, M, bc), dtype=torch.float32, device=a.device)
    _tn_stream("relgnn_gemm_tn_stream_blocks_f32", a, b, out.data_ptr(), bc, M * bc, M, N, bc, V, 0)
    return out


def tn_stream_group_ok(products) -> bool:
    """May these (a [V, M], b [V, N], out [M, N] block) triples go through relgnn_gemm_tn_stream_group_f32?  At most four, the same
    V, whole 64 x 64 tiles, 8-byte aligned operands with even row strides."""
    if not (_cfg.tn == "stream" and 1 <= len(products) <= 4):
        return False
    V = products[0][0].shape[0]
    for a, b, out in products:
        if not (a.is_cuda and a.dtype == b.dtype == out.dtype == torch.float32 and a.shape[0] == b.shape[0] == V and 0 < V <= _TN_MAX_ROWS
                and a.shape[1] % 64 == 0 and b.shape[1] % 64 == 0 and out.shape == (a.shape[1], b.shape[1])
                and all(t.stride(1) == 1 and t.stride(0) % 2 == 0 and t.data_ptr() % 8 == 0 for t in (a, b))
                and out.stride(1) == 1 and out.stride(0) >= out.shape[1]):
            return False
    return sum(a.shape[1] * b.shape[1] for a, b, _ in products) <= 4 * _TN_BLOCKS_MAX_OUT


def tn_stream_group(products, colsum: torch.Tensor = None) -> None:
    """out_i[:] = a_i^T @ b_i for every (a_i, b_i, out_i) — ONE pass of the streaming weight-gradient kernel and one reduction launch
    for all of them (relgnn_gemm_tn_stream_group_f32); colsum (contiguous [N_0]): also the column sums of b_0, the bias gradient of
    the layer whose kernel gradient product 0 is."""
    n = len(products)
    V = products[0][0].shape[0]
    vp, i64, i32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    M = i32(*[a.shape[1] for a, _, _ in products])
    N = i32(*[b.shape[1] for _, b, _ in products])
    nbytes = _lib.load_library().relgnn_gemm_tn_stream_group_workspace_bytes(n, M, N, V, 1 if colsum is not None else 0)
    ws = _lib.scratch(nbytes, products[0][0].device)
    per_operand = [arg for i in range(3) for arg in (vp(*[p[i].data_ptr() for p in products]), i64(*[p[i].stride(0) for p in products]))]
    _lib.launch("relgnn_gemm_tn_stream_group_f32", n, *per_operand, M, N, V, _lib.ptr(colsum), _lib.ptr(ws), nbytes)
