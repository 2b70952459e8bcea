"""Node-side dense layers (Keras `Dense` of the reference: y = x @ kernel (+ bias), kernel [in, out]): which kernel each of their
products runs on, their autograd functions and the public entry points.

Three products per layer and step.  The forward  act(x @ kernel + bias)  and the input gradient  g @ kernel^T  go through lib_gemm,
which asks _route() — THE place that looks at operands and switches — and launches what it answers.  On the default route
(config.settings.gemm = limb) tall operands run on the limb kernels of csrc/limb_gemm*.hip: every fp32 value as three bf16 limbs
(exact), six bf16 MFMA products per fp32 product, fp32 accumulation, the activation and the activation gradient of the layer below
in the epilogue, the weights' limb images cached across the step (weight_images.py).  Everything the limb shape rule does not take
is an exact-fp32 library GEMM with a cached solution (relgnn_blaslt_gemm_f32: hipBLASLt, looked up once per (layout, N, K, V / 4096)
instead of for every new node count).  The weight gradient  dW = x^T @ g  reduces over the node dimension (K = V ~ 3e4 .. 1e6, output
<= 256 x 768), where a single library call leaves most of the 256 CUs idle: matmul_tn_splitk sends outputs up to 256 x 256 to the
streaming MFMA kernel (relgnn_gemm_tn_stream_f32: 59 us at 256 x 256 against 171), larger ones to the limb TN kernel or to one
strided-batched library call over S chunks of the rows whose partial products are summed in order.  The bias gradient is a two-stage
HIP column sum.

Where things live:
  dense.py            routing (_route, lib_gemm, matmul_tn_splitk, grouped_*_gemm, mm_into, dense_multi), _DenseFn / _DenseMultiFn,
                      dense / dense_act / dense_relu
  dense_kernels.py    one wrapper per entry point: operand predicates, scratch, argument lists
  activation_tags.py  the tensor tags by which a consumer folds an activation's gradient into its input-gradient product
  weight_images.py    the cache of the weights' limb images
Every name of the three is reachable as dense.X.
"""
import torch

# config.settings.gemm (RELGNN_GEMM) selects the family; the whole decision is _route() below:
#   limb  (default) tall operands through csrc/limb_gemm.hip wherever limb_shape_ok() holds.  Against float64 at [36 k, 768] x [768, 256]:
#         4.0e-6 (exact-fp32 library GEMM: 5.3e-6); the C2 layer against the oracle: 3.8e-6 abs (library: 6.2e-6,
#         profiles/r03_parity_margin*.json).  Weight gradients with J % 32 == 0, C % 256 == 0 and more than 256 x 256 outputs on the limb
#         TN kernel.  Everything else falls through to `lib`.
#   lib   exact fp32 through relgnn_blaslt_gemm_f32, small weight gradients through relgnn_gemm_tn_stream_f32
#   panel forward / input-gradient products through the exact-fp32 row-panel MFMA kernel (csrc/panel_gemm.hip) wherever its shape
#         constraints hold (N % 64 == 0, K % 4 == 0); the weight gradients keep their `lib` routes
#   torch library GEMMs through torch.mm (a hipBLASLt solution lookup per call: ~70 us of host time for every node count not
#         seen before, i.e. for every batch of a shuffled epoch)
# config.settings.limb (RELGNN_LIMB) = triple (default): the exact split everywhere.  pair: where the producer of the left operand
# supplies per-row magnitudes (the gather in front of the aggregate-first layer's products), the product is evaluated from TWO fp16
# limbs per value behind exact power-of-two scales — three MFMA products instead of six (csrc/limb_gemm.hip, NL = 2; its weight
# gradient: one scale per column of each operand).  Per product its operands carry 22 instead of 24 significant bits; measured against
# float64 on the C2 shapes neither arithmetic is systematically closer end to end (profiles/r04_*).
from . import _lib
from ._lib import ACT_LINEAR, ACT_RELU
from .activations import activation_of_id, apply_activation
from .activation_tags import (_FROM_OUTPUT_ACTS, _IDEMPOTENT_ACTS, fusable_activation_of, is_premasked, mark_activation_output,
                              mark_premasked, mark_zero_padded, vouch_sole_consumer, zero_padded_operand)
from .config import settings as _cfg
from .dense_kernels import (_LIMB_MAX_K, _LIMB_MIN_ROWS, _LIMB_WS, _WORKSPACE, _ZEROS, Limbs, _limb_pc_ok, _limb_ws, _sel_with_image,
                            _workspace, _zeros, absmax, act_bwd_from_output, bias_ok, col_absmax, column_sum, limb_dense,
                            limb_dense_sel, limb_gemm, limb_gemm_tn, limb_gemm_tn_tiles, limb_gemm_weight, limb_gemm_xf32,
                            limb_shape_ok, limb_split, limb_tn_supported, limb_tn_tiles_supported, panel_gemm, panel_gemm_supported,
                            premask_ok, rows_aligned, rows_dense, sum_slabs_tail, tn_stream_blocks, tn_stream_blocks_ok,
                            tn_stream_gemm, tn_stream_group, tn_stream_group_ok, tn_stream_into)
# the limb images of the weights (weight_images.py: one cache, one validity rule), under the names the products below and the
# callers of this module use — weights_changed() is the documented contract: tf_gnn_samples_amd.dense.weights_changed()
from .weight_images import (GEMM_NN, GEMM_NT, GEMM_TN, WEIGHT_NN, WEIGHT_NT, _PerStream, _weight_image_items, _weight_image_shape,
                            _weight_matrices, capture_image_cache, clear as _clear_weight_images, sel_image, sel_weights_cacheable,
                            weight_image, weight_image_ok, weight_limbs, weights_changed)
from .weight_grad_stream import fork

_WARNED_UNSUPPORTED = False


def clear_caches() -> None:
    """Drop every per-stream scratch buffer and every cached limb image of a weight (dense.weight_image re-splits on the next
    request).  For callers that retire streams or devices; never needed for correctness."""
    _LIMB_WS.clear()
    _WORKSPACE.clear()
    _clear_weight_images()
    _ZEROS.clear()


# ---- which kernel a forward / input-gradient product runs on ------------------------------------------------------------------------
# The routes, in the order _route() first asks for them (R_PANELS twice: with any activation of the path in front of R_SCRATCH, with
# ReLU at most behind it); "epilogue": what the launch itself applies besides the bias.
#   route          launched by                                       entry point                                   epilogue
#   R_PADDED       limb_gemm_weight over the zero-padded K           relgnn_limb_gemm_xf32 / _dact / _pc           act, premask
#   R_IMAGE        limb_gemm_weight (256 columns, cached image)      relgnn_limb_gemm_xf32 / _dact / _pc (wave     act, premask
#                                                                    roles: _limb_pc_ok, config limb_pc)
#   R_PANELS       limb_dense_sel (128-column panels)                relgnn_limb_gemm_sel_xf32 on sel_image(b), or  act
#                                                                    relgnn_limb_dense_sel_f32 on scratch (not a
#                                                                    weight, or weight_limb_cache = 0)
#   R_SCRATCH      limb_dense (256 columns, b split into scratch)    relgnn_limb_dense_f32                         ReLU
#   R_CUT          limb_dense_sel, last panel cut at N               relgnn_limb_dense_sel_f32                     ReLU
#   R_PANEL        panel_gemm (config gemm = panel)                  relgnn_panel_gemm_f32                         ReLU
#   R_LIBRARY      _library_gemm                                     relgnn_blaslt_gemm_f32                        ReLU
#   R_TORCH        _torch_gemm                                       —                                             ReLU
# tests/golden/dense_routes.json holds the table case by case (tests/test_gpu_dense_routes.py).
R_PADDED, R_IMAGE, R_PANELS, R_SCRATCH, R_CUT, R_PANEL, R_LIBRARY, R_TORCH = ("padded", "image", "panels", "scratch", "cut", "panel",
                                                                              "library", "torch")
_TORCH_ACT_ = {1: torch.tanh_, 2: torch.relu_, 3: lambda t: torch.nn.functional.leaky_relu_(t, 0.2), 4: torch.nn.functional.elu_,
               5: torch.selu_}


def _limb_columns(layout: int, a: torch.Tensor, b: torch.Tensor, bias) -> int:
    """The widest column chunk of the limb kernels that a @ b (NN) / a @ b^T (NT) fits: 256, 128, or 0 — not a limb product."""
    if not (rows_aligned(a) and rows_aligned(b) and bias_ok(bias, aligned=True)):
        return 0
    N, Kb = (b.shape[1], b.shape[0]) if layout == GEMM_NN else (b.shape[0], b.shape[1])
    rows, K = a.shape
    if Kb != K:
        return 0
    return 256 if limb_shape_ok(rows, N, K, 256) else 128 if limb_shape_ok(rows, N, K, 128) else 0


def _padded_ok(a: torch.Tensor, b: torch.Tensor, bias) -> bool:
    """a [M, k] is tagged as the first k columns of zero-padded rows (mark_zero_padded) and a @ b^T, b [N, k] a weight, may reduce over
    the padded length — for the 121-label PPI head one limb launch with the ReLU' of the layer below in its epilogue instead of a
    library product (K = 121) and a pass over [V, 256]."""
    ap = zero_padded_operand(a)
    return (ap is not None and rows_aligned(ap) and b.dim() == 2 and b.shape[1] == a.shape[1] and ap.shape[1] == (a.shape[1] + 15) // 16 * 16
            and limb_shape_ok(ap.shape[0], b.shape[0], ap.shape[1]) and weight_image_ok([b], WEIGHT_NT) and bias_ok(bias, aligned=True))


def _cut_ok(a: torch.Tensor, b: torch.Tensor, bias) -> bool:
    """a @ b (+ bias) with b [K, N], N % 128 >= 96 (the 121 labels of the PPI head): the 128-column panels with the last one cut at N
    (library pick for [36 k, 256] @ [256, 121]: 59-65 us)."""
    return (_cfg.limb_cut == "1" and rows_aligned(a) and b.is_cuda and b.dtype == torch.float32 and b.dim() == 2 and b.is_contiguous()
            and b.data_ptr() % 16 == 0 and b.shape[0] == a.shape[1] and b.shape[1] % 128 >= 96
            and limb_shape_ok(a.shape[0], 128, a.shape[1], 128) and bias_ok(bias))       # (N: whole panels and a cut one — the rule's
                                                                                         #  own column question is answered above)


def _route(layout: int, a, b, bias, act: int, weight: bool, premask, out, accumulate: bool):
    """(route, late_act, late_premask) of one product of lib_gemm; launches nothing.  late_act: the activation id the route cannot
    carry in its epilogue (0: none left), late_premask: the premask it cannot carry (None: none left) — lib_gemm applies them as
    passes behind the product.  The order of the questions is the specification."""
    fused = premask is not None or act not in (ACT_LINEAR, ACT_RELU)
    fresh = out is None and not accumulate
    if fused and not fresh:
        raise ValueError("lib_gemm: out= / accumulate= cannot be combined with premask= or an activation other than ReLU")
    limb = _cfg.limb_gemm and layout != GEMM_TN and fresh
    if (limb and layout == GEMM_NT and weight and a.is_cuda and _padded_ok(a, b, bias)
            and (premask is None or premask_ok(premask[1], a.shape[0], b.shape[0]))):
        return R_PADDED, 0, None
    if premask is not None:
        shape = (a.shape[0], b.shape[1] if layout == GEMM_NN else b.shape[0])
        if not premask_ok(premask[1], *shape):
            raise ValueError("lib_gemm: premask operand must be a float32 device [%d, %d] matrix with 16-byte aligned rows" % shape)
    columns = _limb_columns(layout, a, b, bias) if limb else 0
    if columns == 256 and weight:
        # (weight_image_ok(b) needs no asking: _limb_columns saw b as a single matrix with aligned dense rows, which is more)
        return R_IMAGE, 0, None
    if columns and premask is None and act != ACT_RELU and act in _TORCH_ACT_:
        # the D = 128 models' Dense layers (C3, C5: tanh between GNN layers), and a 256-column product against something that is
        # no weight: the 128-column panel kernels take any activation of the path in their epilogue (act_rt)
        return R_PANELS, 0, None
    late = (0 if act in (ACT_LINEAR, ACT_RELU) else act), premask      # every route from here on carries ReLU at most
    if columns == 256:
        return (R_SCRATCH,) + late
    if columns == 128:                                                 # the D = 128 models: 128 x 128 panels, two workgroups per CU
        return (R_PANELS,) + late
    if limb and layout == GEMM_NN and _cut_ok(a, b, bias):
        return (R_CUT,) + late
    if _cfg.gemm == "panel" and layout != GEMM_TN and fresh and panel_gemm_supported(layout, a, b) and bias_ok(bias, aligned=True):
        return (R_PANEL,) + late
    if _cfg.gemm != "torch" and rows_dense(a) and rows_dense(b) and bias_ok(bias):
        return (R_LIBRARY,) + late
    return (R_TORCH,) + late


def lib_gemm(layout: int, a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor = None, out: torch.Tensor = None,
             accumulate: bool = False, relu: bool = False, weight: bool = False, act: int = None, premask=None) -> torch.Tensor:
    """NN act(a @ b + bias) | NT a @ b^T | TN a^T @ b on the route _route() names, then the passes that route could not carry.
    weight=True: b is a parameter (or a view of one) — the limb routes keep its limb image across the step (weight_images.py).
    act: an activation id for the epilogue (overrides relu).
    premask = (act id, y): the result times act'(y), y [M, N] the OUTPUT of that activation (an input-gradient product meeting the
    activation gradient of the layer below).
    out= / accumulate=: into (onto) an existing matrix; the library and torch routes only, and not together with premask or an
    activation other than ReLU (ValueError)."""
    if act is None:
        act = ACT_RELU if relu else ACT_LINEAR
    route, late_act, late_premask = _route(layout, a, b, bias, act, weight, premask, out, accumulate)
    epilogue = ACT_LINEAR if late_act else act
    dact, dy = premask if premask is not None and late_premask is None else (0, None)
    if route == R_PADDED:
        res = limb_gemm_weight(zero_padded_operand(a), b, WEIGHT_NT, bias, epilogue, dact=dact, dy=dy)
    elif route == R_IMAGE:
        res = limb_gemm_weight(a, b, WEIGHT_NN if layout == GEMM_NN else WEIGHT_NT, bias, epilogue, dact=dact, dy=dy)
    elif route == R_PANELS:
        res = limb_dense_sel(layout, a, b, bias, epilogue, image=sel_image(b, layout) if weight else None)
    elif route == R_SCRATCH:
        res = limb_dense(layout, a, b, bias, epilogue)
    elif route == R_CUT:
        res = limb_dense_sel(layout, a, b, bias, epilogue)
    elif route == R_PANEL:
        res = panel_gemm(layout, a, b, bias, epilogue)
    elif route == R_LIBRARY:
        res = _library_gemm(layout, a, b, bias, epilogue == ACT_RELU, out, accumulate)
    else:
        res = _torch_gemm(layout, a, b, bias, epilogue == ACT_RELU, out, accumulate)
    if late_act:
        fn = _TORCH_ACT_.get(late_act)
        if fn is None:
            raise ValueError("lib_gemm: no epilogue for activation id %d" % late_act)
        res = fn(res)
    if late_premask is not None:
        res = act_bwd_from_output(late_premask[0], late_premask[1], res, out=res)
    return res


def _torch_gemm(layout: int, a, b, bias, relu: bool, out, accumulate: bool) -> torch.Tensor:
    """Operands the C entry points do not take (not fp32 / not row-dense / CPU), and config gemm = torch."""
    if layout == GEMM_NN:
        res = torch.addmm(bias, a, b) if bias is not None else a @ b
    else:
        res = a @ b.t() if layout == GEMM_NT else a.t() @ b
    if relu:
        res = res.relu_()
    if out is None:
        return res
    return out.add_(res) if accumulate else out.copy_(res)


def _blaslt(layout: int, act: int, a, lda: int, b, ldb: int, bias, out, ldo: int, M: int, N: int, K: int, batch: int = 1,
            strides=(0, 0, 0), accumulate: bool = False) -> int:
    """relgnn_blaslt_gemm_f32 with this stream's workspace; returns the status."""
    ws = _workspace(a.device)
    return _lib.load_library().relgnn_blaslt_gemm_f32(
        layout, act, _lib.ptr(a, rows_strided=True), lda, _lib.ptr(b, rows_strided=True), ldb, _lib.ptr(bias),
        _lib.ptr(out, rows_strided=True), ldo, M, N, K, batch, *strides, 1 if accumulate else 0, _lib.ptr(ws), ws.numel(),
        _lib.current_stream())


def _library_gemm(layout: int, a, b, bias, relu: bool, out, accumulate: bool) -> torch.Tensor:
    """Plain library GEMM with a cached solution (relgnn_blaslt_gemm_f32)."""
    if layout == GEMM_NN:
        M, K, N = a.shape[0], a.shape[1], b.shape[1]
    elif layout == GEMM_NT:
        M, K, N = a.shape[0], a.shape[1], b.shape[0]
    else:
        K, M, N = a.shape[0], a.shape[1], b.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    code = _blaslt(layout, ACT_RELU if relu else ACT_LINEAR, a, a.stride(0), b, b.stride(0), bias, out, out.stride(0), M, N, K,
                   accumulate=accumulate)
    if code == _lib.EUNSUPPORTED:
        # the library has no solution for this problem through the direct interface (never seen on the shapes of the
        # path): same library through torch, said once — still the GPU, still fp32
        global _WARNED_UNSUPPORTED
        if not _WARNED_UNSUPPORTED:
            _WARNED_UNSUPPORTED = True
            import warnings
            warnings.warn("relgnn_blaslt_gemm_f32: no hipBLASLt solution for layout %d, M=%d N=%d K=%d; using torch.mm "
                          "for such shapes" % (layout, M, N, K))
        return _torch_gemm(layout, a, b, bias, relu, out, accumulate)
    _lib.check(code, "relgnn_blaslt_gemm_f32")
    return out


def _limb_group_ok(a: torch.Tensor, ws, kind: str) -> bool:
    if not (_cfg.limb_gemm and rows_aligned(a) and weight_image_ok(ws, kind)):
        return False
    n, k = _weight_image_shape(ws, kind)
    return a.shape[1] == k and limb_shape_ok(a.shape[0], n, k)


def grouped_nn_gemm(a: torch.Tensor, kernels, relu: bool = False, xmax: torch.Tensor = None, xgroups: int = 0) -> torch.Tensor:
    """(relu of) sum_l a[:, block l] @ kernels[l] for a [V, sum_l K_l], kernels[l] [K_l, N]: gnns/rgcn.py:96-98 summed over the
    edge types in one product (the aggregate-first layer's forward)."""
    kernels = list(kernels)
    if _limb_group_ok(a, kernels, WEIGHT_NN):
        return limb_gemm_weight(a, kernels, WEIGHT_NN, None, ACT_RELU if relu else ACT_LINEAR, xmax=xmax, xgroups=xgroups)
    return lib_gemm(GEMM_NN, a, torch.cat(kernels, dim=0) if len(kernels) > 1 else kernels[0], relu=relu)


def grouped_nt_gemm(g: torch.Tensor, kernels, xmax: torch.Tensor = None, xgroups: int = 0, premask=None) -> torch.Tensor:
    """sum_l g[:, block l] @ kernels[l]^T for g [V, sum_l K_l], kernels[l] [N, K_l]: the input gradient of grouped_nn_gemm's layer
    (dH = sum_l dT_l @ W_l^T).  premask = (act id, y): times act'(y), y [V, N] the layer's INPUT as the output of that activation
    (lib_gemm's premask)."""
    kernels = list(kernels)
    if _limb_group_ok(g, kernels, WEIGHT_NT) and (premask is None or premask_ok(premask[1], g.shape[0], kernels[0].shape[0])):
        dact, dy = premask if premask is not None else (0, None)
        return limb_gemm_weight(g, kernels, WEIGHT_NT, xmax=xmax, xgroups=xgroups, dact=dact, dy=dy)
    # (the stacked [sum K_l, N] right operand is W_l^T row blocks, 0.8 MB re-laid per call at C2)
    res = lib_gemm(GEMM_NN, g, torch.cat([k.t() for k in kernels], dim=0))
    return res if premask is None else act_bwd_from_output(premask[0], premask[1], res, out=res)


def mm_into(layout: int, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[:] = a @ b (GEMM_NN) | a @ b^T (GEMM_NT) into a preallocated row block: the limb route when the shapes allow
    (RELGNN_GEMM=limb), else the library through torch.mm.  For the per-edge-type row blocks of an edge MLP (ops.edge._BlockedLinear)."""
    if _cfg.limb_gemm and _limb_columns(layout, a, b, None) == 256 and rows_aligned(out):
        return limb_dense(layout, a, b, out=out)
    return torch.mm(a, b if layout == GEMM_NN else b.t(), out=out)


def enable_gemm_autotuning(max_tuning_ms_per_solution: int = 30, tune: bool = True) -> bool:
    """PyTorch TunableOp: for every GEMM shape the step uses, time the candidate rocBLAS / hipBLASLt solutions once
    (at first use) and keep the fastest.  Measured on MI355X, config C2: 2.72 -> 2.39 ms per training step (the fp32
    node-side GEMMs are ~half of the step).  The result table is written under the system temp directory, not into the
    working directory.  Returns False if this torch build has no TunableOp.  Call
    `enable_gemm_autotuning(tune=False)` after warm-up to freeze the choices."""
    import os
    import tempfile
    tun = getattr(torch.cuda, "tunable", None)
    if tun is None or not torch.cuda.is_available():
        return False
    try:
        tun.enable(True)
        tun.tuning_enable(bool(tune))
    except Exception:
        return False
    for fn, arg in (("set_filename", os.path.join(tempfile.gettempdir(), "relgnn_tunableop_%d.csv" % os.getpid())),
                    ("set_max_tuning_duration", int(max_tuning_ms_per_solution))):
        try:
            if tune:
                getattr(tun, fn)(arg)
        except Exception:
            pass
    return True


def _split_count(V: int, M: int, N: int) -> int:
    """Number of K-chunks: enough output tiles (~128x128) x chunks to fill 256 CUs, chunks >= 512 rows."""
    tiles = max(1, ((M + 127) // 128) * ((N + 127) // 128))
    want = max(1, 512 // tiles)
    return int(max(1, min(want, V // 512, 64)))

def matmul_tn_splitk(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a^T @ b for a [V, M], b [V, N] (both row-major), reduction over V split into S chunks."""
    V, M = a.shape
    N = b.shape[1]
    # small outputs (every Dense of the path except the stacked per-type transforms): the streaming kernel — measured at
    # V = 36 k: [256 x 256] 59 us vs 171 us for the library's strided-batched split-K, [256 x 121] 43 vs 114, [50 x 256]
    # 33 vs 57, [128 x 128] 30 vs 56; the library wins for [768 x 256] (131 vs 223) and for V ~ 1e6
    if _cfg.tn == "stream" and M * N <= 256 * 256 and 0 < V <= (1 << 18) and rows_dense(a) and rows_dense(b):
        return tn_stream_gemm(a, b)
    if _cfg.limb_gemm and limb_tn_supported(a, b):
        return limb_gemm_tn(a, b)
    S = _split_count(V, M, N)
    if S <= 1:
        return lib_gemm(GEMM_TN, a, b)
    if not (a.is_contiguous() and b.is_contiguous()):      # the chunked forms below view the operands as [S, c, .]
        a, b = a.contiguous(), b.contiguous()
    c = V // S
    head = c * S
    # (outputs narrower than one 64-wide tile — the [50, 256] gradient of the input projection — keep torch.bmm: hipBLASLt's
    # strided-batched pick for them measured 148 us against 52 us)
    if _cfg.gemm != "torch" and min(M, N) >= 64 and rows_dense(a) and rows_dense(b):
        # one strided-batched library call: chunk z = rows [z*c, (z+1)*c) of both operands; the partial products are summed in slab
        # order and the < S leftover rows (V = S * c + R) are multiplied in by the same pass
        parts = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
        _lib.check(_blaslt(GEMM_TN, ACT_LINEAR, a, M, b, N, None, parts, N, M, N, c, S, (c * M, c * N, M * N)), "relgnn_blaslt_gemm_f32")
        return sum_slabs_tail(parts, a, b, head)
    out = torch.bmm(a[:head].view(S, c, M).transpose(1, 2), b[:head].view(S, c, N)).sum(0)
    if head < V:
        out.addmm_(a[head:].t(), b[head:])       # the < c leftover rows, accumulated in place
    return out


def _leaf_params(kernel, bias):
    """(kernel, bias) when both are leaf parameters — their gradients go straight to the accumulator — else None: the gradient of a
    VIEW of a parameter (the GRU's recurrent_kernel[:, :2u]) is consumed by the view's backward on the main stream at once."""
    params = (kernel,) if bias is None else (kernel, bias)
    return params if all(p.is_leaf and p.requires_grad for p in params) else None


class _DenseFn(torch.autograd.Function):
    """act(x @ kernel (+ bias)) for act in {linear, tanh, relu, leaky_relu, elu, selu} — the activation in the product's epilogue where
    the route has one, differentiated from the saved OUTPUT — with a split-K weight gradient.
    x_act: the activation x itself is the output of, when the caller may fold its gradient into this function's input-gradient
    product (fusable_activation_of(x)): g_x then leaves already multiplied by x_act'(x) and tagged (mark_premasked)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, act: int, x_act: int):
        y = lib_gemm(GEMM_NN, x, kernel, bias, weight=True, act=act)
        ctx.save_for_backward(x, kernel, y if act else None)
        ctx.has_bias, ctx.act, ctx.x_act = bias is not None, act, x_act
        ctx.leaf_params = _leaf_params(kernel, bias)
        return y

    @staticmethod
    def backward(ctx, g):
        x, kernel, y = ctx.saved_tensors
        if ctx.act:
            # g * act'(y): nothing to do when the consumer of y already folded it into the product that made g
            if not is_premasked(g, y, ctx.act):
                g = act_bwd_from_output(ctx.act, y, g)
        if g.dim() != 2 or g.stride(1) != 1 or not g.is_cuda or (g.stride(0) < g.shape[1] and g.shape[0] != 1):
            g = g.contiguous()             # (a row-strided gradient, e.g. a column block of the GRU's gate gradients, is
        gx = None                          # read in place: every consumer below takes a leading dimension; an expanded one,
                                           # strides (0, 1), is materialised)
        def weight_side():
            gk = matmul_tn_splitk(x if (x.dim() == 2 and x.stride(1) == 1 and x.is_cuda) else x.contiguous(), g) \
                if ctx.needs_input_grad[1] else None
            gb = column_sum(g) if ctx.has_bias and ctx.needs_input_grad[2] else None
            return gk, gb

        aside = fork(weight_side, (x, g), ctx.leaf_params, want=ctx.needs_input_grad[0] and ctx.needs_input_grad[1],
                     join_in_backward=False, contributes=x.is_cuda)
        if ctx.needs_input_grad[0]:
            if ctx.x_act and premask_ok(x, g.shape[0], kernel.shape[0]):
                gx = mark_premasked(lib_gemm(GEMM_NT, g, kernel, weight=True, premask=(ctx.x_act, x)), x, ctx.x_act)
            else:
                gx = lib_gemm(GEMM_NT, g, kernel, weight=True)
        gk, gb = aside.join() if aside is not None else weight_side()
        return gx, gk, gb, None, None


class _DenseMultiFn(torch.autograd.Function):
    """x @ [k_0 | k_1 | ..] for L kernels [K, N] (the per-edge-type Dense kernels of a GGNN / FiLM layer applied to every node:
    gnns/ggnn.py:60-64,81) WITHOUT forming the column-concatenated [K, L*N] operand: the limb images of the kernels, one behind the
    other, ARE the image of the concatenation (row blocks of 32 output columns are contiguous), and they come from the step's cache.
    Round 6: per layer one torch.cat, its five slice copies in the backward and three split launches less."""

    @staticmethod
    def forward(ctx, x, *kernels):
        y = limb_dense_sel(GEMM_NN, x, list(kernels), image=sel_image(kernels, GEMM_NN), as_one=True)
        ctx.save_for_backward(x, *kernels)
        ctx.leaf_params = tuple(kernels) if all(k.is_leaf for k in kernels) else None
        return y

    @staticmethod
    def backward(ctx, g):
        x, *kernels = ctx.saved_tensors
        L, (K, N) = len(kernels), kernels[0].shape
        g = g.contiguous()
        gx = gks = None

        def weight_side():
            # dk_l = x^T @ g[:, block l].  Each gradient has to be a dense [K, N] tensor of its own — autograd's accumulator keeps
            # such a tensor as it is, a column block of a [K, L*N] product it would clone (five copies, and on the main stream
            # while the side stream still writes it) — so the ONE product x^T @ g writes its column blocks as L matrices
            # (tn_stream_blocks: x read once, two launches instead of 2 L; C3: 50 us instead of 5 x 50 per layer)
            if all(ctx.needs_input_grad[1:]) and tn_stream_blocks_ok(x, g):
                return tuple(tn_stream_blocks(x, g, L).unbind(0))
            return tuple(matmul_tn_splitk(x, g[:, l * N:(l + 1) * N]) if ctx.needs_input_grad[1 + l] else None for l in range(L))

        aside = fork(weight_side, (x, g), ctx.leaf_params, want=ctx.needs_input_grad[0] and any(ctx.needs_input_grad[1:]),
                     join_in_backward=False, contributes=x.is_cuda)
        if ctx.needs_input_grad[0]:
            # gx = sum_l g[:, block l] @ k_l^T: the kernels side by side along the reduction (WEIGHT_NT image), 128 output columns
            im = weight_image(kernels, WEIGHT_NT)                        # B [K, L*N] = [k_0 | k_1 | ..] as stored
            gx = _sel_with_image(g, im, K, L * N)
        gks = aside.join() if aside is not None else (weight_side() if any(ctx.needs_input_grad[1:]) else (None,) * L)
        return (gx,) + tuple(gks)


def dense_multi(x: torch.Tensor, kernels) -> torch.Tensor:
    """x @ [k_0 | k_1 | ..] ([V, L*N]; row v viewed as [L, N] is (x_v k_0, .., x_v k_{L-1})) for L same-shaped kernels [K, N]."""
    kernels = list(kernels)
    K, N = kernels[0].shape
    # (the forward is x @ [K, L*N], the input gradient g [V, L*N] @ [L*N, K]: its reduction length L*N is the one the shape rule bounds)
    if (_cfg.limb_gemm and rows_aligned(x) and x.shape[1] == K and N % 128 == 0 and limb_shape_ok(x.shape[0], K, len(kernels) * N, 128)
            and all(k.is_contiguous() and k.data_ptr() % 16 == 0 for k in kernels) and sel_image(kernels, GEMM_NN) is not None):
        return _DenseMultiFn.apply(x, *kernels)
    return dense(x, torch.cat(kernels, dim=1))


def dense(x: torch.Tensor, kernel: torch.Tensor, bias: torch.Tensor = None, sole_reader: bool = False) -> torch.Tensor:
    """x @ kernel (+ bias) with a split-K weight gradient.  sole_reader: this call is the only reader of x (see the protocol in
    activation_tags.py; it only matters when x is a tagged activation output)."""
    return _DenseFn.apply(x, kernel, bias, 0, fusable_activation_of(x, sole_reader) if x.requires_grad else 0)


def dense_act(x: torch.Tensor, kernel: torch.Tensor, bias: torch.Tensor = None, act: int = 0,
              sole_consumer: bool = False, sole_reader: bool = False) -> torch.Tensor:
    """act(dense(x, kernel, bias)) as ONE product with the activation in its epilogue (activation ids of _lib; gelu and anything the
    epilogue does not take: the two-step route).  The result is tagged as an activation output (mark_activation_output) so that the
    function that consumes it may fold act' into its input-gradient product; sole_consumer: the caller vouches that only the function
    it hands the result to will read it; sole_reader: this call is the only reader of x (both: the protocol in activation_tags.py)."""
    if act == ACT_LINEAR:
        return dense(x, kernel, bias, sole_reader=sole_reader)
    if not (act in _FROM_OUTPUT_ACTS and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and _cfg.gemm != "torch"
            and (_cfg.act_fusion == "1" or act == ACT_RELU)):
        return apply_activation(activation_of_id(act), dense(x, kernel, bias, sole_reader=sole_reader))
    y = _DenseFn.apply(x, kernel, bias, act, fusable_activation_of(x, sole_reader) if x.requires_grad else 0)
    return mark_activation_output(y, act, sole_consumer)


def dense_relu(x: torch.Tensor, kernel: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    """relu(dense(x, kernel, bias)) as one GEMM with a ReLU epilogue (CUDA fp32 operands; anything else takes the two-step
    route)."""
    return dense_act(x, kernel, bias, ACT_RELU)

