"""The optimizer of the model driver: TF1's update rules behind per-variable tf.clip_by_norm, fused into multi-tensor HIP launches on
the GPU."""
import ctypes
import math
from typing import Dict, List

import numpy as np
import torch

from .. import _lib
from ..dense import weights_changed


class _DeferredRows:
    """The state of the row-deferred parameter (TFStyleOptimizer.defer_rows; include/relgnn_sparse_update.h): stamps int32 [F], the
    step each row is current to; step_sizes float32 [capacity], lr_t of steps base + 1 ... ; rowptr, what rows_touched() kept."""

    def __init__(self, index: int, param: torch.Tensor, capacity: int, t: int):
        self.index, self.capacity = index, capacity
        self.rows, self.width = int(param.shape[0]), int(param.shape[1])
        self.sink = None                   # compact_row_gradient(): the RowGradientSink
        self.stamps = torch.empty(self.rows, dtype=torch.int32, device=param.device)
        self.step_sizes = torch.zeros(capacity, dtype=torch.float32, device=param.device)
        self.reset(t)

    def reset(self, t: int) -> None:
        self.base = int(t)
        self.stamps.fill_(int(t))
        self.rowptr = None


class RowGradient:
    """One step's compact gradient of the row-deferred [F, n] parameter: values float32 [T, n] are its rows `words` (int32 [T],
    ascending); slot int32 [F + 1] maps a word to its row of `values`; every other row of the gradient is +0."""

    def __init__(self, words: torch.Tensor, slot: torch.Tensor, values: torch.Tensor, rows: int):
        self.words, self.slot, self.values, self.rows = words, slot, values, int(rows)

    def to_dense(self) -> torch.Tensor:
        """The [F, n] gradient (tests and debugging: the step itself never builds it)."""
        dense = torch.zeros((self.rows, self.values.shape[1]), dtype=self.values.dtype, device=self.values.device)
        dense[self.words.long()] = self.values
        return dense


class RowGradientSink:
    """Where ops.csr_rows_project's backward leaves the compact gradient of the row-deferred parameter (TFStyleOptimizer.
    compact_row_gradient owns it).  One deposit per step; clip_and_step() and zero_grad() empty it."""

    def __init__(self, rows: int, width: int):
        self.rows, self.width = int(rows), int(width)
        self.gradient = None

    def check(self, container) -> None:
        if self.gradient is not None:
            raise RuntimeError("row gradient sink: a second deposit in one step (the projection ran its backward twice; a compact "
                               "gradient is not accumulated)")
        if not getattr(container, "has_named_rows", False):
            raise RuntimeError("row gradient sink: the feature container carries no named rows (SparseRows.named_rows / "
                               "take_rows(named_rows=True) before the step)")

    def deposit(self, named, values: torch.Tensor) -> None:
        self.check_shape(named, values)
        self.gradient = RowGradient(named.words, named.slot, values, self.rows)

    def check_shape(self, named, values: torch.Tensor) -> None:
        if self.gradient is not None:
            raise RuntimeError("row gradient sink: a second deposit in one step")
        if int(named.slot.shape[0]) != self.rows + 1 or tuple(values.shape) != (named.count, self.width):
            raise RuntimeError("row gradient sink: a [%d, %d] gradient over %d words does not belong to the registered [%d, %d] "
                               "parameter" % (values.shape[0], values.shape[1], int(named.slot.shape[0]) - 1, self.rows, self.width))

    def clear(self) -> None:
        self.gradient = None


class TFStyleOptimizer:
    """compute_gradients -> per-variable tf.clip_by_norm -> apply_gradients
    (models/sparse_graph_model.py:227-260) with TF1 update rules [TF-internal]:
      Adam    : lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMA; var -= lr_t*m/(sqrt(v)+eps), eps=1e-8
      RMSProp : ms = d*ms+(1-d)*g^2; mom = momentum*mom + lr*g/sqrt(ms+eps); var -= mom, eps=1e-10, ms0=1
      SGD     : var -= lr*g
    """

    def __init__(self, params: List[torch.nn.Parameter], name: str, learning_rate: float, clamp_gradient_norm: float,
                 decay: float = 0.98, momentum: float = 0.85):
        self.params = [p for p in params if p.requires_grad]
        self.name = name.lower()
        if self.name not in ('sgd', 'rmsprop', 'adam'):
            raise Exception('Unknown optimizer "%s".' % name)
        self.lr, self.clip, self.decay, self.momentum = learning_rate, clamp_gradient_norm, decay, momentum
        self.t = 0
        if self.name == 'adam':
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]
        elif self.name == 'rmsprop':
            self.ms = [torch.ones_like(p) for p in self.params]
            self.mom = [torch.zeros_like(p) for p in self.params]
        self._deferred = None              # defer_rows(): the one row-deferred parameter's _DeferredRows

    # ---- a row-deferred parameter (include/relgnn_sparse_update.h) ----
    def defer_rows(self, param: torch.nn.Parameter, capacity: int = 1024) -> None:
        """Register ONE 2-D [F, n] parameter whose gradient is +0 outside the rows a step's batch names (the weight of the sparse
        input projection under sampled batches) as row-deferred.  Adam only.  The parameter keeps dense Adam's values bit for
        bit, but a step reads and writes only the named rows: rows_touched(rowptr_t) before the step's forward brings the rows
        the batch names up to date (the steps they missed, replayed with g = +0 and each step's own lr_t), clip_and_step() updates
        those rows alone.  BETWEEN STEPS THE PARAMETER TENSOR AND ITS TWO SLOTS HOLD STALE ROWS; flush_deferred() brings all of
        them up to date, and whoever reads the tensor outside a training step calls it first (tf_slot_weights / load_tf_slots do).
        capacity: the length of the table of step sizes = the number of steps any row may fall behind = the bound of any launch's
        replay loop; when the table is full the next step flushes first."""
        if self.name != 'adam':
            raise ValueError("defer_rows: a row-deferred update exists for Adam only (the optimizer is %r)" % self.name)
        if self._deferred is not None:
            raise ValueError("defer_rows: one parameter can be registered, and one already is")
        index = [i for i, p in enumerate(self.params) if p is param]
        if not index:
            raise ValueError("defer_rows: the parameter is not one this optimizer updates")
        if param.dim() != 2 or not param.is_contiguous() or param.dtype != torch.float32:
            raise ValueError("defer_rows: a contiguous two-dimensional float32 parameter is needed, got shape %r" % (tuple(param.shape),))
        n = int(param.shape[1])
        if n % 4 or not 4 <= n <= 1024:            # relgnn_rows_adam_supported, restated: asked before the library is loaded
            raise ValueError("defer_rows: rows of %d floats are outside what the row kernels take (a multiple of 4 in 4 .. 1024)" % n)
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("defer_rows: capacity must be a positive integer, got %r" % (capacity,))
        self._deferred = _DeferredRows(index[0], param, capacity, self.t)

    def compact_row_gradient(self) -> RowGradientSink:
        """On top of defer_rows(): the registered parameter's gradient arrives as the rows a step names only
        (include/relgnn_sparse_gradient.h).  Returns the sink to hand to ops.csr_rows_project(row_gradient_sink=...); its backward
        deposits (words, slot, values [T, n]) there and leaves the parameter's .grad None.  clip_and_step() then computes the
        parameter's norm over those rows with the bits relgnn_mt_l2norm gives the dense gradient, and updates the rows from them."""
        d = self._require_deferred()
        if d.sink is None:
            d.sink = RowGradientSink(d.rows, d.width)
        return d.sink

    @property
    def row_gradient_sink(self):
        """The sink of compact_row_gradient(), None without one."""
        return self._deferred.sink if self._deferred is not None else None

    def rows_touched(self, rowptr_t: torch.Tensor) -> None:
        """Before the forward of a training step: `rowptr_t` (int32 [F + 1], the row pointer of the batch's transposed structure)
        names the rows the step reads and updates.  Those that are behind catch up to self.t on the current stream; the tensor is
        kept for this step's clip_and_step()."""
        d = self._require_deferred()
        if rowptr_t.dtype != torch.int32 or rowptr_t.dim() != 1 or int(rowptr_t.shape[0]) != d.rows + 1:
            raise ValueError("rows_touched: an int32 row pointer of %d entries is needed" % (d.rows + 1))
        self._catch_up(rowptr_t)
        d.rowptr = rowptr_t

    def flush_deferred(self) -> None:
        """Every row of the registered parameter up to date with self.t (nothing is launched when none can be behind, nor
        without a registered parameter)."""
        d = self._deferred
        if d is None or d.base == self.t:
            return
        self._catch_up(None)
        d.base = self.t

    def pending_rows(self) -> int:
        """How many rows of the registered parameter are behind self.t (synchronises: tests and diagnostics)."""
        d = self._require_deferred()
        return int((d.stamps < self.t).sum())

    def _require_deferred(self):
        if self._deferred is None:
            raise RuntimeError("no parameter is registered as row-deferred (TFStyleOptimizer.defer_rows)")
        return self._deferred

    def _catch_up(self, rowptr_t) -> None:
        d = self._deferred
        if d.base == self.t:               # no step since the last flush: every stamp is self.t
            return
        i = d.index
        p = self.params[i]
        _lib.launch("relgnn_rows_adam_catch_up", _lib.ptr(rowptr_t), d.rows, _lib.ptr(p), _lib.ptr(self.m[i]), _lib.ptr(self.v[i]),
                    d.width, d.width, _lib.ptr(d.stamps), _lib.ptr(d.step_sizes), d.base, self.t, 0.9, 0.999, 1e-8)
        weights_changed()                  # (written through raw pointers, as the update itself)

    def _fused_update_available(self):
        return len(self.params) > 0 and all(p.is_cuda for p in self.params)

    @torch.no_grad()
    def clip_and_step(self, lr_scale: float = 1.0, device_step_count: bool = False):
        """clip_by_norm per variable + update.  On the GPU, for all three optimizers: two fused multi-tensor HIP launches per
        48 variables (relgnn_mt_l2norm, then relgnn_mt_adam_clip / relgnn_mt_rmsprop_clip / relgnn_mt_sgd_clip) instead of the
        ~15-30 elementwise kernels of clip_gradients() + step(), which stay as the un-fused restatement (and the CPU path).
        device_step_count=True (hipGraph capture): the caller keeps self.t in step.  Adam's step count and lr_t then live in
        device memory (relgnn_adam_step_size / relgnn_mt_adam_clip_devlr); RMSProp and SGD have no step-dependent factor:
        their lr = self.lr * lr_scale is a launch scalar, frozen into a captured graph.
        A row-deferred parameter (defer_rows) stays in the norm launch, ordered last, so its norm has the bits it always had; it
        leaves the Adam launch and takes relgnn_rows_adam_step over the rows rows_touched() named, with a pointer to its norm.
        With a compact gradient (compact_row_gradient) it leaves the norm launch too: relgnn_rows_l2norm gives the same float
        from the deposited rows, relgnn_rows_adam_step_compact updates from them, and the sink is emptied."""
        if not self._fused_update_available():
            if device_step_count:
                raise RuntimeError("a captured training step needs the fused update: every parameter on the GPU")
            if self._deferred is not None:
                raise RuntimeError("a row-deferred parameter (defer_rows) needs the fused update: every parameter on the GPU")
            self.clip_gradients()
            self.step(lr_scale)
            return
        lib = _lib.load_library()
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        deferred = self._deferred
        compact = deferred.sink.gradient if deferred is not None and deferred.sink is not None else None
        if not idx and compact is None:
            return
        if deferred is not None:
            if deferred.sink is not None and deferred.index in idx:
                raise RuntimeError("the row-deferred parameter has a dense gradient although its gradient is registered as compact "
                                   "(compact_row_gradient): the projection ran without the sink")
            if device_step_count:
                raise RuntimeError("a captured training step cannot update a row-deferred parameter (defer_rows): the rows a step "
                                   "names and the table of step sizes change with every step")
            if compact is None and deferred.index not in idx:
                raise RuntimeError("the row-deferred parameter has no gradient in a step that updates other variables: dense Adam "
                                   "would skip it, the replay would not")
            if self.t - deferred.base == deferred.capacity:       # the table of step sizes is full
                self.flush_deferred()
            if compact is None:
                # last of the last chunk: the dense launch takes the entries in front of it, norms[n - 1] is its own
                idx = [i for i in idx if i != deferred.index] + [deferred.index]
        b1, b2, eps = 0.9, 0.999, 1e-8
        lr = self.lr * lr_scale
        dev_state = None
        if device_step_count and self.name == 'adam':
            dev_state = self._device_state()
            _lib.launch("relgnn_adam_step_size", _lib.ptr(dev_state), lr, b1, b2)
        elif not device_step_count:
            self.t += 1
            lr_t = lr * (1 - b2 ** self.t) ** 0.5 / (1 - b1 ** self.t)
        for c0 in range(0, len(idx), _lib.MT_MAX):
            chunk = idx[c0:c0 + _lib.MT_MAX]
            n = len(chunk)
            grads = [self.params[i].grad if self.params[i].grad.is_contiguous() else self.params[i].grad.contiguous()
                     for i in chunk]
            arr = ctypes.c_void_p * n
            h_g = arr(*[g.data_ptr() for g in grads])
            h_p = arr(*[self.params[i].data_ptr() for i in chunk])
            h_n = (ctypes.c_int64 * n)(*[self.params[i].numel() for i in chunk])
            norms = torch.empty(n, dtype=torch.float32, device=self.params[chunk[0]].device)
            ws_bytes = lib.relgnn_mt_l2norm_workspace_bytes()
            ws = _lib.scratch(ws_bytes, norms.device)
            _lib.launch("relgnn_mt_l2norm", h_g, h_n, n, _lib.ptr(norms), _lib.ptr(ws), ws_bytes)
            h_s = [arr(*[t[i].data_ptr() for i in chunk]) for _, t in self._slots()]      # Adam: m, v; RMSProp: ms, mom; SGD: none
            d_norms, clip = _lib.ptr(norms), float(self.clip)
            if self.name == 'sgd':
                _lib.launch("relgnn_mt_sgd_clip", h_p, h_g, h_n, n, d_norms, clip, lr)
            elif self.name == 'rmsprop':
                _lib.launch("relgnn_mt_rmsprop_clip", h_p, h_g, *h_s, h_n, n, d_norms, clip, lr, float(self.decay), float(self.momentum),
                            1e-10)
            elif dev_state is not None:
                _lib.launch("relgnn_mt_adam_clip_devlr", h_p, h_g, *h_s, h_n, n, d_norms, clip, dev_state[1:].data_ptr(), b1, b2, eps)
            elif deferred is not None and chunk[-1] == deferred.index:
                if n > 1:
                    _lib.launch("relgnn_mt_adam_clip", h_p, h_g, *h_s, h_n, n - 1, d_norms, clip, lr_t, b1, b2, eps)
                i, d = deferred.index, deferred
                _lib.launch("relgnn_rows_adam_step", _lib.ptr(d.rowptr), d.rows, _lib.ptr(self.params[i]), grads[-1].data_ptr(), d.width,
                            _lib.ptr(self.m[i]), _lib.ptr(self.v[i]), d.width, d.width, _lib.ptr(d.stamps), _lib.ptr(d.step_sizes), d.base,
                            self.t, norms[n - 1:].data_ptr(), clip, lr_t, b1, b2, eps)
                d.rowptr = None            # (this step's; without rows_touched() before the next one every row is named)
            else:
                _lib.launch("relgnn_mt_adam_clip", h_p, h_g, *h_s, h_n, n, d_norms, clip, lr_t, b1, b2, eps)
        if compact is not None:
            self._compact_step(compact, float(self.clip), lr_t, b1, b2, eps)
        weights_changed()                  # (written through raw pointers: the tensors' version counters did not move)

    def _compact_step(self, gradient: RowGradient, clip: float, lr_t: float, b1: float, b2: float, eps: float) -> None:
        """The registered parameter's norm and update from its compact gradient (include/relgnn_sparse_gradient.h)."""
        lib, d = _lib.load_library(), self._deferred
        i, T = d.index, int(gradient.values.shape[0])
        values = gradient.values if gradient.values.is_contiguous() else gradient.values.contiguous()
        some = lambda t: _lib.ptr(t) if T else None
        norm = torch.empty(1, dtype=torch.float32, device=values.device)
        ws_bytes = lib.relgnn_rows_l2norm_workspace_bytes()
        ws = _lib.scratch(ws_bytes, values.device)
        _lib.launch("relgnn_rows_l2norm", some(gradient.words), T, some(values), d.width, d.width, d.rows, _lib.ptr(norm), _lib.ptr(ws),
                    ws_bytes)
        _lib.launch("relgnn_rows_adam_step_compact", some(gradient.words), T, d.rows, _lib.ptr(self.params[i]), some(values), d.width,
                    _lib.ptr(self.m[i]), _lib.ptr(self.v[i]), d.width, d.width, _lib.ptr(d.stamps), _lib.ptr(d.step_sizes), d.base,
                    self.t, _lib.ptr(norm), clip, lr_t, b1, b2, eps)
        d.sink.clear()
        d.rowptr = None

    def _device_state(self):
        """[steps taken, lr_t] in device memory, seeded from the host step count."""
        if getattr(self, "_dev_state", None) is None:
            self._dev_state = torch.tensor([float(self.t), 0.0], dtype=torch.float32, device=self.params[0].device)
        return self._dev_state

    def sync_device_step_count(self):
        """Call before switching to device-side counting (the host count may have advanced since the last time)."""
        if getattr(self, "_dev_state", None) is not None:
            self._dev_state[0] = float(self.t)

    @torch.no_grad()
    def clip_gradients(self):
        """tf.clip_by_norm per variable: g * clip / max(||g||, clip)."""
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            return
        norms = torch.stack(torch._foreach_norm(grads))
        scales = self.clip / torch.clamp(norms, min=self.clip)       # == 1 where ||g|| <= clip
        torch._foreach_mul_(grads, list(scales.unbind(0)))

    @torch.no_grad()
    def step(self, lr_scale: float = 1.0):
        ps = [p for p in self.params if p.grad is not None]
        gs = [p.grad for p in ps]
        if not ps:
            return
        lr = self.lr * lr_scale
        self.t += 1
        if self.name == 'sgd':
            torch._foreach_add_(ps, gs, alpha=-lr)
        elif self.name == 'adam':
            b1, b2, eps = 0.9, 0.999, 1e-8
            idx = [i for i, p in enumerate(self.params) if p.grad is not None]
            m = [self.m[i] for i in idx]
            v = [self.v[i] for i in idx]
            torch._foreach_mul_(m, b1)
            torch._foreach_add_(m, gs, alpha=1 - b1)
            torch._foreach_mul_(v, b2)
            torch._foreach_addcmul_(v, gs, gs, value=1 - b2)
            lr_t = lr * (1 - b2 ** self.t) ** 0.5 / (1 - b1 ** self.t)
            denom = torch._foreach_sqrt(v)
            torch._foreach_add_(denom, eps)
            torch._foreach_addcdiv_(ps, m, denom, value=-lr_t)
        else:
            eps = 1e-10
            idx = [i for i, p in enumerate(self.params) if p.grad is not None]
            ms = [self.ms[i] for i in idx]
            mom = [self.mom[i] for i in idx]
            torch._foreach_mul_(ms, self.decay)
            torch._foreach_addcmul_(ms, gs, gs, value=1 - self.decay)
            denom = torch._foreach_add(ms, eps)
            torch._foreach_sqrt_(denom)
            torch._foreach_mul_(mom, self.momentum)
            torch._foreach_addcdiv_(mom, gs, denom, value=lr)
            torch._foreach_sub_(ps, mom)

    def zero_grad(self):
        for p in self.params:
            p.grad = None
        if self.row_gradient_sink is not None:
            self.row_gradient_sink.clear()

    # ---- optimizer state under TF's GLOBAL_VARIABLES names (the reference pickles those too, :91-107) ----
    def _slots(self):
        """(TF slot suffix, tensors) per optimizer [TF-internal slot names: Adam -> '<var>/Adam', '<var>/Adam_1';
        RMSProp -> '<var>/RMSProp' (mean square), '<var>/RMSProp_1' (momentum)]."""
        if self.name == 'adam':
            return [("Adam", self.m), ("Adam_1", self.v)]
        if self.name == 'rmsprop':
            return [("RMSProp", self.ms), ("RMSProp_1", self.mom)]
        return []

    def tf_slot_weights(self, names: List[str]) -> Dict[str, np.ndarray]:
        assert len(names) == len(self.params)
        self.flush_deferred()
        out = {}
        for suffix, tensors in self._slots():
            for n, t in zip(names, tensors):
                out["%s/%s:0" % (n, suffix)] = t.detach().cpu().numpy().copy()
        if self.name == 'adam':      # TF 1.13 keeps beta^(t+1) in two non-trainable scalars
            out["beta1_power:0"] = np.float32(0.9 ** (self.t + 1))
            out["beta2_power:0"] = np.float32(0.999 ** (self.t + 1))
        return out

    @torch.no_grad()
    def load_tf_slots(self, weights, names: List[str]) -> set:
        """Restore the slots a reference pickle carries; returns the consumed keys.  The step count is recovered from
        beta1_power (= 0.9^(t+1))."""
        used = set()
        self.flush_deferred()              # (a caller that overwrites the parameters too flushes before IT does: load_weights)
        for suffix, tensors in self._slots():
            for n, t in zip(names, tensors):
                key = "%s/%s:0" % (n, suffix)
                if key in weights:
                    t.copy_(torch.as_tensor(np.asarray(weights[key]), dtype=torch.float32))
                    used.add(key)
        if self.name == 'adam' and "beta1_power:0" in weights:
            self.t = self._steps_from_beta_powers(weights.get("beta1_power:0"), weights.get("beta2_power:0"))
            used.update(k for k in ("beta1_power:0", "beta2_power:0") if k in weights)
        if self._deferred is not None:     # what was loaded is current to the restored step count, every row of it
            self._deferred.reset(self.t)
        return used

    @staticmethod
    def _steps_from_beta_powers(beta1_power, beta2_power) -> int:
        """Step count t from TF's float32 scalars beta1_power = 0.9^(t+1), beta2_power = 0.999^(t+1).  0.9^(t+1) leaves the
        normal float32 range after ~830 steps and is exactly 0.0 after ~985, so it identifies t only for short runs; past
        that 0.999^(t+1) does (normal up to ~8.7e4 steps); when both have underflowed every bias correction is 1 to fp32
        precision and any large t reproduces the update rule."""
        tiny = float(np.finfo(np.float32).tiny)
        for power, beta in ((beta1_power, 0.9), (beta2_power, 0.999)):
            if power is None:
                continue
            p = float(np.asarray(power).reshape(-1)[0])
            if math.isfinite(p) and tiny <= p < 1.0:
                return max(0, int(round(math.log(p) / math.log(beta))) - 1)
            if p >= 1.0:
                return 0
        return 10 ** 6
