"""The optimizer of the model driver: TF1's update rules behind per-variable tf.clip_by_norm, fused into multi-tensor HIP launches on
the GPU."""
import ctypes
import math
from typing import Dict, List

import numpy as np
import torch

from .. import _lib
from ..dense import weights_changed


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

    def _fused_update_available(self):
        return len(self.params) > 0 and all(p.is_cuda for p in self.params)

    @torch.no_grad()
    def clip_and_step(self, lr_scale: float = 1.0, device_step_count: bool = False):
        """clip_by_norm per variable + update.  On the GPU, for all three optimizers: two fused multi-tensor HIP launches per
        48 variables (relgnn_mt_l2norm, then relgnn_mt_adam_clip / relgnn_mt_rmsprop_clip / relgnn_mt_sgd_clip) instead of the
        ~15-30 elementwise kernels of clip_gradients() + step(), which stay as the un-fused restatement (and the CPU path).
        device_step_count=True (hipGraph capture): the caller keeps self.t in step.  Adam's step count and lr_t then live in
        device memory (relgnn_adam_step_size / relgnn_mt_adam_clip_devlr); RMSProp and SGD have no step-dependent factor:
        their lr = self.lr * lr_scale is a launch scalar, frozen into a captured graph."""
        if not self._fused_update_available():
            if device_step_count:
                raise RuntimeError("a captured training step needs the fused update: every parameter on the GPU")
            self.clip_gradients()
            self.step(lr_scale)
            return
        lib = _lib.load_library()
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not idx:
            return
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
            else:
                _lib.launch("relgnn_mt_adam_clip", h_p, h_g, *h_s, h_n, n, d_norms, clip, lr_t, b1, b2, eps)
        weights_changed()                  # (written through raw pointers: the tensors' version counters did not move)

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
        for suffix, tensors in self._slots():
            for n, t in zip(names, tensors):
                key = "%s/%s:0" % (n, suffix)
                if key in weights:
                    t.copy_(torch.as_tensor(np.asarray(weights[key]), dtype=torch.float32))
                    used.add(key)
        if self.name == 'adam' and "beta1_power:0" in weights:
            self.t = self._steps_from_beta_powers(weights.get("beta1_power:0"), weights.get("beta2_power:0"))
            used.update(k for k in ("beta1_power:0", "beta2_power:0") if k in weights)
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
