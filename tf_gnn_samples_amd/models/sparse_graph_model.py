"""Model driver mirror (models/sparse_graph_model.py of the reference).

Hot-path scope: the per-layer loop of __build_graph_propagation_model
(:162-202) and the abstract hook _apply_gnn_layer (:204-225), same names and argument meaning.
The training-step plumbing around it (optimizer with per-variable clip_by_norm :227-260, epoch
loop with throughput counters :263-311) is restated minimally so that the reference's own
"edges/sec" number (README.md:34-35) can be measured end to end.

TF1 builds a static graph once and feeds numpy batches through sess.run; here the variables
live in a VariableStore under the reference's TF names, batches live in HBM (DeviceBatch), and a
step is eager PyTorch-ROCm around the librelgnn HIP kernels.
"""
import os
import pickle
import time
from abc import ABC, abstractmethod
from typing import Any, Dict, Iterable, List, Optional

import numpy as np
import torch

from ..dense import dense
from ..graph import as_rel_graph, check_pending_graph_errors
from ..tasks import DataFold, DeviceBatch, Sparse_Graph_Task
from ..utils import apply_activation, get_activation, layer_norm, layer_norm_scope
from ..variables import VariableStore


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
        import ctypes
        from .. import _lib
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
        from ..dense import weights_changed
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
        import math
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


class MetricsReadback:
    """The metric scalars of ONE step on their way to the host: packed into one device vector and copied into pinned
    memory by an asynchronous D2H enqueued right behind the step's own kernels.  get() waits for THAT copy only.

    float(tensor) / .item() is a stream-ordered copy on the current stream: called one step late it still waits for
    everything enqueued since — the whole NEXT step — and the GPU then idles until the host has come back and enqueued
    new work (measured: a ~0.2 ms bubble per 2.9 ms C2 step).  The reference has the same round trip once per
    sess.run (models/sparse_graph_model.py:293)."""
    _ring: Dict[Any, list] = {}

    def __init__(self, metrics: Dict[str, Any]):
        self._host_values = {k: v for k, v in metrics.items() if not (torch.is_tensor(v) and v.is_cuda)}
        dev = [(k, v.detach()) for k, v in metrics.items() if torch.is_tensor(v) and v.is_cuda]
        self._names = [k for k, _ in dev]
        self._event = self._slot = None
        self._status_at = None
        if dev:
            device = dev[0][1].device
            # one small kernel when the metrics share a dtype (the usual case: fp32 scalars), converted only if they differ
            dtype = dev[0][1].dtype if all(v.dtype == dev[0][1].dtype for _, v in dev) else torch.float64
            parts = [v.reshape(()) if v.dtype == dtype else v.reshape(()).to(dtype) for _, v in dev]
            # The hand-over status word of the device (ops.handover_word: a wave-role product kernel that gave up on an LDS
            # hand-over has written wrong numbers and says so there) rides in the same copy: its int32 bits as one more fp32
            # entry of the packed vector (a view, no launch of its own); get() raises when it is not zero.
            from .. import ops as _ops
            word = _ops._HANDOVER_WORDS.get(device.index)
            if word is not None:
                if dtype == torch.float32:
                    parts.append(word[0].view(torch.float32))
                else:
                    parts.append(word[0].to(dtype))
                self._status_at = len(dev)
            packed = torch.stack(parts)
            ring = MetricsReadback._ring.setdefault((device, len(parts), dtype), [])
            # a pinned slot is taken until its reader has consumed it (get()) or dropped it
            slot = next((b for b in ring if not b[1]), None)
            if slot is None:
                slot = [torch.empty(len(parts), dtype=dtype).pin_memory(), False]
                ring.append(slot)
            slot[1] = True
            slot[0].copy_(packed, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(device))
            self._slot = slot
            self._device = device

    def get(self) -> Dict[str, float]:
        out = {k: (float(v) if torch.is_tensor(v) else v) for k, v in self._host_values.items()}
        if self._event is not None:
            self._event.synchronize()
            host = self._slot[0]
            status = 0
            if self._status_at is not None:
                status = (int(host[self._status_at:self._status_at + 1].view(torch.int32)[0]) if host.dtype == torch.float32
                          else int(host[self._status_at]))
            out.update(zip(self._names, host.tolist()))
            self._event = None
            self._slot[1] = False
            self._values = {k: out[k] for k in self._names}
            if status:
                from .. import ops as _ops
                _ops._HANDOVER_WORDS[self._device.index][0].zero_()      # reported once; later steps start clean
                _ops.raise_on_handover(status)
        elif self._names:
            out.update(self._values)
        return out

    def __del__(self):
        slot = getattr(self, "_slot", None)
        if slot is not None and getattr(self, "_event", None) is not None:
            try:
                self._event.synchronize()          # the copy must not land in a slot somebody else has taken
            except Exception:
                pass
            slot[1] = False


class _PredictionArena:
    """The outputs of ONE batch's predictions as one packed byte arena: `views` are typed tensors over slices of it (16-byte
    aligned), which the prediction kernels write in place; send() enqueues the single copy to the host right behind them, with
    the device's hand-over status word (ops.handover_word) in the arena's last four bytes; fetch() waits for THAT copy only and
    returns NumPy arrays of the host's own (the pinned arena goes back into its turn)."""

    def __init__(self, layout: Dict[str, Any], device, pinned: list, turn: int):
        self._layout, self._offsets, used = layout, {}, 0
        for key, (shape, dtype) in layout.items():
            used = (used + 15) // 16 * 16
            self._offsets[key] = used
            used += int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        self._status_at = (used + 3) // 4 * 4
        self._nbytes = self._status_at + 4
        self._device, self._pinned, self._turn, self._event = device, pinned, turn, None
        self.buf = torch.empty(self._nbytes, dtype=torch.uint8, device=device)
        self.views = {key: self._view(self.buf, key) for key in layout}

    def _view(self, buf, key):
        shape, dtype = self._layout[key]
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        off = self._offsets[key]
        return buf[off:off + nbytes].view(dtype).view(shape)

    def send(self, outputs: Dict[str, torch.Tensor]):
        for key, view in self.views.items():
            t = outputs[key]
            if t.data_ptr() != view.data_ptr() or tuple(t.shape) != tuple(view.shape):      # (a hook that made a tensor of its own)
                view.copy_(t)
        if self._device.type != "cuda":
            self._host = self.buf
            return
        from .. import ops as _ops
        word = _ops._HANDOVER_WORDS.get(self._device.index)
        status = self.buf[self._status_at:].view(torch.int32)
        if word is not None:
            status.copy_(word[0:1])
        else:
            status.zero_()
        host = self._pinned[self._turn]
        if host is None or host.numel() < self._nbytes:
            host = self._pinned[self._turn] = torch.empty(self._nbytes, dtype=torch.uint8).pin_memory()
        self._host = host[:self._nbytes]
        self._host.copy_(self.buf, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(self._device))

    def fetch(self) -> Dict[str, np.ndarray]:
        if self._event is not None:
            self._event.synchronize()
            self._event = None
            status = int(self._host[self._status_at:].view(torch.int32)[0])
            if status:
                from .. import ops as _ops
                _ops._HANDOVER_WORDS[self._device.index][0].zero_()      # reported once, as a metric fetch does
                _ops.raise_on_handover(status)
        own = self._host.numpy().copy()                                  # one host copy out of the pinned arena; the pieces are its views
        out = {}
        for key, (shape, dtype) in self._layout.items():
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            off = self._offsets[key]
            out[key] = own[off:off + nbytes].view(torch.empty((), dtype=dtype).numpy().dtype).reshape(shape)
        self.buf = self.views = None
        return out


class CapturedTrainStep:
    """A training step recorded as a hipGraph on one fixed batch (Sparse_Graph_Model.capture_train_step), with any of the
    three optimizers.  Adam's step count is device state that every replay advances; the learning rate of an RMSProp or SGD
    step is a launch scalar of the recorded update."""

    def __init__(self, model, graph, metrics, batch):
        self.model, self.graph, self.metrics, self.batch = model, graph, metrics, batch
        self._expected_t = model.optimizer.t

    def replay(self) -> Dict[str, torch.Tensor]:
        """One more training step: a single graph launch.  The returned tensors are overwritten by the next replay.
        With Adam the graph reads the step count from device memory; if the host count moved since the last replay (an eager
        train_step(), load_weights()), the device copy is re-seeded first, so lr_t never comes from a stale count.  RMSProp and
        SGD keep no device state (the re-seeding is a no-op): their update does not depend on the step count.
        (lr_t of a replayed step is computed in float32 on the device, of an eager step in double on the host: the two
        agree to ~1e-7 relative, not bit for bit.)"""
        opt = self.model.optimizer
        if opt.t != self._expected_t:
            opt.sync_device_step_count()
        self.graph.replay()
        from ..dense import weights_changed
        weights_changed()                  # the replayed update rewrote the parameters: limb images kept by eager code are stale
        opt.t += 1
        self._expected_t = opt.t
        return self.metrics

    def handover_status(self) -> int:
        """The device's hand-over status word (ops.handover_status: synchronises).  A replay loop that reads the metric tensors
        itself instead of going through MetricsReadback checks this where it syncs anyway."""
        from .. import ops as _ops
        return _ops.handover_status(device=self.model.device)


class Sparse_Graph_Model(ABC):
    """Abstract superclass of all graph models (reference docstring: models/sparse_graph_model.py:16-20)."""

    @classmethod
    def default_params(cls):
        # models/sparse_graph_model.py:22-45
        return {
            'max_nodes_in_batch': 50000,
            'graph_num_layers': 8,
            'graph_num_timesteps_per_layer': 1,
            'graph_layer_input_dropout_keep_prob': 0.8,
            'graph_dense_between_every_num_gnn_layers': 1,
            'graph_model_activation_function': 'tanh',
            'graph_residual_connection_every_num_layers': 2,
            'graph_inter_layer_norm': False,
            'max_epochs': 10000,
            'patience': 25,
            'optimizer': 'Adam',
            'learning_rate': 0.001,
            'learning_rate_decay': 0.98,
            'lr_for_num_graphs_per_batch': None,
            'momentum': 0.85,
            'clamp_gradient_norm': 1.0,
            'random_seed': 0,
        }

    @staticmethod
    @abstractmethod
    def name(params: Dict[str, Any]) -> str:
        raise NotImplementedError()

    def __init__(self, params: Dict[str, Any], task: Sparse_Graph_Task, run_id: str = "run",
                 result_dir: str = ".", device: Optional[str] = None) -> None:
        self.params = params
        self.task = task
        self.run_id = run_id
        self.result_dir = result_dir
        self.device = torch.device(device if device is not None else "cuda")
        self._native_batchers = {}
        self.training = False
        # under a process group only rank 0 logs (the drivers form the group before they build the model; train(group=...) /
        # test(group=...) go by the rank within THEIR group)
        import torch.distributed as _dist
        self._log_rank = _dist.get_rank() if _dist.is_available() and _dist.is_initialized() else 0
        torch.manual_seed(params['random_seed'])
        np.random.seed(params['random_seed'])
        if self.device.type == "cuda":
            # the hand-over status block of this device (ops.handover_word): exists before any step can be captured into a hipGraph;
            # read back with every step's metrics (MetricsReadback) and by handover_status()
            from .. import ops as _ops
            self.handover_word = _ops.handover_word(self.device)
            # the state block of the fused layer-input dropout (ops.dropout): {seed, replica, step} in HBM, next to the hand-over
            # word for the same reason (a captured step needs a live pointer).  replica = the data-parallel rank (the drivers form
            # their process group before they build the model), so that ranks do not share masks
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self.dropout_state = _ops.dropout_state(self.device, params['random_seed'], rank, 0)
        self.variables = VariableStore(seed=params['random_seed'])
        self.__make_model()
        self.variables.to(self.device)
        self.__make_train_step()

    @property
    def log_file(self):
        return os.path.join(self.result_dir, "%s.log" % self.run_id)

    @property
    def best_model_file(self):
        return os.path.join(self.result_dir, "%s_best_model.pickle" % self.run_id)

    def log_line(self, msg):
        if self._log_rank != 0:
            return
        try:
            with open(self.log_file, 'a') as log_fh:
                log_fh.write(msg + '\n')
        except OSError:
            pass
        print(msg)

    # -------------------- Model Saving/Loading (reference pickle layout :91-126) --------------------
    def save_model(self, path: str) -> None:
        data_to_save = {
            "model_class": self.name(self.params),
            "task_class": self.task.name(),
            "model_params": self.params,
            "task_params": self.task.params,
            "task_metadata": self.task.get_metadata(),
            # every GLOBAL_VARIABLE of the TF graph: the model variables and the optimizer's slots
            "weights": dict(self.variables.tf_weights(), **self.optimizer.tf_slot_weights(self._trainable_names())),
        }
        with open(path, 'wb') as out_file:
            pickle.dump(data_to_save, out_file, pickle.HIGHEST_PROTOCOL)

    def _trainable_names(self) -> List[str]:
        return [n for n in self.variables.names() if self.variables[n].requires_grad]

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """:109-126: assign every variable the pickle names (model variables and optimizer slots), freshly initialise
        (= keep the initial value of) the ones it does not, report saved entries nothing consumed."""
        used = self.variables.load_tf_weights(weights, report_unused=False)
        used |= self.optimizer.load_tf_slots(weights, self._trainable_names())
        from ..dense import weights_changed
        weights_changed()                  # (copy_ moves the version counters too; said once more for limb images kept per step)
        for var_name in weights:
            if var_name not in used:
                print('Saved weights for %s not used by model.' % var_name)

    # -------------------- Model Construction --------------------
    @abstractmethod
    def _gnn_layer_variables(self, in_dim: int) -> Dict[str, Any]:
        """TF-relative variable specs of ONE gnn layer (what the reference's layer function would
        create under variable_scope('gnn_layer_%i'))."""
        raise NotImplementedError()

    def __make_model(self):
        p = self.params
        h_dim = p['hidden_size']
        vs = self.variables
        vs.create_all("", self.task.input_variables())            # :138 make_task_input_model runs before the propagation model
        if self.task.initial_node_feature_size != h_dim:          # :165-170, unnamed Keras Dense
            vs.create("graph_model/dense/kernel", (self.task.initial_node_feature_size, h_dim))
        self._inter_norm_name = []
        for layer_idx in range(p['graph_num_layers']):            # :176-200
            scope = "graph_model/gnn_layer_%i" % layer_idx
            specs = dict(self._gnn_layer_variables(h_dim))
            if p['graph_inter_layer_norm']:
                own = sum(1 for k in specs if k.startswith("LayerNorm") and k.endswith("/gamma"))
                ln = layer_norm_scope(own)          # TF uniquifies: the scope after the layer's own per-timestep norms
                specs[ln + "/beta"] = ((h_dim,), "zeros")
                specs[ln + "/gamma"] = ((h_dim,), "ones")
                self._inter_norm_name.append(ln)
            else:
                self._inter_norm_name.append(None)
            if layer_idx % p['graph_dense_between_every_num_gnn_layers'] == 0:
                specs["Dense/kernel"] = ((h_dim, h_dim), "glorot_uniform")
            vs.create_all(scope, specs)
        # The task names its own output variables (absolute TF scope): PPI's head is an UNNAMED Keras Dense, which TF
        # auto-names after the model's unnamed input projection ("dense" -> "dense_1", tasks/ppi_task.py:176-179);
        # QM9's heads live under variable_scope("out_layer_task%i") at the root (tasks/qm9_task.py:163-176).
        has_projection = self.task.initial_node_feature_size != h_dim
        self._task_scope = self.task.output_variable_scope(has_projection)
        vs.create_all(self._task_scope, self.task.output_variables(h_dim))
        self.log_line("Model has %i parameters." % vs.num_parameters())

    def compute_final_node_representations(self, initial_node_features: torch.Tensor,
                                           adjacency_lists, type_to_num_incoming_edges: torch.Tensor,
                                           dropout_keep_prob: float = 1.0) -> torch.Tensor:
        """__build_graph_propagation_model, models/sparse_graph_model.py:162-202.

        Dropout on the layer inputs (keep-prob < 1) is torch.nn.functional.dropout by default.  With
        config.settings.layer_dropout == "fused" a contiguous fp32 GPU input takes ops.dropout / ops.dropout_residual instead (one
        kernel per layer, the residual average included; no mask stored): the masks are Philox4x32-10 draws keyed by
        self.dropout_state = {random_seed, replica, step} with the layer index as the stream.  The step is bumped here, on the
        device, once per call that drops anything, so every pass (and every replay of a captured step) draws new masks; each pass
        works on its own 24-byte copy of the state, which its backward reads again.  The step is NOT written to checkpoints (the
        reference's pickle layout has no place for it): a restored model starts at step 0."""
        p = self.params
        activation_fn = get_activation(p['graph_model_activation_function'])
        w = self.variables.scope("graph_model")
        num_nodes = initial_node_features.shape[0]
        # bucketed once, shared by every layer; the index range check is read back at the next fetch
        graph = as_rel_graph(adjacency_lists, num_nodes, validate="deferred")
        from ..dense import dense_act, vouch_sole_consumer
        from ..ops import activation_id, dropout as fused_dropout, dropout_residual, dropout_tensor_ok, fused_dropout_on
        act_id = activation_id(p['graph_model_activation_function'])
        num_layers, res_every = p['graph_num_layers'], p['graph_residual_connection_every_num_layers']

        def only_the_next_layer_reads(next_layer_idx: int) -> bool:
            """Is the layer function of iteration `next_layer_idx` the only reader of the tensor handed to it?  (One of the two words
            that let a layer fold a non-idempotent activation gradient — tanh' of the Dense below it — into its input-gradient
            product: dense.py, "activation gradients folded into the product that feeds them"; the other one is the layer's own:
            that it reads its input once.)  At a residual step the tensor is read by the average instead (and kept for the next
            residual step); at layer 0 it is kept for the first residual step too."""
            if next_layer_idx >= num_layers or dropout_keep_prob < 1.0:
                return False
            if next_layer_idx % res_every == 0:
                return next_layer_idx == 0 and res_every >= num_layers
            return True

        if self.task.initial_node_feature_size != p['hidden_size']:
            cur_node_representations = dense_act(initial_node_features, w["dense/kernel"], None, act_id,
                                                 sole_consumer=only_the_next_layer_reads(0))
        else:
            cur_node_representations = initial_node_features
        last_residual_representations = None          # (the reference's zeros_like is overwritten at layer 0 before any use)
        pass_state = None
        if fused_dropout_on(dropout_keep_prob) and getattr(self, "dropout_state", None) is not None:
            with torch.no_grad():
                self.dropout_state[2].add_(1)                  # on the device, stream-ordered: every replay of a captured step advances it
                pass_state = self.dropout_state.clone()        # this pass's 24 bytes: read by its forward kernels and by its backward
        for layer_idx in range(p['graph_num_layers']):
            self._layer_weights = w.scope('gnn_layer_%i' % layer_idx)
            residual_step = layer_idx % res_every == 0
            if pass_state is not None and dropout_tensor_ok(cur_node_representations):
                # csrc/dropout.hip: one kernel for the whole layer-input stage; the layer index is the Philox stream
                if residual_step and layer_idx > 0:
                    last_residual_representations, cur_node_representations = dropout_residual(
                        cur_node_representations, last_residual_representations, dropout_keep_prob, pass_state, layer_idx)
                else:
                    cur_node_representations = fused_dropout(cur_node_representations, dropout_keep_prob, pass_state, layer_idx)
                    if residual_step:
                        last_residual_representations = cur_node_representations
            else:
                if dropout_keep_prob < 1.0:
                    cur_node_representations = torch.nn.functional.dropout(
                        cur_node_representations, p=1.0 - dropout_keep_prob, training=True)
                if residual_step:
                    t = cur_node_representations
                    if layer_idx > 0:
                        cur_node_representations = (cur_node_representations + last_residual_representations) / 2
                    last_residual_representations = t
            cur_node_representations = self._apply_gnn_layer(
                cur_node_representations, graph, type_to_num_incoming_edges, p['graph_num_timesteps_per_layer'])
            if p['graph_inter_layer_norm']:
                ln = self._inter_norm_name[layer_idx]
                cur_node_representations = layer_norm(cur_node_representations,
                                                      self._layer_weights[ln + "/gamma"], self._layer_weights[ln + "/beta"])
            if layer_idx % p['graph_dense_between_every_num_gnn_layers'] == 0:
                # (the layer's / the norm's output is referenced nowhere else: this Dense is its only reader)
                cur_node_representations = dense_act(vouch_sole_consumer(cur_node_representations, True),
                                                     self._layer_weights["Dense/kernel"], None, act_id,
                                                     sole_consumer=only_the_next_layer_reads(layer_idx + 1), sole_reader=True)
            else:
                vouch_sole_consumer(cur_node_representations, only_the_next_layer_reads(layer_idx + 1))
        return vouch_sole_consumer(cur_node_representations, False)     # (a task head may read it more than once)

    @abstractmethod
    def _apply_gnn_layer(self,
                         node_representations: torch.Tensor,
                         adjacency_lists: List[torch.Tensor],
                         type_to_num_incoming_edges: torch.Tensor,
                         num_timesteps: int) -> torch.Tensor:
        """Run a GNN layer on a graph (models/sparse_graph_model.py:204-225; same arguments).
        The current layer's variables are available as self._layer_weights."""
        raise Exception("Models have to implement _apply_gnn_layer!")

    def __make_train_step(self):
        p = self.params
        self.optimizer = TFStyleOptimizer(list(self.variables.parameters()), p['optimizer'], p['learning_rate'],
                                          p['clamp_gradient_norm'], decay=p['learning_rate_decay'],
                                          momentum=p['momentum'])

    # -------------------- Training Loop --------------------
    def _final_node_states(self, batch: DeviceBatch, training: bool) -> torch.Tensor:
        keep = self.params['graph_layer_input_dropout_keep_prob'] if training else 1.0
        batch.wait_ready()               # assembled on a side stream (tasks/resident.py)? wait on the GPU, not the host
        # a batch from the input pipeline may carry its bucketing, built on a side stream (tasks/batcher.py)
        graph = getattr(batch, "graph", None)
        return self.compute_final_node_representations(
            self.task.compute_initial_node_features(batch, self.variables.scope("")),
            graph if graph is not None else batch.adjacency_lists,
            batch.type_to_num_incoming_edges, keep)

    def forward_batch(self, batch: DeviceBatch, training: bool):
        final = self._final_node_states(batch, training)
        return self.task.compute_task_metrics(final, batch, self.variables.scope(self._task_scope))

    def capture_train_step(self, batch: DeviceBatch, warmup_steps: int = 3):
        """One full training step on a FIXED batch as a hipGraph (forward, backward, clip, update with Adam, RMSProp or SGD:
        ~150 launches replayed with one host call).  For workloads whose step is host-enqueue bound (C3: 153 k messages per
        batch) and whose batch shapes repeat.  Runs `warmup_steps` real steps first (allocator / plan caches), then captures;
        returns a CapturedTrainStep whose replay() performs exactly one more step and returns the (static) metric tensors.
        The learning rate of a captured RMSProp or SGD step is a launch scalar.  With lr_for_num_graphs_per_batch set it is
        learning_rate * num_graphs / lr_for_num_graphs_per_batch of THIS batch: constant for the fixed batch, so freezing it
        into the graph is correct (Adam's lr_t changes per step and is computed on the device instead)."""
        from ..graph import as_rel_graph as _as_graph
        if self.device.type != "cuda":
            raise RuntimeError("capture_train_step needs a model on the GPU (a hipGraph records GPU work)")
        batch.wait_ready()
        if getattr(batch, "graph", None) is None:           # the bucketing is part of the fixed batch, not of the step
            batch.graph = _as_graph(batch.adjacency_lists, batch.num_nodes, validate=True)
        opt = self.optimizer
        opt.sync_device_step_count()
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup_steps):
                self.train_step(batch, device_step_count=True)
                opt.t += 1
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad()
        from ..dense import capture_image_cache
        with capture_image_cache(), torch.cuda.graph(graph):      # (limb images of the weights: split once per captured step)
            metrics = self.train_step(batch, device_step_count=True)
        return CapturedTrainStep(self, graph, {k: v for k, v in metrics.items() if torch.is_tensor(v)}, batch)

    _backward_seed: Dict[Any, torch.Tensor] = {}

    def train_step(self, batch: DeviceBatch, grad_hook=None, device_step_count: bool = False,
                   pre_backward=None, lr_num_graphs: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """forward + backward + per-variable clip + optimizer update == one sess.run with train_step (:287-293).
        pre_backward(): called between the forward and the backward (a bucketed gradient all-reduce arms its hooks there);
        grad_hook(params): between the backward and the clipping (the data-parallel reduction);
        lr_num_graphs: the graph count lr_for_num_graphs_per_batch scales by (data-parallel: the step's global count)."""
        self.optimizer.zero_grad()
        metrics = self.forward_batch(batch, training=True)
        if pre_backward is not None:
            pre_backward()
        # one process drives one GPU: running the backward on the calling thread instead of the autograd engine's
        # device thread saves the hand-off per node (host enqueue 1.56 -> 1.29 ms per C2 step) and a busy CPU thread
        from .. import ops
        from contextlib import nullcontext
        # (the weight gradients of the aggregate-first layers run on a side stream; nothing reads them before the reduction / the
        #  optimizer, so their joins move behind the whole backward — not with a reducer that packs gradients from hooks DURING it)
        # (measured on the C2 step, alternated three times: 1.812 / 1.812 / 1.814 ms with the joins per layer, 1.804 / 1.806 / 1.806 deferred)
        defer = ops.deferred_weight_gradient_join() if pre_backward is None else nullcontext()
        with torch.autograd.set_multithreading_enabled(False), defer:
            loss = metrics['loss']
            one = self._backward_seed.get((loss.device, loss.dtype, loss.shape))
            if one is None:       # (loss.backward() would fill a fresh ones_like every step)
                one = self._backward_seed[(loss.device, loss.dtype, loss.shape)] = torch.ones_like(loss)
            loss.backward(gradient=one)
        ops.join_deferred()
        if grad_hook is not None:  # data-parallel gradient all-reduce goes here (before clipping)
            grad_hook(self.optimizer.params)
        lr_scale = self._lr_scale(batch.num_graphs if lr_num_graphs is None else lr_num_graphs)
        self.optimizer.clip_and_step(lr_scale, device_step_count=device_step_count)
        return metrics

    def _lr_scale(self, num_graphs: int) -> float:
        lr_n = self.params.get('lr_for_num_graphs_per_batch')
        return 1.0 if lr_n is None else float(num_graphs) / float(lr_n)

    def _batches(self, data, data_fold: DataFold):
        """Batches of one epoch.  On the GPU the data fold is flattened once and batches come from the C++ builder
        (tasks/batcher.py: packed in pinned memory on a background thread, one async upload each), the stand-in for
        the reference's ThreadedIterator (:272); `native_batching: false` keeps the numpy iterator."""
        native = self.params.get('native_batching', True) and torch.device(self.device).type == "cuda" \
            and hasattr(self.task, "make_graph_store")
        if not native:
            return self.task.make_minibatch_iterator(data, data_fold, self.params['max_nodes_in_batch'])
        return self.task.make_native_minibatch_iterator(self._native_pipeline(data), data_fold, self.params['max_nodes_in_batch'])

    def _native_pipeline(self, data):
        """The input pipeline of one data fold (ResidentDataset or NativeBatcher over its GraphStore), built once and kept."""
        from ..tasks.batcher import NativeBatcher
        key = (id(data), len(data))
        cached = self._native_batchers.get(key)
        if cached is not None and cached[0] is data:
            self._native_batchers[key] = self._native_batchers.pop(key)      # most recently used last
        if cached is None or cached[0] is not data:
            store = self.task.make_graph_store(data)
            pipeline = None
            # small enough folds simply live in HBM, bucketed once (tasks/resident.py); `resident_dataset: false`
            # keeps the host packer, `true` insists
            want = self.params.get('resident_dataset', 'auto')
            if want is True or (want == 'auto' and self._fold_fits_hbm(store)):
                from ..tasks.resident import ResidentDataset
                try:
                    pipeline = ResidentDataset(store, self.device)
                except ValueError:
                    if want is True:
                        raise
            if pipeline is None:
                pipeline = NativeBatcher(store, self.device)
            cached = (data, pipeline)
            self._native_batchers[key] = cached
            # train + validation folds (and one more) stay; anything older — e.g. the fresh list every test() call
            # passes — is dropped so that its resident copy of the fold and its pinned arenas are released
            while len(self._native_batchers) > 3:
                self._native_batchers.pop(next(iter(self._native_batchers)))
        return cached[1]

    @staticmethod
    def _fold_fits_hbm(store, budget_bytes: int = 32 << 30) -> bool:
        """Flat arrays + fold-level bucketing (~9 int32 per message) well inside the 288 GB of an MI355X."""
        nbytes = sum(a.nbytes for a in store.payload) + sum(a.nbytes for a in store.adj) + sum(a.nbytes for a in store.deg)
        messages = sum(int(o[-1]) for o in store.edge_off)
        nodes = int(store.node_off[-1])
        if nodes * max(store.num_edge_types, 1) >= 2 ** 31 - 1 or messages >= 2 ** 31 - 1:
            return False
        return nbytes + 40 * messages + 8 * nodes * max(store.num_edge_types, 1) < budget_bytes

    def _run_epoch(self, epoch_name: str, data: Iterable[Any], data_fold: DataFold, quiet: bool = False):
        """__run_epoch, :263-311: returns (avg loss, task metric results, graphs, graphs/s, nodes/s, edges/s)."""
        batch_iterator = self._batches(data, data_fold)
        start_time = time.time()
        processed_graphs = processed_nodes = processed_edges = 0
        epoch_loss = 0.0
        task_metric_results = []
        batch_iterator = iter(batch_iterator)
        upcoming = next(batch_iterator, None)
        state = {"graphs": 0, "nodes": 0, "edges": 0, "loss": 0.0, "step": 0}

        def fetch(pending):
            """Read one step's metrics back (the host sync of sess.run's fetch, :293)."""
            m, mb = pending
            m = m.get()
            check_pending_graph_errors()
            state["graphs"] += mb.num_graphs
            state["nodes"] += mb.num_nodes
            state["edges"] += mb.num_edges
            state["loss"] += m['loss'] * mb.num_graphs
            task_metric_results.append(m)
            if not quiet:
                print("Running %s, batch %i (has %i graphs). Loss so far: %.4f"
                      % (epoch_name, state["step"], mb.num_graphs, state["loss"] / state["graphs"]), end='\r')
            state["step"] += 1

        pending = None
        while upcoming is not None:
            mb = upcoming
            batch = mb if isinstance(mb, DeviceBatch) else DeviceBatch(mb, self.device)
            if data_fold == DataFold.TRAIN:
                m = self.train_step(batch)
            else:
                with torch.no_grad():
                    m = self.forward_batch(batch, training=False)
            # Pipeline: the step's metrics start their way to pinned host memory right behind the step (MetricsReadback);
            # ask for the next batch (its upload / assembly run on a side stream under this step's kernels), THEN read
            # the metrics of the PREVIOUS step: that wait is for the previous step's copy only, which the GPU has passed
            # long ago, so the device never idles behind a host round trip.  Every step's metrics are still fetched, one
            # step late.
            readback = MetricsReadback(m)          # (also drops the autograd graph: values are detached)
            upcoming = next(batch_iterator, None)
            if pending is not None:
                fetch(pending)
            pending = (readback, mb)
        if pending is not None:
            fetch(pending)
        processed_graphs, processed_nodes, processed_edges = state["graphs"], state["nodes"], state["edges"]
        epoch_loss = state["loss"]
        epoch_time = time.time() - start_time
        per_graph_loss = epoch_loss / max(processed_graphs, 1)
        return (per_graph_loss, task_metric_results, processed_graphs, processed_graphs / epoch_time,
                processed_nodes / epoch_time, processed_edges / epoch_time)

    def train(self, quiet: bool = False, max_epochs: Optional[int] = None, group=None):
        """:318-371 without TensorBoard: early stopping on the task's validation metric.
        group: a torch.distributed process group of W > 1 ranks (one process per GPU, the model built after init_distributed())
        trains data-parallel by graph (_DataParallel below); None or a group of one rank is the single-GPU loop."""
        total_time_start = time.time()
        dp = self._data_parallel(group)
        train_data = self.task._loaded_data[DataFold.TRAIN]
        valid_data = self.task._loaded_data[DataFold.VALIDATION]
        # The loaded folds are millions of long-lived Python objects: frozen for the duration of the loop they cost the cyclic
        # collector nothing, and a step's own cyclic garbage (autograd graphs hold device tensors) is collected by cheap, frequent
        # full collections instead of waiting for a quarter as many survivors as there are tracked objects.
        import gc
        gc.collect()
        gc.freeze()
        try:
            if dp is not None:
                dp.begin_training()
            return self._train_loop(train_data, valid_data, total_time_start, quiet, max_epochs, dp)
        finally:
            gc.unfreeze()
            if dp is not None:
                dp.end()

    def _train_loop(self, train_data, valid_data, total_time_start, quiet, max_epochs, dp=None):
        best_valid_metric, best_epoch = float("+inf"), 0
        self.validation_history = []       # (epoch, early-stopping metric); under a group the same list on every rank
        run_epoch = self._run_epoch if dp is None else dp.run_epoch
        for epoch in range(1, (max_epochs or self.params['max_epochs']) + 1):
            if dp is not None:
                dp.epoch = epoch
            self.log_line("== Epoch %i" % epoch)
            loss, res, n, gs, ns, es = run_epoch("epoch %i (training)" % epoch, train_data, DataFold.TRAIN, quiet)
            self.log_line(" Train: loss: %.5f || %s || graphs/sec: %.2f | nodes/sec: %.0f | edges/sec: %.0f"
                          % (loss, self.task.pretty_print_epoch_task_metrics(res, n), gs, ns, es))
            loss, res, n, gs, ns, es = run_epoch("epoch %i (validation)" % epoch, valid_data, DataFold.VALIDATION, quiet)
            metric = self.task.early_stopping_metric(res, n)
            self.validation_history.append((epoch, metric))
            self.log_line(" Valid: loss: %.5f || %s || graphs/sec: %.2f | nodes/sec: %.0f | edges/sec: %.0f"
                          % (loss, self.task.pretty_print_epoch_task_metrics(res, n), gs, ns, es))
            if metric < best_valid_metric:
                if dp is None or dp.rank == 0:     # (the parameters are identical on every rank: rank 0's pickle is the model)
                    self.save_model(self.best_model_file)
                best_valid_metric, best_epoch = metric, epoch
            elif epoch - best_epoch >= self.params['patience']:
                self.log_line("Stopping training after %i epochs without improvement." % self.params['patience'])
                break
        self.best_epoch = best_epoch
        if dp is not None:
            dp.barrier()                   # nobody leaves (and reads rank 0's files) before everyone is done
        self.log_line("Training took %is." % (time.time() - total_time_start))

    # -------------------- Predictions --------------------
    def predict_iter(self, data, return_states: bool = False):
        """Generator over (samples of the batch, their predictions): one dict of NumPy arrays per graph, in the order of `data`
        (the task's split_predictions says which keys; return_states adds 'node_states' float32 [n, hidden], the rows of
        compute_final_node_representations).

        The forward runs under torch.no_grad() with training=False over self._batches(data, DataFold.TEST): whichever input pipeline
        the model's parameters select.  A batch's outputs are written into ONE packed device arena (the task's kernels write their
        slices in place) that leaves the device as one asynchronous copy into pinned memory, and are read one batch late, as
        _run_epoch reads metrics: batch i is yielded once batch i + 1 is enqueued; two pinned arenas exist at most.  The fetch
        reports what a metric fetch reports: check_pending_graph_errors() and the hand-over status word (ops.HandoverError): the
        predictions of a product kernel that gave up are never handed out.

        Nothing a later training step can see is touched: no .grad, no optimizer state, no torch / NumPy random state, and
        dropout_state does not advance (nothing is dropped).  No collective: under data parallelism each rank predicts its own data."""
        data = data if isinstance(data, list) else list(data)
        # two pinned host arenas, taken in turn (batch i + 1's copy runs while batch i is read); kept with the model between calls
        # (pinning memory costs more than a small batch's forward) and taken out of it while this generator runs, so that a second
        # generator on the same model pins its own
        pinned, self._prediction_pinned = getattr(self, "_prediction_pinned", None) or [None, None], None
        try:
            yield from self._predict_batches(data, return_states, pinned)
        finally:
            self._prediction_pinned = pinned

    def _predict_batches(self, data, return_states, pinned):
        cursor, pending, turn = 0, None, 0
        for mb in self._batches(data, DataFold.TEST):
            with torch.no_grad():      # (around the device work only: a generator suspended inside it would leave the grad mode of
                #                         the CONSUMER's code switched off between two batches)
                batch = mb if isinstance(mb, DeviceBatch) else DeviceBatch(mb, self.device)
                samples = data[cursor:cursor + batch.num_graphs]
                cursor += batch.num_graphs
                final = self._final_node_states(batch, training=False)
                layout = dict(self.task.prediction_layout(batch, final.shape[1]))
                if return_states:
                    layout["node_states"] = (tuple(final.shape), torch.float32)
                arena = _PredictionArena(layout, final.device, pinned, turn)
                turn ^= 1
                outputs = self.task.compute_task_predictions(final, batch, self.variables.scope(self._task_scope), out=arena.views)
                if return_states:
                    outputs = dict(outputs, node_states=final)
                arena.send(outputs)
            if pending is not None:
                yield self._fetch_predictions(*pending)
            pending = (arena, batch, samples)
        if pending is not None:
            yield self._fetch_predictions(*pending)

    def _fetch_predictions(self, arena, batch, samples):
        host = arena.fetch()
        check_pending_graph_errors()
        return samples, self.task.split_predictions(host, batch, samples)

    def predict(self, data, return_states: bool = False, quiet: bool = True) -> List[Dict[str, np.ndarray]]:
        """One entry per graph of `data`, in its order (predict_iter, collected)."""
        results = []
        for step, (samples, predictions) in enumerate(self.predict_iter(data, return_states)):
            results.extend(predictions)
            if not quiet:
                print("Predicting, batch %i (has %i graphs). %i graphs so far." % (step, len(samples), len(results)), end='\r')
        return results

    def test(self, data, quiet: bool = False, group=None):
        """Loss and task metrics of `data`.  group: as in train(); every rank passes the SAME data, evaluates its shard of it, and
        rank 0 logs the metrics of the whole."""
        dp = self._data_parallel(group)
        if dp is None:
            loss, res, n, gs, ns, es = self._run_epoch("Test", list(data), DataFold.TEST, quiet)
        else:
            try:
                loss, res, n, gs, ns, es = dp.run_epoch("Test", list(data), DataFold.TEST, quiet)
            finally:
                dp.end()
        self.log_line("Loss %.5f on %i graphs" % (loss, n))
        self.log_line("Metrics: %s" % self.task.pretty_print_epoch_task_metrics(res, n))

    # -------------------- Data parallelism by graph (train(group=...), test(group=...)) --------------------
    def _data_parallel(self, group):
        """None for the single-GPU loop (no group, or a group of one rank: nothing below runs, no collective is issued); otherwise
        the driver of data-parallel epochs, after the refusals."""
        if group is None:
            return None
        import torch.distributed as dist
        if dist.get_world_size(group) == 1:
            return None
        from .. import config
        world = dist.get_world_size(group)
        self.task.loss_weight(1, 1)        # a task that cannot be split by graph (citation), or does not say how its loss is normalised, raises
        if self.device.type != "cuda":
            raise RuntimeError("train(group=...) / test(group=...) need the model on the GPU (one process per GPU; the gradient pack is a "
                               "HIP kernel): this model is on %s" % self.device)
        if not self.params.get('native_batching', True) or not hasattr(self.task, "make_graph_store"):
            raise RuntimeError("data-parallel training uses the native input pipelines only: %s"
                               % ("native_batching is false" if not self.params.get('native_batching', True)
                                  else "the %s task has no make_graph_store" % type(self.task).__name__))
        if config.settings.allreduce == "overlap":
            raise RuntimeError("allreduce=overlap: the bucketed all-reduce (OverlappedGradientAllReducer) is not wired into train(); "
                               "train(group=...) runs the flat packed form only and does not fall back to it silently: set allreduce=flat")
        return _DataParallel(self, group, world)


class _DataParallel:
    """Epochs of Sparse_Graph_Model.train(group=...) / test(group=...) on one rank of W (parallel.py has the host-side pieces;
    DESIGN.md section 8 the protocol).

    The shard of a fold is fixed for the run (parallel.dp_shard); the rank's pipeline is built over its shard only.  Per epoch and
    fold: shuffle (training; parallel.dp_epoch_rng), plan the local batches, exchange the plans (one all-gather, one host read).
    A training epoch then runs max_r(batches_r) steps on EVERY rank.  With a batch: train_step whose grad_hook is the packed
    reducer with this rank's scale and whose learning rate goes by the step's global graph count.  Without one: zeros into the
    same collective, the same clip and update.  Evaluation epochs run the local batches without a gradient collective.  At the
    end of every epoch the per-batch metrics and the counters are gathered in rank order."""

    def __init__(self, model: Sparse_Graph_Model, group, world: int):
        import torch.distributed as dist
        self.model, self.group, self.world = model, group, world
        self.rank = dist.get_rank(group)
        self.epoch = 0
        # collectives of small tables: device tensors under nccl, host tensors under gloo
        self.comm_device = model.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
        self.reducer = None
        self._saved_log_rank, model._log_rank = model._log_rank, self.rank

    def end(self):
        self.model._log_rank = self._saved_log_rank

    def barrier(self):
        import torch.distributed as dist
        dist.barrier(group=self.group)

    def begin_training(self):
        """Rank 0's parameters, optimizer slots and step count everywhere (a restore()d model on rank 0 included); then torch's
        generator of this device reseeded from (random_seed, rank): the torch dropout route must not share masks across ranks (the
        fused route's state block already carries the rank as its replica)."""
        import torch.distributed as dist
        from ..dense import weights_changed
        from ..parallel import PackedGradientAllReducer, dp_device_seed
        model, opt = self.model, self.model.optimizer
        src = dist.get_global_rank(self.group, 0)
        with torch.no_grad():
            for name in model.variables.names():             # (created in the same order on every rank)
                dist.broadcast(model.variables[name].data, src=src, group=self.group)
            for _, slots in opt._slots():
                for t in slots:
                    dist.broadcast(t, src=src, group=self.group)
            t_step = torch.tensor([opt.t], dtype=torch.int64, device=self.comm_device)
            dist.broadcast(t_step, src=src, group=self.group)
            opt.t = int(t_step.item())
        opt.sync_device_step_count()
        weights_changed()
        torch.cuda.default_generators[model.device.index if model.device.index is not None
                                      else torch.cuda.current_device()].manual_seed(dp_device_seed(model.params['random_seed'], self.rank))
        self.reducer = PackedGradientAllReducer(opt.params, group=self.group)

    def _pipeline(self, data):
        """(the rank's input pipeline over its shard of `data`, or None for an empty shard; the largest shard's graph count)."""
        model = self.model
        folds = model.__dict__.setdefault("_dp_folds", {})
        key = (id(data), len(data), self.world, self.rank)
        kept = folds.get(key)
        if kept is None or kept[0] is not data:
            from ..parallel import dp_shard
            shards = dp_shard(data, self.world)
            kept = folds[key] = (data, [data[i] for i in shards[self.rank]], max(len(s) for s in shards))
            while len(folds) > 3:      # train + validation folds and one more, like the pipelines themselves
                folds.pop(next(iter(folds)))
        _, mine, largest = kept
        return (model._native_pipeline(mine) if mine else None), largest

    def run_epoch(self, epoch_name: str, data, data_fold: DataFold, quiet: bool = False):
        """_run_epoch across the group: the same six results on every rank, over the whole fold."""
        from ..parallel import dp_epoch_rng, dp_exchange_plans, dp_merge_epoch, dp_plan_epoch, dp_schedule
        model, task = self.model, self.model.task
        train = data_fold == DataFold.TRAIN
        max_nodes = model.params['max_nodes_in_batch']
        seed = model.params['random_seed']
        pipeline, largest_shard = self._pipeline(data)
        plan = dp_plan_epoch(pipeline.store if pipeline is not None else None, train, max_nodes,
                             dp_epoch_rng(seed, self.epoch, self.rank))
        plans = dp_exchange_plans(plan, largest_shard, self.group, self.comm_device)
        local_steps = len(plan.batches)
        if train:
            if self.reducer is None:
                raise RuntimeError("a data-parallel training epoch outside train(group=...)")
            schedule = dp_schedule([[(task.loss_weight(g, n), g) for g, n in p] for p in plans])
            steps = schedule.steps
        else:
            schedule, steps = None, local_steps
        batch_iterator = iter(()) if pipeline is None else iter(task.make_native_minibatch_iterator(
            pipeline, data_fold, max_nodes, rng=dp_epoch_rng(seed, self.epoch, self.rank)))
        start_time = time.time()
        task_metric_results = []
        state = {"graphs": 0, "nodes": 0, "edges": 0, "loss": 0.0, "step": 0}

        def fetch(pending):
            m, mb = pending
            m = m.get()
            check_pending_graph_errors()
            state["graphs"] += mb.num_graphs
            state["nodes"] += mb.num_nodes
            state["edges"] += mb.num_edges
            state["loss"] += m['loss'] * mb.num_graphs
            task_metric_results.append(m)
            if not quiet and self.rank == 0:
                print("Running %s, batch %i (has %i graphs on rank 0). Loss so far: %.4f"
                      % (epoch_name, state["step"], mb.num_graphs, state["loss"] / state["graphs"]), end='\r')
            state["step"] += 1

        pending = None
        upcoming = next(batch_iterator, None)
        for k in range(steps):
            if k < local_steps:
                batch = upcoming
                if batch is None or (batch.num_graphs, batch.num_nodes) != (int(plan.graphs[k]), int(plan.nodes[k])):
                    raise RuntimeError("%s, step %d: the input pipeline did not assemble the planned batch" % (epoch_name, k))
                if train:
                    scale = float(schedule.scales[self.rank, k])
                    m = model.train_step(batch, grad_hook=lambda params, s=scale: self.reducer(s),
                                         lr_num_graphs=int(schedule.graph_sums[k]))
                else:
                    with torch.no_grad():
                        m = model.forward_batch(batch, training=False)
                readback = MetricsReadback(m)
                upcoming = next(batch_iterator, None)      # (the same pipelining as _run_epoch: metrics are read one step late)
                if pending is not None:
                    fetch(pending)
                pending = (readback, batch)
            else:
                # no batch left on this rank: zeros into the step's collective, the same clip and update as everyone else
                # (parameters, optimizer slots and the step count stay identical across the ranks)
                model.optimizer.zero_grad()
                self.reducer(0.0)
                model.optimizer.clip_and_step(model._lr_scale(int(schedule.graph_sums[k])))
        if upcoming is not None:
            raise RuntimeError("%s: the input pipeline holds more batches than planned" % epoch_name)
        if pending is not None:
            fetch(pending)
        merged, (loss_sum, graphs, nodes, edges) = dp_merge_epoch(
            task_metric_results, (state["loss"], state["graphs"], state["nodes"], state["edges"]), self.group)
        epoch_time = time.time() - start_time
        graphs, nodes, edges = int(graphs), int(nodes), int(edges)
        return (loss_sum / max(graphs, 1), merged, graphs, graphs / epoch_time, nodes / epoch_time, edges / epoch_time)
