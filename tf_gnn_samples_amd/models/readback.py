"""What a step sends back to the host, read one step late: the metric scalars of a training / evaluation step (MetricsReadback), the
predictions of a batch (_PredictionArena), the order in which a loop reads them (LateFetch) and what an epoch adds up (EpochTally)."""
import time
from typing import Any, Dict

import numpy as np
import torch

from .. import ops
from ..graph import check_pending_graph_errors


class LateFetch:
    """Holds at most one item on its way to the host and fetches it one step late.  The order of one iteration of a loop that
    uses it is the contract (a measured property: read in the wrong place, the device idles ~0.2 ms per 2.9 ms C2 step):

      1. launch the step (train_step, forward_batch, or the prediction forward);
      2. enqueue its readback (MetricsReadback(...); for predictions arena.send(...));
      3. next() on the batch iterator: the next batch's upload / assembly run on a side stream under this step's kernels;
      4. put(this step's item): fetches the PREVIOUS step's.  That wait is for the previous step's copy only, which the GPU has
         passed long ago, so the device never idles behind a host round trip.  `fetch` runs check_pending_graph_errors() and the
         hand-over status check (ops.report_handover);
      5. after the last batch, flush() fetches the last one.

    put() and flush() return what `fetch` returned, None when nothing was pending.  A fetch that raises leaves nothing pending: as
    in a loop that an exception ends, the newer item is dropped unread and a later flush() returns None."""

    def __init__(self, fetch):
        self._fetch, self._pending = fetch, None

    def put(self, item):
        previous, self._pending = self._pending, None
        fetched = None if previous is None else self._fetch(previous)
        self._pending = item
        return fetched

    def flush(self):
        return self.put(None)


class EpochTally:
    """The counters of one epoch (__run_epoch, models/sparse_graph_model.py:263-311 of the reference), fed one (MetricsReadback,
    batch) pair at a time; `where` goes into the progress line behind the batch's graph count."""

    def __init__(self, epoch_name: str, quiet: bool, where: str = ""):
        self._epoch_name, self._quiet, self._where = epoch_name, quiet, where
        self.graphs = self.nodes = self.edges = self.step = 0
        self.loss = 0.0                     # sum of loss * graphs
        self.results = []
        self._start_time = time.time()

    def fetch(self, pending):
        """Read one step's metrics back (the host sync of sess.run's fetch, :293)."""
        readback, mb = pending
        m = readback.get()
        check_pending_graph_errors()
        self.graphs += mb.num_graphs
        self.nodes += mb.num_nodes
        self.edges += mb.num_edges
        self.loss += m['loss'] * mb.num_graphs
        self.results.append(m)
        if not self._quiet:
            print("Running %s, batch %i (has %i graphs%s). Loss so far: %.4f"
                  % (self._epoch_name, self.step, mb.num_graphs, self._where, self.loss / self.graphs), end='\r')
        self.step += 1

    def totals(self):
        return self.loss, self.graphs, self.nodes, self.edges

    def result(self, results=None, totals=None):
        """(avg loss, task metric results, graphs, graphs/s, nodes/s, edges/s) of this tally, or of what the ranks' tallies merge into."""
        loss, graphs, nodes, edges = self.totals() if totals is None else totals
        epoch_time = time.time() - self._start_time
        graphs, nodes, edges = int(graphs), int(nodes), int(edges)
        return (loss / max(graphs, 1), self.results if results is None else results, graphs, graphs / epoch_time,
                nodes / epoch_time, edges / epoch_time)


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
            word = ops.handover_word_if_any(device)
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
            ops.report_handover(status, self._device)
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
        self._table, used = {}, 0           # key -> (offset, nbytes, torch dtype, numpy dtype, shape)
        for key, (shape, dtype) in layout.items():
            np_dtype = torch.empty((), dtype=dtype).numpy().dtype
            offset = (used + 15) // 16 * 16
            nbytes = int(np.prod(shape, dtype=np.int64)) * np_dtype.itemsize
            self._table[key] = (offset, nbytes, dtype, np_dtype, shape)
            used = offset + nbytes
        self._status_at = (used + 3) // 4 * 4
        self._nbytes = self._status_at + 4
        self._device, self._pinned, self._turn, self._event = device, pinned, turn, None
        self.buf = torch.empty(self._nbytes, dtype=torch.uint8, device=device)
        self.views = {key: self._view(self.buf, key) for key in layout}

    def _view(self, buf, key):
        offset, nbytes, dtype, _, shape = self._table[key]
        return buf[offset:offset + nbytes].view(dtype).view(shape)

    def send(self, outputs: Dict[str, torch.Tensor]):
        for key, view in self.views.items():
            t = outputs[key]
            if t.data_ptr() != view.data_ptr() or tuple(t.shape) != tuple(view.shape):      # (a hook that made a tensor of its own)
                view.copy_(t)
        if self._device.type != "cuda":
            self._host = self.buf
            return
        word = ops.handover_word_if_any(self._device)
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
            ops.report_handover(int(self._host[self._status_at:].view(torch.int32)[0]), self._device)      # as a metric fetch does
        own = self._host.numpy().copy()                                  # one host copy out of the pinned arena; the pieces are its views
        out = {key: own[offset:offset + nbytes].view(np_dtype).reshape(shape)
               for key, (offset, nbytes, _, np_dtype, shape) in self._table.items()}
        self.buf = self.views = None
        return out
