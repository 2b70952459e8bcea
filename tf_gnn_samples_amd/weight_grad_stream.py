"""Weight gradients on a side stream: the protocol by which a backward of this package computes its parameters' gradients next to its
input gradient, and the one helper (fork) every autograd function that does so goes through.  The main stream joins the side stream
at the end of the layer's backward() or, inside train_step (deferred_weight_gradient_join), once behind the whole backward
(join_deferred); deferred_targets_ok states when the second is safe, join_deferred verifies afterwards that autograd kept to it.
Users: ops.typed._TypedLinearPanel (one pair table or both of a layer), ops.rgcn._AggregateThenTransform (either join),
dense._DenseFn, _DenseMultiFn and utils._GRUCellFn (deferred only).  ops re-exports the public names below."""
import torch

from .config import settings as _cfg

# config.settings.bwd_overlap (RELGNN_BWD_OVERLAP; auto = on with the limb route): the weight gradient of the aggregate-first RGCN layer on a side stream next to the input gradient's
# gather.  Measured on the C2 step, alternated twice in one process group: 2.006 / 2.014 ms without, 1.955 / 1.955 ms with (round 2
# measured the opposite, 3.08 vs 2.94 ms, with the library's split-K GEMM in that place: it wanted the same CUs and the same L2 as the
# gather; the limb kernel is one 147 KB-LDS workgroup per CU that leaves registers and the L2 path to the gather's waves).
# With the exact-fp32 routes (RELGNN_GEMM=lib / panel) the default is off: 2.45 vs 2.22 ms.
_SIDE_STREAMS = {}


# The join of the side stream (main stream waits for the weight gradient) normally sits at the end of the layer's backward: whatever
# reads the gradient next finds it complete.  A training step that owns the whole backward can do better: nothing reads a weight
# gradient before the optimizer, and next to the gather the side stream's workgroups starve (the gather's 27 k four-wave workgroups
# hold every wave slot and register), so its kernels really start at the gather's tail and finish AFTER the input-gradient product
# — the main stream then idled at every layer's join.  deferred_weight_gradient_join() (models/sparse_graph_model.py: train_step)
# moves the joins to join_deferred(), called once behind the backward.
_DEFER = {"on": False, "pending": [], "targets": set(), "handed": []}


class deferred_weight_gradient_join:
    def __enter__(self):
        self._old = _DEFER["on"]
        _DEFER["on"] = True
        return self

    def __exit__(self, exc_type, exc, tb):
        _DEFER["on"] = self._old
        if exc_type is not None:
            # the backward raised (out of memory, a check inside a Function): nobody will call join_deferred() for this pass.  Wait
            # for the side streams and forget the pass — stale `handed` entries would hold the parameters alive and make the NEXT
            # step's join verify gradients that belong to this one
            pending, _DEFER["pending"] = _DEFER["pending"], []
            _DEFER["handed"] = []
            _DEFER["targets"].clear()
            for device, side in pending:
                try:
                    torch.cuda.current_stream(device).wait_stream(side)
                except Exception:
                    pass
        return False


def _accumulator_keeps_the_tensor(p) -> bool:
    """Will autograd's AccumulateGrad take the gradient tensor of leaf `p` as it is, launching nothing on the main stream?  It
    copies (reads the tensor at once) when a tensor hook sits on the parameter (the gradient passes through Python and gains a
    reference), when the layouts differ, and under create_graph (grad mode on inside the backward); anomaly mode inspects every
    gradient; a post-accumulate hook reads p.grad right behind the accumulation."""
    return (p.is_leaf and p.requires_grad and p.grad is None and p.is_contiguous()
            and not getattr(p, "_backward_hooks", None) and not getattr(p, "_post_accumulate_grad_hooks", None))


def deferred_targets_ok(params, device) -> bool:
    """May a weight gradient be left in flight on the side stream until join_deferred()?  Only if nothing on the main stream reads
    it before: every target must be a LEAF that has no gradient yet and has not been a target in this backward pass — autograd's
    accumulator then keeps the tensor itself and launches nothing (_accumulator_keeps_the_tensor lists what else makes it copy;
    join_deferred() verifies afterwards that it did keep it).  A parameter used twice in the graph (the timesteps of a GGNN
    layer share their weights) has its contributions SUMMED on the main stream (in the engine's input buffer, or `grad += new`),
    which would read tensors that are still being written: on the second sight of a parameter the main stream is made to wait for
    the side stream here and the caller computes on one stream."""
    seen = _DEFER["targets"]
    if (params is not None and not torch.is_grad_enabled() and not torch.is_anomaly_enabled()
            and all(_accumulator_keeps_the_tensor(p) and id(p) not in seen for p in params)):
        seen.update(id(p) for p in params)
        return True
    wait_if_in_flight(params, device)
    return False


def wait_if_in_flight(params, device) -> None:
    """A contribution to `params` is about to be produced on the main stream.  If an earlier one of this backward went aside,
    autograd will sum the two on the main stream: it waits for the side stream first.  The parameters are marked as seen either
    way — a LATER contribution must not go aside either (the engine would add it, still in flight, to the one buffered here).
    Called on every sight of a parameter that does not go aside itself, whatever else the caller computes.  (A view's or a
    non-leaf's gradient never goes aside and is consumed by the view's backward at once: params is None for those.)"""
    if params is None:
        return
    seen = _DEFER["targets"]
    if any(id(p) in seen for p in params):
        side = _SIDE_STREAMS.get(device)
        if side is not None:
            torch.cuda.current_stream(device).wait_stream(side)
        # their first contributions are complete as far as the main stream is concerned from here on: summing into them is safe and
        # join_deferred() has nothing left to verify for these parameters
        mine = {id(p) for p in params}
        _DEFER["handed"] = [h for h in _DEFER["handed"] if id(h[0]) not in mine]
    if _DEFER["on"]:
        seen.update(id(p) for p in params)


def hand_over_deferred(device, side, params, grads) -> None:
    """Record that `grads` (in flight on `side`) are being returned to autograd as the gradients of the leaves `params`."""
    _DEFER["pending"].append((device, side))
    for p, g in zip(params, grads):
        if g is not None:
            _DEFER["handed"].append((p, g.data_ptr(), g._version))


def join_deferred() -> None:
    """Make the current stream wait for every side stream whose join was deferred (no host synchronisation), then check that
    autograd did what the deferral relies on: every parameter's .grad IS the tensor that was handed over (same storage, never
    written in place since).  Anything else means the main stream read or wrote a gradient that was still being produced — raised
    here rather than left as a silently wrong update."""
    pending, _DEFER["pending"] = _DEFER["pending"], []
    handed, _DEFER["handed"] = _DEFER["handed"], []
    _DEFER["targets"].clear()
    done = set()
    for device, side in pending:
        if id(side) not in done:
            torch.cuda.current_stream(device).wait_stream(side)
            done.add(id(side))
    for p, ptr, version in handed:
        g = p.grad
        if g is None or g.data_ptr() != ptr or g._version != version:
            raise RuntimeError(
                "deferred weight-gradient join: the gradient of a %s parameter was %s on the main stream while its producer was "
                "still in flight on the side stream (a second use of the parameter outside this package's layers, a hook, or a "
                "copying accumulator); run the backward without ops.deferred_weight_gradient_join() or set bwd_overlap=0"
                % (tuple(p.shape), "dropped" if g is None else "copied" if g.data_ptr() != ptr else "accumulated into in place"))


def _side_stream(device):
    st = _SIDE_STREAMS.get(device)
    if st is None:
        # (a high-priority queue changes nothing here: measured 1.810 / 1.813 ms on C2, 32.5 / 33.0 ms on C5 — the side stream's
        #  large workgroups still become resident only where the main stream's small ones leave room)
        st = _SIDE_STREAMS[device] = torch.cuda.Stream(device=device)
    return st


class _Aside:
    """The gradients of one backward node in flight on the side stream (fork)."""

    def __init__(self, device, side, params, grads, deferred):
        self.device, self.side, self.params, self.grads, self.deferred = device, side, params, grads, deferred

    def join(self):
        """run()'s gradients, fit to be handed to autograd.  Called BEHIND the caller's input-gradient launches: outside a deferred
        pass the main stream waits for the side stream here, and everything launched between fork() and here is the overlap."""
        cur = torch.cuda.current_stream(self.device)
        if self.deferred:
            hand_over_deferred(self.device, self.side, self.params, self.grads)
        else:
            cur.wait_stream(self.side)
        for g in self.grads:
            if g is not None:
                g.record_stream(cur)
        return self.grads


def fork(run, operands, params, *, want, join_in_backward, contributes):
    """The weight (and bias) gradients of one backward node on the side stream, next to whatever the caller launches until join():
        aside = fork(run, operands, params, want=.., join_in_backward=.., contributes=..)    # None: they stay on this stream
        ...                                                                                 # the input gradient
        grads = aside.join() if aside is not None else run()
    run() launches the products and returns the gradients exactly as they go back to autograd: a tuple, one entry per parameter in
    `params` order, None where none is needed (views — unbind, row blocks — cost no launch).  `operands`: every tensor run() reads
    that lives in the main stream's pool.  `params`: the leaf parameters the gradients go to, or None (a view's or a non-leaf's
    gradient is consumed on the main stream at once and never stays in flight).
    When the work goes aside: only if all of these hold, looked at in this order —
      * `want` (the caller has an input gradient to overlap with and a weight gradient to compute),
      * config.settings.bwd_overlap_on,
      * every operand is a CUDA tensor,
      * inside deferred_weight_gradient_join(): deferred_targets_ok(params, device); outside: `join_in_backward`.  The typed products
        and the aggregate-first layer pass True; the Dense layers and the GRU cell pass False: with the join inside backward() the
        move was measured and lost for them (both of their products are matrix-pipe kernels: 2.02 vs 1.94 ms per C2 step), while
        under a deferred join their gradients leave the critical path and run under the next layer's gather (1.826 -> 1.807 ms).
    deferred_targets_ok has side effects (it marks the parameters as targets of this pass, or makes the main stream wait for their
    earlier contributions): it is evaluated last and only when everything else already holds.
    Fork: side.wait_stream(current); run() under torch.cuda.stream(side); every operand gets record_stream(side).  A tensor that
    run() allocates belongs to the side stream's pool: nothing outside run() may read an intermediate of it.
    Join (_Aside.join): deferred, one hand_over_deferred(device, side, params, grads) per fork, i.e. one _DEFER["pending"] entry per
    backward node that went aside; not deferred, current.wait_stream(side), issued by join() and never here — its place behind the
    input gradient IS the overlap.  Either way every gradient gets record_stream(current).
    Not going aside: wait_if_in_flight(params, device) runs before run() produces the contribution on the main stream, if
    `contributes` (the typed products and the aggregate-first layer: a weight gradient is wanted; the Dense layers and the GRU cell:
    the first operand is on the GPU)."""
    device = operands[0].device
    aside = want and _cfg.bwd_overlap_on and all(t.is_cuda for t in operands)
    if aside and _DEFER["on"]:
        if not deferred_targets_ok(params, device):
            return None                                   # (it has made the main stream wait and marked the parameters itself)
    elif not (aside and join_in_backward):
        # at decision time, also for the callers whose run() comes only behind their input gradient: it does something only while
        # _DEFER["targets"] holds these parameters, i.e. inside a deferred pass, where the main stream has to wait before the
        # contribution either way and the input gradient in between does not touch the side stream
        if contributes:
            wait_if_in_flight(params, device)             # (no-op unless an earlier use of these parameters went aside)
        return None
    side = _side_stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        grads = run()
    for t in operands:
        t.record_stream(side)
    return _Aside(device, side, params, grads, _DEFER["on"])
