"""Data parallelism BY GRAPH across the GPUs of one node.

A minibatch of the reference is a disjoint union of graphs (tasks/ppi_task.py:220-233): no edge
crosses graphs, so message passing never communicates.  Whole graphs are assigned to ranks
(balanced by edge count), every rank builds its own local disjoint-union batch exactly as the
single-GPU batcher would, and the ONLY collective is one all-reduce(SUM) of the flat fp32
gradient per step over RCCL/xGMI (one process per GPU, torch.distributed backend "nccl" == RCCL).

Objective equivalence with the single-batch reference loss (tasks/ppi_task.py:183-191,
loss = total_loss / num_nodes_in_batch): rank r holds g_r = d(total_r / n_r); the global gradient
is sum_r n_r * g_r / sum_r n_r.  The weight n_r rides in the last slot of the same flat buffer, so
there is exactly one collective.  Per-variable clip_by_norm (models/sparse_graph_model.py:253-260)
is applied AFTER the all-reduce.

Sparse_Graph_Model.train(group=...) / test(group=...) drive whole epochs this way.  What they need beyond
one step is below the reducers: the shard of a fold, the per-epoch shuffle, the local batch plan, its exchange (one all-gather
per epoch and fold) and the schedule every rank derives from it on the host: the number of steps, the per-step weight sum W_k
and graph count G_k, and each rank's scale float32(w_rk / W_k).  PackedGradientAllReducer applies that scale while it packs
(csrc/parallel.hip, one launch), so the one all-reduce(SUM) leaves the weighted mean with nothing behind it.
"""
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


def shard_graphs_by_edges(edge_counts: Sequence[int], world_size: int) -> List[List[int]]:
    """Greedy longest-processing-time assignment of whole graphs to ranks, balancing sum_l E_l.
    Deterministic (ties broken by graph index / lowest rank); each shard keeps ascending graph order."""
    order = sorted(range(len(edge_counts)), key=lambda i: (-int(edge_counts[i]), i))
    loads = [0] * world_size
    shards: List[List[int]] = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (loads[k], k))
        shards[r].append(i)
        loads[r] += int(edge_counts[i])
    return [sorted(s) for s in shards]


def refuse_single_graph_task(task_name: str) -> None:
    """Data parallelism here is BY GRAPH; a task whose fold is one graph that is always the whole batch (the citation networks)
    has nothing to split.  Its batch iterators call this: under a process group of more than one rank it raises."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError("the %s task trains on ONE graph that is the whole batch: it cannot be split by graph across %d ranks; "
                           "run it on a single GPU" % (task_name, dist.get_world_size()))


def effective_cpu_count() -> int:
    """CPUs this process may actually keep busy: the cgroup CPU quota (v2 cpu.max, v1 cfs quota) and the affinity
    mask, whichever is smaller.  os.cpu_count() reports the host's hardware threads (256 on the MI355X boxes) even when
    the container is capped at 16 CPUs; running more busy threads than the quota gets the whole process throttled for
    the rest of the 100 ms scheduler period (observed: 30-60 ms stalls in host-side batching)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p_ = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and p_ > 0:
                n = min(n, max(1, q // p_))
        except (OSError, ValueError):
            pass
    return max(1, n)


def init_distributed(backend: str = None):
    """One process per GPU; reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        kwargs = {}
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            # bind the communicator to this rank's GPU up front (no device guessing inside barrier()/collectives)
            kwargs["device_id"] = torch.device("cuda", local_rank)
        try:
            dist.init_process_group(backend=backend, rank=rank, world_size=world, **kwargs)
        except TypeError:        # older torch without device_id
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


class GradientAllReducer:
    """Weighted gradient average across ranks with ONE all-reduce of one flat fp32 buffer."""

    def __init__(self, params: Sequence[torch.nn.Parameter], group=None):
        self.params = [p for p in params if p.requires_grad]
        self.group = group
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device if self.params else torch.device("cpu")
        self.flat = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        self.views = []
        off = 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()

    @property
    def nbytes(self) -> int:
        return self.flat.numel() * 4

    @torch.no_grad()
    def __call__(self, local_weight: float):
        """grad <- sum_r w_r * grad_r / sum_r w_r  (w_r = local_weight, e.g. nodes in the local batch)."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self.group) == 1:
            return
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in self.params]
        torch._foreach_copy_(self.views, grads)
        self.flat[:-1].mul_(float(local_weight))
        self.flat[-1] = float(local_weight)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self.flat[:-1].div_(self.flat[-1])
        # the reduced gradients stay where they are: every .grad becomes a view of the flat buffer (no unpack copies;
        # the next backward allocates fresh .grad tensors after zero_grad() and this buffer is overwritten by the pack)
        for p, v in zip(self.params, self.views):
            p.grad = v


class OverlappedGradientAllReducer(GradientAllReducer):
    """The same weighted average, with the collective cut into buckets that leave while the backward is still running
    (RELGNN_ALLREDUCE=overlap in bench.py; the flat one-collective form stays the default until an N > 1 run has timed both).

    Buckets are contiguous ranges of the same flat buffer, filled from its END (the backward produces the last layers'
    gradients first): a parameter's post-accumulate hook counts its bucket down, a complete bucket is packed (one
    multi-tensor copy + one scale by the local weight) and all-reduced asynchronously.  The local weight n_r — known before the
    backward — is reduced by its own tiny collective at arm() time; finish() (the training step's grad_hook) launches what
    is left (parameters that received no gradient count as zeros), waits, divides by sum_r n_r and points every .grad at its
    slice, exactly like the flat form.  For two ranks the result is bit-identical to the flat form (a sum of two values has
    one order); for more ranks the reduction order of an element may depend on where the library cuts its buffer.

    Collectives must be issued in the SAME sequence on every rank, and the order in which autograd completes buckets is not a
    property of the model: which parameters get a gradient at all, and when, follows the autograd graph of THIS rank's batch
    (hub routes, pair tables and typed panels are picked per batch).  So buckets leave strictly in index order, as in DDP: a
    complete bucket is launched only when every bucket before it has been — otherwise it waits for a later hook or for finish(),
    which launches whatever is left, again in index order.  Two ranks whose backward passes complete their buckets in different
    orders (tests/test_distributed_cpu.py) therefore still pair bucket b with bucket b."""

    def __init__(self, params: Sequence[torch.nn.Parameter], bucket_bytes: int = 1 << 20, group=None):
        super().__init__(params, group)
        offs, off = [], 0
        for p in self.params:
            offs.append(off)
            off += p.numel()
        self.buckets = []                       # (lo, hi, [param indices]) in the order the backward completes them
        members, hi = [], off
        for i in reversed(range(len(self.params))):
            members.append(i)
            if (hi - offs[i]) * 4 >= bucket_bytes or i == 0:
                self.buckets.append((offs[i], hi, members[::-1]))
                members, hi = [], offs[i]
        self.bucket_of = {}
        for b, (_, _, idx) in enumerate(self.buckets):
            for i in idx:
                self.bucket_of[i] = b
        self._armed = False
        self._handles = [p.register_post_accumulate_grad_hook(self._make_hook(i)) for i, p in enumerate(self.params)]

    def close(self) -> None:
        """Remove the post-accumulate hooks (a reducer that is dropped while its parameters live on; with the hooks in place
        ops.deferred_targets_ok keeps every weight gradient on the main stream)."""
        for h in self._handles:
            h.remove()
        self._handles = []

    def _make_hook(self, i):
        def hook(_param):
            if self._armed:
                self._left[self.bucket_of[i]] -= 1
                self._launch_ready_prefix()
        return hook

    def _launch_ready_prefix(self) -> None:
        while self._next < len(self.buckets) and self._left[self._next] == 0:
            self._launch(self._next)
            self._next += 1

    def _active(self) -> bool:
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1

    @torch.no_grad()
    def arm(self, local_weight: float) -> None:
        """Call before the backward of the step."""
        if not self._active():
            return
        self._w = float(local_weight)
        self._left = [len(idx) for _, _, idx in self.buckets]
        self._next = 0                          # buckets [0, _next) have been launched: strictly in index order on every rank
        self.flat[-1] = self._w
        self._works = [dist.all_reduce(self.flat[-1:], op=dist.ReduceOp.SUM, group=self.group, async_op=True)]
        self._armed = True

    @torch.no_grad()
    def _launch(self, b: int) -> None:
        lo, hi, idx = self.buckets[b]
        grads = [self.params[i].grad if self.params[i].grad is not None else torch.zeros_like(self.params[i]) for i in idx]
        torch._foreach_copy_([self.views[i] for i in idx], grads)
        self.flat[lo:hi].mul_(self._w)
        self._works.append(dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    @torch.no_grad()
    def finish(self) -> None:
        """The training step's grad_hook: after the backward, before clipping."""
        if not self._armed:
            return
        self._armed = False
        while self._next < len(self.buckets):   # what the hooks left: incomplete buckets (parameters without a gradient) included
            self._launch(self._next)
            self._next += 1
        for w in self._works:
            w.wait()
        self._works = []
        self.flat[:-1].div_(self.flat[-1])
        for p, v in zip(self.params, self.views):
            p.grad = v

    def __call__(self, local_weight: float):
        """Without arm() before the backward this is the flat form's call: everything at once."""
        if not self._armed:
            self.arm(local_weight)
        self.finish()


# ---- whole epochs: shard, shuffle, plan, exchange, schedule (host only; Sparse_Graph_Model.train(group=...)) -----------------

def dp_shard(data: Sequence, world_size: int) -> List[List[int]]:
    """The shard of every rank for one data fold, fixed for the run: shard_graphs_by_edges over each sample's edge count
    (all edge types).  Every rank computes the whole table, so every rank knows every shard's size."""
    return shard_graphs_by_edges([sum(len(a) for a in g.adjacency_lists) for g in data], world_size)


def dp_epoch_rng(random_seed: int, epoch: int, rank: int) -> np.random.RandomState:
    """The generator that shuffles `rank`'s shard in training epoch `epoch`: seeded from (random_seed, epoch, rank), so a plan
    and the iterator that assembles its batches draw the same order from two instances."""
    return np.random.RandomState(np.array([int(random_seed) % 2 ** 32, int(epoch) % 2 ** 32, int(rank)], dtype=np.uint32))


def dp_device_seed(random_seed: int, rank: int) -> int:
    """Seed of torch's device generator on `rank` (the torch dropout route: ranks must not share masks)."""
    return int(np.random.SeedSequence([int(random_seed) % 2 ** 32, int(rank)]).generate_state(1, dtype=np.uint64)[0] >> np.uint64(1))


class DpEpochPlan(NamedTuple):
    """A rank's batches of one epoch and fold, known before any of them is assembled."""
    ids: np.ndarray                 # the store's graph ids in the epoch's order
    batches: List[np.ndarray]       # store.split_batches(ids, max_nodes_per_batch): what iterate() will assemble, in order
    graphs: np.ndarray              # int64 [local steps]
    nodes: np.ndarray               # int64 [local steps]


def dp_plan_epoch(store, shuffle: bool, max_nodes_per_batch: int, rng: Optional[np.random.RandomState] = None) -> DpEpochPlan:
    """The batches make_native_minibatch_iterator(pipeline over `store`, fold, max_nodes_per_batch, rng) will yield: the same
    arange, the same one shuffle (training folds), the same split rule.  store=None is an empty shard."""
    if store is None or store.num_graphs == 0:
        empty = np.zeros(0, np.int64)
        return DpEpochPlan(empty, [], empty, empty)
    ids = np.arange(store.num_graphs)
    if shuffle:
        (rng or np.random).shuffle(ids)
    batches = store.split_batches(ids, max_nodes_per_batch)
    graphs = np.array([len(b) for b in batches], dtype=np.int64)
    nodes = np.array([int((store.node_off[b + 1] - store.node_off[b]).sum()) for b in batches], dtype=np.int64)
    return DpEpochPlan(ids, batches, graphs, nodes)


def dp_exchange_plans(plan: DpEpochPlan, max_local_steps: int, group=None, device=None) -> List[List[Tuple[int, int]]]:
    """Every rank's (graphs, nodes) per local step, in rank order, on every rank: ONE all-gather of an int64 table of
    max_local_steps + 1 rows (row 0 holds the rank's step count; max_local_steps is a bound every rank knows, e.g. the largest
    shard's graph count) and one read of the gathered tables.  `device`: where the table lives (the GPU under nccl, the host under gloo)."""
    n = len(plan.batches)
    if n > max_local_steps:
        raise ValueError("dp_exchange_plans: %d local steps, the agreed bound is %d" % (n, max_local_steps))
    table = np.zeros((max_local_steps + 1, 2), dtype=np.int64)
    table[0, 0] = n
    table[1:n + 1, 0] = plan.graphs
    table[1:n + 1, 1] = plan.nodes
    mine = torch.from_numpy(table)
    if device is not None and torch.device(device).type != "cpu":
        mine = mine.to(device)
    world = dist.get_world_size(group)
    gathered = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine, group=group)
    host = torch.stack(gathered).cpu().numpy()                      # the epoch's one host read
    return [[(int(g), int(v)) for g, v in host[r, 1:int(host[r, 0, 0]) + 1]] for r in range(world)]


class DpSchedule(NamedTuple):
    steps: int                      # max_r(local steps): every rank issues this many reductions
    weight_sums: np.ndarray         # float64 [steps]: W_k = sum_r w_rk
    graph_sums: np.ndarray          # int64 [steps]:   G_k = sum_r graphs_rk (what lr_for_num_graphs_per_batch scales by)
    scales: np.ndarray              # float32 [world, steps]: float32(w_rk / W_k), the quotient formed in double; 0 without a batch


def dp_schedule(per_rank_steps: Sequence[Sequence[Tuple[float, int]]]) -> DpSchedule:
    """per_rank_steps[r][k] = (loss weight, graphs) of rank r's k-th batch.  A rank with fewer batches than the longest (none at
    all included) takes part in the remaining steps with weight 0."""
    world = len(per_rank_steps)
    steps = max((len(p) for p in per_rank_steps), default=0)
    w = np.zeros((world, steps), dtype=np.float64)
    g = np.zeros((world, steps), dtype=np.int64)
    for r, p in enumerate(per_rank_steps):
        for k, (weight, graphs) in enumerate(p):
            if not weight > 0:
                raise ValueError("dp_schedule: rank %d step %d has loss weight %r; a batch weighs more than nothing" % (r, k, weight))
            w[r, k], g[r, k] = float(weight), int(graphs)
    weight_sums = np.zeros(steps, dtype=np.float64)
    for r in range(world):                                           # in rank order, the same on every rank
        weight_sums += w[r]
    scales = (w / weight_sums).astype(np.float32) if steps else np.zeros((world, 0), np.float32)
    return DpSchedule(steps, weight_sums, g.sum(axis=0), scales)


class SingleGraphSchedule(NamedTuple):
    """One TRAIN epoch of a task whose data is ONE graph, handed out to the ranks batch by batch."""
    steps: int                      # ceil(batches / world): every rank issues this many reductions
    owner: np.ndarray               # int64 [batches]: global batch j belongs to rank j mod world ...
    step: np.ndarray                # int64 [batches]: ... at step j // world
    draws: np.ndarray               # int64 [batches]: the sampler's draw index of batch j, the single-GPU loop's: epoch * batches + j
    scales: np.ndarray              # float32 [world, steps]: dp_schedule's; 0 where a rank holds no batch in the last step


def single_graph_schedule(batch_weights: Sequence[float], world_size: int, epoch: int = 0) -> SingleGraphSchedule:
    """batch_weights[j]: what batch j of the epoch weighs in the mean over its step (the citation task: its seed count under
    `sampled_batches`, the same for every batch under `subgraph_batches`).  The ranks together run the batches of the single-GPU
    epoch, world_size at a time; every epoch has the same number of batches, so the draws of epoch e start at e * batches."""
    batches = len(batch_weights)
    j = np.arange(batches, dtype=np.int64)
    schedule = dp_schedule([[(float(batch_weights[i]), 1) for i in range(r, batches, world_size)] for r in range(world_size)])
    return SingleGraphSchedule(schedule.steps, j % world_size, j // world_size, int(epoch) * batches + j, schedule.scales)


def dp_order_by_batch(per_rank: Sequence[Sequence[Any]]) -> List[Any]:
    """per_rank[r]: what rank r holds for its batches r, r + W, r + 2W, ... of an epoch, in that order.  -> the same items in the
    order of the global batch index, which is the order a single process meets them in."""
    world = len(per_rank)
    total = sum(len(part) for part in per_rank)
    for r, part in enumerate(per_rank):
        if len(part) != len(range(r, total, world)):
            raise ValueError("dp_order_by_batch: rank %d holds %d of %d batches dealt out in turn to %d ranks, not %d"
                             % (r, len(part), total, world, len(range(r, total, world))))
    return [per_rank[j % world][j // world] for j in range(total)]


def dp_gather_by_batch(items: Sequence[Any], group=None) -> List[Any]:
    """End of an epoch whose batches were dealt out in turn: every rank's per-batch items, in batch order, on every rank."""
    gathered = [None] * dist.get_world_size(group)
    dist.all_gather_object(gathered, list(items), group=group)
    return dp_order_by_batch(gathered)


def dp_check_fingerprints(fingerprints: Sequence[Dict[str, Any]]) -> None:
    """fingerprints[r]: what rank r says of the graph, the folds and the sampling parameter it holds.  Every rank must hold the
    same: a RuntimeError names every field in which a rank differs from rank 0, with both values."""
    first = fingerprints[0]
    differing = []
    for r, other in enumerate(fingerprints[1:], start=1):
        for key in sorted(set(first) | set(other), key=str):
            if key not in first or key not in other or first[key] != other[key]:
                differing.append("%s (rank 0: %r, rank %d: %r)" % (key, first.get(key), r, other.get(key)))
    if differing:
        raise RuntimeError("data-parallel training on ONE graph needs the same graph, the same folds and the same sampling parameter "
                           "on every rank; the ranks differ in " + "; ".join(differing))


def dp_merge_epoch(metric_results: List[Dict[str, Any]], sums: Sequence[float], group=None) -> Tuple[List[Dict[str, Any]], List[float]]:
    """End of an epoch: every rank's per-batch metric dicts concatenated in rank order and the ranks' sums (loss * graphs, graphs,
    nodes, edges) added in rank order: the same list and the same totals on every rank."""
    world = dist.get_world_size(group)
    gathered = [None] * world
    dist.all_gather_object(gathered, (list(metric_results), [float(x) for x in sums]), group=group)
    merged = [m for part, _ in gathered for m in part]
    totals = [0.0] * len(sums)
    for _, part in gathered:
        for i, x in enumerate(part):
            totals[i] += x
    return merged, totals


class PackedGradientAllReducer:
    """The reduction of train(group=...): ONE launch writes scale * grad of every trainable variable into the flat buffer
    (relgnn_mt_pack_scaled_f32, one per 48 variables), ONE all-reduce(SUM) follows, every .grad becomes a view of its slice.
    The scale is this rank's share float32(w_r / sum_r w_r) of the step (dp_schedule), so the sum is the weighted mean:
    no weight slot, no divide.  A variable without a gradient, and every variable of a rank that holds no batch in this
    step (scale 0), contributes +0.0."""

    def __init__(self, params: Sequence[torch.nn.Parameter], group=None):
        import ctypes
        self.params = [p for p in params if p.requires_grad]
        self.group = group
        if not self.params or not all(p.is_cuda and p.dtype == torch.float32 for p in self.params):
            raise _lib.RelGnnLibraryError("PackedGradientAllReducer packs float32 variables on the GPU with a HIP kernel; "
                                          "there is no CPU fallback for this path")
        n = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(n, dtype=torch.float32, device=self.params[0].device)
        self.views, offs, off = [], [], 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            offs.append(off)
            off += p.numel()
        self._chunks = []                        # (first variable, count, sizes table, destination pointer)
        for c0 in range(0, len(self.params), _lib.MT_MAX):
            chunk = self.params[c0:c0 + _lib.MT_MAX]
            sizes = (ctypes.c_int64 * len(chunk))(*[p.numel() for p in chunk])
            self._chunks.append((c0, len(chunk), sizes, self.flat.data_ptr() + 4 * offs[c0]))
        self._ptr_table = ctypes.c_void_p * _lib.MT_MAX

    @property
    def nbytes(self) -> int:
        return self.flat.numel() * 4

    @torch.no_grad()
    def pack(self, scale: float) -> torch.Tensor:
        """flat <- scale * grads, on the current stream.  Returns the flat buffer."""
        scale = float(scale)
        keep = []                                # contiguous copies stay alive until their launch is enqueued
        for c0, n, sizes, dst in self._chunks:
            table = self._ptr_table()
            for j in range(n):
                g = self.params[c0 + j].grad
                if g is None:
                    continue                     # (NULL: +0.0 for the variable's length)
                if g.dtype != torch.float32 or not g.is_cuda:
                    raise ValueError("PackedGradientAllReducer: a %s gradient on %s" % (g.dtype, g.device))
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                table[j] = g.data_ptr()
            _lib.launch("relgnn_mt_pack_scaled_f32", table, sizes, n, scale, dst)
        return self.flat

    @torch.no_grad()
    def __call__(self, scale: float):
        """grad <- sum_r scale_r * grad_r, in place of every .grad (views of the flat buffer; nothing is unpacked)."""
        self.pack(scale)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        for p, v in zip(self.params, self.views):
            p.grad = v
