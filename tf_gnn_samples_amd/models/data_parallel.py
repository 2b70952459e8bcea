"""Data parallelism: the epochs of Sparse_Graph_Model.train(group=...) / test(group=...) on one rank of W, by graph (_DataParallel)
or, for a task whose data is ONE graph cut into sampled batches, by batch (_SingleGraphDataParallel)."""
import torch
import torch.distributed as dist

from .. import config
from ..dense import weights_changed
from ..parallel import (PackedGradientAllReducer, dp_check_fingerprints, dp_device_seed, dp_epoch_rng, dp_exchange_plans,
                        dp_gather_by_batch, dp_merge_epoch, dp_plan_epoch, dp_schedule, dp_shard)
from ..tasks import DataFold
from .readback import EpochTally, LateFetch, MetricsReadback


def data_parallel(model, group):
    """None for the single-GPU loop (no group, or a group of one rank: nothing below runs, no collective is issued); otherwise
    the driver of data-parallel epochs, after the refusals."""
    if group is None:
        return None
    world = dist.get_world_size(group)
    if world == 1:
        return None
    single_graph = model.task.single_graph_data_parallel()      # (the citation task's key "data_parallel": batches, not graphs, are dealt out)
    if not single_graph:
        model.task.loss_weight(1, 1)   # a task that cannot be split by graph (citation), or does not say how its loss is normalised, raises
    if model.device.type != "cuda":
        raise RuntimeError("train(group=...) / test(group=...) need the model on the GPU (one process per GPU; the gradient pack is a "
                           "HIP kernel): this model is on %s" % model.device)
    if not model.params.get('native_batching', True) or not hasattr(model.task, "make_graph_store"):
        raise RuntimeError("data-parallel training uses the native input pipelines only: %s"
                           % ("native_batching is false" if not model.params.get('native_batching', True)
                              else "the %s task has no make_graph_store" % type(model.task).__name__))
    if config.settings.allreduce == "overlap":
        raise RuntimeError("allreduce=overlap: the bucketed all-reduce (OverlappedGradientAllReducer) is not wired into train(); "
                           "train(group=...) runs the flat packed form only and does not fall back to it silently: set allreduce=flat")
    return (_SingleGraphDataParallel if single_graph else _DataParallel)(model, group, world)


class _Ranks:
    """What both drivers share: the rank, who logs, and the start of training."""

    def __init__(self, model, group, world: int):
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
        dist.barrier(group=self.group)

    def begin_training(self):
        """Rank 0's parameters, optimizer slots and step count everywhere (a restore()d model on rank 0 included); then torch's
        generator of this device reseeded from (random_seed, rank): the torch dropout route must not share masks across ranks (the
        fused route's state block already carries the rank as its replica)."""
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

    def zero_contribution_step(self, lr_num_graphs: int):
        """A step this rank has no batch for: zeros into the step's collective, the same clip and update as everyone else
        (parameters, optimizer slots and the step count stay identical across the ranks)."""
        self.model.optimizer.zero_grad()
        self.reducer(0.0)
        self.model.optimizer.clip_and_step(self.model._lr_scale(lr_num_graphs))


class _DataParallel(_Ranks):
    """Epochs of Sparse_Graph_Model.train(group=...) / test(group=...) on one rank of W (parallel.py has the host-side pieces;
    DESIGN.md section 8 the protocol).

    The shard of a fold is fixed for the run (parallel.dp_shard); the rank's pipeline is built over its shard only.  Per epoch and
    fold: shuffle (training; parallel.dp_epoch_rng), plan the local batches, exchange the plans (one all-gather, one host read).
    A training epoch then runs max_r(batches_r) steps on EVERY rank.  With a batch: train_step whose grad_hook is the packed
    reducer with this rank's scale and whose learning rate goes by the step's global graph count.  Without one: zeros into the
    same collective, the same clip and update.  Evaluation epochs run the local batches without a gradient collective.  At the
    end of every epoch the per-batch metrics and the counters are gathered in rank order."""

    def _pipeline(self, data):
        """(the rank's input pipeline over its shard of `data`, or None for an empty shard; the largest shard's graph count)."""
        model = self.model
        folds = model.__dict__.setdefault("_dp_folds", {})
        key = (id(data), len(data), self.world, self.rank)
        kept = folds.get(key)
        if kept is None or kept[0] is not data:
            shards = dp_shard(data, self.world)
            kept = folds[key] = (data, [data[i] for i in shards[self.rank]], max(len(s) for s in shards))
            while len(folds) > 3:      # train + validation folds and one more, like the pipelines themselves
                folds.pop(next(iter(folds)))
        _, mine, largest = kept
        return (model._native_pipeline(mine) if mine else None), largest

    def run_epoch(self, epoch_name: str, data, data_fold: DataFold, quiet: bool = False):
        """_run_epoch across the group: the same six results on every rank, over the whole fold."""
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
        tally = EpochTally(epoch_name, quiet or self.rank != 0, where=" on rank 0")
        late = LateFetch(tally.fetch)
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
                upcoming = next(batch_iterator, None)      # (the order of readback.LateFetch: metrics are read one step late)
                late.put((readback, batch))
            else:
                self.zero_contribution_step(int(schedule.graph_sums[k]))      # no batch left on this rank
        if upcoming is not None:
            raise RuntimeError("%s: the input pipeline holds more batches than planned" % epoch_name)
        late.flush()
        return tally.result(*dp_merge_epoch(tally.results, tally.totals(), self.group))


class _SingleGraphDataParallel(_Ranks):
    """Epochs of train(group=...) / test(group=...) on one rank of W for a task whose data is ONE graph cut into sampled batches (the
    citation task with the key "data_parallel").

    Every rank holds the whole graph, the folds and the same task parameters, which begin_training() checks with one all-gather of a
    fingerprint.  A TRAIN epoch is the single-GPU epoch's list of batches, W at a time (parallel.single_graph_schedule): global
    batch j runs on rank j mod W at step j // W with the draw index it has on one GPU, its gradient scaled by its share of the
    step's weight in the packed reducer; a rank without a batch in the last step sends zeros.  There is one graph, so the learning
    rate goes by a graph count of 1.  An evaluation epoch deals the fold's batches out the same way under the key "evaluation", and
    is the full graph on every rank, without a collective, otherwise.  What the ranks report of their batches is gathered and put
    in the order of the global batch index BEFORE anything is summed: every rank's epoch is, number for number, what a single
    process makes of the same per-batch values."""

    def begin_training(self):
        said = [None] * self.world
        self.model.task.bind_sampling_device(self.model.device)     # (a computed partition's CRC is of what this device computes)
        dist.all_gather_object(said, self.model.task.data_parallel_fingerprint(), group=self.group)
        dp_check_fingerprints(said)
        super().begin_training()

    def run_epoch(self, epoch_name: str, data, data_fold: DataFold, quiet: bool = False):
        """_run_epoch across the group: the same six results on every rank, over the whole fold."""
        model, task = self.model, self.model.task
        train = data_fold == DataFold.TRAIN
        if train and self.reducer is None:
            raise RuntimeError("a data-parallel training epoch outside train(group=...)")
        native = model._native_batching()
        schedule = task.train_schedule(data, self.world) if train else None
        batches, dealt = task.rank_epoch_batches(data, data_fold, model.device, model._full_graph_route(native), self.rank, self.world,
                                                 lambda: model._native_pipeline(data))
        batch_iterator = iter(batches)
        tally = EpochTally(epoch_name, quiet or self.rank != 0, where=" on rank 0")
        sizes = []                                 # (nodes, edges) of every batch this rank ran, beside tally.results
        late = LateFetch(tally.fetch)
        upcoming = next(batch_iterator, None)
        step = 0
        while upcoming is not None:
            batch = upcoming
            if train:
                scale = float(schedule.scales[self.rank, step])
                m = model.train_step(batch, grad_hook=lambda params, s=scale: self.reducer(s), lr_num_graphs=1)
            else:
                with torch.no_grad():
                    m = model.forward_batch(batch, training=False)
            readback = MetricsReadback(m)
            upcoming = next(batch_iterator, None)      # (the order of readback.LateFetch: metrics are read one step late)
            late.put((readback, batch))
            sizes.append((batch.num_nodes, batch.num_edges))
            step += 1
        if train:
            scheduled = int((schedule.owner == self.rank).sum())
            if step != scheduled:
                raise RuntimeError("%s: the sampler dealt this rank %d batches, the schedule %d" % (epoch_name, step, scheduled))
            for _ in range(step, schedule.steps):
                self.zero_contribution_step(1)     # no batch for this rank in the last step
        late.flush()
        if not dealt:                              # the full graph, on every rank alike: nothing to merge
            return task.epoch_result(tally.result(), data_fold)
        merged = dp_gather_by_batch(list(zip(tally.results, sizes)), self.group)
        totals = [0.0, 0, 0, 0]                    # as EpochTally.fetch adds them up, batch by batch: every batch is the ONE graph
        for m, (nodes, edges) in merged:
            totals[0] += m['loss']
            totals[1] += 1
            totals[2] += nodes
            totals[3] += edges
        return task.epoch_result(tally.result([m for m, _ in merged], totals), data_fold)
