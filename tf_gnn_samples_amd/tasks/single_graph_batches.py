"""The sampled batches of a task whose data is ONE graph (the citation task): the bound device, the epoch and draw counters, what is
kept per graph and per fold on a device, and the four generators (TRAIN neighbour-sampled, TRAIN subgraph, evaluation, node
prediction).  The task's parsed parameters are read from the task at every use (restore_from_metadata replaces its params).

`sampled_batches` ({"fanouts": [k_1, ..., k_H], "seeds_per_batch": B, "seed": s}; absent or None by default, read
with params.get and kept in the checkpoint's metadata with the other task parameters): the TRAIN fold is no longer
one batch.  An epoch is a permutation of the fold's nodes cut into ceil(n_train / B) seed lists (neighbour_sampling
.epoch_seed_batches); every seed list becomes a fanout-limited subgraph drawn on the device (neighbour_sampling.NeighbourSampler,
csrc/neighbour_sample.hip) whose loss counts the seeds only.  The sampler, the full graph's RelGraph and the device copies of the
feature table, the labels and the fold's mask are built once per (fold, device).  The epochs and the sampled batches (the sampler's
`draw`) are counted here.  VALIDATION, TEST, test() and predict() stay on the full graph unless the key "evaluation" (below)
says otherwise.  GPU only; not together with capture_train_step, nor with a process group unless the key "data_parallel" says so.

The two together: `sampled_batches` takes one more optional key, "sparse_features": true, which requires sparse_node_features
(and sparse_node_features with a sampled_batches that lacks the key stays a ValueError).  The sampling state then keeps the device's
SparseRows instead of a dense table, and every sampled batch carries the [n, 1] stand-in plus SparseRows.take_rows(nodes): the CSR of
the batch's rows, the CSR of that subset's transpose (what the projection's weight gradient runs over) and both long-row plans,
built on the device per batch (csrc/sparse_subset.hip, include/relgnn_sparse_subset.h) with one read-back of eight sizes.  No
[V, F] or [n, F] dense array exists on the host or the device.  The weight gradient itself stays a dense [F, hidden] tensor, and the
optimizer walks all of it unless the next key says otherwise.

One more optional key, "sparse_update": true (requires "sparse_features": true, optimizer Adam and a model with the input projection
`graph_model/dense/kernel`; each is a ValueError when the task or the model is built): the optimizer registers the projection's weight
as row-deferred (TFStyleOptimizer.defer_rows, csrc/sparse_update.hip, include/relgnn_sparse_update.h).  A training step then reads and
writes only the rows of the weight and its two Adam slots whose words the batch holds, and every stored value is still dense Adam's,
bit for bit.  The dense gradient and the norm over it stay unless the next key says otherwise.

One more optional key, "sparse_gradient": true (requires "sparse_update": true, a ValueError otherwise): the projection's weight
gradient exists only as the [touched, hidden] rows whose words the batch holds (csrc/sparse_gradient.hip,
include/relgnn_sparse_gradient.h).  The weight's `.grad` stays None, no [F, hidden] tensor is allocated in a step, the clip norm is
computed over the touched rows with the bits of the dense norm, and the row update reads the compact rows: the optimizer still stores
dense Adam's values bit for bit.

One more optional key, "layered": true (it composes with the three above; none of them depends on the row order of a batch): a batch
is numbered by hop (NeighbourSampler.sample_by_hop: the seeds first, then the nodes first reached in hop 1, ...) and carries one
LevelGraph per layer under extra['layer_graphs'].  Layer l of H runs on the nodes at most H - l + 1 hops from a seed and on the edges
whose targets are at most H - l hops away, a prefix of every type's list, and its output is cut to those targets; the head, the loss
and the metrics see the seed rows only (labels and mask are taken for the seeds).  The model refuses the key unless it has as many
layers as there are fanouts and one timestep per layer (models/sparse_graph_model.py).  With a layer-input keep-probability below 1
the dropout masks differ from the un-layered run's (torch draws by shape, the fused route by element index over another row count):
the two runs are then two draws of the same model, not equal ones.

One more optional key, "evaluation": {"fanouts": [k_1, ..., k_H], "seeds_per_batch": B, "keep": bool} ("keep" optional; it composes with
the four above and does not ask training to be layered): VALIDATION, TEST and test() run over ceil(n_fold / B) batches instead of the
full graph.  Batch i holds the fold's masked nodes i * B .. (i + 1) * B - 1 in ascending id (no shuffle) and is
sample_by_hop(seeds, draw=i).device_batch(..., layered=True) with keep-probability 1, labels and mask of the seeds only, drawn by a
sampler of the fold's own whose replica is 0x40000000 | fold (neighbour_sampling.evaluation_replica): the random words are a function of
(seed, fold, batch index), the same in every epoch and never a training batch's.  The batches are always hop-ordered and layered, so the
model refuses the key unless it has as many layers as there are fanouts and one timestep per layer.  An epoch's loss is
sum(total_loss) / sum(num_masked), its accuracy sum(num_correct) / sum(num_masked), the early-stopping metric sum(total_loss) over the
fold's ONE graph (sampled_evaluation_epoch).  With every fanout 0 the seeds' states and logits are the full-graph forward's rows bit for
bit: every level graph brings its bucketing along and routes its hub buckets as the model's full-graph batch does (RelGraph.route_like).
"keep": the batches of a fold are built once and handed out again every epoch, released with the fold.  The three folds share ONE device
RelGraph and ONE feature table (graph_state, keyed by the adjacency and feature objects the folds share); labels, mask and sampler are
per fold.  predict(data, nodes=...) runs the same batches over the named nodes (the key's fanouts and B, or all-zero fanouts and 1024
without it); predict(data) without nodes stays on the full graph.

`subgraph_batches` ({"roots_per_batch": R, "walk_length": h, "seed": s, "sparse_features": bool}, the last two optional;
absent or None by default, read with params.get and kept in the checkpoint's metadata like its siblings; a ValueError together with
`sampled_batches`): the TRAIN fold is cut into subgraphs instead of receptive fields.  An epoch is the same permutation of the fold's
nodes cut into ceil(n_train / R) ROOT lists (epoch_seed_batches, unchanged); a walk of h steps against the edges starts at every root,
and the batch is the subgraph INDUCED on the visited nodes (subgraph_sampling.SubgraphSampler, csrc/subgraph_sample.hip): every edge
of the full graph between two of them, with the induced in-degrees.  Every layer runs on that one subgraph, so a step costs the same
at any depth.  The loss mask is fold_mask[nodes]: every TRAIN node of the subgraph counts, not only the roots.  "sparse_features": true
requires sparse_node_features (and the reverse), as for sampled_batches; the batch then carries SparseRows.take_rows(nodes).  The
device RelGraph and the feature table are the ones the folds share (graph_state).  VALIDATION, TEST, test() and predict() stay on
the full graph; predict(nodes=...) runs exact receptive fields as it does without the parameter.  Without the next key the loss and
the aggregation are the induced subgraph's.  GPU only; not together with capture_train_step, nor with a process group unless the key
"data_parallel" (below) says so.

One more optional key, "normalisation": {"presample_epochs": E, "aggregation": bool, "max_edge_weight": c} (the last two optional: true
and 1e4; it composes with "sparse_features"): GraphSAINT's normalisation (include/relgnn_subgraph_norm.h).  Before the first TRAIN
batch of a (fold, device) the sampler counts, over N = E * ceil(n_train / R) pre-sampled subgraphs (root lists of the epochs
0x80000000 + e, sampler replica 0x20000000: never a training batch's draws, and a pure function of (seed, E, the graph), so the counts
are recomputed after restore() and not stored), how many hold node v (C_v) and both ends of edge e (C_e), without a read-back.  The
loss term of node v then carries the weight N / max(C_v, 1) and the batch loss is divided by n_train instead of the batch's masked
count (relgnn_softmax_ce_weighted_stats / _bwd): its expectation is the fold's mean loss.  num_masked, num_correct and the accuracy
stay unweighted counts; total_loss is the weighted sum.  "aggregation": every message of a batch is scaled by
min(max(C_v, 1) / max(C_e, 1), c) / (full-graph in-degree + 1e-7) instead of 1 / (induced in-degree + 1e-7) (emitted with the edges,
preset as the batch graph's degree scale): a layer's sum is then an estimate of the aggregate evaluation computes on the full graph.
It needs a model whose layers take the degree table, normalise by it and sum (RGCN, RGDCN, GNN-FiLM with
normalize_messages_by_num_incoming; a ValueError from the model otherwise); "aggregation": false works with every model.

One more optional key, "sampler": "walk" | "node" | "edge" | "parts" (absent: "walk", and the parsed dict is the one it was; it composes
with "sparse_features", "data_parallel" and "normalisation"): who picks the node set of a batch.  The host lists an epoch's batches in
ONE place (subgraph_sampling.sampler_plan, built once per fold and parameter: subgraph_plan; subgraph_sampling.epoch_node_lists), which
the TRAIN generator, train_batch_weights, the pre-sampling and the data-parallel schedule read; the device work of a batch is
relgnn_neighbour_sample_begin or relgnn_subgraph_walk in front of the unchanged induced path.  "node" ({"roots_per_batch": R}, no
"walk_length"; ceil(n_train / R) batches): R targets of uniformly drawn by-target entries, nodes in proportion to their in-degree, made
distinct (SubgraphSampler.sample_nodes).  "edge" (the same keys and count): one walk step from each of R uniformly drawn roots
(SubgraphSampler(graph, 1).sample); over a graph stored in both directions a pair {u, v} is drawn in proportion to
1 / deg u + 1 / deg v, GraphSAINT's edge distribution.  "parts" ({"parts_path": a .npy holding int32 [V] with values 0 .. P - 1 and no
part empty, "parts_per_batch": q}, neither "roots_per_batch" nor "walk_length"; ceil(P / q) batches): a permutation of the parts cut
into runs of q, a batch the union of their nodes (Cluster-GCN's batches over a partition the user brings).
The file is read and validated when the plan is built (a ValueError that names it), the path travels in the checkpoint's metadata
and a CRC of the array joins the data-parallel fingerprint.  In place of "parts_path" (exactly one of the two) "parts" takes
"partition": {"num_parts": P, "imbalance_percent": b, "refine_rounds": T} (the last two optional: 10 and 8): the partition is COMPUTED
when the plan is built (computed_partition: graph_partition.partition_graph over the device RelGraph the folds share, seeded by this
parameter's "seed"; label propagation under the size cap ceil(V (100 + b) / (100 P)), its wish pass in HIP, csrc/graph_partition.hip),
brought to the host once and put through the file's validation.  The key travels in the checkpoint's metadata, never the array:
restore() and every rank of a data-parallel run compute the same partition again, and its CRC joins the fingerprint alike.  GPU only
(a ValueError from a model on the CPU).  The three graph-wide samplers REQUIRE "normalisation" (a ValueError
that names both keys): their batches are not anchored at TRAIN nodes, a batch may hold none, and only the loss divided by n_train is
defined for it (0, with zero gradients).  The pre-sampling runs the same plan for the epochs 0x80000000 + e
(SubgraphSampler.presample_lists), N = E * the epoch's batch count.

One more optional key of `sampled_batches`, "blocks": true (needs "layered": true or the "evaluation" key, a ValueError that names all
three otherwise; it composes with every other key; absent by default; `subgraph_batches` has no levels and does not take it): what
sampled GNN training calls blocks, or message-flow graphs.  A batch that is run level by level buckets ONLY its union graph (the
ordinary RelGraph constructor: the batch's two sorts); the arrays of every smaller level are derived from the union's on the device
in one launch sequence (csrc/level_plan.hip, csrc/level_plan.h, package-internal; neighbour_sampling.derived_level_graphs): the
by-target arrays of a level are a prefix of the union's, its by-source arrays the stable compaction of the union's entries whose
target is among the level's, and no level is sorted.  Every level's graph says which of its rows are targets (RelGraph.num_targets),
and the default RGCN route (ops.aggregate_then_transform) then gathers, multiplies and forms its weight gradient over those rows
only; every other layer function and route ignores the attribute, computes all rows of the level and is cut by the driver as before.
With "layered": true the TRAIN batches bring every level's derived graph and the model buckets nothing; with the "evaluation" key the
evaluation batches and predict(nodes=...) batches take derived levels in the place of H constructor calls, routed as before
(RelGraph.route_like), and "keep" then holds one col_t per batch (a level's is a view of the union's; its other arrays lie in one
arena).  The same arrays run through the same
kernels: GGNN, RGAT and GNN-FiLM give the bits they gave; RGCN gives the forward's bits, and weight gradients that differ by the
rounding of a sum over fewer rows.

Beside both stands the task parameter `layerwise_evaluation` ({"rows_per_batch": B, "keep": bool}; tasks/layerwise.py describes it):
the full-graph batch of a VALIDATION or TEST fold then carries a LayerwisePlan and the model computes it layer by layer over windows
of B target rows; "keep" keeps the windows' blocks in `kept_layerwise`, under the fold's label array.  A ValueError together with the
key "evaluation"; every other key of either parameter composes with it.

Both parameters take one more optional key, "data_parallel": true (a ValueError together with "sparse_update" / "sparse_gradient"; it
composes with every other key): train(group=...) and test(group=...) of a process group of W > 1 ranks are no longer refused
(models/data_parallel.py).  Every rank holds the whole graph; global batch j of a TRAIN epoch goes to rank
j mod W at step j // W with the draw index the single-GPU loop gives it (rank_train_batches), and a step's gradient is the weighted mean
of its batches' (train_batch_weights).  Under "evaluation" batch i of a fold goes to rank i mod W (rank_evaluation_batches); without it
every rank evaluates the full graph itself.  The task's two batch iterators and predict() stay refused under a process group.
"""
import weakref
import zlib
from typing import Any, NamedTuple

import numpy as np
import torch

from ..graph import RelGraph
from ..parallel import refuse_single_graph_task
from .graph_partition import partition_graph
from .neighbour_sampling import (PREDICT_FOLD, NeighbourSampler, epoch_seed_batches, evaluation_replica, evaluation_seed_batches)
from .sparse_features import SparseRows
from .sparse_graph_task import DataFold
from .subgraph_sampling import SubgraphSampler, epoch_node_lists, sampler_plan


class WeakKeyedCache:
    """Values under (anchor objects, extra key), each dropped when ANY of its anchors dies.  A hit needs the same anchor objects, not
    merely their ids: an id is handed out again once its object is gone."""

    def __init__(self):
        self._table = {}                          # (ids of the anchors, key) -> (weak references to the anchors, value)

    def get(self, anchors, key=None):
        held = self._table.get((tuple(map(id, anchors)), key))
        if held is not None and all(ref() is anchor for ref, anchor in zip(held[0], anchors)):
            return held[1]
        return None

    def put(self, anchors, key, value):
        at = (tuple(map(id, anchors)), key)
        drop = lambda _, at=at, table=self._table: table.pop(at, None)
        self._table[at] = ([weakref.ref(anchor, drop) for anchor in anchors], value)
        return value

    def values(self):
        return [value for _, value in self._table.values()]

    def clear(self):
        self._table.clear()

    def __len__(self):
        return len(self._table)


class GraphState(NamedTuple):
    """What the folds of one graph share on one device: ONE bucketing and ONE feature table (or device SparseRows)."""
    graph: RelGraph
    features: Any                                          # float32 [V, F], or the device's SparseRows


class FoldState(NamedTuple):
    """What the sampled batches of one fold on one device are cut from; `sampler.graph` and `features` are the GraphState's."""
    sampler: Any                                           # a NeighbourSampler, or the SubgraphSampler of `subgraph_batches`
    features: Any                                          # float32 [V, F], or the device's SparseRows
    labels: torch.Tensor                                   # int32 [V]
    mask: torch.Tensor                                     # float32 [V], the fold's
    visit_counts: Any = None                               # subgraph_sampling.VisitCounts under `subgraph_batches`' key "normalisation"


class SingleGraphBatches:
    """Everything a single-graph task keeps for sampling.  `task` gives the parsed parameters (sampled_batches, subgraph_batches,
    evaluation), its name, _out_keep and resident_rows; a fold has adjacency_lists, node_features, labels and mask."""

    def __init__(self, task):
        self.task = task
        self.device = None                        # where the model runs (bind)
        self.epoch = self.draw = 0                # TRAIN epochs started / batches sampled so far
        self.graph_states = WeakKeyedCache()      # (first adjacency array, features), device -> GraphState
        self.fold_states = WeakKeyedCache()       # (a fold's label array), (device, replica or "subgraph") -> FoldState
        self.kept_evaluation = WeakKeyedCache()   # (a fold's label array), (device, fold number, route, fanouts, B) -> its batches
        self.kept_layerwise = WeakKeyedCache()    # (a fold's label array), (device, B, route) -> the blocks of its windows (tasks/layerwise.py)
        self.sampler_plans = WeakKeyedCache()     # (a fold's label array), the parsed `subgraph_batches` -> its host SamplerPlan

    def bind(self, device) -> None:
        """The model tells the task where it runs (the NumPy iterator is not told otherwise).  The sampler is a HIP kernel and the
        package has no CPU fallback: a model on the CPU is refused."""
        device = torch.device(device)
        if device.type != "cuda" and "partition" in (self.task.subgraph_batches or {}):
            raise ValueError("subgraph_batches: partition is GPU only: the partitioner's wish pass is a HIP kernel and there is no CPU "
                             "fallback (the model is on %s)" % device)
        if device.type != "cuda":
            raise RuntimeError("sampled_batches needs a model on the GPU: the neighbour sampler is a HIP kernel and there is no CPU "
                               "fallback (the model is on %s)" % device)
        self.device = device

    def bound_device(self):
        if self.device is None:
            raise RuntimeError("sampled_batches: no device bound (Citation_Network_Task.bind_sampling_device); the model does that "
                               "when it asks for a fold's sampled batches")
        return self.device

    def graph_state(self, fold, device) -> GraphState:
        """The device RelGraph (validated once: it knows its hub buckets) and the device feature table of the graph `fold` belongs
        to, built once for all folds that share the adjacency and feature objects (_load_folds, load_synthetic) and released with them."""
        anchors, features = (fold.adjacency_lists[0], fold.node_features), fold.node_features
        held = self.graph_states.get(anchors, str(device))
        if held is not None:
            return held
        graph = RelGraph([_from_host(a.reshape(-1, 2), torch.int32, device) for a in fold.adjacency_lists], len(fold.labels))
        if isinstance(features, SparseRows):                      # the device's one copy of the container: no dense table anywhere
            table = self.task.resident_rows(features, device)
        else:
            table = _from_host(features, torch.float32, device)
        return self.graph_states.put(anchors, str(device), GraphState(graph, table))

    def fold_state(self, fold, device, key, make_sampler, fanouts=None, presample=None) -> FoldState:
        """The state of (fold, device, key), built once and released with the fold's arrays: make_sampler(the shared device RelGraph),
        the fold's labels and mask, presample(sampler) as its visit counts.  Built again when it was made for other fanouts."""
        held = self.fold_states.get((fold.labels,), (str(device), key))
        if held is not None and (fanouts is None or held.sampler.fanouts == list(fanouts)):
            return held
        shared = self.graph_state(fold, device)
        state = FoldState(make_sampler(shared.graph), shared.features, _from_host(fold.labels, torch.int32, device),
                          _from_host(fold.mask, torch.float32, device))
        if presample is not None:
            state = state._replace(visit_counts=presample(state.sampler))
        return self.fold_states.put((fold.labels,), (str(device), key), state)

    def neighbour_state(self, fold, device, fanouts=None, seed=None, replica: int = 0) -> FoldState:
        """The TRAIN fold's state by default (the parameter's fanouts and seed, replica 0); an evaluation fold names its own."""
        def sampler(graph):
            sampled = self.task.sampled_batches if fanouts is None else {"fanouts": fanouts, "seed": seed}
            return NeighbourSampler(graph, sampled["fanouts"], seed=sampled["seed"] or 0, replica=replica)
        return self.fold_state(fold, device, int(replica), sampler, fanouts)

    def subgraph_plan(self, fold):
        """The host plan of `subgraph_batches` over the TRAIN fold (subgraph_sampling.sampler_plan: the in-degrees of "node", the
        validated partition of "parts", read from its file or computed here under the key "partition"), built once per (fold,
        parameter): every reader of an epoch's lists asks here."""
        subgraph = self.task.subgraph_batches
        key = repr(sorted(subgraph.items()))
        held = self.sampler_plans.get((fold.labels,), key)
        if held is None:
            held = self.sampler_plans.put((fold.labels,), key, sampler_plan(subgraph, fold.mask, fold.adjacency_lists, len(fold.labels),
                                                                            partition=lambda: self.computed_partition(fold)))
        return held

    def computed_partition(self, fold) -> np.ndarray:
        """The partition of the key "partition", computed on the device RelGraph the folds share (graph_partition.partition_graph, with
        `subgraph_batches`' own seed) and brought to the host once: int32 [V].  A pure function of (the graph, the key, the seed): it
        is computed again after restore() and by every rank of a data-parallel run, and never stored."""
        subgraph = self.task.subgraph_batches
        asked = subgraph["partition"]
        graph = self.graph_state(fold, self.bound_device()).graph
        try:
            parts = partition_graph(graph, asked["num_parts"], subgraph["seed"], asked["imbalance_percent"], asked["refine_rounds"])
        except ValueError as error:
            raise ValueError("subgraph_batches: partition: %s" % error) from None
        return parts.cpu().numpy()

    def subgraph_state(self, fold, device) -> FoldState:
        """The TRAIN fold's SubgraphSampler over the device RelGraph the folds share, with the fold's labels and mask.  Its walk
        length is the parameter's for "walk", 1 for "edge" and 0 for the samplers that bring the node set themselves."""
        subgraph = self.task.subgraph_batches
        normalisation = subgraph.get("normalisation")
        plan = self.subgraph_plan(fold)
        # GraphSAINT's pre-sampling, before the first TRAIN batch of this state: a pure function of (seed, E, the graph), so it
        # is recomputed here after restore() and never stored in a checkpoint
        presample = None if normalisation is None else (
            lambda sampler: sampler.presample_lists(lambda epoch: epoch_node_lists(plan, epoch), normalisation["presample_epochs"],
                                                    plan.longest(), plan.walked))
        steps = subgraph["walk_length"] if plan.sampler == "walk" else plan.walk_steps
        return self.fold_state(fold, device, "subgraph", lambda graph: SubgraphSampler(graph, steps, seed=subgraph["seed"]),
                               presample=presample)

    # -------------------- TRAIN --------------------
    def train_batches(self, fold):
        """One TRAIN epoch of sampled batches, None when the TRAIN fold is one full-graph batch."""
        return self.rank_train_batches(fold, 0, 1)

    def rank_train_batches(self, fold, rank: int, world: int):
        """The batches of the TRAIN epoch that rank `rank` of `world` runs under the key "data_parallel": batch j of train_batches'
        list when j mod world == rank, each drawn with the draw index it has in that list.  The epoch and draw counters advance as
        train_batches advances them for the whole list, once the generator has run to its end."""
        if self.task.sampled_batches is not None:
            return self.neighbour_batches(fold, rank, world)
        if self.task.subgraph_batches is not None:
            return self.subgraph_batches(fold, rank, world)
        return None

    def train_batch_weights(self, fold):
        """What every batch of the NEXT TRAIN epoch weighs in the mean over a data-parallel step (parallel.single_graph_schedule): its
        seed count under `sampled_batches`, whose batch loss is the mean over the seeds; 1 under `subgraph_batches`, with or
        without "normalisation": a batch's loss is its own estimate of the fold's, and its count of TRAIN nodes is not on the host."""
        sampled, subgraph = self.task.sampled_batches, self.task.subgraph_batches
        if sampled is not None:
            return [float(len(seeds)) for seeds in epoch_seed_batches(fold.mask, sampled["seeds_per_batch"], sampled["seed"], self.epoch)]
        return [1.0] * self.subgraph_plan(fold).batches_per_epoch()

    def fingerprint(self, folds):
        """What every rank of a data-parallel run must hold alike (parallel.dp_check_fingerprints): the graph's size, the masked count
        of every fold in `folds` (name -> fold, "train" among them), a CRC of the TRAIN mask, the parsed sampling parameters and, under
        `subgraph_batches`' "sampler": "parts", a CRC of the partition array."""
        train = folds["train"]
        said = {"nodes": len(train.labels), "edges_per_type": [len(a) for a in train.adjacency_lists],
                "train_mask_crc": zlib.crc32(np.ascontiguousarray(train.mask).tobytes()),
                "sampled_batches": self.task.sampled_batches, "subgraph_batches": self.task.subgraph_batches}
        for name, fold in folds.items():
            said["%s_nodes" % name] = int(np.count_nonzero(fold.mask))
        if (self.task.subgraph_batches or {}).get("sampler") == "parts":          # (every rank reads the file, or computes the partition, itself)
            said["parts_crc"] = zlib.crc32(np.ascontiguousarray(self.subgraph_plan(train).parts).tobytes())
        return said

    def neighbour_batches(self, fold, rank: int = 0, world: int = 1):
        """ceil(n_train / B) sampled batches: one TRAIN epoch; of these, the ones dealt to `rank` of `world`."""
        sampled = self.task.sampled_batches
        state = self.neighbour_state(fold, self.bound_device())
        epoch, self.epoch = self.epoch, self.epoch + 1
        keep = self.task._out_keep(DataFold.TRAIN)
        for j, seeds in enumerate(epoch_seed_batches(fold.mask, sampled["seeds_per_batch"], sampled["seed"], epoch)):
            draw, self.draw = self.draw, self.draw + 1
            if j % world != rank:
                continue
            named_rows = sampled.get("sparse_gradient", False)
            if sampled.get("layered", False) and sampled.get("blocks", False):
                # every level's bucketing travels with the batch, derived from the union graph's: the model buckets nothing
                yield state.sampler.sample_by_hop(seeds, draw).device_batch(state.features, state.labels, state.mask, keep,
                                                                            named_rows=named_rows, derived=True)
                continue
            sample = state.sampler.sample_by_hop if sampled.get("layered", False) else state.sampler.sample
            yield sample(seeds, draw).device_batch(state.features, state.labels, state.mask, keep, named_rows=named_rows)

    def subgraph_batches(self, fold, rank: int = 0, world: int = 1):
        """The subgraph batches of one TRAIN epoch (subgraph_sampling.epoch_node_lists: ceil(n_train / R) of them, ceil(P / q) for
        "parts"); of these, the ones dealt to `rank` of `world`.  Under "walk" every train node is a root once; the loss mask is
        the fold's mask over ALL nodes of the subgraph (seed_mask is ones).  With the key "normalisation"
        every batch carries extra['loss_normalisation'] = (N / max(node_visits, 1) per node, n_train), and with its "aggregation" the
        per-edge weights as its graph's degree scale."""
        subgraph = self.task.subgraph_batches
        state = self.subgraph_state(fold, self.bound_device())
        epoch, self.epoch = self.epoch, self.epoch + 1
        keep = self.task._out_keep(DataFold.TRAIN)
        normalisation, counts = subgraph.get("normalisation"), state.visit_counts
        weighting = (counts, normalisation["max_edge_weight"]) if normalisation is not None and normalisation["aggregation"] else None
        num_train = float(np.count_nonzero(fold.mask))
        plan = self.subgraph_plan(fold)
        for j, ids in enumerate(epoch_node_lists(plan, epoch)):
            draw, self.draw = self.draw, self.draw + 1
            if j % world != rank:
                continue
            if normalisation is None:                 # ("walk" alone: the other samplers require the key)
                yield state.sampler.sample(ids, draw).device_batch(state.features, state.labels, state.mask, keep)
                continue
            sub = state.sampler.sample(ids, draw, weighting) if plan.walked else state.sampler.sample_nodes(ids, weighting)
            batch = sub.device_batch(state.features, state.labels, state.mask, keep)
            batch.extra['loss_normalisation'] = (counts.node_weights(sub.nodes), num_train)
            yield batch

    # -------------------- Evaluation and predictions on sampled receptive fields --------------------
    def evaluation_batch(self, state: FoldState, seeds: np.ndarray, draw: int, full_graph_route: bool):
        """Batch `draw` of a fold: hop-ordered and layered, keep-probability 1, labels and mask of the seeds only, every level with its
        bucketing.  full_graph_route: the levels route their reductions as the device's full graph does (RelGraph.route_like), which
        is what a resident full-graph batch of the same fold does (tasks/resident.py splits a fold's hubs per batch); otherwise
        every bucket keeps one wave, as the full graph bucketed by the model itself does (validate="deferred")."""
        sub = state.sampler.sample_by_hop(seeds, draw)
        blocks = (self.task.sampled_batches or {}).get("blocks", False)       # (needs the "evaluation" key here: predict(nodes=...)
        #                                                                        without it stays on H constructor calls)
        return sub.device_batch(state.features, state.labels, state.mask, 1.0, layered=True, bucketed=True,
                                route_like=state.sampler.graph if full_graph_route else None,
                                derived=bool(blocks and self.task.evaluation is not None))

    def evaluation_batches(self, data, data_fold: DataFold, full_graph_route: bool):
        """ceil(n_fold / B) batches: one VALIDATION or TEST epoch under the "evaluation" key.  Batch i holds the fold's masked nodes
        i * B .. (i + 1) * B - 1 in ascending id and is drawn with draw = i by the fold's own sampler, whose replica is
        neighbour_sampling.evaluation_replica(fold): the same subgraphs in every epoch.  "keep": built once per (fold, device, route, fanouts, B),
        handed out again, released with the fold."""
        refuse_single_graph_task(self.task.name())
        yield from self.rank_evaluation_batches(data, data_fold, full_graph_route, 0, 1)

    def rank_evaluation_batches(self, data, data_fold: DataFold, full_graph_route: bool, rank: int, world: int):
        """The batches of evaluation_batches' list that rank `rank` of `world` runs under the key "data_parallel": batch i when
        i mod world == rank, drawn as it is there.  "keep" keeps the rank's own batches."""
        evaluation, device = self.task.evaluation, self.bound_device()
        fold = next(iter(data))
        key = (str(device), data_fold.value, bool(full_graph_route), tuple(evaluation["fanouts"]), evaluation["seeds_per_batch"],
               int(rank), int(world), bool(self.task.sampled_batches.get("blocks", False)))
        if evaluation.get("keep", False):
            held = self.kept_evaluation.get((fold.labels,), key)
            if held is not None:
                yield from held
                return
        state = self.neighbour_state(fold, device, evaluation["fanouts"], self.task.sampled_batches["seed"],
                                     evaluation_replica(data_fold.value))
        kept = []
        for draw, seeds in enumerate(evaluation_seed_batches(fold.mask, evaluation["seeds_per_batch"])):
            if draw % world != rank:
                continue
            batch = self.evaluation_batch(state, seeds, draw, full_graph_route)
            if evaluation.get("keep", False):
                kept.append(batch)
            yield batch
        if evaluation.get("keep", False):         # (only a whole epoch is kept: an abandoned iterator keeps nothing)
            self.kept_evaluation.put((fold.labels,), key, kept)

    def node_prediction_batches(self, data, distinct_nodes: np.ndarray, fanouts, seeds_per_batch: int, full_graph_route: bool):
        """The batches of predict(nodes=...): the distinct ids ascending in runs of seeds_per_batch, batch i drawn with draw = i by a
        sampler of replica evaluation_replica(PREDICT_FOLD); each batch carries its host seed list under extra['prediction_seeds']."""
        refuse_single_graph_task(self.task.name())
        device = self.bound_device()
        fold = next(iter(data))
        sampled = self.task.sampled_batches
        state = self.neighbour_state(fold, device, list(fanouts), sampled["seed"] if sampled is not None else 0,
                                     evaluation_replica(PREDICT_FOLD))
        for draw, at in enumerate(range(0, len(distinct_nodes), seeds_per_batch)):
            seeds = np.ascontiguousarray(distinct_nodes[at:at + seeds_per_batch], dtype=np.int32)
            batch = self.evaluation_batch(state, seeds, draw, full_graph_route)
            batch.extra['prediction_seeds'] = seeds
            yield batch


def _from_host(array, dtype, device) -> torch.Tensor:
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(device)
