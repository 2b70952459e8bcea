"""Subgraph mini-batches of ONE graph (csrc/subgraph_sample.hip, include/relgnn_subgraph.h): a node set found by random walks from a
root list, against the edges of the by-target bucketing the full graph's RelGraph already holds, and the node-induced subgraph over
it as a SampledSubgraph.  Every layer of a model runs on that one subgraph, so a batch costs the same at any depth; a neighbour-sampled
batch (tasks/neighbour_sampling.py) grows with every hop instead.

Host round trips of SubgraphSampler.sample() and induced_subgraph(): the root (node) list is validated on the host (in range,
distinct; one small copy of a device list), and the subgraph's sizes — n, the per-type edge counts and their total — are read back
ONCE, because its tensors are sized by them.  The buffers in front of that read-back are sized from the bound min(V, R * (h + 1)).
The stamp array, its compaction and the guard that leaves it zero are StampedNodeSet's (tasks/neighbour_sampling.py), shared with NeighbourSampler.

GraphSAINT normalisation (include/relgnn_subgraph_norm.h; the key "normalisation" of the citation task's `subgraph_batches`):
SubgraphSampler.presample() counts over pre-sampled subgraphs how often every node and every by-target entry is held (VisitCounts; no
read-back at all), and sample(..., weighting=(counts, cap)) emits the per-edge aggregation weights with the batch's edges.

Who picks the node set (the key "sampler" of `subgraph_batches`: "walk" | "node" | "edge" | "parts") is a host rule in front of that
path: sampler_plan() and epoch_node_lists() list an epoch's batches for all four, SubgraphSampler.sample() walks a root list ("walk",
and "edge" with walk length 1), SubgraphSampler.sample_nodes() takes a node set as it is ("node", "parts"), and presample_lists()
pre-samples over any plan.  No kernel and no entry point belongs to a sampler.
"""
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..graph import RelGraph
from .graph_partition import parse_partition
from .neighbour_sampling import (SampledSubgraph, StampedNodeSet, epoch_seed_batches, integer_at_least, parse_bool_keys, unknown_keys,
                                  validated_ids)

# relgnn_subgraph_max_walk_length (the library is not loaded to validate a parameter; tests/test_gpu_subgraph_batches.py holds the
# two against each other)
MAX_WALK_LENGTH = 64


def check_walk_length(walk_length) -> int:
    """The walk length as a python int, or a ValueError that says what include/relgnn_subgraph.h supports."""
    if isinstance(walk_length, bool) or not isinstance(walk_length, (int, np.integer)) or not 0 <= walk_length <= MAX_WALK_LENGTH:
        raise ValueError("walk_length must be an integer in [0, %d] (0: the subgraph induced on the roots alone), got %r"
                         % (MAX_WALK_LENGTH, walk_length))
    return int(walk_length)


class _Extractor(StampedNodeSet):
    """The induced-edge path over one RelGraph and its stamp array (StampedNodeSet; `trace`: scripts/bench_subgraph_batches.py)."""

    def __init__(self, graph: RelGraph, what: str):
        def refuse_unsupported(lib):
            if not lib.relgnn_subgraph_supported(1, 0, graph.V, graph.L):
                raise ValueError("%s does not support a graph of %d nodes and %d edge types (relgnn_subgraph_supported)" % (what, graph.V, graph.L))
        super().__init__(graph, what, refuse_unsupported)

    def _node_list(self, nodes_buf: torch.Tensor, B: int, count: torch.Tensor) -> None:
        """The stamped set ascending in nodes_buf[:count] (at most B; `count` stays on the device), every listed stamp now position + 1."""
        self.compact(0, nodes_buf, B, count)
        _lib.launch("relgnn_subgraph_number", _lib.ptr(nodes_buf), _lib.ptr(count), B, _lib.ptr(self.stamp), self.graph.V)

    def _induced(self, stamp_the_set, B: int, weighting=None) -> SampledSubgraph:
        """stamp_the_set() enqueues what stamps the node set (at most B nodes); everything behind it is the same.  Runs under _guarded.
        weighting = (VisitCounts, max_edge_weight): the emit also writes GraphSAINT's per-edge weights (message_weights)."""
        lib, g = _lib.load_library(), self.graph
        V, L, dev = g.V, g.L, g.device
        i32 = lambda n: torch.empty(int(n), dtype=torch.int32, device=dev)
        self._mark("start")
        stamp_the_set()
        self._mark("walks")
        summary = torch.zeros(L + 2, dtype=torch.int32, device=dev)       # [edges per type | edge total | n]: read back once
        nodes_buf = i32(B)
        self._node_list(nodes_buf, B, summary[L + 1:])
        self._mark("node_list")
        counts, offsets = i32(B * L + 1), i32(B * L + 1)
        scan_bytes = lib.relgnn_subgraph_workspace_bytes(B * L + 1)
        scan_ws = _lib.scratch(scan_bytes, dev)
        _lib.launch("relgnn_subgraph_induced_count", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), V, L, _lib.ptr(nodes_buf),
                    _lib.ptr(summary[L + 1:]), B, _lib.ptr(self.stamp), _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(summary[:L + 1]),
                    _lib.ptr(scan_ws), scan_bytes)
        self._mark("induced_count")
        sizes = summary.tolist()                                  # the one read-back of a call
        self._mark("readback")
        type_edges, total, n = sizes[:L], sizes[L], sizes[L + 1]
        nodes = nodes_buf[:n]
        edges = torch.empty((total, 2), dtype=torch.int32, device=dev)
        degrees = torch.empty((L, n), dtype=torch.float32, device=dev)
        message_weights = None
        if weighting is None:
            _lib.launch("relgnn_subgraph_induced_emit", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), V, L, _lib.ptr(nodes_buf), n, B,
                        _lib.ptr(self.stamp), _lib.ptr(offsets), total, _lib.ptr(edges) if total else None, _lib.ptr(degrees))
        else:                                                     # the same edges and degrees, and the per-edge weights in their order
            counts_of, cap = weighting
            message_weights = torch.empty(total, dtype=torch.float32, device=dev)
            _lib.launch("relgnn_subgraph_induced_emit_weighted", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), V, L, g.M, _lib.ptr(nodes_buf),
                        n, B, _lib.ptr(self.stamp), _lib.ptr(offsets), _lib.ptr(counts_of.node_visits),
                        _lib.ptr(counts_of.edge_visits) if g.M else None, float(cap), total, _lib.ptr(edges) if total else None,
                        _lib.ptr(degrees), _lib.ptr(message_weights) if total else None)
        _lib.launch("relgnn_subgraph_clear", _lib.ptr(nodes_buf), n, _lib.ptr(self.stamp), V)
        self._mark("induced_emit")
        adjacency = list(edges.split(type_edges))                 # the types' lists lie one behind the other: views, no copy
        seed_mask = torch.ones(n, dtype=torch.float32, device=dev)        # every node of the subgraph may count in the loss
        return SampledSubgraph(nodes, adjacency, degrees, seed_mask, n, total, message_weights)


class VisitCounts(NamedTuple):
    """How often the pre-sampled subgraphs hold a node and a by-target entry (include/relgnn_subgraph_norm.h): GraphSAINT's C_v and
    C_{u,v} for a node-induced sampler.  On the device; a pure function of (seed, E, R, h, the fold, the graph)."""
    node_visits: torch.Tensor                   # int32 [V]
    edge_visits: torch.Tensor                   # int32 [M], aligned with RelGraph.col_t
    num_subgraphs: int                          # N = E * ceil(n_fold / R)

    def node_weights(self, nodes: torch.Tensor) -> torch.Tensor:
        """The loss weight of every node of a batch: (float)N / (float)max(node_visits[v], 1), float32 [n]."""
        visits = self.node_visits.index_select(0, nodes.long()).clamp_(min=1).to(torch.float32)
        return torch.full_like(visits, float(self.num_subgraphs)) / visits


# the walks of the pre-sampled subgraphs: never a training batch's draws (replica 0) nor an evaluation batch's (0x40000000 | fold)
PRESAMPLE_REPLICA = 0x20000000
PRESAMPLE_EPOCH = 0x80000000                    # the root lists of pre-sampling epoch e are epoch_seed_batches' of epoch 0x80000000 + e


class SubgraphSampler(_Extractor):
    """Random-walk subgraph sampler over one RelGraph (its rowptr_t / col_t are read in place).  Holds the [V] int32 stamp array, all
    zero between calls (and after a call that raised)."""

    def __init__(self, graph: RelGraph, walk_length: int, seed: int = 0, replica: int = 0):
        self.walk_length = check_walk_length(walk_length)
        if not 0 <= int(replica) < 2 ** 31:
            raise ValueError("replica must be in [0, 2^31), got %r" % (replica,))
        super().__init__(graph, "subgraph sampling")
        self.seed, self.replica = int(seed) & 0xffffffff, int(replica)

    def sample(self, roots, draw: int, weighting=None) -> SampledSubgraph:
        """roots: int32 device tensor (a host array is uploaded), distinct node ids, one walk each; draw: the count of sampled batches
        so far.  -> the subgraph induced on the nodes the walks visit, seed_mask all ones.  weighting = (VisitCounts of presample(),
        max_edge_weight): the subgraph also carries GraphSAINT's per-edge weights, message_weights float32 [num_edges] in the order of
        the lists; the lists and the degrees are the unweighted call's."""
        g = self.graph
        roots = validated_ids(roots, g.V, g.device, "root")
        R, draw = int(roots.numel()), int(draw) & 0xffffffff

        def walks():
            _lib.launch("relgnn_subgraph_walk", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), g.V, g.L, _lib.ptr(roots), R, self.walk_length,
                        draw, self.seed, self.replica, _lib.ptr(self.stamp))
        return self._guarded(self._induced, walks, min(g.V, R * (self.walk_length + 1)), weighting)

    def sample_nodes(self, nodes, weighting=None) -> SampledSubgraph:
        """The subgraph induced on a node set the caller brings (the task's node and partition samplers): int32 ids, distinct, any
        order.  induced_subgraph's path on THIS sampler's stamp array and inside its guard, so that `weighting` applies as in sample()."""
        g = self.graph
        nodes = validated_ids(nodes, g.V, g.device, "node")
        return self._guarded(self._induced, lambda: self.begin(nodes), int(nodes.numel()), weighting)

    def presample(self, fold_mask, roots_per_batch: int, epochs: int) -> VisitCounts:
        """GraphSAINT's pre-sampling: E = `epochs` epochs of root lists, epoch_seed_batches(fold_mask, R, seed, 0x80000000 + e), every
        list walked with the reserved replica 0x20000000 and draw = the running index of the pre-sampled subgraph, and counted
        (relgnn_subgraph_visit_count).  Per subgraph: walk, compact, number, count, a reset of the stamps; NOTHING is read back, the
        set's size stays on the device and the buffers are sized from the bound min(V, R * (h + 1))."""
        R, epochs = int(roots_per_batch), int(epochs)
        if R < 1 or epochs < 1:
            raise ValueError("presample: roots_per_batch and epochs must be positive, got %r and %r" % (roots_per_batch, epochs))
        return self.presample_lists(lambda epoch: epoch_seed_batches(fold_mask, R, self.seed, epoch), epochs, R, walked=True)

    def presample_lists(self, epoch_lists, epochs: int, longest: int, walked: bool) -> VisitCounts:
        """presample() over the lists of any plan: epoch_lists(0x80000000 + e) gives pre-sampling epoch e's lists (in range, distinct,
        ascending; none longer than `longest`).  walked: every list is a root list and is walked as presample() walks it; otherwise it
        IS the node set and is stamped by `begin`.  Counted alike, with no read-back."""
        lib, g = _lib.load_library(), self.graph
        V, L, dev = g.V, g.L, g.device
        steps = self.walk_length if walked else 0
        if not lib.relgnn_subgraph_supported(int(longest), steps, V, L):
            raise ValueError("presample: %d walks of %d steps are not supported (relgnn_subgraph_supported)" % (longest, steps))
        B = min(V, int(longest) * (steps + 1))
        counts = VisitCounts(torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(g.M, dtype=torch.int32, device=dev), 0)

        def count_visits():
            nodes_buf = torch.empty(B, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            drawn = 0
            for e in range(int(epochs)):
                for ids in epoch_lists(PRESAMPLE_EPOCH + e):
                    if len(ids) > longest:
                        raise ValueError("presample: a list of %d ids, longer than the %d its buffers were sized for" % (len(ids), longest))
                    ids = torch.as_tensor(ids, device=dev)
                    if walked:
                        _lib.launch("relgnn_subgraph_walk", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), V, L, _lib.ptr(ids), ids.numel(),
                                    self.walk_length, drawn & 0xffffffff, self.seed, PRESAMPLE_REPLICA, _lib.ptr(self.stamp))
                    else:
                        self.begin(ids)
                    self._node_list(nodes_buf, B, count)
                    _lib.launch("relgnn_subgraph_visit_count", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t) if g.M else None, V, L, g.M,
                                _lib.ptr(nodes_buf), _lib.ptr(count), B, _lib.ptr(self.stamp), _lib.ptr(counts.node_visits),
                                _lib.ptr(counts.edge_visits) if g.M else None)
                    self.stamp.zero_()                            # (the set's size never reaches the host: the whole array)
                    drawn += 1
            return drawn
        return counts._replace(num_subgraphs=self._guarded(count_visits))


def induced_subgraph(graph: RelGraph, nodes) -> SampledSubgraph:
    """The subgraph of `graph` induced on a node set the caller brings (a partition, say): int32 ids, distinct, any order.  The
    induced-edge path of SubgraphSampler.sample without the walks; one read-back."""
    extractor = _Extractor(graph, "induced_subgraph")
    nodes = validated_ids(nodes, graph.V, graph.device, "node")
    return extractor._guarded(extractor._induced, lambda: extractor.begin(nodes), int(nodes.numel()))


def parse_normalisation(value) -> Dict:
    """The key "normalisation" of `subgraph_batches` as {"presample_epochs": int >= 1, "aggregation": bool, "max_edge_weight": float > 0}
    (the last two optional: true and 1e4, GraphSAINT's own clip), or a ValueError that names the key."""
    what = "subgraph_batches: normalisation"
    known = ("presample_epochs", "aggregation", "max_edge_weight")
    if not isinstance(value, dict):
        raise ValueError('%s must be {"presample_epochs": E, "aggregation": bool, "max_edge_weight": c}, the last two optional, got %r'
                         % (what, value))
    unknown = unknown_keys(value, known)
    if unknown:
        raise ValueError("%s: unknown key %s (known: %s)" % (what, ", ".join(repr(k) for k in unknown), ", ".join(known)))
    if "presample_epochs" not in value:
        raise ValueError("%s: presample_epochs is required" % what)
    epochs = integer_at_least(value["presample_epochs"], 1, what + ": presample_epochs must be an integer >= 1, got %r")
    aggregation = value.get("aggregation", True)
    if not isinstance(aggregation, bool):
        raise ValueError("%s: aggregation must be true or false, got %r" % (what, aggregation))
    cap = value.get("max_edge_weight", 1e4)
    if isinstance(cap, bool) or not isinstance(cap, (int, float, np.integer, np.floating)) or not 0 < float(cap) < float("inf"):
        raise ValueError("%s: max_edge_weight must be a finite number > 0, got %r" % (what, cap))
    return {"presample_epochs": epochs, "aggregation": aggregation, "max_edge_weight": float(cap)}


# who picks the node set of a batch (the key "sampler" of `subgraph_batches`): the keys each requires and the keys each refuses
SAMPLERS = ("walk", "node", "edge", "parts")
_REQUIRED = {"walk": ("roots_per_batch", "walk_length"), "node": ("roots_per_batch",), "edge": ("roots_per_batch",),
             "parts": ("parts_path", "parts_per_batch")}
_REFUSED = {"walk": ("parts_path", "partition", "parts_per_batch"), "node": ("walk_length", "parts_path", "partition", "parts_per_batch"),
            "edge": ("walk_length", "parts_path", "partition", "parts_per_batch"), "parts": ("roots_per_batch", "walk_length")}


def parse_subgraph_batches(value) -> Optional[Dict]:
    """The task parameter `subgraph_batches` as {"roots_per_batch": int, "walk_length": int, "seed": int}, None when it is absent;
    the optional keys "sparse_features" (a bool: the batches take their feature rows from a SparseRows), "data_parallel" (a bool:
    train(group=...) hands the batches of an epoch out to the ranks), "normalisation" (parse_normalisation: GraphSAINT's loss and
    aggregation weights) and "sampler" (one of SAMPLERS; absent: "walk") are carried only when given.  "node" and "edge" take
    "roots_per_batch" (R draws per batch) and no "walk_length"; "parts" takes "parts_path" (a .npy, int32 [V], read when the TRAIN
    state is built) and "parts_per_batch" in their place, or "partition" (graph_partition.parse_partition: the partition is computed on
    the device when the TRAIN state is built, from this dict's "seed") in place of "parts_path", exactly one of the two; all three
    require "normalisation": their batches are not anchored at TRAIN nodes, and only the loss divided by n_train is defined for a
    batch that holds none."""
    if value is None:
        return None
    known = {"roots_per_batch", "walk_length", "seed", "sparse_features", "data_parallel", "normalisation", "sampler", "parts_path",
             "partition", "parts_per_batch"}
    unknown = unknown_keys(value, known)
    sampler = value.get("sampler", "walk") if isinstance(value, dict) else "walk"
    if not isinstance(value, dict) or unknown or (sampler == "walk" and not set(_REQUIRED["walk"]) <= set(value)):
        said = "; unknown key %s" % ", ".join(repr(k) for k in unknown) if unknown else ""
        raise ValueError('subgraph_batches must be {"roots_per_batch": R, "walk_length": h, "seed": s, "sparse_features": bool, '
                         '"data_parallel": bool, "normalisation": {...}, "sampler": "walk" | "node" | "edge" | "parts"}, the last five '
                         'optional ("node", "edge": no walk_length; "parts": "parts_path" or "partition", and "parts_per_batch", instead of '
                         'both)%s, got %r'
                         % (said, value))
    if not isinstance(sampler, str) or sampler not in SAMPLERS:
        raise ValueError("subgraph_batches: sampler must be one of %s, got %r" % (", ".join('"%s"' % name for name in SAMPLERS), sampler))
    refused = [key for key in _REFUSED[sampler] if key in value]
    if refused:
        raise ValueError('subgraph_batches: "sampler": "%s" takes no %s (it takes %s)'
                         % (sampler, " and no ".join(refused), " and ".join(_REQUIRED[sampler])))
    if sampler == "parts" and "parts_path" in value and "partition" in value:
        raise ValueError('subgraph_batches: "sampler": "parts" takes exactly one of parts_path (a partition the user brings) and '
                         'partition (one computed here), not both')
    missing = [key for key in _REQUIRED[sampler] if key not in value and not (key == "parts_path" and "partition" in value)]
    if missing:
        raise ValueError('subgraph_batches: "sampler": "%s" requires %s' % (sampler, " and ".join(missing)))
    if sampler != "walk" and "normalisation" not in value:
        raise ValueError('subgraph_batches: "sampler": "%s" requires the key "normalisation": its batches are not anchored at TRAIN '
                         'nodes, and the plain mean over a batch that holds none is 0/0' % sampler)
    parsed = {}
    if "roots_per_batch" in value:
        parsed["roots_per_batch"] = integer_at_least(value["roots_per_batch"], 1,
                                                     "subgraph_batches: roots_per_batch must be a positive integer, got %r")
    if "walk_length" in value:
        try:
            parsed["walk_length"] = check_walk_length(value["walk_length"])
        except ValueError as error:
            raise ValueError("subgraph_batches: %s" % error) from None
    if sampler == "parts":
        if "partition" in value:
            parsed["partition"] = parse_partition(value["partition"])
        else:
            if not isinstance(value["parts_path"], str) or not value["parts_path"]:
                raise ValueError("subgraph_batches: parts_path must be the path of a .npy file, got %r" % (value["parts_path"],))
            parsed["parts_path"] = value["parts_path"]
        parsed["parts_per_batch"] = integer_at_least(value["parts_per_batch"], 1,
                                                     "subgraph_batches: parts_per_batch must be a positive integer, got %r")
    seed = value.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("subgraph_batches: seed must be an integer, got %r" % (seed,))
    parsed["seed"] = int(seed)
    parse_bool_keys("subgraph_batches", value, parsed, ("sparse_features", "data_parallel"))
    if "normalisation" in value:
        parsed["normalisation"] = parse_normalisation(value["normalisation"])
    if "sampler" in value:
        parsed["sampler"] = sampler
    return parsed


# ---- one plan per epoch: the host side of every sampler ------------------------------------------------------------------------------
class SamplerPlan(NamedTuple):
    """What the host needs to list an epoch's batches (epoch_node_lists), taken once per TRAIN state from the fold."""
    sampler: str                                # one of SAMPLERS
    seed: int
    fold_mask: np.ndarray                       # the TRAIN mask: "walk" cuts its nodes; the other three take their batch count from it
    per_batch: int                              # R, or q for "parts"
    num_nodes: int                              # V
    entry_ends: Optional[np.ndarray] = None     # "node": int64 [V], the by-target entries up to and including node v's (all types)
    parts: Optional[np.ndarray] = None          # "parts": the validated int32 [V] array of the file
    part_nodes: Optional[List[np.ndarray]] = None       # "parts": per part its nodes, int32 ascending

    @property
    def walk_steps(self) -> int:
        """The walk length of the sampler's device front: "edge" is one step from every root; "node" and "parts" do not walk."""
        return 1 if self.sampler == "edge" else 0

    @property
    def walked(self) -> bool:
        """Are an epoch's lists root lists (walked on the device) and not the node sets themselves?"""
        return self.sampler in ("walk", "edge")

    def longest(self) -> int:
        """No list of any epoch is longer than this."""
        if self.sampler == "parts":
            return int(np.sort([len(nodes) for nodes in self.part_nodes])[-self.per_batch:].sum())
        return min(self.per_batch, self.num_nodes) if self.sampler != "walk" else self.per_batch

    def batches_per_epoch(self) -> int:
        items = len(self.part_nodes) if self.sampler == "parts" else int(np.count_nonzero(np.asarray(self.fold_mask) != 0))
        return -(-items // self.per_batch)


def load_parts(path: str, num_nodes: int) -> np.ndarray:
    """The partition of "parts_path": a .npy holding int32 [V] with values 0 .. P - 1 and no part empty, or a ValueError that names
    the file."""
    try:
        parts = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as error:
        raise ValueError("subgraph_batches: parts_path %r cannot be read as a .npy array (%s)" % (path, error)) from None
    return validated_parts(parts, num_nodes, "parts_path %r" % (path,))


def validated_parts(parts: np.ndarray, num_nodes: int, what: str) -> np.ndarray:
    """What a partition must be wherever it comes from (`what` names the file, or the computed one): int32 [V] with values
    0 .. P - 1 and no part empty, or a ValueError."""
    if parts.dtype != np.int32 or parts.shape != (num_nodes,):
        raise ValueError("subgraph_batches: %s must hold an int32 array of shape (%d,), one part per node; it holds %s %r"
                         % (what, num_nodes, parts.dtype, parts.shape))
    if num_nodes == 0 or parts.min() < 0:
        raise ValueError("subgraph_batches: %s holds a negative part or no node at all" % what)
    sizes = np.bincount(parts)
    if (sizes == 0).any():
        raise ValueError("subgraph_batches: %s: the parts must be 0 .. P - 1 with none empty; of 0 .. %d, part %d has no node"
                         % (what, len(sizes) - 1, int(np.flatnonzero(sizes == 0)[0])))
    return parts


def sampler_plan(subgraph: Dict, fold_mask, adjacency_lists, num_nodes: int, partition=None) -> SamplerPlan:
    """The plan of a parsed `subgraph_batches` over one fold: "node" takes the in-degrees from the fold's adjacency lists here, once;
    "parts" reads and validates its file here (load_parts), or under the key "partition" takes `partition`() -> the computed int32
    [V] host array (graph_partition.partition_graph of the TRAIN state's device RelGraph: the caller holds that graph) through the
    same validation."""
    sampler, V = subgraph.get("sampler", "walk"), int(num_nodes)
    plan = SamplerPlan(sampler, int(subgraph["seed"]) & 0xffffffff, np.asarray(fold_mask),
                       subgraph["parts_per_batch" if sampler == "parts" else "roots_per_batch"], V)
    if sampler == "node":
        in_degree = np.zeros(V, dtype=np.int64)
        for edges in adjacency_lists:
            in_degree += np.bincount(np.asarray(edges).reshape(-1, 2)[:, 1], minlength=V)
        if not in_degree.sum():
            raise ValueError('subgraph_batches: "sampler": "node" draws a by-target entry; the graph has none')
        plan = plan._replace(entry_ends=np.cumsum(in_degree))
    if sampler == "parts":
        if "partition" in subgraph:
            if partition is None:
                raise ValueError('subgraph_batches: partition: the plan of a computed partition needs the device graph '
                                 '(SingleGraphBatches.subgraph_plan computes it from the TRAIN state)')
            parts = validated_parts(np.ascontiguousarray(partition()), V, "partition (the computed one)")
        else:
            parts = load_parts(subgraph["parts_path"], V)
        order = np.argsort(parts, kind="stable").astype(np.int32)           # (a part's nodes ascending)
        plan = plan._replace(parts=parts, part_nodes=np.split(order, np.cumsum(np.bincount(parts))[:-1]))
    return plan


def epoch_node_lists(plan: SamplerPlan, epoch: int) -> List[np.ndarray]:
    """The lists of one epoch, each int32, ascending and distinct: root lists for "walk" (epoch_seed_batches, its bits unchanged) and
    "edge" (one walk step from each, SubgraphSampler(graph, 1).sample), the node sets themselves for "node" and "parts".  A pure
    function of (the plan, epoch): the TRAIN generator, train_batch_weights, the pre-sampling (epochs 0x80000000 + e) and the
    data-parallel schedule all read it."""
    seed, epoch = plan.seed, int(epoch) & 0xffffffff
    if plan.sampler == "walk":
        return epoch_seed_batches(plan.fold_mask, plan.per_batch, seed, epoch)
    if plan.sampler == "parts":
        order = np.random.RandomState([seed, epoch, 3]).permutation(len(plan.part_nodes))
        return [np.sort(np.concatenate([plan.part_nodes[p] for p in order[i:i + plan.per_batch]])).astype(np.int32)
                for i in range(0, len(order), plan.per_batch)]
    lists = []
    for j in range(plan.batches_per_epoch()):
        if plan.sampler == "node":      # the target of a uniformly drawn by-target entry: a node in proportion to its in-degree
            at = np.random.RandomState([seed, epoch, j, 1]).randint(0, int(plan.entry_ends[-1]), size=plan.per_batch, dtype=np.int64)
            drawn = np.searchsorted(plan.entry_ends, at, side="right")
        else:                           # "edge": uniform roots; the step from root u takes entry (u <- v) with probability 1 / deg u
            drawn = np.random.RandomState([seed, epoch, j, 2]).randint(0, plan.num_nodes, size=plan.per_batch)
        lists.append(np.unique(drawn).astype(np.int32))
    return lists
