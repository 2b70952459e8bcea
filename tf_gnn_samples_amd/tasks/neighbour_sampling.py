"""Neighbour-sampled mini-batches of ONE graph (csrc/neighbour_sample.hip, include/relgnn_sampling.h): seed nodes, a fanout-limited
neighbourhood around them drawn on the device from the by-target bucketing the full graph's RelGraph already holds, and the
relabelled subgraph as a DeviceBatch.

Host round trips of NeighbourSampler.sample(): the seed list is validated on the host (in range, distinct; one small copy of a
device seed list), and the subgraph's sizes are read back ONCE behind the last hop, because its tensors are sized by them.  With
every fanout positive the hops themselves run without a read-back: their buffers are sized from frontier bound x types x fanout.  A
hop whose fanout is 0 (take every neighbour) has no such bound and reads its edge count back before it emits: one more round trip
per such hop.

NeighbourSampler stands on StampedNodeSet (a RelGraph plus its stamp array; csrc/node_set.h), as the subgraph sampler does; sample()
and sample_by_hop() share the hops, the read-back and the loop behind it; they differ in the node list and the relabel / degree kernels.

NeighbourSampler.sample_by_hop() gives the same subgraph numbered by hop (include/relgnn_layered_sampling.h) with the same round
trips; HopSubgraph.device_batch(layered=True) puts one LevelGraph per layer beside it, so that a model with as many layers as hops
runs each layer on the hops it needs (the citation task's `sampled_batches` key "layered"; models/sparse_graph_model.py).
With derived=True (the key "blocks") the levels bring their bucketings, derived on the device from the union graph's one
(derived_level_graphs; csrc/level_plan.hip, csrc/level_plan.h), and say which of their rows are targets (RelGraph.num_targets).
"""
import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..graph import RelGraph, _upload, as_rel_graph
from .sparse_features import PhaseTrace, SparseRows
from .sparse_graph_task import DeviceBatch

# relgnn_neighbour_sample_max_fanout / _max_hops (the library is not loaded to validate a parameter; tests/test_gpu_neighbour_sampling.py
# holds the two against each other)
MAX_FANOUT = 64
MAX_HOPS = 8


def check_fanouts(fanouts) -> List[int]:
    """The fanout list as python ints, or a ValueError that says what include/relgnn_sampling.h supports."""
    if not isinstance(fanouts, (list, tuple)) or not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in fanouts):
        raise ValueError("fanouts must be a list of integers, got %r" % (fanouts,))
    out = [int(k) for k in fanouts]
    if not 1 <= len(out) <= MAX_HOPS or any(k < 0 or k > MAX_FANOUT for k in out):
        raise ValueError("fanouts must be 1 to %d integers in [0, %d] (0 takes every neighbour), got %r" % (MAX_HOPS, MAX_FANOUT, fanouts))
    return out


def epoch_seed_batches(fold_mask, seeds_per_batch: int, seed: int, epoch: int) -> List[np.ndarray]:
    """The seed lists of one epoch: a permutation of the fold's nodes (mask != 0) from np.random.RandomState([seed, epoch]), cut into
    batches of seeds_per_batch; every batch int32 and ascending, the last one possibly short."""
    seeds_per_batch = int(seeds_per_batch)
    if seeds_per_batch < 1:
        raise ValueError("seeds_per_batch must be positive, got %r" % (seeds_per_batch,))
    nodes = np.flatnonzero(np.asarray(fold_mask) != 0)
    order = np.random.RandomState([int(seed) & 0xffffffff, int(epoch) & 0xffffffff]).permutation(len(nodes))
    shuffled = nodes[order]
    return [np.sort(shuffled[i:i + seeds_per_batch]).astype(np.int32) for i in range(0, len(shuffled), seeds_per_batch)]


def validated_ids(ids, num_nodes: int, device, what: str) -> torch.Tensor:
    """`ids` (int32, one-dimensional, non-empty, in range, distinct) ascending on the device; `what` ("seed", "root", "node") names them."""
    host = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    if host.ndim != 1 or host.dtype != np.int32:
        raise ValueError("%ss must be a one-dimensional int32 array" % what)
    if len(host) == 0:
        raise ValueError("the %s list is empty" % what)
    if host.min() < 0 or host.max() >= num_nodes:
        raise ValueError("%s outside [0, %d)" % (what, num_nodes))
    ordered = np.sort(host)
    if (ordered[1:] == ordered[:-1]).any():
        raise ValueError("the %s list names a node twice" % what)
    if torch.is_tensor(ids) and ids.is_cuda and np.array_equal(ordered, host):
        return ids.contiguous()
    return torch.as_tensor(ordered, device=device)


def _batch_rows(sub, features, labels, mask, out_keep: float, named_rows: bool, **more):
    """-> (the feature rows of `sub.nodes`, the batch's `extra`).  `features` a SparseRows: the [n, 1] stand-in takes the table's place and
    the rows' subset (SparseRows.take_rows, csrc/sparse_subset.hip) travels under extra['sparse_node_features']; no dense row is built."""
    extra = dict(labels=labels, mask=mask, out_layer_dropout_keep_prob=out_keep, sampled_nodes=sub.nodes, **more)
    if isinstance(features, SparseRows):
        extra['sparse_node_features'] = features.take_rows(sub.nodes, validated=True, named_rows=named_rows)
        return torch.zeros((sub.num_nodes, 1), dtype=torch.float32, device=sub.nodes.device), extra      # sparse_features.node_stand_in
    return features.index_select(0, sub.nodes.long()), extra


class SampledSubgraph(NamedTuple):
    nodes: torch.Tensor                         # int32 [n]: ascending global ids; local id = position
    adjacency_lists: List[torch.Tensor]         # per edge type int32 [E_l, 2] = (source, target) in local ids
    type_to_num_incoming_edges: torch.Tensor    # float32 [L, n]: the sampled in-degrees
    seed_mask: torch.Tensor                     # float32 [n]
    num_nodes: int
    num_edges: int
    message_weights: Optional[torch.Tensor] = None      # float32 [num_edges] in the order of the lists, one behind the other: the
    #                                                     scale of every message in the degree scale's place (subgraph_sampling.py)

    def device_batch(self, features, labels: torch.Tensor, fold_mask: torch.Tensor, out_keep: float = 1.0,
                     named_rows: bool = False) -> DeviceBatch:
        """The subgraph as one training batch: feature and label rows of the device-resident [V, ...] tables, the loss mask
        seed_mask * fold_mask[nodes] (the rows and the rest of `extra`: _batch_rows).
        named_rows: the subset also carries the words it names (`"sparse_gradient": true`; SparseRows.named_rows).
        message_weights set: the batch brings its RelGraph with those weights preset as the scale of its degree table
        (RelGraph.preset_message_scale), so every layer that asks graph.degree_scale(batch degrees) receives them."""
        index = self.nodes.long()
        rows, extra = _batch_rows(self, features, labels.index_select(0, index), self.seed_mask * fold_mask.index_select(0, index),
                                  out_keep, named_rows)
        batch = DeviceBatch.from_tensors(1, self.num_nodes, self.num_edges, rows, self.adjacency_lists,
                                         self.type_to_num_incoming_edges, extra=extra)
        if self.message_weights is not None:
            # (the sampler's ids are in range; like the graph the model buckets itself, validate="deferred", it is not inspected for
            #  hubs: every bucket keeps one wave, so the batch takes the routes it takes without the weights)
            graph = as_rel_graph(self.adjacency_lists, self.num_nodes, validate=False)
            graph.preset_message_scale(batch.type_to_num_incoming_edges, self.message_weights)
            batch.graph = graph
        return batch


class LevelGraph(NamedTuple):
    """What layer l of H (from the input, l = 1 .. H) of a layered batch runs on: a square graph over the first num_sources =
    n_{H-l+1} nodes whose edges are the ones with a target among the first num_targets = n_{H-l}; the layer's output is cut to
    num_targets rows."""
    adjacency_lists: List[torch.Tensor]         # per type the prefix view adjacency[l][:E_{l,H-l}] (no copy)
    num_sources: int
    num_targets: int
    type_to_num_incoming_edges: torch.Tensor    # float32 [L, num_sources]: the sampled in-degrees of the targets, 0 behind them
    graph: Optional[RelGraph] = None            # the level's bucketing where the batch brings it along (evaluation batches, and every
    #                                             batch under "blocks", whose graphs also say graph.num_targets == num_targets); the
    #                                             model buckets adjacency_lists itself otherwise


class HopSubgraph(NamedTuple):
    """The subgraph of SampledSubgraph under another numbering (NeighbourSampler.sample_by_hop): nodes by the hop that first
    reached them.  With n_d = hop_nodes[d] the nodes at most d hops from a seed are the local ids [0, n_d), and the edges whose
    target is among them are the first hop_edges[l][d] entries of type l's list (d < H): hops come out ascending."""
    nodes: torch.Tensor                         # int32 [n]: the seeds ascending, then the nodes first reached in hop 1 ascending, ...
    adjacency_lists: List[torch.Tensor]         # as SampledSubgraph's, in these local ids
    type_to_num_incoming_edges: torch.Tensor    # float32 [L, n]
    seed_mask: torch.Tensor                     # float32 [n]: ones on [0, n_0)
    num_nodes: int
    num_edges: int
    hop_nodes: List[int]                        # [n_0, ..., n_H], cumulative
    hop_edges: List[List[int]]                  # per type [E_{l,0}, ..., E_{l,H-1}]: the type-l edges emitted by hops 0 .. h

    def level_graphs(self, bucketed: bool = False, route_like: Optional[RelGraph] = None, derived: bool = False) -> List[LevelGraph]:
        """One LevelGraph per layer of a model with as many layers as hops; level 1 is the union graph.  bucketed: every level
        carries its RelGraph (the sampler's ids are in range: nothing is validated), routed as `route_like` routes its reductions
        (RelGraph.route_like) when one is given.  derived (the citation task's `"blocks": true`; implies bucketed): the union graph
        is bucketed once and every smaller level's arrays are derived from its (derived_level_graphs: no further sort), and every
        graph says which of its rows are targets (RelGraph.num_targets), so that a layer may compute those alone."""
        H = len(self.hop_nodes) - 1
        degrees, levels = self.type_to_num_incoming_edges, []
        graphs = derived_level_graphs(self, route_like) if derived else None
        for layer in range(1, H + 1):
            sources, targets = self.hop_nodes[H - layer + 1], self.hop_nodes[H - layer]
            adjacency = [a[:edges[H - layer]] for a, edges in zip(self.adjacency_lists, self.hop_edges)]
            if layer == 1:                      # (the nodes behind n_{H-1} are leaves: their columns are zero already)
                table = degrees
            else:
                table = torch.zeros((degrees.shape[0], sources), dtype=degrees.dtype, device=degrees.device)
                table[:, :targets] = degrees[:, :targets]
            graph = None
            if derived:
                graph = graphs[layer - 1]
            elif bucketed:
                graph = RelGraph(adjacency, sources, validate=False)
                if route_like is not None:
                    graph.route_like(route_like)
            levels.append(LevelGraph(adjacency, sources, targets, table, graph))
        return levels

    def device_batch(self, features, labels: torch.Tensor, fold_mask: torch.Tensor, out_keep: float = 1.0,
                     named_rows: bool = False, layered: bool = True, bucketed: bool = False,
                     route_like: Optional[RelGraph] = None, derived: bool = False) -> DeviceBatch:
        """layered=False: the union batch in hop order, through SampledSubgraph.device_batch.  layered=True: feature rows of all n
        nodes, labels and mask of the n_0 seeds only (mask = fold_mask[seeds]: num_masked and num_correct mean what they did), and
        extra['layer_graphs'] = level_graphs(), which models/sparse_graph_model.py runs layer by layer.  bucketed / route_like
        (layered only; an evaluation batch): the levels bring their bucketing, level 1's is the batch's own `graph`.  derived (layered
        only; `"blocks": true`): the same, with the levels' bucketings derived from the union graph's (level_graphs)."""
        union = SampledSubgraph(self.nodes, self.adjacency_lists, self.type_to_num_incoming_edges, self.seed_mask, self.num_nodes,
                                self.num_edges)
        if not layered:
            return union.device_batch(features, labels, fold_mask, out_keep, named_rows=named_rows)
        seeds = self.nodes[:self.hop_nodes[0]].long()
        rows, extra = _batch_rows(self, features, labels.index_select(0, seeds), fold_mask.index_select(0, seeds), out_keep, named_rows,
                                  layer_graphs=self.level_graphs(bucketed, route_like, derived))
        batch = DeviceBatch.from_tensors(1, self.num_nodes, self.num_edges, rows, self.adjacency_lists,
                                         self.type_to_num_incoming_edges, extra=extra)
        if bucketed or derived:
            batch.graph = extra['layer_graphs'][0].graph
        return batch


# ---- level bucketings derived from the union graph's (csrc/level_plan.hip, csrc/level_plan.h) ------------------------------------------
LEVEL_PLAN_FIXED = 11                 # a record of relgnn_level_plan's `desc`: T, S, P, eight offsets, then delta[L] and off'[L + 1]
LEVEL_PLAN_ARRAYS = ("rowptr_t", "perm_t", "inv_perm_t", "rowptr_s", "tgt_s", "frow_s", "pos_t_of_s", "perm_s")


def level_plan_layout(hop_nodes, hop_edges, num_edge_types: int):
    """What relgnn_level_plan is told about the levels d = 0 .. H - 2 of a hop-ordered subgraph (level H - 1 is the union graph), from
    the sizes the sampler read back: -> (desc int64 [H - 1, 12 + 2 L], the int32 length of the output arena, the largest S_d L + 1,
    the largest P_d).  Host arithmetic only.  Every array starts on a multiple of four entries."""
    L, H = int(num_edge_types), len(hop_nodes) - 1
    desc = np.zeros((max(H - 1, 0), LEVEL_PLAN_FIXED + 2 * L + 1), dtype=np.int64)
    union_offsets = np.concatenate([[0], np.cumsum([int(edges[H - 1]) for edges in hop_edges])]).astype(np.int64)
    at, max_rows, max_messages = 0, 0, 0
    for d in range(H - 1):
        targets, sources = int(hop_nodes[d]), int(hop_nodes[d + 1])
        offsets = np.concatenate([[0], np.cumsum([int(edges[d]) for edges in hop_edges])]).astype(np.int64)
        messages, rows = int(offsets[-1]), sources * L + 1
        desc[d, :3] = (targets, sources, messages)
        for k, name in enumerate(LEVEL_PLAN_ARRAYS):
            desc[d, 3 + k] = at
            at += -(-(rows if name.startswith("rowptr") else messages) // 4) * 4
        desc[d, LEVEL_PLAN_FIXED:LEVEL_PLAN_FIXED + L] = union_offsets[:L] - offsets[:L]
        desc[d, LEVEL_PLAN_FIXED + L:] = offsets
        max_rows, max_messages = max(max_rows, rows), max(max_messages, messages)
    if at >= 2 ** 31 - 1:
        raise ValueError("the level graphs are too large for int32 indices")
    return desc, at, max_rows, max_messages


def derived_level_graphs(sub: "HopSubgraph", route_like: Optional[RelGraph] = None) -> List[RelGraph]:
    """The RelGraph of every layer's level, layer 1 (the union graph) first: ONE bucketing (the ordinary constructor over the union
    graph: the batch's two sorts) and one relgnn_level_plan call that derives the arrays of every smaller level from it, on the
    current stream, with no read-back (the sizes come from hop_nodes / hop_edges).  A derived level is a RelGraph.from_arrays graph
    over its num_sources nodes whose arrays are views of one arena, whose col_t is a view of the union's and whose adjacency lists are
    the prefix views; its num_targets is the level's.  The union graph's is n_{H-1}: its leaves have no incoming edge."""
    H, L = len(sub.hop_nodes) - 1, len(sub.adjacency_lists)
    union = RelGraph(sub.adjacency_lists, sub.num_nodes, validate=False)
    union.num_targets = int(sub.hop_nodes[H - 1])
    graphs = [union]
    if H > 1:
        lib = _lib.load_library()
        if H - 1 > lib.relgnn_level_plan_max_levels() or lib.relgnn_level_plan_desc_stride(L) != LEVEL_PLAN_FIXED + 2 * L + 1:
            raise _lib.RelGnnLibraryError("relgnn_level_plan does not take %d levels of %d edge types" % (H - 1, L))
        desc, length, max_rows, max_messages = level_plan_layout(sub.hop_nodes, sub.hop_edges, L)
        dev = union.device
        arena = torch.empty(length, dtype=torch.int32, device=dev)
        ws_bytes = lib.relgnn_level_plan_workspace_bytes(union.M, H - 1)
        ws = _lib.scratch(ws_bytes, dev)
        M = union.M
        _lib.launch("relgnn_level_plan", _lib.ptr(union.rowptr_t), *[_lib.ptr(getattr(union, k)) if M else None
                                                                      for k in ("col_t", "perm_t", "inv_perm_t")],
                    _lib.ptr(union.rowptr_s), *[_lib.ptr(getattr(union, k)) if M else None
                                                for k in ("tgt_s", "frow_s", "pos_t_of_s", "perm_s")],
                    union.V, L, M, _lib.ptr(_upload(desc, dev)), H - 1, max_rows, max_messages, _lib.ptr(arena), length,
                    _lib.ptr(ws) if M else None, ws_bytes)
        for d in range(H - 2, -1, -1):                                 # layer 2 runs on level H - 2, ..., layer H on level 0
            targets, sources, messages = (int(x) for x in desc[d, :3])
            rows = sources * L + 1
            arrays = {name: arena[int(desc[d, 3 + k]):int(desc[d, 3 + k]) + (rows if name.startswith("rowptr") else messages)]
                      for k, name in enumerate(LEVEL_PLAN_ARRAYS)}
            adjacency = [a[:edges[d]] for a, edges in zip(sub.adjacency_lists, sub.hop_edges)]
            graphs.append(RelGraph.from_arrays(adjacency, sources, col_t=union.col_t[:messages], num_targets=targets, **arrays))
    if route_like is not None:
        for graph in graphs:
            graph.route_like(route_like)
    return graphs


class StampedNodeSet(PhaseTrace):
    """One RelGraph on the GPU (rowptr_t / col_t are read in place) and its [V] int32 stamp array, all zero between calls and after a
    call that raised.  A call stamps a node set (`begin`, or a launch of the sampler's own) and lists it ascending (`compact`)."""

    def __init__(self, graph, what: str, refuse_unsupported, trusts_ids: bool = True):
        """what: names the sampler in the refusals; refuse_unsupported(lib) raises ValueError for what the library does not support.
        trusts_ids=False (tasks/layerwise.py): the user's kernels check every id of col_t themselves, and the graph is not inspected
        (check() would also split the hub buckets of a graph the model bucketed with validate="deferred")."""
        if not graph.rowptr_t.is_cuda:
            raise _lib.RelGnnLibraryError("%s runs on the GPU only; the graph is on %s" % (what, graph.rowptr_t.device))
        lib = _lib.load_library()
        refuse_unsupported(lib)
        if trusts_ids:
            graph.check()                                         # (node ids in range: the kernels trust col_t)
        self.graph = graph
        self.stamp = torch.zeros(graph.V, dtype=torch.int32, device=graph.device)
        self._compact_bytes = lib.relgnn_neighbour_sample_workspace_bytes(graph.V)
        self._compact_ws = None                                   # the compaction's workspace, for the length of a call

    def _guarded(self, body, *args):
        """body(*args) on the graph's device with the compaction's workspace in place; the stamps are zeroed if anything raises."""
        try:
            with torch.cuda.device(self.graph.device):
                self._compact_ws = _lib.scratch(self._compact_bytes, self.graph.device)
                return body(*args)
        except BaseException:
            self.stamp.zero_()                                    # whatever a half-run call stamped
            raise
        finally:
            self._compact_ws = None

    def begin(self, ids: torch.Tensor) -> None:
        """Stamps the listed nodes (validated ids) -1."""
        _lib.launch("relgnn_neighbour_sample_begin", _lib.ptr(ids), ids.numel(), _lib.ptr(self.stamp), self.graph.V)

    def compact(self, value: int, out: torch.Tensor, bound: int, count: torch.Tensor) -> None:
        """out[:count] = the nodes stamped `value` (0: any stamp) ascending, at most `bound`; `count` stays on the device.  The
        compaction belongs to the node set, whatever the entry point is called."""
        _lib.launch("relgnn_neighbour_sample_compact", _lib.ptr(self.stamp), self.graph.V, value, _lib.ptr(out), bound, _lib.ptr(count),
                    _lib.ptr(self._compact_ws), self._compact_bytes)


class NeighbourSampler(StampedNodeSet):
    """Sampler over one RelGraph (its rowptr_t / col_t are read in place).  Holds the [V] int32 stamp array, all zero between calls
    (StampedNodeSet; `trace`: scripts/bench_neighbour_sampling.py)."""

    def __init__(self, graph: RelGraph, fanouts: Sequence[int], seed: int = 0, replica: int = 0):
        self.fanouts = check_fanouts(fanouts)

        def refuse_unsupported(lib):
            host = (ctypes.c_int32 * len(self.fanouts))(*self.fanouts)
            if not lib.relgnn_neighbour_sample_supported(host, len(self.fanouts), graph.V, graph.L):
                raise ValueError("neighbour sampling does not support fanouts %r on a graph of %d nodes and %d edge types "
                                 "(relgnn_neighbour_sample_supported)" % (self.fanouts, graph.V, graph.L))
            if not 0 <= int(replica) < 2 ** 31:                   # (refused here, behind the fanouts and in front of graph.check(), as ever)
                raise ValueError("replica must be in [0, 2^31), got %r" % (replica,))
        super().__init__(graph, "neighbour sampling", refuse_unsupported)
        self.seed, self.replica = int(seed) & 0xffffffff, int(replica)
        self.synced_hops = [h for h, k in enumerate(self.fanouts) if k == 0]     # the hops that read their edge count back

    def sample(self, seeds, draw: int) -> SampledSubgraph:
        """seeds: int32 device tensor (a host array is uploaded), distinct node ids; draw: the count of sampled batches so far."""
        return self._call(self._sample, seeds, draw)

    def sample_by_hop(self, seeds, draw: int) -> "HopSubgraph":
        """The subgraph sample(seeds, draw) gives — the same hops, draws and edges — numbered by hop: the seeds, then the nodes first
        reached in hop 1, ..., each group in ascending id.  No read-back beyond sample()'s."""
        return self._call(self._sample_by_hop, seeds, draw)

    def _call(self, body, seeds, draw: int):
        seeds = validated_ids(seeds, self.graph.V, self.graph.device, "seed")
        return self._guarded(body, seeds, int(draw) & 0xffffffff)

    def _sample(self, seeds: torch.Tensor, draw: int) -> SampledSubgraph:
        g = self.graph
        hops, summary, _ = self._hops(seeds, draw)
        node_bound = min(g.V, seeds.numel() + sum(int(e.shape[0]) for _, _, _, e in hops))
        nodes_buf = torch.empty(node_bound, dtype=torch.int32, device=g.device)
        self.compact(0, nodes_buf, node_bound, summary[-1:])
        self._mark("compaction")
        per_hop, n = self._read_back(summary)                     # the one read-back of a call whose fanouts are all positive
        nodes = nodes_buf[:n]
        lengths = [int(seeds.numel())] + [p[g.L + 1] for p in per_hop[:-1]]            # the true length of every hop's frontier
        adjacency, degrees, seed_mask, num_edges, _ = self._relabelled(
            hops, per_hop, lengths, nodes, n, "relgnn_neighbour_sample_relabel", (_lib.ptr(nodes), n),
            "relgnn_neighbour_sample_degrees", lambda h, frontier: (_lib.ptr(frontier), _lib.ptr(nodes), n))
        return SampledSubgraph(nodes, adjacency, degrees, seed_mask, n, num_edges)

    def _sample_by_hop(self, seeds: torch.Tensor, draw: int) -> "HopSubgraph":
        g, H = self.graph, len(self.fanouts)
        hops, summary, last = self._hops(seeds, draw)
        per_hop, _ = self._read_back(summary)                     # the same one read-back; the id-ordered list is never compacted
        lengths = [int(seeds.numel())] + [p[g.L + 1] for p in per_hop]                 # nodes first reached in hop 0 (the seeds) .. H
        starts = [0] + np.cumsum(lengths).tolist()
        hop_nodes, n = starts[1:], starts[-1]                     # n_0 .. n_H
        # the frontier buffers ARE the per-hop lists: cut to their true lengths and laid end to end (a device copy, no kernel of ours)
        nodes = torch.cat([f[:nf] for f, nf in zip([hop[0] for hop in hops] + [last], lengths)])
        host_starts = (ctypes.c_int64 * (H + 2))(*starts)
        adjacency, degrees, seed_mask, num_edges, hop_edges = self._relabelled(
            hops, per_hop, lengths, nodes, n, "relgnn_neighbour_sample_relabel_by_hop",
            (_lib.ptr(self.stamp), g.V, _lib.ptr(nodes), host_starts, H + 1),
            "relgnn_neighbour_sample_degrees_by_hop", lambda h, frontier: (starts[h], n))
        return HopSubgraph(nodes, adjacency, degrees, seed_mask, n, num_edges, hop_nodes, hop_edges)

    def _read_back(self, summary: torch.Tensor):
        """-> ([L + 1 totals | next frontier's length] per hop, the summary's last entry: the node count where a compaction wrote it)."""
        sizes, L = summary.tolist(), self.graph.L
        self._mark("readback")
        return [sizes[h * (L + 2):(h + 1) * (L + 2)] for h in range(len(self.fanouts))], sizes[-1]

    def _relabelled(self, hops, per_hop, lengths, nodes: torch.Tensor, n: int, relabel: str, relabel_args, degrees_of: str, degree_args):
        """What sample and sample_by_hop share behind the read-back.  Per hop: `relabel`(edges, first, count, *relabel_args, out) for every
        type that has edges, `degrees_of`(counts, bound, the frontier's length, L, *degree_args(h, frontier), degrees); then finish, which
        clears the stamps of `nodes`.  -> (adjacency, degrees, seed_mask, the edge total, per type the edges written by hops 0 .. h)."""
        L, dev = self.graph.L, self.graph.device
        type_edges = [sum(p[l] for p in per_hop) for l in range(L)]
        adjacency = [torch.empty((e, 2), dtype=torch.int32, device=dev) for e in type_edges]
        degrees = torch.zeros((L, n), dtype=torch.float32, device=dev)
        written, hop_edges = [0] * L, [[] for _ in range(L)]
        for h, ((frontier, bound, counts, edges), p) in enumerate(zip(hops, per_hop)):
            first = 0
            for l in range(L):
                if p[l]:
                    _lib.launch(relabel, _lib.ptr(edges), first, p[l], *relabel_args, _lib.ptr(adjacency[l][written[l]:written[l] + p[l]]))
                first += p[l]
                written[l] += p[l]
                hop_edges[l].append(written[l])
            _lib.launch(degrees_of, _lib.ptr(counts), bound, lengths[h], L, *degree_args(h, frontier), _lib.ptr(degrees))
        seed_mask = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.launch("relgnn_neighbour_sample_finish", _lib.ptr(nodes), n, _lib.ptr(self.stamp), self.graph.V, _lib.ptr(seed_mask))
        self._mark("relabel")
        return adjacency, degrees, seed_mask, sum(type_edges), hop_edges

    def _hops(self, seeds: torch.Tensor, draw: int):
        """begin, then count / take / compact(h + 1) per hop -> ([(frontier, bound, counts, edges) per hop], the summary still on the
        device, the buffer of the nodes first reached in the last hop)."""
        lib, g = _lib.load_library(), self.graph
        V, L, dev = g.V, g.L, g.device
        i32 = lambda n: torch.empty(int(n), dtype=torch.int32, device=dev)
        self._mark("start")
        self.begin(seeds)
        frontier, bound = seeds, int(seeds.numel())
        count = torch.full((1,), bound, dtype=torch.int32, device=dev)
        hops = []
        # per hop [L + 1 totals | next frontier's length], then the subgraph's node count: read back once
        summary = torch.zeros(len(self.fanouts) * (L + 2) + 1, dtype=torch.int32, device=dev)
        for h, k in enumerate(self.fanouts):
            counts, offsets = i32(bound * L + 1), i32(bound * L + 1)
            totals = summary[h * (L + 2):h * (L + 2) + L + 1]
            hop_ws, hop_ws_bytes = self._compact_ws, self._compact_bytes             # (covers V items: a hop's count fits unless L * bound > V)
            if bound * L + 1 > V:
                hop_ws_bytes = lib.relgnn_neighbour_sample_workspace_bytes(bound * L + 1)
                hop_ws = _lib.scratch(hop_ws_bytes, dev)
            _lib.launch("relgnn_neighbour_sample_count", _lib.ptr(g.rowptr_t), V, L, _lib.ptr(frontier), _lib.ptr(count), bound, k,
                        _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(totals), _lib.ptr(hop_ws), hop_ws_bytes)
            edge_bound = min(bound * L * k, g.M) if k > 0 else int(totals[L])          # k == 0: this hop's one read-back
            edges = torch.empty((edge_bound, 2), dtype=torch.int32, device=dev)
            _lib.launch("relgnn_neighbour_sample_take", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t), V, L, _lib.ptr(frontier), _lib.ptr(count),
                        bound, k, h, draw, self.seed, self.replica, _lib.ptr(offsets), edge_bound, _lib.ptr(self.stamp),
                        _lib.ptr(edges) if edge_bound else None)
            hops.append((frontier, bound, counts, edges))
            self._mark("hops")
            next_bound = max(1, min(V, edge_bound))
            frontier, count = i32(next_bound), summary[h * (L + 2) + L + 1:h * (L + 2) + L + 2]
            self.compact(h + 1, frontier, next_bound, count)
            self._mark("compaction")
            bound = next_bound
        return hops, summary, frontier


def integer_at_least(value, minimum: int, message: str) -> int:
    """`value` as a python int when it is an integer (not a bool) >= minimum, or ValueError(message % (value,))."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < minimum:
        raise ValueError(message % (value,))
    return int(value)


def unknown_keys(value, known) -> list:
    """The keys of the dict `value` that are not among `known`, by their text ([] for what is no dict: the caller refuses that)."""
    return sorted(set(value) - set(known), key=str) if isinstance(value, dict) else []


def parse_sampled_batches(value) -> Optional[Dict]:
    """The task parameter `sampled_batches` as {"fanouts": [ints], "seeds_per_batch": int, "seed": int}, None when it is absent;
    the optional keys "sparse_features" (a bool: the batches take their feature rows from a SparseRows), "sparse_update" (a bool:
    the optimizer updates only the rows of the input projection's weight that a batch names) and "sparse_gradient" (a bool: that
    weight's gradient exists only as the rows a batch names) and "layered" (a bool: the batches are numbered by hop and every layer
    runs on the hops it needs) and "data_parallel" (a bool: train(group=...) hands the batches of an epoch out to the ranks; not
    together with "sparse_update" / "sparse_gradient") are carried only when given, and so is "evaluation" ({"fanouts": [k_1, ..., k_H],
    "seeds_per_batch": B, "keep": bool}, "keep" optional: VALIDATION, TEST and predict(nodes=...) run on sampled receptive fields,
    parse_evaluation) and "blocks" (a bool, behind "evaluation" in the parsed dict; needs "layered": true or "evaluation": the level
    graphs of a batch are derived from its union graph's bucketing and say which rows are targets, derived_level_graphs)."""
    if value is None:
        return None
    if not isinstance(value, dict) or not {"fanouts", "seeds_per_batch"} <= set(value) \
            or unknown_keys(value, ("fanouts", "seeds_per_batch", "seed", "sparse_features", "sparse_update", "sparse_gradient", "layered",
                                    "data_parallel", "evaluation", "blocks")):
        raise ValueError('sampled_batches must be {"fanouts": [k_1, ..., k_H], "seeds_per_batch": B, "seed": s, "sparse_features": bool, '
                         '"sparse_update": bool, "sparse_gradient": bool, "layered": bool, "data_parallel": bool, "evaluation": '
                         '{"fanouts": [...], "seeds_per_batch": B, "keep": bool}, "blocks": bool}, the last eight optional, got %r'
                         % (value,))
    per_batch = integer_at_least(value["seeds_per_batch"], 1, "sampled_batches: seeds_per_batch must be a positive integer, got %r")
    parsed = {"fanouts": check_fanouts(value["fanouts"]), "seeds_per_batch": per_batch, "seed": int(value.get("seed", 0))}
    parse_bool_keys("sampled_batches", value, parsed, ("sparse_features", "sparse_update", "sparse_gradient", "layered", "data_parallel"), {
        "sparse_update": ("sparse_features", "the rows a batch names are read from the transposed structure of its SparseRows"),
        "sparse_gradient": ("sparse_update", "the compact gradient is what the row-deferred update consumes; dense Adam reads a dense one")})
    by_rows = [key for key in ("sparse_update", "sparse_gradient") if parsed.get(key, False)]
    if parsed.get("data_parallel", False) and by_rows:
        raise ValueError('sampled_batches: "data_parallel": true cannot be combined with %s: the row stamps of the deferred update and '
                         'the compact gradient sink do not pass through the packed gradient all-reduce'
                         % " and ".join('"%s": true' % key for key in by_rows))
    if "evaluation" in value:
        parsed["evaluation"] = parse_evaluation(value["evaluation"])
    parse_bool_keys("sampled_batches", value, parsed, ("blocks",))
    if parsed.get("blocks", False) and not (parsed.get("layered", False) or "evaluation" in parsed):
        raise ValueError('sampled_batches: "blocks": true requires "layered": true or an "evaluation" key: only a batch that is run '
                         'level by level has level graphs to derive and target rows to keep')
    return parsed


def parse_bool_keys(what: str, value: Dict, parsed: Dict, keys, needs=None) -> None:
    """The optional bool keys of the parameter `what`, in the order of `keys`: each must be true or false and is carried into `parsed`
    only when given.  needs: key -> (the key that must be true for it to be true, why)."""
    for key in (key for key in keys if key in value):
        if not isinstance(value[key], bool):
            raise ValueError("%s: %s must be true or false, got %r" % (what, key, value[key]))
        needed, why = (needs or {}).get(key, (None, None))
        if needed is not None and value[key] and not parsed.get(needed, False):
            raise ValueError('%s: "%s": true requires "%s": true (%s)' % (what, key, needed, why))
        parsed[key] = value[key]


def check_sparse_node_features(what: str, parsed: Dict, sparse_node_features: bool) -> None:
    """The key "sparse_features" of the parameter `what` ("sampled_batches", "subgraph_batches") and sparse_node_features go together."""
    if sparse_node_features and not parsed.get("sparse_features", False):
        raise ValueError("%s cannot be combined with sparse_node_features unless it says \"sparse_features\": true: "
                         "the weight gradient of the sparse input projection over a row subset needs the transposed structure of "
                         "that subset, which is then built per batch (SparseRows.take_rows)" % what)
    if parsed.get("sparse_features", False) and not sparse_node_features:
        raise ValueError("%s: \"sparse_features\": true requires the task parameter sparse_node_features: True" % what)


def parse_evaluation(value) -> Dict:
    """The "evaluation" key of `sampled_batches` as {"fanouts": [ints], "seeds_per_batch": int}, "keep" (a bool: a fold's evaluation
    batches are built once and handed out again every epoch) carried only when given."""
    if not isinstance(value, dict) or unknown_keys(value, ("fanouts", "seeds_per_batch", "keep")) or not {"fanouts", "seeds_per_batch"} <= set(value):
        raise ValueError('sampled_batches: "evaluation" must be {"fanouts": [k_1, ..., k_H], "seeds_per_batch": B, "keep": bool}, the '
                         'last one optional, got %r' % (value,))
    per_batch = integer_at_least(value["seeds_per_batch"], 1,
                                 'sampled_batches: "evaluation": seeds_per_batch must be a positive integer, got %r')
    try:
        fanouts = check_fanouts(value["fanouts"])
    except ValueError as error:
        raise ValueError('sampled_batches: "evaluation": %s' % error) from None
    parsed = {"fanouts": fanouts, "seeds_per_batch": per_batch}
    if "keep" in value:
        if not isinstance(value["keep"], bool):
            raise ValueError('sampled_batches: "evaluation": keep must be true or false, got %r' % (value["keep"],))
        parsed["keep"] = value["keep"]
    return parsed


# ---- evaluation on sampled receptive fields ----------------------------------------------------------------------------------------
EVALUATION_REPLICA = 0x40000000       # | the fold's number: no data-parallel rank (a training sampler's replica) reaches it
PREDICT_SEEDS_PER_BATCH = 1024        # predict(nodes=...) without the "evaluation" key: exact fields, batches of this many nodes


def evaluation_replica(fold_number: int) -> int:
    """The sampler replica of a fold's evaluation batches (DataFold.VALIDATION.value, DataFold.TEST.value, or PREDICT_FOLD for
    predict(nodes=...)): with the batch's index in the fold as the draw, the random words of an evaluation batch are a function of
    (seed, fold, batch index) alone, the same in every epoch, and never a training batch's (replica = the rank, below 2^30)."""
    fold_number = int(fold_number)
    if not 0 <= fold_number < EVALUATION_REPLICA:
        raise ValueError("fold number out of range: %r" % (fold_number,))
    return EVALUATION_REPLICA | fold_number


PREDICT_FOLD = 3                      # (behind DataFold.TEST.value)


def evaluation_seed_batches(fold_mask, seeds_per_batch: int) -> List[np.ndarray]:
    """The seed lists of an evaluation epoch: the fold's nodes (mask != 0) in ascending id cut into runs of seeds_per_batch, the last one
    possibly short; int32.  No shuffle: batch i holds the same seeds in every epoch."""
    seeds_per_batch = int(seeds_per_batch)
    if seeds_per_batch < 1:
        raise ValueError("seeds_per_batch must be positive, got %r" % (seeds_per_batch,))
    nodes = np.flatnonzero(np.asarray(fold_mask) != 0).astype(np.int32)
    return [nodes[i:i + seeds_per_batch] for i in range(0, len(nodes), seeds_per_batch)]


def check_prediction_nodes(nodes, num_nodes: int):
    """predict(nodes=...): -> (the distinct ids ascending as int32, for every entry of `nodes` its position among them, `nodes` as an
    int64 array), or a ValueError for anything that is not a non-empty one-dimensional int32 / int64 list of ids in [0, num_nodes)."""
    if isinstance(nodes, (list, tuple)):
        if not all(isinstance(n, (int, np.integer)) and not isinstance(n, bool) for n in nodes):
            raise ValueError("nodes must be a list of integer node ids, got %r" % (nodes,))
        nodes = np.asarray(nodes, dtype=np.int64)
    if torch.is_tensor(nodes):
        nodes = nodes.detach().cpu().numpy()
    if not isinstance(nodes, np.ndarray) or nodes.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError("nodes must be an int32 or int64 array or a list of node ids, got %s"
                         % (nodes.dtype if isinstance(nodes, np.ndarray) else type(nodes).__name__,))
    if nodes.ndim != 1:
        raise ValueError("nodes must be one-dimensional, got shape %r" % (nodes.shape,))
    if len(nodes) == 0:
        raise ValueError("nodes is empty: name at least one node")
    if nodes.min() < 0 or nodes.max() >= num_nodes:
        raise ValueError("nodes holds an id outside [0, %d)" % num_nodes)
    distinct, inverse = np.unique(nodes, return_inverse=True)
    return distinct.astype(np.int32), inverse.reshape(-1).astype(np.int64), nodes.astype(np.int64)
