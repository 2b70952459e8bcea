"""Layer-wise full-graph evaluation of ONE graph (csrc/window_block.hip, csrc/window_block.h): the windows of target rows, the block of a
window, and the task parameter that asks for it.

The usual companion of sampled training: layer l is computed for ALL nodes, window of target rows by window, from a stored [V, hidden]
table of layer l - 1, and only then layer l + 1 (models/sparse_graph_model.py, layerwise_final_node_representations).  Every node's
state is computed once per layer, as the full-graph forward does, and what is resident is a few [V, hidden] tables and one window's
temporaries.  It is exact: every in-edge of a window's targets is in the window's block.

The block of the window [a, b) of a graph (window_block): its nodes are the targets a .. b - 1 in order, then every source outside the
window in ascending id; its edges are the by-target slice col_t[rowptr_t[a L] .. rowptr_t[b L]) of the full graph's RelGraph, which is
contiguous because the by-target bucketing is target-major.  The device cuts it in two flat passes over that slice and ONE read-back of
L + 1 sizes (the entries per type and the number of outside sources), in front of which no output is allocated.  The block's RelGraph is
the ordinary constructor over the emitted lists (its two sorts), says num_targets = b - a, and is routed as the full graph routes its
reductions when asked (RelGraph.route_like): every bucket of the block is a whole bucket of the full graph in the full graph's order.

`layerwise_evaluation` ({"rows_per_batch": B, "keep": bool}, "keep" optional and false; absent by default, read with params.get, not
part of default_params() and kept in the checkpoint's metadata with the other task parameters): VALIDATION and TEST epochs of train(),
test() and predict(data) / predict_iter(data) without `nodes` take the layer-wise pass over windows of B rows; the head, the loss and the
metrics run once over the whole final table.  It composes with plain full-graph training, `sparse_node_features`, `subgraph_batches`
(every key) and `sampled_batches` (every key but "evaluation": both together are a ValueError).  "keep": the blocks of a (fold, device, B,
route) are built once, reused by every layer and every later epoch, and released with the fold.  GPU only.
"""
import weakref
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..graph import RelGraph
from .neighbour_sampling import StampedNodeSet, integer_at_least, parse_bool_keys, unknown_keys

WINDOW_STAMP = 1                      # csrc/window_block.hip stamps a source outside the window with this one value


def target_windows(num_nodes: int, rows_per_batch: int) -> List[Tuple[int, int]]:
    """The windows [a, b) of `rows_per_batch` target rows that cover 0 .. num_nodes - 1 in order, the last one possibly short."""
    num_nodes = integer_at_least(num_nodes, 1, "target_windows: the graph must have at least one node, got %r")
    rows_per_batch = integer_at_least(rows_per_batch, 1, "target_windows: rows_per_batch must be a positive integer, got %r")
    return [(a, min(a + rows_per_batch, num_nodes)) for a in range(0, num_nodes, rows_per_batch)]


def parse_layerwise_evaluation(value) -> Optional[Dict]:
    """The task parameter `layerwise_evaluation` as {"rows_per_batch": int, "keep": bool}, None when it is absent."""
    if value is None:
        return None
    if not isinstance(value, dict) or "rows_per_batch" not in value or unknown_keys(value, ("rows_per_batch", "keep")):
        raise ValueError('layerwise_evaluation must be {"rows_per_batch": B, "keep": bool}, the last one optional, got %r' % (value,))
    parsed = {"rows_per_batch": integer_at_least(value["rows_per_batch"], 1,
                                                 "layerwise_evaluation: rows_per_batch must be a positive integer, got %r"),
              "keep": False}
    parse_bool_keys("layerwise_evaluation", value, parsed, ("keep",))
    return parsed


def check_layerwise_evaluation(parsed: Optional[Dict], sampled_batches: Optional[Dict]) -> Optional[Dict]:
    """`layerwise_evaluation` against `sampled_batches`: the key "evaluation" names another way to evaluate."""
    if parsed is not None and sampled_batches is not None and "evaluation" in sampled_batches:
        raise ValueError('layerwise_evaluation cannot be combined with the "evaluation" key of sampled_batches: VALIDATION and TEST run '
                         'layer by layer over windows of all nodes, or on sampled receptive fields of the fold\'s nodes, not both')
    return parsed


class WindowBlock(NamedTuple):
    """A LevelGraph of one level (tasks/neighbour_sampling.py: the same first five fields, read by the same layer step) that also says
    which nodes of the full graph its rows are."""
    adjacency_lists: List[torch.Tensor]         # per type int32 [E_l, 2] = (source, target) in local ids, views of one array
    num_sources: int                            # n
    num_targets: int                            # T = last - first
    type_to_num_incoming_edges: torch.Tensor    # float32 [L, n]: the bucket lengths of the targets, 0 behind them
    graph: Optional[RelGraph]                   # the block's bucketing, num_targets = T
    nodes: torch.Tensor                         # int32 [n]: first .. last - 1, then the outside sources ascending
    first: int
    last: int


class WindowBlocker(StampedNodeSet):
    """The window blocks of one device RelGraph (its rowptr_t / col_t are read in place) and its [V] stamp array, all zero between
    calls and after a call that raised.  `trace`: scripts/bench_layerwise_evaluation.py.  `built` counts the blocks cut so far."""

    def __init__(self, graph: RelGraph):
        def refuse_unsupported(lib):
            if not lib.relgnn_window_block_supported(graph.V, graph.L):
                raise ValueError("window blocks do not support a graph of %d nodes and %d edge types (relgnn_window_block_supported)"
                                 % (graph.V, graph.L))
        super().__init__(graph, "the window block", refuse_unsupported, trusts_ids=False)
        self._boundaries = {}                     # B -> the host copy of rowptr_t at the window boundaries of B, read once
        self.built = 0

    def boundaries(self, rows_per_batch: int) -> Dict[int, int]:
        """first or last of a window of `rows_per_batch` -> rowptr_t[that node * L], read back once per (graph, B)."""
        held = self._boundaries.get(int(rows_per_batch))
        if held is None:
            g = self.graph
            ends = sorted({x for window in target_windows(g.V, rows_per_batch) for x in window})
            rows = torch.as_tensor(ends, dtype=torch.int64, device=g.device) * g.L
            held = self._boundaries[int(rows_per_batch)] = dict(zip(ends, g.rowptr_t.index_select(0, rows).tolist()))
        return held

    def block(self, first: int, last: int, route_like: Optional[RelGraph] = None, slice_ends=None) -> WindowBlock:
        """The block of the targets [first, last).  slice_ends: (rowptr_t[first L], rowptr_t[last L]) when the caller holds them
        (boundaries); read back here otherwise."""
        g = self.graph
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in (first, last)) or not 0 <= first < last <= g.V:
            raise ValueError("window_block: [%r, %r) is not a window of 0 <= a < b <= %d" % (first, last, g.V))
        return self._guarded(self._block, int(first), int(last), route_like, slice_ends)

    def _block(self, first: int, last: int, route_like, slice_ends) -> WindowBlock:
        lib, g = _lib.load_library(), self.graph
        V, L, M, dev, T = g.V, g.L, g.M, g.device, last - first
        if slice_ends is None:
            slice_ends = g.rowptr_t.index_select(0, torch.as_tensor([first * L, last * L], dtype=torch.int64, device=dev)).tolist()
        base, entries = int(slice_ends[0]), int(slice_ends[1]) - int(slice_ends[0])
        i32 = lambda n: torch.empty(int(n), dtype=torch.int32, device=dev)
        self._mark("start")
        counts, offsets, summary = i32(T * L + 1), i32(T * L + 1), torch.zeros(L + 1, dtype=torch.int32, device=dev)
        ws_bytes = lib.relgnn_window_block_workspace_bytes(T, L)
        ws = _lib.scratch(ws_bytes, dev)
        window = (_lib.ptr(g.rowptr_t), _lib.ptr(g.col_t) if M else None, V, L, M, first, last, base, entries)
        _lib.launch("relgnn_window_block_count", *window, _lib.ptr(self.stamp), _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(summary),
                    _lib.ptr(ws), ws_bytes)
        self._mark("stamp")
        bound = min(V - T, entries)                                 # the most sources a window can have outside itself
        outside = i32(bound) if bound else None
        if bound:
            self.compact(WINDOW_STAMP, outside, bound, summary[L:])       # (over the closing total, which the host holds: `entries`)
        self._mark("compaction")
        sizes = summary.tolist() if entries else [0] * (L + 1)      # the one read-back of a window; nothing is allocated in front of it
        self._mark("readback")
        type_edges, num_outside = sizes[:L], (sizes[L] if bound else 0)
        if sum(type_edges) != entries or not 0 <= num_outside <= bound:
            raise RuntimeError("window_block: the device counted %r entries and %d outside sources for a slice of %d entries"
                               % (type_edges, num_outside, entries))
        n = T + num_outside
        nodes, edges = i32(n), torch.empty((entries, 2), dtype=torch.int32, device=dev)
        degrees = torch.empty((L, n), dtype=torch.float32, device=dev)
        _lib.launch("relgnn_window_block_emit", *window, _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(outside) if num_outside else None,
                    num_outside, _lib.ptr(self.stamp), _lib.ptr(nodes), n, _lib.ptr(edges) if entries else None, entries,
                    _lib.ptr(degrees), L * n)
        self._mark("emit")
        starts = [sum(type_edges[:l]) for l in range(L + 1)]
        adjacency = [edges[starts[l]:starts[l + 1]] for l in range(L)]
        graph = RelGraph(adjacency, n, validate=False)            # (the ids are local ranks the kernel clamps into [0, n))
        graph.num_targets = T
        if route_like is not None:
            graph.route_like(route_like)
        self._mark("bucketing")
        self.built += 1
        return WindowBlock(adjacency, n, T, degrees, graph, nodes, first, last)


def window_blocker(graph: RelGraph) -> WindowBlocker:
    """The graph's one WindowBlocker (and stamp array), made when first asked for and kept with the graph."""
    held = graph.__dict__.get("_window_blocker")
    if held is None:
        held = graph.__dict__["_window_blocker"] = WindowBlocker(graph)
    return held


def window_block(graph: RelGraph, first: int, last: int, route_like: Optional[RelGraph] = None) -> WindowBlock:
    """The block of the targets [first, last) of the device RelGraph `graph`: a one-level LevelGraph with num_sources = n,
    num_targets = last - first and `nodes`; its graph is bucketed by the ordinary constructor and routed as `route_like` routes."""
    return window_blocker(graph).block(first, last, route_like)


class KeptBlocks:
    """Where the blocks of one fold are kept under `"keep": true`: a WeakKeyedCache of the task (beside kept_evaluation) under the
    fold's label array, so that they are released with the fold.  The fold is held weakly here too: a batch may carry this."""

    def __init__(self, cache, anchor):
        self.cache, self._anchor = cache, weakref.ref(anchor)

    def get(self, key):
        anchor = self._anchor()
        return None if anchor is None else self.cache.get((anchor,), key)

    def put(self, key, blocks):
        anchor = self._anchor()
        if anchor is not None:
            self.cache.put((anchor,), key, blocks)
        return blocks


class LayerwisePlan(NamedTuple):
    """What a full-graph evaluation batch carries under extra['layerwise_evaluation'] when the task asks for the layer-wise pass."""
    rows_per_batch: int
    blocks: Optional[KeptBlocks]                # None: the blocks are rebuilt per layer and dropped
