"""A device graph partitioner for the Cluster-GCN batches of `subgraph_batches`' "sampler": "parts" (csrc/graph_partition.hip,
csrc/graph_partition.h; DESIGN.md section 3 states the rule): a deterministic, balanced, locality-seeking partition of ONE graph,
computed from the by-target bucketing its RelGraph already holds.  Label propagation under a size cap: P anchors drawn on the host
grow their parts over in-neighbours round by round (grow), what no part reached is dealt into the free room (fill), and T rounds in
which a Philox-drawn half of the nodes may move to the part most of their in-neighbours are in (refine).  Every round reads the
round's start (Jacobi) and admits the wishes for a part in ascending node id up to the part's room, so no part ever exceeds
cap = ceil(V (100 + b) / (100 P)); the cap is an upper bound only.  A pure function of (graph, P, seed, b, T).

What runs where: the wish pass (per-node label counting over in-neighbours, hub rows on a workgroup each) is HIP
(relgnn_partition_wish, package-internal: _lib.INTERNAL); the part sizes, the admission and the fill phase are integer torch ops on
the device (stable sort, searchsorted, cumsum).  The only read-back is the grow phase's 4-byte moved count, once per round.  GPU only.
"""
import time
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from .neighbour_sampling import integer_at_least, unknown_keys

MAX_PARTS = 8192                                # the wish pass's LDS count table (relgnn_partition_supported holds the same)
MAX_REFINE_ROUNDS = 64
ELIGIBLE_KEY = 0x10000000                       # the second Philox key word of the refine phase's eligibility draw


def parse_partition(value) -> Dict:
    """The key "partition" of `subgraph_batches` as {"num_parts": P >= 1, "imbalance_percent": 0 .. 100, "refine_rounds": 0 .. 64}
    (the last two optional: 10 and 8), or a ValueError that names the key."""
    what = "subgraph_batches: partition"
    known = ("num_parts", "imbalance_percent", "refine_rounds")
    if not isinstance(value, dict):
        raise ValueError('%s must be {"num_parts": P, "imbalance_percent": b, "refine_rounds": T}, the last two optional, got %r'
                         % (what, value))
    unknown = unknown_keys(value, known)
    if unknown:
        raise ValueError("%s: unknown key %s (known: %s)" % (what, ", ".join(repr(k) for k in unknown), ", ".join(known)))
    if "num_parts" not in value:
        raise ValueError("%s: num_parts is required" % what)
    parsed = {"num_parts": integer_at_least(value["num_parts"], 1, what + ": num_parts must be an integer in [1, %d], got %%r" % MAX_PARTS),
              "imbalance_percent": integer_at_least(value.get("imbalance_percent", 10), 0,
                                                    what + ": imbalance_percent must be an integer in [0, 100], got %r"),
              "refine_rounds": integer_at_least(value.get("refine_rounds", 8), 0,
                                                what + ": refine_rounds must be an integer in [0, %d], got %%r" % MAX_REFINE_ROUNDS)}
    if parsed["num_parts"] > MAX_PARTS:
        raise ValueError("%s: num_parts must be an integer in [1, %d], got %r" % (what, MAX_PARTS, value["num_parts"]))
    if parsed["imbalance_percent"] > 100:
        raise ValueError("%s: imbalance_percent must be an integer in [0, 100], got %r" % (what, value["imbalance_percent"]))
    if parsed["refine_rounds"] > MAX_REFINE_ROUNDS:
        raise ValueError("%s: refine_rounds must be an integer in [0, %d], got %r" % (what, MAX_REFINE_ROUNDS, value["refine_rounds"]))
    return parsed


def partition_cap(num_nodes: int, num_parts: int, imbalance_percent: int) -> int:
    """ceil(V (100 + b) / (100 P)), in integers: no part ever holds more."""
    return -(-int(num_nodes) * (100 + int(imbalance_percent)) // (100 * int(num_parts)))


def partition_anchors(num_nodes: int, num_parts: int, seed: int) -> np.ndarray:
    """The P anchors, int32 ascending, drawn on the host in the style of epoch_node_lists: anchor i starts in part i and never moves."""
    V, P = int(num_nodes), int(num_parts)
    if not 1 <= P <= V:
        raise ValueError("partition_anchors: num_parts must be in [1, num_nodes = %d], got %r" % (V, num_parts))
    return np.sort(np.random.RandomState([int(seed) & 0xffffffff, 4]).choice(V, P, replace=False)).astype(np.int32)


class Partitioner:
    """The rounds of one partition over one device RelGraph (its rowptr_t / col_t are read in place and never written).  The pieces
    are methods so that the tests and scripts/bench_graph_partition.py can run each alone; partition_graph() is the whole."""

    def __init__(self, graph, num_parts: int, seed: int = 0, imbalance_percent: int = 10, refine_rounds: int = 8):
        if torch.device(graph.device).type != "cuda":
            raise ValueError("partition_graph is GPU only: the wish pass is a HIP kernel and there is no CPU fallback (the graph is "
                             "on %s)" % (graph.device,))
        for name, value in (("num_parts", num_parts), ("seed", seed), ("imbalance_percent", imbalance_percent),
                            ("refine_rounds", refine_rounds)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError("partition_graph: %s must be an integer, got %r" % (name, value))
        lib = _lib.load_library()
        V, L = graph.V, graph.L
        if not lib.relgnn_partition_supported(V, L, int(num_parts), int(imbalance_percent), int(refine_rounds)):
            raise ValueError("partition_graph does not support %d nodes, %d edge types, %d parts, imbalance_percent %d, refine_rounds %d "
                             "(relgnn_partition_supported: 1 <= P <= min(V, %d), 0 <= b <= 100, 0 <= T <= %d, V * L < 2^31)"
                             % (V, L, num_parts, imbalance_percent, refine_rounds, MAX_PARTS, MAX_REFINE_ROUNDS))
        self.graph, self.P, self.seed = graph, int(num_parts), int(seed) & 0xffffffff
        self.refine_rounds = int(refine_rounds)
        self.cap = partition_cap(V, self.P, imbalance_percent)
        dev = graph.device
        self.anchors = partition_anchors(V, self.P, self.seed)
        anchors = torch.as_tensor(self.anchors, device=dev).long()
        self.anchor_flag = torch.zeros(V, dtype=torch.int32, device=dev)
        self.anchor_flag[anchors] = 1
        self.start = torch.full((V,), -1, dtype=torch.int32, device=dev)
        self.start[anchors] = torch.arange(self.P, dtype=torch.int32, device=dev)
        # the rows the wave kernel leaves to the workgroup kernel, ascending in front of all others; their count stays on the device
        ends = graph.rowptr_t[::L]
        long_row = (ends[1:] - ends[:-1]) > int(lib.relgnn_partition_wave_row_max())
        self.long_count = long_row.sum(dtype=torch.int32).reshape(1)
        self.long_nodes = torch.sort(~long_row, stable=True).indices.to(torch.int32)
        self.labels = torch.arange(self.P + 1, dtype=torch.int32, device=dev)
        self.positions = torch.arange(V, dtype=torch.int64, device=dev)
        self.readbacks = 0

    def room(self, part: torch.Tensor) -> torch.Tensor:
        """cap - the part sizes of `part`, int32 [P] (a sort and a searchsorted: no atomics, no read-back)."""
        bounds = torch.searchsorted(torch.sort(part).values, self.labels)
        return (self.cap - (bounds[1:] - bounds[:-1])).to(torch.int32)

    def wish(self, part: torch.Tensor, room: torch.Tensor, refine_round: Optional[int] = None, classes: int = 3) -> torch.Tensor:
        """One wish pass (csrc/graph_partition.h): int32 [V], -1 where a node wishes nothing.  refine_round None: the grow phase's
        eligibility.  classes: 1 the rows of one wave, 2 the rows of a workgroup, 3 both (the others' entries stay -1)."""
        g = self.graph
        wish = torch.full((g.V,), -1, dtype=torch.int32, device=g.device) if classes != 3 else torch.empty(g.V, dtype=torch.int32, device=g.device)
        refine = refine_round is not None
        _lib.launch("relgnn_partition_wish", _lib.ptr(g.rowptr_t), _lib.ptr(g.col_t) if g.M else None, g.V, g.L, g.M, _lib.ptr(part),
                    _lib.ptr(room), self.P, _lib.ptr(self.anchor_flag), int(refine), int(refine_round or 0), self.seed,
                    _lib.ptr(self.long_nodes), _lib.ptr(self.long_count), g.V, int(classes), _lib.ptr(wish))
        return wish

    def admit(self, wish: torch.Tensor, room: torch.Tensor) -> torch.Tensor:
        """Who moves, bool [V]: per label the nodes that wish it in ascending id, the first room[label] of them (a stable sort by
        label keeps the ids ascending; a node's rank is its sorted position minus its label's first)."""
        key = torch.where(wish >= 0, wish, self.P)
        sorted_key, order = torch.sort(key, stable=True)
        label = sorted_key.long()
        rank = self.positions - torch.searchsorted(sorted_key, self.labels)[label]
        admitted = rank < torch.cat([room, room.new_zeros(1)])[label]
        return torch.empty_like(admitted).scatter_(0, order, admitted)

    def round(self, part: torch.Tensor, refine_round: Optional[int] = None):
        """One round -> (the new part array, who moved)."""
        room = self.room(part)
        wish = self.wish(part, room, refine_round)
        moved = self.admit(wish, room)
        return torch.where(moved, wish, part), moved

    def grow(self, part: torch.Tensor):
        """Rounds over the unassigned nodes until one moves nobody -> (part, rounds run).  One 4-byte read-back per round."""
        for rounds in range(1, self.graph.V + 2):                 # (every round but the last assigns a node: at most V + 1 of them)
            part, moved = self.round(part)
            self.readbacks += 1
            if int(moved.sum(dtype=torch.int32)) == 0:
                break
        return part, rounds

    def fill(self, part: torch.Tensor) -> torch.Tensor:
        """The k-th node still unassigned, ascending, goes to part searchsorted(cumsum(room), k, side="right")."""
        left = part < 0
        k = torch.cumsum(left, 0) - 1
        target = torch.searchsorted(torch.cumsum(self.room(part).long(), 0), k, right=True)
        return torch.where(left, target.to(torch.int32), part)

    def refine(self, part: torch.Tensor) -> torch.Tensor:
        """T rounds over the Philox-drawn half of the non-anchor nodes; no read-back."""
        if self.P == self.graph.V:                                # every node is an anchor: nobody is eligible, nothing is launched
            return part
        for r in range(self.refine_rounds):
            part, _ = self.round(part, r)
        return part

    def run(self, stats: Optional[dict] = None) -> torch.Tensor:
        """The whole partition.  stats (a dict): filled with the grow rounds run, the read-backs and the phases' wall times in
        milliseconds, each phase closed by a synchronize that a plain call does not make."""
        def timed(name, phase, *args):
            if stats is None:
                return phase(*args)
            torch.cuda.synchronize(self.graph.device)
            t0 = time.perf_counter()
            out = phase(*args)
            torch.cuda.synchronize(self.graph.device)
            stats[name + "_ms"] = (time.perf_counter() - t0) * 1e3
            return out
        part, rounds = timed("grow", self.grow, self.start)
        part = timed("fill", self.fill, part)
        part = timed("refine", self.refine, part)
        if stats is not None:
            stats.update(grow_rounds=rounds, readbacks=self.readbacks)
        return part


def partition_graph(graph, num_parts: int, seed: int = 0, imbalance_percent: int = 10, refine_rounds: int = 8) -> torch.Tensor:
    """The partition of `graph` (a RelGraph on the GPU) into `num_parts` parts: int32 [V] on the graph's device, labels 0 .. P - 1,
    no part empty, none above ceil(V (100 + imbalance_percent) / (100 P)).  np.save of its host copy is a "parts_path" file.  A
    ValueError for a graph on the CPU and for arguments relgnn_partition_supported refuses."""
    return Partitioner(graph, num_parts, seed, imbalance_percent, refine_rounds).run()


def partition_report(graph, parts) -> Dict:
    """How a partition (int32 [V], a tensor or a host array) cuts `graph`: {"sizes": int64 [P] part sizes, "entries": the by-target
    entries whose source is not their target, "kept_entries": those of them whose two ends share a part}.  Reads back; not a hot path."""
    V, L, M, dev = graph.V, graph.L, graph.M, graph.device
    parts = torch.as_tensor(np.asarray(parts) if not isinstance(parts, torch.Tensor) else parts, device=dev).long()
    if parts.shape != (V,):
        raise ValueError("partition_report: parts must have shape (%d,), got %r" % (V, tuple(parts.shape)))
    ends = graph.rowptr_t[::L].long()
    target = torch.repeat_interleave(torch.arange(V, device=dev), ends[1:] - ends[:-1], output_size=M)
    source = torch.div(graph.col_t.long(), L, rounding_mode="floor")
    apart = source != target
    kept = apart & (parts[source] == parts[target])
    sizes = torch.zeros(int(parts.max()) + 1 if V else 0, dtype=torch.int64, device=dev)
    sizes.scatter_add_(0, parts, torch.ones_like(parts))
    return {"sizes": sizes.cpu().numpy(), "entries": int(apart.sum()), "kept_entries": int(kept.sum())}
