#!/usr/bin/env python
"""config graph_partition: the device graph partitioner behind `subgraph_batches`' "sampler": "parts" with the key "partition"
(tasks/graph_partition.py, csrc/graph_partition.hip) on one MI355X: what the partition costs, what it keeps, and what its batches
cost against a random partition's, everything in one process.
  graphs   uniform_hubs: scripts/bench_subgraph_samplers.py's: synthetic, V = 2^20 nodes, a mean of 16 neighbour entries per node plus a
           self loop, 2 % of the entries redirected to 64 hub nodes (Zipf 1.5).  Its endpoints are uniform: there may be little
           locality to find.
           planted: the same nodes, features and folds; V / 1024 communities interleaved by id (node v in community v mod C, so id
           blocks are useless); every node draws 8 neighbours inside its community and 1 anywhere, stored in both directions, plus
           the self loops.
  model    RGCN, 8 layers, hidden 256, Adam
  parts    P = V / 1024, imbalance_percent 10, refine_rounds 8, seed 0; 4 parts a batch, normalised with E = 1
Reported per graph, median [min, max] over ROUNDS rounds (what is compared alternates inside every round):
  partition_ms, grow_ms, fill_ms, refine_ms   wall clock of partition_graph's phases, each closed by a synchronisation; grow_rounds and
                                 readbacks (the grow phase's 4-byte moved count, once per round; nothing else reads back)
  wish_short_us, wish_long_us    one wish pass (refine round 0 over the final partition) over the rows of one wave alone and over the
                                 rows of a workgroup alone (each with the -1 prefill of the entries its class does not write), with
                                 long_rows and long_row_entries, short_row_entries
  computed / random              partition_report of the computed partition and of a random one of EQUAL sizes (the computed labels
                                 permuted): kept_share = kept_entries / entries; sizes min, median, max; then per batch of the first
                                 round nodes and edges (means), sampler_us (SubgraphSampler.sample_nodes, wall clock, the weighting,
                                 host validation and the one size read-back included), batch_us (device_batch() on top) and step_ms
                                 (one training step on a fixed batch)
Nothing about model quality is measured.  One JSON line per graph, also appended to profiles/graph_partition.jsonl (or --out FILE).
--nodes N shrinks the graphs (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks.graph_partition import Partitioner, partition_report
from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler, epoch_node_lists, parse_subgraph_batches, sampler_plan

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS, WISH_CALLS = 7, 20, 20, 10
PART_NODES, PARTS_PER_BATCH, HIDDEN, LAYERS = 1024, 4, 256, 8
OUT = ROOT / "profiles" / "graph_partition.jsonl"


def med(values, digits=1):
    s = sorted(values)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


def timed_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def planted_edges(V, communities, seed=0):
    """-> int32 [E, 2]: every node's 8 draws inside its community (v mod C) and 1 anywhere, each in both directions."""
    rng = np.random.default_rng([seed, 7])
    nodes = np.arange(V, dtype=np.int64)
    inside = rng.integers(0, V // communities, size=(V, 8)) * communities + (nodes % communities)[:, None]
    drawn = np.concatenate([inside, rng.integers(0, V, size=(V, 1))], axis=1)
    pairs = np.stack([np.repeat(nodes, 9), drawn.reshape(-1)], axis=1)
    return np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int32)


def measure(name, task, fold, model, num_parts):
    V = len(fold.labels)
    t0 = time.time()
    state = task.batches.fold_state(fold, dev, "bench-" + name, lambda graph: SubgraphSampler(graph, 0, seed=0))
    graph, sampler = state.sampler.graph, state.sampler
    torch.cuda.synchronize()
    print("%s: device graph in %.1f s, %d entries" % (name, time.time() - t0, graph.M), flush=True)
    n_train = float(np.count_nonzero(fold.mask))
    ends = graph.rowptr_t[::graph.L]
    in_degree = ends[1:] - ends[:-1]

    # ---- the partition itself
    phases = {"partition_ms": [], "grow_ms": [], "fill_ms": [], "refine_ms": []}
    parts = None
    for r in range(ROUNDS + 1):                                   # (the first run warms the allocator and is not counted)
        stats, rounds = {}, Partitioner(graph, num_parts, seed=0)
        out = rounds.run(stats)
        assert parts is None or torch.equal(out, parts)
        parts = out
        if r:
            for key in ("grow_ms", "fill_ms", "refine_ms"):
                phases[key].append(stats[key])
            phases["partition_ms"].append(stats["grow_ms"] + stats["fill_ms"] + stats["refine_ms"])
    row = {"what": "graph_partition", "graph": name, "nodes_in_graph": V, "entries_in_graph": int(graph.M),
           "highest_in_degree": int(in_degree.max()), "num_parts": num_parts, "cap": rounds.cap, "parts_per_batch": PARTS_PER_BATCH,
           "model": "RGCN, hidden %d, %d layers, Adam" % (HIDDEN, LAYERS), "rounds": ROUNDS,
           "grow_rounds": stats["grow_rounds"], "readbacks": stats["readbacks"], **{k: med(v, 2) for k, v in phases.items()}}

    # ---- the wish pass by row class
    room = rounds.room(parts)
    long_row = in_degree > 64
    row.update(long_rows=int(long_row.sum()), long_row_entries=int(in_degree[long_row].sum()), short_row_entries=int(in_degree[~long_row].sum()))
    short_us, long_us = [], []
    for r in range(ROUNDS):
        short_us.append(timed_ms(lambda: rounds.wish(parts, room, 0, classes=1), WISH_CALLS) * 1e3)
        long_us.append(timed_ms(lambda: rounds.wish(parts, room, 0, classes=2), WISH_CALLS) * 1e3)
    row.update(wish_short_us=med(short_us), wish_long_us=med(long_us))

    # ---- against a random partition of equal sizes
    host_parts = parts.cpu().numpy()
    arrays = {"computed": host_parts, "random": host_parts[np.random.RandomState(0).permutation(V)]}
    value = parse_subgraph_batches({"sampler": "parts", "partition": {"num_parts": num_parts}, "parts_per_batch": PARTS_PER_BATCH, "seed": 0,
                                    "normalisation": {"presample_epochs": 1}})
    cap = value["normalisation"]["max_edge_weight"]
    plans, counts, epoch0, fixed = {}, {}, {}, {}

    def batch_of(kind, sub):
        batch = sub.device_batch(state.features, state.labels, state.mask, 1.0)
        batch.extra['loss_normalisation'] = (counts[kind].node_weights(sub.nodes), n_train)
        return batch

    for kind, array in arrays.items():
        report = partition_report(graph, array)
        sizes = np.sort(report["sizes"])
        row[kind] = {"entries": report["entries"], "kept_entries": report["kept_entries"],
                     "kept_share": round(report["kept_entries"] / max(report["entries"], 1), 4),
                     "sizes_min_median_max": [int(sizes[0]), int(sizes[len(sizes) // 2]), int(sizes[-1])]}
        plan = plans[kind] = sampler_plan(value, fold.mask, fold.adjacency_lists, V, partition=lambda array=array: array)
        counts[kind] = sampler.presample_lists(lambda epoch, plan=plan: epoch_node_lists(plan, epoch), 1, plan.longest(), plan.walked)
        epoch0[kind] = epoch_node_lists(plan, 0)
        fixed[kind] = batch_of(kind, sampler.sample_nodes(epoch0[kind][0], (counts[kind], cap)))
    for _ in range(3):
        for kind in arrays:
            model.train_step(fixed[kind])
    torch.cuda.synchronize()
    wall, batch_wall, step = ({kind: [] for kind in arrays} for _ in range(3))
    for r in range(ROUNDS):
        for kind in arrays:
            lists = [epoch0[kind][(r * SAMPLE_CALLS + i) % len(epoch0[kind])] for i in range(SAMPLE_CALLS)]
            torch.cuda.synchronize()
            t = time.perf_counter()
            subs = [sampler.sample_nodes(ids, (counts[kind], cap)) for ids in lists]
            torch.cuda.synchronize()
            wall[kind].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            if r == 0:
                row[kind].update(nodes=round(float(np.mean([s.num_nodes for s in subs])), 1),
                                 edges=round(float(np.mean([s.num_edges for s in subs])), 1))
            t = time.perf_counter()
            for s in subs:
                batch_of(kind, s)
            torch.cuda.synchronize()
            batch_wall[kind].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            del subs
            step[kind].append(timed_ms(lambda: model.train_step(fixed[kind]), STEP_CALLS))
        print("%s: round %d done" % (name, r), flush=True)
    assert not bool(sampler.stamp.any())
    for kind in arrays:
        row[kind].update(sampler_us=med(wall[kind]), batch_us=med(batch_wall[kind]), step_ms=med(step[kind], 3),
                         fixed_batch_nodes=fixed[kind].num_nodes, fixed_batch_edges=fixed[kind].num_edges)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    OUT.parent.mkdir(parents=True, exist_ok=True)
    num_parts = max(V // PART_NODES, PARTS_PER_BATCH)
    t0 = time.time()
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params()))
    task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=LAYERS, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    uniform = task._loaded_data[DataFold.TRAIN][0]
    measure("uniform_hubs", task, uniform, model, num_parts)
    task.batches.graph_states.clear()                             # one graph on the device at a time
    task.batches.fold_states.clear()
    torch.cuda.empty_cache()
    edges = planted_edges(V, max(V // PART_NODES, 1))
    degrees = np.stack([np.ones(V, dtype=np.int32), np.bincount(edges[:, 1], minlength=V).astype(np.int32)])
    planted = uniform._replace(adjacency_lists=[uniform.adjacency_lists[0].copy(), edges], type_to_node_to_num_incoming_edges=degrees)
    measure("planted", task, planted, model, num_parts)


if __name__ == "__main__":
    main()
