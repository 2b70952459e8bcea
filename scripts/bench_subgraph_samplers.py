#!/usr/bin/env python
"""config subgraph_samplers: the key "sampler" of the citation task's subgraph_batches ("walk" | "node" | "edge" | "parts";
tasks/subgraph_sampling.py: sampler_plan, epoch_node_lists, SubgraphSampler.sample / sample_nodes / presample_lists) on one MI355X, the
four samplers in one process over one device graph.  No kernel differs between them: a batch is relgnn_subgraph_walk or
relgnn_neighbour_sample_begin in front of the same induced path, so what is compared is the node set each sampler brings to that path.
  graph    scripts/bench_subgraph_batches.py's: synthetic, V = 2^20 nodes, a mean of 16 neighbour entries per node plus a self loop, 2 % of
           the entries redirected to 64 hub nodes (Zipf 1.5; the longest by-target bucket is reported); 128 dense features, 7 classes,
           a train fold of V / 2 nodes
  model    RGCN, 8 layers, hidden 256, Adam
  samplers walk: 1024 roots, walk length 4 | node: 1024 draws | edge: 1024 roots, one step | parts: V / 1024 parts of 1024 nodes each
           (node v in part perm(v) mod P: a random partition keeps few edges; a computed one: scripts/bench_graph_partition.py), 4 parts a batch
Every sampler runs normalised (E = 1 pre-sampling epoch, "aggregation": true): the three graph-wide ones require the key.
Reported per sampler, median [min, max] over ROUNDS alternating rounds (the four samplers in turn in every round):
  nodes, edges, longest_bucket   of the batches of the first round (means; longest_bucket: the largest induced in-degree of a batch, the
                                 bucket ONE wave walks in the count and the emit), and hub_share: the share of those batches that
                                 hold the graph's highest in-degree node
  host_draw_us                   epoch_node_lists() of one epoch on the host, per batch
  sampler_us                     wall clock per sample() / sample_nodes() call with the weighting, host validation and the one
                                 size read-back included
  walks_us, node_list_us, induced_count_us, readback_us, induced_emit_us
                                 the same calls split by timed events behind each phase ("walks": whatever stamps the set, the walk
                                 kernel or begin)
  batch_us                       device_batch() on top, with the batch's RelGraph and the preset per-edge weights, and the node weights
  step_ms                        one training step on a fixed batch of the sampler's
  presample_subgraph_us          presample_lists() for E = 1, wall clock with a synchronisation behind it, per pre-sampled subgraph
Nothing about model quality is measured.  One JSON line, also appended to profiles/subgraph_samplers.jsonl (or --out FILE).
--nodes N shrinks the graph (a dry run)."""
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks.subgraph_sampling import (SAMPLERS, SubgraphSampler, epoch_node_lists, parse_subgraph_batches,
                                                         sampler_plan)

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS = 7, 20, 20
ROOTS, WALK, PART_NODES, PARTS_PER_BATCH, HIDDEN, LAYERS = 1024, 4, 1024, 4, 256, 8
NORMALISATION = {"presample_epochs": 1}
OUT = ROOT / "profiles" / "subgraph_samplers.jsonl"


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


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    OUT.parent.mkdir(parents=True, exist_ok=True)
    scratch = tempfile.TemporaryDirectory()
    parts_path = str(Path(scratch.name) / "parts.npy")
    num_parts = max(V // PART_NODES, PARTS_PER_BATCH)
    np.save(parts_path, (np.random.RandomState(0).permutation(V) % num_parts).astype(np.int32))
    values = {"walk": {"roots_per_batch": ROOTS, "walk_length": WALK},
              "node": {"roots_per_batch": ROOTS}, "edge": {"roots_per_batch": ROOTS},
              "parts": {"parts_path": parts_path, "parts_per_batch": PARTS_PER_BATCH}}
    values = {name: dict(value, sampler=name, seed=0, normalisation=dict(NORMALISATION)) for name, value in values.items()}
    t0 = time.time()
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), subgraph_batches=values["walk"]))
    task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=LAYERS, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    t0 = time.time()
    state = task.batches.subgraph_state(fold, dev)              # the walk sampler's state: the device graph, the table, labels and mask
    torch.cuda.synchronize()
    print("the walk sampler's state with its counts in %.1f s" % (time.time() - t0), flush=True)
    graph = state.sampler.graph
    n_train = float(np.count_nonzero(fold.mask))
    in_degree = (graph.rowptr_t[graph.L::graph.L] - graph.rowptr_t[:-1:graph.L])
    top = int(in_degree.argmax())
    cap = task.subgraph_batches["normalisation"]["max_edge_weight"]

    plans, samplers, counts = {}, {}, {}
    for name in SAMPLERS:
        t0 = time.time()
        plans[name] = sampler_plan(parse_subgraph_batches(values[name]), fold.mask, fold.adjacency_lists, V)
        steps = WALK if name == "walk" else plans[name].walk_steps
        samplers[name] = state.sampler if name == "walk" else SubgraphSampler(graph, steps, seed=0)
        print("%s: plan in %.1f s, %d batches an epoch" % (name, time.time() - t0, plans[name].batches_per_epoch()), flush=True)

    def presample(name):
        plan = plans[name]
        return samplers[name].presample_lists(lambda epoch: epoch_node_lists(plan, epoch), 1, plan.longest(), plan.walked)

    def sample(name, ids, draw):
        weighting = (counts[name], cap)
        return samplers[name].sample(ids, draw, weighting) if plans[name].walked else samplers[name].sample_nodes(ids, weighting)

    def batch_of(name, sub):
        batch = sub.device_batch(state.features, state.labels, state.mask, 1.0)
        batch.extra['loss_normalisation'] = (counts[name].node_weights(sub.nodes), n_train)
        return batch

    epoch0, fixed = {}, {}
    for name in SAMPLERS:
        counts[name] = state.visit_counts if name == "walk" else presample(name)
        epoch0[name] = epoch_node_lists(plans[name], 0)
        fixed[name] = batch_of(name, sample(name, epoch0[name][0], 0))
    for _ in range(3):
        for name in SAMPLERS:
            model.train_step(fixed[name])
    torch.cuda.synchronize()

    new = lambda: {name: [] for name in SAMPLERS}
    host, wall, batch_wall, step, presampled = new(), new(), new(), new(), new()
    phases, sizes = {name: {} for name in SAMPLERS}, {}
    for r in range(ROUNDS):
        for name in SAMPLERS:
            sampler, lists_of_epoch = samplers[name], epoch0[name]
            t = time.perf_counter()
            drawn = epoch_node_lists(plans[name], 1 + r)
            host[name].append((time.perf_counter() - t) * 1e6 / len(drawn))
            lists = [lists_of_epoch[(r * SAMPLE_CALLS + i) % len(lists_of_epoch)] for i in range(SAMPLE_CALLS)]
            sampler.trace = []
            torch.cuda.synchronize()
            t = time.perf_counter()
            subs = [sample(name, ids, i) for i, ids in enumerate(lists)]
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            trace, sampler.trace = sampler.trace, None
            spent = {}
            for (_, before), (phase, after) in zip(trace[:-1], trace[1:]):
                if phase != "start":
                    spent[phase] = spent.get(phase, 0.0) + before.elapsed_time(after) * 1e3
            for phase, us in spent.items():
                phases[name].setdefault(phase, []).append(us / SAMPLE_CALLS)
            if r == 0:
                sizes[name] = [(s.num_nodes, s.num_edges, float(s.type_to_num_incoming_edges.max()), bool((s.nodes == top).any()))
                               for s in subs]
            t = time.perf_counter()
            for s in subs:
                batch_of(name, s)
            torch.cuda.synchronize()
            batch_wall[name].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            del subs
            step[name].append(timed_ms(lambda: model.train_step(fixed[name]), STEP_CALLS))
            torch.cuda.synchronize()
            t = time.perf_counter()
            again = presample(name)
            torch.cuda.synchronize()
            presampled[name].append((time.perf_counter() - t) * 1e6 / again.num_subgraphs)
            assert again.num_subgraphs == counts[name].num_subgraphs and torch.equal(again.edge_visits, counts[name].edge_visits)
            del again
        print("round %d done" % r, flush=True)
    assert not any(bool(samplers[name].stamp.any()) for name in SAMPLERS)

    row = {"what": "subgraph_samplers", "nodes_in_graph": V, "edges_in_graph": int(graph.M), "train_nodes": int(n_train),
           "longest_bucket_in_graph": int((graph.rowptr_t[1:] - graph.rowptr_t[:-1]).max()), "highest_in_degree": int(in_degree.max()),
           "model": "RGCN, hidden %d, %d layers, Adam" % (HIDDEN, LAYERS), "roots": ROOTS, "walk_length": WALK, "num_parts": num_parts,
           "parts_per_batch": PARTS_PER_BATCH, "rounds": ROUNDS, "calls_per_round": SAMPLE_CALLS}
    for name in SAMPLERS:
        held = np.asarray([s[:3] for s in sizes[name]], np.float64)
        row[name] = {"batches_per_epoch": plans[name].batches_per_epoch(), "presampled_subgraphs": counts[name].num_subgraphs,
                     "nodes": round(float(held[:, 0].mean()), 1), "edges": round(float(held[:, 1].mean()), 1),
                     "longest_bucket": round(float(held[:, 2].mean()), 1), "hub_share": round(float(np.mean([s[3] for s in sizes[name]])), 3),
                     "host_draw_us": med(host[name]), "sampler_us": med(wall[name]),
                     **{"%s_us" % phase: med(v) for phase, v in phases[name].items()},
                     "batch_us": med(batch_wall[name]), "step_ms": med(step[name], 3),
                     "fixed_batch_nodes": fixed[name].num_nodes, "fixed_batch_edges": fixed[name].num_edges,
                     "presample_subgraph_us": med(presampled[name])}
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    scratch.cleanup()


if __name__ == "__main__":
    main()
