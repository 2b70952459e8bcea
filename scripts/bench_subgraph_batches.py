#!/usr/bin/env python
"""config subgraph_batches: the citation task's subgraph_batches mode (csrc/subgraph_sample.hip) on one MI355X, same build, same
process, against the two things the task could do with a default-depth model before it.
  graph    scripts/bench_neighbour_sampling.py's: synthetic, V = 2^20 nodes, a mean of 16 neighbour entries per node plus a self loop,
           2 % of the entries redirected to 64 hub nodes (Zipf 1.5): load_synthetic(hub_nodes=64); 128 dense features, 7 classes
  model    RGCN, 8 layers (the default depth), hidden 256, Adam
  sampler  1024 roots per batch (drawn from all nodes, a fresh list and a fresh draw per call), walk length h in {2, 4, 8}
Reported median [min, max] over ROUNDS alternating rounds; per walk length under "h<h>":
  sampler_us             wall clock per SubgraphSampler.sample() call, host validation and the one size read-back included
  walks_us, node_list_us, induced_count_us, readback_us, induced_emit_us
                         the same calls split by timed events recorded behind each phase (the walks | the flag scan that gives the
                         node list and the numbering of the stamps | count, scan, totals | the wait for the sizes | emit in local ids,
                         degree table and stamp reset: the relabelling is part of the emit, there is no pass of its own)
  batch_us               device_batch() on top: the feature / label / mask rows gathered from the device-resident tables
  step_ms, peak_bytes    one training step on a subgraph batch (the batch fixed, so that only the step is timed) and its peak of
                         allocated device memory above the resting state
  nodes, edges           of the subgraph batches (mean over the calls of the first round)
and for the same model on the routes the task had before:
  neighbour_step_ms, neighbour_peak_bytes    the un-layered neighbour-sampled step, fanouts [10, 10], 1024 seeds (a fixed batch)
  full_step_ms, full_peak_bytes              the full-graph step
Nothing about model quality is measured.  One JSON line, also appended to profiles/subgraph_batches.jsonl (or --out FILE).
--nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold, DeviceBatch
from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
from tf_gnn_samples_amd.tasks.subgraph_sampling import SubgraphSampler

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS, FULL_CALLS = 7, 20, 20, 3
WALK_LENGTHS, ROOTS, HIDDEN, LAYERS, FANOUTS = [2, 4, 8], 1024, 256, 8, [10, 10]
OUT = ROOT / "profiles" / "subgraph_batches.jsonl"


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - before)


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    OUT.parent.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(),
                                      subgraph_batches={"roots_per_batch": ROOTS, "walk_length": WALK_LENGTHS[0], "seed": 0}))
    task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=LAYERS, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    state = task.batches.subgraph_state(fold, dev)              # the fold's labels and mask; the graph and the table the folds share
    graph = state.sampler.graph
    samplers = {h: SubgraphSampler(graph, h, seed=0) for h in WALK_LENGTHS}
    neighbour = NeighbourSampler(graph, FANOUTS, seed=0)
    longest = int((graph.rowptr_t[1:] - graph.rowptr_t[:-1]).max())
    rng = np.random.RandomState(0)
    draw = [0]

    def roots():
        return np.sort(rng.choice(V, size=ROOTS, replace=False)).astype(np.int32)

    def sample(sampler, root_list):
        draw[0] += 1
        return sampler.sample(root_list, draw[0])

    batch_of = lambda sub: sub.device_batch(state.features, state.labels, state.mask, 1.0)
    (mb,) = [b for b in task.make_minibatch_iterator([fold], DataFold.VALIDATION, 10 ** 9)]
    full = DeviceBatch(mb, dev)
    fixed = {h: batch_of(sample(samplers[h], roots())) for h in WALK_LENGTHS}
    fixed_neighbour = batch_of(sample(neighbour, roots()))
    for _ in range(3):
        for h in WALK_LENGTHS:
            model.train_step(fixed[h])
            sample(samplers[h], roots())
        model.train_step(fixed_neighbour)
    model.train_step(full)
    torch.cuda.synchronize()

    wall, batch_wall, step = ({h: [] for h in WALK_LENGTHS} for _ in range(3))
    phases, sizes = {h: {} for h in WALK_LENGTHS}, {}
    neighbour_step, full_step = [], []
    for r in range(ROUNDS):
        for h in WALK_LENGTHS:
            sampler = samplers[h]
            lists = [roots() for _ in range(SAMPLE_CALLS)]
            sampler.trace = []
            torch.cuda.synchronize()
            t = time.perf_counter()
            subs = [sample(sampler, s) for s in lists]
            torch.cuda.synchronize()
            wall[h].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            trace, sampler.trace = sampler.trace, None
            spent = {}
            for (_, before), (phase, after) in zip(trace[:-1], trace[1:]):
                if phase != "start":
                    spent[phase] = spent.get(phase, 0.0) + before.elapsed_time(after) * 1e3
            for phase, us in spent.items():
                phases[h].setdefault(phase, []).append(us / SAMPLE_CALLS)
            if r == 0:
                sizes[h] = [(s.num_nodes, s.num_edges) for s in subs]
            t = time.perf_counter()
            for s in subs:
                batch_of(s)
            torch.cuda.synchronize()
            batch_wall[h].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            del subs
            step[h].append(timed_ms(lambda: model.train_step(fixed[h]), STEP_CALLS))
        neighbour_step.append(timed_ms(lambda: model.train_step(fixed_neighbour), STEP_CALLS))
        full_step.append(timed_ms(lambda: model.train_step(full), FULL_CALLS))
    assert not any(s.stamp.any() for s in samplers.values())
    row = {"what": "subgraph_batches", "nodes_in_graph": V, "edges_in_graph": int(graph.M), "longest_bucket": longest,
           "features": 128, "classes": 7, "model": "RGCN, hidden %d, %d layers, Adam" % (HIDDEN, LAYERS), "roots": ROOTS,
           "rounds": ROUNDS, "sample_calls": SAMPLE_CALLS, "size_readbacks_per_call": 1,
           "neighbour_fanouts": FANOUTS, "neighbour_batch_nodes": fixed_neighbour.num_nodes, "neighbour_batch_edges": fixed_neighbour.num_edges,
           "neighbour_step_ms": med(neighbour_step, 3), "neighbour_peak_bytes": peak_bytes(lambda: model.train_step(fixed_neighbour)),
           "full_step_ms": med(full_step, 3), "full_peak_bytes": peak_bytes(lambda: model.train_step(full))}
    for h in WALK_LENGTHS:
        case = {"nodes": round(float(np.mean([n for n, _ in sizes[h]])), 1), "edges": round(float(np.mean([e for _, e in sizes[h]])), 1),
                "fixed_batch_nodes": fixed[h].num_nodes, "fixed_batch_edges": fixed[h].num_edges,
                "sampler_us": med(wall[h]), "batch_us": med(batch_wall[h]), "step_ms": med(step[h], 3),
                "peak_bytes": peak_bytes(lambda: model.train_step(fixed[h]))}
        for phase, values in phases[h].items():
            case[phase + "_us"] = med(values)
        row["h%d" % h] = case
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
