#!/usr/bin/env python
"""config neighbour_sampling: the citation task's sampled_batches mode (csrc/neighbour_sample.hip) on one MI355X, same build, same
process.
  graph    synthetic, V = 2^20 nodes, a mean of 16 neighbour entries per node (8 neighbour-list entries, both directions) plus a self
           loop, 2 % of the entries redirected to 64 hub nodes (Zipf 1.5): load_synthetic(hub_nodes=64); 128 dense features, 7 classes
  model    RGCN, 2 layers, hidden 256, Adam
  sampler  fanouts [10, 10], 1024 seeds per batch (drawn from all nodes, a fresh list and a fresh draw per call)
Reported per case, median [min, max] over ROUNDS alternating rounds:
  sampler_us             wall clock per NeighbourSampler.sample() call, host validation and the one size read-back included
  hops_us, compaction_us, readback_us, relabel_us
                         the same calls split by timed events recorded behind each phase (count + take | the flag scans that give the
                         next frontier and the node list | the wait for the sizes | relabel, degree table, seed mask and stamp reset)
  batch_us               device_batch() on top: the feature / label / mask rows gathered from the device-resident tables
  sampled_step_ms        one training step on a sampled batch (the batch fixed, so that only the step is timed)
  full_step_ms           one training step on the full graph, for scale
  nodes, edges           of the sampled batches (mean over the calls of the first round)
One JSON line, also appended to profiles/neighbour_sampling.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
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

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS, FULL_CALLS = 7, 20, 20, 3
FANOUTS, SEEDS, HIDDEN = [10, 10], 1024, 256
OUT = ROOT / "profiles" / "neighbour_sampling.jsonl"


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
    t0 = time.time()
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(),
                                      sampled_batches={"fanouts": FANOUTS, "seeds_per_batch": SEEDS, "seed": 0}))
    task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    sampler = state.sampler
    rowptr = sampler.graph.rowptr_t
    longest = int((rowptr[1:] - rowptr[:-1]).max())
    rng = np.random.RandomState(0)
    draw = [0]

    def seeds():
        return np.sort(rng.choice(V, size=SEEDS, replace=False)).astype(np.int32)

    def sample(seed_list):
        draw[0] += 1
        return sampler.sample(seed_list, draw[0])

    (mb,) = [b for b in task.make_minibatch_iterator([fold], DataFold.VALIDATION, 10 ** 9)]
    full = DeviceBatch(mb, dev)
    fixed = sample(seeds()).device_batch(state.features, state.labels, state.mask, 1.0)
    for _ in range(3):
        model.train_step(fixed)
        sample(seeds())
    model.train_step(full)
    torch.cuda.synchronize()

    wall, batch_wall, phases, sampled_step, full_step, sizes = [], [], {}, [], [], []
    for r in range(ROUNDS):
        lists = [seeds() for _ in range(SAMPLE_CALLS)]
        sampler.trace = []
        torch.cuda.synchronize()
        t = time.perf_counter()
        subs = [sample(s) for s in lists]
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
        trace, sampler.trace = sampler.trace, None
        spent = {}
        for (_, before), (phase, after) in zip(trace[:-1], trace[1:]):
            if phase != "start":
                spent[phase] = spent.get(phase, 0.0) + before.elapsed_time(after) * 1e3
        for phase, us in spent.items():
            phases.setdefault(phase, []).append(us / SAMPLE_CALLS)
        if r == 0:
            sizes = [(s.num_nodes, s.num_edges) for s in subs]
        t = time.perf_counter()
        for s in subs:
            s.device_batch(state.features, state.labels, state.mask, 1.0)
        torch.cuda.synchronize()
        batch_wall.append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
        del subs
        sampled_step.append(timed_ms(lambda: model.train_step(fixed), STEP_CALLS))
        full_step.append(timed_ms(lambda: model.train_step(full), FULL_CALLS))
    assert not sampler.stamp.any()
    row = {"what": "neighbour_sampling", "nodes_in_graph": V, "edges_in_graph": int(sampler.graph.M), "longest_bucket": longest,
           "features": 128, "classes": 7, "model": "RGCN, hidden %d, 2 layers, Adam" % HIDDEN, "fanouts": FANOUTS, "seeds": SEEDS,
           "rounds": ROUNDS, "sample_calls": SAMPLE_CALLS, "hop_syncs": len(sampler.synced_hops), "size_readbacks_per_call": 1,
           "nodes": round(float(np.mean([n for n, _ in sizes])), 1), "edges": round(float(np.mean([e for _, e in sizes])), 1),
           "fixed_batch_nodes": fixed.num_nodes, "fixed_batch_edges": fixed.num_edges,
           "sampler_us": med(wall), "batch_us": med(batch_wall), "sampled_step_ms": med(sampled_step, 3), "full_step_ms": med(full_step, 3)}
    for phase, values in phases.items():
        row[phase + "_us"] = med(values)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
