#!/usr/bin/env python
"""config sparse_sampling: the citation task with sparse_node_features AND sampled_batches + "sparse_features": true
(csrc/sparse_subset.hip feeding csrc/csr_project.hip) on one MI355X, same build, same process.
  graph     as scripts/bench_neighbour_sampling.py: V = 2^20 nodes, a mean of 16 neighbour entries per node plus a self loop, 2 % of the
            entries redirected to 64 hub nodes: load_synthetic(hub_nodes=64); 7 classes
  features  as the large case of scripts/bench_sparse_features.py: F = 2^17, 32 word draws per node from a Zipf-like distribution,
            row-normalised, one SparseRows for the folds (the dense table would be 512 GiB)
  model     RGCN, 2 layers, hidden 256, Adam
  sampler   fanouts [10, 10], 1024 seeds per batch (drawn from all nodes, a fresh list and a fresh draw per call)
Reported, median [min, max] over ROUNDS alternating rounds:
  take_rows_us           wall clock per SparseRows.take_rows(nodes, validated=True) call, the one size read-back included
  count_us, readback_us, copy_us, transpose_us, plans_us
                         the same calls split by timed events recorded behind each phase (row lengths, per-word counts, plan offsets |
                         the wait for the eight sizes | the entries' copy | radix sort + gather | slabs and combos of both structures)
  sampler_us             NeighbourSampler.sample() per call, for scale
  projection_forward_us, projection_forward_backward_us
                         ops.csr_rows_project on one batch's container (hidden 256, tanh) and the same + the weight gradient
  sampled_step_ms        one training step on a sampled batch over sparse features (the batch fixed, so that only the step is timed)
  full_step_ms           one training step on the full graph over sparse features: how the task trained this shape before
  sampled_step_peak_MiB, full_step_peak_MiB
                         peak device memory during one such step, above what the model, the graph and the container hold
One JSON line, also appended to profiles/sparse_sampling.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd import ops
from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold, DeviceBatch
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS, FULL_CALLS, PROJECTION_CALLS = 7, 20, 20, 3, 50
FANOUTS, SEEDS, HIDDEN, DRAWS = [10, 10], 1024, 256, 32
ACT = ops.activation_id("tanh")
OUT = ROOT / "profiles" / "sparse_sampling.jsonl"


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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, 1)


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    F = int(sys.argv[sys.argv.index("--features") + 1]) if "--features" in sys.argv else 2 ** 17
    OUT.parent.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True,
                                      sampled_batches={"fanouts": FANOUTS, "seeds_per_batch": SEEDS, "seed": 0, "sparse_features": True}))
    task.load_synthetic(num_nodes=V, num_features=F, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.0, seed=0, hub_nodes=64)
    rng = np.random.default_rng(0)
    rowptr, col = random_rows(rng, V, F, np.full(V, DRAWS), draw=lambda size: (rng.zipf(1.2, size=size) - 1) % F)
    words = np.diff(rowptr)
    host = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / words.astype(np.float32), words), (V, F))
    for which in (DataFold.TRAIN, DataFold.VALIDATION):                  # the folds share the one container
        task._loaded_data[which] = [f._replace(node_features=host) for f in task._loaded_data[which]]
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph and features built in %.1f s (%d entries)" % (time.time() - t0, host.nnz), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    sampler, rows = state.sampler, state.features
    assert isinstance(rows, SparseRows) and rows.is_cuda
    rng = np.random.RandomState(0)
    draw = [0]

    def seeds():
        return np.sort(rng.choice(V, size=SEEDS, replace=False)).astype(np.int32)

    def sample(seed_list):
        draw[0] += 1
        return sampler.sample(seed_list, draw[0])

    (mb,) = [b for b in task.make_minibatch_iterator([fold], DataFold.VALIDATION, 10 ** 9)]
    full = DeviceBatch(mb, dev)
    fixed = sample(seeds()).device_batch(rows, state.labels, state.mask, 1.0)
    taken = fixed.extra["sparse_node_features"]
    for _ in range(3):
        model.train_step(fixed)
        rows.take_rows(sample(seeds()).nodes, validated=True)
    model.train_step(full)
    torch.cuda.synchronize()
    print("warm after %.1f s" % (time.time() - t0), flush=True)

    W = (torch.rand((F, HIDDEN), device=dev) * 0.2 - 0.1).requires_grad_(True)
    gout = torch.rand((taken.shape[0], HIDDEN), device=dev) - 0.5

    def projection_forward():
        return ops.csr_rows_project(taken, W, ACT)

    def projection_forward_backward():
        torch.autograd.grad(projection_forward(), [W], gout)
        ops.join_deferred()

    wall, sampler_wall, phases, forward, forward_backward, sampled_step, full_step, sizes = [], [], {}, [], [], [], [], []
    for r in range(ROUNDS):
        lists = [seeds() for _ in range(SAMPLE_CALLS)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        subs = [sample(s) for s in lists]
        torch.cuda.synchronize()
        sampler_wall.append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
        rows.trace = []
        torch.cuda.synchronize()
        t = time.perf_counter()
        containers = [rows.take_rows(s.nodes, validated=True) for s in subs]
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
        trace, rows.trace = rows.trace, None
        spent = {}
        for (_, before), (phase, after) in zip(trace[:-1], trace[1:]):
            if phase != "start":
                spent[phase] = spent.get(phase, 0.0) + before.elapsed_time(after) * 1e3
        for phase, us in spent.items():
            phases.setdefault(phase, []).append(us / SAMPLE_CALLS)
        if r == 0:
            sizes = [(c.shape[0], c.nnz, int(c.rows.slabs.shape[0]), int(c.transposed.slabs.shape[0]), int(c.transposed.combos.shape[0]))
                     for c in containers]
        del subs, containers
        forward.append(timed_ms(projection_forward, PROJECTION_CALLS) * 1e3)
        forward_backward.append(timed_ms(projection_forward_backward, PROJECTION_CALLS) * 1e3)
        sampled_step.append(timed_ms(lambda: model.train_step(fixed), STEP_CALLS))
        full_step.append(timed_ms(lambda: model.train_step(full), FULL_CALLS))
    assert ops.ROUTES["csr_project"] == "hip" and not sampler.stamp.any()
    sampled_peak = peak_mib(lambda: model.train_step(fixed))
    with_take_peak = peak_mib(lambda: model.train_step(sample(seeds()).device_batch(rows, state.labels, state.mask, 1.0)))
    full_peak = peak_mib(lambda: model.train_step(full))
    mean = lambda i: round(float(np.mean([s[i] for s in sizes])), 1)
    row = {"what": "sparse_sampling", "nodes_in_graph": V, "edges_in_graph": int(sampler.graph.M), "features": F, "entries": host.nnz,
           "classes": 7, "model": "RGCN, hidden %d, 2 layers, Adam" % HIDDEN, "fanouts": FANOUTS, "seeds": SEEDS, "rounds": ROUNDS,
           "sample_calls": SAMPLE_CALLS, "size_readbacks_per_take_rows": 1, "nodes": mean(0), "batch_entries": mean(1),
           "batch_slabs": mean(2), "batch_transposed_slabs": mean(3), "batch_transposed_combos": mean(4),
           "fixed_batch_nodes": fixed.num_nodes, "fixed_batch_edges": fixed.num_edges, "fixed_batch_entries": taken.nnz,
           "take_rows_us": med(wall), "sampler_us": med(sampler_wall), "projection_forward_us": med(forward),
           "projection_forward_backward_us": med(forward_backward), "sampled_step_ms": med(sampled_step, 3),
           "full_step_ms": med(full_step, 3), "sampled_step_peak_MiB": sampled_peak, "sample_take_rows_and_step_peak_MiB": with_take_peak,
           "full_step_peak_MiB": full_peak, "dense_rows_of_the_batch_MiB": round(fixed.num_nodes * F * 4 / 2 ** 20, 1)}
    for phase, values in phases.items():
        row[phase + "_us"] = med(values)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
