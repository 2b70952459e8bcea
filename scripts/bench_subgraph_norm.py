#!/usr/bin/env python
"""config subgraph_norm: the key "normalisation" of the citation task's subgraph_batches (GraphSAINT's loss and aggregation weights:
csrc/subgraph_sample.hip, csrc/train_utils.hip, include/relgnn_subgraph_norm.h) on one MI355X, with and without the key in one process.
  graph    scripts/bench_subgraph_batches.py's: synthetic, V = 2^20 nodes, a mean of 16 neighbour entries per node plus a self loop, 2 % of
           the entries redirected to 64 hub nodes (Zipf 1.5); 128 dense features, 7 classes, a train fold of V / 2 nodes
  model    RGCN, 8 layers, hidden 256, Adam (for the estimator figures: a second one, trained for one epoch of un-normalised batches, then FIXED)
  sampler  1024 roots per batch, walk length 4
Reported median [min, max] over ROUNDS alternating rounds (plain, then normalised, in every round):
  presample_epoch_ms, presample_subgraph_us   SubgraphSampler.presample() for E = 1 (ceil(n_train / 1024) subgraphs), wall clock with a
                                              synchronisation behind it, and the same per subgraph
  sampler_us {plain, weighted}                wall clock per sample() call over the same root lists and draws; the weighted call also
                                              writes the per-edge weights
  emit_us {plain, weighted}                   the emit phase of those calls alone (timed events)
  batch_us {plain, normalised}                device_batch() on top (normalised: the batch's RelGraph is built here, with the preset
                                              scale, and the node weights are gathered; the plain batch leaves the bucketing to the first
                                              layer, inside the step)
  step_ms {plain, normalised}                 one training step on a fixed batch of either kind
  peak_bytes {plain, normalised}              peak of allocated device memory of that step above the resting state
  count_bytes                                 the two count arrays, int32 [V] and int32 [M], held for the life of the sampling state
and the estimator, over the ceil(n_train / 1024) batches of training epoch 0 at the fixed model, in evaluation mode:
  full_graph_loss                             the train fold's masked mean loss on the full graph (what the batches estimate)
  mean_batch_loss {plain, loss_only, normalised, loss_only_E8, normalised_E8}
                                              the mean over the epoch's batches of the batch loss: without the key | with
                                              "aggregation": false | with the key's defaults | the last two with the counts of
                                              E = 8 pre-sampling epochs
Nothing about trained-model quality is measured.  One JSON line, also appended to profiles/subgraph_norm.jsonl (or --out FILE).
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
from tf_gnn_samples_amd.tasks.neighbour_sampling import epoch_seed_batches

dev = torch.device("cuda:0")
ROUNDS, SAMPLE_CALLS, STEP_CALLS = 7, 20, 20
ROOTS, WALK, HIDDEN, LAYERS = 1024, 4, 256, 8
OUT = ROOT / "profiles" / "subgraph_norm.jsonl"


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
    value = {"roots_per_batch": ROOTS, "walk_length": WALK, "seed": 0, "normalisation": {"presample_epochs": 1}}
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), subgraph_batches=value))
    task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=LAYERS, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    model = RGCN_Model(p, task, device=str(dev))
    task.bind_sampling_device(dev)
    t0 = time.time()
    state = task.batches.subgraph_state(fold, dev)              # pre-samples once (the first call also pays the graph's bucketing)
    torch.cuda.synchronize()
    print("sampling state with the counts in %.1f s" % (time.time() - t0), flush=True)
    sampler, counts = state.sampler, state.visit_counts
    graph = sampler.graph
    n_train = float(np.count_nonzero(fold.mask))
    cap = task.subgraph_batches["normalisation"]["max_edge_weight"]
    epoch0 = epoch_seed_batches(fold.mask, ROOTS, 0, 0)

    def batch_of(sub, loss_counts):
        batch = sub.device_batch(state.features, state.labels, state.mask, 1.0)
        if loss_counts is not None:
            batch.extra['loss_normalisation'] = (loss_counts.node_weights(sub.nodes), n_train)
        return batch

    # kind -> (the sampler's weighting, the counts behind the loss weights)
    kinds = {"plain": (None, None), "loss_only": (None, counts), "normalised": ((counts, cap), counts)}
    fixed = {k: batch_of(sampler.sample(epoch0[0], 0, w), lw) for k, (w, lw) in kinds.items()}
    for _ in range(3):
        for k in ("plain", "normalised"):
            model.train_step(fixed[k])
    torch.cuda.synchronize()

    presample, wall, emit, batch_wall, step = [], {"plain": [], "weighted": []}, {"plain": [], "weighted": []}, \
        {"plain": [], "normalised": []}, {"plain": [], "normalised": []}
    for r in range(ROUNDS):
        lists = [epoch0[(r * SAMPLE_CALLS + i) % len(epoch0)] for i in range(SAMPLE_CALLS)]
        for name, weighting, batch_kind in (("plain", None, "plain"), ("weighted", (counts, cap), "normalised")):
            sampler.trace = []
            torch.cuda.synchronize()
            t = time.perf_counter()
            subs = [sampler.sample(s, i, weighting) for i, s in enumerate(lists)]
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            trace, sampler.trace = sampler.trace, None
            spent = sum(before.elapsed_time(after) * 1e3 for (_, before), (phase, after) in zip(trace[:-1], trace[1:]) if phase == "induced_emit")
            emit[name].append(spent / SAMPLE_CALLS)
            t = time.perf_counter()
            for s in subs:
                batch_of(s, counts if weighting is not None else None)
            torch.cuda.synchronize()
            batch_wall[batch_kind].append((time.perf_counter() - t) * 1e6 / SAMPLE_CALLS)
            del subs
            step[batch_kind].append(timed_ms(lambda: model.train_step(fixed[batch_kind]), STEP_CALLS))
        torch.cuda.synchronize()
        t = time.perf_counter()
        again = sampler.presample(fold.mask, ROOTS, 1)
        torch.cuda.synchronize()
        presample.append((time.perf_counter() - t) * 1e3)
        assert again.num_subgraphs == counts.num_subgraphs and torch.equal(again.edge_visits, counts.edge_visits)
        del again
    assert not sampler.stamp.any()
    peaks = {k: peak_bytes(lambda: model.train_step(fixed[k])) for k in ("plain", "normalised")}

    # the estimator at a FIXED model: a second model of the same seed, trained for ONE epoch on the un-normalised batches of epoch 1 (a
    # fresh model gives every node the loss ln(classes), which any weighting averages to the same number; the model above has seen one
    # batch a thousand times), then in evaluation mode over the batches of epoch 0, nothing updated any more
    fixed_model = RGCN_Model(p, task, device=str(dev))
    for i, s in enumerate(epoch_seed_batches(fold.mask, ROOTS, 0, 1)):
        fixed_model.train_step(batch_of(sampler.sample(s, len(epoch0) + i), None))
    counts_8 = sampler.presample(fold.mask, ROOTS, 8)
    kinds["loss_only_E8"], kinds["normalised_E8"] = (None, counts_8), ((counts_8, cap), counts_8)
    with torch.no_grad():
        (mb,) = [b for b in task.make_minibatch_iterator([fold], DataFold.VALIDATION, 10 ** 9)]       # the full graph, the TRAIN fold's mask
        full_loss = float(fixed_model.forward_batch(DeviceBatch(mb, dev), training=False)["loss"])
        means = {}
        for k, (weighting, loss_weights) in kinds.items():
            losses = [float(fixed_model.forward_batch(batch_of(sampler.sample(s, i, weighting), loss_weights), training=False)["loss"])
                      for i, s in enumerate(epoch0)]
            means[k] = float(np.mean(losses))
    row = {"what": "subgraph_norm", "nodes_in_graph": V, "edges_in_graph": int(graph.M), "train_nodes": int(n_train),
           "model": "RGCN, hidden %d, %d layers, Adam" % (HIDDEN, LAYERS), "roots": ROOTS, "walk_length": WALK, "rounds": ROUNDS,
           "presampled_subgraphs": counts.num_subgraphs, "presample_epoch_ms": med(presample, 2),
           "presample_subgraph_us": med([v * 1e3 / counts.num_subgraphs for v in presample]),
           "sampler_us": {k: med(v) for k, v in wall.items()}, "emit_us": {k: med(v) for k, v in emit.items()},
           "batch_us": {k: med(v) for k, v in batch_wall.items()}, "step_ms": {k: med(v, 3) for k, v in step.items()},
           "fixed_batch_nodes": fixed["plain"].num_nodes, "fixed_batch_edges": fixed["plain"].num_edges, "peak_bytes": peaks,
           "count_bytes": int(counts.node_visits.numel() + counts.edge_visits.numel()) * 4,
           "max_node_visits": int(counts.node_visits.max()), "max_edge_visits": int(counts.edge_visits.max()),
           "edges_never_presampled": round(float((counts.edge_visits == 0).float().mean()), 4),
           "estimator_batches": len(epoch0), "full_graph_loss": round(full_loss, 6),
           "mean_batch_loss": {k: round(v, 6) for k, v in means.items()}}
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
