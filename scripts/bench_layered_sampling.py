#!/usr/bin/env python
"""config layered_sampling: the citation task's sampled batches with and without `"layered": true` (NeighbourSampler.sample_by_hop,
HopSubgraph.device_batch, the level graphs of models/sparse_graph_model.py) on one MI355X, same build, same process, the same seed
lists and the same HopSubgraph through both forms of the batch.
  graph     as scripts/bench_neighbour_sampling.py: V = 2^20 nodes, 17.8 M edges with hubs, 128 dense features, 7 classes
  model     RGCN, hidden 256, Adam, as many layers as fanouts
  --cases   base       fanouts [10, 10], 1024 seeds per batch
            hops3      fanouts [10, 10, 10], 1024 seeds, 3 layers
            seeds8192  fanouts [10, 10], 8192 seeds
            zipf       the sparse-feature shape of scripts/bench_sparse_gradient.py (F = 2^17 words, 32 Zipf-like draws per node) with
                       sparse_features, sparse_update and sparse_gradient on in both models; fanouts [10, 10], 1024 seeds
            (a comma-separated list; the dense cases share one graph, zipf builds its own features and runs alone)
  batches   BATCHES HopSubgraphs, drawn once; "layered" is device_batch(layered=True) of each, "plain" device_batch(layered=False) of the
            same one; "id_order" is sample().device_batch() of the same seed list and draw: the path without this feature.  Both models
            are built from one seed; every model sees one form only.
Reported per case, median [min, max] over ROUNDS rounds that alternate which form goes first:
  sample_us / sample_by_hop_us        wall clock per call, host validation and the one size read-back included, the same seed lists
  graphs_us_union / graphs_us_levels  building the bucketing of the one union graph / of the H level graphs (level 1 is the union graph),
                                      device events; *_wall_us: the host's time for the same
  forward_ms_*, backward_ms_*         a training forward (the graph builds included) and the backward behind it, device events
  step_ms_*                           one whole training step over an epoch of the BATCHES distinct batches, every step building its graphs
  fixed_step_ms_*                     one whole training step on one fixed batch, its graphs cached: what the sampled_step_ms of
                                      profiles/neighbour_sampling.jsonl measures (parent_sampled_step_ms is that file's last record)
  peak_MiB_*                          peak device memory during one step above what is held before it
  rows                                n_0 .. n_H of the batches (mean)
One JSON line per case, also appended to profiles/layered_sampling.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd.graph import RelGraph, clear_graph_cache
from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, BATCHES, FIXED_CALLS = 7, 16, 20
HIDDEN, DRAWS = 256, 32
CASES = {"base": ([10, 10], 1024), "hops3": ([10, 10, 10], 1024), "seeds8192": ([10, 10], 8192), "zipf": ([10, 10], 1024)}
OUT = ROOT / "profiles" / "layered_sampling.jsonl"
FORMS = ("layered", "plain", "id_order")


def med(values, digits=1):
    s = sorted(values)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


class Timer:
    def __init__(self):
        self.start, self.stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        torch.cuda.synchronize()
        self.wall = time.perf_counter()
        self.start.record()
        return self

    def __exit__(self, *exc):
        self.stop.record()
        self.host_us = (time.perf_counter() - self.wall) * 1e6           # the host's time to enqueue
        self.stop.synchronize()
        self.ms = self.start.elapsed_time(self.stop)


def epoch(model, batches):
    """-> (forward ms, backward ms, step ms) per batch over one pass of train_step: timed events in front of and behind the step's
    forward and in front of its clip-and-update split it.  The graph cache is emptied first, so every step builds its graphs as a step
    on a fresh batch does."""
    marks = []
    forward_batch, clip_and_step = model.forward_batch, model.optimizer.clip_and_step

    def mark():
        event = torch.cuda.Event(enable_timing=True)
        event.record()
        marks.append(event)

    def timed_forward(batch, training):
        mark()
        metrics = forward_batch(batch, training)
        mark()
        return metrics

    def timed_update(*args, **kwargs):
        mark()
        return clip_and_step(*args, **kwargs)
    clear_graph_cache()
    model.forward_batch, model.optimizer.clip_and_step = timed_forward, timed_update
    try:
        with Timer() as t:
            for b in batches:
                model.train_step(b)
    finally:
        model.forward_batch, model.optimizer.clip_and_step = forward_batch, clip_and_step
    torch.cuda.synchronize()
    steps = [marks[i:i + 3] for i in range(0, len(marks), 3)]
    assert len(marks) == 3 * len(batches)
    forward = float(np.mean([e[0].elapsed_time(e[1]) for e in steps]))
    backward = float(np.mean([e[1].elapsed_time(e[2]) for e in steps]))
    return forward, backward, t.ms / len(batches)


def fixed_step_ms(model, batch):
    model.train_step(batch)
    with Timer() as t:
        for _ in range(FIXED_CALLS):
            model.train_step(batch)
    return t.ms / FIXED_CALLS


def peak_mib(model, batch):
    model.train_step(batch)
    model.optimizer.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    model.train_step(batch)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, 1)


def build_task(case, V):
    """The task of one case with the fold loaded; cases of one kind share the fold (`shared`)."""
    fanouts, seeds = CASES[case]
    sampled = {"fanouts": fanouts, "seeds_per_batch": seeds, "seed": 0, "layered": True}
    if case != "zipf":
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sampled_batches=sampled))
        task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                            neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
        return task
    F = 2 ** 17 if V == 2 ** 20 else max(64, V // 8)
    sampled.update(sparse_features=True, sparse_update=True, sparse_gradient=True)
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True, sampled_batches=sampled))
    task.load_synthetic(num_nodes=V, num_features=F, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.0, seed=0, hub_nodes=64)
    rng = np.random.default_rng(0)
    rowptr, col = random_rows(rng, V, F, np.full(V, DRAWS), draw=lambda size: (rng.zipf(1.2, size=size) - 1) % F)
    words = np.diff(rowptr)
    host = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / words.astype(np.float32), words), (V, F))
    for which in (DataFold.TRAIN, DataFold.VALIDATION):
        task._loaded_data[which] = [f._replace(node_features=host) for f in task._loaded_data[which]]
    return task


def parent_record():
    path = ROOT / "profiles" / "neighbour_sampling.jsonl"
    if not path.exists():
        return None
    lines = [l for l in path.read_text().splitlines() if l.strip()]
    return json.loads(lines[-1]).get("sampled_step_ms") if lines else None


def run_case(case, task, V):
    fanouts, num_seeds = CASES[case]
    H = len(fanouts)
    task.params["sampled_batches"] = dict(task.params["sampled_batches"], fanouts=fanouts, seeds_per_batch=num_seeds)
    named = bool(task.sparse_gradient)
    fold = task._loaded_data[DataFold.TRAIN][0]
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    sampler = NeighbourSampler(state.sampler.graph, fanouts, seed=0)      # (the state's sampler has the fanouts of the first case)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=H, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    models = {form: RGCN_Model(dict(p), task, device=str(dev)) for form in FORMS}
    rng = np.random.RandomState(0)
    lists = [np.sort(rng.choice(V, size=num_seeds, replace=False)).astype(np.int32) for _ in range(BATCHES)]
    subs = [sampler.sample_by_hop(s, d + 1) for d, s in enumerate(lists)]
    batches = {"layered": [s.device_batch(state.features, state.labels, state.mask, 1.0, named_rows=named, layered=True) for s in subs],
               "plain": [s.device_batch(state.features, state.labels, state.mask, 1.0, named_rows=named, layered=False) for s in subs],
               "id_order": [sampler.sample(s, d + 1).device_batch(state.features, state.labels, state.mask, 1.0, named_rows=named)
                            for d, s in enumerate(lists)]}
    assert all("layer_graphs" in b.extra for b in batches["layered"]) and not any("layer_graphs" in b.extra for b in batches["plain"])
    assert all(a.num_nodes == b.num_nodes and a.num_edges == b.num_edges for a, b in zip(batches["plain"], batches["id_order"]))
    for form in FORMS:                                                   # warm: plans, scratch, the library's handles
        epoch(models[form], batches[form])
    torch.cuda.synchronize()
    print("%s: warm; rows %s" % (case, [round(float(np.mean([s.hop_nodes[d] for s in subs])), 1) for d in range(H + 1)]), flush=True)

    out = {}
    push = lambda key, value: out.setdefault(key, []).append(value)
    for r in range(ROUNDS):
        order = FORMS if r % 2 == 0 else FORMS[::-1]
        for form in order:
            forward, backward, step = epoch(models[form], batches[form])
            push("forward_ms_" + form, forward), push("backward_ms_" + form, backward), push("step_ms_" + form, step)
        for form in order:
            push("fixed_step_ms_" + form, fixed_step_ms(models[form], batches[form][0]))
        for which in (("by_hop", "by_id") if r % 2 == 0 else ("by_id", "by_hop")):
            call = sampler.sample_by_hop if which == "by_hop" else sampler.sample
            torch.cuda.synchronize()
            t = time.perf_counter()
            for d, s in enumerate(lists):
                call(s, d + 1)
            torch.cuda.synchronize()
            push("sample_by_hop_us" if which == "by_hop" else "sample_us", (time.perf_counter() - t) * 1e6 / len(lists))
        for which in (("union", "levels") if r % 2 == 0 else ("levels", "union")):
            device_us, wall_us = [], []
            for s in subs:
                levels = s.level_graphs()
                with Timer() as t:
                    if which == "union":
                        RelGraph(s.adjacency_lists, s.num_nodes, validate="deferred")
                    else:
                        for level in levels:
                            RelGraph(level.adjacency_lists, level.num_sources, validate="deferred")
                device_us.append(t.ms * 1e3), wall_us.append(t.host_us)
            push("graphs_us_" + which, float(np.mean(device_us))), push("graphs_wall_us_" + which, float(np.mean(wall_us)))
    assert not sampler.stamp.any()
    peaks = {form: peak_mib(models[form], batches[form][0]) for form in FORMS}
    row = {"what": "layered_sampling", "case": case, "nodes_in_graph": V, "edges_in_graph": int(sampler.graph.M),
           "features": int(task.initial_node_feature_size), "model": "RGCN, hidden %d, %d layers, Adam" % (HIDDEN, H), "fanouts": fanouts,
           "seeds": num_seeds, "keys": sorted(k for k, v in task.sampled_batches.items() if v is True), "rounds": ROUNDS, "batches": BATCHES,
           "rows": [round(float(np.mean([s.hop_nodes[d] for s in subs])), 1) for d in range(H + 1)],
           "edges": round(float(np.mean([s.num_edges for s in subs])), 1), "parent_sampled_step_ms": parent_record()}
    for key, values in sorted(out.items()):
        row[key] = med(values, 1 if key.endswith("_us") or "_us_" in key else 3)
    for form in FORMS:
        row["peak_MiB_" + form] = peaks[form]
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    del models, batches, subs
    clear_graph_cache()
    torch.cuda.empty_cache()


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    cases = sys.argv[sys.argv.index("--cases") + 1].split(",") if "--cases" in sys.argv else ["base", "hops3", "seeds8192"]
    if any(c not in CASES for c in cases) or ("zipf" in cases and len(cases) > 1):
        raise SystemExit("--cases takes a comma-separated list of %s; zipf runs alone" % sorted(CASES))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    task = build_task(cases[0], V)
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    for case in cases:
        run_case(case, task, V)


if __name__ == "__main__":
    main()
