#!/usr/bin/env python
"""config layerwise_evaluation: a validation epoch of the citation task on the full graph, on exact receptive fields (the `sampled_batches`
key "evaluation") and layer by layer over windows of target rows (`layerwise_evaluation`), on one MI355X, same build, same process,
one model per (case, model).
  graph     as scripts/bench_neighbour_sampling.py: V = 2^20 nodes, 17.8 M edges with hubs (the longest bucket 64 656 entries), 7 classes
  --cases   dense      128 dense features
            zipf       the sparse-feature shape of scripts/bench_sparse_gradient.py (F = 2^17 words, 32 Zipf-like draws per node)
  --models  RGCN_Model (the rectangular route: target rows only), GGNN_Model (a square route: all n rows of a window, T kept); hidden
            256, 2 layers
  forms     full              one full-graph batch (the parent's form)
            exact             "evaluation": {"fanouts": [0, 0], "seeds_per_batch": 1024}: the fold's nodes only
            layerwise_<B>     "layerwise_evaluation": {"rows_per_batch": B}, B = 4 096, 65 536, 262 144
            layerwise_<B>_keep   ... with "keep": true (the first, building epoch is not timed)
Reported, median [min, max] over ROUNDS rounds that alternate the order of the forms:
  validation_ms_<form>    wall clock of one validation epoch of the 65 536-node fold (Sparse_Graph_Model._run_epoch)
  peak_GiB_<form>         the device's peak (allocated bytes) above the resting state over one such epoch
  split_ms_<B>            one layer-wise pass without "keep", summed over its windows and layers: stamp (count, scan and stamp pass),
                          compaction, readback, emit, bucketing (the constructor's two sorts and the routing), gather (the rows of
                          table[block.nodes]), layer (the shared layer step), write_back
A form that runs out of device memory is recorded as null.  One JSON line per record, also appended to profiles/layerwise_evaluation.jsonl
(or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd import models
from tf_gnn_samples_amd.graph import clear_graph_cache
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks import layerwise
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, HIDDEN, DRAWS, SEEDS = 7, 256, 32, 1024
TRAINING = {"fanouts": [10, 10], "seeds_per_batch": SEEDS, "seed": 0}
WINDOWS = (4096, 65536, 262144)
OUT = ROOT / "profiles" / "layerwise_evaluation.jsonl"


def forms(V):
    out = {"full": (None, None), "exact": ({"fanouts": [0, 0], "seeds_per_batch": SEEDS}, None)}
    for B in (B for B in WINDOWS if B < V or B == WINDOWS[0]):
        out["layerwise_%d" % B] = (None, {"rows_per_batch": B})
        out["layerwise_%d_keep" % B] = (None, {"rows_per_batch": B, "keep": True})
    return out


def med(values, digits=2):
    if not values or any(v is None for v in values):
        return None
    s = sorted(values)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


def build_task(case, V):
    sampled = dict(TRAINING)
    valid = min(65536, V // 8)
    if case == "dense":
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sampled_batches=sampled))
        task.load_synthetic(num_nodes=V, num_features=128, num_classes=7, num_train=V // 2, num_valid=valid, num_test=V // 8,
                            neighbours_per_node=8.0, feature_density=0.1, seed=0, hub_nodes=64)
        return task
    F = 2 ** 17 if V == 2 ** 20 else max(64, V // 8)
    sampled["sparse_features"] = True
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True, sampled_batches=sampled))
    task.load_synthetic(num_nodes=V, num_features=F, num_classes=7, num_train=V // 2, num_valid=valid, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.0, seed=0, hub_nodes=64)
    rng = np.random.default_rng(0)
    rowptr, col = random_rows(rng, V, F, np.full(V, DRAWS), draw=lambda size: (rng.zipf(1.2, size=size) - 1) % F)
    words = np.diff(rowptr)
    host = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / words.astype(np.float32), words), (V, F))
    for which in (DataFold.TRAIN, DataFold.VALIDATION):
        task._loaded_data[which] = [f._replace(node_features=host) for f in task._loaded_data[which]]
    task.synthetic_test_data = [f._replace(node_features=host) for f in task.synthetic_test_data]
    return task


def set_form(task, form):
    evaluation, asked = form
    sampled = {k: v for k, v in task.params["sampled_batches"].items() if k != "evaluation"}
    if evaluation is not None:
        sampled["evaluation"] = dict(evaluation)
    task.params["sampled_batches"] = sampled
    task.params.pop("layerwise_evaluation", None)
    if asked is not None:
        task.params["layerwise_evaluation"] = dict(asked)


def epoch(model, data):
    """-> (wall clock ms, peak GiB above the resting state) of one validation epoch."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    t = time.perf_counter()
    model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 30


def guarded(call):
    try:
        return call()
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def validation_record(case, name, task, model, data, V):
    table = forms(V)
    row = {"what": "layerwise_evaluation", "record": "validation_epoch", "case": case, "model": "%s, hidden %d, 2 layers" % (name, HIDDEN),
           "nodes_in_graph": V, "validation_nodes": int(np.count_nonzero(data[0].mask)), "rounds": ROUNDS}
    alive = []
    for form in table:                                             # warm; the kept forms build their blocks
        set_form(task, table[form])
        clear_graph_cache()
        if guarded(lambda: epoch(model, data)) is not None:
            alive.append(form)
        print("%s %s %s: warm" % (case, name, form), flush=True)
    times, peaks = {form: [] for form in table}, {form: [] for form in table}
    for r in range(ROUNDS):
        for form in (alive if r % 2 == 0 else alive[::-1]):
            set_form(task, table[form])
            clear_graph_cache()
            got = guarded(lambda: epoch(model, data))
            times[form].append(None if got is None else got[0])
            peaks[form].append(None if got is None else got[1])
    for form in table:
        row["validation_ms_" + form] = med(times[form]) if form in alive else None
        row["peak_GiB_" + form] = med(peaks[form], 3) if form in alive else None
    task.batches.kept_evaluation.clear()
    task.batches.kept_layerwise.clear()
    torch.cuda.empty_cache()
    return row


def split_record(case, name, task, model, data, V, B):
    """One pass without "keep", every phase behind a timed event: the blocker's own marks, and the driver's three steps around
    _layer_step (patched here for the length of the pass)."""
    set_form(task, (None, {"rows_per_batch": B}))
    (batch,) = model._batches(data, DataFold.VALIDATION)
    trace = []
    layerwise.WindowBlocker.trace = trace
    step = model._layer_step

    def mark(phase):
        event = torch.cuda.Event(enable_timing=True)
        event.record()
        trace.append((phase, event))

    def timed(layer_idx, rows, *args):
        mark("gather")                                             # (behind the block and the index_select of its rows)
        out = step(layer_idx, rows, *args)
        mark("layer")
        return out
    model._layer_step = timed
    try:
        with torch.no_grad():
            mark("start")
            model._final_node_states(batch, training=False)
            mark("write_back")
    finally:
        model._layer_step = step
        layerwise.WindowBlocker.trace = None
    torch.cuda.synchronize()
    sums, previous, behind = {}, None, None
    for phase, event in trace:
        if phase == "start" and previous is not None:
            # a block's start: behind a layer step lies a write-back, behind the pass's own start the input projection and the boundaries
            phase = "write_back" if behind == "layer" else "projection"
        if previous is not None:
            sums[phase] = sums.get(phase, 0.0) + previous.elapsed_time(event)
        previous, behind = event, phase
    return {"what": "layerwise_evaluation", "record": "window_split", "case": case, "model": name, "nodes_in_graph": V,
            "rows_per_batch": B, "windows": -(-V // B), "split_ms": {k: round(v, 2) for k, v in sums.items()}}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    cases = sys.argv[sys.argv.index("--cases") + 1].split(",") if "--cases" in sys.argv else ["dense", "zipf"]
    names = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else ["RGCN_Model", "GGNN_Model"]
    if any(c not in ("dense", "zipf") for c in cases):
        raise SystemExit("--cases takes a comma-separated list of dense, zipf")
    OUT.parent.mkdir(parents=True, exist_ok=True)
    for case in cases:
        t0 = time.time()
        task = build_task(case, V)
        print("%s: graph built in %.1f s" % (case, time.time() - t0), flush=True)
        valid = task._loaded_data[DataFold.VALIDATION]
        for name in names:
            cls = getattr(models, name)
            p = cls.default_params()
            p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
            model = cls(p, task, device=str(dev))
            task.bind_sampling_device(dev)
            emit(validation_record(case, name, task, model, valid, V))
            for B in (B for B in WINDOWS if B < V or B == WINDOWS[0]):
                emit(split_record(case, name, task, model, valid, V, B))
            set_form(task, (None, None))
            model._native_batchers.clear()
            del model
            clear_graph_cache()
            torch.cuda.empty_cache()
        del task, valid


if __name__ == "__main__":
    main()
