#!/usr/bin/env python
"""config sampled_evaluation: the citation task's validation epochs, predict(nodes=...) and the peak memory of a train() epoch with and
without the `sampled_batches` key "evaluation" on one MI355X, same build, same process, one model.
  graph     as scripts/bench_neighbour_sampling.py: V = 2^20 nodes, 17.8 M edges with hubs, 7 classes
  --cases   dense      128 dense features
            zipf       the sparse-feature shape of scripts/bench_sparse_gradient.py (F = 2^17 words, 32 Zipf-like draws per node) with
                       sparse_features on
            (a comma-separated list; every case builds its own fold)
  model     RGCN, hidden 256, 2 layers, Adam; training batches: fanouts [10, 10], 1024 seeds
  forms     full          the key absent: one full-graph batch (the resident pipeline's)
            exact         "evaluation": {"fanouts": [0, 0], "seeds_per_batch": 1024}
            exact_keep    ... with "keep": true (the first, building epoch is not timed)
            sampled       "evaluation": {"fanouts": [10, 10], "seeds_per_batch": 1024}
            sampled_keep  ... with "keep": true
Reported, median [min, max] over ROUNDS rounds that alternate the order of the forms:
  validation_ms_<form>     wall clock of one validation epoch (Sparse_Graph_Model._run_epoch: sampling, read-backs and the metric fetch
                           included), for validation folds of 1 024 and 65 536 nodes
  field_<form>             batches per epoch, mean nodes and edges of a batch (the receptive field), the largest batch's nodes
  peak_GiB_*               the device's peak (allocated bytes) behind the training half and behind the whole of one train() epoch
                           (training on sampled batches, then validation); --peak-form FORM runs that one form alone, in a process
                           of its own, and nothing else
  predict_ms_*             predict(test fold) against predict(test fold, nodes=16 / 1 024 random nodes), exact fields
A form that runs out of device memory is recorded as null.  One JSON line per record, also appended to profiles/sampled_evaluation.jsonl
(or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd.graph import clear_graph_cache
from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, HIDDEN, DRAWS, SEEDS = 7, 256, 32, 1024
TRAINING = {"fanouts": [10, 10], "seeds_per_batch": SEEDS, "seed": 0}
FORMS = {"full": None,
         "exact": {"fanouts": [0, 0], "seeds_per_batch": SEEDS},
         "exact_keep": {"fanouts": [0, 0], "seeds_per_batch": SEEDS, "keep": True},
         "sampled": {"fanouts": [10, 10], "seeds_per_batch": SEEDS},
         "sampled_keep": {"fanouts": [10, 10], "seeds_per_batch": SEEDS, "keep": True}}
OUT = ROOT / "profiles" / "sampled_evaluation.jsonl"


def med(values, digits=2):
    if any(v is None for v in values):
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
    sampled = {k: v for k, v in task.params["sampled_batches"].items() if k != "evaluation"}
    if FORMS[form] is not None:
        sampled["evaluation"] = dict(FORMS[form])
    task.params["sampled_batches"] = sampled


def small_fold(fold, count):
    """The first `count` nodes of the fold as a fold of their own: the same adjacency and feature objects, so the same device state."""
    ids = np.flatnonzero(fold.mask)[:count]
    mask = np.zeros_like(fold.mask)
    mask[ids] = 1.0
    return [fold._replace(mask=mask, labels=np.where(mask != 0, fold.labels, 0).astype(np.int32))]


def epoch_ms(model, data):
    torch.cuda.synchronize()
    t = time.perf_counter()
    model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def guarded(call):
    try:
        return call()
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def release(task, kept=True):
    """Between two timed epochs only the graph cache goes (every epoch buckets its batches, as an epoch behind a training epoch
    does); the allocator's blocks stay, as they do in a training loop."""
    if kept:
        task.batches.kept_evaluation.clear()
        torch.cuda.empty_cache()
    clear_graph_cache()


def validation_record(case, task, model, data, V):
    n = int(np.count_nonzero(data[0].mask))
    row = {"what": "sampled_evaluation", "record": "validation_epoch", "case": case, "nodes_in_graph": V, "validation_nodes": n,
           "seeds_per_batch": SEEDS, "model": "RGCN, hidden %d, 2 layers" % HIDDEN, "rounds": ROUNDS}
    alive = []
    for form in FORMS:                                               # warm; the receptive fields; the kept forms build their batches
        set_form(task, form)
        release(task, kept=False)
        if FORMS[form] is not None and not form.endswith("_keep"):        # (a kept form's fields are the un-kept form's)
            sizes = guarded(lambda: [(b.num_nodes, b.num_edges) for b in model._batches(data, DataFold.VALIDATION)])
            release(task, kept=False)
            if sizes is not None:
                row["field_" + form] = {"batches": len(sizes), "mean_nodes": round(float(np.mean([s[0] for s in sizes])), 1),
                                        "mean_edges": round(float(np.mean([s[1] for s in sizes])), 1), "max_nodes": max(s[0] for s in sizes)}
        if guarded(lambda: epoch_ms(model, data)) is not None:
            alive.append(form)
        print("%s n=%d %s: warm %s" % (case, n, form, row.get("field_" + form)), flush=True)
    times = {form: [] for form in FORMS}
    for r in range(ROUNDS):
        for form in (alive if r % 2 == 0 else alive[::-1]):
            set_form(task, form)
            release(task, kept=False)                                # (a kept form keeps its batches between rounds: that is the form)
            times[form].append(guarded(lambda: epoch_ms(model, data)))
    for form in FORMS:
        row["validation_ms_" + form] = med(times[form]) if form in alive else None
    release(task)
    return row


def peak_record(case, task, model, V, form):
    """One whole train() epoch, training then validation, in a process that has run nothing else (--peak-form: the scratch and the
    workspaces a full-graph pass leaves behind would count in every later form's peak)."""
    row = {"what": "sampled_evaluation", "record": "train_epoch_peak", "case": case, "nodes_in_graph": V, "form": form,
           "training_steps": -(-int(np.count_nonzero(task._loaded_data[DataFold.TRAIN][0].mask)) // SEEDS),
           "validation_nodes": int(np.count_nonzero(task._loaded_data[DataFold.VALIDATION][0].mask))}
    set_form(task, form)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    model._run_epoch("training", task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, quiet=True)
    torch.cuda.synchronize()
    row["peak_GiB_training"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    model._run_epoch("validation", task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, quiet=True)
    torch.cuda.synchronize()
    row["peak_GiB_epoch"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    return row


def predict_record(case, task, model, V):
    set_form(task, "exact")
    data = task.synthetic_test_data
    rng = np.random.RandomState(1)
    lists = {16: rng.choice(V, size=16, replace=False), 1024: rng.choice(V, size=1024, replace=False)}
    calls = {"full": lambda: model.predict(data)}
    for m, nodes in lists.items():
        calls["nodes_%d" % m] = lambda nodes=nodes: model.predict(data, nodes=nodes)
    row = {"what": "sampled_evaluation", "record": "predict", "case": case, "nodes_in_graph": V, "rounds": ROUNDS}
    for m, nodes in lists.items():
        sizes = [(b.num_nodes, b.num_edges) for b in task.node_prediction_batches(data, np.sort(nodes).astype(np.int32), [0, 0], SEEDS, True)]
        row["field_nodes_%d" % m] = {"nodes": sizes[0][0], "edges": sizes[0][1]}
    times = {name: [] for name in calls}
    for name, call in calls.items():
        call()
    for r in range(ROUNDS):
        for name in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            calls[name]()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
    for name in calls:
        row["predict_ms_" + name] = med(times[name])
    model._native_batchers.clear()
    release(task)
    return row


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
    records = sys.argv[sys.argv.index("--records") + 1].split(",") if "--records" in sys.argv else ["validation", "predict"]
    peak_form = sys.argv[sys.argv.index("--peak-form") + 1] if "--peak-form" in sys.argv else None
    if peak_form is not None and peak_form not in FORMS:
        raise SystemExit("--peak-form takes one of %s" % sorted(FORMS))
    if any(c not in ("dense", "zipf") for c in cases):
        raise SystemExit("--cases takes a comma-separated list of dense, zipf")
    OUT.parent.mkdir(parents=True, exist_ok=True)
    for case in cases:
        t0 = time.time()
        task = build_task(case, V)
        print("%s: graph built in %.1f s" % (case, time.time() - t0), flush=True)
        p = RGCN_Model.default_params()
        p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
        model = RGCN_Model(p, task, device=str(dev))
        task.bind_sampling_device(dev)
        valid = task._loaded_data[DataFold.VALIDATION]
        if peak_form is not None:
            emit(peak_record(case, task, model, V, peak_form))
            continue
        if "validation" in records:
            for data in (small_fold(valid[0], 1024), valid):
                emit(validation_record(case, task, model, data, V))
                model._native_batchers.clear()
        if "predict" in records:
            emit(predict_record(case, task, model, V))
        del model, task, valid
        clear_graph_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
