#!/usr/bin/env python
"""Sparse_Graph_Model.predict() against test() on the same fold, on one MI355X, same build, same process: what the predictions cost
beside the forward pass that both run.
  ppi   a PPI-shaped fold of 24 graphs, the README's RGCN (hidden 256, 3 layers, sum aggregation, ReLU), max_nodes_in_batch as
        bench.py sets it for two graphs per batch
  qm9   the C3 batch of bench_other.py: the 256 committed molecules tiled to one 50 000-node batch, GGNN, D = 128, 6 layers, GRU
The calls alternate ROUNDS times after a warm-up of each: test(data); the same evaluation epoch on the list predict() gets (test()
passes a fresh list, which rebuilds the input pipeline); predict(data); predict(data, return_states=True); predict_iter(data)
drained without keeping the results.  A device synchronise in front of and behind every call, host clock around it.  One JSON
line per fold, also appended to profiles/predict.jsonl (or --out FILE); times
in milliseconds (median [min, max] over the rounds)."""
import gzip
import io
import json
import sys
import time
from contextlib import redirect_stdout
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from tf_gnn_samples_amd import ops
from tf_gnn_samples_amd.models import RGCN_Model, name_to_model_class
from tf_gnn_samples_amd.tasks import PPI_Task, QM9_Task

dev = torch.device("cuda:0")
ROUNDS = 7
OUT = ROOT / "profiles" / "predict.jsonl"


def quiet(fn):
    with redirect_stdout(io.StringIO()):
        return fn()


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    s = sorted(v)
    return [round(s[len(s) // 2], 3), round(s[0], 3), round(s[-1], 3)]


def host_shares(model, data):
    """Where the host spends a predict(data) call, from a pass of its own with clocks around two of its parts (median of ROUNDS):
    fetch = waiting for a batch's copy + the copy out of pinned memory, split = the per-graph dicts; the rest of the call is the
    enqueue of the forward and of the prediction kernels (and, behind the last batch, the device finishing them)."""
    from tf_gnn_samples_amd.models import sparse_graph_model as sgm
    acc = {"fetch": 0.0, "split": 0.0}
    arena_fetch, split = sgm._PredictionArena.fetch, model.task.split_predictions

    def clocked(name, fn):
        def wrapper(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kwargs)
            finally:
                acc[name] += (time.perf_counter() - t0) * 1e3
        return wrapper
    rows = {"fetch": [], "split": [], "total": []}
    sgm._PredictionArena.fetch = clocked("fetch", arena_fetch)
    model.task.split_predictions = clocked("split", split)
    try:
        for _ in range(ROUNDS):
            acc.update(fetch=0.0, split=0.0)
            rows["total"].append(timed_ms(lambda: model.predict(data)))
            rows["fetch"].append(acc["fetch"])
            rows["split"].append(acc["split"])
    finally:
        sgm._PredictionArena.fetch = arena_fetch
        del model.task.split_predictions
    return {name: spread(v)[0] for name, v in rows.items()}


def measure(what, model, data, **row):
    def drain():
        for _ in model.predict_iter(data):
            pass
    from tf_gnn_samples_amd.tasks import DataFold
    # (test() hands _run_epoch a fresh list, so every call flattens and uploads the fold again; "epoch_same_list" is the same epoch on
    #  the list predict() gets, whose input pipeline is kept: the like-for-like of predict)
    calls = {"test": lambda: quiet(lambda: model.test(data, quiet=True)),
             "epoch_same_list": lambda: model._run_epoch("Test", data, DataFold.TEST, quiet=True), "predict": lambda: model.predict(data),
             "predict_with_states": lambda: model.predict(data, return_states=True), "predict_iter_drained": drain}
    for fn in calls.values():
        for _ in range(2):
            fn()
    ts = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            ts[name].append(timed_ms(fn))
    assert ops.handover_status(device=dev) == 0
    row.update(host_share_of_predict_ms=host_shares(model, data))
    predictions = model.predict(data, return_states=True)
    out_bytes = sum(a.nbytes for entry in predictions for k, a in entry.items() if k != "node_states")
    state_bytes = sum(entry["node_states"].nbytes for entry in predictions)
    med = {name: spread(v)[0] for name, v in ts.items()}
    row.update(case=what, rounds=ROUNDS, graphs=len(data), **{name + "_ms": spread(v) for name, v in ts.items()},
               predict_over_test=round(med["predict"] / med["test"], 3),
               predict_over_epoch_same_list=round(med["predict"] / med["epoch_same_list"], 3),
               predict_with_states_over_test=round(med["predict_with_states"] / med["test"], 3),
               prediction_bytes=out_bytes, node_state_bytes=state_bytes)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def run_ppi():
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(24, 1, seed=0)
    from tf_gnn_samples_amd.tasks import DataFold
    data = task._loaded_data[DataFold.TRAIN]
    p = RGCN_Model.default_params()
    p.update(hidden_size=256, graph_num_layers=3, graph_num_timesteps_per_layer=1, message_aggregation_function="sum",
             graph_activation_function="ReLU", graph_layer_input_dropout_keep_prob=1.0)
    nodes = sorted(len(g.node_features) for g in data)
    p['max_nodes_in_batch'] = int(sum(nodes) / max(1, len(data) // 2)) + nodes[-1]
    model = quiet(lambda: RGCN_Model(p, task, device=str(dev)))
    measure("ppi", model, data, model_name="RGCN h=256, 3 layers", nodes=sum(nodes), max_nodes_in_batch=p['max_nodes_in_batch'])


def run_qm9():
    with gzip.open(ROOT / "tests" / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
        raw = [json.loads(line) for line in f]
    task = QM9_Task(QM9_Task.default_params())
    samples = task.load_raw(raw * 11)
    taken, nodes = [], 0
    for s in samples:                                          # the graphs of the one 50 000-node batch bench_other.py builds
        if nodes + len(s.node_features) >= 50000:
            break
        taken.append(s)
        nodes += len(s.node_features)
    cls, _ = name_to_model_class("GGNN")
    p = cls.default_params()
    p.update(hidden_size=128, graph_num_layers=6, graph_rnn_cell="GRU", message_aggregation_function="mean", max_nodes_in_batch=50000)
    model = quiet(lambda: cls(p, task, device=str(dev)))
    measure("qm9_c3", model, taken, model_name="GGNN D=128, 6 layers, GRU, mean", nodes=nodes, max_nodes_in_batch=50000)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        OUT = Path(args[args.index("--out") + 1])
        del args[args.index("--out"):args.index("--out") + 2]
    OUT.parent.mkdir(parents=True, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py measures on a GPU; none is visible")
    for name, fn in (("ppi", run_ppi), ("qm9", run_qm9)):
        if not args or name in args:
            fn()
