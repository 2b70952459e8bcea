#!/usr/bin/env python
"""config qm9_head: fused (csrc/qm9_head.hip) against compose, on one MI355X, same build, same process.
  head_forward            QM9_Task.compute_task_metrics on the final node states of the batch (autograd recording on)
  head_forward_backward   the same + loss.backward() down to the states and the head's variables
  head_launches           device operations (kernels, fills, copies) of those two, counted in a profiler context (a run of its own)
  train_step_eager        one GGNN training step (forward, backward, clip, RMSProp), bucketing rebuilt per step as bench_other.py does
  train_step_captured     the same step on the fixed batch as one hipGraph, replayed
on the C3 batch of bench_other.py (the 256 committed QM9 molecules tiled to one 50 000-node batch; GGNN, GRU, mean, D = 128, 6 layers)
with T = 1 (task_ids [0]) and T = 13 (all targets).  Host clock around work that ends in a device synchronise; every shape warmed
up; the routes alternate ROUNDS times and compose is timed twice per round: the second pass against the first is the spread a
difference has to exceed.  One JSON line per case, also appended to profiles/qm9_head.jsonl (or --out FILE); times in microseconds
(median [min, max] over the rounds)."""
import gzip
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from tf_gnn_samples_amd import config
from tf_gnn_samples_amd.graph import check_pending_graph_errors, clear_graph_cache
from tf_gnn_samples_amd.models import name_to_model_class
from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, QM9_Task, qm9_task

dev = torch.device("cuda:0")
ROUNDS = 7
OUT = ROOT / "profiles" / "qm9_head.jsonl"
PASSES = (("compose", "compose"), ("fused", "fused"), ("compose_again", "compose"))


def timed_us(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(fns, inner, warm=3):
    """{pass: [us per round]}: fns[route]() warmed up, the routes taking turns within every round."""
    for route in ("compose", "fused"):
        with config.override(qm9_head=route):
            for _ in range(warm):
                fns[route]()
    ts = {name: [] for name, _ in PASSES}
    for _ in range(ROUNDS):
        for name, route in PASSES:
            with config.override(qm9_head=route):
                ts[name].append(timed_us(fns[route], inner))
    check_pending_graph_errors()
    return ts


def summary(ts):
    out = {}
    for name, v in ts.items():
        s = sorted(v)
        out[name + "_us"] = [round(s[len(s) // 2], 1), round(s[0], 1), round(s[-1], 1)]
    return out


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def device_operations(fn):
    """Kernels / fills and copies that fn() puts on the device, from a profiler context."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    if not names:
        raise RuntimeError("the profiler recorded no device activity")
    copies = sum(1 for n in names if "memcpy" in n.lower() or "memset" in n.lower())
    return {"kernels": len(names) - copies, "fills_and_copies": copies}


def bench_tasks(raw, num_tasks):
    p = QM9_Task.default_params()
    p.update(task_ids=list(range(num_tasks)))
    task = QM9_Task(p)
    samples = task.load_raw(raw * 11)
    mb = next(task.make_minibatch_iterator(list(samples), DataFold.VALIDATION, 50000))
    cls, _ = name_to_model_class("GGNN")
    mp = cls.default_params()
    mp.update(hidden_size=128, graph_num_layers=6, graph_rnn_cell="GRU", message_aggregation_function="mean", optimizer="RMSProp")
    base = {"tasks": num_tasks, "nodes": mb.num_nodes, "graphs": mb.num_graphs, "edges": mb.num_edges, "hidden": 128,
            "rounds": ROUNDS, "model": "GGNN, GRU, mean, 6 layers, RMSProp"}
    model = cls(mp, task, device=str(dev))
    batch = DeviceBatch(mb, dev)
    with torch.no_grad():
        final = model.compute_final_node_representations(batch.initial_node_features, batch.adjacency_lists,
                                                         batch.type_to_num_incoming_edges).clone()
    weights = model.variables.scope(model._task_scope)
    head_vars = [v for n, v in ((n, model.variables[n]) for n in model.variables.names()) if "out_layer_task" in n]
    routes = {}

    def forward(route):
        def fn():
            states = final.detach().requires_grad_(True)
            metrics = task.compute_task_metrics(states, batch, weights)
            routes[route] = qm9_task.ROUTES["head"]
            return states, metrics
        return fn

    def forward_backward(route):
        fwd = forward(route)

        def fn():
            states, metrics = fwd()
            torch.autograd.grad(metrics['loss'], [states] + head_vars)
        return fn

    ts = alternate({r: forward(r) for r in ("compose", "fused")}, inner=20)
    assert routes == {"compose": "composition", "fused": "hip"}, routes
    emit(dict(base, what="head_forward", **summary(ts)))
    emit(dict(base, what="head_forward_backward", **summary(alternate({r: forward_backward(r) for r in ("compose", "fused")}, inner=20))))
    counts = {}
    for route in ("compose", "fused"):
        with config.override(qm9_head=route):
            try:
                counts[route] = {"forward": device_operations(forward(route)), "forward_backward": device_operations(forward_backward(route))}
            except Exception as e:                       # (say so instead of a guess)
                counts[route] = "not measured: %r" % (e,)
    emit(dict(base, what="head_launches", **counts))

    def step():
        clear_graph_cache()
        model.train_step(batch)
    emit(dict(base, what="train_step_eager", **summary(alternate({"compose": step, "fused": step}, inner=12, warm=6))))

    replays = {}
    for route in ("compose", "fused"):
        with config.override(qm9_head=route):
            m = cls(mp, task, device=str(dev))
            replays[route] = m.capture_train_step(DeviceBatch(mb, dev)).replay
            assert qm9_task.ROUTES["head"] == routes[route]
    emit(dict(base, what="train_step_captured", **summary(alternate(replays, inner=12, warm=3))))


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with gzip.open(ROOT / "tests" / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
        raw = [json.loads(line) for line in f]
    for num_tasks in (1, 13):
        bench_tasks(raw, num_tasks)


if __name__ == "__main__":
    main()
