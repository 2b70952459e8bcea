#!/usr/bin/env python
"""config edge_mlp: fused (csrc/edge_mlp_fused.hip) against materialize, on one MI355X, same build, same process.
  product   the fused launch against pair_materialize + the per-type products as they run today (ops.blocked_linear), alone
  layer     one sparse_gnn_edge_mlp_layer forward under no_grad
  step      one training step of GNN_Edge_MLP_Model (1 hidden edge layer), with torch.cuda.max_memory_allocated of the step
on the C2-shaped batch (PPI-shaped, hidden 256, 3 edge types) and on a D = 128 many-type batch (VarMisuse-shaped, 23 edge types), as
scripts/bench_configs.py builds them.  Device events; every shape warmed up; the routes alternate ROUNDS times and the materialize
route is timed twice per round — the second pass against the first is the spread a difference has to exceed.  One JSON line per
case, also appended to profiles/edge_mlp_fused.jsonl; times in microseconds (median [min, max] over the rounds)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from tf_gnn_samples_amd import config, ops
from tf_gnn_samples_amd.gnns import sparse_gnn_edge_mlp_layer
from tf_gnn_samples_amd.gnns.gnn_edge_mlp import gnn_edge_mlp_layer_variables
from tf_gnn_samples_amd.graph import as_rel_graph, clear_graph_cache
from tf_gnn_samples_amd.models import name_to_model_class
from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
from tf_gnn_samples_amd.tasks.synthetic import make_varmisuse_shaped_graphs

dev = torch.device("cuda:0")
ROUNDS = 5
OUT = ROOT / "profiles" / "edge_mlp_fused.jsonl"
PASSES = (("materialize", "materialize"), ("fused", "fused"), ("materialize_again", "materialize"))


def timed_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def alternate(fn, inner=5, warm=3):
    """{pass: [us per round]}: fn() under each route, warmed up, the routes taking turns within every round."""
    for _, route in PASSES[:2]:
        with config.override(edge_mlp=route):
            for _ in range(warm):
                fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in PASSES}
    for _ in range(ROUNDS):
        for name, route in PASSES:
            with config.override(edge_mlp=route):
                ts[name].append(timed_us(fn, inner))
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


def rand(shape, scale=1.0):
    return ((torch.rand(shape, device=dev) * 2 - 1) * scale)


def bench_batch(tag, task, mb, D, model_layers):
    batch = DeviceBatch(mb, dev)
    graph = as_rel_graph(batch.adjacency_lists, mb.num_nodes)
    V, L, M = mb.num_nodes, graph.L, graph.M
    base = {"batch": tag, "nodes": V, "messages": M, "edge_types": L, "D": D, "rounds": ROUNDS}

    # ---- the product alone -----------------------------------------------------------------------------------------------
    P, Q = rand((V * L, D)), rand((V * L, D))
    W = [rand((D, D), 0.1) for _ in range(L)]
    offs = graph.type_offsets

    def product():
        with torch.no_grad():
            if config.settings.edge_mlp == "fused":
                return ops.edge_mlp_first_product(P, Q, graph, "elu", W, None)
            return ops.blocked_linear(ops.pair_materialize(P, Q, graph, "elu"), offs, W)
    with config.override(edge_mlp="fused"):
        a = product()
    b = product()
    row = dict(base, case="product", **summary(alternate(product)))
    row["max_abs_difference"] = float((a - b).abs().max())        # (D = 256: the same arithmetic; D = 128: today's route is torch.mm)
    # algorithmic bytes: gathered rows (P and Q) + the result, and for today's route the hidden tensor written and read back
    row["bytes_fused"] = 4 * M * (2 * D + D) + 8 * M
    row["bytes_materialize"] = row["bytes_fused"] + 2 * 4 * M * D
    row["note"] = "fused gathers the rows once per 128-column chunk (%d chunks); the repeats are counted once" % (D // 128)
    emit(row)
    del P, Q, W, a, b

    # ---- one layer forward -----------------------------------------------------------------------------------------------
    specs = gnn_edge_mlp_layer_variables(L, D, D, True, 1, 1)
    w = {k: (rand(s, 0.05) if "kernel" in k else (torch.ones(s, device=dev) if "gamma" in k else torch.zeros(s, device=dev)))
         for k, (s, _) in specs.items()}
    h = rand((V, D))

    def layer():
        with torch.no_grad():
            return sparse_gnn_edge_mlp_layer(h, batch.adjacency_lists, batch.type_to_num_incoming_edges, D, 1, "ReLU", "sum",
                                             False, True, 1, weights=w)
    emit(dict(base, case="layer_forward", **summary(alternate(layer))))
    del w, h

    # ---- one training step ------------------------------------------------------------------------------------------------
    cls, extra = name_to_model_class("GNN-Edge-MLP1")
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=D, graph_num_layers=model_layers)
    so, sys.stdout = sys.stdout, sys.stderr
    try:
        model = cls(p, task, device="cuda:0")
    finally:
        sys.stdout = so

    def step():
        clear_graph_cache()
        model.train_step(batch)
    row = dict(base, case="train_step", layers=model_layers, **summary(alternate(step, inner=3, warm=4)))
    for route in ("materialize", "fused"):
        with config.override(edge_mlp=route):
            step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            row["max_memory_allocated_" + route] = torch.cuda.max_memory_allocated()
    emit(row)


which = sys.argv[1:] or ["C2", "VM"]
OUT.parent.mkdir(exist_ok=True)
if "C2" in which:
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(16, 1, seed=0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 9))
    bench_batch("C2 PPI-shaped", task, mb, 256, 3)
if "VM" in which:
    graphs = make_varmisuse_shaped_graphs(16, seed=0)
    task = PPI_Task(PPI_Task.default_params())
    task._PPI_Task__num_edge_types = 23; task._PPI_Task__initial_node_feature_size = 128; task._PPI_Task__num_labels = 1
    mb = next(task.make_minibatch_iterator(list(graphs), DataFold.VALIDATION, 10 ** 9))
    bench_batch("VarMisuse-shaped, 16 graphs", task, mb, 128, 3)
