#!/usr/bin/env python
"""config layer_dropout: fused (csrc/dropout.hip) against torch, on one MI355X, same build, same process.
  stage_dropout            the layer-input stage of a non-residual layer on one [V, D] tensor: dropout alone
  stage_dropout_residual   the stage of a residual layer after the first: dropout, + last, / 2
                           each forward (autograd recording on) and forward + backward down to the inputs
  kernel_rate              the fused kernels alone at growing tensor sizes: us per launch and GB/s of the bytes each must move,
                           which says what bounds them (a launch floor at small sizes, a bandwidth plateau at large ones; a kernel
                           bound by its integer multiplies would plateau below the copy rate torch.clone reaches on the same tensor)
  train_step_eager         one training step (forward, backward, clip, update) on the fixed batch
  train_step_captured      the same step as one hipGraph, replayed
  step_peak_bytes          torch.cuda.max_memory_allocated of one eager step
  step_launches            device operations (kernels, fills, copies) of one eager step, counted in a profiler context (a run of its own)
at two shapes: the C5 batch of bench_other.py (GNN-FiLM, 23 edge types, D = 128, 10 layers, keep 0.8, residual every 2) and a
PPI-shaped batch (RGCN, D = 256, 4 layers, keep 0.8, residual every 2).  Host clock around work that ends in a device synchronise;
every shape warmed up; the routes alternate ROUNDS times and torch is timed twice per round: the second pass against the first is
the spread a difference has to exceed.  One JSON line per case, also appended to profiles/layer_dropout.jsonl (or --out FILE);
times in microseconds (median [min, max] over the rounds)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from tf_gnn_samples_amd import config, ops
from tf_gnn_samples_amd.graph import check_pending_graph_errors
from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task

dev = torch.device("cuda:0")
ROUNDS = 7
KEEP = 0.8
OUT = ROOT / "profiles" / "layer_dropout.jsonl"
PASSES = (("torch", "torch"), ("fused", "fused"), ("torch_again", "torch"))


def timed_us(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(fns, inner, warm=3):
    """{pass: [us per round]}: fns[route]() warmed up, the routes taking turns within every round."""
    for route in ("torch", "fused"):
        with config.override(layer_dropout=route):
            for _ in range(warm):
                fns[route]()
    ts = {name: [] for name, _ in PASSES}
    for _ in range(ROUNDS):
        for name, route in PASSES:
            with config.override(layer_dropout=route):
                ts[name].append(timed_us(fns[route], inner))
    check_pending_graph_errors()
    return ts


def spread(v):
    s = sorted(v)
    return [round(s[len(s) // 2], 1), round(s[0], 1), round(s[-1], 1)]


def summary(ts):
    return {name + "_us": spread(v) for name, v in ts.items()}


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


def bench_stage(base, V, D):
    """The per-layer input stage alone, as the driver loop writes it on either route."""
    gen = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.randn((V, D), device=dev, generator=gen)
    last0 = torch.randn((V, D), device=dev, generator=gen)
    g = torch.randn((V, D), device=dev, generator=gen)
    state = ops.dropout_state(dev, 0, 0, 1)

    def stage(route, residual, backward):
        def fn():
            x, last = x0.detach().requires_grad_(True), last0.detach().requires_grad_(True)
            if route == "fused":
                if residual:
                    t, cur = ops.dropout_residual(x, last, KEEP, state, 2)
                else:
                    t = cur = ops.dropout(x, KEEP, state, 2)
            else:
                t = cur = torch.nn.functional.dropout(x, p=1.0 - KEEP, training=True)
                if residual:
                    cur = (cur + last) / 2
            if backward:
                if residual:
                    torch.autograd.grad([t, cur], [x, last], [g, g])
                else:
                    torch.autograd.grad([cur], [x], [g])
        return fn

    for residual in (False, True):
        for backward in (False, True):
            ts = alternate({r: stage(r, residual, backward) for r in ("torch", "fused")}, inner=50)
            emit(dict(base, what="stage_dropout_residual" if residual else "stage_dropout",
                      passes="forward_backward" if backward else "forward", rows=V, D=D, **summary(ts)))


def bench_kernel_rate():
    """us per launch and GB/s of the bytes moved for the two forward kernels, against torch.clone (one read + one write) on the
    same tensor: 64 KiB .. 1 GiB per tensor (beyond the 256 MiB Infinity Cache at the top)."""
    state = ops.dropout_state(dev, 0, 0, 1)
    for log2n in (14, 18, 20, 22, 24, 26, 28):
        n = 1 << log2n
        x = torch.randn(n, device=dev)
        last = torch.randn(n, device=dev)
        inner = 200 if log2n <= 22 else 20
        with torch.no_grad():
            cases = {"dropout": (lambda: ops.dropout(x, KEEP, state, 0), 8 * n),
                     "dropout_residual": (lambda: ops.dropout_residual(x, last, KEEP, state, 0), 16 * n),
                     "clone": (lambda: x.clone(), 8 * n)}
            row = {"what": "kernel_rate", "elements": n, "tensor_bytes": 4 * n, "rounds": ROUNDS}
            for fn, _ in cases.values():
                for _ in range(3):
                    fn()
            ts = {name: [] for name in cases}
            for _ in range(ROUNDS):
                for name, (fn, _) in cases.items():
                    ts[name].append(timed_us(fn, inner))
            for name, (_, nbytes) in cases.items():
                us = spread(ts[name])
                row[name + "_us"] = us
                row[name + "_GBps"] = round(nbytes / us[0] / 1e3, 1)
        emit(row)
        del x, last


def bench_steps(base, model_factory, mb):
    model = model_factory()
    batch = DeviceBatch(mb, dev)

    def step():
        model.train_step(batch)
    emit(dict(base, what="train_step_eager", **summary(alternate({"torch": step, "fused": step}, inner=8, warm=6))))

    peaks, counts = {}, {}
    for route in ("torch", "fused"):
        with config.override(layer_dropout=route):
            step()
            model.optimizer.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            step()
            torch.cuda.synchronize()
            peaks[route] = torch.cuda.max_memory_allocated(dev)
            counts[route] = device_operations(step)
    emit(dict(base, what="step_peak_bytes", **peaks))
    emit(dict(base, what="step_launches", **counts))
    del model

    replays = {}
    for route in ("torch", "fused"):
        with config.override(layer_dropout=route):
            m = model_factory()
            replays[route] = m.capture_train_step(DeviceBatch(mb, dev)).replay
    emit(dict(base, what="train_step_captured", **summary(alternate(replays, inner=8, warm=3))))


def c5_case():
    import bench_other
    task, graphs = bench_other.c5_task_and_graphs(42)
    mb = next(task.make_minibatch_iterator(list(graphs), DataFold.VALIDATION, 10 ** 9))

    def factory():
        model, _ = bench_other.c5_model(task, dev)
        assert model.params['graph_layer_input_dropout_keep_prob'] == KEEP
        return model
    base = {"shape": "C5", "model": "GNN-FiLM, 23 edge types, 10 layers, residual every 2, Adam", "hidden": 128, "keep": KEEP,
            "nodes": mb.num_nodes, "edges": mb.num_edges, "rounds": ROUNDS}
    return base, factory, mb


def ppi_case():
    from tf_gnn_samples_amd.models import RGCN_Model
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(16, 1, seed=0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 9))

    def factory():
        p = RGCN_Model.default_params()
        p.update(hidden_size=256, graph_num_layers=4, graph_residual_connection_every_num_layers=2,
                 graph_layer_input_dropout_keep_prob=KEEP)
        return RGCN_Model(p, task, device=str(dev))
    base = {"shape": "PPI", "model": "RGCN, 3 edge types, 4 layers, residual every 2, Adam", "hidden": 256, "keep": KEEP,
            "nodes": mb.num_nodes, "edges": mb.num_edges, "rounds": ROUNDS}
    return base, factory, mb


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    which = [a for a in sys.argv[1:] if a in ("rate", "C5", "PPI")] or ["rate", "C5", "PPI"]
    if "rate" in which:
        bench_kernel_rate()
    for name, case in (("C5", c5_case), ("PPI", ppi_case)):
        if name in which:
            base, factory, mb = case()
            bench_stage(base, mb.num_nodes, base["hidden"])
            bench_steps(base, factory, mb)


if __name__ == "__main__":
    main()
