#!/usr/bin/env python
"""The fused RMSProp update (relgnn_mt_l2norm + relgnn_mt_rmsprop_clip behind TFStyleOptimizer.clip_and_step) against the foreach
restatement (clip_gradients(); step()), on one MI355X, same build, same process:
  update      the update alone on the variable sets of the BASELINE C3 model (GGNN / QM9, D = 128, 6 layers, optimizer RMSProp) and
              of the C2 model (RGCN / PPI, D = 256, 3 layers): CALLS calls between two device events per sample, the two forms
              taking turns, SAMPLES samples each; host time per call next to it (the update is launches and host time, not bytes)
  eager_step  the eager C3 training step (bench_other.py's loop: bucketing rebuilt per step) with the fused update, and in the same
              process with the update forced onto the foreach restatement, taking turns
  captured    the same C3 RMSProp step recorded as one hipGraph, per replay
One JSON line per measurement (microseconds / milliseconds: median [min, max] over the samples), also appended to
profiles/optimizer_fused.jsonl.  `--step-loop-only` runs nothing but the eager step loop with the update the checkout has: the
way to take the `eager_step` figure of a commit from before the fused update with the same loop.  There is no CPU fallback."""
import gzip
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

if not torch.cuda.is_available():
    raise SystemExit("bench_optimizer_update.py needs an MI355X: the fused update has no CPU form to measure")

from tf_gnn_samples_amd.graph import clear_graph_cache
from tf_gnn_samples_amd.models import name_to_model_class
from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task, QM9_Task

dev = torch.device("cuda:0")
CALLS, SAMPLES = 200, 7
STEPS, STEP_SAMPLES = 24, 5
OUT = ROOT / "profiles" / "optimizer_fused.jsonl"
STEP_LOOP_ONLY = "--step-loop-only" in sys.argv[1:]


def quiet(fn):
    so, sys.stdout = sys.stdout, sys.stderr
    try:
        return fn()
    finally:
        sys.stdout = so


def spread(v, digits):
    s = sorted(v)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if not STEP_LOOP_ONLY:
        OUT.parent.mkdir(exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


def c3_model_and_batch():
    with gzip.open(ROOT / "tests" / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
        raw = [json.loads(line) for line in f]
    task = QM9_Task(QM9_Task.default_params())
    samples = task.load_raw(raw * 11)
    mb = next(task.make_minibatch_iterator(list(samples), DataFold.VALIDATION, 50000))
    cls, extra = name_to_model_class("GGNN")
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=128, graph_num_layers=6, graph_rnn_cell="GRU", message_aggregation_function="mean", optimizer="RMSProp")
    return quiet(lambda: cls(p, task, device=str(dev))), mb, DeviceBatch(mb, dev)


def c2_model():
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(1, 1, seed=0)                  # (the variable set does not depend on the graphs)
    cls, extra = name_to_model_class("RGCN")
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=256, graph_num_layers=3, graph_num_timesteps_per_layer=1, message_aggregation_function="sum",
             graph_activation_function="ReLU", optimizer="RMSProp")
    return quiet(lambda: cls(p, task, device=str(dev)))


def timed(fn, calls):
    """(device microseconds per call between two events, host microseconds per call spent enqueuing)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3, host / calls * 1e6


def bench_update(tag, model):
    """The update alone on copies of the model's variables with fixed random gradients (every other one clipped)."""
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.optimizer.params]
    opt = TFStyleOptimizer(params, "RMSProp", 1e-3, 1.0, decay=0.98, momentum=0.85)
    for i, p in enumerate(params):
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * (5.0 if i % 2 == 0 else 0.01)
    forms = {"fused": lambda: opt.clip_and_step(), "foreach": lambda: (opt.clip_gradients(), opt.step())}
    for fn in forms.values():
        for _ in range(10):
            fn()
    ts = {k: ([], []) for k in forms}
    for _ in range(SAMPLES):
        for k, fn in forms.items():
            d, h = timed(fn, CALLS)
            ts[k][0].append(d)
            ts[k][1].append(h)
    row = {"case": "update", "variables_of": tag, "optimizer": "RMSProp", "variables": len(params),
           "elements": sum(p.numel() for p in params), "calls_per_sample": CALLS, "samples": SAMPLES}
    for k in forms:
        row[k + "_us"] = spread(ts[k][0], 1)
        row[k + "_host_us"] = spread(ts[k][1], 1)
    row["what"] = "microseconds per call, median [min, max] over the samples; *_us between device events, *_host_us the host's enqueue time"
    emit(row)


def step_loop_ms(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_c3_steps():
    import gc
    model, mb, batch = c3_model_and_batch()
    gc.collect()
    gc.freeze()
    opt = model.optimizer
    base = {"config": "C3 GGNN / QM9 (real molecules), GRU, mean aggregation, D=128, 6 layers", "optimizer": "RMSProp",
            "nodes": mb.num_nodes, "edges": mb.num_edges, "steps_per_sample": STEPS, "samples": STEP_SAMPLES}

    def step():
        clear_graph_cache()
        model.train_step(batch)

    if STEP_LOOP_ONLY:
        for _ in range(6):
            step()
        emit(dict(base, case="eager_step_of_this_checkout", train_ms=spread([step_loop_ms(step, STEPS) for _ in range(STEP_SAMPLES)], 3)))
        return

    def foreach_update(lr_scale=1.0, device_step_count=False):
        opt.clip_gradients()
        opt.step(lr_scale)

    ts = {"fused": [], "foreach": []}
    for _ in range(6):
        step()
    for _ in range(STEP_SAMPLES):
        for k in ts:
            if k == "foreach":
                opt.clip_and_step = foreach_update       # (what clip_and_step did for RMSProp before the fused update)
            try:
                step()
                ts[k].append(step_loop_ms(step, STEPS))
            finally:
                opt.__dict__.pop("clip_and_step", None)
    emit(dict(base, case="eager_step", train_ms_fused=spread(ts["fused"], 3), train_ms_foreach=spread(ts["foreach"], 3),
              what="milliseconds per step, median [min, max]; the two updates take turns in one process"))

    cap = model.capture_train_step(batch)
    for _ in range(3):
        cap.replay()
    ms = [step_loop_ms(cap.replay, STEPS) for _ in range(STEP_SAMPLES)]
    assert cap.handover_status() == 0
    emit(dict(base, case="captured", train_ms_hipgraph=spread(ms, 3),
              what="the same step on the same fixed batch (bucketing kept with the batch) as one captured hipGraph, per replay"))
    return model


if STEP_LOOP_ONLY:
    bench_c3_steps()
else:
    c3 = bench_c3_steps()
    bench_update("C3 GGNN / QM9, D=128, 6 layers", c3)
    bench_update("C2 RGCN / PPI, D=256, 3 layers", c2_model())
