#!/usr/bin/env python
"""The preparation of the data-parallel gradient reduction, the collective itself left out, on one MI355X, same build, same process:
  packed    PackedGradientAllReducer.pack(scale): relgnn_mt_pack_scaled_f32, one launch per 48 variables, nothing behind the collective
  sequence  what GradientAllReducer.__call__ does around its all-reduce: the list of gradients, torch._foreach_copy_ into the views,
            mul_ by the weight, the scalar write flat[-1] = w, and the div_ by flat[-1] behind the collective
on the variable sets of the C2 model (RGCN / PPI, D = 256, 3 layers) and of the C5 model (GNN-FiLM, 23 edge types, D = 128, 10
layers), with fixed random gradients.  Per form: device microseconds per call between two events (synchronised outside the window),
host microseconds per call spent enqueuing (a host clock around the calls, no synchronise inside), and the launches of one call
(kernels and copies counted by torch's profiler).  Warm-up first, then the two forms take turns, SAMPLES rounds; median [min, max].
One JSON line per variable set, also appended to profiles/dp_train.jsonl.  No scaling figure comes out of this: one GPU."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

if not torch.cuda.is_available():
    raise SystemExit("bench_dp_pack.py needs an MI355X: the pack is a HIP kernel with no CPU form to measure")

from tf_gnn_samples_amd.models import name_to_model_class
from tf_gnn_samples_amd.parallel import GradientAllReducer, PackedGradientAllReducer
from tf_gnn_samples_amd.tasks import PPI_Task

dev = torch.device("cuda:0")
CALLS, SAMPLES = 200, 9
OUT = ROOT / "profiles" / "dp_train.jsonl"


def quiet(fn):
    so, sys.stdout = sys.stdout, sys.stderr
    try:
        return fn()
    finally:
        sys.stdout = so


def spread(v, digits):
    s = sorted(v)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


def c2_model():
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(1, 1, seed=0)                  # (the variable set does not depend on the graphs)
    cls, extra = name_to_model_class("RGCN")
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=256, graph_num_layers=3, graph_num_timesteps_per_layer=1, message_aggregation_function="sum",
             graph_activation_function="ReLU")
    return quiet(lambda: cls(p, task, device=str(dev)))


def c5_model():
    task = PPI_Task(PPI_Task.default_params())          # (scripts/bench_configs.py's C5: the PPI head over VarMisuse-shaped graphs)
    task._PPI_Task__num_edge_types, task._PPI_Task__initial_node_feature_size, task._PPI_Task__num_labels = 23, 128, 1
    cls, extra = name_to_model_class("GNN-FiLM")
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=128, graph_num_layers=10, graph_dense_between_every_num_gnn_layers=1, graph_residual_connection_every_num_layers=2)
    return quiet(lambda: cls(p, task, device=str(dev)))


def timed(fn, calls):
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


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def bench(tag, model):
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.optimizer.params]
    grads = [torch.randn(p.shape, device=dev, generator=gen) for p in params]
    packed, old = PackedGradientAllReducer(params), GradientAllReducer(params)
    weight = 2245.0

    def set_grads():
        for p, g in zip(params, grads):
            p.grad = g

    def form_packed():
        packed.pack(0.4375)

    @torch.no_grad()
    def form_sequence():                                 # GradientAllReducer.__call__ without its dist.all_reduce
        gs = [p.grad if p.grad is not None else torch.zeros_like(p) for p in old.params]
        torch._foreach_copy_(old.views, gs)
        old.flat[:-1].mul_(weight)
        old.flat[-1] = weight
        old.flat[:-1].div_(old.flat[-1])

    forms = {"packed": form_packed, "sequence": form_sequence}
    set_grads()
    for fn in forms.values():
        for _ in range(20):
            fn()
    ts = {k: ([], []) for k in forms}
    for _ in range(SAMPLES):
        for k, fn in forms.items():
            d, h = timed(fn, CALLS)
            ts[k][0].append(d)
            ts[k][1].append(h)
    row = {"case": "dp_pack", "variables_of": tag, "variables": len(params), "elements": sum(p.numel() for p in params),
           "calls_per_sample": CALLS, "samples": SAMPLES}
    for k, fn in forms.items():
        row[k + "_us"] = spread(ts[k][0], 1)
        row[k + "_host_us"] = spread(ts[k][1], 1)
        row[k + "_launches"] = launches(fn)
    row["what"] = ("microseconds per call, median [min, max] over the samples, the two forms taking turns; *_us between device events, "
                   "*_host_us the host's enqueue time, *_launches device kernels and copies of one call; the collective is in neither")
    line = json.dumps(row)
    print(line, flush=True)
    OUT.parent.mkdir(exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


bench("C2 RGCN / PPI, D=256, 3 layers", c2_model())
bench("C5 GNN-FiLM, 23 edge types, D=128, 10 layers", c5_model())
