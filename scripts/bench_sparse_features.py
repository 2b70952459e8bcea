#!/usr/bin/env python
"""config sparse_features: the citation task's sparse_node_features mode (csrc/csr_project.hip) against the dense input projection,
on one MI355X, same build, same process.
  projection_forward            act(X W): ops.csr_rows_project on the SparseRows against dense_act on the dense table
  projection_forward_backward   the same + the weight gradient (one launch over the transposed structure / the Dense route's TN product)
  train_step                    one RGCN training step (hidden 256, forward, backward, clip, Adam) in either mode
at  cora    2708 x 1433, 1.27 % dense        pubmed  19717 x 500, 10 % dense        (synthetic, row-normalised bags of words)
and, sparse only (the dense table would be 512 GiB),
    large   V = 2^20, F = 2^17, 32 word draws per node from a Zipf-like distribution (so that long transposed rows occur),
for which the achieved bytes/s against the bytes the algorithm needs are reported:
    forward   nnz (4 n + 8) + V 4 n + 4 (V + 1)             gradient   nnz (8 n + 8) + F 4 n + 4 (F + 1)
Device events around CALLS calls; every shape warmed up; the routes alternate ROUNDS times; times in microseconds per call,
median [min, max] over the rounds.  One JSON line per case, also appended to profiles/sparse_features.jsonl (or --out FILE)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd import ops
from tf_gnn_samples_amd.dense import dense_act
from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold, DeviceBatch
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, CALLS, HIDDEN = 7, 200, 256
ACT = ops.activation_id("tanh")
OUT = ROOT / "profiles" / "sparse_features.jsonl"


def timed_us(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def alternate(fns, calls, warm=5):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            ts[name].append(timed_us(fn, calls))
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


def projection_cases(rows, dense, base, calls):
    """forward and forward + backward of the projection alone; dense None: sparse only."""
    W = (torch.rand((rows.shape[1], HIDDEN), device=dev) * 0.2 - 0.1).requires_grad_(True)
    gout = torch.rand((rows.shape[0], HIDDEN), device=dev) - 0.5

    def forward(x):
        if isinstance(x, SparseRows):
            return lambda: ops.csr_rows_project(x, W, ACT)
        return lambda: dense_act(x, W, None, ACT)

    def forward_backward(x):
        fwd = forward(x)

        def fn():
            torch.autograd.grad(fwd(), [W], gout)
            ops.join_deferred()
        return fn
    operands = {"sparse": rows} if dense is None else {"dense": dense, "sparse": rows}
    f = alternate({k: forward(x) for k, x in operands.items()}, calls)
    assert ops.ROUTES["csr_project"] == "hip"
    fb = alternate({k: forward_backward(x) for k, x in operands.items()}, calls)
    emit(dict(base, what="projection_forward", **f))
    emit(dict(base, what="projection_forward_backward", **fb))
    return f, fb


def train_step_case(name, V, F, density, base):
    steps = {}
    for mode in ("dense", "sparse"):
        task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=mode == "sparse"))
        task.load_synthetic(num_nodes=V, num_features=F, feature_density=density, seed=1)
        p = RGCN_Model.default_params()
        p.update(hidden_size=HIDDEN, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
        model = RGCN_Model(p, task, device=str(dev))
        (mb,) = task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, 10 ** 9)
        batch = DeviceBatch(mb, dev)
        steps[mode] = (lambda m, b: lambda: m.train_step(b))(model, batch)
    emit(dict(base, what="train_step", model="RGCN, hidden %d, %d layers, Adam" % (HIDDEN, p['graph_num_layers']), **alternate(steps, CALLS)))


def synthetic(rng, V, F, density):
    rowptr, col = random_rows(rng, V, F, rng.binomial(F, density, size=V))
    words = np.diff(rowptr)
    return SparseRows(rowptr, col, np.repeat(np.float32(1.0) / np.maximum(words, 1).astype(np.float32), words), (V, F))


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(0)
    for name, V, F, density in (("cora", 2708, 1433, 0.0127), ("pubmed", 19717, 500, 0.10)):
        host = synthetic(rng, V, F, density)
        rows = host.to(dev)
        base = {"shape": name, "nodes": V, "features": F, "nnz": host.nnz, "density": round(host.nnz / (V * F), 4), "hidden": HIDDEN,
                "activation": "tanh", "rounds": ROUNDS, "calls": CALLS}
        projection_cases(rows, rows.to_dense(), base, CALLS)
        train_step_case(name, V, F, density, base)
    if "--skip-large" in sys.argv:
        return
    V, F, draws = 2 ** 20, 2 ** 17, 32
    rowptr, col = random_rows(rng, V, F, np.full(V, draws), draw=lambda size: (rng.zipf(1.2, size=size) - 1) % F)
    words = np.diff(rowptr)
    host = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / words.astype(np.float32), words), (V, F))
    longest = int(np.diff(host.transposed.rowptr.numpy()).max())
    rows = host.to(dev)
    base = {"shape": "large", "nodes": V, "features": F, "nnz": host.nnz, "draws_per_node": draws, "longest_transposed_row": longest,
            "slabs": int(host.transposed.slabs.shape[0]), "hidden": HIDDEN, "activation": "tanh", "rounds": ROUNDS, "calls": CALLS}
    f, fb = projection_cases(rows, None, base, CALLS)
    n, nnz = HIDDEN, host.nnz
    fwd_bytes = nnz * (4 * n + 8) + V * 4 * n + 4 * (V + 1)
    bwd_bytes = nnz * (8 * n + 8) + F * 4 * n + 4 * (F + 1)
    fwd_us = f["sparse_us"][0]
    bwd_us = fb["sparse_us"][0] - fwd_us
    emit(dict(base, what="projection_bandwidth", forward_algorithmic_bytes=fwd_bytes, gradient_algorithmic_bytes=bwd_bytes,
              forward_TBps=round(fwd_bytes / fwd_us * 1e-6, 3), gradient_TBps=round(bwd_bytes / bwd_us * 1e-6, 3),
              note="gradient time = forward_backward - forward (medians)"))


if __name__ == "__main__":
    main()
