#!/usr/bin/env python
"""config sparse_update: the citation task's sampled batches over sparse features with and without `"sparse_update": true`
(csrc/sparse_update.hip: the row-deferred Adam update of the input projection's weight) on one MI355X, same build, same process,
the same batches through both models.
  --shape zipf      graph and features as scripts/bench_sparse_sampling.py: V = 2^20 nodes, F = 2^17 words, 32 Zipf-like word draws
                    per node (24.5 M entries), row-normalised
  --shape identity  the same graph with F = V = 2^20 and the identity matrix as features: learnable node-id embeddings
  model     RGCN, 2 layers, hidden 256, Adam; fanouts [10, 10], 1024 seeds per batch
  batches   BATCHES sampled batches, drawn once, each with its own SparseRows.take_rows container; an "epoch" below is one pass over them
Both models are built from one seed and take the same batches in the same order throughout, so that the flushed "on" model must equal
the "off" model bit for bit at the end (`bit_equal_after_flush`).
Reported, median [min, max] over ROUNDS rounds that alternate which model goes first:
  step_ms_on, step_ms_off           one whole training step (wall clock by events over an epoch / BATCHES)
  catch_up_us, rows_step_us         the two row kernels of a step of the "on" model, by events around the launch
  dense_adam_us_on, dense_adam_us_off, l2norm_us_on, l2norm_us_off
                                    relgnn_mt_adam_clip (on: the other variables; off: all of them) and relgnn_mt_l2norm, the same way
  flush_us                          flush_deferred() after an epoch; flush_pending_fraction: the rows it had to replay
  touched_fraction                  rows a batch names / F;  stale_fraction_of_touched: those among them behind at rows_touched()
  peak_MiB_on, peak_MiB_off         peak device memory during one step above what is held before it
One JSON line per shape, also appended to profiles/sparse_update.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from tf_gnn_samples_amd import _lib
from tf_gnn_samples_amd.models import RGCN_Model
from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, random_rows

dev = torch.device("cuda:0")
ROUNDS, BATCHES = 7, 16
FANOUTS, SEEDS, HIDDEN, DRAWS = [10, 10], 1024, 256, 32
KERNEL = "graph_model/dense/kernel"
OUT = ROOT / "profiles" / "sparse_update.jsonl"
TRACED = {"relgnn_rows_adam_catch_up": "catch_up_us", "relgnn_rows_adam_step": "rows_step_us", "relgnn_mt_adam_clip": "dense_adam_us",
          "relgnn_mt_l2norm": "l2norm_us"}


def med(values, digits=1):
    s = sorted(values)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


class LaunchTrace:
    """Timed events around the launches named in TRACED while active (the optimizer launches through _lib.launch)."""

    def __init__(self):
        self.events, self._launch = [], _lib.launch

    def __enter__(self):
        def launch(name, *args):
            if name not in TRACED:
                return self._launch(name, *args)
            before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before.record()
            self._launch(name, *args)
            after.record()
            self.events.append((TRACED[name], before, after))
        _lib.launch = launch
        return self

    def __exit__(self, *exc):
        _lib.launch = self._launch

    def microseconds(self):
        torch.cuda.synchronize()
        spent = {}
        for key, before, after in self.events:
            spent.setdefault(key, []).append(before.elapsed_time(after) * 1e3)
        return spent


def epoch_ms(model, batches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for b in batches:
        model.train_step(b)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / len(batches)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, 1)


def main():
    global OUT
    if "--out" in sys.argv:
        OUT = Path(sys.argv[sys.argv.index("--out") + 1])
    shape = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else "zipf"
    V = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 2 ** 20
    F = V if shape == "identity" else (int(sys.argv[sys.argv.index("--features") + 1]) if "--features" in sys.argv else 2 ** 17)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    off_key = {"fanouts": FANOUTS, "seeds_per_batch": SEEDS, "seed": 0, "sparse_features": True}
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True, sampled_batches=dict(off_key)))
    task.load_synthetic(num_nodes=V, num_features=F, num_classes=7, num_train=V // 2, num_valid=V // 8, num_test=V // 8,
                        neighbours_per_node=8.0, feature_density=0.0, seed=0, hub_nodes=64)
    if shape == "identity":
        host = SparseRows(np.arange(V + 1), np.arange(V), np.ones(V, np.float32), (V, V))
    else:
        rng = np.random.default_rng(0)
        rowptr, col = random_rows(rng, V, F, np.full(V, DRAWS), draw=lambda size: (rng.zipf(1.2, size=size) - 1) % F)
        words = np.diff(rowptr)
        host = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / words.astype(np.float32), words), (V, F))
    for which in (DataFold.TRAIN, DataFold.VALIDATION):                  # the folds share the one container
        task._loaded_data[which] = [f._replace(node_features=host) for f in task._loaded_data[which]]
    fold = task._loaded_data[DataFold.TRAIN][0]
    print("graph and features built in %.1f s (%d entries)" % (time.time() - t0, host.nnz), flush=True)
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=1)
    models = {"off": RGCN_Model(dict(p), task, device=str(dev))}
    task.params["sampled_batches"] = dict(off_key, sparse_update=True)      # (read when a model is built: the optimizer registers the weight)
    models["on"] = RGCN_Model(dict(p), task, device=str(dev))
    opt = models["on"].optimizer
    assert opt._deferred is not None and models["off"].optimizer._deferred is None
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    rng = np.random.RandomState(0)
    batches = []
    for draw in range(BATCHES):
        seeds = np.sort(rng.choice(V, size=SEEDS, replace=False)).astype(np.int32)
        batches.append(state.sampler.sample(seeds, draw + 1).device_batch(state.features, state.labels, state.mask, 1.0))
    named = [(b.extra["sparse_node_features"].transposed.rowptr[1:] > b.extra["sparse_node_features"].transposed.rowptr[:-1]) for b in batches]
    touched = [float(n.float().mean()) for n in named]
    for which in ("on", "off"):
        epoch_ms(models[which], batches)
    torch.cuda.synchronize()
    print("warm after %.1f s; a batch names %.4f of the %d rows" % (time.time() - t0, float(np.mean(touched)), F), flush=True)

    step_ms, spent, flush_us, flush_pending, stale = {"on": [], "off": []}, {}, [], [], []
    for r in range(ROUNDS):
        order = ("on", "off") if r % 2 == 0 else ("off", "on")
        for which in order:
            step_ms[which].append(epoch_ms(models[which], batches))
        for which in order:                                 # the same epoch again, the optimizer's launches timed one by one
            with LaunchTrace() as trace:
                for b, n in zip(batches, named):
                    if which == "on" and r == 0:
                        behind = opt._deferred.stamps[n] < opt.t
                        stale.append(float(behind.float().mean()))
                    models[which].train_step(b)
            for key, values in trace.microseconds().items():
                spent.setdefault(key + ("" if key in ("catch_up_us", "rows_step_us") else "_" + which), []).append(float(np.mean(values)))
        flush_pending.append(opt.pending_rows() / F)
        before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before.record()
        opt.flush_deferred()
        after.record()
        after.synchronize()
        flush_us.append(before.elapsed_time(after) * 1e3)
    equal = all(torch.equal(models["on"].variables[n], models["off"].variables[n]) for n in models["on"].variables.names()) \
        and all(torch.equal(a, b) for a, b in zip(opt.m + opt.v, models["off"].optimizer.m + models["off"].optimizer.v))
    peaks = {which: peak_mib(lambda: models[which].train_step(batches[0])) for which in ("on", "off")}
    row = {"what": "sparse_update", "shape": shape, "nodes_in_graph": V, "features": F, "entries": host.nnz, "hidden": HIDDEN,
           "model": "RGCN, hidden %d, 2 layers, Adam" % HIDDEN, "fanouts": FANOUTS, "seeds": SEEDS, "rounds": ROUNDS, "batches": BATCHES,
           "batch_nodes": round(float(np.mean([b.num_nodes for b in batches])), 1), "touched_fraction": med(touched, 4),
           "stale_fraction_of_touched": med(stale, 4), "step_ms_on": med(step_ms["on"], 3), "step_ms_off": med(step_ms["off"], 3),
           "flush_us": med(flush_us), "flush_pending_fraction": med(flush_pending, 4), "peak_MiB_on": peaks["on"],
           "peak_MiB_off": peaks["off"], "bit_equal_after_flush": bool(equal)}
    for key, values in sorted(spent.items()):
        row[key] = med(values)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    assert equal, "the flushed model differs from the dense one"


if __name__ == "__main__":
    main()
