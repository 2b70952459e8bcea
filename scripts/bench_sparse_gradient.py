#!/usr/bin/env python
"""config sparse_gradient: the citation task's sampled batches over sparse features with `"sparse_update": true`, without and with
`"sparse_gradient": true` (csrc/sparse_gradient.hip: the projection's weight gradient as the rows a batch names, the dense norm's
bits over them, the row step on compact rows) on one MI355X, same build, same process, the same batches through both models.
  --shape zipf      graph and features as scripts/bench_sparse_update.py: V = 2^20 nodes, F = 2^17 words, 32 Zipf-like word draws
                    per node (24.5 M entries), row-normalised
  --shape identity  the same graph with F = V = 2^20 and the identity matrix as features: learnable node-id embeddings
  model     RGCN, 2 layers, hidden 256, Adam; fanouts [10, 10], 1024 seeds per batch
  batches   BATCHES sampled batches, drawn once, each with its own SparseRows.take_rows(named_rows=True) container (the "off" model
            does not look at the named rows); an "epoch" below is one pass over them
"off" is the `"sparse_update"`-only model: the path of the commit before this key existed.  Both models are built from one seed and
take the same batches in the same order throughout, so that flushed they must be equal bit for bit (`bit_equal_after_flush`).
Reported, median [min, max] over ROUNDS rounds that alternate which model goes first:
  step_ms_on, step_ms_off           one whole training step (device events over an epoch / BATCHES)
  l2norm_us_off / l2norm_us_on      relgnn_mt_l2norm (off: every variable, the dense [F, hidden] gradient among them; on: the others)
  rows_l2norm_us                    relgnn_rows_l2norm, the projection weight's norm from its compact rows (on)
  grad_launch_us_on / _off          the projection's weight-gradient launch (relgnn_csr_project_f32 in the backward): over the named
                                    rows, over all F rows
  rows_step_us_on / _off            relgnn_rows_adam_step_compact, relgnn_rows_adam_step
  take_rows_ms_named / _plain       SparseRows.take_rows of a batch's nodes with and without named_rows=True (read-back included)
  touched_fraction                  rows a batch names / F
  peak_MiB_on, peak_MiB_off         peak device memory during one step above what is held before it
One JSON line per shape, also appended to profiles/sparse_gradient.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
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
OUT = ROOT / "profiles" / "sparse_gradient.jsonl"
TRACED = {"relgnn_mt_l2norm": "l2norm_us", "relgnn_rows_l2norm": "rows_l2norm_us", "relgnn_rows_adam_step": "rows_step_us",
          "relgnn_rows_adam_step_compact": "rows_step_us", "relgnn_csr_project_f32": "csr_project"}


def med(values, digits=1):
    s = sorted(values)
    return [round(s[len(s) // 2], digits), round(s[0], digits), round(s[-1], digits)]


class LaunchTrace:
    """Timed events around the launches named in TRACED while active (every launch goes through _lib.launch).  The projection
    launches twice per step, forward and weight gradient: step() starts a new step, the second launch of a step is the gradient."""

    def __init__(self):
        self.events, self._launch, self._projections = [], _lib.launch, 0

    def step(self):
        self._projections = 0

    def __enter__(self):
        def launch(name, *args):
            key = TRACED.get(name)
            if key == "csr_project":
                self._projections += 1
                key = "grad_launch_us" if self._projections == 2 else None
            if key is None:
                return self._launch(name, *args)
            before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before.record()
            self._launch(name, *args)
            after.record()
            self.events.append((key, before, after))
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


def take_rows_ms(features, node_lists, named_rows):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for nodes in node_lists:
        features.take_rows(nodes, validated=True, named_rows=named_rows)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / len(node_lists)


def peak_mib(model, batch):
    model.optimizer.zero_grad()                             # (the last step's gradients are not what this one is held against)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    model.train_step(batch)
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
    off_key = {"fanouts": FANOUTS, "seeds_per_batch": SEEDS, "seed": 0, "sparse_features": True, "sparse_update": True}
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
    task.params["sampled_batches"] = dict(off_key, sparse_gradient=True)      # (read when a model is built: the optimizer gets its sink)
    models["on"] = RGCN_Model(dict(p), task, device=str(dev))
    opts = {which: models[which].optimizer for which in models}
    assert opts["on"].row_gradient_sink is not None and opts["off"].row_gradient_sink is None and opts["off"]._deferred is not None
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    rng = np.random.RandomState(0)
    batches = []
    for draw in range(BATCHES):
        seeds = np.sort(rng.choice(V, size=SEEDS, replace=False)).astype(np.int32)
        batches.append(state.sampler.sample(seeds, draw + 1).device_batch(state.features, state.labels, state.mask, 1.0, named_rows=True))
    touched = [b.extra["sparse_node_features"].named_rows().count / F for b in batches]
    node_lists = [b.extra["sampled_nodes"] for b in batches]
    for which in ("on", "off"):
        epoch_ms(models[which], batches)
    for named_rows in (True, False):
        take_rows_ms(state.features, node_lists, named_rows)
    torch.cuda.synchronize()
    print("warm after %.1f s; a batch names %.4f of the %d rows" % (time.time() - t0, float(np.mean(touched)), F), flush=True)

    step_ms, spent, taken = {"on": [], "off": []}, {}, {True: [], False: []}
    for r in range(ROUNDS):
        order = ("on", "off") if r % 2 == 0 else ("off", "on")
        for which in order:
            step_ms[which].append(epoch_ms(models[which], batches))
        for which in order:                                 # the same epoch again, the launches of interest timed one by one
            with LaunchTrace() as trace:
                for b in batches:
                    trace.step()
                    models[which].train_step(b)
            for key, values in trace.microseconds().items():
                spent.setdefault(key if key == "rows_l2norm_us" else key + "_" + which, []).append(float(np.mean(values)))
        for named_rows in ((True, False) if r % 2 == 0 else (False, True)):
            taken[named_rows].append(take_rows_ms(state.features, node_lists, named_rows))
    for opt in opts.values():
        opt.flush_deferred()
    equal = all(torch.equal(models["on"].variables[n], models["off"].variables[n]) for n in models["on"].variables.names()) \
        and all(torch.equal(a, b) for a, b in zip(opts["on"].m + opts["on"].v, opts["off"].m + opts["off"].v))
    peaks = {which: peak_mib(models[which], batches[0]) for which in ("on", "off")}
    row = {"what": "sparse_gradient", "shape": shape, "nodes_in_graph": V, "features": F, "entries": host.nnz, "hidden": HIDDEN,
           "model": "RGCN, hidden %d, 2 layers, Adam" % HIDDEN, "fanouts": FANOUTS, "seeds": SEEDS, "rounds": ROUNDS, "batches": BATCHES,
           "batch_nodes": round(float(np.mean([b.num_nodes for b in batches])), 1), "touched_fraction": med(touched, 4),
           "step_ms_on": med(step_ms["on"], 3), "step_ms_off": med(step_ms["off"], 3),
           "take_rows_ms_named": med(taken[True], 3), "take_rows_ms_plain": med(taken[False], 3),
           "peak_MiB_on": peaks["on"], "peak_MiB_off": peaks["off"], "bit_equal_after_flush": bool(equal)}
    for key, values in sorted(spent.items()):
        row[key] = med(values)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    assert equal, "the flushed models differ"


if __name__ == "__main__":
    main()
