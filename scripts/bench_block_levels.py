#!/usr/bin/env python
"""config block_levels: the citation task's layered sampled batches with and without `"blocks": true` (level bucketings derived from the
union graph's, csrc/level_plan.hip; target rows only in ops/rgcn.py) on one MI355X, same build, same process, the same HopSubgraphs
through both forms of the batch.  The protocol of scripts/bench_layered_sampling.py, whose graph, timers and epoch it uses: the
comparison is always `"layered"` without the key in this run, never a figure of another day.
  graph     V = 2^20 nodes, 17.8 M edges with hubs, 128 dense features, 7 classes
  --cases   rgcn2   RGCN, hidden 256, 2 layers, fanouts [10, 10], 1024 seeds per batch
            rgcn3   RGCN, 3 layers, fanouts [10, 10, 10]
            ggnn2   GGNN, 2 layers, fanouts [10, 10]: no rectangular route, the derivation alone
            valid   a validation epoch of RGCN 2 x 256 over a fold of 1024 nodes with exact fields (all fanouts 0, one batch), with
                    and without "keep"
            products  (needs no graph) the forward product of RGCN's layer 2 at the rgcn2 shape alone: [1024, 512] x [512, 256], which
                    the key leaves below the limb kernels' row minimum and on the library, against the [11040, 512] x [512, 256] limb
                    product the layered form runs in its place; 200 calls between device events
  batches   BATCHES HopSubgraphs, drawn once; "blocks" is device_batch(layered=True, derived=True) of each, "layered"
            device_batch(layered=True) of the same one.  Two models from one seed; every model sees one form only.
Reported per case, median [min, max] over ROUNDS rounds that alternate which form goes first:
  graphs_us_union / _levels / _derived  the bucketing of the one union graph / of the H level graphs by H constructor calls / of the
                                        H level graphs by one constructor call and the derivation; device events (*_wall_us: the host)
  forward_ms_*, backward_ms_*, step_ms_*  over an epoch of the BATCHES batches made beforehand: the layered form buckets its levels
                                        inside the forward, the blocks form brought them along (their cost is graphs_us_derived)
  fresh_step_ms_*                       device_batch(...) of the HopSubgraph and the training step on it, together: everything
                                        between the sampler and the update, in both forms
  peak_MiB_*                            peak device memory during one step above what is held before it
  routes_*                              rows x route of every forward / input-gradient product of one step (dense._route, and the limb
                                        group product of the aggregate-first layer): which products fell below the limb kernels' row
                                        minimum and took the library
  valid: epoch_ms_{layered,blocks}[_keep]  wall clock of model._run_epoch over the fold, host synchronised
One JSON line per case, also appended to profiles/block_levels.jsonl (or --out FILE).  --nodes N shrinks the graph (a dry run)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np
import torch

import bench_layered_sampling as BL
from tf_gnn_samples_amd import dense as DN, models as model_classes, ops
from tf_gnn_samples_amd.graph import RelGraph, clear_graph_cache
from tf_gnn_samples_amd.tasks import DataFold
from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler, derived_level_graphs

dev = BL.dev
ROUNDS, BATCHES, HIDDEN = BL.ROUNDS, BL.BATCHES, BL.HIDDEN
CASES = {"rgcn2": ("RGCN_Model", [10, 10]), "rgcn3": ("RGCN_Model", [10, 10, 10]), "ggnn2": ("GGNN_Model", [10, 10])}
SEEDS = 1024
OUT = ROOT / "profiles" / "block_levels.jsonl"
FORMS = ("blocks", "layered")
med, Timer = BL.med, BL.Timer


def make_model(name, task, num_layers):
    cls = getattr(model_classes, name)
    p = cls.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=num_layers, graph_num_timesteps_per_layer=1, graph_layer_input_dropout_keep_prob=1.0,
             random_seed=1)
    return cls(dict(p), task, device=str(dev))


def routes_of_a_step(model, batch):
    """rows x route of every product of one training step that asks dense._route, and of the limb group products."""
    seen, route, group = [], DN._route, DN._limb_group_ok

    def recording_route(layout, a, b, *rest):
        out = route(layout, a, b, *rest)
        seen.append("%dx%d:%s" % (a.shape[0], a.shape[1], out[0]))
        return out

    def recording_group(a, kernels, layout):
        ok = group(a, kernels, layout)
        if ok:
            seen.append("%dx%d:limb-group" % (a.shape[0], a.shape[1]))
        return ok
    DN._route, DN._limb_group_ok = recording_route, recording_group
    try:
        model.train_step(batch)
        torch.cuda.synchronize()
    finally:
        DN._route, DN._limb_group_ok = route, group
    return seen


def fresh_epoch(model, subs, state, derived):
    """ms per HopSubgraph for device_batch(...) and the training step on it."""
    clear_graph_cache()
    with Timer() as t:
        for s in subs:
            model.train_step(s.device_batch(state.features, state.labels, state.mask, 1.0, layered=True, derived=derived))
    return t.ms / len(subs)


def run_case(case, task, V):
    model_name, fanouts = CASES[case]
    H = len(fanouts)
    task.params["sampled_batches"] = {"fanouts": fanouts, "seeds_per_batch": SEEDS, "seed": 0, "layered": True, "blocks": True}
    fold = task._loaded_data[DataFold.TRAIN][0]
    task.bind_sampling_device(dev)
    state = task.batches.neighbour_state(fold, dev)
    sampler = NeighbourSampler(state.sampler.graph, fanouts, seed=0)
    models = {form: make_model(model_name, task, H) for form in FORMS}
    rng = np.random.RandomState(0)
    lists = [np.sort(rng.choice(V, size=SEEDS, replace=False)).astype(np.int32) for _ in range(BATCHES)]
    subs = [sampler.sample_by_hop(s, d + 1) for d, s in enumerate(lists)]
    batches = {form: [s.device_batch(state.features, state.labels, state.mask, 1.0, layered=True, derived=form == "blocks") for s in subs]
               for form in FORMS}
    assert all(level.graph is not None for b in batches["blocks"] for level in b.extra["layer_graphs"])
    assert all(level.graph is None for b in batches["layered"] for level in b.extra["layer_graphs"])
    for form in FORMS:                                                   # warm: plans, scratch, the library's handles
        BL.epoch(models[form], batches[form])
        fresh_epoch(models[form], subs, state, form == "blocks")
    torch.cuda.synchronize()
    rows = [round(float(np.mean([s.hop_nodes[d] for s in subs])), 1) for d in range(H + 1)]
    print("%s: warm; rows %s" % (case, rows), flush=True)

    out = {}
    push = lambda key, value: out.setdefault(key, []).append(value)
    for r in range(ROUNDS):
        order = FORMS if r % 2 == 0 else FORMS[::-1]
        for form in order:
            forward, backward, step = BL.epoch(models[form], batches[form])
            push("forward_ms_" + form, forward), push("backward_ms_" + form, backward), push("step_ms_" + form, step)
        for form in order:
            push("fresh_step_ms_" + form, fresh_epoch(models[form], subs, state, form == "blocks"))
        kinds = ("union", "levels", "derived")
        for which in (kinds if r % 2 == 0 else kinds[::-1]):
            device_us, wall_us = [], []
            for s in subs:
                levels = s.level_graphs()
                with Timer() as t:
                    if which == "union":
                        RelGraph(s.adjacency_lists, s.num_nodes, validate=False)
                    elif which == "levels":
                        for level in levels:
                            RelGraph(level.adjacency_lists, level.num_sources, validate=False)
                    else:
                        derived_level_graphs(s)
                device_us.append(t.ms * 1e3), wall_us.append(t.host_us)
            push("graphs_us_" + which, float(np.mean(device_us))), push("graphs_wall_us_" + which, float(np.mean(wall_us)))
    assert not sampler.stamp.any()
    row = {"what": "block_levels", "case": case, "nodes_in_graph": V, "edges_in_graph": int(sampler.graph.M),
           "model": "%s, hidden %d, %d layers, Adam" % (model_name, HIDDEN, H), "fanouts": fanouts, "seeds": SEEDS, "rounds": ROUNDS,
           "batches": BATCHES, "rows": rows, "edges": round(float(np.mean([s.num_edges for s in subs])), 1)}
    for key, values in sorted(out.items()):
        row[key] = med(values, 1 if "_us_" in key else 3)
    for form in FORMS:
        row["peak_MiB_" + form] = BL.peak_mib(models[form], batches[form][0])
        ops.ROUTES["rgcn_rows"] = None
        row["routes_" + form] = routes_of_a_step(models[form], batches[form][0])
        row["rgcn_rows_" + form] = ops.ROUTES["rgcn_rows"]
    emit(row)
    del models, batches, subs
    clear_graph_cache()
    torch.cuda.empty_cache()


def run_validation(task, V):
    """One validation epoch over a fold of 1024 nodes, exact fields, one batch: {layered, blocks} x {built every epoch, kept}."""
    valid = task._loaded_data[DataFold.VALIDATION][0]
    ids = np.flatnonzero(valid.mask)[:SEEDS]
    mask = np.zeros(len(valid.mask), dtype=valid.mask.dtype)
    mask[ids] = 1
    data = [valid._replace(mask=mask, labels=np.where(mask != 0, valid.labels, 0).astype(valid.labels.dtype))]
    forms = [(blocks, keep) for blocks in (True, False) for keep in (False, True)]

    def params(blocks, keep):
        value = {"fanouts": [10, 10], "seeds_per_batch": SEEDS, "seed": 0,
                 "evaluation": dict({"fanouts": [0, 0], "seeds_per_batch": SEEDS}, **({"keep": True} if keep else {}))}
        return dict(value, blocks=True) if blocks else value
    task.params["sampled_batches"] = params(False, False)
    task.bind_sampling_device(dev)
    model = make_model("RGCN_Model", task, 2)

    def epoch_ms(blocks, keep):
        task.params["sampled_batches"] = params(blocks, keep)
        torch.cuda.synchronize()
        t = time.perf_counter()
        loss = model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)[0]
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, loss
    losses = {form: epoch_ms(*form)[1] for form in forms}                # warm (and the kept batches are built)
    for form in forms:
        epoch_ms(*form)
    assert len(set(losses.values())) == 1, losses
    out = {}
    for r in range(ROUNDS):
        for form in (forms if r % 2 == 0 else forms[::-1]):
            out.setdefault(form, []).append(epoch_ms(*form)[0])
    task.params["sampled_batches"] = params(True, False)
    batch = next(iter(model._batches(data, DataFold.VALIDATION)))
    row = {"what": "block_levels", "case": "valid", "nodes_in_graph": V, "model": "RGCN_Model, hidden %d, 2 layers" % HIDDEN,
           "fanouts": [0, 0], "seeds": SEEDS, "rounds": ROUNDS, "loss": losses[forms[0]],
           "rows": [int(level.num_targets) for level in batch.extra["layer_graphs"]][::-1] + [int(batch.num_nodes)],
           "edges": int(batch.num_edges)}
    for (blocks, keep), values in out.items():
        row["epoch_ms_%s%s" % ("blocks" if blocks else "layered", "_keep" if keep else "")] = med(values, 3)
    emit(row)


def run_products():
    """dense.grouped_nn_gemm on two [256, 256] kernels over 1024 and 11040 bucket-sum rows, us per call."""
    rng = torch.Generator(device=dev).manual_seed(0)
    kernels = [torch.nn.Parameter(torch.randn((HIDDEN, HIDDEN), generator=rng, device=dev) * 0.05) for _ in range(2)]
    shapes = {"target_rows": 1024, "all_rows": 11040}
    inputs = {name: torch.randn((rows, 2 * HIDDEN), generator=rng, device=dev) for name, rows in shapes.items()}
    routes = {}
    for name, a in inputs.items():
        seen, route, group = [], DN._route, DN._limb_group_ok
        DN._route = lambda layout, a, b, *rest: (lambda out: (seen.append(out[0]), out)[1])(route(layout, a, b, *rest))
        DN._limb_group_ok = lambda a, ws, kind: (lambda ok: (seen.append("limb-group") if ok else None, ok)[1])(group(a, ws, kind))
        try:
            with torch.no_grad():
                for _ in range(20):
                    DN.grouped_nn_gemm(a, kernels)
        finally:
            DN._route, DN._limb_group_ok = route, group
        routes[name] = sorted(set(seen))
    out = {}
    for r in range(ROUNDS):
        for name in (list(shapes) if r % 2 == 0 else list(shapes)[::-1]):
            with torch.no_grad(), Timer() as t:
                for _ in range(200):
                    DN.grouped_nn_gemm(inputs[name], kernels)
            out.setdefault(name, []).append(t.ms * 1e3 / 200)
    row = {"what": "block_levels", "case": "products", "product": "[rows, 512] x [512, 256], two edge types", "rows": shapes,
           "routes": routes, "rounds": ROUNDS, "calls": 200}
    for name, values in out.items():
        row["product_us_" + name] = med(values, 2)
    emit(row)


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
    cases = sys.argv[sys.argv.index("--cases") + 1].split(",") if "--cases" in sys.argv else ["rgcn2", "rgcn3", "ggnn2", "valid"]
    if any(c not in CASES and c not in ("valid", "products") for c in cases):
        raise SystemExit("--cases takes a comma-separated list of %s" % (sorted(CASES) + ["valid", "products"]))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    if "products" in cases:
        run_products()
        cases = [c for c in cases if c != "products"]
        if not cases:
            return
    t0 = time.time()
    task = BL.build_task("base", V)
    print("graph built in %.1f s" % (time.time() - t0), flush=True)
    for case in cases:
        if case == "valid":
            run_validation(task, V)
        else:
            run_case(case, task, V)


if __name__ == "__main__":
    main()
