"""`"blocks": true` on the GPU (csrc/level_plan.hip; tasks/neighbour_sampling.py: derived_level_graphs; ops/rgcn.py: target rows only):
the derived level bucketings against the ordinary constructor bit for bit, models on one HopSubgraph with and without derived levels,
exact evaluation fields and predict(nodes=...) with the key, train() with the key on both input pipelines and under "data_parallel",
and the peak memory of a step."""
import math
import multiprocessing as mp
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import block_levels_dp_cases as DP  # noqa: E402
import block_levels_reference as BR  # noqa: E402
import layered_sampling_reference as LR  # noqa: E402
import test_gpu_layered_sampling as TL  # noqa: E402   (its graphs, models, float64 run and relation: helpers, not tests)
import test_gpu_sampled_evaluation as SE  # noqa: E402
import test_gpu_single_graph_dp as SG  # noqa: E402

pytestmark = pytest.mark.gpu

V = LR.V
FLOOR = 2.0 ** -22


def assert_the_constructor_s(graph, lists, sources, targets, what):
    """Every array RelGraph(prefix lists, S, validate=False) computes, both row pointers included, bit for bit."""
    from tf_gnn_samples_amd.graph import RelGraph
    want = RelGraph(lists, sources, validate=False)
    assert (graph.V, graph.L, graph.M, graph.edge_counts, graph.num_targets) == (sources, want.L, want.M, want.edge_counts, targets), what
    assert want.num_targets == sources
    for name in BR.ARRAYS:
        got, ref = getattr(graph, name), getattr(want, name)
        assert got.dtype == torch.int32 and got.is_contiguous() and got.shape == ref.shape, (what, name, tuple(got.shape), tuple(ref.shape))
        assert torch.equal(got, ref), (what, name, int((got != ref).sum()))
    for got, ref in zip(graph.adjacency_lists, lists):
        assert got.shape == ref.shape and (got.numel() == 0 or got.data_ptr() == ref.data_ptr())           # the prefix views
    return want


def check_derived(sub, graphs, what, route_like=None):
    H = len(sub.hop_nodes) - 1
    assert len(graphs) == H
    union = graphs[0]
    assert (union.V, union.num_targets) == (sub.num_nodes, sub.hop_nodes[H - 1])
    assert all(got.data_ptr() == ref.data_ptr() or ref.numel() == 0 for got, ref in zip(union.adjacency_lists, sub.adjacency_lists))
    for layer in range(2, H + 1):
        d = H - layer
        lists = [a[:edges[d]] for a, edges in zip(sub.adjacency_lists, sub.hop_edges)]
        graph = graphs[layer - 1]
        assert_the_constructor_s(graph, lists, sub.hop_nodes[d + 1], sub.hop_nodes[d], (what, "layer", layer))
        assert graph.M == 0 or graph.col_t.data_ptr() == union.col_t.data_ptr()                          # a view of the union's


@pytest.mark.parametrize("fanouts", [[3, 2], [2, 2, 2], [0, 4], [3]], ids=str)
@pytest.mark.parametrize("L", [1, 2, 3])
def test_derived_levels_are_the_constructor_s_bit_for_bit(gpu_device, L, fanouts):
    """The graphs, seed lists and fanouts of tests/test_block_levels_cpu.py (an edge type with no edges and a level that adds none:
    "dead_end"; a hop that reached nothing new, T = S: "all"; M = 0 and levels with no edges: "isolated") and H = 1, where the union
    graph is all there is.  With three edge types "all" holds more entries than one tile of the compaction."""
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler, derived_level_graphs
    sampler = NeighbourSampler(TL.device_graph(L, gpu_device), fanouts, seed=11, replica=2)
    tile = _lib.load_library().relgnn_level_plan_tile()
    sizes = {}
    for name, seeds in LR.seed_lists(L).items():
        sub = sampler.sample_by_hop(torch.as_tensor(seeds, device=gpu_device), 7)
        check_derived(sub, derived_level_graphs(sub), (L, fanouts, name))
        sizes[name] = (sub.num_edges, sub.hop_nodes, sub.hop_edges)
        levels = sub.level_graphs(derived=True)
        plain = sub.level_graphs()
        for level, ref in zip(levels, plain):
            assert level.graph is not None and (level.num_sources, level.num_targets) == (ref.num_sources, ref.num_targets)
            assert (level.graph.V, level.graph.num_targets) == (level.num_sources, level.num_targets)
            assert torch.equal(level.type_to_num_incoming_edges, ref.type_to_num_incoming_edges)
    assert sizes["isolated"][0] == 0 and sizes["all"][1][0] == sizes["all"][1][1] == V
    if L == 3 and len(fanouts) > 1:
        assert sizes["all"][0] > tile                                  # more than one tile of the compaction
    if L > 1:
        assert sizes["dead_end"][2][1][-1] == 0                        # an edge type with no edges


def hand_built(device, L, empty_type=None, seed=0):
    """A hop-ordered subgraph of H = 3 written by hand: ONE source (the first node of hop 1) with 5 000 type-0 edges into the seeds,
    50 into hop 1 and 30 into hop 2, so its by-source bucket crosses five tiles and is thinned at both derived levels; random edges
    around it.  Per type the edges with a target in hop d stand in front of those of hop d + 1, shuffled inside a hop."""
    from tf_gnn_samples_amd.tasks.neighbour_sampling import HopSubgraph
    rng = np.random.default_rng(seed)
    n = [5200, 5300, 5400, 5500]
    hub = n[0]
    lists, hop_edges = [], []
    for l in range(L):
        parts, cumulative = [], []
        for d, (extra, own) in enumerate(((300, 5000), (400, 50), (300, 30))):
            lo = 0 if d == 0 else n[d - 1]
            tgt = rng.integers(lo, n[d], size=extra)
            src = rng.integers(0, n[d + 1], size=extra)
            if l == 0:
                mine = np.arange(own) if d == 0 else rng.integers(lo, n[d], size=own)
                tgt, src = np.concatenate([tgt, mine]), np.concatenate([src, np.full(own, hub)])
            if l == empty_type:
                tgt, src = tgt[:0], src[:0]
            e = np.stack([src, tgt], axis=1)[rng.permutation(len(tgt))]
            parts.append(e)
            cumulative.append(len(e) + (cumulative[-1] if cumulative else 0))
        lists.append(torch.as_tensor(np.ascontiguousarray(np.concatenate(parts), dtype=np.int32), device=device))
        hop_edges.append(cumulative)
    total = sum(e[-1] for e in hop_edges)
    return HopSubgraph(None, lists, None, None, n[-1], total, n, hop_edges), hub


@pytest.mark.parametrize("L, empty_type", [(1, None), (2, None), (3, 1)])
def test_a_source_with_five_thousand_out_edges_and_a_side_stream(gpu_device, L, empty_type):
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.neighbour_sampling import derived_level_graphs
    sub, hub = hand_built(gpu_device, L, empty_type)
    tile = _lib.load_library().relgnn_level_plan_tile()
    assert sub.num_edges > 5 * tile and sub.num_edges % tile != 0
    graphs = derived_level_graphs(sub)
    check_derived(sub, graphs, ("hand built", L))
    union = graphs[0]
    bucket = (int(union.rowptr_s[hub * L]), int(union.rowptr_s[hub * L + 1]))
    assert bucket[1] - bucket[0] >= 5080 and bucket[0] // tile + 4 <= (bucket[1] - 1) // tile          # one bucket over five tiles
    kept = [int(g.rowptr_s[hub * L + 1] - g.rowptr_s[hub * L]) for g in graphs]
    assert kept[0] > kept[1] > kept[2] >= 5000
    # the same bits on a stream that is not the default one
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        again = derived_level_graphs(sub)
        side.synchronize()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    for a, b in zip(graphs, again):
        assert all(torch.equal(getattr(a, name), getattr(b, name)) for name in BR.ARRAYS)
    check_derived(sub, again, ("hand built on a side stream", L))


# ---- models on one HopSubgraph, with and without derived levels ---------------------------------------------------------------------
def _two_batches(task, device, fanouts, num_seeds=32):
    fold, sub = TL._hop_subgraph(task, device, fanouts, num_seeds=num_seeds)
    tables = (torch.as_tensor(fold.node_features, device=device), torch.as_tensor(fold.labels, device=device),
              torch.as_tensor(fold.mask, device=device))
    assert sub.num_nodes < 4096                                        # (every product below the row count where the Dense route changes)
    return fold, sub, sub.device_batch(*tables, 1.0, layered=True), sub.device_batch(*tables, 1.0, layered=True, derived=True)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _layer_rows(model):
    """The row count of every layer's output, straight from the layer function."""
    rows, real = [], model._apply_gnn_layer

    def recording(*args, **kwargs):
        out = real(*args, **kwargs)
        rows.append(int(out.shape[0]))
        return out
    model._apply_gnn_layer = recording
    return rows


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("fanouts", [[3, 2], [3, 2, 2]], ids=str)
@pytest.mark.parametrize("model_name", ["GGNN_Model", "RGAT_Model", "GNN_FiLM_Model"])
def test_models_without_a_rectangular_route_give_the_same_bits(gpu_device, monkeypatch, model_name, fanouts, norm):
    """The same arrays through the same kernels: loss, seed states, seed logits, num_correct and every gradient bit for bit; the
    batch with derived levels bucketed ONE graph when it was made and the model buckets nothing."""
    from tf_gnn_samples_amd import graph as graph_module
    built, real = [], graph_module.RelGraph.__init__
    monkeypatch.setattr(graph_module.RelGraph, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    H = len(fanouts)
    task = TL._citation_task()
    before = len(built)
    fold, sub, plain_batch, blocks_batch = _two_batches(task, gpu_device, fanouts)
    assert len(built) - before == 2                                    # the sampler's full graph (_hop_subgraph) and the union graph
    n0 = sub.hop_nodes[0]
    model = TL._model(model_name, task, gpu_device, H, graph_inter_layer_norm=norm, graph_residual_connection_every_num_layers=2)
    rows = _layer_rows(model)
    levels = blocks_batch.extra["layer_graphs"]
    assert blocks_batch.graph is levels[0].graph and all(level.graph is not None for level in levels)
    before = len(built)
    blocks, _ = TL._forward_and_gradients(model, blocks_batch, n0)
    assert len(built) == before and rows == [level.num_sources for level in levels]          # no rectangular route: all rows
    plain, _ = TL._forward_and_gradients(model, plain_batch, n0)
    assert len(built) - before == H                                    # the model bucketed every level itself
    differing = [name for name in plain if not _same_bits(plain[name], blocks[name])]
    assert not differing, differing


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("fanouts", [[3, 2], [3, 2, 2]], ids=str)
def test_rgcn_computes_the_target_rows_only(gpu_device, fanouts, norm):
    """RGCN's default route: every layer returns its level's num_targets rows (the rectangular route ran), loss, seed states and seed
    logits are the plain layered run's bit for bit, and every gradient lies within twice the plain layered run's own distance from a
    float64 run of the un-layered model, plus 2^-22 (tests/test_gpu_layered_sampling.py, check_relation: the weight gradient sums
    over fewer rows in other tiles).  Every figure is printed before anything is asserted."""
    from tf_gnn_samples_amd import ops
    H = len(fanouts)
    task = TL._citation_task()
    fold, sub, plain_batch, blocks_batch = _two_batches(task, gpu_device, fanouts)
    n0 = sub.hop_nodes[0]
    model = TL._model("RGCN_Model", task, gpu_device, H, graph_inter_layer_norm=norm, graph_residual_connection_every_num_layers=2)
    rows = _layer_rows(model)
    levels = blocks_batch.extra["layer_graphs"]
    ops.ROUTES["rgcn_rows"] = None
    blocks, _ = TL._forward_and_gradients(model, blocks_batch, n0)
    assert ops.ROUTES["rgcn_rows"] == "targets"
    assert rows == [level.num_targets for level in levels] and rows[0] < levels[0].num_sources and rows[-1] == n0
    del rows[:]
    plain, _ = TL._forward_and_gradients(model, plain_batch, n0)
    assert ops.ROUTES["rgcn_rows"] == "all" and rows == [level.num_sources for level in levels]
    want = TL._float64_run(model, "RGCN_Model", fold, sub)
    report = []
    for name in want:
        a, b = TL.deviation(blocks[name], want[name]), TL.deviation(plain[name], want[name])
        report.append((name, a, b, _same_bits(blocks[name], plain[name])))
        print("RGCN H=%d norm=%s %s: blocks %.3g  layered %.3g  bound %.3g  identical bits: %s" % (H, norm, name, a, b, 2 * b + FLOOR, report[-1][3]))
    for name, a, b, same in report:
        if name.startswith("grad "):
            assert math.isfinite(a) and a <= 2 * b + FLOOR, (name, a, b)
        else:
            assert same, name                                          # loss, seed states, seed logits, num_correct: the forward


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
def _evaluation_pair(L, H, device, **model_params):
    """Two tasks over SE's hub graph and two RGCN models from one seed: exact evaluation fields with and without the key."""
    out = {}
    for blocks in (False, True):
        more = dict(blocks=True) if blocks else {}
        task = SE.citation_task(L, SE.sampled({"fanouts": [0] * H, "seeds_per_batch": 32}, **more))
        out[blocks] = (task, SE.make_model("RGCN_Model", task, device, H, **model_params))
    return out


@pytest.mark.parametrize("H, L", [(2, 2), (2, 3), (3, 2)])
def test_exact_fields_with_the_key_are_the_full_graph_s_rows(gpu_device, monkeypatch, H, L):
    """All fanouts 0, "evaluation" and "blocks": for every seed of every batch the logits are the full-graph forward's rows bit for bit,
    under either iterator: the resident full graph splits the 5 000-entry hub bucket inside the field (full_graph_route: the derived
    levels carry its SplitPlan on the whole row pointer, and the rectangular gather runs on that object), the one the model buckets
    itself folds it in one wave.  A batch buckets ONE graph, not H; the epoch's loss, counts and accuracy are those of the run without
    the key."""
    from tf_gnn_samples_amd import graph as graph_module, ops
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    pair = _evaluation_pair(L, H, gpu_device)
    built, real = [], graph_module.RelGraph.__init__
    monkeypatch.setattr(graph_module.RelGraph, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    task, model = pair[True]
    assert task.blocks and task.evaluation is not None and not task.layered
    for native in (True, False):
        epochs = {}
        for blocks, (task, model) in pair.items():
            model.params["native_batching"] = native
            for B in (32, 7):
                task.params["sampled_batches"]["evaluation"]["seeds_per_batch"] = B
                data = task._loaded_data[DataFold.VALIDATION]
                (full_batch,) = model._batches(data, DataFold.VALIDATION, full_graph=True)
                if not isinstance(full_batch, DeviceBatch):
                    full_batch = DeviceBatch(full_batch, model.device)
                _, full_logits = SE.states_and_logits(model, full_batch)
                list(model._batches(data, DataFold.VALIDATION))         # (the fold's sampler and the device's full graph are built once)
                before = len(built)
                batches = list(model._batches(data, DataFold.VALIDATION))
                assert len(built) - before == len(batches) * (1 if blocks else H)
                seen = []
                for i, batch in enumerate(batches):
                    levels = batch.extra["layer_graphs"]
                    n0 = levels[-1].num_targets
                    seeds = batch.extra["sampled_nodes"][:n0].cpu().numpy()
                    seen.extend(seeds.tolist())
                    assert all(level.graph is not None and level.graph.has_long_buckets == native for level in levels)
                    assert all(level.graph.num_targets == (level.num_targets if blocks else level.num_sources) for level in levels)
                    ops.ROUTES["rgcn_rows"] = None
                    states, logits = SE.states_and_logits(model, batch)
                    assert ops.ROUTES["rgcn_rows"] == ("targets" if blocks else "all")
                    assert SE.same_bits(logits, full_logits[seeds]), (H, L, native, blocks, B, i)
                assert seen == SE.VALID and max(b.num_nodes for b in batches) > 100               # the hub's bucket sits inside a field
                loss, res, graphs, _, _, _ = model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)
                epochs[(blocks, B)] = (loss, [(m["total_loss"], m["num_masked"], m["num_correct"]) for m in res], graphs)
        for B in (32, 7):
            assert epochs[(True, B)] == epochs[(False, B)], (native, B)


def test_predict_nodes_with_the_key_gives_the_same_classes_and_probabilities(gpu_device):
    pair = _evaluation_pair(3, 2, gpu_device)
    nodes = [40, 5, SE.HUB, 5, 11, 12, 13, 14, 15, 200, 201, 299, 7]
    out = {blocks: model.predict(task.synthetic_test_data, nodes=nodes, return_states=True) for blocks, (task, model) in pair.items()}
    assert np.array_equal(out[True]["nodes"], out[False]["nodes"]) and np.array_equal(out[True]["classes"], out[False]["classes"])
    assert SE.same_bits(out[True]["probabilities"], out[False]["probabilities"])
    assert SE.same_bits(out[True]["node_states"], out[False]["node_states"])
    (full,) = pair[True][1].predict(pair[True][0].synthetic_test_data)
    assert SE.same_bits(out[True]["probabilities"], full["probabilities"][np.asarray(nodes)])


def test_kept_evaluation_batches_build_nothing_in_the_second_epoch(gpu_device, monkeypatch):
    from tf_gnn_samples_amd import graph as graph_module
    from tf_gnn_samples_amd.tasks import DataFold
    built, real = [], graph_module.RelGraph.__init__
    monkeypatch.setattr(graph_module.RelGraph, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    task = SE.citation_task(2, SE.sampled({"fanouts": [0, 0], "seeds_per_batch": 7, "keep": True}, blocks=True))
    model = SE.make_model("RGCN_Model", task, gpu_device, 2)
    data = task._loaded_data[DataFold.VALIDATION]
    first = model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)
    count = len(built)
    second = model._run_epoch("validation", data, DataFold.VALIDATION, quiet=True)
    assert len(built) == count and first[0] == second[0] and [dict(m) for m in first[1]] == [dict(m) for m in second[1]]
    a, b = list(model._batches(data, DataFold.VALIDATION)), list(model._batches(data, DataFold.VALIDATION))
    assert len(a) == 3 and all(x is y for x, y in zip(a, b))
    for batch in a:                                                    # one col_t per batch: the derived level reads the union's
        union, level = (lv.graph for lv in batch.extra["layer_graphs"])
        assert level.M == 0 or level.col_t.data_ptr() == union.col_t.data_ptr()


# ---- training ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native_batching", [True, False], ids=["native", "numpy"])
def test_train_with_the_key(gpu_device, tmp_path, native_batching):
    """Two epochs of train() with the key and without it from one seed: the same epochs, steps and counters; the first step's loss is
    the same float (the forward's bits are), every loss is finite; the checkpoint carries the key."""
    from tf_gnn_samples_amd import models, ops
    sampled = dict(TL.SAMPLED, blocks=True)
    ops.ROUTES["rgcn_rows"] = None
    task, model, record = TL._train_two_epochs(gpu_device, tmp_path / "blocks", sampled, native_batching=native_batching)
    _, _, plain = TL._train_two_epochs(gpu_device, tmp_path / "layered", dict(TL.SAMPLED), native_batching=native_batching)
    assert [(r[0], r[1], r[2], r[3]) for r in record] == [(r[0], r[1], r[2], r[3]) for r in plain]
    assert [(r[1], r[2]) for r in record] == [(5, 5), (1, 1), (5, 5), (1, 1)] and record[0][3] == [32.0, 32.0, 32.0, 32.0, 12.0]
    assert all(math.isfinite(x) for r in record for x in r[4]) and record[0][4][0] == plain[0][4][0]
    assert (task.batches.epoch, task.batches.draw) == (2, 10)
    from tf_gnn_samples_amd.tasks import DataFold
    batch = next(iter(model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)))
    levels = batch.extra["layer_graphs"]
    assert len(levels) == 2 and batch.graph is levels[0].graph and [lv.graph.num_targets for lv in levels] == [lv.num_targets for lv in levels]
    float(model.forward_batch(batch, training=True)["loss"].detach())
    assert ops.ROUTES["rgcn_rows"] == "targets"
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.sampled_batches == sampled and restored.task.blocks and restored.task.layered


def _run_two_ranks(kind, num_train, tmp_path, refusals=False):
    """tests/test_gpu_single_graph_dp.py's, with the worker of tests/block_levels_dp_cases.py: the child knows the case "blocks"."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = SG._free_port()
    procs = [ctx.Process(target=DP.worker, args=(r, 2, port, q, kind, num_train, str(tmp_path), refusals)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=240) for _ in range(2)), key=lambda d: d["rank"])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return results


@pytest.mark.timeout(300)
def test_two_ranks_with_the_key_are_the_one_process_replay(gpu_device, tmp_path, monkeypatch):
    """"layered", "evaluation", "blocks" and "data_parallel": two ranks over gloo on one card, two epochs of train(group=WORLD) and a
    test(group=WORLD), against the replay of the same schedule by this process (tests/test_gpu_single_graph_dp.py, _check_two_ranks):
    the reduced gradient of every step, the parameters, the slots and every epoch's metrics, bit for bit."""
    monkeypatch.setattr(SG, "_run_two_ranks", _run_two_ranks)
    SG._check_two_ranks(DP.KIND, 54, gpu_device, tmp_path, batches=4, evaluation_batches=3)


def test_a_step_with_the_key_peaks_no_higher(gpu_device):
    """The peak device memory of a training step on a batch with derived levels is at most the peak of the step on the plain layered
    batch of the same HopSubgraph; both are read here, from the same resting state, after a warming step each."""
    task = TL._citation_task()
    fold, sub = TL._hop_subgraph(task, gpu_device, [5, 5], num_seeds=64)
    tables = (torch.as_tensor(fold.node_features, device=gpu_device), torch.as_tensor(fold.labels, device=gpu_device),
              torch.as_tensor(fold.mask, device=gpu_device))
    peaks = {}
    for which in ("layered", "blocks"):
        model = TL._model("RGCN_Model", task, gpu_device, 2, hidden_size=128)
        batch = sub.device_batch(*tables, 1.0, layered=True, derived=which == "blocks")
        model.train_step(batch)                                        # warm: plans, scratch, the bucketing of every level
        model.optimizer.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(gpu_device)
        before = torch.cuda.memory_allocated(gpu_device)
        model.train_step(batch)
        model.optimizer.zero_grad()
        torch.cuda.synchronize()
        peaks[which] = torch.cuda.max_memory_allocated(gpu_device) - before
        del model, batch
    print("peak of a step above the resting state: layered %d bytes, with derived levels and target rows %d bytes (%d nodes, %d one hop "
          "out, %d seeds)" % (peaks["layered"], peaks["blocks"], sub.hop_nodes[2], sub.hop_nodes[1], sub.hop_nodes[0]))
    assert 0 < peaks["blocks"] <= peaks["layered"], peaks
