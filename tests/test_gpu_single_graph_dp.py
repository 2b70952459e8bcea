"""Data-parallel train() / test() on the sampled batches of ONE graph (the citation task's key "data_parallel").

In this process: the batches rank_train_batches deals to the ranks, interleaved, are train_batches' of a single process bit for bit,
and a group of ONE rank is the single-GPU loop without a collective.  In two spawned ranks that share the card over gloo
(tests/single_graph_dp_cases.py): two epochs of train(group=WORLD) and a test(group=WORLD), replayed afterwards by this process
alone: per step the step's batches in rank order through the same kernels, each gradient packed with its scale by the same launch,
the two buffers added (a sum of two has one order), one clip and update.  The replay must give the bits of every reduced gradient, of
every variable and optimizer slot, and of the losses the ranks reported; an evaluation epoch the ranks split must be the epoch a
single process computes over all the batches.  The ranks and the replay run with gemm=torch, as in tests/test_gpu_dp_train.py."""
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import single_graph_dp_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_same_batch(got, want, where):
    assert (got.num_graphs, got.num_nodes, got.num_edges) == (want.num_graphs, want.num_nodes, want.num_edges), where
    assert _same_bits(got.extra["sampled_nodes"], want.extra["sampled_nodes"]), where
    assert len(got.adjacency_lists) == len(want.adjacency_lists) == 3
    for a, b in zip(got.adjacency_lists, want.adjacency_lists):
        assert a.dtype == torch.int32 and _same_bits(a, b), where
    assert _same_bits(got.type_to_num_incoming_edges, want.type_to_num_incoming_edges), where
    assert _same_bits(got.initial_node_features, want.initial_node_features), where
    assert _same_bits(got.extra["labels"], want.extra["labels"]) and _same_bits(got.extra["mask"], want.extra["mask"]), where
    assert got.extra["out_layer_dropout_keep_prob"] == want.extra["out_layer_dropout_keep_prob"]
    assert ("layer_graphs" in got.extra) == ("layer_graphs" in want.extra)
    for a, b in zip(got.extra.get("layer_graphs", ()), want.extra.get("layer_graphs", ())):
        assert (a.num_sources, a.num_targets) == (b.num_sources, b.num_targets), where
        assert all(_same_bits(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists)), where
        assert _same_bits(a.type_to_num_incoming_edges, b.type_to_num_incoming_edges), where
    assert ("loss_normalisation" in got.extra) == ("loss_normalisation" in want.extra)
    if "loss_normalisation" in want.extra:
        (weights, denominator), (want_weights, want_denominator) = got.extra["loss_normalisation"], want.extra["loss_normalisation"]
        assert denominator == want_denominator and _same_bits(weights, want_weights), where
        # the per-message weights: preset as the scale of the batch graph's degree table
        assert _same_bits(got.graph.degree_scale(got.type_to_num_incoming_edges), want.graph.degree_scale(want.type_to_num_incoming_edges)), where


# =================================================================================================================================
# the ranks' batches are the single process's
# =================================================================================================================================
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind", ["sampled", "layered", "subgraph", "subgraph_normalisation"])
def test_the_ranks_batches_interleaved_are_the_batches_of_one_process(gpu_device, kind, world):
    from tf_gnn_samples_amd.tasks import DataFold
    alone = C.citation_task(kind, 54)
    ranks = [C.citation_task(kind, 54) for _ in range(world)]
    for task in [alone] + ranks:
        task.bind_sampling_device(gpu_device)
    fold = lambda task: task._loaded_data[DataFold.TRAIN][0]
    for epoch in range(2):
        want = list(alone.batches.train_batches(fold(alone)))
        dealt = [list(task.batches.rank_train_batches(fold(task), r, world)) for r, task in enumerate(ranks)]
        assert len(want) == 4 and [len(d) for d in dealt] == [len(range(r, 4, world)) for r in range(world)]
        schedule = alone.train_schedule(alone._loaded_data[DataFold.TRAIN], world)        # (of the NEXT epoch: the same owners and steps)
        for j, batch in enumerate(want):
            assert (schedule.owner[j], schedule.step[j]) == (j % world, j // world)
            _assert_same_batch(dealt[j % world][j // world], batch, "epoch %d, batch %d" % (epoch, j))
        if kind == "subgraph_normalisation":
            assert want[0].graph is not None and "loss_normalisation" in want[0].extra
        if kind == "layered":
            assert len(want[0].extra["layer_graphs"]) == 2
        # the counters went where the single process's went, on every rank
        assert all((task.batches.epoch, task.batches.draw) == (alone.batches.epoch, alone.batches.draw) == (epoch + 1, 4 * (epoch + 1))
                   for task in ranks)
    # the two epochs differ (another permutation, other draws): the comparison above was not of one batch with itself
    again = list(alone.batches.train_batches(fold(alone)))
    assert not all(_same_bits(a.extra["sampled_nodes"], b.extra["sampled_nodes"]) for a, b in zip(again, want))


# =================================================================================================================================
# a group of one rank is the single-GPU loop
# =================================================================================================================================
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_a_group_of_one_rank_with_the_key_is_the_single_gpu_loop_without_a_collective(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    from tf_gnn_samples_amd.tasks import DataFold
    assert not dist.is_initialized()
    dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)
    try:
        issued = []
        for name in ("all_reduce", "all_gather", "all_gather_object", "all_gather_into_tensor", "broadcast", "barrier", "reduce",
                     "broadcast_object_list"):
            monkeypatch.setattr(dist, name, lambda *a, _name=name, **k: issued.append(_name))
        task = C.citation_task("sampled_evaluation", 54)
        grouped = C.citation_model(task, gpu_device, tmp_path, "grouped")
        grouped.train(quiet=True, max_epochs=1, group=dist.group.WORLD)
        grouped.test(task.synthetic_test_data, quiet=True, group=dist.group.WORLD)
        assert issued == []
        alone = C.citation_model(C.citation_task("sampled_evaluation", 54, data_parallel=False), gpu_device, tmp_path, "alone")
        alone.train(quiet=True, max_epochs=1)
        a, b = C.model_state(grouped), C.model_state(alone)
        assert a[2] == b[2] == 4
        assert all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and all(_same_bits(x, y) for x, y in zip(a[1], b[1]))
        assert grouped.validation_history == alone.validation_history
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()


# =================================================================================================================================
# two ranks
# =================================================================================================================================
class _Packed(Exception):
    pass


def _run_two_ranks(kind, num_train, tmp_path, refusals=False):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=C.worker, args=(r, 2, port, q, kind, num_train, str(tmp_path), refusals)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=240) for _ in range(2)), key=lambda d: d["rank"])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:                    # (a rank that is still there after a failure waits for a peer that is gone)
            if p.is_alive():
                p.kill()
    return results


def _tally(results):
    """An epoch's loss as EpochTally adds it up: every batch is the ONE graph."""
    loss = 0.0
    for m in results:
        loss += m["loss"] * 1
    return loss / max(len(results), 1)


def _replay(kind, num_train, device, result_dir):
    """The run of the two ranks, alone.  -> (the reduced flat gradient of every step, per epoch (train loss, per-batch train metrics,
    the validation epoch), the state after the last epoch, the test epoch)."""
    from tf_gnn_samples_amd.parallel import PackedGradientAllReducer
    from tf_gnn_samples_amd.tasks import DataFold
    task = C.citation_task(kind, num_train, data_parallel=False)
    model = C.citation_model(task, device, result_dir, run_id="replay")
    train, valid = task._loaded_data[DataFold.TRAIN], task._loaded_data[DataFold.VALIDATION]
    reducer = PackedGradientAllReducer(model.optimizer.params)
    forward, seen = model.forward_batch, []

    def recording_forward(batch, training):
        out = forward(batch, training)
        if training:
            seen.append(out)
        return out

    model.forward_batch = recording_forward
    task.bind_sampling_device(device)
    steps_out, epochs = [], []
    for epoch in range(2):
        schedule = task.train_schedule(train, 2)
        batches = list(task.batches.train_batches(train[0]))             # (the interleaving test: these are the ranks' batches)
        assert len(batches) == len(schedule.owner) and schedule.draws[0] == epoch * len(batches)
        del seen[:]
        for k in range(schedule.steps):
            buffers = []
            for r in range(2):
                scale = float(schedule.scales[r, k])
                if 2 * k + r < len(batches):
                    def pack_and_stop(params, s=scale):
                        buffers.append(reducer.pack(s).clone())
                        raise _Packed()                                  # the gradient is all the replay wants of this train_step
                    with pytest.raises(_Packed):
                        model.train_step(batches[2 * k + r], grad_hook=pack_and_stop, lr_num_graphs=1)
                else:
                    assert scale == 0.0 and r == 1
                    model.optimizer.zero_grad()
                    buffers.append(reducer.pack(0.0).clone())
            reducer.flat.copy_(buffers[0] + buffers[1])                  # the two-operand fp32 sum of the collective
            steps_out.append(reducer.flat.detach().cpu().numpy().copy())
            for p, v in zip(reducer.params, reducer.views):
                p.grad = v
            model.optimizer.clip_and_step(model._lr_scale(1))
        metrics = [C.host_metrics(m) for m in seen]
        assert len(metrics) == len(batches)
        valid_epoch = model._run_epoch("validation", valid, DataFold.VALIDATION, quiet=True)
        epochs.append((_tally(metrics), metrics, valid_epoch))
    test_epoch = model._run_epoch("Test", list(task.synthetic_test_data), DataFold.TEST, quiet=True)
    return steps_out, epochs, C.model_state(model), test_epoch, task


def _check_two_ranks(kind, num_train, gpu_device, tmp_path, batches, evaluation_batches, refusals=False):
    from tf_gnn_samples_amd import config
    results = _run_two_ranks(kind, num_train, tmp_path, refusals)
    a, b = results
    steps_per_epoch = -(-batches // 2)
    # identical state on both ranks, and everything they report
    assert a["t"] == b["t"] == 2 * steps_per_epoch
    assert all(_same_bits(x, y) for x, y in zip(a["params"], b["params"])) and len(a["params"]) == len(b["params"]) > 0
    assert all(_same_bits(x, y) for x, y in zip(a["slots"], b["slots"])) and len(a["slots"]) == len(b["slots"]) > 0
    assert a["epochs"] == b["epochs"] and a["history"] == b["history"] and [e for e, _ in a["history"]] == [1, 2]
    assert a["counters"] == b["counters"] == (2, 2 * batches)
    assert len(a["reduced"]) == len(b["reduced"]) == a["t"] and all(_same_bits(x, y) for x, y in zip(a["reduced"], b["reduced"]))
    assert [name for name, *_ in a["epochs"]] == ["epoch 1 (training)", "epoch 1 (validation)", "epoch 2 (training)",
                                                  "epoch 2 (validation)", "Test"]
    with config.override(gemm=C.REPLAY_GEMM):
        steps, epochs, state, test_epoch, task = _replay(kind, num_train, gpu_device, tmp_path)
    assert len(steps) == a["t"]
    for k, (mine, theirs) in enumerate(zip(steps, a["reduced"])):
        assert _same_bits(mine, theirs), "step %d: %d of %d floats of the reduced gradient differ, by at most %.3g" % (
            k, int((mine.view(np.int32) != theirs.view(np.int32)).sum()), mine.size, float(np.abs(mine - theirs).max()))
    params, slots, t = state
    assert t == a["t"]
    assert all(_same_bits(x, y) for x, y in zip(params, a["params"])) and all(_same_bits(x, y) for x, y in zip(slots, a["slots"]))
    for e, (train_loss, train_metrics, valid_epoch) in enumerate(epochs):
        _, loss, metrics, graphs = a["epochs"][2 * e]
        assert len(metrics) == batches and graphs == batches
        assert metrics == train_metrics and loss == train_loss, "epoch %d: the training epoch in batch order" % (e + 1)
        _, loss, metrics, graphs = a["epochs"][2 * e + 1]
        assert len(metrics) == evaluation_batches and graphs == 1
        assert metrics == [C.host_metrics(m) for m in valid_epoch[1]] and loss == valid_epoch[0] and valid_epoch[2] == 1
        assert a["history"][e] == (e + 1, task.early_stopping_metric(valid_epoch[1], 1))
    _, loss, metrics, graphs = a["epochs"][4]
    assert metrics == [C.host_metrics(m) for m in test_epoch[1]] and loss == test_epoch[0] and graphs == 1
    return results


@pytest.mark.timeout(300)
def test_two_ranks_sampled_batches_pair_sixteen_seeds_with_six(gpu_device, tmp_path):
    """n_train = 54: the second step's batches weigh 16 / 22 and 6 / 22.  150 validation nodes in evaluation batches of 64: rank 0 runs
    batches 0 and 2, rank 1 batch 1, and the merged epoch is the single process's."""
    results = _check_two_ranks("sampled_evaluation", 54, gpu_device, tmp_path, batches=4, evaluation_batches=3, refusals=True)
    for r in results:
        refusals = dict(r["refusals"])
        assert refusals["without the key"] is not None and "cannot be split by graph" in refusals["without the key"]
        assert refusals["overlap"] is not None and "overlap" in refusals["overlap"] and "not wired" in refusals["overlap"]
        assert refusals["capture_train_step"] is not None and "sampled batch" in refusals["capture_train_step"]
        assert refusals["predict"] is not None and "cannot be split by graph" in refusals["predict"]
        assert refusals["predict nodes"] is not None and "cannot be split by graph" in refusals["predict nodes"]
        assert refusals["iterator"] is not None and "cannot be split by graph" in refusals["iterator"]


@pytest.mark.timeout(300)
def test_two_ranks_sampled_batches_with_a_last_step_one_rank_has_no_batch_for(gpu_device, tmp_path):
    """n_train = 70: five batches, the fifth alone in its step with scale 1, zeros from rank 1."""
    _check_two_ranks("sampled_evaluation", 70, gpu_device, tmp_path, batches=5, evaluation_batches=3)


@pytest.mark.timeout(300)
def test_two_ranks_normalised_subgraph_batches_weigh_the_same_and_validate_on_the_full_graph(gpu_device, tmp_path):
    """R = 16, h = 2 with GraphSAINT's normalisation: every rank pre-samples everything; every batch of a step weighs 1 / 2; each rank
    evaluates the full graph itself."""
    _check_two_ranks("subgraph_normalisation", 54, gpu_device, tmp_path, batches=4, evaluation_batches=1)
