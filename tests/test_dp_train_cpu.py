"""Data-parallel train() / test() (Sparse_Graph_Model.train(group=...)), the host side: the schedule every
rank derives from the exchanged batch plans, the plan over a real GraphStore, the exchange and the metric merge over gloo, the
tasks' loss_weight hook and the host-side argument checks of include/relgnn_parallel.h (tests/test_abi.py holds the header itself).
The GPU half is tests/test_gpu_dp_train.py."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


# ---- the schedule as a pure function --------------------------------------------------------------------------------------------
def test_schedule_of_unequal_ranks_and_a_rank_without_batches():
    from tf_gnn_samples_amd.parallel import dp_schedule
    per_rank = [[(310.0, 2), (95.0, 1), (120.0, 1)], [], [(205.0, 1), (77.0, 1)], [(1.0, 1)]]
    s = dp_schedule(per_rank)
    assert s.steps == 3
    assert s.weight_sums.dtype == np.float64 and s.weight_sums.tolist() == [516.0, 172.0, 120.0]
    assert s.graph_sums.tolist() == [4, 2, 1]
    assert s.scales.dtype == np.float32 and s.scales.shape == (4, 3)
    for r, p in enumerate(per_rank):
        for k in range(3):
            want = np.float32(p[k][0] / s.weight_sums[k]) if k < len(p) else np.float32(0.0)      # the quotient formed in double
            assert s.scales[r, k] == want and not np.signbit(s.scales[r, k])
    assert (s.scales[1] == 0).all() and s.scales[0, 2] == np.float32(1.0)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_the_scales_of_a_step_sum_to_one_within_an_ulp_per_rank(world):
    """Each scale is one rounding of an exact share: |s_r - w_r / W| <= ulp(1) / 2 (the shares are <= 1), so |sum_r s_r - 1| <= world * ulp / 2
    and the double sum of the float32 scales adds nothing to that: the bar is world * ulp(1)."""
    from tf_gnn_samples_amd.parallel import dp_schedule
    rng = np.random.RandomState(world)
    per_rank = [[(float(w), int(rng.randint(1, 9))) for w in rng.randint(1, 50000, size=int(rng.randint(0, 40)))] for _ in range(world)]
    per_rank[0] = [(float(w), 1) for w in rng.randint(1, 50000, size=40)]
    s = dp_schedule(per_rank)
    assert s.steps == 40
    total = s.scales.astype(np.float64).sum(axis=0)
    assert np.abs(total - 1.0).max() <= world * float(np.finfo(np.float32).eps)
    assert s.graph_sums.tolist() == [sum(p[k][1] for p in per_rank if k < len(p)) for k in range(40)]


def test_schedule_of_nobody_and_of_a_weightless_batch():
    from tf_gnn_samples_amd.parallel import dp_schedule
    s = dp_schedule([[], []])
    assert s.steps == 0 and s.scales.shape == (2, 0)
    with pytest.raises(ValueError, match="loss weight"):
        dp_schedule([[(0.0, 1)], [(3.0, 1)]])


# ---- the plan over a real GraphStore ----------------------------------------------------------------------------------------------
def _ppi_graphs(n=9, seed=4):
    from tf_gnn_samples_amd.tasks.synthetic import make_ppi_shaped_graphs
    return make_ppi_shaped_graphs(n, seed=seed, mean_nodes=150, std_nodes=50, min_nodes=60, max_nodes=260, fwd_edges_per_node=3.0,
                                  feature_size=8, num_labels=4)


def test_plan_over_a_store_is_what_the_iterator_assembles():
    from tf_gnn_samples_amd.parallel import dp_epoch_rng, dp_plan_epoch, dp_shard
    from tf_gnn_samples_amd.tasks import PPI_Task
    from tf_gnn_samples_amd.tasks.batcher import GraphStore
    graphs = _ppi_graphs()
    shards = dp_shard(graphs, 2)
    assert sorted(i for s in shards for i in s) == list(range(9)) and all(shards)
    task = PPI_Task(PPI_Task.default_params())
    mine = [graphs[i] for i in shards[1]]
    store = GraphStore(mine, 3, task.NODE_PAYLOADS, {})
    plan = dp_plan_epoch(store, True, 400, dp_epoch_rng(5, 1, 1))
    assert sorted(plan.ids.tolist()) == list(range(len(mine)))                               # every graph of the shard, once
    assert np.concatenate(plan.batches).tolist() == plan.ids.tolist()
    split = store.split_batches(plan.ids, 400)                                               # the rule iterate() applies
    assert len(split) == len(plan.batches) > 1 and all(np.array_equal(a, b) for a, b in zip(split, plan.batches))
    assert plan.graphs.tolist() == [len(b) for b in plan.batches]
    assert plan.nodes.tolist() == [sum(len(mine[i].node_features) for i in b) for b in plan.batches]
    assert all(n < 400 for n in plan.nodes)
    # the shuffle is the one make_native_minibatch_iterator draws from a generator seeded alike
    ids = np.arange(store.num_graphs)
    dp_epoch_rng(5, 1, 1).shuffle(ids)
    assert ids.tolist() == plan.ids.tolist()
    again = dp_plan_epoch(store, True, 400, dp_epoch_rng(5, 1, 1))
    assert again.ids.tolist() == plan.ids.tolist() and again.nodes.tolist() == plan.nodes.tolist()
    orders = {tuple(dp_plan_epoch(store, True, 400, dp_epoch_rng(5, e, 1)).ids.tolist()) for e in range(1, 7)}
    assert len(orders) > 1                                                                   # another epoch, another order
    assert dp_plan_epoch(store, True, 400, dp_epoch_rng(5, 1, 0)).ids.tolist() != plan.ids.tolist() or len(mine) < 3
    fixed = dp_plan_epoch(store, False, 400)
    assert fixed.ids.tolist() == list(range(len(mine)))                                      # evaluation folds keep their order
    empty = dp_plan_epoch(None, True, 400, dp_epoch_rng(5, 1, 1))
    assert empty.batches == [] and empty.graphs.shape == (0,)


def test_device_seeds_differ_by_rank_and_by_seed():
    from tf_gnn_samples_amd.parallel import dp_device_seed
    seeds = {dp_device_seed(s, r) for s in (0, 1, 5) for r in range(8)}
    assert len(seeds) == 24 and all(0 <= x < 2 ** 63 for x in seeds)
    assert dp_device_seed(5, 1) == dp_device_seed(5, 1)


# ---- the exchange and the metric merge over gloo ----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, num_graphs, q, result_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    from tf_gnn_samples_amd.parallel import (dp_epoch_rng, dp_exchange_plans, dp_merge_epoch, dp_plan_epoch, dp_schedule, dp_shard,
                                             init_distributed)
    from tf_gnn_samples_amd.tasks import PPI_Task
    from tf_gnn_samples_amd.tasks.batcher import GraphStore
    r, _, w = init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    graphs = _ppi_graphs(num_graphs)
    shards = dp_shard(graphs, world)
    mine = [graphs[i] for i in shards[rank]]
    task = PPI_Task(PPI_Task.default_params())
    store = GraphStore(mine, 3, task.NODE_PAYLOADS, {}) if mine else None
    plan = dp_plan_epoch(store, True, 300, dp_epoch_rng(3, 1, rank))
    plans = dp_exchange_plans(plan, max(len(s) for s in shards), dist.group.WORLD)
    schedule = dp_schedule([[(task.loss_weight(g, n), g) for g, n in p] for p in plans])
    metrics = [{"loss": float(rank) + 0.25 * k, "f1_score": 0.5, "step": (rank, k)} for k in range(len(plan.batches))]
    merged, totals = dp_merge_epoch(metrics, (float(plan.nodes.sum()), len(mine), int(plan.nodes.sum()), rank), dist.group.WORLD)
    refusal = None
    if world == 2:                                  # a model that is not on the GPU is refused by name (the check needs W > 1)
        from tf_gnn_samples_amd.models import RGCN_Model
        task.load_synthetic(2, 1, mean_nodes=60, std_nodes=5, min_nodes=40, max_nodes=80)
        p = RGCN_Model.default_params()
        p.update(hidden_size=16, graph_num_layers=1)
        model = RGCN_Model(p, task, run_id="cpu_rank%d" % rank, result_dir=result_dir, device="cpu")
        try:
            model.train(quiet=True, max_epochs=1, group=dist.group.WORLD)
        except RuntimeError as e:
            refusal = str(e)
    q.put((rank, shards[rank], list(zip(plan.graphs.tolist(), plan.nodes.tolist())), plans,
           (schedule.steps, schedule.weight_sums.tolist(), schedule.graph_sums.tolist(), schedule.scales.tolist()), merged, totals, refusal))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world,num_graphs", [(2, 7), (4, 3)], ids=["world2", "world4_one_shard_empty"])
def test_gloo_ranks_agree_on_plans_schedule_and_merged_metrics(world, num_graphs, tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, num_graphs, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=150) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shards = [r[1] for r in results]
    assert sorted(i for s in shards for i in s) == list(range(num_graphs))
    assert sum(1 for s in shards if not s) == (1 if world == 4 else 0)
    local = [r[2] for r in results]
    for _, _, _, plans, schedule, merged, totals, refusal in results:
        assert [[tuple(x) for x in p] for p in plans] == local                      # every rank's table, in rank order, on every rank
        assert schedule == results[0][4] and merged == results[0][5] and totals == results[0][6]
        assert (refusal is not None and "on the GPU" in refusal and "cpu" in refusal) if world == 2 else refusal is None
    steps, weight_sums, graph_sums, scales = results[0][4]
    assert steps == max(len(p) for p in local)
    assert weight_sums == [float(sum(p[k][1] for p in local if k < len(p))) for k in range(steps)]        # PPI weighs by nodes
    assert graph_sums == [sum(p[k][0] for p in local if k < len(p)) for k in range(steps)]
    for r, p in enumerate(local):
        assert all(scales[r][k] == 0.0 for k in range(len(p), steps))
    merged, totals = results[0][5], results[0][6]
    assert [m["step"] for m in merged] == [(r, k) for r, p in enumerate(local) for k in range(len(p))]    # concatenated in rank order
    nodes = sum(n for p in local for _, n in p)
    assert totals == [float(nodes), float(num_graphs), float(nodes), float(sum(range(world)))]


# ---- the tasks' loss_weight hook ---------------------------------------------------------------------------------------------------
def test_loss_weight_is_what_each_task_normalises_its_loss_by():
    from tf_gnn_samples_amd.tasks import PPI_Task, QM9_Task, Sparse_Graph_Task
    from tf_gnn_samples_amd.tasks.citation_network_task import Citation_Network_Task
    from tf_gnn_samples_amd.tasks.varmisuse_task import VarMisuse_Task
    assert PPI_Task(PPI_Task.default_params()).loss_weight(3, 700) == 700.0
    assert QM9_Task(QM9_Task.default_params()).loss_weight(3, 700) == 3.0
    assert VarMisuse_Task(VarMisuse_Task.default_params()).loss_weight(3, 700) == 3.0
    with pytest.raises(RuntimeError, match="ONE graph"):
        Citation_Network_Task(Citation_Network_Task.default_params()).loss_weight(1, 2708)
    with pytest.raises(NotImplementedError, match="loss_weight"):
        Sparse_Graph_Task({}).loss_weight(1, 1)


def test_the_pack_refuses_bad_arguments_without_a_launch():
    """Argument checks run on the host in front of the launch: no GPU needed to see them."""
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    sizes = (ctypes.c_int64 * 2)(4, -1)
    table = (ctypes.c_void_p * 2)(None, None)
    assert lib.relgnn_mt_pack_scaled_f32(table, sizes, 2, 1.0, None, None) == _lib.EINVAL          # a negative size
    assert lib.relgnn_mt_pack_scaled_f32(table, sizes, _lib.MT_MAX + 1, 1.0, None, None) == _lib.EINVAL
    assert lib.relgnn_mt_pack_scaled_f32(table, sizes, -1, 1.0, None, None) == _lib.EINVAL
    assert lib.relgnn_mt_pack_scaled_f32(None, None, 0, 1.0, None, None) == _lib.OK                # nothing to do
    zeros = (ctypes.c_int64 * 2)(0, 0)
    assert lib.relgnn_mt_pack_scaled_f32(table, zeros, 2, 1.0, None, None) == _lib.OK              # sizes of 0 are legal
    sizes = (ctypes.c_int64 * 2)(4, 4)
    assert lib.relgnn_mt_pack_scaled_f32(table, sizes, 2, 1.0, None, None) == _lib.EINVAL          # something to write, nowhere to


# ---- the public interface ---------------------------------------------------------------------------------------------------------
def test_train_and_test_take_a_group_that_defaults_to_none():
    import inspect
    from tf_gnn_samples_amd.models import Sparse_Graph_Model
    assert list(inspect.signature(Sparse_Graph_Model.train).parameters) == ["self", "quiet", "max_epochs", "group"]
    assert list(inspect.signature(Sparse_Graph_Model.test).parameters) == ["self", "data", "quiet", "group"]
    assert inspect.signature(Sparse_Graph_Model.train).parameters["group"].default is None
