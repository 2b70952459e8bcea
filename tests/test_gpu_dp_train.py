"""Data-parallel train() / test() on the GPU (Sparse_Graph_Model.train(group=...)).

In this process: the multi-tensor scaled pack (csrc/parallel.hip, include/relgnn_parallel.h) bit for bit against torch, and a
group of ONE rank, which must be the single-GPU loop without a collective.  In two spawned ranks (process handling as in
tests/test_gpu_dp.py: both ranks on cuda:0 over gloo when one device is visible, nccl on two devices): two epochs of
train(group=WORLD), replayed afterwards by the parent alone: every rank's local gradient through the same kernels, packed with its
scale by the new kernel, the two buffers added in fp32, the same clip and update.  A two-operand fp32 sum has one order, so the replay
must give the bits of every reduced step gradient and of the final parameters.

The ranks and the replay run with the switch gemm=torch (REPLAY_GEMM below): on the default route a product the limb kernels do
not take (hidden size 64) goes to hipBLASLt through csrc/blaslt_gemm.hip, which keeps ONE solution per 4096-row bucket of the node
count, the one the heuristic named for the first batch the PROCESS saw in that bucket.  The bits of a batch's gradient then depend
on which batch its process met first, so one process cannot stand in for two ranks there: measured on an MI355X, rank 1's first
scaled gradient differed from the replay's in 34 204 of 39 737 floats by at most 1.5e-8 (one ulp), and equalled, bit for bit, what a
fresh process gives that computes rank 1's batch first.  torch.mm asks the library per exact shape; everything the feature adds
(plan, schedule, pack, collective, update) is the same code on either route."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


# =================================================================================================================================
# the pack kernel
# =================================================================================================================================
def _pack(grads, sizes, scale, dst):
    """relgnn_mt_pack_scaled_f32 over any number of tensors: chunks of _lib.MT_MAX, the destination advancing (what
    PackedGradientAllReducer.pack does)."""
    from tf_gnn_samples_amd import _lib
    at = 0
    for c0 in range(0, len(grads), _lib.MT_MAX):
        chunk, n = grads[c0:c0 + _lib.MT_MAX], sizes[c0:c0 + _lib.MT_MAX]
        table = (ctypes.c_void_p * len(chunk))(*[None if g is None else g.data_ptr() for g in chunk])
        _lib.launch("relgnn_mt_pack_scaled_f32", table, (ctypes.c_int64 * len(chunk))(*n), len(chunk), float(scale),
                    dst.data_ptr() + 4 * at)
        at += sum(n)
    return at


def _expected(grads, sizes, scale):
    parts = [torch.zeros(n, dtype=torch.float32, device="cuda") if g is None else (g * scale).flatten() for g, n in zip(grads, sizes)]
    return torch.cat(parts) if parts else torch.zeros(0, device="cuda")


SENTINEL = -7.25


def _check(grads, scale, dst_offset=0):
    """Pack into a sentinel-filled buffer at `dst_offset` floats; the packed range has the bits of torch's g * scale, every float
    in front of it and behind it is untouched."""
    sizes = [n if g is None else g.numel() for g, n in grads]
    tensors = [g for g, _ in grads]
    total = sum(sizes)
    buf = torch.full((dst_offset + total + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    assert _pack(tensors, sizes, scale, buf[dst_offset:]) == total
    want = _expected(tensors, sizes, scale)
    got = buf[dst_offset:dst_offset + total]
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        "first differing element: %s" % (got.view(torch.int32) != want.view(torch.int32)).nonzero()[:1].tolist()
    assert bool((buf[:dst_offset] == SENTINEL).all()) and bool((buf[dst_offset + total:] == SENTINEL).all())


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).cuda()


# the kernel gives a block 4096 elements behind the 0-3 scalar head elements of a slice: its edges, and the edges of two blocks
ELEMENT_COUNTS = [0, 1, 3, 4, 5, 4095, 4096, 4097, 70001, 4098, 4099, 4100, 8191, 8192, 8193, 8195]


def test_pack_element_counts_and_odd_destination_offsets(gpu_device):
    """All the sizes in ONE call, in this order: the slices behind sizes 1, 3 and 5 start at every 4-byte phase of a 16-byte line."""
    grads = [(_randn(n, 100 + i), n) for i, n in enumerate(ELEMENT_COUNTS)]
    _check(grads, 1.0 / 3.0)
    for n in ELEMENT_COUNTS:                                  # and each size alone, at each phase of the destination
        for phase in range(4) if n in (0, 1, 3, 4, 5, 4097, 70001) else (1,):
            _check([(_randn(n, n), n)], 1.0 / 3.0, dst_offset=phase)


@pytest.mark.parametrize("count", [1, 48, 49, 97])
def test_pack_tensor_counts_across_the_chunk_of_48(gpu_device, count):
    rng = np.random.RandomState(count)
    grads = [(_randn(int(n), 7 * i), int(n)) for i, n in enumerate(rng.randint(0, 41, size=count))]
    _check(grads, 1.0 / 3.0)


def test_pack_sources_that_are_views_at_odd_offsets(gpu_device):
    base = _randn(3 * 5000 + 16, 3)
    grads = [(base[1:1 + 4097], 4097), (base[5003:5003 + 4096], 4096), (base[10002:10002 + 9], 9), (base[15001:15004], 3)]
    assert sorted({(g.data_ptr() // 4) % 4 for g, _ in grads}) == [1, 2, 3]
    for phase in range(4):                                    # every source phase against every destination phase
        _check(grads, 1.0 / 3.0, dst_offset=phase)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_pack_null_entries_write_positive_zeros(gpu_device, where):
    grads = [(_randn(n, n), n) for n in (5, 4097, 3, 64, 7)]
    holes = {"first": [0], "middle": [2], "last": [4], "all": [0, 1, 2, 3, 4]}[where]
    for i in holes:
        grads[i] = (None, grads[i][1])
    _check(grads, 1.0 / 3.0)
    _check(grads, -2.0, dst_offset=3)                         # +0.0, not scale * 0 = -0.0 (the comparison is by bits)


@pytest.mark.parametrize("scale", [1.0, 0.0, 1.0 / 3.0, 2.0 ** -20], ids=["one", "zero", "third", "two_to_minus_20"])
def test_pack_scales_and_special_values(gpu_device, scale):
    tiny = float(np.finfo(np.float32).tiny)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), tiny, -tiny, tiny / 8, 1e-45, -1e-45, 0.0, -0.0, 3.4e38, -3.4e38,
                            1.0, -1.0, 1.17549421e-38], dtype=torch.float32).cuda()
    x = torch.cat([special, _randn(4100, 9) * 1e-30, special, _randn(70, 10), special[:3]])
    _check([(x, x.numel()), (special, special.numel()), (x[1:], x.numel() - 1)], scale)


def test_pack_runs_on_the_current_non_default_stream(gpu_device):
    from tf_gnn_samples_amd import _lib
    side = torch.cuda.Stream()
    g = _randn(300000, 1)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert _lib.current_stream() == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        big = torch.zeros(1 << 26, device="cuda")
        for _ in range(8):
            big.add_(1.0)                                     # work queued on the side stream in front of the source's last write
        g.copy_(big[:300000] * 0.5)
        buf = torch.full((300000 + 8,), SENTINEL, device="cuda")
        _pack([g], [300000], 0.25, buf)
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()                                        # the side stream alone: the pack was ordered behind the copy on it
    assert bool((buf[:300000] == 1.0).all()) and bool((buf[300000:] == SENTINEL).all())


def test_packed_reducer_packs_every_variable_in_optimizer_order(gpu_device):
    """97 variables (three launches), some without a gradient, one whose gradient is not contiguous."""
    from tf_gnn_samples_amd.parallel import PackedGradientAllReducer
    rng = np.random.RandomState(0)
    params = [torch.nn.Parameter(torch.zeros(int(a), int(b), device="cuda")) for a, b in rng.randint(1, 12, size=(97, 2))]
    frozen = torch.nn.Parameter(torch.zeros(5, device="cuda"), requires_grad=False)
    for i, p in enumerate(params):
        if i % 10 != 3:
            p.grad = _randn(p.numel(), i).view_as(p)
    params[5].grad = _randn(params[5].numel(), 5).view(params[5].shape[1], params[5].shape[0]).t()
    reducer = PackedGradientAllReducer(params[:40] + [frozen] + params[40:])
    assert len(reducer.params) == 97 and reducer.flat.numel() == sum(p.numel() for p in params)
    flat = reducer.pack(1.0 / 3.0)
    want = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad * (1.0 / 3.0)).contiguous().flatten() for p in params])
    assert torch.equal(flat.view(torch.int32), want.view(torch.int32))
    for p, v in zip(params, reducer.views):
        assert v.shape == p.shape and v.data_ptr() >= flat.data_ptr()
    with pytest.raises(Exception, match="GPU"):
        PackedGradientAllReducer([torch.nn.Parameter(torch.zeros(3))])


# =================================================================================================================================
# a group of one rank is the single-GPU loop
# =================================================================================================================================
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ppi_case(device, result_dir, run_id="dp", keep_prob=1.0):
    """7 training and 3 validation graphs of 60-260 nodes; max_nodes_in_batch = 400 gives each of two ranks two or three batches.
    With synthetic seed 7 and random_seed 5 the first epoch has 2 batches on rank 0 and 3 on rank 1 (the second 3 and 3)."""
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(7, 3, seed=7, mean_nodes=150, std_nodes=60, min_nodes=60, max_nodes=260, fwd_edges_per_node=6.0)
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, graph_layer_input_dropout_keep_prob=keep_prob, random_seed=5, max_nodes_in_batch=400,
             optimizer="Adam")
    return task, RGCN_Model(p, task, run_id=run_id, result_dir=str(result_dir), device=str(device))


def _qm9_case(device, result_dir, run_id="dp"):
    """GGNN with its default optimizer on 48 + 16 molecules of the committed QM9 file, the learning rate scaled by the graphs of a step."""
    sys.path.insert(0, str(ROOT / "tests"))
    from test_golden_cpu import read_qm9_fixture
    from tf_gnn_samples_amd.models import GGNN_Model
    from tf_gnn_samples_amd.tasks import DataFold, QM9_Task
    task = QM9_Task(QM9_Task.default_params())
    raw = read_qm9_fixture()
    task._loaded_data[DataFold.TRAIN] = task.load_raw(raw[:48])
    task._loaded_data[DataFold.VALIDATION] = task.load_raw(raw[48:64])
    p = GGNN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, random_seed=5, max_nodes_in_batch=120, lr_for_num_graphs_per_batch=8)
    return task, GGNN_Model(p, task, run_id=run_id, result_dir=str(result_dir), device=str(device))


CASES = {"ppi_rgcn": _ppi_case, "qm9_ggnn": _qm9_case}
REPLAY_GEMM = "torch"          # the route on which a batch's gradient bits do not depend on the process's earlier batches (module docstring)


def _state(model):
    """Parameters, optimizer slots and step count as host arrays."""
    torch.cuda.synchronize()
    opt = model.optimizer
    return ([p.detach().cpu().numpy().copy() for p in opt.params],
            [t.detach().cpu().numpy().copy() for _, slots in opt._slots() for t in slots], opt.t)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_a_group_of_one_rank_is_the_single_gpu_loop_without_a_collective(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)
    try:
        issued = []
        for name in ("all_reduce", "all_gather", "all_gather_object", "all_gather_into_tensor", "broadcast", "barrier", "reduce",
                     "broadcast_object_list"):
            monkeypatch.setattr(dist, name, lambda *a, _name=name, **k: issued.append(_name))
        _, grouped = _ppi_case(gpu_device, tmp_path, "grouped", keep_prob=0.8)
        seed_before = torch.cuda.initial_seed()
        grouped.train(quiet=True, max_epochs=1, group=dist.group.WORLD)
        from tf_gnn_samples_amd.tasks import DataFold
        grouped.test(grouped.task._loaded_data[DataFold.VALIDATION], quiet=True, group=dist.group.WORLD)
        assert issued == []                                          # asserted here: a refusal that needs W > 1 is checked in a worker
        assert torch.cuda.initial_seed() == seed_before              # no reseeding either
        _, alone = _ppi_case(gpu_device, tmp_path, "alone", keep_prob=0.8)
        alone.train(quiet=True, max_epochs=1)
        a, b = _state(grouped), _state(alone)
        assert a[2] == b[2] > 0
        assert all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and all(_same_bits(x, y) for x, y in zip(a[1], b[1]))
        assert grouped.validation_history == alone.validation_history
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()


# =================================================================================================================================
# two ranks
# =================================================================================================================================
def _worker(rank, world, port, share_gpu, q, case, result_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0" if share_gpu else str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    import tf_gnn_samples_amd.parallel as par
    from tf_gnn_samples_amd import config
    r, local_rank, w = par.init_distributed(backend="gloo" if share_gpu else "nccl")
    assert (r, w) == (rank, world)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    # what the parent compares: every exchanged plan and every reduced flat gradient, in the order they happened
    plans, reduced, packed = [], [], []
    exchange, reduce_call, pack = par.dp_exchange_plans, par.PackedGradientAllReducer.__call__, par.PackedGradientAllReducer.pack

    def recording_exchange(*a, **k):
        out = exchange(*a, **k)
        plans.append(out)
        return out

    def recording_call(self, scale):
        reduce_call(self, scale)
        reduced.append(self.flat.detach().cpu().numpy().copy())

    def recording_pack(self, scale):
        out = pack(self, scale)
        packed.append(out.detach().cpu().numpy().copy())      # this rank's own scaled gradient: lets a mismatch name its rank
        return out

    par.dp_exchange_plans = recording_exchange
    par.PackedGradientAllReducer.pack = recording_pack
    par.PackedGradientAllReducer.__call__ = recording_call
    config.settings.gemm = REPLAY_GEMM                        # (this process ends with the test)
    task, model = CASES[case](device, result_dir)
    model.train(quiet=True, max_epochs=2, group=dist.group.WORLD)
    params, slots, t = _state(model)
    out = dict(rank=rank, backend=dist.get_backend(), plans=plans, reduced=reduced, packed=packed, params=params, slots=slots, t=t,
               history=model.validation_history, best_epoch=model.best_epoch, device_seed=torch.cuda.initial_seed(),
               replica=int(model.dropout_state[1].item()), refusals=[])
    from tf_gnn_samples_amd.tasks import DataFold
    model.test(task._loaded_data[DataFold.VALIDATION], quiet=True, group=dist.group.WORLD)      # one fold, sharded the same way
    if case == "ppi_rgcn":
        def refused(what, fn):
            try:
                fn()
                out["refusals"].append((what, None))
            except Exception as e:
                out["refusals"].append((what, "%s: %s" % (type(e).__name__, e)))

        with config.override(allreduce="overlap"):
            refused("overlap", lambda: model.train(quiet=True, max_epochs=1, group=dist.group.WORLD))
        model.params['native_batching'] = False
        refused("native_batching", lambda: model.train(quiet=True, max_epochs=1, group=dist.group.WORLD))
        model.params['native_batching'] = True
        from tf_gnn_samples_amd.tasks.citation_network_task import Citation_Network_Task
        citation = Citation_Network_Task(Citation_Network_Task.default_params())
        refused("citation", lambda: next(citation.make_minibatch_iterator([], DataFold.TRAIN, 10)))
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


class _Packed(Exception):
    pass


def _replay(case, device, result_dir, results):
    """The run of the two ranks, alone: returns (reduced flat gradient per step of every epoch, the two packed buffers per step, the
    state after each epoch, the union gradient of step 1 from one batch)."""
    from tf_gnn_samples_amd.parallel import PackedGradientAllReducer, dp_epoch_rng, dp_plan_epoch, dp_schedule, dp_shard
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    task, model = CASES[case](device, result_dir, run_id="replay")
    seed, max_nodes = model.params['random_seed'], model.params['max_nodes_in_batch']
    data = task._loaded_data[DataFold.TRAIN]
    shards = dp_shard(data, 2)
    mine = [[data[i] for i in s] for s in shards]
    pipelines = [model._native_pipeline(m) for m in mine]
    reducer = PackedGradientAllReducer(model.optimizer.params)
    steps_out, packed_out, union, after_epoch = [], [], None, []
    for epoch in (1, 2):
        local = [dp_plan_epoch(p.store, True, max_nodes, dp_epoch_rng(seed, epoch, r)) for r, p in enumerate(pipelines)]
        tables = [list(zip(pl.graphs.tolist(), pl.nodes.tolist())) for pl in local]
        assert tables == [[tuple(x) for x in p] for p in results[0]["plans"][2 * (epoch - 1)]], "epoch %d: the exchanged plan" % epoch
        schedule = dp_schedule([[(task.loss_weight(g, n), g) for g, n in t] for t in tables])
        if epoch == 1 and case == "ppi_rgcn":                  # step 1 as ONE batch of both ranks' graphs, before anything is updated
            graphs = [mine[r][i] for r in range(2) for i in local[r].batches[0]]
            mb = next(task.make_minibatch_iterator(graphs, DataFold.VALIDATION, 10 ** 9))
            model.optimizer.zero_grad()
            model.forward_batch(DeviceBatch(mb, device), training=True)['loss'].backward()
            union = [p.grad.detach().cpu().numpy().copy() for p in model.optimizer.params]
        iterators = [iter(task.make_native_minibatch_iterator(p, DataFold.TRAIN, max_nodes, rng=dp_epoch_rng(seed, epoch, r)))
                     for r, p in enumerate(pipelines)]
        for k in range(schedule.steps):
            buffers = []
            for r in range(2):
                scale = float(schedule.scales[r, k])
                if k < len(tables[r]):
                    def pack_and_stop(params, s=scale):
                        buffers.append(reducer.pack(s).clone())
                        raise _Packed()                        # the gradient is all the replay wants of this train_step
                    with pytest.raises(_Packed):
                        model.train_step(next(iterators[r]), grad_hook=pack_and_stop)
                else:
                    assert scale == 0.0
                    model.optimizer.zero_grad()
                    buffers.append(reducer.pack(0.0).clone())
            reducer.flat.copy_(buffers[0] + buffers[1])        # the two-operand fp32 sum of the collective
            steps_out.append(reducer.flat.detach().cpu().numpy().copy())
            packed_out.append([b.cpu().numpy() for b in buffers])
            for p, v in zip(reducer.params, reducer.views):
                p.grad = v
            model.optimizer.clip_and_step(model._lr_scale(int(schedule.graph_sums[k])))
        for it in iterators:
            assert next(it, None) is None
        after_epoch.append(_state(model))
    return steps_out, packed_out, after_epoch, union


def _run_two_ranks(case, tmp_path):
    world = 2
    share_gpu = torch.cuda.device_count() < 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, share_gpu, q, case, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=240) for _ in range(world)), key=lambda d: d["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert results[0]["backend"] == ("gloo" if share_gpu else "nccl")
    return results


def _check_two_ranks(case, gpu_device, tmp_path):
    from tf_gnn_samples_amd.models import restore
    from tf_gnn_samples_amd.parallel import dp_device_seed
    results = _run_two_ranks(case, tmp_path)
    a, b = results
    # identical state on both ranks
    assert a["t"] == b["t"] > 0
    assert all(_same_bits(x, y) for x, y in zip(a["params"], b["params"])) and len(a["params"]) == len(b["params"]) > 0
    assert all(_same_bits(x, y) for x, y in zip(a["slots"], b["slots"])) and len(a["slots"]) == len(b["slots"])
    assert a["history"] == b["history"] and [e for e, _ in a["history"]] == [1, 2] and a["best_epoch"] == b["best_epoch"] in (1, 2)
    assert a["plans"] == b["plans"] and len(a["plans"]) == 5          # train, validation per epoch; the test fold
    assert len(a["reduced"]) == len(b["reduced"]) == a["t"] and all(_same_bits(x, y) for x, y in zip(a["reduced"], b["reduced"]))
    train_plans = [a["plans"][0], a["plans"][2]]
    assert a["t"] == sum(max(len(p) for p in plan) for plan in train_plans)      # Adam's t (the step count) advanced on every rank, every step
    assert all(min(len(p) for p in plan) >= 2 for plan in train_plans)           # several batches per rank
    # seeding
    assert [a["device_seed"], b["device_seed"]] == [dp_device_seed(5, 0), dp_device_seed(5, 1)] and a["device_seed"] != b["device_seed"]
    assert [a["replica"], b["replica"]] == [0, 1]
    # files: one pickle, one log, rank 0's
    files = sorted(os.listdir(tmp_path))
    assert files == ["dp.log", "dp_best_model.pickle"], files
    log = (tmp_path / "dp.log").read_text()
    assert log.count("== Epoch 1") == 1 and log.count("Model has") == 1 and log.count("Training took") == 1
    # the replay
    from tf_gnn_samples_amd import config
    with config.override(gemm=REPLAY_GEMM):
        steps, packed, after_epoch, union = _replay(case, gpu_device, tmp_path, results)
    assert len(steps) == a["t"]
    restored = restore(str(tmp_path / "dp_best_model.pickle"), str(tmp_path), run_id="restored", device=str(gpu_device))
    names, sizes = restored._trainable_names(), [p.numel() for p in restored.optimizer.params]

    def differing(mine, theirs):
        """Which variables differ, how many floats, the largest difference."""
        out, at = [], 0
        for name, n in zip(names, sizes):
            x, y = mine[at:at + n], theirs[at:at + n]
            bad = int((x.view(np.int32) != y.view(np.int32)).sum())
            if bad:
                out.append("%s: %d of %d, max |diff| %.3g of max |value| %.3g" % (name, bad, n, float(np.abs(x - y).max()), float(np.abs(y).max())))
            at += n
        return "; ".join(out)

    for k in range(len(steps)):
        for r in range(2):
            assert _same_bits(packed[k][r], results[r]["packed"][k]), \
                "step %d, the scaled gradient of rank %d alone: %s" % (k, r, differing(packed[k][r], results[r]["packed"][k]))
        assert _same_bits(steps[k], a["reduced"][k]), "step %d, the sum of the two: %s" % (k, differing(steps[k], a["reduced"][k]))
    params, slots, t = after_epoch[-1]
    assert t == a["t"]
    assert all(_same_bits(x, y) for x, y in zip(params, a["params"])) and all(_same_bits(x, y) for x, y in zip(slots, a["slots"]))
    # rank 0's pickle is the model after its best epoch: rank 0's parameters and slots then (the final ones when that is the last)
    got, want = _state(restored), after_epoch[a["best_epoch"] - 1]
    assert all(_same_bits(x, y) for x, y in zip(got[0], want[0])) and all(_same_bits(x, y) for x, y in zip(got[1], want[1]))
    assert got[2] == want[2] or restored.optimizer.name != "adam"      # (the step count comes back through beta1_power: Adam only)
    return results, steps, union


@pytest.mark.timeout(300)
def test_two_ranks_ppi_rgcn_with_a_step_one_rank_has_no_batch_for(gpu_device, tmp_path):
    results, steps, union = _check_two_ranks("ppi_rgcn", gpu_device, tmp_path)
    train_plans = [results[0]["plans"][0], results[0]["plans"][2]]
    assert any(len(plan[0]) != len(plan[1]) for plan in train_plans)             # a zero-weight step really ran
    # step 1 against the gradient of the union batch from one process (the bar of tests/test_gpu_dp.py for the same comparison)
    offset = 0
    for g in union:
        got = results[0]["reduced"][0][offset:offset + g.size].reshape(g.shape)
        offset += g.size
        assert np.abs(got - g).max() <= 2e-6 + 1e-5 * np.abs(g).max(), np.abs(got - g).max()
    assert offset == results[0]["reduced"][0].size
    for r in results:
        refusals = dict(r["refusals"])
        assert refusals["overlap"] is not None and "overlap" in refusals["overlap"] and "not wired" in refusals["overlap"]
        assert refusals["native_batching"] is not None and "native_batching" in refusals["native_batching"]
        assert refusals["citation"] is not None and "ONE graph" in refusals["citation"]


@pytest.mark.timeout(300)
def test_two_ranks_qm9_ggnn_weighs_by_graphs_and_scales_the_rate_by_the_global_count(gpu_device, tmp_path):
    results, steps, _ = _check_two_ranks("qm9_ggnn", gpu_device, tmp_path)
    plan = results[0]["plans"][0]
    assert sum(g for p in plan for g, _ in p) == 48
    # (the replay applied lr * G_k / 8 with G_k the graphs of BOTH ranks and weights = graphs; it matched bit for bit above)
    assert all(len(p) >= 2 for p in plan)
