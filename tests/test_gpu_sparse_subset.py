"""SparseRows.take_rows on the GPU (csrc/sparse_subset.hip, include/relgnn_sparse_subset.h): every array of the subset, its transpose
and both plans bit for bit against tests/sparse_subset_reference.py; the device split_plan on its own; the CSR projection over the
result against a host-built container, the full projection and float64; streams and over-allocated buffers; the citation task with
`sparse_node_features` and `sampled_batches` + "sparse_features": true together.

One structure (V = 1300, F = 800) holds forward rows of 0, 1, 63, 64, 65, 128, 129, 130, 512, 513 and 700 entries and words held by
0, 1, 128, 129, 512, 513 and 1025 nodes: both sides of the split threshold (128), one slab exactly (512), two slabs, and three."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import sparse_features_reference as R  # noqa: E402
import sparse_subset_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

_HELD = {}


def device_rows(device):
    """The structure's container on the device, built once."""
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    key = str(device)
    if key not in _HELD:
        rowptr, col, val = S.structure()
        _HELD[key] = SparseRows(rowptr, col, val, (S.V, S.F)).to(device)
    return _HELD[key]


def host_built(name, device):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    want = S.reference(name).rows
    return SparseRows(want.rowptr, want.col, want.val, S.reference(name).shape).to(device)


@pytest.mark.parametrize("name", list(S.subsets()))
def test_every_array_equals_the_reference(gpu_device, name):
    from tf_gnn_samples_amd.tasks import sparse_features
    rows = device_rows(gpu_device)
    nodes = S.subsets()[name]
    sparse_features.ROUTES["take_rows"] = None
    got = rows.take_rows(torch.as_tensor(nodes, device=gpu_device))
    assert sparse_features.ROUTES["take_rows"] == "hip" and got.device == rows.device
    S.compare(got, S.reference(name), name)
    S.compare(rows.take_rows(nodes, validated=True), S.reference(name), name + " (a host list, trusted)")
    S.compare(host_built(name, gpu_device), S.reference(name), name + " (the host constructor)")
    if name == "all":                                                        # the container itself
        for side in ("rows", "transposed"):
            for field in S.FIELDS:
                assert torch.equal(getattr(getattr(got, side), field), getattr(getattr(rows, side), field)), (side, field)


def test_empty_and_bad_node_lists(gpu_device):
    from tf_gnn_samples_amd.tasks import sparse_features
    rows = device_rows(gpu_device)
    empty = rows.take_rows(torch.zeros(0, dtype=torch.int32, device=gpu_device))
    assert sparse_features.ROUTES["take_rows"] == "host"                     # no launch
    assert empty.shape == (0, S.F) and empty.nnz == 0 and empty.device == rows.device
    for bad in (np.array([0, S.V], np.int32), np.array([-1], np.int32), np.array([1, 2], np.int64), np.array([[1, 2]], np.int32)):
        with pytest.raises(ValueError):
            rows.take_rows(torch.as_tensor(bad, device=gpu_device))


def _plan_on_the_device(rowptr, device, pad=0):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    num_rows = len(rowptr) - 1
    ptr = torch.as_tensor(np.asarray(rowptr, np.int32), device=device)
    offsets = torch.empty((num_rows + 1, 4), dtype=torch.int32, device=device)
    sizes = torch.empty(3, dtype=torch.int32, device=device)
    nbytes = lib.relgnn_split_plan_workspace_bytes(num_rows)
    ws = _lib.scratch(nbytes, device)
    _lib.launch("relgnn_split_plan_count", _lib.ptr(ptr), num_rows, _lib.ptr(offsets), _lib.ptr(sizes), _lib.ptr(ws), nbytes)
    num_slabs, num_combos, ws_rows = sizes.tolist()
    slabs = torch.full((num_slabs + pad, 4), -7, dtype=torch.int32, device=device)
    combos = torch.full((num_combos + pad, 3), -7, dtype=torch.int32, device=device)
    _lib.launch("relgnn_split_plan_fill", _lib.ptr(ptr), num_rows, _lib.ptr(offsets), _lib.ptr(slabs) if num_slabs + pad else None, num_slabs,
                _lib.ptr(combos) if num_combos + pad else None, num_combos)
    return slabs.cpu().numpy(), combos.cpu().numpy(), ws_rows, (num_slabs, num_combos)


def test_device_split_plan_against_the_host_s(gpu_device):
    from tf_gnn_samples_amd.tasks.sparse_features import split_plan
    long_rows = np.array([3, 128, 0, 129, 512, 17, 513, 1024, 1025, 0, 5000, 64, 700, 128])
    short_rows = np.array([0, 1, 128, 64, 0, 127, 128])
    for lengths in (long_rows, short_rows, np.zeros(0, np.int64)):
        rowptr = np.concatenate([[0], np.cumsum(lengths)])
        want_slabs, want_combos, want_ws = split_plan(rowptr)
        slabs, combos, ws_rows, (num_slabs, num_combos) = _plan_on_the_device(rowptr, gpu_device, pad=3)
        assert (num_slabs, num_combos, ws_rows) == (len(want_slabs), len(want_combos), want_ws)
        assert np.array_equal(slabs[:num_slabs], want_slabs) and np.array_equal(combos[:num_combos], want_combos)
        assert (slabs[num_slabs:] == -7).all() and (combos[num_combos:] == -7).all()           # nothing behind the stated capacity
    assert len(split_plan(np.concatenate([[0], np.cumsum(long_rows)]))[1]) == 5 and not len(split_plan(np.concatenate([[0], np.cumsum(short_rows)]))[0])


OP_SUBSET = "a node twice"


@pytest.mark.parametrize("act", ["tanh", "linear"])
@pytest.mark.parametrize("n", [4, 64, 260, 320])
def test_projection_over_the_subset(gpu_device, n, act):
    """csr_rows_project over take_rows(S) and its weight gradient: the bits of the same call on a host-built container, forward rows
    = rows S of the full projection, both inside the float64 bounds of tests/sparse_features_reference.py."""
    from tf_gnn_samples_amd import ops
    act_id = ops.activation_id(None if act == "linear" else act)
    rows = device_rows(gpu_device)
    nodes = S.subsets()[OP_SUBSET]
    want = S.reference(OP_SUBSET)
    rng = np.random.default_rng([5, n])
    weight, gout = R._signed(rng, (S.F, n)), R._signed(rng, (len(nodes), n))
    results = {}
    for which, container in (("device", rows.take_rows(torch.as_tensor(nodes, device=gpu_device))), ("host", host_built(OP_SUBSET, gpu_device))):
        W = torch.as_tensor(weight, device=gpu_device).clone().requires_grad_(True)
        out = ops.csr_rows_project(container, W, act_id)
        assert ops.ROUTES["csr_project"] == "hip"
        out.backward(torch.as_tensor(gout, device=gpu_device))
        results[which] = (out.detach().cpu().numpy(), W.grad.cpu().numpy())
    for a, b, what in zip(results["device"], results["host"], ("forward", "weight gradient")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    out, grad = results["device"]
    full = ops.csr_rows_project(rows, torch.as_tensor(weight, device=gpu_device), act_id).cpu().numpy()
    assert np.array_equal(out.view(np.uint32), full[nodes].view(np.uint32))
    csr = R.Csr(want.rows.rowptr.astype(np.int64), want.rows.col.astype(np.int64), want.rows.val, want.shape)
    value, tol, _ = R.forward_act64(csr, weight, act)
    err = np.abs(out.astype(np.float64) - value)
    print("forward n %d %s: worst error / tolerance %.3f" % (n, act, float((err / np.maximum(tol, 1e-300))[tol > 0].max())))
    assert (err <= tol).all()
    t = R.Csr(want.transposed.rowptr.astype(np.int64), want.transposed.col.astype(np.int64), want.transposed.val, (S.F, len(nodes)))
    res, gtol = R.gradient64(t, gout, out, act)
    gerr = np.abs(grad.astype(np.float64) - res.value)
    print("weight gradient n %d %s: worst error / tolerance %.3f" % (n, act, float((gerr / np.maximum(gtol, 1e-300))[gtol > 0].max())))
    assert (gerr <= gtol).all() and not grad[gtol == 0].any()
    assert int(np.diff(t.rowptr).max()) > 128 and int(np.diff(csr.rowptr).max()) == 700


def _raw_take(rows, nodes, pad):
    """The C entry points with every output buffer `pad` elements longer than the subset's sizes, filled with a sentinel."""
    from tf_gnn_samples_amd import _lib
    lib, s, dev = _lib.load_library(), rows.rows, rows.device
    V, F = rows.shape
    n = int(nodes.shape[0])
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    f32 = lambda k: torch.full((k,), -7.0, dtype=torch.float32, device=dev)
    sub_rowptr, sub_rowptr_t, offsets, offsets_t, sizes = i32(n + 1 + pad), i32(F + 1 + pad), i32(n + 1, 4), i32(F + 1, 4), i32(8 + pad)
    nbytes = lib.relgnn_sparse_subset_count_workspace_bytes(n, F)
    ws = _lib.scratch(nbytes, dev)
    _lib.launch("relgnn_sparse_subset_count", _lib.ptr(s.rowptr), _lib.ptr(s.col), V, F, _lib.ptr(nodes), n, _lib.ptr(sub_rowptr),
                _lib.ptr(sub_rowptr_t), _lib.ptr(offsets), _lib.ptr(offsets_t), _lib.ptr(sizes), _lib.ptr(ws), nbytes)
    nnz, *plan = sizes.tolist()[:7]
    out = {"rowptr": sub_rowptr, "rowptr_t": sub_rowptr_t, "sizes": sizes, "col": i32(nnz + pad), "val": f32(nnz + pad),
           "col_t": i32(nnz + pad), "val_t": f32(nnz + pad)}
    _lib.launch("relgnn_sparse_subset_copy", _lib.ptr(s.rowptr), _lib.ptr(s.col), _lib.ptr(s.val), V, _lib.ptr(nodes), n,
                _lib.ptr(sub_rowptr), nnz, _lib.ptr(out["col"]), _lib.ptr(out["val"]))
    nbytes = lib.relgnn_sparse_subset_transpose_workspace_bytes(nnz, F)
    ws = _lib.scratch(nbytes, dev)
    _lib.launch("relgnn_sparse_subset_transpose", _lib.ptr(sub_rowptr), n, _lib.ptr(out["col"]), _lib.ptr(out["val"]), nnz, F,
                _lib.ptr(out["col_t"]), _lib.ptr(out["val_t"]), _lib.ptr(ws), nbytes)
    for tag, ptr, off, (num_slabs, num_combos, _), num_rows in (("", sub_rowptr, offsets, plan[:3], n), ("_t", sub_rowptr_t, offsets_t, plan[3:], F)):
        out["slabs" + tag], out["combos" + tag] = i32(num_slabs + pad, 4), i32(num_combos + pad, 3)
        _lib.launch("relgnn_split_plan_fill", _lib.ptr(ptr), num_rows, _lib.ptr(off), _lib.ptr(out["slabs" + tag]), num_slabs,
                    _lib.ptr(out["combos" + tag]), num_combos)
    return out, (n, F, nnz, plan)


def test_same_bits_again_on_a_side_stream_and_nothing_behind_the_sizes(gpu_device):
    rows = device_rows(gpu_device)
    name = "every second"
    nodes = torch.as_tensor(S.subsets()[name], device=gpu_device)
    want = S.reference(name)
    for _ in range(2):
        S.compare(rows.take_rows(nodes, validated=True), want, name)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        on_side = rows.take_rows(nodes, validated=True)
        on_side.record_stream(torch.cuda.current_stream(gpu_device))       # a per-batch container: its tensors are recorded
        side.synchronize()
        S.compare(on_side, want, name + " on a side stream")
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    pad = 37
    out, (n, F, nnz, plan) = _raw_take(rows, nodes, pad)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    assert nnz == len(want.rows.col) and plan == [len(want.rows.slabs), len(want.rows.combos), want.rows.ws_rows,
                                                  len(want.transposed.slabs), len(want.transposed.combos), want.transposed.ws_rows]
    pairs = (("rowptr", want.rows.rowptr, n + 1), ("rowptr_t", want.transposed.rowptr, F + 1), ("col", want.rows.col, nnz), ("val", want.rows.val, nnz),
             ("col_t", want.transposed.col, nnz), ("val_t", want.transposed.val, nnz), ("slabs", want.rows.slabs, plan[0]),
             ("combos", want.rows.combos, plan[1]), ("slabs_t", want.transposed.slabs, plan[3]), ("combos_t", want.transposed.combos, plan[4]))
    for key, expected, size in pairs:
        assert np.array_equal(host[key][:size], expected), key
        assert len(host[key][size:]) == pad and (host[key][size:] == -7).all(), key + ": written behind the stated size"
    assert (host["sizes"][8:] == -7).all() and host["sizes"][7] == 0


# ---- the task ---------------------------------------------------------------------------------------------------------------------
BOTH = {"fanouts": [3, 2], "seeds_per_batch": 16, "seed": 2, "sparse_features": True}


def _task(num_nodes=300, num_features=40, density=0.08, sampled=BOTH, **sizes):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    params = dict(Citation_Network_Task.default_params(), sparse_node_features=True)
    if sampled is not None:
        params["sampled_batches"] = sampled
    task = Citation_Network_Task(params)
    sizes = dict(dict(num_train=60, num_valid=60, num_test=60), **sizes)
    task.load_synthetic(num_nodes=num_nodes, num_features=num_features, num_classes=3, feature_density=density, seed=5, **sizes)
    return task


def _model(name, task, device, result_dir=None, **params):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(dict(dict(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=6), **params))
    extra = {} if result_dir is None else dict(run_id="both", result_dir=str(result_dir))
    return cls(p, task, device=str(device), **extra)


def _loss_and_gradients(model, batch):
    from tf_gnn_samples_amd import ops
    for p in model.variables.parameters():
        p.grad = None
    metrics = model.forward_batch(batch, training=False)
    metrics["loss"].backward()
    ops.join_deferred()
    torch.cuda.synchronize()
    grads = {n: (None if model.variables[n].grad is None else model.variables[n].grad.cpu().numpy().copy()) for n in model.variables.names()}
    return np.float32(float(metrics["loss"].detach())), grads


@pytest.mark.parametrize("model_name", ["RGCN_Model", "GGNN_Model"])
def test_every_sampled_batch_equals_the_hand_fed_one(gpu_device, model_name):
    """One epoch of sampled batches over sparse features; each batch's subgraph fed again through DeviceBatch(MinibatchData) with a
    HOST-built SparseRows of its nodes: the same loss and every variable's gradient, bit for bit (mean aggregation)."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, MinibatchData
    from tf_gnn_samples_amd.tasks import sparse_features
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows, node_stand_in
    task = _task()
    train = task._loaded_data[DataFold.TRAIN]
    fold = train[0]
    full = fold.node_features
    assert isinstance(full, SparseRows) and not full.is_cuda
    rowptr, col, val = (a.numpy() for a in (full.rows.rowptr, full.rows.col, full.rows.val))
    model = _model(model_name, task, gpu_device, message_aggregation_function="mean")
    batches = list(model._batches(train, DataFold.TRAIN))
    assert len(batches) == 4 and [float(b.extra["mask"].sum()) for b in batches] == [16.0, 16.0, 16.0, 12.0]
    assert sparse_features.ROUTES["take_rows"] == "hip"
    for i, batch in enumerate(batches):
        nodes = batch.extra["sampled_nodes"].cpu().numpy()
        taken = batch.extra["sparse_node_features"]
        assert tuple(batch.initial_node_features.shape) == (len(nodes), 1) and taken.shape == (len(nodes), 40) and taken.is_cuda
        assert task.compute_initial_node_features(batch, {}) is taken
        want = S.take_rows(rowptr, col, val, full.shape, nodes)
        S.compare(taken, want, "batch %d" % i)
        feed = {"initial_node_features": node_stand_in(len(nodes)), "adjacency_lists": [a.cpu().numpy() for a in batch.adjacency_lists],
                "type_to_num_incoming_edges": batch.type_to_num_incoming_edges.cpu().numpy(), "num_graphs": 1,
                "labels": batch.extra["labels"].cpu().numpy(), "mask": batch.extra["mask"].cpu().numpy(), "out_layer_dropout_keep_prob": 1.0,
                "sparse_node_features": SparseRows(want.rows.rowptr, want.rows.col, want.rows.val, want.shape)}
        by_hand = DeviceBatch(MinibatchData(feed, 1, len(nodes), batch.num_edges), gpu_device)
        ops.ROUTES["csr_project"] = None
        loss_a, grads_a = _loss_and_gradients(model, batch)
        assert ops.ROUTES["csr_project"] == "hip"
        loss_b, grads_b = _loss_and_gradients(model, by_hand)
        assert np.isfinite(loss_a) and loss_a.view(np.uint32) == loss_b.view(np.uint32), i
        for name in grads_a:
            assert grads_a[name] is not None and np.abs(grads_a[name]).max() > 0, name
            assert np.array_equal(grads_a[name].view(np.uint32), grads_b[name].view(np.uint32)), (i, name)


def test_both_pipeline_settings_train_alike_and_the_checkpoint_trains_on(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    runs = {}
    for native in (True, False):
        task = _task()
        (tmp_path / str(native)).mkdir()
        model = _model("RGCN_Model", task, gpu_device, tmp_path / str(native), native_batching=native)
        loss, results, steps, *_ = model._run_epoch("train", task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, quiet=True)
        runs[native] = [float(m["loss"]) for m in results]
        assert len(results) == 4 and np.isfinite(runs[native]).all()
    assert runs[True] == runs[False]
    # the native iterator asked directly reaches the sampled generator too (make_graph_store keeps the fold in sparse mode)
    train = task._loaded_data[DataFold.TRAIN]
    native_batches = list(task.make_native_minibatch_iterator(model._native_pipeline(train), DataFold.TRAIN, 10 ** 6))
    assert len(native_batches) == 4 and all(isinstance(b, DeviceBatch) and "sparse_node_features" in b.extra for b in native_batches)
    # validation stays the full graph, sparse; train() runs, saves, restores, and trains on
    model.train(quiet=True, max_epochs=1)
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.sampled_batches == BOTH and restored.task.sparse_node_features is True
    assert restored.task.get_metadata() == task.get_metadata()
    restored.task.load_synthetic(num_nodes=300, num_features=40, num_classes=3, feature_density=0.08, seed=5, num_train=60, num_valid=60, num_test=60)
    before = {n: restored.variables[n].detach().clone() for n in restored.variables.names()}
    loss, results, *_ = restored._run_epoch("train", restored.task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, quiet=True)
    assert len(results) == 4 and np.isfinite(loss) and all("num_masked" in m for m in results)
    assert all(not torch.equal(before[n], restored.variables[n]) for n in before)
    (prediction,) = restored.predict(restored.task.synthetic_test_data)
    assert prediction["classes"].shape == (300,)
    with pytest.raises(RuntimeError, match="sampled batch"):
        restored.capture_train_step(native_batches[0])


def test_the_full_graph_is_a_sample_of_itself_in_sparse_mode(gpu_device):
    """All nodes as seeds, fanouts [0], against the non-sampled sparse step, at the bars tests/test_gpu_neighbour_sampling.py's dense
    counterpart measures: the loss and the last layer's and the head's gradients bit for bit; the first layer's and the projection's
    within 1.2e-7 of the gradient's largest entry (the sampled lists are in bucket order, so the input gradient of the first layer
    adds the same messages in another order)."""
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    task = _task(sampled=None)
    fold = task._loaded_data[DataFold.TRAIN][0]
    n = len(fold.labels)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in fold.adjacency_lists], n)
    sub = NeighbourSampler(g, [0]).sample(torch.arange(n, dtype=torch.int32, device=gpu_device), 0)
    assert np.array_equal(sub.nodes.cpu().numpy(), np.arange(n))
    model = _model("RGCN_Model", task, gpu_device)
    (mb,) = task.make_minibatch_iterator([fold], DataFold.TRAIN, 10 ** 6)
    want_loss, want = _loss_and_gradients(model, DeviceBatch(mb, gpu_device))
    rows = fold.node_features.to(gpu_device)
    as_sample = sub.device_batch(rows, torch.as_tensor(fold.labels, device=gpu_device), torch.as_tensor(fold.mask, device=gpu_device), 1.0)
    taken = as_sample.extra["sparse_node_features"]
    for side in ("rows", "transposed"):
        for field in S.FIELDS:
            assert torch.equal(getattr(getattr(taken, side), field), getattr(getattr(rows, side), field)), (side, field)
    got_loss, got = _loss_and_gradients(model, as_sample)
    print("loss: full graph %.9g, as a sample %.9g" % (want_loss, got_loss))
    assert got_loss.view(np.uint32) == want_loss.view(np.uint32)
    assert sorted(want) == ["OutputDenseLayer/kernel", "graph_model/dense/kernel"] + sorted(k for k in want if "gnn_layer_" in k)
    for name in want:
        a, b = want[name].astype(np.float64), got[name].astype(np.float64)
        scale = float(np.abs(a).max())
        err = float(np.abs(a - b).max())
        same = np.array_equal(want[name].view(np.uint32), got[name].view(np.uint32))
        print("%s: err / scale %.3g  identical bits: %s" % (name, err / scale, same))
        if name == "OutputDenseLayer/kernel" or "gnn_layer_1" in name:
            assert same, name
        else:
            assert "gnn_layer_0" in name or name == "graph_model/dense/kernel"
            assert err <= 1.2e-7 * scale, (name, err, scale)


def test_a_sampled_step_stays_below_one_dense_table_of_its_batch(gpu_device, tmp_path):
    """V = 4096, F = 262144, 256 seeds: everything from the sampling state to the end of one Adam step, on top of the model's own
    variables and optimizer slots, peaks below the n x F float32 table of the batch's own rows (the projection's dense [F, 64]
    gradient, 64 MiB, is inside the peak)."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks import DataFold
    V, F = 4096, 262144
    task = _task(num_nodes=V, num_features=F, density=16.0 / F, sampled=dict(BOTH, seeds_per_batch=256), num_train=500, num_valid=500, num_test=500)
    model = _model("RGCN_Model", task, gpu_device, tmp_path, hidden_size=64)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    batch = next(iter(model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)))
    metrics = model.train_step(batch)
    torch.cuda.synchronize()
    assert ops.ROUTES["csr_project"] == "hip" and np.isfinite(float(metrics["loss"].detach())) and float(batch.extra["mask"].sum()) == 256.0
    peak = torch.cuda.max_memory_allocated(gpu_device) - before
    table = batch.num_nodes * F * 4
    print("peak %.1f MiB for one sampled step of %d nodes (their dense rows: %.0f MiB)" % (peak / 2 ** 20, batch.num_nodes, table / 2 ** 20))
    assert batch.num_nodes > 256 and peak < table
