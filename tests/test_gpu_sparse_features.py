"""Sparse node features on the GPU: the CSR projection kernels (csrc/csr_project.hip) against float64 under the bounds derived in
tests/sparse_features_reference.py, determinism, routes, the citation models in `sparse_node_features` mode against the reference
run, the three input pipelines, predictions, checkpoints across the two modes, the captured step and the memory the mode is for.

Shapes.  The issue names row lengths up to 700 next to F = 97 table rows; a row of 700 distinct columns needs at least 700, so the
table has 797 rows (odd, like 97) and 197 rows of the lengths 0 .. 17, 63 .. 65 and, around this kernel's own thresholds, 128 / 129 /
130 (a row is split above 128 entries), 512 / 513 (a slab holds 512) and 700 (two slabs).  A second structure keeps F = 97 with the
lengths that fit."""
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for p in (str(HERE / "golden"), str(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import sparse_features_reference as R  # noqa: E402
from test_citation_task_cpu import GOLDEN, MODELS, build_model, build_task, check_metrics  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 64, 252, 256, 260, 320]
PIPELINES = {"numpy": dict(native_batching=False), "packer": dict(resident_dataset=False), "resident": dict(resident_dataset=True)}


def _act_id(name):
    from tf_gnn_samples_amd import ops
    return ops.activation_id(None if name == "linear" else name)


def _rows(csr, device):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    return SparseRows(csr.rowptr, csr.col, csr.val, csr.shape).to(device)


def _dev(a, device):
    return torch.as_tensor(np.array(a), device=device)                  # (a copy: the reference's arrays are read-only)


def _check(got, want, tol, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(tol, 1e-300))[tol > 0].max()) if (tol > 0).any() else 0.0
    print("%s: worst error / tolerance %.3f" % (what, ratio))
    assert (err <= tol).all(), (what, ratio)


def test_plan_constants_are_the_library_s():
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks import sparse_features as SF
    lib = _lib.load_library()
    assert lib.relgnn_csr_project_split_above() == SF.SPLIT_ABOVE == 128 and lib.relgnn_csr_project_slab() == SF.SLAB == 512
    assert [n for n in range(0, 1040) if lib.relgnn_csr_project_supported(n)] == list(range(4, 1025, 4))
    slabs, combos, ws_rows = SF.split_plan(R.structure().rowptr)
    lengths = np.diff(R.structure().rowptr)
    assert len(slabs) == int(((lengths[lengths > 128] + 511) // 512).sum()) and len(combos) == int((lengths > 512).sum()) == 4
    assert ws_rows == 8 and sorted(slabs[slabs[:, 3] >= 0, 3]) == list(range(8))


@pytest.mark.parametrize("n", WIDTHS)
def test_kernel_against_float64(gpu_device, n):
    """Forward with every activation of the table and the gradient form with every activation whose derivative the output
    determines, over the 197-row structure; then the autograd op: its backward over the container's own transpose."""
    from tf_gnn_samples_amd import ops
    csr = R.structure()
    rows = _rows(csr, gpu_device)
    table, dout = (a[:, :n] for a in R.tables())
    td, gd = _dev(table, gpu_device), _dev(dout, gpu_device)
    for name in R.ACTIVATIONS:
        want, tol, _ = R.forward_act64(csr, table, name)
        got = ops._csr_project_raw(rows.rows, td, _act_id(name)).cpu().numpy()
        _check(got, want, tol, "forward n %d %s" % (n, name))
        assert not got[np.diff(csr.rowptr) == 0].any()                     # an empty row is act(0) = 0, exactly
    for name in R.GRADIENT_ACTIVATIONS:
        y = R.outputs(name)[:, :n]
        res, tol = R.gradient64(csr, dout, y, name)
        got = ops._csr_project_raw(rows.rows, gd, _act_id(name), _dev(y, gpu_device)).cpu().numpy()
        _check(got, res.value, tol, "gradient n %d %s" % (n, name))
    # the op: out = act(X W), dW over the transpose with the forward's own output as y
    t = R.transpose(csr)
    gout = R.tables()[1][:csr.shape[0], :n]
    for name in R.ACTIVATIONS:
        W = td.clone().requires_grad_(True)
        out = ops.csr_rows_project(rows, W, _act_id(name))
        assert ops.ROUTES["csr_project"] == "hip"
        want, tol, pre = R.forward_act64(csr, table, name)
        if name == "gelu":                   # (the linear kernel, then torch's erf form: its own evaluation error)
            tol = tol + 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        _check(out.detach().cpu().numpy(), want, tol, "op forward n %d %s" % (n, name))
        out.backward(_dev(gout, gpu_device))
        if name == "gelu":
            # torch scales dOut by gelu' at the float32 pre-activation the linear kernel wrote (the same bits on every run).  Its
            # 1 + erf cancels for negative arguments, so gelu' carries an ABSOLUTE error: the allowance of an evaluated activation,
            # ACT_ALLOWANCE * max(1, |gelu'|), per term, as seg_reduce_reference.msgact_bwd64 grants a per-message derivative
            pre32 = ops._csr_project_raw(rows.rows, td, 0).cpu().numpy()
            d = R.act64("gelu", pre32)[1]
            res, tol = R.gradient64(t, gout.astype(np.float64) * d, None, "linear")
            weight = np.abs(t.val.astype(np.float64)[:, None] * gout.astype(np.float64)[t.col]) * np.maximum(1.0, np.abs(d[t.col]))
            tol = tol + R.ACT_ALLOWANCE * R._sum_rows(t, weight).sum_abs
        else:
            res, tol = R.gradient64(t, gout, out.detach().cpu().numpy(), name)
        _check(W.grad.cpu().numpy(), res.value, tol, "op backward n %d %s" % (n, name))


def test_kernel_with_97_table_rows_empty_and_one_row_matrices(gpu_device):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    rng = np.random.default_rng(3)
    lengths = np.array([l for l in (0, 1, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 97) for _ in range(14)])
    rng.shuffle(lengths)
    col = np.concatenate([np.sort(rng.choice(97, size=l, replace=False)) for l in lengths]).astype(np.int64)
    csr = R.Csr(np.concatenate([[0], np.cumsum(lengths)]), col, R._signed(rng, len(col)), (len(lengths), 97))
    table = R._signed(rng, (97, 68))
    rows = _rows(csr, gpu_device)
    pre = R.forward64(csr, table)
    _check(ops._csr_project_raw(rows.rows, _dev(table, gpu_device), 0).cpu().numpy(), pre.value, R.bound(pre.k, pre.sum_abs), "F = 97")
    t = R.transpose(csr)
    gout = R._signed(rng, (len(lengths), 68))
    res, tol = R.gradient64(t, gout, None, "linear")
    _check(ops._csr_project_raw(rows.transposed, _dev(gout, gpu_device), 0).cpu().numpy(), res.value, tol, "F = 97, transposed")
    # no rows; rows without entries; one row
    W = _dev(table, gpu_device)
    for shape in ((0, 97), (5, 97)):
        empty = SparseRows(np.zeros(shape[0] + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), shape).to(gpu_device)
        for act in (0, 1, 2):
            Wg = W.clone().requires_grad_(True)
            out = ops.csr_rows_project(empty, Wg, act)
            assert out.shape == (shape[0], 68) and not out.any()
            out.sum().backward()
            assert Wg.grad.shape == W.shape and not Wg.grad.any()
    one = R.Csr(np.array([0, 5]), np.array([2, 11, 40, 41, 96]), R._signed(rng, 5), (1, 97))
    pre = R.forward64(one, table)
    Wg = W.clone().requires_grad_(True)
    out = ops.csr_rows_project(_rows(one, gpu_device), Wg, 0)
    _check(out.detach().cpu().numpy(), pre.value, R.bound(pre.k, pre.sum_abs), "one row")
    out.backward(torch.ones_like(out))
    want = R.dense64(one).T @ np.ones((1, 68))
    assert np.array_equal(Wg.grad.cpu().numpy(), want.astype(np.float32))                 # one term per element: exact


@pytest.mark.parametrize("n", [64, 320])
def test_same_bits_on_every_run_on_a_side_stream_and_with_strided_rows(gpu_device, n):
    from tf_gnn_samples_amd import ops
    csr = R.structure()
    rows = _rows(csr, gpu_device)
    table, dout = (_dev(a[:, :n], gpu_device) for a in R.tables())
    y = _dev(R.outputs("tanh")[:, :n], gpu_device)

    def run(t, g, yy):
        return ops._csr_project_raw(rows.rows, t, 1), ops._csr_project_raw(rows.rows, g, 1, yy)

    base = run(table, dout, y)
    again = run(table, dout, y)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        on_side = run(table, dout, y)
    torch.cuda.current_stream(gpu_device).wait_stream(side)

    def wide(t):                                   # rows of the same values with ld = n + 12, NaN behind every row
        buf = torch.full((t.shape[0], n + 12), float("nan"), device=gpu_device)
        buf[:, :n] = t
        return buf[:, :n]
    strided = run(wide(table), wide(dout), wide(y))
    assert not wide(table).is_contiguous()
    for other in (again, on_side, strided):
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1])
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()


def test_routes(gpu_device):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.dense import dense_act
    from tf_gnn_samples_amd.ops import segment
    csr = R.structure()
    rows = _rows(csr, gpu_device)
    table = R.tables()[0]
    ops.csr_rows_project(rows, _dev(table[:, :8], gpu_device), 1)
    assert ops.ROUTES["csr_project"] == "hip"
    segment._WARNED.discard(6)
    W = _dev(table[:, :6], gpu_device).requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = ops.csr_rows_project(rows, W, 1)
        ops.csr_rows_project(rows, W, 1)
    assert ops.ROUTES["csr_project"] == "dense" and len([w for w in caught if "densified" in str(w.message)]) == 1
    W2 = W.detach().clone().requires_grad_(True)
    want = dense_act(rows.to_dense(), W2, None, 1)
    assert torch.equal(out, want)
    g = _dev(R.tables()[1][:csr.shape[0], :6], gpu_device)
    out.backward(g)
    want.backward(g)
    ops.join_deferred()
    assert torch.equal(W.grad, W2.grad)
    # CPU tensors: the composition
    cpu = ops.csr_rows_project(_rows(csr, "cpu"), torch.as_tensor(table[:, :8].copy()), 1)
    assert ops.ROUTES["csr_project"] == "composition" and cpu.shape == (csr.shape[0], 8)
    # the features are data
    rows.rows.val.requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        ops.csr_rows_project(rows, _dev(table[:, :8], gpu_device), 1)


def _device_batch(task, data, fold, device):
    from tf_gnn_samples_amd.tasks import DeviceBatch
    (mb,) = task.make_minibatch_iterator(data, fold, 50000)
    return DeviceBatch(mb, device)


@pytest.mark.parametrize("model_name", ["RGCN_Model", "GGNN_Model"])
@pytest.mark.parametrize("kind", ["cora", "citeseer"])
def test_sparse_mode_models_reproduce_the_reference_run(gpu_device, tmp_path, kind, model_name):
    """tests/test_gpu_citation.py::test_hip_models_reproduce_the_reference_run in sparse_node_features mode: the same fixtures, the
    same bars (metrics at check_metrics; every variable's gradient at 2e-5 of its largest entry and 2e-5 in the Frobenius norm)."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    assert model_name in MODELS
    task, folds = build_task(kind, tmp_path, sparse_node_features=True)
    assert isinstance(folds["train"][0].node_features, SparseRows)
    assert folds["train"][0].node_features is folds["valid"][0].node_features        # ONE container for the folds of a load
    model, entry = build_model(kind, model_name, task, str(gpu_device))
    ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    ops.ROUTES["csr_project"] = None
    for name in ("valid", "test"):
        with torch.no_grad():
            check_metrics(model.forward_batch(_device_batch(task, folds[name], ids[name], gpu_device), training=False), entry["metrics"][name])
    assert ops.ROUTES["csr_project"] == "hip"
    metrics = model.forward_batch(_device_batch(task, folds["train"], DataFold.TRAIN, gpu_device), training=False)
    check_metrics(metrics, entry["metrics"]["train"])
    metrics["loss"].backward()
    ops.join_deferred()
    torch.cuda.synchronize()
    grads = np.load(GOLDEN / ("reference_run_citation_grad_%s.npz" % kind))
    for n in entry["variables"]:
        want = grads["%s/%s/grad/%s" % (kind, model_name, n)].astype(np.float64)
        g = model.variables[n].grad
        got = np.zeros_like(want) if g is None else g.cpu().numpy().astype(np.float64)
        scale = max(1e-6, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        fro = float(np.linalg.norm(got - want) / max(1e-12, np.linalg.norm(want)))
        print("%s %s %s: err / scale %.3g  fro %.3g" % (kind, model_name, n, err / scale, fro))
        assert err <= 2e-5 * scale and fro <= 2e-5, (n, err, scale, fro)
    # one device copy per device, shared by the folds of a load
    assert len(task._device_rows) == 2 and all(len(per_device) == 1 for per_device in task._device_rows.values())


def _model(task, device, result_dir, **params):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(dict(dict(hidden_size=64, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3), **params))
    return RGCN_Model(p, task, run_id="citation_sparse", result_dir=str(result_dir), device=str(device))


def test_pipelines_predictions_and_checkpoints_in_sparse_mode(gpu_device, tmp_path):
    """Three steps on each of the three input pipelines: the same losses and the same variables, bit for bit; predict() the same bits
    on all three; each fold's accuracy recomputed from the predictions is the reported metric; a sparse-mode checkpoint restored in
    dense mode predicts the same classes."""
    from tf_gnn_samples_amd import models, ops
    from tf_gnn_samples_amd.tasks import DataFold
    (tmp_path / "data").mkdir()
    task, folds = build_task("cora", tmp_path / "data", sparse_node_features=True)
    runs, predictions, variables = {}, {}, {}
    for name, params in PIPELINES.items():
        (tmp_path / name).mkdir()
        model = _model(task, gpu_device, tmp_path / name, **params)
        losses = []
        for _ in range(3):
            loss, results, *_ = model._run_epoch("train", folds["train"], DataFold.TRAIN, quiet=True)
            losses.append((loss, results[0]["total_loss"], results[0]["accuracy"]))
        assert ops.ROUTES["csr_project"] == "hip"
        runs[name] = losses
        variables[name] = {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}
        predictions[name] = {fold: model.predict(folds[fold]) for fold in folds}
        # the table is in no per-batch payload: the batch carries the [V, 1] stand-in
        batch = next(iter(model._batches(folds["valid"], DataFold.VALIDATION)))
        features = batch.initial_node_features if hasattr(batch, "initial_node_features") else batch.feed_dict["initial_node_features"]
        assert tuple(features.shape) == (660, 1)
    assert all(np.isfinite(l[0]) for l in runs["numpy"]) and runs["numpy"][0][0] > runs["numpy"][2][0]
    for name in ("packer", "resident"):
        assert runs[name] == runs["numpy"], name
        for n in variables["numpy"]:
            assert variables[name][n].tobytes() == variables["numpy"][n].tobytes(), (name, n)
        for fold in folds:
            for a, b in zip(predictions[name][fold], predictions["numpy"][fold]):
                assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), (name, fold)
    for fold in folds:                      # (`model` is the resident one; evaluated, not trained: DataFold.TEST for each)
        _, metrics, *_ = model._run_epoch("Test", list(folds[fold]), DataFold.TEST, quiet=True)
        sample, classes = folds[fold][0], predictions["resident"][fold][0]["classes"]
        assert classes.shape == (660,) and predictions["resident"][fold][0]["probabilities"].shape == (660, 5)
        correct = float(sample.mask[classes == sample.labels].sum())
        assert correct > 0 and np.float32(correct) / np.float32(sample.mask.sum()) == np.float32(metrics[0]["accuracy"])
    # ---- metadata keeps the mode; the checkpoint restores in either ----
    path = str(tmp_path / "sparse.pickle")
    model.save_model(path)
    sparse_again = models.restore(path, str(tmp_path), device=str(gpu_device))
    assert sparse_again.task.params["sparse_node_features"] is True and sparse_again.task.get_metadata() == task.get_metadata()
    test_sparse = sparse_again.task.load_eval_data_from_path(str(tmp_path / "data"))
    again = sparse_again.predict(test_sparse)
    assert again[0]["classes"].tobytes() == predictions["resident"]["test"][0]["classes"].tobytes()
    assert again[0]["probabilities"].tobytes() == predictions["resident"]["test"][0]["probabilities"].tobytes()
    dense_model = models.restore(path, str(tmp_path), device=str(gpu_device))
    dense_model.task.params = dict(dense_model.task.params, sparse_node_features=False)
    test_dense = dense_model.task.load_eval_data_from_path(str(tmp_path / "data"))
    assert isinstance(test_dense[0].node_features, np.ndarray)
    ops.ROUTES["csr_project"] = None
    dense_out = dense_model.predict(test_dense)[0]
    assert ops.ROUTES["csr_project"] is None
    # The two modes differ by the rounding of the projection (a few float32 steps of a 48-term sum), carried through two layers
    # and the head: 1e-5 on a probability bounds it generously.  A class may differ only where the two largest probabilities are
    # closer than that.
    top2 = np.sort(dense_out["probabilities"], axis=1)[:, -2:]
    differ = dense_out["classes"] != again[0]["classes"]
    print("sparse checkpoint in dense mode: %d of %d classes differ; max |p_sparse - p_dense| %.3g"
          % (int(differ.sum()), len(differ), float(np.abs(dense_out["probabilities"] - again[0]["probabilities"]).max())))
    assert np.abs(dense_out["probabilities"] - again[0]["probabilities"]).max() <= 1e-5
    assert ((top2[:, 1] - top2[:, 0])[differ] < 1e-5).all()
    assert float(differ.mean()) == 0.0


def test_a_dense_checkpoint_restores_in_sparse_mode_and_equal_sizes_need_no_projection(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models, ops
    (tmp_path / "data").mkdir()
    task, folds = build_task("cora", tmp_path / "data")
    model = _model(task, gpu_device, tmp_path)
    want = model.predict(folds["test"])[0]
    path = str(tmp_path / "dense.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device=str(gpu_device))
    restored.task.params = dict(restored.task.params, sparse_node_features=True)
    got = restored.predict(restored.task.load_eval_data_from_path(str(tmp_path / "data")))[0]
    assert ops.ROUTES["csr_project"] == "hip"
    assert np.abs(got["probabilities"] - want["probabilities"]).max() <= 1e-5 and (got["classes"] == want["classes"]).all()
    # F == hidden_size: the reference has no projection; the container is densified on the device
    outs = {}
    for mode in (False, True):
        t, f = build_task("cora", tmp_path / "data", sparse_node_features=mode)
        m = _model(t, gpu_device, tmp_path, hidden_size=48)
        assert "graph_model/dense/kernel" not in m.variables.names()
        outs[mode] = m.predict(f["test"])[0]
    assert outs[True]["probabilities"].tobytes() == outs[False]["probabilities"].tobytes()


def test_captured_step_replays_the_eager_step_bit_for_bit(gpu_device, tmp_path):
    from tf_gnn_samples_amd.tasks import DataFold
    task, folds = build_task("cora", tmp_path, sparse_node_features=True)

    def fresh():
        return _model(task, gpu_device, tmp_path), _device_batch(task, folds["train"], DataFold.TRAIN, gpu_device)
    eager, batch_e = fresh()
    eager.optimizer.sync_device_step_count()
    for _ in range(4):
        eager.train_step(batch_e, device_step_count=True)
        eager.optimizer.t += 1
    captured, batch_c = fresh()
    step = captured.capture_train_step(batch_c, warmup_steps=3)           # 3 real steps, then the recorded one
    step.replay()                                                         # step 4
    torch.cuda.synchronize()
    for n in eager.variables.names():
        assert torch.equal(eager.variables[n], captured.variables[n]), n


def test_a_training_step_never_holds_the_dense_table(gpu_device, tmp_path):
    """V = 4096, F = 262144, 16 words per node, hidden 64: the dense table alone would be 4 GiB.  One Adam step stays below a quarter
    of that; the weight, its gradient and the two Adam slots are 256 MiB of it."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    V, F = 4096, 262144
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True))
    task.load_synthetic(num_nodes=V, num_features=F, num_train=500, num_valid=500, num_test=500, feature_density=16.0 / F, seed=2)
    rows = task._loaded_data[DataFold.TRAIN][0].node_features
    assert rows.shape == (V, F) and 14 * V < rows.nnz <= 18 * V
    model = _model(task, gpu_device, tmp_path)
    assert model.params["optimizer"].lower() == "adam"
    metrics = model.train_step(_device_batch(task, task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, gpu_device))
    torch.cuda.synchronize()
    assert ops.ROUTES["csr_project"] == "hip" and np.isfinite(float(metrics["loss"]))
    peak = torch.cuda.max_memory_allocated(gpu_device) - before
    print("peak %.1f MiB of device memory for one step (the dense table: %.0f MiB)" % (peak / 2 ** 20, V * F * 4 / 2 ** 20))
    assert peak < V * F * 4 // 4
