"""The citation task's `sparse_node_features` mode without a GPU: the container (tasks/sparse_features.py), the loaders, the torch
composition of ops.csr_rows_project under the model driver's input projection, metadata and checkpoints.

The package has no CPU message passing (the layers are HIP kernels; tests/test_citation_task_cpu.py runs the GNN body through the NumPy
oracle), so "the RGCN model on the CPU" is here what the mode changes of it: the driver's input projection
(Sparse_Graph_Model._project_input, tanh) feeding the task's output head, loss and gradients — with no layer in between, the gradient
of graph_model/dense/kernel is exactly the quantity tests/sparse_features_reference.py bounds."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for p in (str(HERE / "golden"), str(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import sparse_features_reference as R  # noqa: E402
from citation_fixture import KINDS, expected_sizes  # noqa: E402
from test_citation_task_cpu import MANIFEST, Z, build_task  # noqa: E402


def _csr_of(rows):
    s = rows.rows
    return R.Csr(s.rowptr.numpy().astype(np.int64), s.col.numpy().astype(np.int64), s.val.numpy(), rows.shape)


@pytest.mark.parametrize("kind", list(KINDS))
def test_sparse_loader_holds_the_dense_loader_s_table_bit_for_bit(tmp_path, kind):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    _, dense = build_task(kind, tmp_path)
    task, sparse = build_task(kind, tmp_path, sparse_node_features=True)
    V, F, _, _ = expected_sizes(kind)
    rows = sparse["train"][0].node_features
    assert isinstance(rows, SparseRows) and rows.shape == (V, F) and len(rows) == V and task.initial_node_feature_size == F
    assert rows is sparse["valid"][0].node_features                       # the folds of one load share ONE container
    for name in ("train", "valid", "test"):
        got = sparse[name][0].node_features.to_dense().numpy()
        want = dense[name][0].node_features
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), Z[kind + "/features"].view(np.uint32))
        for field in ("labels", "mask", "type_to_node_to_num_incoming_edges"):
            assert np.array_equal(getattr(sparse[name][0], field), getattr(dense[name][0], field))
    assert rows.nnz == int((Z[kind + "/features"] != 0).sum())
    empty = np.flatnonzero(np.diff(rows.rows.rowptr.numpy()) == 0)
    assert len(empty) and not Z[kind + "/features"][empty].any()          # documents without words: rows without entries
    if kind == "citeseer":
        holes = sorted(set(range(560, V)) - set(MANIFEST["kinds"][kind]["directory"]["test_ids"]))
        assert len(holes) == 7 and set(holes) <= set(empty.tolist())


def test_the_transpose_is_the_transpose_with_ascending_ids(tmp_path):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    _, folds = build_task("citeseer", tmp_path, sparse_node_features=True)
    rows = folds["train"][0].node_features
    dense = rows.to_dense().numpy()
    t = rows.transposed
    assert t.num_rows == rows.shape[1] and t.num_cols == rows.shape[0] and t.nnz == rows.nnz
    back = np.zeros((rows.shape[1], rows.shape[0]), np.float32)
    back[t.row_ids().numpy(), t.col.numpy()] = t.val.numpy()
    assert np.array_equal(back.view(np.uint32), dense.T.view(np.uint32))
    for s in (rows.rows, t):
        ptr, col = s.rowptr.numpy(), s.col.numpy()
        assert ptr.dtype == np.int32 and col.dtype == np.int32 and s.val.dtype == torch.float32
        assert all((np.diff(col[ptr[r]:ptr[r + 1]]) > 0).all() for r in range(s.num_rows))
    want = R.transpose(_csr_of(rows))
    assert np.array_equal(t.rowptr.numpy(), want.rowptr) and np.array_equal(t.col.numpy(), want.col) and np.array_equal(t.val.numpy(), want.val)
    # from_scipy: any scipy matrix, duplicates summed, zeros dropped, columns sorted
    import scipy.sparse as sp
    m = sp.coo_matrix((np.array([1.0, 2.0, 0.0, 3.0, -3.0, 5.0]), (np.array([0, 0, 1, 2, 2, 2]), np.array([3, 1, 1, 0, 0, 2]))), shape=(4, 5))
    got = SparseRows.from_scipy(m)
    assert got.shape == (4, 5) and got.nnz == 3
    assert got.to_dense().numpy().tolist() == [[0, 2, 0, 1, 0], [0] * 5, [0, 0, 5, 0, 0], [0] * 5]
    assert got.to("cpu") is got


@pytest.mark.parametrize("case", ["rowptr_start", "rowptr_end", "rowptr_steps_down", "rowptr_length", "col_negative", "col_too_large",
                                  "col_unsorted", "col_duplicate", "explicit_zero", "lengths_differ", "float_ids"])
def test_a_malformed_structure_raises_value_error(case):
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    rowptr, col, val = np.array([0, 2, 2, 5]), np.array([1, 3, 0, 2, 4]), np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    SparseRows(rowptr, col, val, (3, 5))                                  # the well-formed one
    if case == "rowptr_start":
        rowptr = np.array([1, 2, 2, 5])
    elif case == "rowptr_end":
        rowptr = np.array([0, 2, 2, 4])
    elif case == "rowptr_steps_down":
        rowptr = np.array([0, 3, 2, 5])
    elif case == "rowptr_length":
        rowptr = np.array([0, 2, 5])
    elif case == "col_negative":
        col = np.array([-1, 3, 0, 2, 4])
    elif case == "col_too_large":
        col = np.array([1, 5, 0, 2, 4])
    elif case == "col_unsorted":
        col = np.array([3, 1, 0, 2, 4])
    elif case == "col_duplicate":
        col = np.array([1, 3, 2, 2, 4])
    elif case == "explicit_zero":
        val = np.array([1.0, 2.0, 0.0, 4.0, 5.0], np.float32)
    elif case == "lengths_differ":
        val = val[:4]
    elif case == "float_ids":
        col = col.astype(np.float32)
    with pytest.raises(ValueError):
        SparseRows(rowptr, col, val, (3, 5))


def test_default_params_are_unchanged_and_the_mode_travels_in_the_metadata():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    assert Citation_Network_Task.default_params() == MANIFEST["task"]["default_params"]
    assert "sparse_node_features" not in Citation_Network_Task.default_params()
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    assert task.sparse_node_features is False
    on = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True))
    on.load_synthetic(num_nodes=700, num_features=16, num_classes=3, num_train=20, num_valid=500, num_test=100)
    meta = on.get_metadata()
    assert meta["params"]["sparse_node_features"] is True
    task.restore_from_metadata(meta)
    assert task.sparse_node_features is True and task.get_metadata() == meta


def test_dense_mode_synthetic_data_is_what_it_was():
    """With the mode off load_synthetic draws what it always drew: the arrays of the code as it stood, restated here."""
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    task.load_synthetic(num_nodes=300, num_features=20, num_classes=3, num_train=20, num_valid=100, num_test=100, feature_density=0.2, seed=4)
    rng = np.random.default_rng(4)
    lengths = rng.poisson(2.0, size=300)
    for node in range(300):
        rng.integers(0, 300, size=int(lengths[node]))
    bag = (rng.random((300, 20)) < 0.2).astype(np.float32)
    row_sum = bag.sum(1, keepdims=True)
    want = np.divide(bag, row_sum, out=np.zeros_like(bag), where=row_sum > 0)
    labels = rng.integers(0, 3, size=300)
    fold = task._loaded_data[DataFold.TRAIN][0]
    assert isinstance(fold.node_features, np.ndarray) and np.array_equal(fold.node_features, want)
    assert np.array_equal(fold.labels[:20], labels[:20])


def test_sparse_synthetic_data_never_builds_the_dense_table():
    """V = 2000, F = 2^20: the dense table would be 8 GB."""
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), sparse_node_features=True))
    start = time.perf_counter()
    task.load_synthetic(num_nodes=2000, num_features=2 ** 20, feature_density=16.0 / 2 ** 20, seed=1)
    elapsed = time.perf_counter() - start
    rows = task._loaded_data[DataFold.TRAIN][0].node_features
    print("load_synthetic, 2000 x 2^20 sparse: %.3f s, %d entries" % (elapsed, rows.nnz))
    assert elapsed < 1.0
    assert isinstance(rows, SparseRows) and rows.shape == (2000, 2 ** 20) and 12 * 2000 < rows.nnz < 20 * 2000
    assert rows is task._loaded_data[DataFold.VALIDATION][0].node_features is task.synthetic_test_data[0].node_features
    per_row = np.diff(rows.rows.rowptr.numpy())
    sums = np.zeros(2000)
    np.add.at(sums, rows.rows.row_ids().numpy(), rows.rows.val.numpy().astype(np.float64))
    assert np.allclose(sums[per_row > 0], 1.0, atol=1e-6)                 # row-normalised


def _projection_and_head(task, folds, hidden=64, seed=3):
    """One forward / backward of the driver's input projection and the task's head on the train fold, on the CPU."""
    from tf_gnn_samples_amd import models, ops
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    p = models.RGCN_Model.default_params()
    p.update(hidden_size=hidden, graph_num_layers=2, random_seed=seed)
    model = models.RGCN_Model(p, task, device="cpu")
    (mb,) = task.make_minibatch_iterator(folds["train"], DataFold.TRAIN, 50000)
    batch = DeviceBatch(mb, "cpu")
    features = task.compute_initial_node_features(batch, model.variables.scope(""))
    act_id = ops.activation_id(p['graph_model_activation_function'])
    h = model._project_input(features, model.variables.scope("graph_model"), act_id, False)
    if h.requires_grad:                      # (without a projection h is the feature table itself)
        h.retain_grad()
    metrics = task.compute_task_metrics(h, batch, model.variables.scope(model._task_scope))
    metrics["loss"].backward()
    return model, batch, features, h, metrics


def test_cpu_projection_and_head_agree_between_the_two_modes(tmp_path):
    from tf_gnn_samples_amd import models, ops
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    name = models.RGCN_Model.default_params()['graph_model_activation_function'].lower()
    assert name == "tanh"
    runs = {}
    for mode in (False, True):
        task, folds = build_task("cora", tmp_path, sparse_node_features=mode)
        ops.ROUTES["csr_project"] = None
        runs[mode] = _projection_and_head(task, folds)
        assert ops.ROUTES["csr_project"] == ("composition" if mode else None)
    model_s, batch_s, features, h_s, metrics_s = runs[True]
    model_d, batch_d, dense_features, h_d, metrics_d = runs[False]
    assert isinstance(features, SparseRows) and tuple(batch_s.initial_node_features.shape) == (660, 1)
    assert torch.is_tensor(dense_features) and tuple(dense_features.shape) == (660, 48)
    for n in model_s.variables.names():
        assert torch.equal(model_s.variables[n], model_d.variables[n]), n                 # the same seed, the same variables
    csr = _csr_of(features)
    W = model_s.variables["graph_model/dense/kernel"].detach().numpy()
    want, tol, _ = R.forward_act64(csr, W, name)
    for h in (h_s, h_d):                     # either mode's projection within the forward tolerance of float64
        assert (np.abs(h.detach().numpy().astype(np.float64) - want) <= tol).all()
    # the loss: the projection's tolerance propagated to first order through the head, |dLoss/dh| * |h_sparse - h_dense| summed
    # (half as much again for the second order), plus four float32 steps of the loss for the head's own arithmetic
    gap = np.abs(h_s.detach().numpy().astype(np.float64) - h_d.detach().numpy())
    assert (gap <= 2.0 * tol).all()
    loss_s, loss_d = float(metrics_s["loss"].detach()), float(metrics_d["loss"].detach())
    loss_bound = 1.5 * float((np.abs(h_s.grad.numpy().astype(np.float64)) * 2.0 * tol).sum()) + 4.0 * float(np.spacing(np.float32(loss_s)))
    print("loss sparse %.9g dense %.9g, |difference| %.3g, bound %.3g" % (loss_s, loss_d, abs(loss_s - loss_d), loss_bound))
    assert abs(loss_s - loss_d) <= loss_bound
    assert float(metrics_s["accuracy"]) == float(metrics_d["accuracy"])
    # d loss / d graph_model/dense/kernel: each mode against the float64 sum over the transposed structure of ITS OWN dOut and y,
    # under the reference module's gradient tolerance (it holds for any summation order: torch's X^T product included)
    t = R.transpose(csr)
    for mode, (model, _, _, h, _) in runs.items():
        res, gtol = R.gradient64(t, h.grad.numpy(), h.detach().numpy(), name)
        got = model.variables["graph_model/dense/kernel"].grad.numpy().astype(np.float64)
        worst = float((np.abs(got - res.value) / np.maximum(gtol, 1e-300))[gtol > 0].max())
        print("dense/kernel gradient, sparse mode %s: worst error / tolerance %.3f" % (mode, worst))
        assert (np.abs(got - res.value) <= gtol).all()
        assert float(np.abs(res.value).max()) > 1e-4


def test_checkpoints_are_interchangeable_and_equal_sizes_need_no_projection(tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    (tmp_path / "data").mkdir()
    for written_sparse in (True, False):
        task, folds = build_task("cora", tmp_path / "data", sparse_node_features=written_sparse)
        model, _, _, _, metrics = _projection_and_head(task, folds)
        path = str(tmp_path / ("written_%s.pickle" % written_sparse))
        model.save_model(path)
        restored = models.restore(path, str(tmp_path), device="cpu")
        assert restored.task.sparse_node_features is written_sparse and restored.task.get_metadata() == task.get_metadata()
        assert restored.variables.names() == model.variables.names()
        for n in model.variables.names():
            assert torch.equal(model.variables[n], restored.variables[n]), n
        restored.task.params = dict(restored.task.params, sparse_node_features=not written_sparse)      # ... and run in the other mode
        data = restored.task.load_eval_data_from_path(str(tmp_path / "data"))
        (mb,) = restored.task.make_minibatch_iterator(data, DataFold.TEST, 50000)
        batch = DeviceBatch(mb, "cpu")
        with torch.no_grad():
            h = restored._project_input(restored.task.compute_initial_node_features(batch, restored.variables.scope("")),
                                        restored.variables.scope("graph_model"), 1, False)
            got = restored.task.compute_task_metrics(h, batch, restored.variables.scope(restored._task_scope))
        assert np.isfinite(float(got["loss"])) and h.shape == (660, 64)
    # F == hidden_size: no dense/kernel; the container is densified
    out = {}
    for mode in (False, True):
        task, folds = build_task("cora", tmp_path / "data", sparse_node_features=mode)
        model, _, _, h, _ = _projection_and_head(task, folds, hidden=48)
        assert "graph_model/dense/kernel" not in model.variables.names()
        out[mode] = h.detach().numpy()
    assert np.array_equal(out[True].view(np.uint32), out[False].view(np.uint32))
    assert np.array_equal(out[True].view(np.uint32), Z["cora/features"].view(np.uint32))


def test_host_packer_carries_the_stand_in_and_the_container(tmp_path):
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.batcher import NativeBatcher
    task, folds = build_task("citeseer", tmp_path, sparse_node_features=True)
    rows = folds["valid"][0].node_features
    store = task.make_graph_store(folds["valid"])
    assert store.sparse_rows is rows and [a.shape for a in store.payload][0] == (667, 1)
    assert sum(a.nbytes for a in store.payload) == 667 * 12               # stand-in, labels, mask: the table is in no payload
    batcher = NativeBatcher(store, "cpu")
    (batch,) = task.make_native_minibatch_iterator(batcher, DataFold.VALIDATION, 100)
    (mb,) = task.make_minibatch_iterator(folds["valid"], DataFold.VALIDATION, 100)
    assert tuple(batch.initial_node_features.shape) == (667, 1) == mb.feed_dict["initial_node_features"].shape
    assert batch.extra["sparse_node_features"] is rows is mb.feed_dict["sparse_node_features"]
    assert task.compute_initial_node_features(batch, {}) is rows          # already on the batch's device
    assert (batch.num_nodes, batch.num_edges) == (mb.num_nodes, mb.num_edges) == (667, sum(len(a) for a in folds["valid"][0].adjacency_lists))
    np.testing.assert_array_equal(batch.extra["labels"].numpy(), folds["valid"][0].labels)


def test_header_binding_and_library_agree():
    """What the library says of include/relgnn_sparse_features.h's limits (tests/test_abi.py holds the header against the binding)."""
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = _lib.load_library()
    assert lib.relgnn_csr_project_split_above() == 128 and lib.relgnn_csr_project_slab() == 512
    assert [lib.relgnn_csr_project_supported(n) for n in (0, 4, 6, 256, 1024, 1028)] == [0, 1, 0, 1, 1, 0]


def test_the_features_are_data():
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks.sparse_features import SparseRows
    rows = SparseRows(np.array([0, 1, 2]), np.array([0, 1]), np.array([1.0, 2.0], np.float32), (2, 2))
    W = torch.eye(2, requires_grad=True)
    out = ops.csr_rows_project(rows, W, 0)
    assert out.tolist() == [[1.0, 0.0], [0.0, 2.0]]
    W_inf = torch.tensor([[1.0, float("inf")], [3.0, 4.0]])
    one = SparseRows(np.array([0, 1]), np.array([1]), np.array([2.0], np.float32), (1, 2))
    assert ops.csr_rows_project(one, W_inf, 0).tolist() == [[6.0, 8.0]]  # the infinite row is not stored: it contributes nothing
    assert torch.isnan(one.to_dense() @ W_inf).any()                      # ... where the dense product gives 0 * inf
    rows.rows.val.requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        ops.csr_rows_project(rows, W, 0)
    with pytest.raises(ValueError):
        ops.csr_rows_project(one, torch.zeros(3, 2), 0)
