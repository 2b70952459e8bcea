"""Predictions on the GPU: the three kernels of include/relgnn_predict.h against float64 and against the metric kernels whose label
rules they share (csrc/common.h), then Sparse_Graph_Model.predict for the four tasks: the three input pipelines, the metric
recomputed from the predictions, node states, checkpoints, and that predict leaves nothing behind that a training step can see."""
import gzip
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

pytestmark = pytest.mark.gpu

SPECIAL = [0.0, -0.0, 1e-8, 1.0, -1.0, float("inf"), float("-inf"), float("nan")]


def dev_tensor(a, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=device, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_sigmoid
# ---------------------------------------------------------------------------------------------------------------------------------
def sigmoid_logits(rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 4).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    special = SPECIAL + [-90.0, -100.0, 85.0, -80.0, 80.0, -87.5]
    for base in (0, n // 2, n - len(special)):                # the first, a middle and the last elements
        for k, v in enumerate(special):
            if 0 <= base + k < n:
                flat[base + k] = v
    return x


def stats_counts(logits, targets):
    """(true_pos, false_pos, false_neg) as _SigmoidCEStats counts them."""
    from tf_gnn_samples_amd.tasks.ppi_task import _SigmoidCEStats
    return [int(v) for v in _SigmoidCEStats.apply(logits.contiguous(), targets.contiguous(), 1.0)[3].tolist()]


def run_sigmoid(x, layout, device):
    """-> (probabilities, labels) as NumPy arrays, launched in one of the three layouts."""
    from tf_gnn_samples_amd.predict import predict_sigmoid
    rows, cols = x.shape
    if layout == "contiguous":
        logits = dev_tensor(x, device)
        probs, labels = predict_sigmoid(logits)
        assert probs.is_contiguous() and labels.is_contiguous()
    elif layout == "ld+3":
        ld = cols + 3
        wide = torch.full((rows, ld), float("nan"), device=device)
        wide[:, :cols] = dev_tensor(x, device)
        logits = wide[:, :cols]
        pbuf = torch.full((rows, ld), -7.0, device=device)
        lbuf = torch.full((rows, ld), 9, dtype=torch.uint8, device=device)
        probs, labels = predict_sigmoid(logits, pbuf[:, :cols], lbuf[:, :cols])
        assert bool((pbuf[:, cols:] == -7.0).all()) and bool((lbuf[:, cols:] == 9).all())        # nothing behind the columns is written
    else:                                                      # slices of one byte arena, the uint8 plane at an odd byte offset
        logits = dev_tensor(x, device)
        nbytes = rows * cols * 4
        arena = torch.full((16 + nbytes + 3 + rows * cols + 5,), 0xAB, dtype=torch.uint8, device=device)
        pview = arena[16:16 + nbytes].view(torch.float32).view(rows, cols)
        lview = arena[16 + nbytes + 3:16 + nbytes + 3 + rows * cols].view(rows, cols)
        assert lview.data_ptr() % 2 == 1
        probs, labels = predict_sigmoid(logits, pview, lview)
        assert probs.data_ptr() == pview.data_ptr() and labels.data_ptr() == lview.data_ptr()
        guard = torch.cat([arena[:16], arena[16 + nbytes:16 + nbytes + 3], arena[-5:]])
        assert bool((guard == 0xAB).all())
    return probs.cpu().numpy(), labels.cpu().numpy(), logits


@pytest.mark.parametrize("layout", ["contiguous", "ld+3", "arena"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 121), (3, 121), (64, 4), (257, 121), (1000, 128)])
def test_predict_sigmoid_against_float64_and_the_stats_kernel(gpu_device, shape, layout):
    rows, cols = shape
    x = sigmoid_logits(rows, cols, seed=rows * 1000 + cols)
    p, labels, logits = run_sigmoid(x, layout, gpu_device)
    assert p.dtype == np.float32 and labels.dtype == np.uint8 and p.shape == x.shape and labels.shape == x.shape
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        want = np.where(x64 >= 0, 1.0 / (1.0 + np.exp(-x64)), np.exp(x64) / (1.0 + np.exp(x64)))
    finite = np.isfinite(x)
    body = finite & (np.abs(x) <= 80)
    rel = np.abs(p[body].astype(np.float64) - want[body]) / want[body]
    worst = float(rel.max()) if rel.size else 0.0
    print("predict_sigmoid %s %s: worst relative error %.3e over %d elements" % (shape, layout, worst, rel.size))
    assert worst <= 1e-6
    tail = finite & (x < -87)
    assert np.all((p[tail] >= 0) & (p[tail] <= 2e-38))
    assert np.all(np.isfinite(p[finite])) and np.all((p[finite] >= 0) & (p[finite] <= 1))
    assert np.all(np.isnan(p[np.isnan(x)])) and np.all(labels[np.isnan(x)] == 0)
    assert np.all(p[x == np.inf] == 1.0) and np.all(labels[x == np.inf] == 1)
    assert np.all(p[x == -np.inf] == 0.0) and np.all(labels[x == -np.inf] == 0)
    assert set(np.unique(labels)) <= {0, 1}
    # the counts of the metric kernel, recounted on the host from the predicted labels
    rng = np.random.default_rng(5)
    targets = (rng.random((rows, cols)) < 0.4).astype(np.float32)
    pred, z = labels.astype(bool), targets.astype(bool)
    recount = [int((pred & z).sum()), int((pred & ~z).sum()), int((~pred & z).sum())]
    assert recount == stats_counts(logits, dev_tensor(targets, gpu_device))


@pytest.mark.parametrize("x", [1e-8, 5.9e-8, 6e-8, 1.2e-7, 2.4e-7, 1e-6])
def test_predict_sigmoid_label_near_the_threshold_is_the_stats_kernel_s(gpu_device, x):
    from tf_gnn_samples_amd.predict import predict_sigmoid
    logits = torch.tensor([[x]], dtype=torch.float32, device=gpu_device)
    _, labels = predict_sigmoid(logits)
    tp, fp, fn = stats_counts(logits, torch.ones((1, 1), device=gpu_device))
    print("x = %g: label %d, stats (tp, fp, fn) = %s" % (x, int(labels[0, 0]), (tp, fp, fn)))
    assert int(labels[0, 0]) == tp and fp == 0 and tp + fn == 1


def test_predict_sigmoid_of_no_rows_launches_nothing(gpu_device):
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.predict import predict_sigmoid
    probs, labels = predict_sigmoid(torch.empty((0, 121), device=gpu_device))
    assert tuple(probs.shape) == (0, 121) and tuple(labels.shape) == (0, 121)
    lib = _lib.load_library()
    assert lib.relgnn_predict_sigmoid_f32(None, 121, 0, 121, None, 121, None, 121, _lib.current_stream()) == _lib.OK
    assert lib.relgnn_predict_softmax_f32(None, 7, 0, 7, None, 7, None, _lib.current_stream()) == _lib.OK
    assert lib.relgnn_predict_candidates_f32(None, 0, 5, None, None, _lib.current_stream()) == _lib.OK
    assert lib.relgnn_predict_candidates_f32(None, 4, 9, None, None, _lib.current_stream()) == _lib.EINVAL      # more than 8 candidates
    assert lib.relgnn_predict_sigmoid_f32(None, 120, 4, 121, None, 121, None, 121, _lib.current_stream()) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_softmax
# ---------------------------------------------------------------------------------------------------------------------------------
def run_softmax(x, device, pad=0):
    from tf_gnn_samples_amd.predict import predict_softmax
    rows, cols = x.shape
    if pad:
        wide = torch.full((rows, cols + pad), float("nan"), device=device)
        wide[:, :cols] = dev_tensor(x, device)
        pbuf = torch.full((rows, cols + pad), -7.0, device=device)
        probs, classes = predict_softmax(wide[:, :cols], pbuf[:, :cols])
        assert bool((pbuf[:, cols:] == -7.0).all())
    else:
        probs, classes = predict_softmax(dev_tensor(x, device))
    return probs.cpu().numpy(), classes.cpu().numpy()


def softmax64(x):
    x64 = x.astype(np.float64)
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


SOFTMAX_COLS = [1, 2, 3, 7, 8, 9, 16, 17, 128, 129, 300]


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_predict_softmax_against_float64(gpu_device, cols):
    """(cols + 32) * 2^-24 relative, 2^-24 being half an ulp: a float32 sum of cols positive terms (at most cols half-ulps in any
    order), the rounded x - max of magnitude <= 20 (up to 20 * 2^-24 absolute in the exponent, which is relative in the value: the
    largest term), expf, and one division; the terms of the denominator carry the same errors, weighted by their share."""
    bound = (cols + 32) * 2.0 ** -24
    worst = 0.0
    for rows in (1, 63, 64, 65, 257):
        rng = np.random.default_rng(cols * 1000 + rows)
        x = rng.uniform(-10, 10, size=(rows, cols)).astype(np.float32)
        want = softmax64(x)
        for pad in (0, 5):
            p, classes = run_softmax(x, gpu_device, pad)
            assert p.dtype == np.float32 and classes.dtype == np.int32 and p.shape == x.shape and classes.shape == (rows,)
            rel = float((np.abs(p.astype(np.float64) - want) / want).max())
            worst = max(worst, rel)
            assert rel <= bound, (rows, pad, rel, bound)
            assert np.array_equal(classes, np.argmax(x, axis=1))
    print("predict_softmax cols = %d: worst relative error %.3e (bound %.3e)" % (cols, worst, bound))


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_predict_softmax_ties_infinities_and_the_stats_kernel_s_count(gpu_device, cols):
    from tf_gnn_samples_amd.tasks.citation_network_task import softmax_ce_stats
    rng = np.random.default_rng(cols)
    x = rng.uniform(-10, 10, size=(70, cols)).astype(np.float32)
    want_class = np.argmax(x, axis=1)
    x[3, :] = 2.5                                              # cols equal maxima
    want_class[3] = 0
    if cols >= 2:
        first = cols // 3
        x[5, first] = x[5, cols - 1] = 11.0                    # two equal maxima
        want_class[5] = first
        x[9, cols - 1] = -np.inf                               # a -inf column beside finite ones
        want_class[9] = int(np.argmax(x[9]))
    p, classes = run_softmax(x, gpu_device)
    assert np.array_equal(classes, want_class)
    assert np.allclose(p[3], 1.0 / cols, rtol=(cols + 32) * 2.0 ** -24)
    if cols >= 2:
        assert p[9, cols - 1] == 0.0 and np.all(p[9, :cols - 1] > 0)
        assert p[5, first] == p[5, cols - 1]
    # rows that are NaN throughout, and no other row's bits move
    bad = np.concatenate([x[:20], np.zeros((3, cols), np.float32), x[20:]])
    bad[20, cols // 2] = np.nan
    bad[21, cols - 1] = np.inf
    bad[22, :] = -np.inf
    pb, cb = run_softmax(bad, gpu_device)
    assert np.all(np.isnan(pb[20:23]))
    keep = np.r_[0:20, 23:73]
    assert np.array_equal(pb[keep].view(np.uint32), p.view(np.uint32)) and np.array_equal(cb[keep], classes)
    # the accuracy count of the metric kernel, recounted from the classes
    labels = rng.integers(0, cols, size=70).astype(np.int32)
    labels[::3] = want_class[::3]
    mask = (rng.random(70) < 0.6).astype(np.float32)
    counts = softmax_ce_stats(dev_tensor(x, gpu_device), dev_tensor(labels, gpu_device), dev_tensor(mask, gpu_device))[3].tolist()
    assert float(mask[classes == labels].sum()) == counts[2] and float(mask.sum()) == counts[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# predict_candidates
# ---------------------------------------------------------------------------------------------------------------------------------
def candidate_logits(rows, cols, seed):
    """Random logits in [-5, 5], masked columns (never column 0) at -1e7; one row in ten is a near-tie pair [a, nextafter(a)] with
    a over 1e-4 .. 10, at columns 0 / 1 in either order.  -> (logits, mask)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5, 5, size=(rows, cols)).astype(np.float32)
    mask = np.ones((rows, cols), np.float32)
    if cols >= 2:
        mask[:, 1:] = (rng.random((rows, cols - 1)) < 0.7).astype(np.float32)
        for r in range(0, rows, 10):
            a = np.float32(10.0 ** rng.uniform(-4, 1))
            pair = [a, np.nextafter(a, np.float32(np.inf))]
            if rng.random() < 0.5:
                pair.reverse()
            x[r, :2] = pair
            x[r, 2:] = np.minimum(x[r, 2:], np.float32(-1.0)) if rng.random() < 0.5 else x[r, 2:]
            mask[r, :2] = 1.0
    x[mask == 0] = -1e7
    return x, mask


def head_on_logits(x, mask, device):
    """relgnn_varmisuse_head_fwd on states built to give exactly these logits (slot row = e_0, candidate row c = x[c] e_0, 0 for a
    masked candidate: 0 + (1 - 0) * -1e7) -> (num_correct_predictions, the head's logits)."""
    from tf_gnn_samples_amd.tasks.varmisuse_task import varmisuse_head
    rows, cols = x.shape
    per_graph = cols + 1
    states = np.zeros((rows * per_graph, 64), np.float32)
    states[0::per_graph, 0] = 1.0
    for c in range(cols):
        states[1 + c::per_graph, 0] = np.where(mask[:, c] != 0, x[:, c], 0.0)
    slot = (np.arange(rows) * per_graph).astype(np.int32)
    cands = (slot[:, None] + 1 + np.arange(cols)[None, :]).astype(np.int32)
    with torch.no_grad():
        out = varmisuse_head(dev_tensor(states, device), dev_tensor(slot, device), dev_tensor(cands, device), dev_tensor(mask, device),
                             None, None)
    return float(out[3]), out[4]


@pytest.mark.parametrize("cols", [1, 2, 5, 8])
@pytest.mark.parametrize("rows", [1, 4, 5, 1000])
def test_predict_candidates_counts_what_the_head_counts(gpu_device, rows, cols):
    from tf_gnn_samples_amd.predict import predict_candidates
    x, mask = candidate_logits(rows, cols, seed=rows * 10 + cols)
    correct, head_logits = head_on_logits(x, mask, gpu_device)
    assert np.array_equal(head_logits.cpu().numpy().view(np.uint32), x.view(np.uint32))       # the construction gives these logits
    probs, predicted = predict_candidates(head_logits)
    p, predicted = probs.cpu().numpy(), predicted.cpu().numpy()
    assert p.dtype == np.float32 and predicted.dtype == np.int32 and p.shape == x.shape
    assert int((predicted == 0).sum()) == int(correct)
    assert np.all(p[mask == 0] == 0.0) and np.all(p[mask != 0] > 0.0)
    assert np.all((predicted >= 0) & (predicted < cols)) and np.all(mask[np.arange(rows), predicted] == 1)
    want = softmax64(x)
    assert np.allclose(p, want, rtol=(cols + 32) * 2.0 ** -24, atol=0)
    assert np.array_equal(p[np.arange(rows), predicted], p.max(axis=1))                       # the first of the largest probabilities
    assert all(predicted[r] == int(np.flatnonzero(p[r] == p[r].max())[0]) for r in range(rows))


def test_predict_candidates_designed_near_ties(gpu_device):
    from tf_gnn_samples_amd.predict import predict_candidates
    a, b = np.float32(1e-3), np.float32(1.0)
    x = np.array([[a, np.nextafter(a, np.float32(1))], [b, np.nextafter(b, np.float32(2))], [2.0, -1e7]], np.float32)
    correct, head_logits = head_on_logits(x, np.array([[1, 1], [1, 1], [1, 0]], np.float32), gpu_device)
    probs, predicted = predict_candidates(head_logits)
    assert predicted.tolist() == [0, 1, 0] and correct == 2.0
    p = probs.cpu().numpy()
    assert p[0, 0] == 0.5 and p[0, 1] == 0.5 and p[1, 1] > p[1, 0] and p[2, 1] == 0.0 and p[2, 0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------
PIPELINES = {"numpy": dict(native_batching=False), "packer": dict(native_batching=True, resident_dataset=False),
             "resident": dict(native_batching=True, resident_dataset=True)}


def pick_max_nodes(sizes):
    """max_nodes_in_batch for which the packing rule (graphs are taken while the node count stays below it) cuts `sizes` into at
    least three batches of which one holds a single graph."""
    for limit in range(max(sizes) + 1, sum(sizes) + 2):
        batches, current, offset = [], 0, 0
        for n in sizes:
            if current and offset + n >= limit:
                batches.append(current)
                current, offset = 0, 0
            current += 1
            offset += n
        batches.append(current)
        if len(batches) >= 3 and 1 in batches and max(batches) >= 2:
            return limit, batches
    raise AssertionError("no batch limit cuts %s as wanted" % (sizes,))


def build_ppi(device, pipeline, result_dir):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(5, 1, seed=4, mean_nodes=70, std_nodes=8, min_nodes=60, max_nodes=80, fwd_edges_per_node=4.0)
    data = task._loaded_data[DataFold.TRAIN]
    limit, _ = pick_max_nodes([len(g.node_features) for g in data])
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, max_nodes_in_batch=limit, random_seed=7, **PIPELINES[pipeline])
    return RGCN_Model(p, task, run_id="ppi", result_dir=str(result_dir), device=str(device)), data


def build_qm9(device, pipeline, result_dir):
    from tf_gnn_samples_amd.models import GGNN_Model
    from tf_gnn_samples_amd.tasks import QM9_Task
    tp = QM9_Task.default_params()
    tp["task_ids"] = [0, 3, 7]
    task = QM9_Task(tp)
    with gzip.open(HERE / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
        data = task.load_raw([json.loads(line) for _, line in zip(range(11), f)])
    limit, _ = pick_max_nodes([len(g.node_features) for g in data])
    p = GGNN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, max_nodes_in_batch=limit, random_seed=7, **PIPELINES[pipeline])
    return GGNN_Model(p, task, run_id="qm9", result_dir=str(result_dir), device=str(device)), data


def build_citation(device, pipeline, result_dir):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    task.load_synthetic(num_nodes=700, num_features=64, num_classes=7, num_train=100, num_valid=200, num_test=300, feature_density=0.2,
                        seed=5)
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, random_seed=7, **PIPELINES[pipeline])
    return RGCN_Model(p, task, run_id="citation", result_dir=str(result_dir), device=str(device)), task._loaded_data[DataFold.VALIDATION]


def build_varmisuse(device, pipeline, result_dir, **task_params):
    from tf_gnn_samples_amd.models import GNN_FiLM_Model
    from tf_gnn_samples_amd.tasks import DataFold, VarMisuse_Task
    task = VarMisuse_Task(dict(VarMisuse_Task.default_params(), add_self_loop_edges=True, **task_params))
    task.load_synthetic(num_graphs=7, seed=3, mean_nodes=150.0, std_nodes=40.0, min_nodes=60, max_nodes=260)
    data = task._loaded_data[DataFold.TRAIN]
    limit, _ = pick_max_nodes([len(g.node_labels_to_unique_labels) for g in data])
    p = GNN_FiLM_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, max_nodes_in_batch=limit, random_seed=11, **PIPELINES[pipeline])
    return GNN_FiLM_Model(p, task, run_id="varmisuse", result_dir=str(result_dir), device=str(device)), data


BUILDERS = {"ppi": build_ppi, "qm9": build_qm9, "citation": build_citation, "varmisuse": build_varmisuse}
KEYS = {"ppi": {"probabilities": np.float32, "labels": np.uint8}, "qm9": {"values": np.float32},
        "citation": {"probabilities": np.float32, "classes": np.int32}, "varmisuse": {"probabilities": np.float32, "predicted": np.int32}}


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k


def check_metric(name, task, samples, predictions, metrics):
    """The task's metric of ONE batch, recomputed on the host from its predictions, against what _run_epoch fetched for it."""
    if name == "ppi":
        labels = np.concatenate([p["labels"] for p in predictions]).astype(bool)
        targets = np.concatenate([np.asarray(s.node_labels) for s in samples]).astype(bool)
        tp, fp, fn = float((labels & targets).sum()), float((labels & ~targets).sum()), float((~labels & targets).sum())
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = 2 * precision * recall / (precision + recall)
        print("ppi batch: F1 %.8f from the predictions, %.8f from the metric kernel" % (f1, metrics["f1_score"]))
        assert abs(f1 - metrics["f1_score"]) <= 1e-6
    elif name == "citation":
        fold = samples[0]
        correct = float(fold.mask[predictions[0]["classes"] == fold.labels].sum())
        assert np.float32(correct) / np.float32(fold.mask.sum()) == np.float32(metrics["accuracy"])
        assert correct > 0
    elif name == "varmisuse":
        assert float(sum(int(p["predicted"] == 0) for p in predictions)) == metrics["num_correct_predictions"]
    else:
        for column, task_id in enumerate(task.params["task_ids"]):
            err = sum(abs(float(p["values"][column]) - float(np.float32(s.target_values[column]))) for p, s in zip(predictions, samples))
            want = metrics["abs_err_task%i" % task_id]
            print("qm9 batch, task %d: sum |value - target| %.8g from the predictions, %.8g from the head" % (task_id, err, want))
            assert abs(err - want) <= 1e-5 * abs(want)


def check_predictions(name, device, tmp_path, **task_params):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    build = BUILDERS[name]
    results = {}
    for pipeline in PIPELINES:
        model, data = build(device, pipeline, tmp_path, **task_params)
        results[pipeline] = model.predict(data)
    base = results["numpy"]
    same_bits(base, results["packer"])
    same_bits(base, results["resident"])                       # (`model` is the resident one from here on)
    task = model.task
    # ---- one entry per graph, in order, with the documented keys and shapes ----
    assert len(base) == len(data)
    for entry, sample in zip(base, data):
        assert {k: v.dtype for k, v in entry.items()} == {k: np.dtype(v) for k, v in KEYS[name].items()}
        n = task.num_nodes_of(sample)
        if name == "ppi":
            assert entry["probabilities"].shape == (n, task.num_labels) and entry["labels"].shape == (n, task.num_labels)
        elif name == "citation":
            assert entry["probabilities"].shape == (n, task.num_output_classes) and entry["classes"].shape == (n,)
        elif name == "qm9":
            assert entry["values"].shape == (len(task.params["task_ids"]),)
        else:
            width = task.params["max_variable_candidates"]
            assert entry["probabilities"].shape == (width,) and entry["predicted"].shape == ()
            assert np.all(entry["probabilities"][~np.asarray(sample.variable_candidate_nodes_mask, bool)] == 0.0)
    # ---- batches, the metric of each and the node states ----
    _, metrics, num_graphs, *_ = model._run_epoch("Test", list(data), DataFold.TEST, quiet=True)
    per_batch = []
    for item in model.predict_iter(data, return_states=True):
        assert torch.is_grad_enabled()                         # the generator leaves the consumer's grad mode alone between batches
        per_batch.append(item)
    assert len(model._prediction_pinned) == 2 and all(t is None or t.is_pinned() for t in model._prediction_pinned)      # two at most
    sizes = [len(samples) for samples, _ in per_batch]
    assert sum(sizes) == len(data) == num_graphs and len(per_batch) == len(metrics)
    if name != "citation":
        assert len(sizes) >= 3 and 1 in sizes, sizes
    flat = [entry for _, predictions in per_batch for entry in predictions]
    same_bits(base, [{k: v for k, v in entry.items() if k != "node_states"} for entry in flat])
    feeds = list(task.make_minibatch_iterator(list(data), DataFold.TEST, model.params["max_nodes_in_batch"]))
    assert [mb.num_graphs for mb in feeds] == sizes
    cursor = 0
    for (samples, predictions), batch_metrics, mb in zip(per_batch, metrics, feeds):
        assert all(a is b for a, b in zip(samples, data[cursor:cursor + len(samples)]))
        cursor += len(samples)
        check_metric(name, task, samples, predictions, batch_metrics)
        with torch.no_grad():
            final = model._final_node_states(DeviceBatch(mb, model.device), training=False)
        states = np.concatenate([entry["node_states"] for entry in predictions])
        assert states.dtype == np.float32 and states.shape == (mb.num_nodes, model.params["hidden_size"])
        assert states.tobytes() == final.cpu().numpy().tobytes()
        assert [entry["node_states"].shape[0] for entry in predictions] == [task.num_nodes_of(s) for s in samples]
    # ---- save -> restore -> the same bits ----
    path = str(tmp_path / ("%s.pickle" % name))
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device=str(device))
    same_bits(base, restored.predict(data))
    # ---- predict leaves nothing a training step can see ----
    step_batch = lambda: DeviceBatch(next(iter(task.make_minibatch_iterator(list(data), DataFold.VALIDATION,      # noqa: E731
                                                                             model.params["max_nodes_in_batch"]))), model.device)
    plain, _ = build(device, "resident", tmp_path, **task_params)
    want_loss = plain.train_step(step_batch())["loss"].detach().cpu().numpy().tobytes()
    model, _ = build(device, "resident", tmp_path, **task_params)
    sentinel = {n: torch.full_like(model.variables[n], 0.25) for n in model.variables.names()[:2]}
    for n, g in sentinel.items():
        model.variables[n].grad = g
    before = (torch.cuda.get_rng_state(device).clone(), torch.get_rng_state().clone(), np.random.get_state(),
              model.dropout_state.clone(), model.optimizer.t, [m.clone() for m in model.optimizer.m])
    model.predict(data, return_states=True)
    assert torch.equal(torch.cuda.get_rng_state(device), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    after = np.random.get_state()
    assert after[0] == before[2][0] and np.array_equal(after[1], before[2][1]) and after[2:] == before[2][2:]
    assert torch.equal(model.dropout_state, before[3]) and model.optimizer.t == before[4]
    assert all(torch.equal(a, b) for a, b in zip(model.optimizer.m, before[5]))
    for n in model.variables.names():
        grad = model.variables[n].grad
        assert (grad is sentinel[n] and bool((grad == 0.25).all())) if n in sentinel else grad is None, n
    assert model.train_step(step_batch())["loss"].detach().cpu().numpy().tobytes() == want_loss


def test_ppi_model_predictions(gpu_device, tmp_path):
    check_predictions("ppi", gpu_device, tmp_path)


def test_citation_model_predictions(gpu_device, tmp_path):
    check_predictions("citation", gpu_device, tmp_path)


@pytest.mark.parametrize("head", ["compose", "fused"])
def test_qm9_model_predictions(gpu_device, tmp_path, head):
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.tasks import qm9_task
    with config.override(qm9_head=head):
        check_predictions("qm9", gpu_device, tmp_path)
        assert qm9_task.ROUTES["head"] == ("hip" if head == "fused" else "composition")


@pytest.mark.parametrize("loss_function,route", [("max-likelihood", "hip"), ("max-margin", "composition")])
def test_varmisuse_model_predictions(gpu_device, tmp_path, loss_function, route):
    from tf_gnn_samples_amd.tasks import varmisuse_task
    check_predictions("varmisuse", gpu_device, tmp_path, loss_function=loss_function)
    assert varmisuse_task.ROUTES["head"] == route


def test_varmisuse_predictions_without_the_linear_layer(gpu_device, tmp_path):
    model, data = build_varmisuse(gpu_device, "numpy", tmp_path, slot_score_via_linear_layer=False)
    from tf_gnn_samples_amd.tasks import DataFold
    predictions = model.predict(data)
    _, metrics, *_ = model._run_epoch("Test", list(data), DataFold.TEST, quiet=True)
    assert sum(int(p["predicted"] == 0) for p in predictions) == sum(m["num_correct_predictions"] for m in metrics)


def test_predict_raises_when_a_product_kernel_gave_up_on_a_hand_over(gpu_device):
    """The debug knob of tests/test_gpu_limb_gemm.py (word 1 of the status block: the poll bound) on a C2-height product: the
    predictions of that forward are wrong and must not be handed out."""
    from tf_gnn_samples_amd import config as _config
    if not (_config.settings.limb_gemm and _config.settings.limb == "triple" and _config.settings.limb_pc != "0"):
        pytest.skip("the wave-role product kernel runs on the exact-split limb route only")
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(4, 1, seed=3)
    p = RGCN_Model.default_params()
    p.update(hidden_size=256, graph_num_layers=3, max_nodes_in_batch=10 ** 9)
    model = RGCN_Model(p, task, device=str(gpu_device))
    data = task._loaded_data[DataFold.TRAIN]
    assert sum(len(g.node_features) for g in data) >= 4096                # tall enough for the limb kernels
    word = ops.handover_word(gpu_device)
    assert ops.handover_status() == 0
    good = model.predict(data)
    assert len(good) == 4 and ops.handover_status() == 0
    word[1] = 1
    try:
        with pytest.raises(ops.HandoverError, match="gave up on an LDS hand-over"):
            model.predict(data)
        assert int(word[0].item()) == 0                                  # reported once, then cleared
    finally:
        word[1] = 0
        word[0] = 0
    same_bits(good, model.predict(data))


def test_gru_cell_saves_nothing_for_a_backward_under_no_grad(gpu_device):
    """A GGNN cell of [8192, 128]: with grad the one-kernel cell writes and saves z, r, r * h and the candidate (4 x [V, 128]); under
    no_grad (evaluation, prediction) it writes the output alone: the peak is at least three of those tensors lower, same bits."""
    from tf_gnn_samples_amd import utils
    gen = torch.Generator(device=gpu_device).manual_seed(1)
    V, u = 8192, 128
    x = torch.randn((V, u), device=gpu_device, generator=gen) * 0.5
    h = torch.randn((V, u), device=gpu_device, generator=gen) * 0.5
    weights = {"kernel": torch.nn.Parameter(torch.randn((u, 3 * u), device=gpu_device, generator=gen) * 0.08),
               "recurrent_kernel": torch.nn.Parameter(torch.randn((u, 3 * u), device=gpu_device, generator=gen) * 0.08),
               "bias": torch.nn.Parameter(torch.zeros(3 * u, device=gpu_device))}
    cell = utils.get_gated_unit(u, "gru", "tanh", weights)

    def peak(grad):
        with torch.set_grad_enabled(grad):
            cell(x, [h])                                         # warm-up: the weights' limb images, the allocator's blocks
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(gpu_device)
            start = torch.cuda.memory_allocated(gpu_device)
            out, _ = cell(x, [h])
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated(gpu_device) - start, out
    with_grad, out_grad = peak(True)
    without, out_plain = peak(False)
    print("GRU cell [%d, %d]: peak %d bytes with grad, %d under no_grad" % (V, u, with_grad, without))
    assert out_grad.requires_grad and not out_plain.requires_grad
    assert torch.equal(out_grad.detach(), out_plain)
    assert with_grad - without >= 3 * V * u * 4
