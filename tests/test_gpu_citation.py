"""The citation-network task on the GPU: the masked softmax cross-entropy kernel pair (csrc/train_utils.hip: relgnn_softmax_ce_stats,
relgnn_softmax_ce_bwd) against float64 NumPy, the four models against the reference-run fixture
(tests/golden/make_reference_run_citation.py), the three input pipelines, checkpoints."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for p in (str(HERE / "golden"), str(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from citation_fixture import KINDS, write_planetoid_dir  # noqa: E402
from test_citation_task_cpu import GOLDEN, MANIFEST, MODELS, build_model, build_task, check_metrics  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 667, 4099]
# the issue's widths, and the widths at which the kernel changes the number of lanes per row (1 lane up to 8 columns, 16 up to 128)
COLS = [1, 2, 3, 7, 16, 17, 64, 121, 1000, 8, 9, 128, 129]


def reference_stats(x32, labels, mask):
    """float64 restatement of tasks/citation_network_task.py:133-148 on the float32 logits -> (total_loss, sum of mask, masked correct
    count, loss, accuracy); the count, the sum and the accuracy as float32 arithmetic gives them from np.argmax (first maximum)."""
    x = x32.astype(np.float64)
    rows = x.shape[0]
    if rows:
        m = x.max(axis=1)
        # (log of the sum first, then the difference to the label's logit: at |logits| of 3e38 a float64 "maximum + log" would
        #  swallow the logarithm)
        losses = np.log(np.exp(x - m[:, None]).sum(axis=1)) + (m - x[np.arange(rows), labels])
        correct = (np.argmax(x32, axis=1) == labels)
    else:
        losses, correct = np.zeros(0), np.zeros(0, bool)
    total = float((losses * mask).sum())
    nmask = np.float32(mask.astype(np.float64).sum())
    ncorrect = np.float32((correct * mask.astype(np.float64)).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return total, nmask, ncorrect, total / float(nmask) if nmask else float("nan"), ncorrect / nmask


def run_stats(x32, labels, mask, device, ld=None):
    from tf_gnn_samples_amd.tasks.citation_network_task import softmax_ce_stats
    rows, cols = x32.shape
    ld = ld or cols
    base = torch.full((rows, ld), float("nan"), device=device)              # whatever sits behind a row must not be read
    base[:, :cols] = torch.as_tensor(x32, device=device)
    loss, total, accuracy, counts = softmax_ce_stats(base[:, :cols], torch.as_tensor(labels.astype(np.int32), device=device),
                                                     torch.as_tensor(mask.astype(np.float32), device=device))
    return torch.stack([counts[0], counts[1], counts[2], loss, accuracy]).cpu().numpy(), float(total)


def check_stats(got, want, what):
    total, nmask, ncorrect, loss, accuracy = want
    print("%s: total %.9g (want %.9g)  loss %.9g (want %.9g)  mask %g  correct %g" % (what, got[0], total, got[3], loss, got[1], got[2]))
    assert got[1] == nmask and got[2] == ncorrect, what                                    # exactly
    assert abs(float(got[0]) - total) <= 1e-5 * abs(total), (what, float(got[0]), total)
    if nmask == 0:
        assert np.isnan(got[3]) and np.isnan(got[4]) and got[0] == 0.0, what               # 0 / 0, as the reference's graph divides
    else:
        assert abs(float(got[3]) - loss) <= 1e-5, (what, float(got[3]), loss)
        assert got[4] == accuracy, (what, got[4], accuracy)                                # exactly: float32(count) / float32(sum)


@pytest.mark.parametrize("cols", COLS)
def test_softmax_ce_stats_kernel_against_float64(gpu_device, cols):
    rng = np.random.default_rng(cols)
    for rows in ROWS:
        x = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
        x[::2] = np.round(x[::2])                                       # every other row on a coarse grid: equal maxima do occur
        labels = rng.integers(0, cols, size=rows)
        masks = {"random": (rng.random(rows) < 0.4), "ones": np.ones(rows, bool), "single": np.zeros(rows, bool)}
        if rows:
            masks["single"][rng.integers(0, rows)] = True
            labels[::3] = np.argmax(x[::3], axis=1)                     # a third of the rows is classified correctly
        for mi, (name, mask) in enumerate(masks.items()):
            lab = labels.copy()
            if name == "random" and rows:
                out = np.flatnonzero(~mask)[:2]                         # labels outside the row where the mask is 0: never used as an index
                lab[out] = [cols, -1][:len(out)]
            ld = cols if (rows + mi) % 2 == 0 else cols + 1 + (rows % 5)
            got, _ = run_stats(x, lab, mask, gpu_device, ld)
            again, _ = run_stats(x, lab, mask, gpu_device, ld)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), (rows, cols, name)       # the same bits on every run
            safe = np.where((lab >= 0) & (lab < cols), lab, 0)
            check_stats(got, reference_stats(x, safe, mask.astype(np.float32)), "rows %d cols %d ld %d mask %s" % (rows, cols, ld, name))


@pytest.mark.parametrize("cols", [3, 17, 200])
def test_softmax_ce_stats_ties_and_extreme_logits(gpu_device, cols):
    """Equal maxima pick the LOWEST index; logits of +-1e4, +-3e38 and a leading -inf give the finite losses float64 gives: the row maximum is
    subtracted before anything is exponentiated.  (A label on a -3e38 logit next to a +3e38 one would be a loss of 6e38, which no
    float32 holds: those rows carry their label on a maximum.)"""
    big = np.float32(3e38)
    rows = []
    for value in (0.0, 7.5, -1e4, 1e4, big, -big):
        rows.append((np.full(cols, value, np.float32), 0))              # all equal: index 0 is the prediction, the loss is log(cols)
        rows.append((np.full(cols, value, np.float32), cols - 1))       # ... and any other label is wrong
    r = np.full(cols, -1e4, np.float32); r[1] = 1e4
    rows += [(r, 1), (r.copy(), 0)]                                     # loss 0 and loss 2e4
    r = np.full(cols, -big, np.float32); r[[0, 2]] = big
    rows += [(r, 0), (r.copy(), 2)]                                     # two equal maxima of 3e38: log 2, the prediction is index 0
    r = np.full(cols, 1e4, np.float32); r[cols - 1] = np.float32(1e4 + 1)
    rows += [(r, cols - 1), (r.copy(), 0)]
    r = np.full(cols, 1.0, np.float32); r[0] = -np.inf
    rows += [(r, 1), (r.copy(), cols - 1)]                              # a first column of -inf counts as exp(-inf) = 0: log(cols - 1)
    x = np.stack([a for a, _ in rows])
    labels = np.array([l for _, l in rows])
    # every row on its own (a loss of exactly 2e4 is a float32; its mean with other rows would not be, and the bar on `loss` is absolute)
    for i in range(len(rows)):
        mask = np.zeros(len(rows), np.float32)
        mask[i] = 1.0
        got, _ = run_stats(x, labels, mask, gpu_device)
        assert np.isfinite(got).all(), i
        check_stats(got, reference_stats(x, labels, mask), "extremes, cols %d, row %d" % (cols, i))
    # and together, the rows whose loss is O(1)
    small = np.array([i for i in range(len(rows)) if reference_stats(x[i:i + 1], labels[i:i + 1], np.ones(1, np.float32))[0] < 50.0])
    assert len(small) >= len(rows) - 2
    for mask in (np.ones(len(small), np.float32), (np.arange(len(small)) % 3 != 1).astype(np.float32)):
        got, _ = run_stats(x[small], labels[small], mask, gpu_device)
        assert np.isfinite(got).all()
        check_stats(got, reference_stats(x[small], labels[small], mask), "extremes together, cols %d" % cols)
    first = np.flatnonzero(labels == 0)
    got, _ = run_stats(x[first], labels[first], np.ones(len(first), np.float32), gpu_device)
    assert got[2] >= 6.0                                                # the six all-equal rows with label 0 count as correct: index 0


def reference_gradient(x32, labels, mask, g_loss, g_total):
    x = x32.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    soft = e / e.sum(axis=1, keepdims=True)
    soft[np.arange(x.shape[0]), labels] -= 1.0
    return mask[:, None].astype(np.float64) * soft * (g_total + g_loss / float(mask.sum()))


@pytest.mark.parametrize("cols", [3, 7, 8, 9, 17, 121, 128, 129, 200])
@pytest.mark.parametrize("rows", [1, 65, 667])
def test_softmax_ce_backward_kernel_against_float64(gpu_device, rows, cols):
    from tf_gnn_samples_amd import _lib, config
    from tf_gnn_samples_amd.tasks.citation_network_task import softmax_ce_stats
    rng = np.random.default_rng(rows * 1000 + cols)
    x = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
    labels = rng.integers(0, cols, size=rows)
    mask = (rng.random(rows) < 0.5).astype(np.float32)
    mask[0] = 1.0
    ld = torch.as_tensor(labels.astype(np.int32), device=gpu_device)
    md = torch.as_tensor(mask, device=gpu_device)
    # through autograd: either incoming gradient alone, and both at once, on either route of the head_pad switch
    for pad in ("0", "1"):
        for g_loss, g_total in ((1.0, 0.0), (0.0, 1.0), (0.7, -0.25)):
            xd = torch.as_tensor(x, device=gpu_device).requires_grad_(True)
            with config.override(head_pad=pad):
                loss, total, accuracy, counts = softmax_ce_stats(xd, ld, md)
                assert not accuracy.requires_grad and not counts.requires_grad
                (loss * g_loss + total * g_total if g_loss and g_total else (loss * g_loss if g_loss else total * g_total)).backward()
            got = xd.grad.cpu().numpy()
            want = reference_gradient(x, labels, mask, g_loss, g_total)
            err = float(np.abs(got - want).max())
            print("rows %d cols %d pad %s g (%g, %g): max error %.3g" % (rows, cols, pad, g_loss, g_total, err))
            assert err <= 1e-5
            assert not got[mask == 0].any()                             # masked-out rows: exactly zero
    # the kernel itself, rows of the next multiple of 16 floats: zeros behind the classes, exact zeros in masked-out rows
    lib = _lib.load_library()
    ldg = (cols + 15) // 16 * 16
    xd = torch.as_tensor(x, device=gpu_device)
    xd[torch.as_tensor(mask == 0, device=gpu_device)] = float("inf")                                        # whatever a masked-out row holds, its gradient is 0
    stats = torch.empty(5, device=gpu_device)
    ws = torch.empty(lib.relgnn_softmax_ce_stats_workspace_bytes() // 8, dtype=torch.float64, device=gpu_device)
    _lib.check(lib.relgnn_softmax_ce_stats(xd.data_ptr(), cols, ld.data_ptr(), md.data_ptr(), rows, cols, stats.data_ptr(),
                                           ws.data_ptr(), ws.numel() * 8, _lib.current_stream()), "relgnn_softmax_ce_stats")
    out = torch.full((rows, ldg), float("nan"), device=gpu_device)
    g = torch.tensor([0.5], device=gpu_device)
    _lib.check(lib.relgnn_softmax_ce_bwd(xd.data_ptr(), cols, ld.data_ptr(), md.data_ptr(), rows, cols, stats.data_ptr(), g.data_ptr(),
                                         None, out.data_ptr(), ldg, _lib.current_stream()), "relgnn_softmax_ce_bwd")
    out = out.cpu().numpy()
    assert not out[:, cols:].any() and not np.isnan(out).any()
    assert not out[mask == 0].any()
    keep = mask != 0
    want = reference_gradient(x[keep], labels[keep], mask[keep], 0.5, 0.0)
    assert float(np.abs(out[keep][:, :cols] - want).max()) <= 1e-5


def _device_batch(task, data, fold, device):
    from tf_gnn_samples_amd.tasks import DeviceBatch
    (mb,) = task.make_minibatch_iterator(data, fold, 50000)
    return DeviceBatch(mb, device)


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_hip_models_reproduce_the_reference_run(gpu_device, tmp_path, kind, model_name):
    """Metrics of the three folds at the bars of the CPU suite; d loss / d variable on the train fold for EVERY variable against the
    float64 gradients of the reference's own code, at the element-wise bar tests/test_gpu_reference_run.py holds kink-free cases to
    (the fixture runs tanh everywhere): 2e-5 of the gradient's largest entry, and 2e-5 in the Frobenius norm."""
    from tf_gnn_samples_amd.tasks import DataFold
    task, folds = build_task(kind, tmp_path)
    model, entry = build_model(kind, model_name, task, str(gpu_device))
    ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    for name in ("valid", "test"):
        with torch.no_grad():
            check_metrics(model.forward_batch(_device_batch(task, folds[name], ids[name], gpu_device), training=False), entry["metrics"][name])
    metrics = model.forward_batch(_device_batch(task, folds["train"], DataFold.TRAIN, gpu_device), training=False)
    check_metrics(metrics, entry["metrics"]["train"])
    metrics["loss"].backward()
    from tf_gnn_samples_amd import ops
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


def _synthetic_task(num_nodes, num_features=64, num_classes=7, **params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))
    task.load_synthetic(num_nodes=num_nodes, num_features=num_features, num_classes=num_classes, num_train=300, num_valid=500,
                        num_test=500, feature_density=0.2, seed=5)
    return task


@pytest.mark.parametrize("case", ["fixture", "limb_route"])
def test_head_pad_routes_take_the_same_training_step(gpu_device, tmp_path, monkeypatch, case):
    """One training step with the loss gradient in plain rows (head_pad 0) and in rows padded to 16 columns (head_pad 1): the same
    updated variables within 1e-5 absolute.

    limb_route: 4352 nodes at hidden_size 256 — the head's input-gradient product [V, 7 -> 16] x [256, 7]^T then takes
    dense.R_PADDED (the limb product over the padded reduction length with the tanh' of the last Dense in its epilogue) under
    head_pad 1 and never under head_pad 0; asserted on what dense._route answers.  The limb kernels want >= 4096 rows and an output
    width that is a multiple of 256, so:
    fixture: the 660-node fixture graph at hidden_size 64 (like Cora and CiteSeer at any width) — the padded rows are written and
    tagged, and the product stays on the plain route: no R_PADDED under either value.

    The step is plain gradient descent: the update is then linear in the gradient, whereas Adam's first step moves every entry by
    lr * g / (|g| + 1e-8) — for an entry whose gradient is rounding noise that is +-lr whatever the route."""
    from tf_gnn_samples_amd import config, dense, models
    from tf_gnn_samples_amd.tasks import DataFold
    if case == "fixture":
        task, folds = build_task("cora", tmp_path)
        data, hidden = folds["train"], 64
    else:
        task = _synthetic_task(4352)
        data, hidden = task._loaded_data[DataFold.TRAIN], 256
    routes = []
    real_route = dense._route

    def recording(layout, a, b, *rest):
        out = real_route(layout, a, b, *rest)
        routes.append((layout, tuple(a.shape), tuple(b.shape), out[0]))
        return out
    monkeypatch.setattr(dense, "_route", recording)
    after, before, head = {}, {}, {}
    for pad in ("0", "1"):
        with config.override(head_pad=pad):
            p = models.RGCN_Model.default_params()
            p.update(hidden_size=hidden, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=2)
            model = models.RGCN_Model(p, task, device=str(gpu_device))
            model.optimizer = models.sparse_graph_model.TFStyleOptimizer(list(model.variables.parameters()), "SGD", 0.1, 1.0)
            before[pad] = {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}
            del routes[:]
            model.train_step(_device_batch(task, data, DataFold.TRAIN, gpu_device))
            torch.cuda.synchronize()
            after[pad] = {n: model.variables[n].detach().cpu().numpy().copy() for n in model.variables.names()}
            classes = task.num_output_classes
            head[pad] = [r for r in routes if r[0] == dense.GEMM_NT and r[2] == (hidden, classes)]
            assert len(head[pad]) == 1, routes                          # the head's input-gradient product
            padded = [r for r in routes if r[3] == dense.R_PADDED]
            print(case, "head_pad", pad, "head product:", head[pad][0], "padded:", padded)
            if case == "limb_route" and pad == "1":
                assert config.settings.limb_gemm and head[pad][0][3] == dense.R_PADDED and padded == head[pad]
            else:
                assert not padded
    for n in after["0"]:
        assert np.array_equal(before["0"][n], before["1"][n]), n        # the same initial values
        moved = float(np.abs(after["0"][n] - before["0"][n]).max())
        diff = float(np.abs(after["0"][n] - after["1"][n]).max())
        print("%s %s: moved by %.3g, head_pad 0 vs 1 differ by %.3g" % (case, n, moved, diff))
        assert diff <= 1e-5, (n, diff)
    assert max(float(np.abs(after["0"][n] - before["0"][n]).max()) for n in after["0"]) > 1e-4   # the step did move the variables


def test_output_dropout_on_the_gpu(gpu_device):
    """out_layer_dropout_keep_prob < 1 on the TRAIN fold (tasks/citation_network_task.py:123-125 of the reference): a finite loss
    that differs from the one without dropout, gradients for every variable; the other folds are fed keep 1.0 and do not change."""
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold
    losses = {}
    for keep in (1.0, 0.8):
        task = _synthetic_task(1000, num_features=32, num_classes=5, out_layer_dropout_keep_prob=keep)
        p = models.RGCN_Model.default_params()
        p.update(hidden_size=64, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=4)
        model = models.RGCN_Model(p, task, device=str(gpu_device))
        torch.manual_seed(0)
        train = _device_batch(task, task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, gpu_device)
        valid = _device_batch(task, task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, gpu_device)
        assert train.extra["out_layer_dropout_keep_prob"] == keep and valid.extra["out_layer_dropout_keep_prob"] == 1.0
        with torch.no_grad():
            v = float(model.forward_batch(valid, training=False)["loss"])
        m = model.forward_batch(train, training=False)
        m["loss"].backward()
        assert all(model.variables[n].grad is not None and torch.isfinite(model.variables[n].grad).all() for n in model.variables.names())
        losses[keep] = (float(m["loss"]), v)
    assert all(np.isfinite(x) for pair in losses.values() for x in pair)
    assert losses[0.8][0] != losses[1.0][0] and losses[0.8][1] == losses[1.0][1], losses


def _train_three_epochs(task, device, result_dir, **params):
    """train(max_epochs=3) -> per epoch and fold (loss, total_loss, accuracy, graphs, batches)."""
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3, **params)
    model = RGCN_Model(p, task, run_id="citation", result_dir=str(result_dir), device=str(device))
    record, run_epoch = [], model._run_epoch

    def recording(epoch_name, data, fold, quiet=False):
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, out[0], out[1][0]["total_loss"], out[1][0]["accuracy"], out[2], len(out[1])))
        return out
    model._run_epoch = recording
    model.train(quiet=True, max_epochs=3)
    model._run_epoch = run_epoch
    return model, record


def test_three_pipelines_train_identically_and_checkpoints_round_trip(gpu_device, tmp_path, monkeypatch):
    """The numpy iterator, the host packer and the resident fold feed the same single batch: identical per-epoch train and validation
    losses (the agreement tests/test_gpu_resident.py demands of the pipelines: equality).  max_nodes_in_batch below the graph's size
    is still one batch per epoch.  Then save_model -> restore -> test() reproduces the metrics."""
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold
    (tmp_path / "data").mkdir()
    task, folds = build_task("cora", tmp_path / "data")
    from tf_gnn_samples_amd.tasks.resident import ResidentDataset
    assembled, assemble = [], ResidentDataset.assemble

    def counting(self, *args, **kwargs):
        assembled.append(self)
        return assemble(self, *args, **kwargs)
    monkeypatch.setattr(ResidentDataset, "assemble", counting)
    runs = {}
    for name, params in (("numpy", dict(native_batching=False)), ("packer", dict(resident_dataset=False)),
                         ("resident", dict(resident_dataset=True)), ("small", dict(max_nodes_in_batch=100))):
        (tmp_path / name).mkdir()
        model, runs[name] = _train_three_epochs(task, gpu_device, tmp_path / name, **params)
        assert len(runs[name]) == 6 and all(r[4] == 1 and r[5] == 1 for r in runs[name]), runs[name]        # one graph, one batch
        for r in runs[name]:
            print(name, r)
        # a resident fold is bucketed and assembled ONCE and handed out again every epoch: two folds, three epochs, two assemblies
        assert len(assembled) == (2 if name in ("resident", "small") else 0), (name, len(assembled))
        assert len(set(map(id, assembled))) == len(assembled)
        del assembled[:]
    assert all(np.isfinite(r[1]) for r in runs["numpy"])
    assert runs["numpy"][0][1] > runs["numpy"][4][1]                    # the training loss goes down
    for name in ("packer", "resident", "small"):
        assert runs[name] == runs["numpy"], name
    # ---- save, restore, test (the last model: the default pipeline at max_nodes_in_batch = 100) ----
    test_data = folds["test"]
    _, want, n, *_ = model._run_epoch("Test", list(test_data), DataFold.TEST, quiet=True)
    path = str(tmp_path / "saved.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device=str(gpu_device))
    assert type(restored.task).__name__ == "Citation_Network_Task" and restored.task.get_metadata() == task.get_metadata()
    for v in model.variables.names():
        assert torch.equal(model.variables[v], restored.variables[v]), v
    _, got, n2, *_ = restored._run_epoch("Test", list(test_data), DataFold.TEST, quiet=True)
    assert (n, n2) == (1, 1) and got == want
    restored.test(test_data, quiet=True)
    log = open(restored.log_file).read()
    assert "Metrics: Acc: %.2f%%" % (want[0]["accuracy"] * 100) in log and "Loss %.5f on 1 graphs" % want[0]["loss"] in log


def test_reference_written_checkpoint_tests_like_the_reference(gpu_device, tmp_path):
    """restore() of the pickle the reference's own save_model wrote, then test() on the test fold: the fixture's metrics."""
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold
    entry = MANIFEST["kinds"]["cora"]["models"]["RGCN_Model"]
    model = models.restore(str(GOLDEN / entry["checkpoint"]), str(tmp_path), device=str(gpu_device))
    write_planetoid_dir(str(tmp_path), "cora")
    test_data = model.task.load_eval_data_from_path(str(tmp_path))
    _, results, n, *_ = model._run_epoch("Test", list(test_data), DataFold.TEST, quiet=True)
    assert n == 1 and len(results) == 1
    check_metrics(results[0], entry["metrics"]["test"])
    model.test(test_data, quiet=True)
    assert "Metrics: Acc: %.2f%%" % (entry["metrics"]["test"]["accuracy"] * 100) in open(model.log_file).read()
