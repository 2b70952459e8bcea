"""VarMisuse on the GPU: the character-CNN kernels and the head kernels (csrc/varmisuse.hip) against float64, the three models against
the reference's own run (tests/golden/make_reference_run_varmisuse.py), the three input pipelines against each other, checkpoints."""
import numpy as np
import pytest
import torch

from varmisuse_cases import (FOLDS, GOLDEN, MANIFEST, MODELS, Z, build_model, build_task, charcnn_numpy, check_gradient, check_logits,
                             check_metrics, one_batch, random_labels, reference_gradients)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cnn_weights(rng, num_chars, out_dim, dtype=torch.float32, device=DEV, requires_grad=False):
    shapes = [(5, 68, 16), (16,), (num_chars - 8, 16, out_dim), (out_dim,)]
    scales = [1 / np.sqrt(5), 0.1, 1 / np.sqrt((num_chars - 8) * 16), 0.1]
    return [torch.tensor(rng.standard_normal(s) * k, dtype=dtype, device=device, requires_grad=requires_grad) for s, k in zip(shapes, scales)]


def range_labels(backward):
    from tf_gnn_samples_amd import _lib
    return int(_lib.load_library().relgnn_charcnn_range_labels(1 if backward else 0))


def run_cnn(chars, label_of_node, weights):
    from tf_gnn_samples_amd.tasks import varmisuse_task as vm
    c = torch.as_tensor(chars, device=DEV)
    m = None if label_of_node is None else torch.as_tensor(label_of_node, dtype=torch.int32, device=DEV)
    out = vm.node_label_embeddings(c, m, *weights)
    return out, vm.ROUTES["charcnn"]


# ---------------------------------------------------------------------------------------------------------------------------------
# character CNN, forward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_labels,num_chars,out_dim", [(1, 19, 64), (63, 19, 64), (257, 19, 64), (97, 12, 32), (None, 19, 64),
                                                          (40, 9, 16), (21, 32, 128)])
def test_charcnn_forward_against_float64(num_labels, num_chars, out_dim):
    if num_labels is None:
        num_labels = 2 * range_labels(False) + 3             # three workgroup steps of the forward
    rng = np.random.default_rng(num_labels * 100 + num_chars)
    chars = random_labels(rng, num_labels, num_chars)
    weights = cnn_weights(rng, num_chars, out_dim)
    out, route = run_cnn(chars, None, weights)
    assert route == "hip" and out.shape == (num_labels, out_dim)
    want = charcnn_numpy(chars, None, *[w.cpu().numpy() for w in weights])
    err = np.abs(out.cpu().numpy() - want).max()
    print("U=%d C=%d D=%d: largest difference %.3g (largest value %.3g)" % (num_labels, num_chars, out_dim, err, np.abs(want).max()))
    assert err <= 1e-5


def test_charcnn_forward_with_a_map_and_position_independence():
    rng = np.random.default_rng(5)
    chars = random_labels(rng, 120, 19)
    weights = cnn_weights(rng, 19, 64)
    label_of_node = rng.integers(0, 100, size=500)                # repeated labels; labels 100 .. 119 are unused
    out, route = run_cnn(chars, label_of_node, weights)
    assert route == "hip"
    want = charcnn_numpy(chars, label_of_node, *[w.cpu().numpy() for w in weights])
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5
    plain, _ = run_cnn(chars, None, weights)
    assert torch.equal(out, plain[torch.as_tensor(label_of_node, device=DEV)])
    # the same labels at other positions and among another number of labels: identical bits
    perm = rng.permutation(120)
    shuffled, _ = run_cnn(chars[perm], None, weights)
    assert torch.equal(shuffled, plain[torch.as_tensor(perm, device=DEV)])
    alone, _ = run_cnn(chars[37:38], None, weights)
    assert torch.equal(alone[0], plain[37])
    more, _ = run_cnn(np.concatenate([random_labels(rng, 301, 19), chars]), None, weights)
    assert torch.equal(more[301:], plain)


def test_a_map_entry_out_of_range_is_reported():
    from tf_gnn_samples_amd.graph import check_pending_graph_errors
    rng = np.random.default_rng(6)
    check_pending_graph_errors()
    out, _ = run_cnn(random_labels(rng, 10, 19), np.array([0, 3, 10, 2]), cnn_weights(rng, 19, 64))
    assert float(out[2].abs().max()) == 0.0
    with pytest.raises(ValueError):
        check_pending_graph_errors()


# ---------------------------------------------------------------------------------------------------------------------------------
# character CNN, backward
# ---------------------------------------------------------------------------------------------------------------------------------
def cnn_gradients(chars, label_of_node, weights, g):
    from tf_gnn_samples_amd.tasks import varmisuse_task as vm
    leaves = [w.detach().clone().requires_grad_(True) for w in weights]
    c = torch.as_tensor(chars, device=leaves[0].device)
    m = None if label_of_node is None else torch.as_tensor(label_of_node, dtype=torch.int32, device=leaves[0].device)
    out = vm.node_label_embeddings(c, m, *leaves)
    return torch.autograd.grad(out, leaves, grad_outputs=g), vm.ROUTES["charcnn"]


@pytest.mark.parametrize("num_labels,num_nodes", [(257, 1000), (None, None), (5, None)])
def test_charcnn_backward_against_float64_autograd(num_labels, num_nodes):
    from tf_gnn_samples_amd.tasks.varmisuse_task import charcnn_composition
    if num_labels is None:
        num_labels = 2 * range_labels(True) + 5              # three label ranges = three workgroups with partial tables
    rng = np.random.default_rng(num_labels)
    chars = random_labels(rng, num_labels, 19)
    label_of_node = None if num_nodes is None else rng.integers(0, num_labels - 7, size=num_nodes)
    rows = num_labels if num_nodes is None else num_nodes
    weights = cnn_weights(rng, 19, 64)
    g = torch.tensor(rng.standard_normal((rows, 64)), dtype=torch.float32, device=DEV)
    got, route = cnn_gradients(chars, label_of_node, weights, g)
    assert route == "hip"
    again, _ = cnn_gradients(chars, label_of_node, weights, g)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                       # two runs, the same bits
    leaves = [w.detach().cpu().double().requires_grad_(True) for w in weights]
    ref = charcnn_composition(torch.as_tensor(chars), None if label_of_node is None else torch.as_tensor(label_of_node), *leaves)
    want = torch.autograd.grad(ref, leaves, grad_outputs=g.cpu().double())
    for name, a, b in zip(("conv1d/kernel", "conv1d/bias", "conv1d_1/kernel", "conv1d_1/bias"), got, want):
        check_gradient("U=%d %s" % (num_labels, name), a.cpu().numpy(), b.numpy())


def test_an_unsupported_shape_takes_the_composition():
    rng = np.random.default_rng(9)
    chars = random_labels(rng, 30, 40)                       # 40 characters: outside the kernel's 9 .. 32
    weights = cnn_weights(rng, 40, 64)
    out, route = run_cnn(chars, None, weights)
    assert route == "composition"
    assert np.abs(out.cpu().numpy() - charcnn_numpy(chars, None, *[w.cpu().numpy() for w in weights])).max() <= 1e-4
    _, route = run_cnn(random_labels(rng, 30, 19), None, cnn_weights(rng, 19, 24))      # 24 is no multiple of 16
    assert route == "composition"
    _, route = run_cnn(random_labels(rng, 30, 19), None, cnn_weights(rng, 19, 64))
    assert route == "hip"


# ---------------------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------------------
def head_case(rng, num_graphs, hidden, scale=0.3):
    """Graphs of 7 .. 13 nodes, 1 .. 5 valid candidates, padding = the graph's node 0; graph 0: the slot IS node 0 (padded ids
    coincide with the slot), graph 1: node 0 is a real candidate (padded ids coincide with it), graph 2: one node twice."""
    sizes = rng.integers(7, 14, size=num_graphs)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    slot = np.zeros(num_graphs, np.int32)
    cands = np.zeros((num_graphs, 5), np.int32)
    mask = np.zeros((num_graphs, 5), np.float32)
    for g in range(num_graphs):
        n = (g % 5) + 1 if g != 0 else 3
        nodes = rng.permutation(np.arange(1, sizes[g]))
        slot[g] = 0 if g == 0 else nodes[0]
        cands[g, :n] = nodes[1:1 + n]
        if g == 1:
            cands[g, 0] = 0
        if g == 2 and n >= 2:
            cands[g, 1] = cands[g, 0]
        mask[g, :n] = 1.0
    states = (rng.standard_normal((int(sizes.sum()), hidden)) * scale).astype(np.float32)
    w = (rng.standard_normal((2 * hidden + 1, 1)) / np.sqrt(hidden)).astype(np.float32)
    return states, slot, cands, mask, first, w


def run_head(states, slot, cands, mask, first, w, local_ids):
    from tf_gnn_samples_amd.tasks.varmisuse_task import varmisuse_head
    h = torch.tensor(states, device=DEV, requires_grad=True)
    wt = None if w is None else torch.tensor(w, device=DEV, requires_grad=True)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=DEV)
    if local_ids:
        out = varmisuse_head(h, t(slot, torch.int32), t(cands, torch.int32), t(mask, torch.float32), t(first, torch.int32), wt)
    else:
        out = varmisuse_head(h, t(slot + first, torch.int32), t(cands + first[:, None], torch.int32), t(mask, torch.float32), None, wt)
    loss, total, accuracy, correct, logits = out
    grads = torch.autograd.grad(loss + 0.25 * total, [h] + ([] if wt is None else [wt]))
    return [x.detach() for x in (loss, total, accuracy, correct, logits)], grads


@pytest.mark.parametrize("linear", [True, False])
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("num_graphs", [1, 5, 130])
def test_head_against_float64(num_graphs, hidden, linear):
    from tf_gnn_samples_amd.tasks.varmisuse_task import head_logits_composition, head_metrics_composition
    rng = np.random.default_rng(1000 * num_graphs + hidden + int(linear))
    states, slot, cands, mask, first, w = head_case(rng, num_graphs, hidden)
    if not linear:
        w = None
    (loss, total, accuracy, correct, logits), grads = run_head(states, slot, cands, mask, first, w, local_ids=True)
    (loss2, total2, _, _, logits2), grads2 = run_head(states, slot, cands, mask, first, w, local_ids=False)
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2) and torch.equal(total, total2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))                   # local ids + offsets and absolute ids: the same bits
    h64 = torch.tensor(states, dtype=torch.float64, requires_grad=True)
    w64 = None if w is None else torch.tensor(w, dtype=torch.float64, requires_grad=True)
    ref_logits = head_logits_composition(h64, torch.as_tensor(slot + first), torch.as_tensor(cands + first[:, None]),
                                         torch.as_tensor(mask, dtype=torch.float64), w64)
    ref = head_metrics_composition(ref_logits, "max-likelihood", 0.0)
    check_logits(logits.cpu().numpy(), ref_logits.detach().numpy())
    print("loss %.9g / %.9g  total %.9g / %.9g" % (float(loss), float(ref["loss"]), float(total), float(ref["total_loss"])))
    assert abs(float(loss) - float(ref["loss"])) <= 1e-6 * abs(float(ref["loss"]))
    assert abs(float(total) - float(ref["total_loss"])) <= 1e-6 * abs(float(ref["total_loss"]))
    assert float(correct) == float(ref["num_correct_predictions"]) and abs(float(accuracy) - float(ref["accuracy"])) <= 1e-5
    want = torch.autograd.grad(ref["loss"] + 0.25 * ref["total_loss"], [h64] + ([] if w64 is None else [w64]))
    check_gradient("d states (G=%d, D=%d)" % (num_graphs, hidden), grads[0].cpu().numpy(), want[0].numpy())
    if w is not None:
        check_gradient("d w", grads[1].cpu().numpy(), want[1].numpy())
    touched = np.zeros(states.shape[0], bool)
    touched[slot + first] = True
    touched[(cands + first[:, None]).reshape(-1)] = True
    assert float(grads[0][torch.as_tensor(~touched, device=DEV)].abs().max() if (~touched).any() else 0.0) == 0.0


def test_head_ties_and_extreme_logits():
    """Equal logits at positions 0 and 2: the first maximum is position 0 = correct; a larger logit at 1: wrong; logits of +-80 next
    to masked entries: everything stays finite."""
    hidden = 64
    states = np.zeros((12, hidden), np.float32)
    e = lambda i, v: np.eye(hidden, dtype=np.float32)[i] * v
    # graph 0 (nodes 0 .. 3): slot e0, candidates e0 * 2, e0 * 1, e0 * 2 -> logits 2, 1, 2
    states[0], states[1], states[2], states[3] = e(0, 1), e(0, 2), e(0, 1), e(0, 2)
    # graph 1 (nodes 4 .. 7): logits 1, 3, 1
    states[4], states[5], states[6], states[7] = e(1, 1), e(1, 1), e(1, 3), e(1, 1)
    # graph 2 (nodes 8 .. 11): logits -80, 80, masked
    states[8], states[9], states[10] = e(2, 1), e(2, -80), e(2, 80)
    slot = np.array([0, 0, 0], np.int32)
    cands = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 0]], np.int32)
    mask = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0]], np.float32)
    first = np.array([0, 4, 8], np.int32)
    (loss, total, accuracy, correct, logits), grads = run_head(states, slot, cands, mask, first, None, local_ids=True)
    assert logits.cpu().numpy()[:2].tolist() == [[2.0, 1.0, 2.0], [1.0, 3.0, 1.0]]
    assert logits.cpu().numpy()[2].tolist() == [-80.0, 80.0, 1.0 - 1e7]      # (the padded id is the graph's node 0 = the slot: <slot, slot> = 1)
    assert float(correct) == 1.0 and abs(float(accuracy) - 1 / 3) <= 1e-7
    want = np.log(2 + np.exp(-1.0)) + (np.log(2 * np.exp(-2.0) + 1) + 2.0) + 160.0
    assert np.isfinite(float(total)) and abs(float(total) - want) <= 1e-6 * want
    assert all(bool(torch.isfinite(g).all()) for g in grads)


# ---------------------------------------------------------------------------------------------------------------------------------
# models against the reference's run
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    return build_task(tmp_path_factory.mktemp("varmisuse"), 1)


@pytest.mark.parametrize("model_name", MODELS)
def test_models_against_the_reference_run(loaded, model_name):
    from tf_gnn_samples_amd.tasks import DeviceBatch
    from tf_gnn_samples_amd.tasks import varmisuse_task as vm
    task, folds = loaded
    model, entry = build_model(model_name, task, DEV)
    assert model.variables.names() == entry["variables"] and task.num_edge_types == 23
    for name in FOLDS:
        batch = DeviceBatch(one_batch(task, folds[name]), DEV)
        if name != "train":
            with torch.no_grad():
                check_metrics(model.forward_batch(batch, training=False), entry["metrics"][name])
            continue
        initial = task.compute_initial_node_features(batch, model.variables.scope(""))
        want = Z["model/%s/initial_node_features" % model_name]
        print("initial node features: largest difference %.3g" % np.abs(initial.detach().cpu().numpy() - want).max())
        assert np.abs(initial.detach().cpu().numpy() - want).max() <= 1e-5
        metrics = model.forward_batch(batch, training=False)
        assert vm.ROUTES == {"charcnn": "hip", "head": "hip"}
        check_metrics(metrics, entry["metrics"][name])
        check_logits(task.last_logits.cpu().numpy(), Z["model/%s/logits" % model_name])
        names = model.variables.names()
        grads = torch.autograd.grad(metrics["loss"], [model.variables[n] for n in names], allow_unused=True)
        reference = reference_gradients()
        assert [n for n, g in zip(names, grads) if g is None] == entry["without_gradient"]
        for n, g in zip(names, grads):
            want = reference["model/%s/grad/%s" % (model_name, n)]
            check_gradient(n, np.zeros_like(want) if g is None else g.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# pipelines and checkpoints
# ---------------------------------------------------------------------------------------------------------------------------------
def synthetic_model(pipeline):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import VarMisuse_Task
    task = VarMisuse_Task(dict(VarMisuse_Task.default_params(), add_self_loop_edges=True))
    task.load_synthetic(num_graphs=10, seed=3, mean_nodes=150.0, std_nodes=40.0, min_nodes=60, max_nodes=260)
    p = models.GNN_FiLM_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, max_nodes_in_batch=600, random_seed=11, graph_layer_input_dropout_keep_prob=1.0,
             native_batching=pipeline != "numpy", resident_dataset=pipeline == "resident")
    return models.GNN_FiLM_Model(p, task, device=DEV), task


def test_three_pipelines_train_to_identical_bits():
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    results = {}
    for pipeline in ("numpy", "packer", "resident"):
        model, task = synthetic_model(pipeline)
        np.random.seed(77)
        losses = []
        batches = model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)
        for step, mb in enumerate(batches):
            if step == 3:
                break
            batch = mb if isinstance(mb, DeviceBatch) else DeviceBatch(mb, model.device)
            losses.append(model.train_step(batch)["loss"].detach().clone())
        if hasattr(batches, "close"):
            batches.close()
        assert len(losses) == 3
        results[pipeline] = (torch.stack(losses).cpu(), {n: model.variables[n].detach().cpu().clone() for n in model.variables.names()})
    base_losses, base_vars = results["numpy"]
    assert bool(torch.isfinite(base_losses).all())
    for pipeline in ("packer", "resident"):
        losses, variables = results[pipeline]
        assert torch.equal(losses, base_losses), (pipeline, losses, base_losses)
        assert all(torch.equal(variables[n], base_vars[n]) for n in base_vars), pipeline
    moved = [n for n in base_vars if n.startswith("conv1d")]
    fresh, _ = synthetic_model("numpy")
    assert all(not torch.equal(fresh.variables[n].detach().cpu(), base_vars[n]) for n in moved)      # the input model is being trained


def test_checkpoint_round_trip_and_epoch_loop(tmp_path):
    from tf_gnn_samples_amd import models
    model, task = synthetic_model("resident")
    model.result_dir = str(tmp_path)
    model.train(quiet=True, max_epochs=1)
    path = tmp_path / "model.pickle"
    model.save_model(str(path))
    restored = models.restore(str(path), str(tmp_path), device=DEV)
    assert type(restored.task).__name__ == "VarMisuse_Task" and restored.task.num_edge_types == 23
    assert all(torch.equal(restored.variables[n], model.variables[n]) for n in model.variables.names())
    batch = next(iter(model._batches(task.synthetic_test_data, task_fold("TEST"))))
    with torch.no_grad():
        a = model.forward_batch(batch, training=False)
        b = restored.forward_batch(batch, training=False)
    assert all(torch.equal(a[k], b[k]) for k in a)


def task_fold(name):
    from tf_gnn_samples_amd.tasks import DataFold
    return getattr(DataFold, name)


def test_reference_written_checkpoint_through_test(tmp_path, capsys):
    from tf_gnn_samples_amd import models
    from varmisuse_cases import write_varmisuse_dir
    entry = MANIFEST["parts"]["sl1"]["models"]["RGCN_Model"]
    model = models.restore(str(GOLDEN / entry["checkpoint"]), str(tmp_path), device=DEV)
    data_dir = tmp_path / "data"
    write_varmisuse_dir(str(data_dir))
    test_data = list(model.task.load_eval_data_from_path(str(data_dir / "graphs-test")))
    for pipeline in (dict(native_batching=False), dict(native_batching=True, resident_dataset=False), dict(resident_dataset=True)):
        model.params.update(pipeline)
        capsys.readouterr()
        model.test(test_data, quiet=True)
        out = capsys.readouterr().out
        want = entry["metrics"]["test"]
        assert "Metrics: Accuracy: %.3f" % want["accuracy"] in out
        loss = float([l for l in out.splitlines() if l.startswith("Loss ")][0].split()[1])
        assert abs(loss - want["loss"]) <= 1e-5, (pipeline, loss, want["loss"])           # (printed with five decimals)
