"""Shared by tests/test_varmisuse_task_cpu.py and tests/test_gpu_varmisuse.py: the fixtures of
tests/golden/make_reference_run_varmisuse.py (the reference's own VarMisuse task, loader and models over the TensorFlow shims), the
dataset they were made from (tests/varmisuse_fixture.py, written again with the same seed), float64 restatements of the two
task-owned model parts, and the error bars.

Bars (the suite's standing ones): values <= 1e-5 absolute, loss <= 1e-6 relative; a gradient against float64 <= 2e-5 of that
gradient's largest entry element-wise and <= 2e-5 relative in Frobenius norm."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
for p in (str(GOLDEN), str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parent.parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

from varmisuse_fixture import write_varmisuse_dir  # noqa: E402

FOLDS = ("train", "valid", "test")
MODELS = ["RGCN_Model", "GGNN_Model", "GNN_FiLM_Model"]
Z = np.load(GOLDEN / "reference_run_varmisuse.npz")
MANIFEST = json.loads(bytes(Z["manifest"]).decode())
VALUE_BAR, LOSS_BAR, GRAD_BAR = 1e-5, 1e-6, 2e-5
_GRADS = {}


def reference_gradients():
    if not _GRADS:
        for path in sorted(GOLDEN.glob("reference_run_varmisuse_grad_*.npz")):
            with np.load(path) as z:
                _GRADS.update({k: z[k] for k in z.files})
    return _GRADS


def build_task(directory, self_loops, **params):
    """The package's task on the re-written directory -> (task, {fold name: list of samples})."""
    from tf_gnn_samples_amd.tasks import DataFold, VarMisuse_Task
    p = VarMisuse_Task.default_params()
    p.update(add_self_loop_edges=bool(self_loops), **params)
    task = VarMisuse_Task(p)
    write_varmisuse_dir(str(directory))
    task.load_data(str(directory))
    test = list(task.load_eval_data_from_path(str(Path(directory) / "graphs-test")))
    return task, {"train": task._loaded_data[DataFold.TRAIN], "valid": task._loaded_data[DataFold.VALIDATION], "test": test}


def build_model(model_name, task, device):
    """The package's model with the fixture's hyper-parameters and the variables the reference's __make_model drew."""
    from make_reference_run_varmisuse import regenerate_variables
    from tf_gnn_samples_amd import models
    entry = MANIFEST["parts"]["sl1"]["models"][model_name]
    cls = getattr(models, model_name)
    p = cls.default_params()
    p.update(entry["model_params"])
    model = cls(p, task, device=device)
    values = regenerate_variables(entry["variables"], entry["variable_shapes"], entry["variable_seed"])
    for n in entry["variables"]:
        assert float(np.asarray(values[n], np.float64).sum()) == entry["variable_checksums"][n], n
    with torch.no_grad():
        for n in entry["variables"]:
            model.variables[n].copy_(torch.as_tensor(values[n], device=device))
    from tf_gnn_samples_amd.dense import weights_changed
    weights_changed()
    return model, entry


def one_batch(task, data):
    from tf_gnn_samples_amd.tasks import DataFold
    (mb,) = task.make_minibatch_iterator(list(data), DataFold.VALIDATION, 100000)
    return mb


def torch_adapter(model_name, p):
    """models/{rgcn,ggnn,gnn_film}_model.py:_apply_gnn_layer restated for oracle.torch_model.graph_propagation."""
    from oracle import torch_model as TM
    from oracle import torch_ref as R
    layer_only = lambda w: {k: v for k, v in w.items() if not k.startswith("Dense")}
    if model_name == "RGCN_Model":
        return TM.rgcn_apply(p)
    if model_name == "GGNN_Model":
        return lambda i, h, adj, deg, steps, w: R.sparse_ggnn_layer(
            h, adj, p['hidden_size'], num_timesteps=steps, gated_unit_type=p['graph_rnn_cell'],
            activation_function=p['graph_activation_function'], message_aggregation_function=p['message_aggregation_function'],
            weights=layer_only(w))
    return lambda i, h, adj, deg, steps, w: R.sparse_gnn_film_layer(
        h, adj, deg, p['hidden_size'], num_timesteps=steps, activation_function=p['graph_activation_function'],
        message_aggregation_function=p['message_aggregation_function'],
        normalize_by_num_incoming=p['normalize_messages_by_num_incoming'], weights=layer_only(w))


def cpu_forward(model, model_name, mb):
    """The package has no CPU message passing (the layers are HIP kernels): on the CPU the GNN body is the torch oracle's driver loop
    over the model's own variables; the INPUT MODEL and the OUTPUT HEAD are the package's (the task's torch compositions).
    -> (metrics with an autograd graph, initial node features, logits)."""
    from oracle import torch_model as TM
    from tf_gnn_samples_amd.tasks import DeviceBatch
    batch = DeviceBatch(mb, "cpu")
    initial = model.task.compute_initial_node_features(batch, model.variables.scope(""))
    W = {n[len("graph_model/"):]: model.variables[n] for n in model.variables.names() if n.startswith("graph_model/")}
    final = TM.graph_propagation(initial, [a.long() for a in batch.adjacency_lists], batch.type_to_num_incoming_edges, model.params, W,
                                 torch_adapter(model_name, model.params))
    metrics = model.task.compute_task_metrics(final, batch, model.variables.scope(model._task_scope))
    return metrics, initial.detach().numpy(), model.task.last_logits.numpy()


def check_metrics(got, want):
    got = {k: float(v.detach()) for k, v in got.items()}
    assert set(got) == set(want) == {"loss", "total_loss", "accuracy", "num_correct_predictions"}
    print("metrics", got, want)
    assert abs(got["loss"] - want["loss"]) <= LOSS_BAR * abs(want["loss"]), (got, want)
    assert abs(got["total_loss"] - want["total_loss"]) <= VALUE_BAR, (got, want)
    assert abs(got["accuracy"] - want["accuracy"]) <= VALUE_BAR and got["num_correct_predictions"] == want["num_correct_predictions"]


def check_logits(got, want):
    """<= 1e-5 on the live entries; a masked entry is x - 1e7 in float32, where one ulp is 1.0: those must agree to that ulp."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    live = want > -1e6
    print("logits: largest difference %.3g (live), %.3g (masked)" % (np.abs(got - want)[live].max(), np.abs(got - want)[~live].max(initial=0.0)))
    assert np.array_equal(live, got > -1e6)
    assert np.abs(got - want)[live].max() <= VALUE_BAR
    assert np.abs(got - want)[~live].max(initial=0.0) <= 1.0


def check_gradient(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    fro = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300)
    print("%-60s max |g| %.3e  element error / max %.2e  Frobenius %.2e" % (name, scale, err / max(scale, 1e-300), fro))
    if scale == 0.0:
        assert err == 0.0, name
        return
    assert err <= GRAD_BAR * scale, (name, err, scale)
    assert fro <= GRAD_BAR, (name, fro)


# ---- float64 restatements (NumPy) of the two task-owned parts, for the kernel tests ----
def charcnn_numpy(chars, label_of_node, w1, b1, w2, b2):
    """tasks/varmisuse_task.py:341-366 in float64: one_hot(depth 68) -> conv(5) -> leaky -> maxpool(5, 1) -> conv(C - 8) -> leaky."""
    from numpy.lib.stride_tricks import sliding_window_view
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    one_hot = (np.asarray(chars)[..., None] == np.arange(w1.shape[1])).astype(np.float64)
    leaky = lambda x: np.where(x > 0, x, 0.2 * x)
    conv1 = leaky(np.einsum("utck,kcf->utf", sliding_window_view(one_hot, w1.shape[0], axis=1), w1) + b1)
    pool = sliding_window_view(conv1, w1.shape[0], axis=1).max(axis=-1)
    conv2 = leaky(np.einsum("utck,kcf->utf", sliding_window_view(pool, w2.shape[0], axis=1), w2) + b2)
    rep = conv2[:, 0, :]
    return rep if label_of_node is None else rep[np.asarray(label_of_node)]


def random_labels(rng, num_labels, num_chars):
    """Labels with what the kernel can get wrong: all-PAD rows, UNK, the two codes outside the one-hot depth, full-length rows,
    short rows padded with zeros."""
    chars = np.zeros((num_labels, num_chars), np.uint8)
    for u in range(num_labels):
        kind = u % 5
        if kind == 0 and u > 0:
            continue                                     # all PAD
        length = num_chars if kind == 1 else int(rng.integers(1, num_chars + 1))
        chars[u, :length] = rng.integers(1, 70, size=length)
        if kind == 2:
            chars[u, :min(3, length)] = [1, 68, 69][:min(3, length)]
    return chars
