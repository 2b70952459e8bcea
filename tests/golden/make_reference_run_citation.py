#!/usr/bin/env python
"""Runs the UNMODIFIED reference sources of the citation-network task (/root/reference: tasks/citation_network_task.py,
utils/citation_network_utils.py, models/*.py, gnns/*.py) in the build container, in the manner of make_reference_run.py, and writes

    tests/golden/reference_run_citation.npz     for the kinds "cora" and "citeseer" of tests/citation_fixture.py:
        * what Citation_Network_Task.load_data / load_eval_data_from_path return: adjacency lists, in-degree table, the
          row-normalised features (cast to float32 as the float32 placeholder casts them), labels and mask of the three folds;
        * what make_minibatch_iterator yields per fold (sizes, keep probability, number of batches — also with
          max_nodes_per_batch = 100), the feed arrays being the fold's own objects (asserted here);
        * name(), default_params(), default_data_path(), the metadata, the name table of utils/model_utils.py;
        * per model (RGCN, GGNN, RGAT, GNN-FiLM at hidden_size 64, 2 layers, tanh, dropout off): the variable inventory
          __make_model creates (names, shapes, the seed the values are re-drawn from), the logits and the task metrics of every
          fold (float32 NumPy run), and d loss / d variable on the train fold for every variable (float64 torch run; stored
          rounded to float32, 6e-8 relative, to keep the file small — the tests' bar is 2e-5 of a gradient's largest entry).
    tests/golden/reference_run_citation_grad_<kind>.npz     those gradients, one file per kind (182 k parameters each)
    tests/golden/reference_run_checkpoints/CitationNetwork_RGCN_Model.pickle     written by the reference's own save_model.

The existing shims (tf_numpy_shim.py, tf_torch_shim.py) are installed as they are; the few TensorFlow symbols only the citation head
touches are ADDED here (add_citation_symbols): tf.nn.sparse_softmax_cross_entropy_with_logits, tf.argmax, tf.equal, tf.constant and
a tf.placeholder_with_default that takes its first argument by the keyword the task uses (input=).  As with the other fixtures the
reference decides WHAT is computed, the shim only how one op evaluates ([TF-internal]: the cross-entropy kernel subtracts the row
maximum and takes the log of the summed exponentials in the logits' dtype; tf.argmax returns the first index among equal maxima).

Run from the repo root IN THE BUILD CONTAINER:    python tests/golden/make_reference_run_citation.py
"""
import io
import json
import os
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent
for p in (ROOT, OUT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import tf_numpy_shim as S  # noqa: E402
from citation_fixture import KINDS, write_planetoid_dir  # noqa: E402

REFERENCE = "/root/reference"
CAPTURED = {}            # the logits the reference's head handed to the cross-entropy op in the last model build

MODELS = ["RGCN_Model", "GGNN_Model", "RGAT_Model", "GNN_FiLM_Model"]
# tanh everywhere (the driver's Dense layers AND the layers' own activation: RGCN and GNN-FiLM default to ReLU there): no kinks, so
# the float32 runs can be held to the element-wise gradient bar
MODEL_PARAMS = dict(hidden_size=64, graph_num_layers=2, graph_model_activation_function="tanh", graph_activation_function="tanh",
                    graph_layer_input_dropout_keep_prob=1.0)
FOLDS = ("train", "valid", "test")


def add_citation_symbols(backend: str) -> None:
    """The symbols of tasks/citation_network_task.py:116-141 the installed shim lacks, on NumPy (float32) or torch (float64)."""
    tf = sys.modules["tensorflow"]
    if backend == "numpy":
        def sparse_ce(labels=None, logits=None, **unused):
            x = np.asarray(logits)
            CAPTURED["logits"] = np.array(x)
            shifted = x - x.max(axis=1, keepdims=True)
            log_sum = np.log(np.exp(shifted).sum(axis=1, dtype=x.dtype))
            return log_sum - shifted[np.arange(x.shape[0]), np.asarray(labels)]
        tf.nn.sparse_softmax_cross_entropy_with_logits = sparse_ce
        tf.argmax = lambda x, axis=None, output_type=np.int64, **unused: np.argmax(np.asarray(x), axis=axis).astype(output_type)
        tf.equal = lambda a, b, **unused: np.equal(a, b)
        tf.constant = lambda value, dtype=None, **unused: np.asarray(value, dtype=dtype)[()]
        tf.placeholder_with_default = lambda input=None, shape=None, name=None: S.FEEDS.get(name, input)
    else:
        import torch

        def sparse_ce(labels=None, logits=None, **unused):
            CAPTURED["logits"] = logits.detach().numpy().copy()
            return -torch.log_softmax(logits, dim=1).gather(1, labels.long().unsqueeze(1)).squeeze(1)
        tf.nn.sparse_softmax_cross_entropy_with_logits = sparse_ce
        tf.argmax = lambda x, axis=None, output_type=None, **unused: torch.argmax(x, dim=axis)
        tf.equal = lambda a, b, **unused: torch.eq(a, b)
        tf.placeholder_with_default = lambda input=None, shape=None, name=None: S.FEEDS.get(name, input)


def _placeholders():
    ph = {k: "ph:" + k for k in ("initial_node_features", "type_to_num_incoming_edges", "num_graphs", "labels", "mask",
                                 "out_layer_dropout_keep_prob")}
    ph["adjacency_lists"] = ["ph:adjacency_list_0", "ph:adjacency_list_1"]
    return ph


def _quiet(fn, *args):
    stdout, sys.stdout = sys.stdout, io.StringIO()
    try:
        return fn(*args), sys.stdout.getvalue()
    finally:
        sys.stdout = stdout


def _load_task(task_cls, kind, tmp, **params):
    from dpu_utils.utils import RichPath
    from tasks.sparse_graph_task import DataFold
    p = task_cls.default_params()
    p.update(data_kind=kind, **params)
    task = task_cls(p)
    _quiet(task.load_data, RichPath(tmp))
    test, _ = _quiet(task.load_eval_data_from_path, RichPath(tmp))
    return task, {"train": task._loaded_data[DataFold.TRAIN], "valid": task._loaded_data[DataFold.VALIDATION], "test": test}


def _feeds(fold):
    d = fold[0]
    feeds = {"initial_node_features": d.features, "type_to_num_incoming_edges": d.num_incoming_edges, "labels": d.labels, "mask": d.mask,
             "out_layer_dropout_keep_prob": 1.0, "num_graphs": 1}
    for l in range(2):
        feeds["adjacency_e%s" % l] = np.asarray(d.adj_lists[l], dtype=np.int32).reshape(-1, 2)
    return feeds


def _build(model_cls, mp, task, tmp, shim_feeds, feeds):
    """The reference's __make_model (minus the optimizer) on one fold; -> (model, ops, what it logged)."""
    shim_feeds.clear()
    shim_feeds.update(feeds)
    model = object.__new__(model_cls)             # (the constructor opens a tf.Session; everything it sets is set here)
    model.params, model.task, model.run_id, model.result_dir = mp, task, "shim", tmp
    model._Sparse_Graph_Model__placeholders, model._Sparse_Graph_Model__ops = {}, {}
    model._Sparse_Graph_Model__make_train_step = lambda: None
    _, log = _quiet(model._Sparse_Graph_Model__make_model)
    return model, model._Sparse_Graph_Model__ops, log.strip().splitlines()


def run_numpy(arrays, manifest):
    import models as ref_models
    from tasks.citation_network_task import Citation_Network_Task
    from tasks.sparse_graph_task import DataFold
    from utils import model_utils
    fold_ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    for ki, kind in enumerate(KINDS):
        tmp = tempfile.mkdtemp()
        try:
            written = write_planetoid_dir(tmp, kind)
            task, folds = _load_task(Citation_Network_Task, kind, tmp, out_layer_dropout_keep_prob=0.8)
            first = folds["train"][0]
            entry = dict(kind=kind, directory=written, num_edge_types=int(task.num_edge_types), metadata=task.get_metadata(),
                         initial_node_feature_size=int(task.initial_node_feature_size), task_params=task.params,
                         feature_dtype_of_the_reference=str(first.features.dtype), folds={}, models={})
            arrays[kind + "/features"] = np.asarray(first.features, dtype=np.float32)        # the float32 placeholder's cast
            arrays[kind + "/deg"] = np.asarray(first.num_incoming_edges)
            for l in range(2):
                arrays["%s/adj%d" % (kind, l)] = np.asarray(first.adj_lists[l], dtype=np.int32).reshape(-1, 2)
            ph = _placeholders()
            for name in FOLDS:
                assert len(folds[name]) == 1
                d = folds[name][0]
                assert d.features is first.features or np.array_equal(d.features, first.features)
                assert d.adj_lists == first.adj_lists and np.array_equal(d.num_incoming_edges, first.num_incoming_edges)
                arrays["%s/%s/labels" % (kind, name)] = np.asarray(d.labels)
                arrays["%s/%s/mask" % (kind, name)] = np.asarray(d.mask)
                batches = list(task.make_minibatch_iterator(folds[name], fold_ids[name], ph, 50000))
                small = list(task.make_minibatch_iterator(folds[name], fold_ids[name], ph, 100))
                mb = batches[0]
                fd = mb.feed_dict
                assert fd[ph["initial_node_features"]] is d.features and fd[ph["labels"]] is d.labels and fd[ph["mask"]] is d.mask
                assert fd[ph["adjacency_lists"][0]] is d.adj_lists[0] and fd[ph["adjacency_lists"][1]] is d.adj_lists[1]
                assert fd[ph["type_to_num_incoming_edges"]] is d.num_incoming_edges
                entry["folds"][name] = dict(num_batches=len(batches), num_batches_at_max_nodes_100=len(small),
                                            num_graphs=int(mb.num_graphs), num_nodes=int(mb.num_nodes), num_edges=int(mb.num_edges),
                                            fed_num_graphs=int(fd[ph["num_graphs"]]), keep_prob=float(fd[ph["out_layer_dropout_keep_prob"]]),
                                            feed_keys=sorted(str(k) for k in fd), num_masked=int(np.count_nonzero(d.mask)),
                                            label_dtype=str(np.asarray(d.labels).dtype), mask_dtype=str(np.asarray(d.mask).dtype))
            # ---- the four models: variable inventory, logits, metrics of every fold (float32 NumPy) ----
            for mi, model_name in enumerate(MODELS):
                model_cls = getattr(ref_models, model_name)
                mp = model_cls.default_params()
                mp.update(MODEL_PARAMS)
                seed = 7000 + 10 * ki + mi
                m_entry = dict(model_params=mp, variable_seed=seed, metrics={})
                for name in FOLDS:
                    S.reset(seed)
                    model, ops, log = _build(model_cls, mp, task, tmp, S.FEEDS, _feeds(folds[name]))
                    names = [n for n in S.VARIABLES if n not in S.NON_TRAINABLE]
                    if name == "train":
                        m_entry.update(variables=names, variable_shapes=[list(S.VARIABLES[n].shape) for n in names], logged=log,
                                       variable_checksums={n: float(np.asarray(S.VARIABLES[n], np.float64).sum()) for n in names})
                        arrays["%s/%s/logits" % (kind, model_name)] = np.asarray(CAPTURED["logits"], dtype=np.float32)
                        if kind == "cora" and model_name == "RGCN_Model":
                            model.sess = S.session_stub()          # the reference's own save_model (sparse_graph_model.py:90-107)
                            (OUT / "reference_run_checkpoints").mkdir(exist_ok=True)
                            m_entry["checkpoint"] = "reference_run_checkpoints/%s_%s.pickle" % (task.name(), model_name)
                            model.save_model(str(OUT / m_entry["checkpoint"]))
                    else:
                        assert names == m_entry["variables"]
                        assert np.array_equal(CAPTURED["logits"], arrays["%s/%s/logits" % (kind, model_name)])
                    m_entry["metrics"][name] = {k: float(np.asarray(v)) for k, v in ops["task_metrics"].items()}
                    for k, v in ops["task_metrics"].items():
                        assert np.asarray(v).dtype == np.float32, (k, np.asarray(v).dtype)
                entry["models"][model_name] = m_entry
                print("%-9s %-15s %3d variables  %s  train %s" % (kind, model_name, len(m_entry["variables"]), m_entry["logged"],
                                                                 {k: round(v, 5) for k, v in m_entry["metrics"]["train"].items()}))
            manifest["kinds"][kind] = entry
        finally:
            shutil.rmtree(tmp)
    # ---- names, defaults, the name table (utils/model_utils.py:12-29) ----
    table = {}
    for n in ("cora", "Cora", "citeseer", "PubMed", "citationnetwork", "CitationNetwork", "not_a_task"):
        try:
            cls, extra = model_utils.name_to_task_class(n)
            table[n] = [cls.__name__, extra]
        except ValueError as e:
            table[n] = ["ValueError", str(e)]
    manifest["task"] = dict(name=Citation_Network_Task.name(), default_params=Citation_Network_Task.default_params(),
                            default_data_path=Citation_Network_Task.default_data_path(), task_names=table)


def run_torch(arrays, manifest):
    """d loss / d variable on the train fold through the reference's own model and head code under torch.autograd (float64)."""
    import torch
    import tf_torch_shim as TS
    for name in list(sys.modules):
        if name.split(".")[0] in ("gnns", "utils", "tasks", "models"):
            del sys.modules[name]
    TS.install()
    add_citation_symbols("torch")
    import models as ref_models
    from tasks.citation_network_task import Citation_Network_Task
    for ki, kind in enumerate(KINDS):
        tmp = tempfile.mkdtemp()
        try:
            write_planetoid_dir(tmp, kind)
            task, folds = _load_task(Citation_Network_Task, kind, tmp)
            for mi, model_name in enumerate(MODELS):
                entry = manifest["kinds"][kind]["models"][model_name]
                model_cls = getattr(ref_models, model_name)
                TS.reset(entry["variable_seed"])
                _, ops, _ = _build(model_cls, entry["model_params"], task, tmp, TS.N.FEEDS, _feeds(folds["train"]))
                names = [n for n in TS.TVARS if n not in TS.N.NON_TRAINABLE]
                assert names == entry["variables"]
                loss = ops["task_metrics"]["loss"]
                want = entry["metrics"]["train"]["loss"]
                assert abs(float(loss) - want) <= 2e-5 * max(1.0, abs(want)), (kind, model_name, float(loss), want)
                assert np.abs(CAPTURED["logits"] - arrays["%s/%s/logits" % (kind, model_name)]).max() <= 2e-5
                grads = torch.autograd.grad(loss, [TS.TVARS[n] for n in names], allow_unused=True)
                entry["without_gradient"] = [n for n, g in zip(names, grads) if g is None]
                entry["loss_float64"] = float(loss)
                for n, g in zip(names, grads):
                    g = np.zeros(tuple(TS.TVARS[n].shape)) if g is None else g.numpy()
                    arrays["%s/%s/grad/%s" % (kind, model_name, n)] = g.astype(np.float32)
                print("%-9s %-15s loss %.6f (float32 run %.6f)  %d gradients" % (kind, model_name, float(loss), want, len(names)))
        finally:
            shutil.rmtree(tmp)


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("make_reference_run_citation.py needs %s (the build container)" % REFERENCE)
    S.install()
    add_citation_symbols("numpy")
    sys.path.insert(0, REFERENCE)
    arrays, manifest = {}, dict(kinds={}, numpy=np.__version__)
    import scipy
    manifest["scipy"] = scipy.__version__
    run_numpy(arrays, manifest)
    run_torch(arrays, manifest)
    arrays["manifest"] = np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8)
    # the gradients (182 k parameters per kind over the four models) go into one file per kind: no committed file above 1 MiB
    files = {"reference_run_citation.npz": {k: v for k, v in arrays.items() if "/grad/" not in k}}
    for kind in KINDS:
        files["reference_run_citation_grad_%s.npz" % kind] = {k: v for k, v in arrays.items() if "/grad/" in k and k.startswith(kind + "/")}
    for name, content in files.items():
        np.savez_compressed(OUT / name, **content)
        print("%s: %d arrays, %d bytes" % (name, len(content), (OUT / name).stat().st_size))


if __name__ == "__main__":
    main()
