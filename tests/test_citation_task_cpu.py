"""The citation-network task against fixtures written by the REFERENCE'S OWN code (tests/golden/make_reference_run_citation.py: the
unmodified tasks/citation_network_task.py + utils/citation_network_utils.py + model classes executed over the TensorFlow shims).
tests/citation_fixture.py writes the Planetoid-format directory again (seeded); the package loads it with its own loader."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
for p in (str(GOLDEN), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

from citation_fixture import KINDS, expected_sizes, write_planetoid_dir  # noqa: E402

FOLDS = ("train", "valid", "test")
MODELS = ["RGCN_Model", "GGNN_Model", "RGAT_Model", "GNN_FiLM_Model"]


def load_fixture():
    z = np.load(GOLDEN / "reference_run_citation.npz")
    return z, json.loads(bytes(z["manifest"]).decode())


Z, MANIFEST = load_fixture()


def build_task(kind, directory, **params):
    """The package's task on the re-written directory -> (task, {fold name: data})."""
    from tf_gnn_samples_amd.tasks import DataFold, name_to_task_class
    cls, extra = name_to_task_class(kind)
    p = cls.default_params()
    p.update(extra)
    p.update(params)
    task = cls(p)
    write_planetoid_dir(str(directory), kind)
    task.load_data(str(directory))
    test = task.load_eval_data_from_path(str(directory))
    return task, {"train": task._loaded_data[DataFold.TRAIN], "valid": task._loaded_data[DataFold.VALIDATION], "test": test}


def build_model(kind, model_name, task, device):
    """The package's model with the fixture's hyper-parameters and the variables the reference's __make_model drew."""
    from make_reference_run import regenerate_variables
    from tf_gnn_samples_amd import models
    entry = MANIFEST["kinds"][kind]["models"][model_name]
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


def check_metrics(got, want):
    """loss and accuracy at the project's standing 1e-5 absolute bar, total_loss at 1e-5 relative (it grows with the number of masked
    rows), accuracy exactly (a ratio of two small integers in float32)."""
    assert abs(float(got["loss"]) - want["loss"]) <= 1e-5, (float(got["loss"]), want["loss"])
    assert abs(float(got["total_loss"]) - want["total_loss"]) <= 1e-5 * abs(want["total_loss"]), (float(got["total_loss"]), want["total_loss"])
    assert np.float32(float(got["accuracy"])) == np.float32(want["accuracy"]), (float(got["accuracy"]), want["accuracy"])


@pytest.mark.parametrize("kind", list(KINDS))
def test_loader_output_is_the_reference_s(tmp_path, kind):
    task, folds = build_task(kind, tmp_path)
    entry = MANIFEST["kinds"][kind]
    V, F, C, masked = expected_sizes(kind)
    assert task.num_edge_types == entry["num_edge_types"] == 2
    assert task.initial_node_feature_size == entry["metadata"]["initial_node_feature_size"] == F
    assert task.get_metadata()["num_output_classes"] == entry["metadata"]["num_output_classes"] == C
    for name, count in zip(FOLDS, masked):
        (d,) = folds[name]
        for l in range(2):                                            # element for element, in order
            got = np.asarray(d.adjacency_lists[l])
            assert got.dtype == np.int32 and got.shape == Z["%s/adj%d" % (kind, l)].shape
            np.testing.assert_array_equal(got, Z["%s/adj%d" % (kind, l)])
        np.testing.assert_array_equal(d.type_to_node_to_num_incoming_edges, Z[kind + "/deg"])
        assert d.type_to_node_to_num_incoming_edges.shape == (2, V)
        assert d.labels.dtype == np.int32 and d.mask.dtype == np.float32 and d.node_features.dtype == np.float32
        np.testing.assert_array_equal(d.labels, Z["%s/%s/labels" % (kind, name)])
        np.testing.assert_array_equal(d.mask, Z["%s/%s/mask" % (kind, name)].astype(np.float32))
        assert int(d.mask.sum()) == count == entry["folds"][name]["num_masked"]
        want = Z[kind + "/features"]
        assert d.node_features.shape == want.shape == (V, F)
        assert np.array_equal(d.node_features.view(np.uint32), want.view(np.uint32))       # bit for bit
        assert np.isfinite(d.node_features).all()
    assert (Z[kind + "/features"].sum(1) == 0).any()                  # the fixture has documents without words: 1 / 0 counted as 0
    if kind == "citeseer":                                            # the ids the files leave out: zero features, class 0
        holes = sorted(set(range(560, V)) - set(entry["directory"]["test_ids"]))
        assert len(holes) == 7
        assert not folds["test"][0].node_features[holes].any() and not folds["test"][0].labels[holes].any()
        assert not folds["test"][0].mask[holes].any()


@pytest.mark.parametrize("kind", list(KINDS))
def test_iterator_feeds_one_whole_graph_batch_per_fold(tmp_path, kind):
    from tf_gnn_samples_amd.tasks import DataFold
    task, folds = build_task(kind, tmp_path, out_layer_dropout_keep_prob=0.8)
    ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    for name in FOLDS:
        want = MANIFEST["kinds"][kind]["folds"][name]
        for cap in (50000, 100):                                       # max_nodes_per_batch is not consulted
            batches = list(task.make_minibatch_iterator(folds[name], ids[name], cap))
            assert len(batches) == 1 == want["num_batches"] == want["num_batches_at_max_nodes_100"]
            mb = batches[0]
            assert (mb.num_graphs, mb.num_nodes, mb.num_edges) == (1, want["num_nodes"], want["num_edges"])
            fd = mb.feed_dict
            assert mb.num_edges == sum(len(a) for a in fd["adjacency_lists"])
            assert fd["num_graphs"] == want["fed_num_graphs"] == 1
            assert fd["out_layer_dropout_keep_prob"] == want["keep_prob"] == (0.8 if name == "train" else 1.0)
            d = folds[name][0]
            assert fd["initial_node_features"] is d.node_features and fd["labels"] is d.labels and fd["mask"] is d.mask
            assert fd["type_to_num_incoming_edges"] is d.type_to_node_to_num_incoming_edges
            for l in range(2):
                np.testing.assert_array_equal(fd["adjacency_lists"][l], Z["%s/adj%d" % (kind, l)])
            assert len(fd) == len(want["feed_keys"]) - 1               # (the reference feeds its two lists under two keys)


def test_registry_names_defaults_and_metadata():
    from tf_gnn_samples_amd import tasks
    t = MANIFEST["task"]
    for name, (cls_name, extra) in t["task_names"].items():
        if cls_name == "ValueError":
            with pytest.raises(ValueError) as e:
                tasks.name_to_task_class(name)
            assert str(e.value) == extra
        else:
            cls, got_extra = tasks.name_to_task_class(name)
            assert cls.__name__ == cls_name and got_extra == extra, name
    cls = tasks.Citation_Network_Task
    assert cls.name() == t["name"] == "CitationNetwork"
    assert cls.default_data_path() == t["default_data_path"]
    assert cls.default_params() == t["default_params"]
    for name in ("ppi", "QM9"):                                        # the names that were there stay what they were
        assert tasks.name_to_task_class(name)[1] == {}
    want = MANIFEST["kinds"]["cora"]["metadata"]
    task = cls(dict(cls.default_params(), data_kind="cora"))
    task.restore_from_metadata(want)
    assert task.get_metadata() == want
    assert task.initial_node_feature_size == 48 and task.num_output_classes == 5 and task.num_edge_types == 2


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_variable_inventory_is_the_reference_s(tmp_path, capsys, kind, model_name):
    task, _ = build_task(kind, tmp_path)
    model, entry = build_model(kind, model_name, task, "cpu")
    names = model.variables.names()
    assert {n: list(model.variables[n].shape) for n in names} == dict(zip(entry["variables"], entry["variable_shapes"]))
    assert "OutputDenseLayer/kernel" in names
    logged = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Model has")]
    assert logged == [l for l in entry["logged"] if l.startswith("Model has")]


def oracle_adapter(model_name, p):
    """models/{rgcn,ggnn,rgat,gnn_film}_model.py:_apply_gnn_layer restated for oracle.model.graph_propagation."""
    from oracle import gnns as G
    from oracle import model as OM
    layer_only = lambda w: {k: v for k, v in w.items() if not k.startswith("Dense")}
    if model_name == "RGCN_Model":
        return OM.rgcn_apply(p)
    if model_name == "GGNN_Model":
        return lambda i, h, adj, deg, steps, w: G.sparse_ggnn_layer(
            h, adj, p['hidden_size'], num_timesteps=steps, gated_unit_type=p['graph_rnn_cell'],
            activation_function=p['graph_activation_function'], message_aggregation_function=p['message_aggregation_function'],
            weights=layer_only(w))
    if model_name == "RGAT_Model":
        return lambda i, h, adj, deg, steps, w: G.sparse_rgat_layer(
            h, adj, p['hidden_size'], num_heads=p['num_heads'], num_timesteps=steps,
            activation_function=p['graph_activation_function'], weights=layer_only(w))
    return lambda i, h, adj, deg, steps, w: G.sparse_gnn_film_layer(
        h, adj, deg, p['hidden_size'], num_timesteps=steps, activation_function=p['graph_activation_function'],
        message_aggregation_function=p['message_aggregation_function'],
        normalize_by_num_incoming=p['normalize_messages_by_num_incoming'], weights=layer_only(w))


def cpu_forward(model, model_name, mb):
    """The package has no CPU message passing (the layers are HIP kernels): on the CPU the GNN body is the NumPy oracle's driver loop
    over the model's own variables, the OUTPUT HEAD is the package's — Citation_Network_Task.compute_task_metrics on CPU tensors."""
    from oracle import model as OM
    from tf_gnn_samples_amd.tasks import DeviceBatch
    fd = mb.feed_dict
    W = {n[len("graph_model/"):]: model.variables[n].detach().numpy() for n in model.variables.names() if n.startswith("graph_model/")}
    final = OM.graph_propagation(fd['initial_node_features'], fd['adjacency_lists'],
                                 fd['type_to_num_incoming_edges'].astype(np.float32), model.params, W,
                                 oracle_adapter(model_name, model.params))
    batch = DeviceBatch(mb, "cpu")
    with torch.no_grad():
        return model.task.compute_task_metrics(torch.as_tensor(final), batch, model.variables.scope(model._task_scope))


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_cpu_forward_reproduces_the_reference_s_metrics(tmp_path, kind, model_name):
    from tf_gnn_samples_amd.tasks import DataFold
    task, folds = build_task(kind, tmp_path)
    model, entry = build_model(kind, model_name, task, "cpu")
    ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    for name in FOLDS:
        (mb,) = task.make_minibatch_iterator(folds[name], ids[name], 50000)
        metrics = cpu_forward(model, model_name, mb)
        assert set(metrics) == {"loss", "total_loss", "accuracy"}
        check_metrics(metrics, entry["metrics"][name])


def test_cpu_head_ties_take_the_first_index_and_an_empty_mask_divides_by_zero():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DeviceBatch, MinibatchData
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    task.restore_from_metadata({'initial_node_feature_size': 3, 'num_output_classes': 3})
    final = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [5.0, 0.0, 5.0], [0.0, 0.0, 1.0]])
    feed = {'initial_node_features': np.zeros((4, 3), np.float32), 'adjacency_lists': [np.zeros((0, 2), np.int32)] * 2,
            'type_to_num_incoming_edges': np.zeros((2, 4), np.float32), 'labels': np.array([0, 2, 0, 2], np.int32),
            'mask': np.array([1, 1, 1, 0], np.float32), 'out_layer_dropout_keep_prob': 1.0}
    batch = DeviceBatch(MinibatchData(feed, 1, 4, 0), "cpu")
    m = task.compute_task_metrics(final, batch, {"kernel": torch.eye(3)})
    assert float(m["accuracy"]) == np.float32(2.0) / np.float32(3.0)           # rows 0 and 2 pick index 0, row 1 picks 1, row 3 is masked out
    want = np.log(3.0) + np.log(2 + np.exp(-2.0)) + np.log(2 + np.exp(-5.0))
    assert abs(float(m["total_loss"]) - want) <= 1e-5 * want and abs(float(m["loss"]) - want / 3) <= 1e-5
    batch.extra['mask'] = torch.zeros(4)
    m = task.compute_task_metrics(final, batch, {"kernel": torch.eye(3)})
    assert float(m["total_loss"]) == 0.0 and np.isnan(float(m["loss"])) and np.isnan(float(m["accuracy"]))


def test_reference_written_checkpoint_restores_and_tests(tmp_path, capsys):
    """tests/golden/reference_run_checkpoints/CitationNetwork_RGCN_Model.pickle comes out of the reference's own save_model; restore()
    rebuilds task and model from it, and the test fold's metrics come out as the reference computed them (on the CPU through
    cpu_forward; model.test() itself runs the HIP layers: tests/test_gpu_citation.py)."""
    import pickle
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks import DataFold
    entry = MANIFEST["kinds"]["cora"]["models"]["RGCN_Model"]
    path = GOLDEN / entry["checkpoint"]
    data = pickle.load(open(path, "rb"))
    assert data["task_class"] == "CitationNetwork"
    assert set(data["weights"]) == {n + ":0" for n in entry["variables"]} | {"total_num_graphs:0"}
    model = models.restore(str(path), str(tmp_path), device="cpu")
    out = capsys.readouterr().out
    assert "Freshly initializing" not in out
    assert [l for l in out.splitlines() if "not used by model" in l] in ([], ["Saved weights for total_num_graphs:0 not used by model."])
    assert type(model).__name__ == "RGCN_Model" and type(model.task).__name__ == "Citation_Network_Task"
    assert model.task.params["data_kind"] == "cora" and model.task.num_output_classes == 5
    assert model.task.get_metadata() == data["task_metadata"]
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    write_planetoid_dir(str(data_dir), "cora")
    test_data = model.task.load_eval_data_from_path(str(data_dir))
    (mb,) = model.task.make_minibatch_iterator(test_data, DataFold.TEST, 50000)
    metrics = cpu_forward(model, "RGCN_Model", mb)
    check_metrics(metrics, entry["metrics"]["test"])
    assert model.task.pretty_print_epoch_task_metrics([{k: float(v) for k, v in metrics.items()}], 1) \
        == "Acc: %.2f%%" % (entry["metrics"]["test"]["accuracy"] * 100)
    assert abs(model.task.early_stopping_metric([{k: float(v) for k, v in metrics.items()}], 1) - entry["metrics"]["test"]["total_loss"]) \
        <= 1e-5 * entry["metrics"]["test"]["total_loss"]


def test_data_parallel_ranks_are_refused(monkeypatch):
    """One graph cannot be split by graph: the task's iterators refuse a process group of more than one rank."""
    import torch.distributed as dist
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    task.load_synthetic(num_nodes=700, num_features=16, num_classes=3, num_train=20, num_valid=500, num_test=100)
    data = task._loaded_data[DataFold.TRAIN]
    assert len(list(task.make_minibatch_iterator(data, DataFold.TRAIN, 10))) == 1
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="cannot be split by graph"):
        list(task.make_minibatch_iterator(data, DataFold.TRAIN, 10))


@pytest.mark.parametrize("kind", list(KINDS))
def test_host_packer_delivers_the_same_single_batch(tmp_path, kind):
    """The native route (GraphStore + NativeBatcher, here with host tensors): labels and mask travel as node payloads, and a graph
    larger than max_nodes_per_batch is still ONE batch — the packer's strict `nodes < max_nodes` rule would refuse it."""
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.batcher import NativeBatcher
    task, folds = build_task(kind, tmp_path, out_layer_dropout_keep_prob=0.8)
    for name, fold in (("train", DataFold.TRAIN), ("valid", DataFold.VALIDATION)):
        store = task.make_graph_store(folds[name])
        with pytest.raises(ValueError):
            store.split_batches([0], 100)
        batcher = NativeBatcher(store, "cpu")
        (mb,) = task.make_minibatch_iterator(folds[name], fold, 100)
        for _ in range(2):                                             # every epoch the same batch
            (batch,) = task.make_native_minibatch_iterator(batcher, fold, 100)
            assert (batch.num_graphs, batch.num_nodes, batch.num_edges) == (1, mb.num_nodes, mb.num_edges)
            fd = mb.feed_dict
            np.testing.assert_array_equal(batch.initial_node_features.numpy(), fd["initial_node_features"])
            np.testing.assert_array_equal(batch.type_to_num_incoming_edges.numpy(), fd["type_to_num_incoming_edges"].astype(np.float32))
            for got, want in zip(batch.adjacency_lists, fd["adjacency_lists"]):
                np.testing.assert_array_equal(got.numpy(), want)
            assert batch.extra["labels"].dtype == torch.int32 and batch.extra["mask"].dtype == torch.float32
            np.testing.assert_array_equal(batch.extra["labels"].numpy(), fd["labels"])
            np.testing.assert_array_equal(batch.extra["mask"].numpy(), fd["mask"])
            assert batch.extra["out_layer_dropout_keep_prob"] == fd["out_layer_dropout_keep_prob"] == (0.8 if name == "train" else 1.0)
            assert not batch.graph_nodes_list.any()
