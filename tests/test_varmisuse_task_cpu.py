"""The VarMisuse task against fixtures written by the REFERENCE'S OWN code (tests/golden/make_reference_run_varmisuse.py: the unmodified
tasks/varmisuse_task.py + model classes executed over the TensorFlow shims).  tests/varmisuse_fixture.py writes the raw dataset again
(seeded); the package loads it with its own loader.  No GPU: the input model and the head run as the task's torch compositions, the
GNN body between them through the torch oracle (tests/varmisuse_cases.py: cpu_forward)."""
import json
import pickle

import numpy as np
import pytest
import torch

from varmisuse_cases import (FOLDS, GOLDEN, MANIFEST, MODELS, Z, build_model, build_task, check_gradient, check_logits, check_metrics,
                             cpu_forward, one_batch, reference_gradients)


def split_types(flat, counts):
    ends = np.cumsum(counts)
    return [flat[e - c:e] for c, e in zip(counts, ends)]


@pytest.mark.parametrize("self_loops", [0, 1])
def test_loader_output_is_the_reference_s(tmp_path, self_loops):
    tag = "sl%d" % self_loops
    part = MANIFEST["parts"][tag]
    task, folds = build_task(tmp_path, self_loops)
    assert task.num_edge_types == part["num_edge_types"] == 22 + self_loops
    assert {k: len(v) for k, v in folds.items()} == part["fold_sizes"]
    for name in FOLDS:
        for i, g in enumerate(folds[name]):
            key = "%s/loader/%s/%d" % (tag, name, i)
            want_adj = split_types(Z[key + "/adj"], Z[key + "/adj_counts"])
            dtypes = json.loads(bytes(Z[key + "/adj_dtypes"]).decode())
            assert len(g.adjacency_lists) == len(want_adj) == task.num_edge_types
            for got, want, dtype in zip(g.adjacency_lists, want_adj, dtypes):
                assert np.array_equal(np.asarray(got).reshape(-1, 2), want) and str(np.asarray(got).dtype) == dtype
            for field, stored in (("type_to_node_to_num_incoming_edges", "deg"), ("unique_labels_as_characters", "unique"),
                                  ("node_labels_to_unique_labels", "inverse"), ("variable_candidate_nodes", "cands"),
                                  ("variable_candidate_nodes_mask", "mask")):
                got, want = np.asarray(getattr(g, field)), Z[key + "/" + stored]
                assert got.dtype == want.dtype and np.array_equal(got, want), (key, field)
            assert g.slot_node_id == int(Z[key + "/slot"])
            # the added field: the per-node character table
            assert g.node_features.dtype == np.uint8
            assert np.array_equal(g.node_features, g.unique_labels_as_characters[g.node_labels_to_unique_labels])
    # what the fixture is there to cover, seen in the loaded data
    train = folds["train"]
    assert train[0].slot_node_id == 0 and not train[0].variable_candidate_nodes_mask.all()
    assert 0 in train[1].variable_candidate_nodes[train[1].variable_candidate_nodes_mask]
    assert sorted(int(g.variable_candidate_nodes_mask.sum()) for g in train[:4]) == [1, 3, 5, 5]       # 7 candidates are cut to 5
    codes = np.concatenate([g.node_features.reshape(-1) for g in train])
    assert {0, 1, 68, 69} <= set(codes.tolist()) and codes.max() == 69


@pytest.mark.parametrize("self_loops", [0, 1])
def test_every_batch_feed_is_the_reference_s(tmp_path, self_loops):
    from tf_gnn_samples_amd.tasks import DataFold
    tag = "sl%d" % self_loops
    part = MANIFEST["parts"][tag]
    task, folds = build_task(tmp_path, self_loops)
    ids = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    placeholder_dtypes = {"unique_labels_as_characters": np.int32, "node_labels_to_unique_labels": np.int32,
                          "type_to_num_incoming_edges": np.float32, "slot_node_ids": np.int32, "candidate_node_ids": np.int32,
                          "candidate_node_ids_mask": np.float32}
    split_somewhere = False
    for max_nodes in MANIFEST["max_nodes"]:
        for name in FOLDS:
            data = list(folds[name])
            np.random.seed(MANIFEST["shuffle_seed"])
            batches = list(task.make_minibatch_iterator(data, ids[name], max_nodes))
            # the TRAIN shuffle has consumed np.random exactly as the reference's
            assert float(np.random.random()) == part["next_random_after_%d_%s" % (max_nodes, name)]
            assert len(batches) == part["batches"]["%d/%s" % (max_nodes, name)]
            split_somewhere |= len(batches) > 1
            for b, mb in enumerate(batches):
                key = "%s/batch/%d/%s/%d" % (tag, max_nodes, name, b)
                fd = mb.feed_dict
                assert [mb.num_graphs, mb.num_nodes, mb.num_edges] == Z[key + "/sizes"].tolist()
                for field, dtype in placeholder_dtypes.items():
                    want = np.asarray(Z[key + "/" + field]).astype(dtype)          # (the placeholder's dtype: what Session.run feeds)
                    assert fd[field].dtype == dtype and np.array_equal(fd[field], want), (key, field)
                want_adj = split_types(Z[key + "/adj"], Z[key + "/adj_counts"])
                assert len(fd["adjacency_lists"]) == task.num_edge_types
                for got, want in zip(fd["adjacency_lists"], want_adj):
                    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
                assert "out_layer_dropout_rate" not in fd                            # never fed (:490)
    assert split_somewhere


def test_an_oversized_first_graph_is_a_clear_error(tmp_path):
    from tf_gnn_samples_amd.tasks import DataFold
    task, folds = build_task(tmp_path, 0)
    data = sorted(folds["valid"], key=lambda g: -len(g.node_features))
    biggest = len(data[0].node_features)
    with pytest.raises(ValueError, match="does not fit max_nodes_per_batch"):
        list(task.make_minibatch_iterator(data, DataFold.VALIDATION, biggest))
    # a LATER graph that alone reaches the limit is a batch of its own, as in the reference
    last = list(task.make_minibatch_iterator(data[::-1], DataFold.VALIDATION, biggest))[-1]
    assert (last.num_graphs, last.num_nodes) == (1, biggest)


def test_names_defaults_metadata_and_files(tmp_path):
    from tf_gnn_samples_amd import tasks
    from tf_gnn_samples_amd.tasks import VarMisuse_Task
    part = MANIFEST["parts"]["sl0"]
    assert VarMisuse_Task.name() == part["name"] == "VarMisuse"
    assert VarMisuse_Task.default_params() == part["default_params"]
    assert VarMisuse_Task.default_data_path() == part["default_data_path"]
    task, folds = build_task(tmp_path, 0)
    assert task.get_metadata() == part["metadata"]
    assert task.initial_node_feature_size == part["initial_node_feature_size"] == 64
    assert tasks.CHECKPOINT_TASK_CLASSES == {"VarMisuse": VarMisuse_Task}
    # edge-type counts are per instance: a self-loop task does not change a later task
    assert VarMisuse_Task(dict(VarMisuse_Task.default_params(), add_self_loop_edges=True)).num_edge_types == 23
    assert VarMisuse_Task(VarMisuse_Task.default_params()).num_edge_types == 22
    # max_num_data_files keeps the first files in sorted order: the .jsonl.gz chunk of five graphs
    limited, limited_folds = build_task(tmp_path, 0, max_num_data_files=1)
    assert len(limited_folds["train"]) == 5
    assert all(np.array_equal(a.node_features, b.node_features) for a, b in zip(limited_folds["train"], folds["train"]))
    assert limited.pretty_print_epoch_task_metrics([{"num_correct_predictions": 3.0}, {"num_correct_predictions": 2.0}], 8) == "Accuracy: 0.625"
    assert limited.early_stopping_metric([{"num_correct_predictions": 3.0}, {"num_correct_predictions": 2.0}], 8) == -0.625


def test_restated_codeutils():
    from tf_gnn_samples_amd.tasks.varmisuse_task import get_language_keywords, split_identifier_into_parts
    assert split_identifier_into_parts("getValueCount") == ["get", "value", "count"]
    assert split_identifier_into_parts("HTTPServerName") == ["http", "server", "name"]
    assert split_identifier_into_parts("my_var_name2") == ["my", "var", "name", "2"]
    assert split_identifier_into_parts("_") == ["_"]
    assert {"if", "return", "foreach"} <= get_language_keywords("csharp") and "getValue" not in get_language_keywords("csharp")


@pytest.mark.parametrize("model_name", MODELS)
def test_variable_inventory_is_the_reference_s(tmp_path, capsys, model_name):
    task, _ = build_task(tmp_path, 1)
    model, entry = build_model(model_name, task, "cpu")
    names = model.variables.names()
    assert names == entry["variables"]                                               # creation order too
    assert [list(model.variables[n].shape) for n in names] == entry["variable_shapes"]
    assert names[:4] == ["conv1d/kernel", "conv1d/bias", "conv1d_1/kernel", "conv1d_1/bias"] and names[4].startswith("graph_model/")
    assert names[-1] == "slot_score_linear_layer/kernel"
    logged = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Model has")]
    assert logged == [l for l in entry["logged"] if l.startswith("Model has")]


@pytest.mark.parametrize("model_name", MODELS)
def test_cpu_composition_reproduces_features_logits_metrics_and_gradients(tmp_path, model_name):
    task, folds = build_task(tmp_path, 1)
    model, entry = build_model(model_name, task, "cpu")
    for name in FOLDS:
        metrics, initial, logits = cpu_forward(model, model_name, one_batch(task, folds[name]))
        check_metrics(metrics, entry["metrics"][name])
        if name == "train":
            want = Z["model/%s/initial_node_features" % model_name]
            print("initial node features: largest difference %.3g" % np.abs(initial - want).max())
            assert np.abs(initial - want).max() <= 1e-5
            check_logits(logits, Z["model/%s/logits" % model_name])
            names = [n for n in model.variables.names()]
            grads = torch.autograd.grad(metrics["loss"], [model.variables[n] for n in names], allow_unused=True)
            reference = reference_gradients()
            assert [n for n, g in zip(names, grads) if g is None] == entry["without_gradient"]
            for n, g in zip(names, grads):
                want = reference["model/%s/grad/%s" % (model_name, n)]
                check_gradient(n, np.zeros_like(want) if g is None else g.numpy(), want)


def test_no_dropout_in_any_fold_and_the_other_head_form(tmp_path):
    """out_layer_dropout_rate is accepted and never applied (the reference never feeds it); slot_score_via_linear_layer=False makes
    the inner product the logit and the head has no variable."""
    task, folds = build_task(tmp_path, 0, out_layer_dropout_rate=0.9)
    from tf_gnn_samples_amd.tasks import DeviceBatch
    batch = DeviceBatch(one_batch(task, folds["train"]), "cpu")
    states = torch.randn(batch.num_nodes, 16, generator=torch.Generator().manual_seed(0))
    w = torch.randn(33, 1, generator=torch.Generator().manual_seed(1))
    a = task.compute_task_metrics(states, batch, {"slot_score_linear_layer/kernel": w})
    b = task.compute_task_metrics(states, batch, {"slot_score_linear_layer/kernel": w})
    assert all(float(a[k]) == float(b[k]) for k in a)
    plain, _ = build_task(tmp_path, 0, slot_score_via_linear_layer=False)
    assert plain.output_variables(16) == {}
    plain.compute_task_metrics(states, batch, {})
    slot, cands = batch.extra["slot_node_ids"], batch.extra["candidate_node_ids"]
    want = (states[slot].unsqueeze(1) * states[cands]).sum(-1) + (1.0 - batch.extra["candidate_node_ids_mask"]) * -1e7
    assert torch.allclose(plain.last_logits, want, rtol=0, atol=1e-5)


def test_max_margin_against_a_hand_computation():
    """A stated deviation (the reference cannot run this loss): relu(max wrong log-prob - correct log-prob + margin) per graph."""
    from tf_gnn_samples_amd.tasks import DeviceBatch, MinibatchData, VarMisuse_Task
    p = VarMisuse_Task.default_params()
    p.update(loss_function="max-margin", slot_score_via_linear_layer=False, max_variable_candidates=3)
    p["max-margin_loss_margin"] = 0.5
    task = VarMisuse_Task(p)
    # 2 graphs of 4 nodes in a 2-dimensional state space; slot = node 0 of each graph, candidates = its nodes 1, 2, 3
    states = torch.tensor([[1.0, 0.0], [2.0, 0.0], [1.0, 5.0], [0.0, 1.0],
                           [0.0, 1.0], [9.0, 1.0], [0.0, 3.0], [7.0, 0.0]])
    feed = {"adjacency_lists": [np.zeros((0, 2), np.int32)] * 22, "type_to_num_incoming_edges": np.zeros((22, 8), np.float32),
            "slot_node_ids": np.array([0, 4], np.int32), "candidate_node_ids": np.array([[1, 2, 3], [5, 6, 4]], np.int32),
            "candidate_node_ids_mask": np.array([[1, 1, 1], [1, 1, 0]], np.float32)}
    m = task.compute_task_metrics(states, DeviceBatch(MinibatchData(feed, 2, 8, 0), "cpu"), {})
    # graph 0: logits (2, 1, 0): log-probs differ by the logits' differences: max wrong - correct = 1 - 2 = -1 -> relu(-1 + 0.5) = 0
    # graph 1: logits (1, 3, masked): 3 - 1 = 2 -> relu(2 + 0.5) = 2.5
    assert abs(float(m["total_loss"]) - 2.5) <= 1e-6 and abs(float(m["loss"]) - 1.25) <= 1e-6
    assert float(m["num_correct_predictions"]) == 1.0 and float(m["accuracy"]) == 0.5
    with pytest.raises(Exception, match="Invalid loss function"):
        VarMisuse_Task(dict(p, loss_function="hinge")).compute_task_metrics(states, DeviceBatch(MinibatchData(feed, 2, 8, 0), "cpu"), {})


def test_cpu_head_ties_take_the_first_index():
    from tf_gnn_samples_amd.tasks.varmisuse_task import head_metrics_composition
    logits = torch.tensor([[2.0, 1.0, 2.0], [1.0, 2.0, 2.0], [0.0, 0.0, 0.0]])
    m = head_metrics_composition(logits, "max-likelihood", 0.0)
    assert float(m["num_correct_predictions"]) == 2.0


def test_reference_written_checkpoint_restores(tmp_path, capsys):
    """tests/golden/reference_run_checkpoints/VarMisuse_RGCN_Model.pickle comes out of the reference's own save_model; restore()
    finds the task through CHECKPOINT_TASK_CLASSES (the name table keeps refusing the name) and the test fold's metrics come out as
    the reference computed them (model.test() itself runs the HIP layers: tests/test_gpu_varmisuse.py)."""
    from tf_gnn_samples_amd import models
    entry = MANIFEST["parts"]["sl1"]["models"]["RGCN_Model"]
    path = GOLDEN / entry["checkpoint"]
    data = pickle.load(open(path, "rb"))
    assert data["task_class"] == "VarMisuse"
    assert set(data["weights"]) == {n + ":0" for n in entry["variables"]} | {"total_num_graphs:0"}
    model = models.restore(str(path), str(tmp_path), device="cpu")
    out = capsys.readouterr().out
    assert "Freshly initializing" not in out
    assert [l for l in out.splitlines() if "not used by model" in l] in ([], ["Saved weights for total_num_graphs:0 not used by model."])
    assert type(model).__name__ == "RGCN_Model" and type(model.task).__name__ == "VarMisuse_Task"
    assert model.task.num_edge_types == 23 and model.task.get_metadata() == data["task_metadata"]
    data_dir = tmp_path / "data"
    from varmisuse_cases import write_varmisuse_dir
    write_varmisuse_dir(str(data_dir))
    test_data = list(model.task.load_eval_data_from_path(str(data_dir / "graphs-test")))
    with torch.no_grad():
        metrics, _, _ = cpu_forward(model, "RGCN_Model", one_batch(model.task, test_data))
    check_metrics(metrics, entry["metrics"]["test"])
    # a checkpoint of the package's own goes the same way
    own = tmp_path / "own.pickle"
    model.save_model(str(own))
    again = models.restore(str(own), str(tmp_path), device="cpu")
    assert all(torch.equal(again.variables[n], model.variables[n]) for n in model.variables.names())
