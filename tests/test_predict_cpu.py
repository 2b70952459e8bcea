"""Predictions without a GPU: the four task hooks on CPU tensors against hand-written expectations, and the per-graph split.  (The
C ABI of include/relgnn_predict.h is held against its binding by tests/test_abi.py.)"""
import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------------------------
# the hooks on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch(feed, num_graphs, num_nodes):
    from tf_gnn_samples_amd.tasks import DeviceBatch, MinibatchData
    return DeviceBatch(MinibatchData(feed, num_graphs, num_nodes, 0), "cpu")


SPECIAL = [0.0, -0.0, 1e-8, 1.0, -1.0, float("inf"), float("-inf"), float("nan")]


def test_ppi_hook_labels_follow_the_metric_s_rounding():
    from tf_gnn_samples_amd.tasks import PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.restore_from_metadata({'num_edge_types': 3, 'initial_node_feature_size': 1, 'num_labels': 1})
    others = [3.0, -3.0, 90.0, -90.0, 0.5, -0.5, 1e-3, -1e-3]
    final = torch.tensor(SPECIAL + others, dtype=torch.float32).reshape(16, 1)                # one logit per node: x * 1 + 0
    feed = {'initial_node_features': np.zeros((16, 1), np.float32), 'adjacency_lists': [np.zeros((0, 2), np.int32)] * 3,
            'type_to_num_incoming_edges': np.zeros((3, 16), np.float32)}                      # no target_labels: the hook reads none
    batch = _batch(feed, 1, 16)
    weights = {"kernel": torch.ones((1, 1)), "bias": torch.zeros(1)}
    out = task.compute_task_predictions(final, batch, weights)
    assert out["labels"].dtype == torch.uint8 and out["probabilities"].dtype == torch.float32
    assert tuple(out["labels"].shape) == (16, 1) and tuple(out["probabilities"].shape) == (16, 1)
    assert out["labels"][:8, 0].tolist() == [0, 0, 0, 1, 0, 1, 0, 0]
    assert out["labels"][8:, 0].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    p = out["probabilities"].numpy()[:, 0]
    assert p[0] == 0.5 and p[1] == 0.5 and p[2] == 0.5 and p[5] == 1.0 and p[6] == 0.0 and np.isnan(p[7])
    want = 1.0 / (1.0 + np.exp(-np.array(others, np.float32).astype(np.float64)))
    assert np.all(np.abs(p[8:] - want) <= 1e-6 * want + 1e-38)
    assert 0.0 <= p[11] <= 2e-38                                                              # exp(-90): a denormal or zero, never NaN
    views = {k: torch.empty(shape, dtype=dtype) for k, (shape, dtype) in task.prediction_layout(batch, 1).items()}
    again = task.compute_task_predictions(final, batch, weights, out=views)
    assert again["labels"] is views["labels"] and torch.equal(views["labels"], out["labels"])
    assert np.array_equal(views["probabilities"].numpy()[:, 0], p, equal_nan=True)


def test_citation_hook_takes_the_lowest_index_of_a_tie_for_every_node():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(Citation_Network_Task.default_params())
    task.restore_from_metadata({'initial_node_feature_size': 3, 'num_output_classes': 3})
    final = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [5.0, 0.0, 5.0], [0.0, 0.0, 1.0], [-1e4, 0.0, 0.0]])      # (-inf would turn the identity product into NaN)
    feed = {'initial_node_features': np.zeros((5, 3), np.float32), 'adjacency_lists': [np.zeros((0, 2), np.int32)] * 2,
            'type_to_num_incoming_edges': np.zeros((2, 5), np.float32)}                       # no labels, no mask
    out = task.compute_task_predictions(final, _batch(feed, 1, 5), {"kernel": torch.eye(3)})
    assert out["classes"].dtype == torch.int32 and out["classes"].tolist() == [0, 1, 0, 2, 1]
    p = out["probabilities"].numpy()
    assert p.dtype == np.float32 and p.shape == (5, 3)
    assert np.allclose(p[0], 1.0 / 3.0, rtol=1e-6) and p[4, 0] == 0.0 and p[4, 1] == 0.5
    assert np.allclose(p.sum(1), 1.0, rtol=1e-6)


def _varmisuse_predictions(logit_rows, masks, loss_function="max-likelihood"):
    """The hook on a state space built to give exactly these logits: slot row = e_0, candidate row c = logit * e_0."""
    from tf_gnn_samples_amd.tasks import VarMisuse_Task
    num_graphs, num_cands = len(logit_rows), len(logit_rows[0])
    p = VarMisuse_Task.default_params()
    p.update(slot_score_via_linear_layer=False, max_variable_candidates=num_cands, loss_function=loss_function)
    task = VarMisuse_Task(p)
    per_graph = num_cands + 1
    states = torch.zeros((num_graphs * per_graph, 2), dtype=torch.float32)
    for g, row in enumerate(logit_rows):
        states[g * per_graph, 0] = 1.0
        for c, x in enumerate(row):
            states[g * per_graph + 1 + c, 0] = float(x)
    nodes = num_graphs * per_graph
    feed = {"adjacency_lists": [np.zeros((0, 2), np.int32)] * 22, "type_to_num_incoming_edges": np.zeros((22, nodes), np.float32),
            "slot_node_ids": np.arange(num_graphs, dtype=np.int32) * per_graph,
            "candidate_node_ids": (np.arange(num_graphs)[:, None] * per_graph + 1 + np.arange(num_cands)[None, :]).astype(np.int32),
            "candidate_node_ids_mask": np.asarray(masks, np.float32)}
    batch = _batch(feed, num_graphs, nodes)
    out = task.compute_task_predictions(states, batch, {})
    metrics = task.compute_task_metrics(states, batch, {})
    return out, metrics


@pytest.mark.parametrize("loss_function", ["max-likelihood", "max-margin"])
def test_varmisuse_hook_takes_the_first_maximum_of_the_probabilities(loss_function):
    a = np.float32(1e-3)
    b = np.float32(1.0)
    rows = [[a, np.nextafter(a, np.float32(1))],              # one ulp apart at 1e-3: exp(-1.2e-10) rounds to 1, equal probabilities -> 0
            [b, np.nextafter(b, np.float32(2))],              # one ulp apart at 1: exp(-1.2e-7) < 1 -> candidate 1
            [np.float32(2.0), np.float32(0.0)]]               # second column masked
    out, metrics = _varmisuse_predictions(rows, [[1, 1], [1, 1], [1, 0]], loss_function)
    assert out["predicted"].dtype == torch.int32 and out["predicted"].tolist() == [0, 1, 0]
    p = out["probabilities"].numpy()
    assert p.dtype == np.float32 and p[0, 0] == 0.5 and p[0, 1] == 0.5 and p[1, 1] > p[1, 0]
    assert p[2, 1] == 0.0 and p[2, 0] == 1.0                                                  # a padded candidate: exactly 0
    assert float(metrics["num_correct_predictions"]) == float((out["predicted"] == 0).sum())


def test_varmisuse_hook_pads_to_max_candidates():
    out, _ = _varmisuse_predictions([[0.5, 1.5, -1.0, 0.0, 0.0]], [[1, 1, 1, 0, 0]])
    p = out["probabilities"].numpy()[0]
    want = np.exp(np.array([0.5, 1.5, -1.0]) - 1.5)
    want /= want.sum()
    assert out["predicted"].tolist() == [1] and np.all(p[3:] == 0.0) and np.allclose(p[:3], want, rtol=1e-6)


def test_qm9_hook_values_are_the_composition_s_per_graph_outputs(monkeypatch):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.tasks import QM9_Task

    def segment_sum(data, segment_ids, num_segments):         # (the package's segment sum is a HIP kernel: torch's stands in on the CPU)
        return torch.zeros((num_segments,) + tuple(data.shape[1:]), dtype=data.dtype).index_add_(0, segment_ids.long(), data)
    monkeypatch.setattr(ops, "unsorted_segment_sum", segment_sum)
    p = QM9_Task.default_params()
    p["task_ids"] = [3, 0]
    task = QM9_Task(p)
    task.restore_from_metadata({'num_edge_types': 4, 'annotation_size': 2})
    gen = torch.Generator().manual_seed(3)
    hidden, nodes = 4, 7
    final = torch.randn((nodes, hidden), generator=gen)
    features = torch.randn((nodes, 2), generator=gen)
    graph_of_node = np.array([0, 0, 0, 1, 2, 2, 2], np.int32)
    feed = {'initial_node_features': features.numpy(), 'adjacency_lists': [np.zeros((0, 2), np.int32)] * 4,
            'type_to_num_incoming_edges': np.zeros((4, nodes), np.float32), 'graph_nodes_list': graph_of_node}   # no target_values
    batch = _batch(feed, 3, nodes)
    weights = {}
    for t in p["task_ids"]:
        s = "out_layer_task%i/" % t
        weights[s + "regression/dense/kernel"] = torch.randn((hidden, 1), generator=gen)
        weights[s + "regression/dense/bias"] = torch.randn((1,), generator=gen)
        weights[s + "regression_gate/dense/kernel"] = torch.randn((hidden + 2, 1), generator=gen)
        weights[s + "regression_gate/dense/bias"] = torch.randn((1,), generator=gen)

    class Scope(dict):
        def scope(self, name):
            return Scope({k[len(name) + 1:]: v for k, v in self.items() if k.startswith(name + "/")})
    out = task.compute_task_predictions(final, batch, Scope(weights))
    values = out["values"].numpy()
    assert values.dtype == np.float32 and values.shape == (3, 2)
    for column, t in enumerate(p["task_ids"]):
        s = "out_layer_task%i/" % t
        per_node = final.double() @ weights[s + "regression/dense/kernel"].double() + weights[s + "regression/dense/bias"].double()
        gate = torch.sigmoid(torch.cat([final, features], 1).double() @ weights[s + "regression_gate/dense/kernel"].double()
                             + weights[s + "regression_gate/dense/bias"].double())
        gated = (gate * per_node).squeeze(1).numpy()
        want = np.array([gated[graph_of_node == g].sum() for g in range(3)])
        assert np.allclose(values[:, column], want, rtol=1e-5, atol=1e-6)
        got = task._per_graph_outputs(final, batch, Scope(weights).scope("out_layer_task%i" % t)).numpy()
        assert np.array_equal(values[:, column], got)                                        # the composition's own tensor, bit for bit


# ---------------------------------------------------------------------------------------------------------------------------------
# split_predictions
# ---------------------------------------------------------------------------------------------------------------------------------
class _Sample:
    def __init__(self, n):
        self.node_features = np.zeros((n, 2), np.float32)


class _Batch:
    def __init__(self, num_graphs, num_nodes):
        self.num_graphs, self.num_nodes = num_graphs, num_nodes


def test_split_predictions_cuts_ragged_graphs():
    from tf_gnn_samples_amd.tasks import PPI_Task, QM9_Task
    task = PPI_Task(PPI_Task.default_params())
    counts = [3, 1, 5]
    host = {"probabilities": np.arange(9 * 4, dtype=np.float32).reshape(9, 4), "labels": np.arange(9 * 4, dtype=np.uint8).reshape(9, 4),
            "node_states": np.arange(9 * 2, dtype=np.float32).reshape(9, 2)}
    parts = task.split_predictions(host, _Batch(3, 9), [_Sample(n) for n in counts])
    assert len(parts) == 3 and [p["labels"].shape[0] for p in parts] == counts
    assert np.array_equal(np.concatenate([p["probabilities"] for p in parts]), host["probabilities"])
    assert np.array_equal(parts[1]["node_states"], host["node_states"][3:4]) and np.array_equal(parts[2]["labels"], host["labels"][4:])
    one = task.split_predictions(host, _Batch(1, 9), [_Sample(9)])                           # a batch of one graph
    assert len(one) == 1 and np.array_equal(one[0]["labels"], host["labels"])
    # per-graph outputs are indexed by the graph, per-node ones ('node_states') still cut
    qm9 = QM9_Task(QM9_Task.default_params())
    host = {"values": np.array([[1.0], [2.0], [3.0]], np.float32), "node_states": np.zeros((9, 2), np.float32)}
    parts = qm9.split_predictions(host, _Batch(3, 9), [_Sample(n) for n in counts])
    assert [p["values"].tolist() for p in parts] == [[1.0], [2.0], [3.0]] and parts[2]["node_states"].shape == (5, 2)


def test_split_predictions_refuses_counts_that_do_not_add_up():
    from tf_gnn_samples_amd.tasks import PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    host = {"probabilities": np.zeros((9, 4), np.float32), "labels": np.zeros((9, 4), np.uint8)}
    with pytest.raises(ValueError, match="nodes"):
        task.split_predictions(host, _Batch(3, 9), [_Sample(3), _Sample(1), _Sample(4)])
    with pytest.raises(ValueError, match="samples"):
        task.split_predictions(host, _Batch(3, 9), [_Sample(4), _Sample(5)])
    with pytest.raises(ValueError, match="rows"):
        task.split_predictions({"labels": np.zeros((8, 4), np.uint8)}, _Batch(2, 9), [_Sample(4), _Sample(5)])


def test_num_nodes_of_does_not_need_a_graph_nodes_list():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, VarMisuse_Task
    from tf_gnn_samples_amd.tasks.varmisuse_task import GraphSample

    sample = GraphSample([], np.zeros((22, 6)), np.zeros((2, 19), np.uint8), np.array([0, 1, 1, 0, 1, 0]), 0, np.zeros(5, np.int64),
                         np.ones(5, bool), np.zeros((6, 19), np.uint8))
    assert VarMisuse_Task.num_nodes_of(sample) == 6
    assert Citation_Network_Task.num_nodes_of(_Sample(11)) == 11


def test_the_base_class_hooks_name_the_task():
    from tf_gnn_samples_amd.tasks import Sparse_Graph_Task

    class Bare_Task(Sparse_Graph_Task):
        pass
    task = Bare_Task({})
    with pytest.raises(NotImplementedError, match="Bare_Task"):
        task.compute_task_predictions(torch.zeros((1, 1)), None, {})
    with pytest.raises(NotImplementedError, match="Bare_Task"):
        task.prediction_layout(None, 1)


def test_prediction_arena_packs_and_returns_host_arrays_on_the_cpu():
    from tf_gnn_samples_amd.models.sparse_graph_model import _PredictionArena
    layout = {"probabilities": ((3, 5), torch.float32), "labels": ((3, 5), torch.uint8), "classes": ((3,), torch.int32)}
    arena = _PredictionArena(layout, torch.device("cpu"), [None, None], 0)
    assert all(v.data_ptr() % 16 == 0 for v in arena.views.values())
    arena.views["probabilities"].copy_(torch.arange(15, dtype=torch.float32).reshape(3, 5))
    arena.views["labels"].fill_(7)
    arena.send({"probabilities": arena.views["probabilities"], "labels": arena.views["labels"],
                "classes": torch.tensor([4, 5, 6], dtype=torch.int32)})                      # a tensor of the hook's own is copied in
    host = arena.fetch()
    assert host["probabilities"].dtype == np.float32 and host["probabilities"].tolist() == np.arange(15.0).reshape(3, 5).tolist()
    assert host["labels"].dtype == np.uint8 and np.all(host["labels"] == 7) and host["classes"].tolist() == [4, 5, 6]


def test_predict_iter_on_the_cpu_with_a_stand_in_forward(monkeypatch):
    """The generator's plumbing without a GPU (the layers are HIP kernels: a seeded stand-in makes the node states): one entry per
    graph in order, one batch late, the consumer's grad mode untouched, the two host arenas kept with the model."""
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(5, 1, seed=2, mean_nodes=50, std_nodes=5, min_nodes=40, max_nodes=60)
    data = task._loaded_data[DataFold.TRAIN]
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, max_nodes_in_batch=125, native_batching=False)
    model = RGCN_Model(p, task, device="cpu")
    grad_modes = []

    def stand_in(batch, training):
        grad_modes.append(torch.is_grad_enabled())
        assert training is False
        return torch.randn((batch.num_nodes, 16), generator=torch.Generator().manual_seed(batch.num_nodes))
    monkeypatch.setattr(model, "_final_node_states", stand_in)
    seen = []
    for samples, predictions in model.predict_iter(data, return_states=True):
        assert torch.is_grad_enabled() and len(samples) == len(predictions)
        seen.extend(samples)
        for s, entry in zip(samples, predictions):
            n = len(s.node_features)
            assert entry["labels"].shape == (n, task.num_labels) and entry["node_states"].shape == (n, 16)
    assert len(seen) == 5 and all(a is b for a, b in zip(seen, data)) and grad_modes and not any(grad_modes)
    assert len(model._prediction_pinned) == 2
    everything = model.predict(data)
    assert len(everything) == 5 and all(sorted(e) == ["labels", "probabilities"] for e in everything)
    kernel, bias = (model.variables.scope(model._task_scope)[k].detach() for k in ("kernel", "bias"))
    first = stand_in(type("B", (), {"num_nodes": sum(len(g.node_features) for g in data[:2])})(), False)
    want = (first @ kernel + bias)[:len(data[0].node_features)]
    assert np.array_equal(everything[0]["labels"], ((want > 0) & (1 / (1 + torch.exp(-want.abs())) > 0.5)).numpy().astype(np.uint8))


class _LoggedBatches:
    """An iterator over `batches` that writes ("next", k) into `log` for its k-th next(), the exhausted one included."""

    def __init__(self, batches, log):
        self._it, self._log, self._k = iter(batches), log, 0

    def __iter__(self):
        return self

    def __next__(self):
        self._log.append(("next", self._k))
        self._k += 1
        return next(self._it)


# what one pipelined pass over three batches does after it has asked for batch 0: the readback of step k - 1 is fetched only after
# the request for batch k + 1, which follows the launch of step k
PIPELINED_ORDER = [("step", 0), ("next", 1), ("step", 1), ("next", 2), ("fetch", 0), ("step", 2), ("next", 3), ("fetch", 1), ("fetch", 2)]


def _cpu_model_with_logged_batches(monkeypatch, log):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(5, 1, seed=2, mean_nodes=50, std_nodes=5, min_nodes=40, max_nodes=60)
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, max_nodes_in_batch=125, native_batching=False)
    model = RGCN_Model(p, task, device="cpu")
    batches = model._batches
    monkeypatch.setattr(model, "_batches", lambda data, fold, **how: _LoggedBatches(batches(data, fold, **how), log))
    return model, task._loaded_data[DataFold.TRAIN]


def _log_fetches(monkeypatch, cls, method, log):
    inner, count = getattr(cls, method), [0]

    def logged(self):
        log.append(("fetch", count[0]))
        count[0] += 1
        return inner(self)
    monkeypatch.setattr(cls, method, logged)


def test_an_evaluation_epoch_fetches_a_step_only_after_the_next_batch_is_requested(monkeypatch):
    from tf_gnn_samples_amd.models.sparse_graph_model import MetricsReadback
    from tf_gnn_samples_amd.tasks import DataFold
    log = []
    model, data = _cpu_model_with_logged_batches(monkeypatch, log)

    def stand_in(batch, training):
        assert training is False
        log.append(("step", sum(1 for e in log if e[0] == "step")))
        return {"loss": torch.tensor(0.5), "num_nodes": batch.num_nodes}
    monkeypatch.setattr(model, "forward_batch", stand_in)
    _log_fetches(monkeypatch, MetricsReadback, "get", log)
    loss, results, graphs = model._run_epoch("epoch 1 (validation)", data, DataFold.VALIDATION, quiet=True)[:3]
    assert log == [("next", 0)] + PIPELINED_ORDER
    assert loss == 0.5 and graphs == 5 and len(results) == 3


def test_predict_iter_fetches_a_batch_only_after_the_next_one_is_requested(monkeypatch):
    from tf_gnn_samples_amd.models.sparse_graph_model import _PredictionArena
    log = []
    model, data = _cpu_model_with_logged_batches(monkeypatch, log)

    def stand_in(batch, training):
        log.append(("step", sum(1 for e in log if e[0] == "step")))
        return torch.randn((batch.num_nodes, 16), generator=torch.Generator().manual_seed(batch.num_nodes))
    monkeypatch.setattr(model, "_final_node_states", stand_in)
    _log_fetches(monkeypatch, _PredictionArena, "fetch", log)
    assert sum(len(predictions) for _, predictions in model.predict_iter(data)) == 5
    assert log == [("next", 0)] + PIPELINED_ORDER
