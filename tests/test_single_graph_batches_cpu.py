"""The weak-keyed cache of tasks/single_graph_batches.py and the hooks the model driver asks a task through (tasks/sparse_graph_task.py):
a task without batching modes of its own uses the base class's as they are."""
import gc

import numpy as np
import pytest


def test_a_value_is_returned_again_for_the_same_anchors():
    from tf_gnn_samples_amd.tasks.single_graph_batches import WeakKeyedCache
    cache = WeakKeyedCache()
    a, b = np.zeros(3), np.ones(3)
    assert cache.get((a, b), "cuda:0") is None and len(cache) == 0
    value = object()
    assert cache.put((a, b), "cuda:0", value) is value
    assert cache.get((a, b), "cuda:0") is value and cache.values() == [value] and len(cache) == 1
    assert cache.get((a, b), "cuda:1") is None and cache.get((b, a), "cuda:0") is None and cache.get((a,), "cuda:0") is None
    other = cache.put((a, b), "cuda:1", object())
    assert len(cache) == 2 and cache.get((a, b), "cuda:0") is value and cache.get((a, b), "cuda:1") is other
    cache.clear()
    assert len(cache) == 0 and not cache and cache.get((a, b), "cuda:0") is None


def test_another_object_under_a_reused_id_is_a_miss(monkeypatch):
    from tf_gnn_samples_amd.tasks import single_graph_batches
    cache = single_graph_batches.WeakKeyedCache()
    first, second = np.zeros(3), np.zeros(3)
    # the same id for both objects, as the allocator gives a new array a dead one's address
    monkeypatch.setattr(single_graph_batches, "id", lambda obj: 7, raising=False)
    cache.put((first,), "k", "first's")
    assert cache.get((first,), "k") == "first's"
    assert cache.get((second,), "k") is None
    cache.put((second,), "k", "second's")
    assert cache.get((second,), "k") == "second's" and cache.get((first,), "k") is None


def test_the_entry_goes_with_any_anchor():
    from tf_gnn_samples_amd.tasks.single_graph_batches import WeakKeyedCache
    cache = WeakKeyedCache()
    a, b, c = np.zeros(3), np.ones(3), np.ones(2)
    cache.put((a, b), "x", "ab")
    cache.put((a, c), "x", "ac")
    cache.put((c,), "y", "c")
    assert len(cache) == 3
    del b
    gc.collect()
    assert len(cache) == 2 and sorted(cache.values()) == ["ac", "c"] and cache.get((a, c), "x") == "ac"
    del c
    gc.collect()
    assert len(cache) == 0


def _other_tasks():
    from tf_gnn_samples_amd.tasks import PPI_Task, QM9_Task
    ppi = PPI_Task(PPI_Task.default_params())
    ppi.load_synthetic(3, 1, seed=2, mean_nodes=50, std_nodes=5, min_nodes=40, max_nodes=60)
    qm9 = QM9_Task(QM9_Task.default_params())
    return [ppi, qm9]


def test_a_task_without_batching_modes_uses_the_hooks_as_they_are():
    from tf_gnn_samples_amd.tasks import DataFold, Sparse_Graph_Task
    from tf_gnn_samples_amd.tasks.sparse_graph_task import ModelRequirements
    for task in _other_tasks():
        for hook in ("model_requirements", "epoch_batches", "epoch_result", "check_prediction_nodes"):
            assert getattr(type(task), hook) is getattr(Sparse_Graph_Task, hook), (task.name(), hook)
        need = task.model_requirements()
        assert need == ModelRequirements() and need.layered == () and need.message_scale is None
        assert not need.deferred_projection_rows and not need.compact_projection_gradient
        for fold in DataFold:
            assert task.epoch_batches([], fold, "cuda:0", True) is None and task.epoch_batches([], fold, "cpu", False, full_graph=True) is None
            result = (0.5, [{"loss": 0.5}], 1, 1.0, 2.0, 3.0)
            assert task.epoch_result(result, fold) is result
        with pytest.raises(ValueError, match=r"predict\(nodes=\.\.\.\) is not defined for the %s task: its predictions are per graph of "
                                             r"`data`, and only a task whose data is ONE graph names single nodes" % task.name()):
            task.check_prediction_nodes([], [0])


def test_predict_nodes_is_refused_by_the_model_of_such_a_task():
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold
    ppi = _other_tasks()[0]
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, native_batching=False)
    model = RGCN_Model(p, ppi, device="cpu")
    for call in (model.predict, model.predict_iter):
        with pytest.raises(ValueError, match=r"predict\(nodes=\.\.\.\) is not defined for the PPI task"):
            call(ppi._loaded_data[DataFold.TRAIN], nodes=[0])
