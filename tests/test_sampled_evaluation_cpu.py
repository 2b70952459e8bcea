"""Evaluation and predictions on sampled receptive fields, the host side (tasks/neighbour_sampling.py: parse_evaluation,
evaluation_seed_batches, evaluation_replica, check_prediction_nodes; tasks/citation_network_task.py: evaluation_batches,
node_prediction_batches, sampled_evaluation_epoch; models/sparse_graph_model.py: the refusals and predict(nodes=...)): the key's parsing
and refusals, the seed batches and the draw rule of a fold, the epoch's sums, the argument's validation."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import layered_sampling_reference as LR  # noqa: E402

PLAIN = {"fanouts": [5, 5], "seeds_per_batch": 32, "seed": 1}
EVALUATION = {"fanouts": [0, 0], "seeds_per_batch": 7}
GOOD = dict(PLAIN, evaluation=EVALUATION)
SMALL = dict(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


def _loaded(task):
    task.load_synthetic(**SMALL)
    return task


def _cpu_model(task, **params):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(dict(dict(hidden_size=16, graph_num_layers=2, random_seed=1), **params))
    return RGCN_Model(p, task, device="cpu")


# ---- the key ------------------------------------------------------------------------------------------------------------------------
def test_the_key_is_parsed_and_carried_only_when_given():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import parse_evaluation, parse_sampled_batches
    assert parse_sampled_batches(GOOD) == GOOD
    assert "evaluation" not in parse_sampled_batches(PLAIN)
    assert parse_evaluation({"fanouts": (3, np.int64(2)), "seeds_per_batch": np.int32(9)}) == {"fanouts": [3, 2], "seeds_per_batch": 9}
    assert "keep" not in parse_evaluation(EVALUATION)
    for keep in (True, False):
        assert parse_evaluation(dict(EVALUATION, keep=keep)) == dict(EVALUATION, keep=keep)
    assert _task(sampled_batches=GOOD).evaluation == EVALUATION
    assert _task(sampled_batches=PLAIN).evaluation is None and _task().evaluation is None
    # it composes with the four other keys, and does not need "layered"
    every = dict(GOOD, sparse_features=True, sparse_update=True, sparse_gradient=True, layered=True)
    assert _task(sampled_batches=every, sparse_node_features=True).sampled_batches == every
    assert not _task(sampled_batches=GOOD).layered


# every dict the existing tests feed parse_sampled_batches, with what it gave before this key existed
UNCHANGED = [
    ({"fanouts": [0, 64], "seeds_per_batch": 7}, {"fanouts": [0, 64], "seeds_per_batch": 7, "seed": 0}),
    (PLAIN, PLAIN),
    (dict(PLAIN, sparse_features=False), dict(PLAIN, sparse_features=False)),
    (dict(PLAIN, sparse_features=True), dict(PLAIN, sparse_features=True)),
    (dict(PLAIN, sparse_features=True, sparse_update=True), dict(PLAIN, sparse_features=True, sparse_update=True)),
    (dict(PLAIN, sparse_features=True, sparse_update=True, sparse_gradient=True),
     dict(PLAIN, sparse_features=True, sparse_update=True, sparse_gradient=True)),
    (dict(PLAIN, layered=True), dict(PLAIN, layered=True)),
    (dict(PLAIN, layered=False), dict(PLAIN, layered=False)),
    ({"fanouts": (np.int32(3), 2), "seeds_per_batch": np.int64(4), "seed": np.int64(9)}, {"fanouts": [3, 2], "seeds_per_batch": 4, "seed": 9}),
]


@pytest.mark.parametrize("value, want", UNCHANGED)
def test_parse_sampled_batches_is_unchanged_without_the_key(value, want):
    from tf_gnn_samples_amd.tasks.neighbour_sampling import parse_sampled_batches
    parsed = parse_sampled_batches(value)
    assert parsed == want and list(parsed) == list(want)
    assert parse_sampled_batches(None) is None


@pytest.mark.parametrize("bad, message", [
    (7, '"evaluation" must be'), ([0, 0], '"evaluation" must be'), (None, '"evaluation" must be'), (True, '"evaluation" must be'),
    ({"fanouts": [0, 0]}, '"evaluation" must be'),                                            # a missing sub-key
    ({"seeds_per_batch": 4}, '"evaluation" must be'),
    (dict(EVALUATION, seed=3), '"evaluation" must be'),                                       # an unknown sub-key
    (dict(EVALUATION, kep=True), '"evaluation" must be'),
    (dict(EVALUATION, seeds_per_batch=True), '"evaluation": seeds_per_batch must be a positive integer'),
    (dict(EVALUATION, seeds_per_batch=0), '"evaluation": seeds_per_batch must be a positive integer'),
    (dict(EVALUATION, seeds_per_batch=2.0), '"evaluation": seeds_per_batch must be a positive integer'),
    (dict(EVALUATION, fanouts=[]), '"evaluation": fanouts must be'),
    (dict(EVALUATION, fanouts=[0, -1]), '"evaluation": fanouts must be'),
    (dict(EVALUATION, fanouts=[0, 65]), '"evaluation": fanouts must be'),
    (dict(EVALUATION, fanouts=[0, True]), '"evaluation": fanouts must be'),
    (dict(EVALUATION, fanouts=3), '"evaluation": fanouts must be'),
    (dict(EVALUATION, fanouts=[0] * 9), '"evaluation": fanouts must be'),
    (dict(EVALUATION, keep=1), '"evaluation": keep must be true or false'),
    (dict(EVALUATION, keep="yes"), '"evaluation": keep must be true or false'),
])
def test_malformed_values_are_refused_when_the_task_is_made(bad, message):
    with pytest.raises(ValueError, match=message):
        _task(sampled_batches=dict(PLAIN, evaluation=bad))


def test_an_unknown_top_level_key_keeps_its_message():
    with pytest.raises(ValueError, match="^sampled_batches must be"):
        _task(sampled_batches=dict(GOOD, evaluatoin=EVALUATION))
    with pytest.raises(ValueError, match="^sampled_batches must be"):
        _task(sampled_batches={"evaluation": EVALUATION})                                    # the key alone is no sampled_batches


def test_the_metadata_round_trip(tmp_path):
    from tf_gnn_samples_amd import models
    kept = dict(PLAIN, evaluation=dict(EVALUATION, keep=True))
    task = _loaded(_task(sampled_batches=kept))
    assert task.get_metadata()["params"]["sampled_batches"] == kept
    path = str(tmp_path / "model.pickle")
    _cpu_model(task).save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.sampled_batches == kept and restored.task.evaluation == dict(EVALUATION, keep=True)
    other = _task()
    other.restore_from_metadata(task.get_metadata())
    assert other.evaluation == dict(EVALUATION, keep=True)


def test_the_model_refuses_what_evaluation_batches_cannot_do():
    """Where "layered"'s refusals are raised, each naming "evaluation"; the key does not ask the TRAINING fanouts for anything."""
    from tf_gnn_samples_amd.tasks import DataFold
    task = _loaded(_task(sampled_batches=GOOD))
    with pytest.raises(ValueError, match='"evaluation".*graph_num_layers'):
        _cpu_model(task, graph_num_layers=3)
    with pytest.raises(ValueError, match='"evaluation".*graph_num_timesteps_per_layer'):
        _cpu_model(task, graph_num_timesteps_per_layer=2)
    three = _loaded(_task(sampled_batches=dict(PLAIN, fanouts=[4, 4, 4], evaluation=EVALUATION)))      # 3 training hops, 2 layers
    model = _cpu_model(three)
    # "layered"'s own messages are as they were
    with pytest.raises(ValueError, match='"layered": true requires as many fanouts as graph_num_layers'):
        _cpu_model(_loaded(_task(sampled_batches=dict(PLAIN, layered=True))), graph_num_layers=3)
    # a CPU model is refused as it is for sampled training, for either evaluation fold and by both iterators' switch
    for native in (True, False):
        model = _cpu_model(task, native_batching=native)
        for fold in (DataFold.VALIDATION, DataFold.TEST):
            with pytest.raises(RuntimeError, match="needs a model on the GPU"):
                model._batches(task._loaded_data[DataFold.VALIDATION], fold)
    with pytest.raises(RuntimeError, match="no device bound"):
        next(iter(task.evaluation_batches(task._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, False)))
    # without the key the evaluation folds are the full graph
    plain = _loaded(_task(sampled_batches=PLAIN))
    (mb,) = _cpu_model(plain)._batches(plain._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION)
    assert mb.num_nodes == SMALL["num_nodes"] and "layer_graphs" not in mb.feed_dict


# ---- the batches of a fold -----------------------------------------------------------------------------------------------------------
def test_the_seed_batches_of_a_fold():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import evaluation_seed_batches
    mask = np.zeros(100, dtype=np.float32)
    nodes = np.array([3, 4, 9, 17, 18, 19, 40, 41, 60, 61, 62, 63, 64, 80, 81, 98, 99])      # 17 nodes: 7 + 7 + 3
    mask[nodes] = 1.0
    batches = evaluation_seed_batches(mask, 7)
    assert [len(b) for b in batches] == [7, 7, 3] and all(b.dtype == np.int32 for b in batches)
    assert np.array_equal(np.concatenate(batches), nodes)                                    # ascending, nothing shuffled
    assert all(np.array_equal(a, b) for a, b in zip(batches, evaluation_seed_batches(mask, 7)))
    assert [len(b) for b in evaluation_seed_batches(mask, 17)] == [17] and [len(b) for b in evaluation_seed_batches(mask, 100)] == [17]
    assert len(evaluation_seed_batches(mask, 1)) == 17 and evaluation_seed_batches(np.zeros(5), 3) == []
    assert [len(b) for b in evaluation_seed_batches(mask != 0, 16)] == [16, 1]               # a bool mask
    for bad in (0, -2):
        with pytest.raises(ValueError, match="seeds_per_batch"):
            evaluation_seed_batches(mask, bad)


def test_the_replica_lies_outside_any_rank():
    from tf_gnn_samples_amd.tasks import DataFold
    from tf_gnn_samples_amd.tasks.neighbour_sampling import EVALUATION_REPLICA, PREDICT_FOLD, evaluation_replica
    assert EVALUATION_REPLICA == 0x40000000
    assert evaluation_replica(DataFold.VALIDATION.value) == 0x40000001 and evaluation_replica(DataFold.TEST.value) == 0x40000002
    assert evaluation_replica(PREDICT_FOLD) == 0x40000003 and PREDICT_FOLD not in [f.value for f in DataFold]
    assert all(evaluation_replica(f) < 2 ** 31 for f in (0, 1, 2, 3))                         # NeighbourSampler takes [0, 2^31)
    for bad in (-1, 0x40000000):
        with pytest.raises(ValueError):
            evaluation_replica(bad)


class _Recorder:
    """Stands in for the device: records what the task asks the sampling state and the sampler for."""

    def __init__(self, monkeypatch, task):
        self.states, self.batches = [], []
        monkeypatch.setattr(task.batches, "device", "cuda:0")

        def state_of(fold, device, fanouts=None, seed=None, replica=0):
            self.states.append((None if fanouts is None else list(fanouts), seed, replica))
            return ("state", replica)
        monkeypatch.setattr(task.batches, "neighbour_state", state_of)

        def batch(state, seeds, draw, full_graph_route):
            self.batches.append((state[1], draw, seeds.tolist(), full_graph_route))
            return type("Batch", (), {"extra": {}, "seeds": seeds, "draw": draw})()
        monkeypatch.setattr(task.batches, "evaluation_batch", batch)


def test_the_draws_are_a_function_of_seed_fold_and_batch_index(monkeypatch):
    """Two epochs ask for the same (replica, draw, seeds); VALIDATION and TEST differ in the replica; no evaluation draw is a training
    draw: the training sampler's replica is the rank (0 here), the evaluation replicas carry bit 30, and the task's training counters
    do not move."""
    from tf_gnn_samples_amd.tasks import DataFold
    task = _loaded(_task(sampled_batches=dict(PLAIN, evaluation={"fanouts": [3, 2], "seeds_per_batch": 7})))
    rec = _Recorder(monkeypatch, task)
    valid = task._loaded_data[DataFold.VALIDATION]
    first = list(task.evaluation_batches(valid, DataFold.VALIDATION, True))
    epoch_one, rec.batches = rec.batches, []
    second = list(task.evaluation_batches(valid, DataFold.VALIDATION, True))
    assert epoch_one == rec.batches and len(first) == len(second) == 5                       # ceil(30 / 7)
    assert [b[1] for b in epoch_one] == [0, 1, 2, 3, 4] and [len(b[2]) for b in epoch_one] == [7, 7, 7, 7, 2]
    assert np.array_equal(np.concatenate([b[2] for b in epoch_one]), np.arange(30, 60))       # the fold's nodes ascending
    assert {b[0] for b in epoch_one} == {0x40000001} and all(b[3] is True for b in epoch_one)
    assert rec.states[0] == ([3, 2], PLAIN["seed"], 0x40000001)
    assert first[0] is not second[0]                                                         # without "keep": built again
    rec.batches = []
    list(task.evaluation_batches(task.synthetic_test_data, DataFold.TEST, False))
    assert {b[0] for b in rec.batches} == {0x40000002} and [b[1] for b in rec.batches] == [0, 1, 2, 3, 4]
    assert (task.batches.epoch, task.batches.draw) == (0, 0)
    # the training batches: the parameter's own fanouts and seed, replica 0
    rec.states = []
    monkeypatch.setattr(type(task.batches), "neighbour_batches", lambda self, fold: iter(()))
    task.batches.neighbour_state(valid[0], "cuda:0")
    assert rec.states == [(None, None, 0)]
    # the reference sampler: one (seed, replica, draw) is one subgraph; the evaluation replica's is not the training one's
    _, (rowptr, col, _) = LR.graph(2)
    seeds = LR.seed_lists(2)["mixed"]
    a = LR.sample_by_hop(rowptr, col, LR.V, 2, seeds, [3, 2], 1, seed=1, replica=0x40000001)
    b = LR.sample_by_hop(rowptr, col, LR.V, 2, seeds, [3, 2], 1, seed=1, replica=0x40000001)
    training = LR.sample_by_hop(rowptr, col, LR.V, 2, seeds, [3, 2], 1, seed=1, replica=0)
    assert np.array_equal(a.nodes, b.nodes) and all(np.array_equal(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists))
    assert not (np.array_equal(a.nodes, training.nodes) and all(np.array_equal(x, y) for x, y in zip(a.adjacency_lists, training.adjacency_lists)))
    # with every fanout 0 no random word is drawn: replica and draw do not matter
    exact = [LR.sample_by_hop(rowptr, col, LR.V, 2, seeds, [0, 0], draw, seed=1, replica=r) for draw, r in ((0, 0), (5, 0x40000002))]
    assert np.array_equal(exact[0].nodes, exact[1].nodes) and all(np.array_equal(x, y) for x, y in zip(exact[0].adjacency_lists, exact[1].adjacency_lists))


def test_kept_batches_are_handed_out_again_and_released_with_the_fold(monkeypatch):
    import gc
    from tf_gnn_samples_amd.tasks import DataFold
    task = _loaded(_task(sampled_batches=dict(PLAIN, evaluation=dict(EVALUATION, keep=True))))
    rec = _Recorder(monkeypatch, task)
    valid = task._loaded_data[DataFold.VALIDATION]
    first = list(task.evaluation_batches(valid, DataFold.VALIDATION, True))
    built = len(rec.batches)
    second = list(task.evaluation_batches(valid, DataFold.VALIDATION, True))
    assert built == 5 and len(rec.batches) == built and all(a is b for a, b in zip(first, second))
    other_route = list(task.evaluation_batches(valid, DataFold.VALIDATION, False))              # another route: other batches
    assert len(rec.batches) == 2 * built and other_route[0] is not first[0]
    test = list(task.evaluation_batches(task.synthetic_test_data, DataFold.TEST, True))
    assert test[0] is not first[0] and len(task.batches.kept_evaluation) == 3
    # an iterator that is abandoned keeps nothing
    fresh = _loaded(_task(sampled_batches=dict(PLAIN, evaluation=dict(EVALUATION, keep=True))))
    _Recorder(monkeypatch, fresh)
    next(iter(fresh.evaluation_batches(fresh._loaded_data[DataFold.VALIDATION], DataFold.VALIDATION, True)))
    assert not fresh.batches.kept_evaluation
    # released with the fold
    del valid, first, second, other_route
    task._loaded_data[DataFold.VALIDATION] = None
    gc.collect()
    assert len(task.batches.kept_evaluation) == 1                                                   # the test fold's


def test_the_epoch_adds_up_to_the_fold_s_one_graph():
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    results = [{"loss": 0.5, "total_loss": 3.5, "accuracy": 3 / 7, "num_masked": 7.0, "num_correct": 3.0},
               {"loss": 1.0, "total_loss": 7.0, "accuracy": 1 / 7, "num_masked": 7.0, "num_correct": 1.0},
               {"loss": 2.0, "total_loss": 4.0, "accuracy": 1.0, "num_masked": 2.0, "num_correct": 2.0}]
    loss, res, graphs, gs, ns, es = Citation_Network_Task.sampled_evaluation_epoch((3.5 / 3, results, 3, 30.0, 300.0, 3000.0))
    assert loss == 14.5 / 16 and res is results and graphs == 1 and (gs, ns, es) == (10.0, 300.0, 3000.0)
    task = _task(sampled_batches=GOOD)
    assert task.early_stopping_metric(res, graphs) == 14.5                                   # the sum of total_loss over ONE graph
    assert task.pretty_print_epoch_task_metrics(res, graphs) == "Acc: %.2f%%" % (6 / 16 * 100)
    assert task.pretty_print_epoch_task_metrics(res[:1], 1) == "Acc: %.2f%%" % (3 / 7 * 100)      # a fold of one batch


# ---- predict(nodes=...) ----------------------------------------------------------------------------------------------------------------
def test_check_prediction_nodes():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import check_prediction_nodes
    distinct, inverse, given = check_prediction_nodes([5, 2, 9, 2, 5], 10)
    assert distinct.dtype == np.int32 and distinct.tolist() == [2, 5, 9] and inverse.tolist() == [1, 0, 2, 0, 1]
    assert given.dtype == np.int64 and given.tolist() == [5, 2, 9, 2, 5] and np.array_equal(distinct[inverse], given)
    for nodes in (np.array([3, 0], np.int32), np.array([3, 0], np.int64), (3, 0), torch.tensor([3, 0]), [np.int64(3), 0]):
        distinct, inverse, given = check_prediction_nodes(nodes, 4)
        assert distinct.tolist() == [0, 3] and inverse.tolist() == [1, 0] and given.tolist() == [3, 0]
    assert check_prediction_nodes([7], 8)[0].tolist() == [7]
    for bad, message in (([], "empty"), (np.zeros(0, np.int64), "empty"), ([1.0], "integer"), ([True], "integer"),
                         (np.array([1.0]), "int32 or int64"), (np.array([1], np.uint8), "int32 or int64"), (np.array([True]), "int32 or int64"),
                         (np.zeros((2, 2), np.int32), "one-dimensional"), (np.int64(3), "int32 or int64"), (3, "int32 or int64"),
                         ("12", "int32 or int64"), ([-1], "outside"), ([10], "outside"), (np.array([0, 2 ** 40]), "outside")):
        with pytest.raises(ValueError, match=message):
            check_prediction_nodes(bad, 10)


def test_nodes_is_validated_and_refused_on_the_host(monkeypatch):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = _loaded(_task())
    model = _cpu_model(task)
    data = task._loaded_data[DataFold.VALIDATION]
    for bad in ([], [SMALL["num_nodes"]], [-1], [0.5], np.zeros((1, 1), np.int64)):
        with pytest.raises(ValueError):
            model.predict_iter(data, nodes=bad)                                              # before the generator is made
        with pytest.raises(ValueError):
            model.predict(data, nodes=bad)
    with pytest.raises(ValueError, match="ONE graph"):
        model.predict(data + data, nodes=[1])
    # a CPU model is refused as sampled training is
    with pytest.raises(RuntimeError, match="needs a model on the GPU"):
        model.predict(data, nodes=[1, 2])
    # a model that cannot run layered batches
    with pytest.raises(ValueError, match="graph_num_timesteps_per_layer"):
        _cpu_model(task, graph_num_timesteps_per_layer=2).predict(data, nodes=[1])
    three = _loaded(_task(sampled_batches=GOOD))
    model3 = _cpu_model(three)
    monkeypatch.setitem(model3.params, "graph_num_layers", 3)                                # (the key's two fanouts against three layers)
    with pytest.raises(ValueError, match="as many fanouts as graph_num_layers"):
        model3.predict(three._loaded_data[DataFold.VALIDATION], nodes=[1])
    # the fanouts and the batch size: the key's, or zeros and 1024
    assert _task(sampled_batches=dict(PLAIN, evaluation={"fanouts": [3, 2], "seeds_per_batch": 9})).node_prediction_settings() \
        == {"fanouts": [3, 2], "seeds_per_batch": 9}
    assert task.node_prediction_settings() == {"fanouts": None, "seeds_per_batch": 1024}
    assert _task(sampled_batches=PLAIN).node_prediction_settings() == {"fanouts": None, "seeds_per_batch": 1024}
    # other tasks refuse the argument by name
    ppi = PPI_Task(PPI_Task.default_params())
    ppi.load_synthetic(3, 1, seed=2, mean_nodes=50, std_nodes=5, min_nodes=40, max_nodes=60)
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, native_batching=False)
    other = RGCN_Model(p, ppi, device="cpu")
    for call in (other.predict, other.predict_iter):
        with pytest.raises(ValueError, match="PPI"):
            call(ppi._loaded_data[DataFold.TRAIN], nodes=[0])


def test_predict_nodes_maps_duplicates_and_order_with_a_stand_in_forward(monkeypatch):
    """The plumbing without a GPU: the task's batches and the forward are stood in for.  The sampler sees distinct ascending seeds in
    runs of B with draw = the batch index; the one dict has a row per given node, in the given order."""
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    from tf_gnn_samples_amd.tasks.neighbour_sampling import PREDICT_FOLD, evaluation_replica
    task = _loaded(_task(sampled_batches=dict(PLAIN, evaluation={"fanouts": [3, 2], "seeds_per_batch": 4})))
    model = _cpu_model(task)
    rec = _Recorder(monkeypatch, task)
    monkeypatch.setattr(task, "bind_sampling_device", lambda device: None)

    def batch(state, seeds, draw, full_graph_route):
        rec.batches.append((state[1], draw, seeds.tolist(), full_graph_route))
        levels = [None, type("Level", (), {"num_targets": len(seeds)})()]
        return DeviceBatch.from_tensors(1, 50, 0, torch.zeros((50, 1)), [], torch.zeros((2, 50)), extra={"layer_graphs": levels})
    monkeypatch.setattr(task.batches, "evaluation_batch", batch)

    def stand_in(batch, training):
        seeds = torch.as_tensor(batch.extra["prediction_seeds"]).float()
        return seeds.unsqueeze(1) * torch.ones(16) / 100.0
    monkeypatch.setattr(model, "_final_node_states", stand_in)
    nodes = [17, 3, 99, 3, 40, 41, 42, 17, 0]
    out = model.predict(task._loaded_data[DataFold.VALIDATION], nodes=nodes, return_states=True)
    assert sorted(out) == ["classes", "node_states", "nodes", "probabilities"]
    assert out["nodes"].tolist() == nodes and out["nodes"].dtype == np.int64
    assert out["probabilities"].shape == (9, 4) and out["classes"].shape == (9,) and out["node_states"].shape == (9, 16)
    assert np.array_equal(out["node_states"][:, 0], np.array(nodes, np.float32) / np.float32(100.0))
    assert np.array_equal(out["probabilities"][1], out["probabilities"][3]) and np.array_equal(out["node_states"][0], out["node_states"][7])
    replica = evaluation_replica(PREDICT_FOLD)
    assert rec.batches == [(replica, 0, [0, 3, 17, 40], False), (replica, 1, [41, 42, 99], False)]
    assert rec.states == [([3, 2], PLAIN["seed"], replica)]
    # predict_iter: one (ids, [rows]) pair per batch
    pairs = list(model.predict_iter(task._loaded_data[DataFold.VALIDATION], nodes=nodes))
    assert [ids.tolist() for ids, _ in pairs] == [[0, 3, 17, 40], [41, 42, 99]]
    assert all(len(rows) == 1 and rows[0]["classes"].shape == (len(ids),) for ids, rows in pairs)
