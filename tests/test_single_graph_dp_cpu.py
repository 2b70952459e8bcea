"""Data-parallel training on the sampled batches of ONE graph (the citation task's key "data_parallel"), everything that runs without
a GPU: the key, the host schedule (parallel.single_graph_schedule), the fingerprint comparison and the reordering of what the
ranks gather."""
import numpy as np
import pytest

SAMPLED = {"fanouts": [3, 3], "seeds_per_batch": 16, "seed": 1}
SUBGRAPH = {"roots_per_batch": 16, "walk_length": 2, "seed": 1}


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parameter, good", [("sampled_batches", SAMPLED), ("subgraph_batches", SUBGRAPH)])
def test_the_key_is_a_bool_carried_only_when_given(parameter, good):
    for bad in (1, "true", None, [True]):
        with pytest.raises(ValueError, match="%s: data_parallel must be true or false" % parameter):
            _task(**{parameter: dict(good, data_parallel=bad)})
    assert "data_parallel" not in getattr(_task(**{parameter: good}), parameter)
    assert not _task(**{parameter: good}).single_graph_data_parallel()
    assert not _task(**{parameter: dict(good, data_parallel=False)}).single_graph_data_parallel()
    with_key = _task(**{parameter: dict(good, data_parallel=True)})
    assert getattr(with_key, parameter)["data_parallel"] is True and with_key.single_graph_data_parallel()
    assert not _task().single_graph_data_parallel()


def test_the_hook_defaults_to_false_on_every_other_task():
    from tf_gnn_samples_amd.tasks import PPI_Task, QM9_Task, Sparse_Graph_Task
    assert Sparse_Graph_Task({}).single_graph_data_parallel() is False
    assert PPI_Task(PPI_Task.default_params()).single_graph_data_parallel() is False
    assert QM9_Task(QM9_Task.default_params()).single_graph_data_parallel() is False


@pytest.mark.parametrize("parameter, good", [("sampled_batches", dict(SAMPLED, layered=True, evaluation={"fanouts": [0, 0], "seeds_per_batch": 64})),
                                             ("subgraph_batches", dict(SUBGRAPH, normalisation={"presample_epochs": 2}))])
def test_the_key_is_kept_in_checkpoint_metadata_and_restored(tmp_path, parameter, good):
    from tf_gnn_samples_amd import models
    given = dict(good, data_parallel=True)
    task = _task(**{parameter: given})
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    assert task.get_metadata()["params"][parameter] == given
    p = models.RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=2, random_seed=1)
    model = models.RGCN_Model(p, task, device="cpu")
    path = str(tmp_path / "model.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.single_graph_data_parallel() and getattr(restored.task, parameter)["data_parallel"] is True
    assert restored.task.get_metadata() == task.get_metadata()
    plain = _task()
    assert not plain.single_graph_data_parallel()
    plain.restore_from_metadata(task.get_metadata())
    assert plain.single_graph_data_parallel()


@pytest.mark.parametrize("keys", [("sparse_update",), ("sparse_update", "sparse_gradient")])
def test_the_row_deferred_update_and_the_compact_gradient_are_refused_with_the_key(keys):
    sampled = dict(SAMPLED, sparse_features=True, data_parallel=True, **{key: True for key in keys})
    with pytest.raises(ValueError) as refusal:
        _task(sampled_batches=sampled, sparse_node_features=True)
    assert '"data_parallel": true' in str(refusal.value) and all('"%s": true' % key in str(refusal.value) for key in keys)
    # each of them alone stays what it was, and "sparse_features" composes with the key
    _task(sampled_batches=dict(sampled, data_parallel=False), sparse_node_features=True)
    assert _task(sampled_batches=dict(SAMPLED, sparse_features=True, data_parallel=True), sparse_node_features=True).single_graph_data_parallel()


class _Model:
    """What data_parallel() reads of a model in front of its device check."""

    def __init__(self, task):
        import torch
        self.task, self.device, self.params = task, torch.device("cpu"), {}


def test_without_the_key_everything_stays_refused_and_with_it_a_cpu_model_and_the_iterators_do(monkeypatch):
    import torch.distributed as dist
    from tf_gnn_samples_amd.models.data_parallel import data_parallel
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    with pytest.raises(RuntimeError, match="cannot be split by graph"):
        Citation_Network_Task(Citation_Network_Task.default_params()).loss_weight(1, 2708)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    group = object()
    for params in ({}, {"sampled_batches": SAMPLED}, {"subgraph_batches": SUBGRAPH}, {"sampled_batches": dict(SAMPLED, data_parallel=False)}):
        with pytest.raises(RuntimeError, match="cannot be split by graph across ranks; run it on a single GPU"):
            data_parallel(_Model(_task(**params)), group)
    for params in ({"sampled_batches": dict(SAMPLED, data_parallel=True)}, {"subgraph_batches": dict(SUBGRAPH, data_parallel=True)}):
        task = _task(**params)
        with pytest.raises(RuntimeError, match="cannot be split by graph"):      # (the hook is asked first: loss_weight still raises)
            task.loss_weight(1, 1)
        with pytest.raises(RuntimeError, match="need the model on the GPU"):
            data_parallel(_Model(task), group)
        task.load_synthetic(num_nodes=100, num_features=8, num_classes=3, num_train=20, num_valid=20, num_test=20)
        with pytest.raises(RuntimeError, match="cannot be split by graph"):      # the driver does not use the task's iterators
            list(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN, 100))
        with pytest.raises(RuntimeError, match="cannot be split by graph"):
            list(task.make_native_minibatch_iterator(None, DataFold.TRAIN, 100))


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("sizes", [[16, 16, 16, 6], [16, 16, 16, 16, 6], [16]], ids=["four", "five", "fewer_than_ranks"])
def test_schedule_deals_every_batch_once_with_its_share_of_the_step(sizes, world):
    from tf_gnn_samples_amd.parallel import single_graph_schedule
    nb = len(sizes)
    for epoch in (0, 1):
        s = single_graph_schedule(sizes, world, epoch)
        assert s.steps == -(-nb // world) and s.scales.dtype == np.float32 and s.scales.shape == (world, s.steps)
        assert s.owner.tolist() == [j % world for j in range(nb)] and s.step.tolist() == [j // world for j in range(nb)]
        assert s.draws.tolist() == list(range(epoch * nb, (epoch + 1) * nb))
        slots = sorted(zip(s.step.tolist(), s.owner.tolist()))
        assert slots == sorted(set(slots)) and len(slots) == nb                     # every batch exactly once, no slot twice
        taken = np.zeros((world, s.steps), dtype=bool)
        for j in range(nb):
            step_sizes = [sizes[i] for i in range(nb) if i // world == j // world]
            assert s.scales[j % world, j // world] == np.float32(sizes[j] / sum(step_sizes))      # by hand: the quotient in double, rounded once
            taken[j % world, j // world] = True
        assert (s.scales[~taken] == 0).all() and int((~taken).sum()) == world * s.steps - nb         # the empty slots
        for k in range(s.steps):
            total = np.float32(0)
            for r in range(world):
                total = np.float32(total + s.scales[r, k])
            assert total == np.float32(1)                                             # in float32, added in rank order


def test_schedule_pairs_sixteen_seeds_with_six_and_leaves_a_rank_without_a_batch():
    """The two steps tests/test_gpu_single_graph_dp.py runs on two ranks: n_train = 54 and n_train = 70 with B = 16."""
    from tf_gnn_samples_amd.parallel import single_graph_schedule
    from tf_gnn_samples_amd.tasks.neighbour_sampling import epoch_seed_batches
    mask = np.zeros(600, np.float32)
    mask[:54] = 1
    sizes = [len(b) for b in epoch_seed_batches(mask, 16, 1, 0)]
    assert sizes == [16, 16, 16, 6]
    s = single_graph_schedule(sizes, 2)
    assert s.scales[:, 1].tolist() == [np.float32(16 / 22), np.float32(6 / 22)]
    mask[:70] = 1
    sizes = [len(b) for b in epoch_seed_batches(mask, 16, 1, 0)]
    assert sizes == [16, 16, 16, 16, 6]
    s = single_graph_schedule(sizes, 2)
    assert s.steps == 3 and s.scales[:, 2].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("normalisation", [None, {"presample_epochs": 2}])
def test_subgraph_batches_of_a_step_weigh_the_same_and_sampled_batches_by_their_seeds(normalisation):
    from tf_gnn_samples_amd.parallel import single_graph_schedule
    from tf_gnn_samples_amd.tasks import DataFold
    subgraph = dict(SUBGRAPH, data_parallel=True, **({} if normalisation is None else {"normalisation": normalisation}))
    task = _task(subgraph_batches=subgraph)
    task.load_synthetic(num_nodes=600, num_features=16, num_classes=4, num_train=54, num_valid=100, num_test=100)
    train = task._loaded_data[DataFold.TRAIN]
    assert task.batches.train_batch_weights(train[0]) == [1.0] * 4
    s = task.train_schedule(train, 2)
    assert s.scales.tolist() == [[0.5, 0.5], [0.5, 0.5]] and s.draws.tolist() == [0, 1, 2, 3]
    assert single_graph_schedule([1.0] * 5, 2).scales.tolist() == [[0.5, 0.5, 1.0], [0.5, 0.5, 0.0]]
    sampled = _task(sampled_batches=dict(SAMPLED, data_parallel=True))
    sampled.load_synthetic(num_nodes=600, num_features=16, num_classes=4, num_train=54, num_valid=100, num_test=100)
    assert sampled.batches.train_batch_weights(sampled._loaded_data[DataFold.TRAIN][0]) == [16.0, 16.0, 16.0, 6.0]
    sampled.batches.epoch = 1                                  # the next epoch's schedule: its draws follow the first epoch's
    assert sampled.train_schedule(sampled._loaded_data[DataFold.TRAIN], 2).draws.tolist() == [4, 5, 6, 7]


# ---- the fingerprint ---------------------------------------------------------------------------------------------------------------------
def _loaded(num_train=54, seed=0, **sampled):
    task = _task(sampled_batches=dict(SAMPLED, data_parallel=True, **sampled))
    task.load_synthetic(num_nodes=600, num_features=16, num_classes=4, num_train=num_train, num_valid=100, num_test=100, seed=seed)
    return task


def test_fingerprints_that_differ_raise_and_name_the_field():
    from tf_gnn_samples_amd.parallel import dp_check_fingerprints
    mine = _loaded().data_parallel_fingerprint()
    assert mine["nodes"] == 600 and mine["train_nodes"] == 54 and mine["validation_nodes"] == 100 and len(mine["edges_per_type"]) == 2
    assert mine["sampled_batches"] == dict(SAMPLED, data_parallel=True) and mine["subgraph_batches"] is None
    dp_check_fingerprints([mine, _loaded().data_parallel_fingerprint(), dict(mine)])
    for other, fields in ((_loaded(num_train=70), ["train_mask_crc", "train_nodes"]), (_loaded(seed=1), ["edges_per_type"]),
                          (_loaded(layered=True), ["sampled_batches"])):
        with pytest.raises(RuntimeError) as refusal:
            dp_check_fingerprints([mine, mine, other.data_parallel_fingerprint()])
        assert "rank 2" in str(refusal.value) and all(field in str(refusal.value) for field in fields), str(refusal.value)
    # the same size, other nodes in the fold: only the CRC sees it
    moved = dict(mine, train_mask_crc=mine["train_mask_crc"] ^ 1)
    with pytest.raises(RuntimeError, match=r"differ in train_mask_crc \(rank 0: \d+, rank 1: \d+\)$"):
        dp_check_fingerprints([mine, moved])


# ---- the reordering ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world, total", [(2, 4), (2, 5), (3, 5), (4, 2), (3, 0), (1, 3)])
def test_what_the_ranks_hold_comes_back_in_batch_order(world, total):
    from tf_gnn_samples_amd.parallel import dp_order_by_batch
    per_rank = [[{"batch": j} for j in range(r, total, world)] for r in range(world)]
    assert dp_order_by_batch(per_rank) == [{"batch": j} for j in range(total)]


def test_lists_that_were_not_dealt_in_turn_are_refused():
    from tf_gnn_samples_amd.parallel import dp_order_by_batch
    with pytest.raises(ValueError, match="rank 0 holds 2 of 5 batches dealt out in turn to 2 ranks, not 3"):
        dp_order_by_batch([[0, 2], [1, 3, 4]])
