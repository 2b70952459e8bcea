"""The device graph partitioner on the GPU (csrc/graph_partition.hip, tasks/graph_partition.py) against its NumPy restatement
(tests/graph_partition_reference.py), element for element: the wish pass alone over every row class and label count, the admission, the
whole partition on planted, hub, disconnected and degenerate graphs, the same bits twice and on a side stream; then the task: a
computed partition against the same array read from a file, restore(), the data-parallel fingerprint, and two ranks over gloo against a
one-process replay (tests/test_gpu_single_graph_dp.py's, over the case of tests/graph_partition_dp_cases.py)."""
import pickle
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import graph_partition_dp_cases as D  # noqa: E402
import graph_partition_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 5000)
SEED = 11


def _device_graph(adjacency, V, device):
    """-> (the RelGraph, its rowptr_t and col_t on the host: what the reference reads)."""
    from tf_gnn_samples_amd.graph import RelGraph
    graph = RelGraph([torch.as_tensor(np.ascontiguousarray(a), device=device) for a in adjacency], V)
    rowptr, col = graph.rowptr_t.cpu().numpy(), graph.col_t.cpu().numpy()
    want_rowptr, want_col = R.bucketing(adjacency, V)
    assert np.array_equal(rowptr, want_rowptr) and np.array_equal(col, want_col)
    return graph, rowptr, col


# ---- 1. the wish pass -----------------------------------------------------------------------------------------------------------------
def crafted_graph(V, L, seed=SEED):
    """Rows (all types together) of every length in ROW_LENGTHS at nodes drawn for them, 0 .. 11 entries elsewhere; duplicate entries
    (half of a long row's entries come from 40 nodes), 5 % self entries.  -> (adjacency lists, the nodes of the special rows)."""
    rng = np.random.default_rng([seed, V, L])
    degree = rng.integers(0, 12, size=V)
    special = rng.choice(V, len(ROW_LENGTHS), replace=False)
    degree[special] = ROW_LENGTHS
    target = np.repeat(np.arange(V), degree)
    source = rng.integers(0, V, size=len(target))
    pool = rng.choice(V, 40, replace=False)
    pooled = (degree[target] > 200) & (rng.random(len(target)) < 0.5)
    source[pooled] = pool[rng.integers(0, 40, size=int(pooled.sum()))]
    own = rng.random(len(target)) < 0.05
    source[own] = target[own]
    types = rng.integers(0, L, size=len(target))
    return [np.stack([source[types == l], target[types == l]], axis=1).astype(np.int32) for l in range(L)], special


def wish_case(V, L, P, special, seed=SEED):
    """A round's start for the crafted graph: a quarter of the nodes unassigned (every other special row among them), rooms 0, 1 or 2
    (a third of the parts are full).  -> (part int32 [V], room int32 [P])."""
    rng = np.random.default_rng([seed, V, L, P])
    part = rng.integers(0, P, size=V)
    part[rng.random(V) < 0.25] = -1
    part[special[::2]] = -1
    part[special[1::2]] = rng.integers(0, P, size=len(special[1::2]))
    room = rng.integers(0, 3, size=P).astype(np.int32)
    room[P - 1] = 2                                               # whatever was drawn: somebody has room, and with P > 2 somebody has none
    if P > 2:
        room[0] = 0
    return part.astype(np.int32), room


_CRAFTED = {}


def _crafted(V, L, device):
    if (V, L) not in _CRAFTED:
        adjacency, special = crafted_graph(V, L)
        _CRAFTED[V, L] = _device_graph(adjacency, V, device) + (special,)
    return _CRAFTED[V, L]


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("V, P", [(1100, 2), (1100, 7), (1100, 64), (1100, 65), (1100, 1000), (8300, 8192)])
def test_the_wish_pass_is_the_references_element_for_element(gpu_device, V, P, L):
    from tf_gnn_samples_amd.tasks.graph_partition import Partitioner
    graph, rowptr, col, special = _crafted(V, L, gpu_device)
    degree = np.diff(rowptr.astype(np.int64)[::L])
    assert sorted(degree[special].tolist()) == sorted(ROW_LENGTHS) and (col // L == np.repeat(np.arange(V), degree)).any()   # self entries
    rowptr_before, col_before = graph.rowptr_t.clone(), graph.col_t.clone()
    rounds = Partitioner(graph, P, seed=SEED)
    assert np.array_equal(rounds.anchors, R.anchors_of(V, P, SEED)) and rounds.cap == R.cap_of(V, P, 10)
    assert int(rounds.long_count) == int((degree > 64).sum()) >= 5
    assert rounds.long_nodes[:int(rounds.long_count)].cpu().tolist() == np.flatnonzero(degree > 64).tolist()
    part, room = wish_case(V, L, P, special)
    part_t, room_t = torch.as_tensor(part, device=gpu_device), torch.as_tensor(room, device=gpu_device)
    # the pass alone takes any anchor flags: at P close to V nearly every node is an anchor of the partition itself, so the flags
    # here name 30 nodes outside the special rows; the refine rounds are 0, 63 and every special row's first eligible one
    anchors = np.setdiff1d(np.arange(V), special)[::V // 30]
    rounds.anchor_flag = torch.zeros(V, dtype=torch.int32, device=gpu_device)
    rounds.anchor_flag[torch.as_tensor(anchors, device=gpu_device)] = 1
    by_round = np.stack([R.refine_eligible(V, r, SEED, anchors) for r in range(64)])
    assert by_round[:, special].any(axis=0).all() and not by_round[:, anchors].any()
    refine_rounds = sorted({0, 63} | {int(np.argmax(by_round[:, v])) for v in special})
    served = np.zeros(V, dtype=bool)
    for refine_round in [None] + refine_rounds:
        eligible = part < 0 if refine_round is None else by_round[refine_round]
        want = R.wishes(rowptr, col, L, part, room, eligible)
        got = rounds.wish(part_t, room_t, refine_round).cpu().numpy()
        differ = np.flatnonzero(got != want)
        assert not len(differ), "round %r: %d wishes differ, first at node %d (row of %d): %d, not %d" % (
            refine_round, len(differ), differ[0], degree[differ[0]], got[differ[0]], want[differ[0]])
        assert (want >= 0).any() and (want[eligible] < 0).any() and (got[~eligible] == -1).all()
        served |= eligible
        # the two row classes alone: each writes its own rows and leaves the others' -1
        short, long_rows = (rounds.wish(part_t, room_t, refine_round, classes=c).cpu().numpy() for c in (1, 2))
        assert np.array_equal(short, np.where(degree <= 64, want, -1)) and np.array_equal(long_rows, np.where(degree > 64, want, -1))
    assert served[special].all()                                  # every special row was somebody's eligible row
    assert torch.equal(graph.rowptr_t, rowptr_before) and torch.equal(graph.col_t, col_before)
    assert torch.equal(part_t.cpu(), torch.as_tensor(part)) and torch.equal(room_t.cpu(), torch.as_tensor(room))


# ---- 2. the admission -----------------------------------------------------------------------------------------------------------------
def test_the_admission_is_the_references(gpu_device):
    """Part 0 has no room for its three wishers; part 1 has room for exactly its three; part 2 room for three of its four: the highest
    id stays; nobody wishes part 3.  Then a round in which nobody wishes anything."""
    from tf_gnn_samples_amd.tasks.graph_partition import Partitioner
    V, P = 64, 4
    graph, *_ = _device_graph(R.planted_graph(V, 4, 0), V, gpu_device)
    rounds = Partitioner(graph, P, seed=1)
    wish = np.full(V, -1, dtype=np.int32)
    wish[[3, 5, 9]], wish[[1, 2, 40]], wish[[7, 8, 20, 63]] = 0, 1, 2
    room = np.array([0, 3, 3, 5], dtype=np.int32)
    want = R.admitted(wish, room)
    assert np.flatnonzero(want).tolist() == [1, 2, 7, 8, 20, 40]
    got = rounds.admit(torch.as_tensor(wish, device=gpu_device), torch.as_tensor(room, device=gpu_device))
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    nobody = rounds.admit(torch.full((V,), -1, dtype=torch.int32, device=gpu_device), torch.as_tensor(room, device=gpu_device))
    assert not nobody.any()
    rng = np.random.default_rng(5)                                # and a random one: every label wished by more nodes than it has room for
    wish = rng.integers(-1, P, size=V).astype(np.int32)
    got = rounds.admit(torch.as_tensor(wish, device=gpu_device), torch.as_tensor(room, device=gpu_device))
    assert np.array_equal(got.cpu().numpy(), R.admitted(wish, room))
    part = rng.integers(-1, P, size=V).astype(np.int32)           # the part sizes behind the rooms
    assert rounds.room(torch.as_tensor(part, device=gpu_device)).cpu().tolist() == (rounds.cap - R.sizes_of(part, P)).tolist()


# ---- 3. the whole partition ----------------------------------------------------------------------------------------------------------
def _both(adjacency, V, P, device, seed=0, b=10, T=8, after_round=None):
    """-> (the device's partition on the host, the reference's, the RelGraph)."""
    from tf_gnn_samples_amd.tasks.graph_partition import partition_graph
    graph, rowptr, col = _device_graph(adjacency, V, device)
    got = partition_graph(graph, P, seed=seed, imbalance_percent=b, refine_rounds=T)
    assert got.dtype == torch.int32 and tuple(got.shape) == (V,) and got.device == graph.device
    want = R.partition(rowptr, col, len(adjacency), P, seed=seed, b=b, T=T, after_round=after_round)
    return got.cpu().numpy(), want, graph


def _assert_same(got, want, P, cap):
    differ = np.flatnonzero(got != want)
    assert not len(differ), "%d of %d nodes differ, first %d: part %d, not %d" % (len(differ), len(want), differ[0], got[differ[0]], want[differ[0]])
    sizes = np.bincount(got, minlength=P)
    assert got.min() == 0 and len(sizes) == P and sizes.min() >= 1 and sizes.max() <= cap


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("V, C, P, L", [(512, 8, 8, 1), (512, 8, 16, 3), (300, 5, 7, 2)])
def test_planted_graphs_bit_for_bit(gpu_device, V, C, P, L, seed):
    from tf_gnn_samples_amd.tasks.graph_partition import partition_report
    got, want, graph = _both(R.planted_graph(V, C, seed, L), V, P, gpu_device, seed=seed)
    _assert_same(got, want, P, R.cap_of(V, P, 10))
    report = partition_report(graph, torch.as_tensor(got, device=gpu_device))
    kept, entries = R.kept_entries(graph.rowptr_t.cpu().numpy(), graph.col_t.cpu().numpy(), L, want)
    assert (report["kept_entries"], report["entries"]) == (kept, entries) and report["sizes"].dtype == np.int64
    assert report["sizes"].tolist() == np.bincount(want, minlength=P).tolist()
    assert partition_report(graph, got)["kept_entries"] == kept                            # a host array too


def test_a_hub_row_of_5000_entries_bit_for_bit(gpu_device):
    V, P = 1200, 12
    rng = np.random.default_rng(3)
    hub = np.stack([rng.integers(0, V, size=5000), np.zeros(5000, dtype=np.int64)], axis=1).astype(np.int32)
    adjacency = [np.concatenate([R.planted_graph(V, 6, 4)[0], hub])]
    got, want, graph = _both(adjacency, V, P, gpu_device, seed=4)
    assert int(graph.rowptr_t[1]) >= 5000
    _assert_same(got, want, P, R.cap_of(V, P, 10))
    # and a tight cap: rooms run out, in the hub's wishes too
    got, want, _ = _both(adjacency, V, P, gpu_device, seed=4, b=0)
    _assert_same(got, want, P, R.cap_of(V, P, 0))


def test_isolated_nodes_and_a_component_without_an_anchor_are_placed_by_the_fill(gpu_device):
    V, P, seed = 400, 6, 2
    anchors = R.anchors_of(V, P, seed)
    free = np.setdiff1d(np.arange(V), anchors)
    ring, isolated = free[5:25], free[40:52]
    apart = np.concatenate([ring, isolated])
    edges = R.planted_graph(V, 4, seed)[0]
    edges = edges[~np.isin(edges[:, 0], apart) & ~np.isin(edges[:, 1], apart)]
    around = np.stack([ring, np.roll(ring, 1)], axis=1)
    adjacency = [np.concatenate([edges, around, around[:, ::-1]]).astype(np.int32)]
    left_to_fill = []

    def after_round(phase, part):
        if phase == "grow":
            left_to_fill[:] = [np.flatnonzero(part < 0)]
    got, want, _ = _both(adjacency, V, P, gpu_device, seed=seed, after_round=after_round)
    assert set(apart.tolist()) <= set(left_to_fill[0].tolist())                          # the grow phase reached none of them
    _assert_same(got, want, P, R.cap_of(V, P, 10))


@pytest.mark.parametrize("P, T, b", [(8, 0, 10), (1, 8, 10), (1, 0, 0), (60, 8, 10), (60, 2, 100), (5, 64, 3)], ids=lambda x: str(x))
def test_degenerate_shapes_bit_for_bit(gpu_device, P, T, b):
    """No refine round; one part; P = V: every node an anchor, nobody ever eligible; the most rounds; loose and tight caps."""
    V = 60
    got, want, _ = _both(R.planted_graph(V, 3, 1, 2), V, P, gpu_device, seed=1, b=b, T=T)
    _assert_same(got, want, P, R.cap_of(V, P, b))
    if P == V:
        assert got.tolist() == list(range(V))


def test_the_same_bits_twice_and_on_a_side_stream_and_the_graph_stays_untouched(gpu_device):
    from tf_gnn_samples_amd.tasks.graph_partition import Partitioner, partition_graph
    V, P = 512, 16
    graph, rowptr, col = _device_graph(R.planted_graph(V, 8, 1, 3), V, gpu_device)
    rowptr_before, col_before = graph.rowptr_t.clone(), graph.col_t.clone()
    first = partition_graph(graph, P, seed=1)
    again = partition_graph(graph, P, seed=1)
    torch.cuda.synchronize()
    side_stream = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side_stream):
        side = partition_graph(graph, P, seed=1)
    side_stream.synchronize()
    assert torch.equal(first, again) and torch.equal(first, side)
    assert not torch.equal(first, partition_graph(graph, P, seed=2))
    assert torch.equal(graph.rowptr_t, rowptr_before) and torch.equal(graph.col_t, col_before)
    # the only read-back is the grow phase's moved count, once per round
    stats, rounds = {}, Partitioner(graph, P, seed=1)
    assert torch.equal(rounds.run(stats), first)
    assert stats["readbacks"] == stats["grow_rounds"] >= 2 and {"grow_ms", "fill_ms", "refine_ms"} <= set(stats)


def test_arguments_are_refused_before_any_launch(gpu_device):
    from tf_gnn_samples_amd.tasks.graph_partition import partition_graph
    V = 60
    graph, *_ = _device_graph(R.planted_graph(V, 3, 1), V, gpu_device)
    for bad in (dict(num_parts=0), dict(num_parts=61), dict(num_parts=4, imbalance_percent=101), dict(num_parts=4, refine_rounds=65),
                dict(num_parts=4, refine_rounds=-1), dict(num_parts=4.0), dict(num_parts=True)):
        with pytest.raises(ValueError, match="partition_graph"):
            partition_graph(graph, **bad)


# ---- 4. the task ----------------------------------------------------------------------------------------------------------------------
SYNTHETIC = dict(num_nodes=200, num_features=24, num_classes=4, num_train=60, num_valid=50, num_test=50, feature_density=0.2, seed=2)
PARTITION = {"num_parts": 12, "refine_rounds": 4}
TASK_SEED = 7


def _value(**more):
    return dict({"sampler": "parts", "parts_per_batch": 3, "seed": TASK_SEED, "normalisation": {"presample_epochs": 2}}, **more)


def _task(value):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), subgraph_batches=value))
    task.load_synthetic(**SYNTHETIC)
    return task


def _rgcn(task, device, result_dir):
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3)
    result_dir.mkdir()
    return RGCN_Model(p, task, run_id="partition", result_dir=str(result_dir), device=str(device))


def _train_one_epoch(device, result_dir, value):
    """-> (the task, the model, the bits of every batch's loss, the checkpoint's variables as bytes)."""
    task = _task(value)
    model = _rgcn(task, device, result_dir)
    record, run_epoch = [], model._run_epoch

    def recording(epoch_name, data, fold, quiet=False):
        out = run_epoch(epoch_name, data, fold, quiet)
        record.append((epoch_name, [np.float32(float(m["loss"])).tobytes() for m in out[1]]))
        return out
    model._run_epoch = recording
    try:
        model.train(quiet=True, max_epochs=1)
    finally:
        model._run_epoch = run_epoch
    torch.cuda.synchronize()
    with open(model.best_model_file, "rb") as f:
        saved = {k: np.asarray(v).tobytes() for k, v in pickle.load(f)["weights"].items()}
    return task, model, record, saved


def _train_fold(task):
    from tf_gnn_samples_amd.tasks import DataFold
    return task._loaded_data[DataFold.TRAIN][0]


def _same_batches(got, want):
    assert len(got) == len(want) == 4                             # ceil(12 / 3)
    for j, (a, b) in enumerate(zip(got, want)):
        assert (a.num_nodes, a.num_edges) == (b.num_nodes, b.num_edges), j
        assert len(a.adjacency_lists) == 2 and all(torch.equal(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists)), j
        assert torch.equal(a.extra["sampled_nodes"], b.extra["sampled_nodes"]) and torch.equal(a.extra["mask"], b.extra["mask"]), j
        assert torch.equal(a.initial_node_features, b.initial_node_features), j
        assert torch.equal(a.extra["loss_normalisation"][0], b.extra["loss_normalisation"][0]), j
        assert torch.equal(a.graph.degree_scale(a.type_to_num_incoming_edges), b.graph.degree_scale(b.type_to_num_incoming_edges)), j


def test_a_computed_partition_trains_as_the_same_array_read_from_a_file_and_restore_rebuilds_it(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.tasks.graph_partition import partition_graph
    computed = _value(partition=dict(PARTITION))
    task, model, record, saved = _train_one_epoch(gpu_device, tmp_path / "computed", computed)
    assert [len(r[1]) for r in record] == [4, 1] and (task.batches.epoch, task.batches.draw) == (1, 4)
    losses = [np.frombuffer(b, np.float32)[0] for r in record for b in r[1]]
    assert np.isfinite(losses).all() and any(x > 0 for x in losses)
    # what the plan holds is partition_graph over the TRAIN state's device RelGraph, with the parameter's seed
    plan = task.batches.subgraph_plan(_train_fold(task))
    graph = task.batches.graph_state(_train_fold(task), gpu_device).graph
    parts = partition_graph(graph, 12, seed=TASK_SEED, refine_rounds=4).cpu().numpy()
    assert plan.parts.dtype == np.int32 and np.array_equal(plan.parts, parts) and len(plan.part_nodes) == 12
    assert np.array_equal(parts, R.partition(graph.rowptr_t.cpu().numpy(), graph.col_t.cpu().numpy(), graph.L, 12, seed=TASK_SEED, T=4))
    # the file route over the saved array: the same batches, losses and checkpoint, bit for bit
    np.save(tmp_path / "parts.npy", parts)
    from_file = _value(parts_path=str(tmp_path / "parts.npy"))
    file_task, _, file_record, file_saved = _train_one_epoch(gpu_device, tmp_path / "file", from_file)
    assert file_record == record and file_saved == saved
    _same_batches(list(file_task.batches.train_batches(_train_fold(file_task))), list(task.batches.train_batches(_train_fold(task))))
    # restore(): the key comes back, no array and no file; the plan is computed again and the next epoch's batches are the run's
    restored = models.restore(model.best_model_file, str(tmp_path), device=str(gpu_device))
    assert restored.task.subgraph_batches == task.subgraph_batches and "parts_path" not in restored.task.subgraph_batches
    assert restored.task.subgraph_batches["partition"] == {"num_parts": 12, "imbalance_percent": 10, "refine_rounds": 4}
    restored.task.load_synthetic(**SYNTHETIC)
    restored.task.bind_sampling_device(gpu_device)
    rebuilt = restored.task.batches.subgraph_plan(_train_fold(restored.task))
    assert np.array_equal(rebuilt.parts, parts) and all(np.array_equal(a, b) for a, b in zip(rebuilt.part_nodes, plan.part_nodes))
    restored.task.batches.epoch, restored.task.batches.draw = task.batches.epoch, task.batches.draw
    _same_batches(list(restored.task.batches.train_batches(_train_fold(restored.task))), list(task.batches.train_batches(_train_fold(task))))


def test_a_cpu_model_is_a_value_error_and_an_unsupported_count_names_the_key(gpu_device, tmp_path):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold
    task = _task(_value(partition=dict(PARTITION)))
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, random_seed=1)
    model = RGCN_Model(p, task, device="cpu")
    with pytest.raises(ValueError, match="partition is GPU only"):
        model._batches(task._loaded_data[DataFold.TRAIN], DataFold.TRAIN)
    many = _task(_value(partition={"num_parts": 201}))            # more parts than nodes: known when the plan is built
    many.bind_sampling_device(gpu_device)
    with pytest.raises(ValueError, match="subgraph_batches: partition: .* 201 parts"):
        many.batches.subgraph_plan(_train_fold(many))


def test_the_data_parallel_fingerprint_carries_the_crc_of_the_computed_array(gpu_device):
    from tf_gnn_samples_amd.parallel import dp_check_fingerprints
    from tf_gnn_samples_amd.tasks.graph_partition import partition_graph
    prints = []
    for partition in (PARTITION, PARTITION, dict(PARTITION, refine_rounds=0)):
        task = _task(_value(partition=dict(partition), data_parallel=True))
        task.bind_sampling_device(gpu_device)
        prints.append(task.data_parallel_fingerprint())
        graph = task.batches.graph_state(_train_fold(task), gpu_device).graph
        parts = partition_graph(graph, 12, seed=TASK_SEED, refine_rounds=partition["refine_rounds"]).cpu().numpy()
        assert prints[-1]["parts_crc"] == zlib.crc32(np.ascontiguousarray(parts).tobytes())
        assert prints[-1]["subgraph_batches"]["partition"]["num_parts"] == 12
    dp_check_fingerprints(prints[:2])
    with pytest.raises(RuntimeError):
        dp_check_fingerprints(prints[1:])


# ---- 5. two ranks on one card over gloo -----------------------------------------------------------------------------------------------
def _run_two_ranks(kind, num_train, tmp_path, refusals=False):
    """tests/test_gpu_single_graph_dp.py's, with the worker that knows this file's case."""
    import test_gpu_single_graph_dp as T
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = T._free_port()
    procs = [ctx.Process(target=D.worker, args=(r, 2, port, q, kind, num_train, str(tmp_path), refusals)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=240) for _ in range(2)), key=lambda d: d["rank"])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return results


@pytest.mark.timeout(300)
def test_two_ranks_equal_a_one_process_replay(gpu_device, tmp_path, monkeypatch):
    """Two epochs of train(group=WORLD) and a test(group=WORLD) on the batches of a computed partition, four an epoch, dealt out in turn,
    every rank computing the partition itself; replayed by this process alone: the bits of every reduced gradient, variable, optimizer
    slot and reported loss."""
    import test_gpu_single_graph_dp as T
    D.register()
    monkeypatch.setattr(T, "_run_two_ranks", _run_two_ranks)
    try:
        results = T._check_two_ranks(D.KIND, D.NUM_TRAIN, gpu_device, tmp_path, batches=D.BATCHES, evaluation_batches=1)
    finally:
        T.C.TASK_PARAMS.pop(D.KIND, None)
    assert all(r["counters"] == (2, 2 * D.BATCHES) for r in results)
