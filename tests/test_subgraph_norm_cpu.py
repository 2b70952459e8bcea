"""GraphSAINT normalisation of the subgraph batches without a GPU: the key's validation and its way through the checkpoint metadata, the
estimator identities of tests/subgraph_norm_reference.py, exact on the pre-sampled subgraphs themselves, and three plausible wrong
restatements that break them; the model's refusals of "aggregation": true."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import subgraph_norm_reference as N  # noqa: E402

U = 2.0 ** -24
GOOD = {"roots_per_batch": 32, "walk_length": 4, "seed": 1}
R, H, SEED = 16, 3, 5


def _task(**params):
    from tf_gnn_samples_amd.tasks import Citation_Network_Task
    return Citation_Network_Task(dict(Citation_Network_Task.default_params(), **params))


# ---- 1. the parameter -----------------------------------------------------------------------------------------------------------------
def test_good_forms_and_defaults():
    from tf_gnn_samples_amd.tasks.subgraph_sampling import parse_normalisation, parse_subgraph_batches
    full = {"presample_epochs": 2, "aggregation": True, "max_edge_weight": 1e4}
    assert parse_normalisation({"presample_epochs": 2}) == full
    assert parse_normalisation({"presample_epochs": np.int64(2), "aggregation": False, "max_edge_weight": 3}) == \
        {"presample_epochs": 2, "aggregation": False, "max_edge_weight": 3.0}
    assert isinstance(parse_normalisation({"presample_epochs": 1, "max_edge_weight": np.float32(2)})["max_edge_weight"], float)
    assert _task(subgraph_batches=dict(GOOD, normalisation={"presample_epochs": 2})).subgraph_batches == dict(GOOD, normalisation=full)
    assert "normalisation" not in parse_subgraph_batches(GOOD)                            # carried only when given
    both = dict(GOOD, sparse_features=True, normalisation=full)
    assert _task(subgraph_batches=both, sparse_node_features=True).subgraph_batches == both
    assert parse_subgraph_batches(parse_subgraph_batches(both)) == both                   # the parsed form parses to itself


@pytest.mark.parametrize("bad, message", [
    (True, "must be .*got True"), ([2], r"must be .*got \[2\]"), (2, "must be .*got 2"), (None, "must be .*got None"),
    ({}, "presample_epochs is required"), ({"aggregation": True}, "presample_epochs is required"),
    ({"presample_epochs": 2, "epochs": 1}, "unknown key 'epochs'"),
    ({"presample_epochs": 0}, "presample_epochs must be an integer >= 1"), ({"presample_epochs": -1}, "presample_epochs must be"),
    ({"presample_epochs": 1.0}, "presample_epochs must be"), ({"presample_epochs": True}, "presample_epochs must be"),
    ({"presample_epochs": "2"}, "presample_epochs must be"),
    ({"presample_epochs": 2, "aggregation": 1}, "aggregation must be true or false"),
    ({"presample_epochs": 2, "aggregation": None}, "aggregation must be true or false"),
    ({"presample_epochs": 2, "max_edge_weight": 0}, "max_edge_weight must be"),
    ({"presample_epochs": 2, "max_edge_weight": -1.0}, "max_edge_weight must be"),
    ({"presample_epochs": 2, "max_edge_weight": float("nan")}, "max_edge_weight must be"),
    ({"presample_epochs": 2, "max_edge_weight": float("inf")}, "max_edge_weight must be"),
    ({"presample_epochs": 2, "max_edge_weight": "big"}, "max_edge_weight must be"),
    ({"presample_epochs": 2, "max_edge_weight": True}, "max_edge_weight must be"),
])
def test_malformed_values_are_value_errors_that_name_the_key(bad, message):
    with pytest.raises(ValueError, match="subgraph_batches: normalisation.*%s" % message):
        _task(subgraph_batches=dict(GOOD, normalisation=bad))


def _cpu_model(name, task, **params):
    from tf_gnn_samples_amd import models
    cls = getattr(models, name)
    p = cls.default_params()
    p.update(dict(hidden_size=16, graph_num_layers=1, random_seed=1), **params)
    return cls(p, task, device="cpu")


def test_the_key_travels_in_the_checkpoint_metadata(tmp_path):
    from tf_gnn_samples_amd import models
    value = dict(GOOD, normalisation={"presample_epochs": 3, "aggregation": False, "max_edge_weight": 50.0})
    task = _task(subgraph_batches=value)
    task.load_synthetic(num_nodes=120, num_features=10, num_classes=4, num_train=30, num_valid=30, num_test=30)
    assert task.get_metadata()["params"]["subgraph_batches"] == value
    model = _cpu_model("RGCN_Model", task)
    path = str(tmp_path / "model.pickle")
    model.save_model(path)
    restored = models.restore(path, str(tmp_path), device="cpu")
    assert restored.task.subgraph_batches == value and restored.task.get_metadata() == task.get_metadata()
    plain = _task()
    plain.restore_from_metadata(task.get_metadata())
    assert plain.subgraph_batches["normalisation"] == value["normalisation"]


@pytest.mark.parametrize("name, params, missing", [
    ("GGNN_Model", {}, "layers take the in-degree table"),
    ("RGAT_Model", {}, "layers take the in-degree table"),
    ("RGIN_Model", {}, "layers take the in-degree table"),
    ("RGCN_Model", {"message_aggregation_function": "mean"}, 'message_aggregation_function "sum"'),
    ("RGCN_Model", {"message_aggregation_function": "max"}, 'message_aggregation_function "sum"'),
    ("RGCN_Model", {"message_aggregation_function": "sqrt_n"}, 'message_aggregation_function "sum"'),
    ("GNN_FiLM_Model", {"normalize_messages_by_num_incoming": False}, "normalize_messages_by_num_incoming true"),
    ("GNN_Edge_MLP_Model", {}, "normalises by in-degree"),
])
def test_aggregation_weights_need_a_model_that_reads_the_degree_scale(name, params, missing):
    """The model checks the key when it is built.  (GNN-Edge-MLP: its adapter forwards no normalisation flag and the layer's default
    is off, so its layers never ask for the degree scale: the weights would be dropped silently.)"""
    def task(aggregation):
        t = _task(subgraph_batches=dict(GOOD, normalisation={"presample_epochs": 1, "aggregation": aggregation}))
        t.load_synthetic(num_nodes=100, num_features=8, num_classes=3, num_train=20, num_valid=20, num_test=20)
        return t
    with pytest.raises(ValueError, match='subgraph_batches: normalisation: "aggregation": true requires .*%s' % missing):
        _cpu_model(name, task(True), **params)
    _cpu_model(name, task(False), **params)                                              # the loss normalisation alone: every model


@pytest.mark.parametrize("name, params", [("RGCN_Model", {}), ("RGDCN_Model", {}),
                                          ("GNN_FiLM_Model", {"normalize_messages_by_num_incoming": True})])
def test_models_that_read_the_degree_scale_take_the_key(name, params):
    task = _task(subgraph_batches=dict(GOOD, normalisation={"presample_epochs": 1}))
    task.load_synthetic(num_nodes=100, num_features=8, num_classes=3, num_train=20, num_valid=20, num_test=20)
    _cpu_model(name, task, **params)


# ---- 2. the reference's own pieces ----------------------------------------------------------------------------------------------------
def test_the_reference_cuts_the_epochs_as_the_task_does():
    from tf_gnn_samples_amd.tasks.neighbour_sampling import epoch_seed_batches
    from tf_gnn_samples_amd.tasks import subgraph_sampling
    assert (subgraph_sampling.PRESAMPLE_REPLICA, subgraph_sampling.PRESAMPLE_EPOCH) == (N.PRESAMPLE_REPLICA, N.PRESAMPLE_EPOCH) \
        == (0x20000000, 0x80000000)
    mask = N.norm_graph("bucket")[2]
    for epoch in (0, 3, N.PRESAMPLE_EPOCH, N.PRESAMPLE_EPOCH + 2):
        ours, theirs = N.seed_batches(mask, R, SEED, epoch), epoch_seed_batches(mask, R, SEED, epoch)
        assert len(ours) == len(theirs) == 8 and all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(ours, theirs))


@pytest.mark.parametrize("which", ["bucket", "walk"])
def test_the_test_graphs_hold_what_the_tests_need(which):
    adjacency, (rowptr, col, _), mask = N.norm_graph(which)
    assert len(adjacency) == N.L == 3 and int(mask.sum()) == 128 and len(col) == sum(len(a) for a in adjacency)
    lengths = np.diff(rowptr.astype(np.int64))
    if which == "bucket":
        assert lengths[np.arange(len(N.LENGTHS)) * 3].tolist() == N.LENGTHS == [0, 1, 63, 64, 65, 512, 513, 5000]
        assert mask[:len(N.LENGTHS)].all()
    else:
        assert not lengths.reshape(N.V, 3)[N.NO_IN_EDGE].any() and mask[N.NO_IN_EDGE].all()


def _presampled(which, epochs):
    _, (rowptr, col, _), mask = N.norm_graph(which)
    sets = N.presampled_node_sets(rowptr, col, N.V, N.L, mask, R, H, SEED, epochs)
    return sets, N.visit_counts(rowptr, col, N.V, N.L, sets)


@pytest.mark.parametrize("which", ["bucket", "walk"])
def test_visit_counts_count_membership(which):
    _, (rowptr, col, _), mask = N.norm_graph(which)
    for epochs in (1, 3):
        sets, (node_visits, edge_visits) = _presampled(which, epochs)
        assert len(sets) == epochs * 8 and node_visits.dtype == edge_visits.dtype == np.int32
        assert node_visits.sum() == sum(len(s) for s in sets) and (node_visits[mask != 0] >= epochs).all()     # a root once per epoch
        # an entry's count is the number of induced subgraphs that list it, and never above either end's count
        listed = np.zeros(len(col), np.int64)
        for s in sets:
            for at in N.kept_positions(rowptr, col, N.V, N.L, s):
                listed[at] += 1
        assert np.array_equal(listed, edge_visits)
        target, _, source = N._positions(rowptr, col, N.V, N.L)
        assert (edge_visits <= np.minimum(node_visits[target], node_visits[source])).all()
        loops = target == source
        assert np.array_equal(edge_visits[loops], node_visits[target[loops]])
    assert (edge_visits == 0).any() and edge_visits.max() > 1


# ---- 3. the estimator identities, on the pre-sampled subgraphs themselves -------------------------------------------------------------------
def _replayed_aggregate(which, epochs, mistake=""):
    """Per by-target position the sum over the pre-sampled subgraphs of its float32 weight (float64 sum), the number of terms, and the
    counts."""
    _, (rowptr, col, _), _ = N.norm_graph(which)
    sets, (node_visits, edge_visits) = _presampled(which, epochs)
    summed, terms = np.zeros(len(col)), np.zeros(len(col), np.int64)
    for s in sets:
        at = np.concatenate(N.kept_positions(rowptr, col, N.V, N.L, s))
        w = N.edge_weights(rowptr, col, N.V, N.L, s, node_visits, edge_visits, mistake=mistake)
        assert w.dtype == np.float32 and w.shape == at.shape
        summed[at] += w.astype(np.float64)
        terms[at] += 1
    return summed, terms, node_visits, edge_visits


def _aggregate_errors(which, epochs, mistake=""):
    """Per (target, type) bucket with a visited target: |sum_b weighted aggregate / C_v - the full graph's 1/(deg + 1e-7) aggregate over
    the entries that were seen| and the bound (k + 3) * 2^-24 * sum|term|, for one random float32 value per source row."""
    _, (rowptr, col, _), _ = N.norm_graph(which)
    summed, terms, node_visits, edge_visits = _replayed_aggregate(which, epochs, mistake)
    assert np.array_equal(terms, edge_visits)
    x = np.random.default_rng(1).standard_normal(N.V * N.L).astype(np.float32).astype(np.float64)[col]
    target, typ, _ = N._positions(rowptr, col, N.V, N.L)
    row = target * N.L + typ
    deg = np.diff(rowptr.astype(np.int64))[row]
    seen = edge_visits >= 1
    c_v = np.maximum(node_visits[target], 1).astype(np.float64)
    estimate = np.bincount(row, weights=summed * x / c_v, minlength=N.V * N.L)
    full = np.bincount(row, weights=np.where(seen, x / (deg + np.float64(np.float32(1e-7))), 0.0), minlength=N.V * N.L)
    k = np.bincount(row, weights=terms, minlength=N.V * N.L)
    bound = (k + 3) * U * np.bincount(row, weights=np.abs(summed * x) / c_v, minlength=N.V * N.L)
    return np.abs(estimate - full), bound, k


@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("which", ["bucket", "walk"])
def test_the_identities_hold_on_the_presampled_subgraphs(which, epochs):
    _, (rowptr, col, _), mask = N.norm_graph(which)
    sets, (node_visits, edge_visits) = _presampled(which, epochs)
    n_sub = len(sets)
    # every train node: sum_b [v in b] * w_v / N == 1 (w_v is one float32 quotient)
    total = np.zeros(N.V)
    for s in sets:
        total[s] += N.node_weights(node_visits, s, n_sub).astype(np.float64) / n_sub
    train = mask != 0
    assert (node_visits[train] >= 1).all() and np.abs(total[train] - 1.0).max() <= U
    assert np.abs(total[node_visits >= 1] - 1.0).max() <= U
    # every entry that was seen (the default clip of 1e4 is far away): sum_b [e in b] * (C_v / C_e) / C_v == 1
    target, _, _ = N._positions(rowptr, col, N.V, N.L)
    ratio = (np.maximum(node_visits[target], 1).astype(np.float32) / np.maximum(edge_visits, 1).astype(np.float32)).astype(np.float64)
    seen = edge_visits >= 1
    assert ratio.max() < 1e4 and np.abs(edge_visits * ratio / np.maximum(node_visits[target], 1) - 1.0)[seen].max() <= U
    # hence the weighted aggregates of the replayed subgraphs add up to the full graph's aggregate over those entries
    error, bound, k = _aggregate_errors(which, epochs)
    assert (k > 0).sum() > 100 and (error <= bound).all(), float((error - bound).max())
    if which == "bucket":
        assert k[N.HUB * N.L] > 64 and bound[N.HUB * N.L] > 0                             # the hub's bucket is part of it


@pytest.mark.parametrize("mistake", ["induced_degree", "inverted"])
def test_wrong_edge_weights_land_outside_the_bound(mistake):
    for which in ("bucket", "walk"):
        error, bound, k = _aggregate_errors(which, 3, mistake)
        outside = (error > bound) & (k > 0)
        assert outside.sum() > 50, (which, int(outside.sum()))
        assert (error[outside] > 100 * bound[outside]).any()                                 # not a rounding matter


def test_node_weights_from_edge_visits_break_the_identity():
    _, (rowptr, col, _), mask = N.norm_graph("bucket")
    sets, (node_visits, edge_visits) = _presampled("bucket", 3)
    total = np.zeros(N.V)
    for s in sets:
        total[s] += N.node_weights(node_visits, s, len(sets), "from_edge_visits", rowptr, edge_visits, N.L).astype(np.float64) / len(sets)
    assert (np.abs(total[mask != 0] - 1.0) > 1e-3).sum() > 30


def test_a_clip_and_unseen_entries_are_part_of_the_weights():
    """A later batch holds entries no pre-sampled subgraph held (count 0, clamped to 1), and a clip of 2 is hit."""
    _, (rowptr, col, _), mask = N.norm_graph("bucket")
    _, (node_visits, edge_visits) = _presampled("bucket", 1)
    nodes = N.S.walk_nodes(rowptr, col, N.V, N.L, N.seed_batches(mask, R, SEED, 0)[0], H, 0, SEED, 0)
    at = np.concatenate(N.kept_positions(rowptr, col, N.V, N.L, nodes))
    assert (edge_visits[at] == 0).any()
    target, typ, _ = N._positions(rowptr, col, N.V, N.L)
    ratio = np.maximum(node_visits[target[at]], 1) / np.maximum(edge_visits[at], 1)
    assert (ratio > 2).any() and (ratio < 2).any()
    free = N.edge_weights(rowptr, col, N.V, N.L, nodes, node_visits, edge_visits)
    clipped = N.edge_weights(rowptr, col, N.V, N.L, nodes, node_visits, edge_visits, max_edge_weight=2.0)
    deg = np.diff(rowptr.astype(np.int64))[target[at] * N.L + typ[at]]
    assert np.array_equal(clipped[ratio > 2], (np.float32(2.0) * (np.float32(1.0) / (deg[ratio > 2].astype(np.float32) + np.float32(1e-7)))))
    assert np.array_equal(clipped[ratio <= 2], free[ratio <= 2]) and (clipped[ratio > 2] < free[ratio > 2]).all()


# ---- 4. the loss estimator ------------------------------------------------------------------------------------------------------------
def fixed_logits(which, classes=5):
    """Fixed "full-graph logits" and labels: the same rows whatever subgraph a node is in."""
    rng = np.random.default_rng(7 if which == "bucket" else 8)
    return (rng.standard_normal((N.V, classes)) * 3).astype(np.float32), rng.integers(0, classes, size=N.V)


@pytest.mark.parametrize("which", ["bucket", "walk"])
def test_the_weighted_batch_loss_averages_to_the_fold_s_mean_loss_and_the_plain_one_does_not(which):
    """sum_b stats[3] / N over the replayed pre-sampled subgraphs against the full-graph masked mean loss: within 1e-5 of it relative
    (the bar the head's own test holds a float32 total to; float64 is far inside), while the unweighted head's mean over the same
    batches is off by more than ten times that bar: the GPU test asserts both on these inputs."""
    _, _, mask = N.norm_graph(which)
    sets, (node_visits, _) = _presampled(which, 2)
    x, labels = fixed_logits(which)
    n_train = float(mask.sum())
    full = float((N.row_losses(x, labels) * mask).sum() / n_train)
    weighted = plain = 0.0
    for s in sets:
        m = mask[s]
        stats, _ = N.weighted_stats(x[s], labels[s], m, N.node_weights(node_visits, s, len(sets)), n_train)
        weighted += stats[3] / len(sets)
        ones, _ = N.weighted_stats(x[s], labels[s], m, np.ones(len(s), np.float32), float(m.sum()))
        plain += ones[3] / len(sets)
    bar = 1e-5 * full
    print("%s: full %.9g weighted %.9g plain %.9g bar %.3g" % (which, full, weighted, plain, bar))
    assert abs(weighted - full) <= bar
    assert abs(plain - full) > 10 * bar


def test_weighted_stats_and_gradient_reduce_to_the_plain_head():
    rng = np.random.default_rng(2)
    x, labels = (rng.standard_normal((40, 7)) * 3).astype(np.float32), rng.integers(0, 7, size=40)
    mask = (rng.random(40) < 0.5).astype(np.float32)
    stats, scale = N.weighted_stats(x, labels, mask, np.ones(40, np.float32), mask.sum())
    losses = N.row_losses(x, labels)
    assert stats[0] == float((losses * mask).sum()) == scale and stats[5] == stats[1] == mask.sum()
    assert stats[3] == stats[0] / mask.sum()
    doubled, _ = N.weighted_stats(x, labels, mask, np.full(40, 2.0, np.float32), mask.sum())
    assert doubled[0] == 2 * stats[0] and doubled[1:3] == stats[1:3] and doubled[4] == stats[4] and doubled[5] == 2 * stats[5]
    # the gradient is the derivative of stats[3] * g_loss + stats[0] * g_total: a central difference in float64
    weights = (2.0 ** rng.integers(-3, 4, size=40)).astype(np.float32)
    grad = N.weighted_gradient(x, labels, mask, weights, 17.0, 0.7, -0.25)
    assert not grad[mask == 0].any()
    value = lambda z: (lambda s: 0.7 * s[3] - 0.25 * s[0])(N.weighted_stats(z, labels, mask, weights, 17.0)[0])
    for r, c in ((int(np.flatnonzero(mask)[0]), 3), (int(np.flatnonzero(mask)[-1]), 0)):
        step = np.zeros_like(x, dtype=np.float64)
        step[r, c] = 1e-3
        lo, hi = (x.astype(np.float64) - step), (x.astype(np.float64) + step)
        numeric = (value(hi) - value(lo)) / 2e-3
        assert abs(numeric - grad[r, c]) <= 1e-5 * max(1.0, abs(grad[r, c]))
