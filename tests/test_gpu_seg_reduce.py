"""The fused gather + scale + segment-reduce HIP kernel vs the oracle.

Integer/bookkeeping: bit-exact.  Float: the kernel accumulates each segment sequentially in the
reference's message order with separately rounded mul and add, so for identical inputs the
result must EQUAL the oracle's sequential fp32 fold bit for bit; the stated north-star tolerance
(1e-5 abs) is used only where a GEMM sits in between."""
import numpy as np
import pytest
import torch

from oracle import bookkeeping, tf_ops as T
from helpers import degree_table, random_relational_graph

pytestmark = pytest.mark.gpu

AGGS = ["sum", "mean", "sqrt_n", "max"]


def _oracle_gather_reduce(X, adj, V, L, agg, w_by_msg=None):
    """reference order: type-major message list; message m gathers X[src*L + l]."""
    rows, tgts = [], []
    for l, a in enumerate(adj):
        rows.append(a[:, 0].astype(np.int64) * L + l)
        tgts.append(a[:, 1])
    rows, tgts = np.concatenate(rows), np.concatenate(tgts).astype(np.int32)
    msgs = X[rows]
    if w_by_msg is not None:
        msgs = w_by_msg[:, None] * msgs
    return T.get_aggregation_function(agg)(msgs, tgts, V)


@pytest.mark.parametrize("D", [4, 12, 32, 64, 100, 128, 256, 320, 512, 1028])
@pytest.mark.parametrize("agg", AGGS)
def test_seg_reduce_matches_oracle_bit_exact(gpu_device, D, agg):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng = np.random.default_rng(D)
    V, L = 97, 3
    adj = random_relational_graph(rng, V, L, [700, 0, 300])
    X = rng.standard_normal((V * L, D)).astype(np.float32)
    deg = degree_table(adj, V)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    Xd = torch.as_tensor(X, device=gpu_device)
    # un-weighted
    out = ops.seg_gather_reduce(Xd, g.plan_transformed(None), agg).cpu().numpy()
    np.testing.assert_array_equal(out, _oracle_gather_reduce(X, adj, V, L, agg))
    # degree-weighted (RGCN default)
    w = g.degree_scale(torch.as_tensor(deg, device=gpu_device))
    tg = np.concatenate([a[:, 1] for a in adj]); ty = np.concatenate([np.full(len(a), l) for l, a in enumerate(adj)])
    w_msg = (np.float32(1.0) / (deg[ty, tg] + np.float32(1e-7))).astype(np.float32)
    out = ops.seg_gather_reduce(Xd, g.plan_transformed(w), agg).cpu().numpy()
    np.testing.assert_array_equal(out, _oracle_gather_reduce(X, adj, V, L, agg, w_msg))


def test_seg_reduce_unaligned_and_strided_input(gpu_device):
    """D % 4 != 0 takes the scalar-lane kernel, and so does a base that is not 16-byte aligned; a row stride larger than D
    alone (stride 24, D = 16: still 16-byte aligned rows) stays on the vector kernel."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng = np.random.default_rng(5)
    V, L, D = 50, 2, 7
    adj = random_relational_graph(rng, V, L, 200)
    X = rng.standard_normal((V * L, D)).astype(np.float32)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    out = ops.seg_gather_reduce(torch.as_tensor(X, device=gpu_device), g.plan_transformed(None), "sum").cpu().numpy()
    np.testing.assert_array_equal(out, _oracle_gather_reduce(X, adj, V, L, "sum"))
    wide = torch.as_tensor(rng.standard_normal((V * L, 24)).astype(np.float32), device=gpu_device)
    view = wide[:, :16]  # stride 24, D = 16
    out = ops.seg_gather_reduce(view, g.plan_transformed(None), "sum").cpu().numpy()
    np.testing.assert_array_equal(out, _oracle_gather_reduce(wide.cpu().numpy()[:, :16].copy(), adj, V, L, "sum"))
    view = wide[:, 1:17]  # stride 24, D = 16, base 4 bytes past a 16-byte boundary
    assert view.data_ptr() % 16 != 0
    out = ops.seg_gather_reduce(view, g.plan_transformed(None), "sum").cpu().numpy()
    np.testing.assert_array_equal(out, _oracle_gather_reduce(wide.cpu().numpy()[:, 1:17].copy(), adj, V, L, "sum"))


def test_empty_segments_and_no_messages(gpu_device):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    V, L, D = 6, 2, 8
    adj = [np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)]
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    X = torch.ones((V * L, D), device=gpu_device)
    assert ops.seg_gather_reduce(X, g.plan_transformed(None), "sum").abs().max().item() == 0
    assert ops.seg_gather_reduce(X, g.plan_transformed(None), "mean").abs().max().item() == 0
    mx = ops.seg_gather_reduce(X, g.plan_transformed(None), "max").cpu().numpy()
    assert (mx == np.float32(-3.4028235e38)).all()  # float32 lowest, not -inf


@pytest.mark.parametrize("agg", AGGS)
def test_unsorted_segment_dropin(gpu_device, agg):
    """get_aggregation_function(name)(data, segment_ids, num_segments) == the TF op (oracle)."""
    from tf_gnn_samples_amd.utils import get_aggregation_function
    rng = np.random.default_rng(21)
    M, S, D = 4000, 300, 48
    data = rng.standard_normal((M, D)).astype(np.float32)
    ids = rng.integers(0, S - 20, size=M).astype(np.int32)  # last 20 segments stay empty
    fn = get_aggregation_function(agg)
    out = fn(torch.as_tensor(data, device=gpu_device), torch.as_tensor(ids, device=gpu_device), S).cpu().numpy()
    np.testing.assert_array_equal(out, T.get_aggregation_function(agg)(data, ids, S))
    # 1-D data (as used per attention head in gnns/rgat.py:126-136)
    out1 = fn(torch.as_tensor(data[:, 0].copy(), device=gpu_device), torch.as_tensor(ids, device=gpu_device), S)
    np.testing.assert_array_equal(out1.cpu().numpy(), T.get_aggregation_function(agg)(data[:, 0].copy(), ids, S))
    with pytest.raises(ValueError):
        fn(torch.as_tensor(data, device=gpu_device), torch.as_tensor(ids + S, device=gpu_device), S)


def test_unknown_aggregation_and_activation_names(gpu_device):
    from tf_gnn_samples_amd.utils import get_activation, get_aggregation_function
    with pytest.raises(ValueError, match="Unknown aggregation function"):
        get_aggregation_function("median")
    with pytest.raises(ValueError, match="Unknown activation function"):
        get_activation("swish")


@pytest.mark.parametrize("agg", AGGS)
def test_seg_reduce_gradient_matches_autograd_reference(gpu_device, agg):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    from oracle import torch_ref as R
    rng = np.random.default_rng(31)
    V, L, D = 120, 3, 64
    adj = random_relational_graph(rng, V, L, [500, 100, 0])
    deg = degree_table(adj, V)
    X = rng.standard_normal((V * L, D)).astype(np.float32)
    if agg == "max":  # force exact ties so that the equal-split rule is exercised
        X = np.round(X * 2) / 2
    gout = rng.standard_normal((V, D)).astype(np.float32)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    w = g.degree_scale(torch.as_tensor(deg, device=gpu_device)) if agg != "max" else None
    Xd = torch.as_tensor(X, device=gpu_device).requires_grad_(True)
    out = ops.seg_gather_reduce(Xd, g.plan_transformed(w), agg)
    out.backward(torch.as_tensor(gout, device=gpu_device))
    # fp64 autograd reference in the reference's op order
    Xr = torch.as_tensor(X, dtype=torch.float64).requires_grad_(True)
    rows = torch.cat([torch.as_tensor(a[:, 0].astype(np.int64) * L + l) for l, a in enumerate(adj)])
    tg = np.concatenate([a[:, 1] for a in adj]); ty = np.concatenate([np.full(len(a), l) for l, a in enumerate(adj)])
    msgs = Xr.index_select(0, rows)
    if w is not None:
        wm = 1.0 / (torch.as_tensor(deg[ty, tg], dtype=torch.float64) + 1e-7)
        msgs = wm.unsqueeze(1) * msgs
    ref = R.unsorted_segment(agg, msgs, torch.as_tensor(tg), V)
    ref.backward(torch.as_tensor(gout, dtype=torch.float64))
    nonempty = np.bincount(tg, minlength=V) > 0   # an empty max-segment is dtype-lowest: differs between fp32 and fp64
    assert np.abs(out.detach().cpu().numpy()[nonempty] - ref.detach().numpy()[nonempty]).max() < 1e-5
    scale = max(1.0, float(Xr.grad.abs().max()))
    assert np.abs(Xd.grad.cpu().numpy() - Xr.grad.numpy()).max() < 1e-5 * scale


def test_full_size_properties_c2_shape(gpu_device):
    """At the BASELINE config-2 size (~2M messages, D=256) the oracle is too slow to run per test;
    check size-independent properties instead: linearity, agreement with an fp64 reduction on a
    sample of targets, and determinism (two runs bit-identical: no atomics)."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    from tf_gnn_samples_amd.tasks import PPI_Task, DataFold
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(16, 1, seed=0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 9))
    V, L, D = mb.num_nodes, 3, 256
    assert 1.5e6 < mb.num_edges < 2.6e6
    adj = [torch.as_tensor(a, device=gpu_device) for a in mb.feed_dict['adjacency_lists']]
    g = RelGraph(adj, V)
    w = g.degree_scale(torch.as_tensor(mb.feed_dict['type_to_num_incoming_edges'], dtype=torch.float32, device=gpu_device))
    plan = g.plan_transformed(w)
    gen = torch.Generator(device=gpu_device).manual_seed(0)
    A = torch.rand((V * L, D), device=gpu_device, generator=gen) * 2 - 1
    B = torch.rand((V * L, D), device=gpu_device, generator=gen) * 2 - 1
    oa, ob = ops.seg_gather_reduce(A, plan, "sum"), ops.seg_gather_reduce(B, plan, "sum")
    oab = ops.seg_gather_reduce(A + B, plan, "sum")
    assert (oab - (oa + ob)).abs().max().item() < 1e-5          # linearity
    assert torch.equal(oa, ops.seg_gather_reduce(A, plan, "sum"))  # deterministic, bit for bit
    # mean-normalised rows are convex combinations of inputs in [-1, 1]
    assert oa.abs().max().item() <= 3.0 + 1e-5   # three edge types, each a weighted mean
    # fp64 check on 64 sampled targets
    rowptr, col = g.rowptr_t.cpu().numpy(), g.col_t.cpu().numpy()
    wn, An = w.cpu().numpy().astype(np.float64), A.cpu().numpy().astype(np.float64)
    oan = oa.cpu().numpy()
    for v in np.random.default_rng(0).integers(0, V, size=64):
        b, e = rowptr[v * L], rowptr[(v + 1) * L]
        ref = (wn[b:e, None] * An[col[b:e]]).sum(0)
        assert np.abs(oan[v] - ref).max() < 1e-5


@pytest.mark.parametrize("V,N", [(1, 1), (1000, 121), (32203, 121), (5000, 300), (257, 64)])
def test_dense_bias_gradient_column_sum(gpu_device, V, N):
    from tf_gnn_samples_amd.dense import column_sum, dense
    rng = np.random.default_rng(V + N)
    g = rng.standard_normal((V, N)).astype(np.float32)
    out = column_sum(torch.as_tensor(g, device=gpu_device)).cpu().numpy()
    ref = g.astype(np.float64).sum(0)
    assert np.abs(out - ref).max() < 1e-5 * max(1.0, np.abs(ref).max()) * 4
    # whole Dense (split-K weight gradient + bias gradient) against torch autograd in fp64
    x = rng.standard_normal((V, 48)).astype(np.float32)
    k = rng.standard_normal((48, N)).astype(np.float32) * 0.1
    b = rng.standard_normal(N).astype(np.float32)
    xd, kd, bd = [torch.as_tensor(a, device=gpu_device).requires_grad_(True) for a in (x, k, b)]
    dense(xd, kd, bd).backward(torch.as_tensor(g, device=gpu_device))
    xr, kr, br = [torch.as_tensor(a, dtype=torch.float64).requires_grad_(True) for a in (x, k, b)]
    (xr @ kr + br).backward(torch.as_tensor(g, dtype=torch.float64))
    for a, r in ((xd, xr), (kd, kr), (bd, br)):
        scale = max(1.0, float(r.grad.abs().max()))
        assert float((a.grad.cpu().double() - r.grad).abs().max()) < 2e-5 * scale


@pytest.mark.parametrize("agg", ["sum", "mean", "max", "sqrt_n"])
def test_unsorted_segment_dropin_drops_negative_ids(gpu_device, agg):
    """tf.unsorted_segment_*: rows with a negative segment id are dropped (and get a zero gradient); ids >=
    num_segments raise (TF-CPU: InvalidArgumentError)."""
    from oracle import tf_ops as T
    from tf_gnn_samples_amd.utils import get_aggregation_function
    rng = np.random.default_rng(7)
    data = rng.standard_normal((300, 20)).astype(np.float32)
    ids = rng.integers(-3, 25, size=300).astype(np.int32)
    ref = getattr(T, "unsorted_segment_" + agg)(data, ids, 25)
    x = torch.as_tensor(data, device=gpu_device).requires_grad_(True)
    out = get_aggregation_function(agg)(x, torch.as_tensor(ids, device=gpu_device), 25)
    assert out.shape == (25, 20)
    if agg in ("sum", "max"):
        np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    else:
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-6, atol=1e-6)
    out.sum().backward()
    g = x.grad.cpu().numpy()
    assert np.all(g[ids < 0] == 0.0)
    if agg != "max":                                   # max: only the arg-max rows of a segment receive gradient
        assert np.all(np.abs(g[ids >= 0]).sum(1) > 0)
    with pytest.raises(ValueError):
        get_aggregation_function(agg)(x.detach(), torch.as_tensor(np.array([0] * 299 + [25], np.int32), device=gpu_device), 25)


@pytest.mark.parametrize("D", [132, 256, 320, 512, 1024])
@pytest.mark.parametrize("agg", ["sum", "mean", "sqrt_n"])
def test_float64_bucket_accumulators_round_once(gpu_device, D, agg):
    """relgnn_seg_reduce_acc64_fwd (the bucket sums that feed the aggregate-first GEMM): w * x is exact in float64 and the
    bucket is folded in message order in float64, so the result must EQUAL the float64 sequential fold of the exact products
    rounded to float32 once — bit for bit; narrower rows are refused (the caller then keeps the float32 kernel)."""
    from tf_gnn_samples_amd import _lib, ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng = np.random.default_rng(D + len(agg))
    V, L = 211, 3
    adj = random_relational_graph(rng, V, L, [3000, 211, 1500])
    X = rng.standard_normal((V * L, D)).astype(np.float32)
    deg = degree_table(adj, V)
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    w = g.degree_scale(torch.as_tensor(deg, device=gpu_device))
    plan = g.plan_transformed(w)
    mode = ops.aggregation_mode_id(agg)
    out = ops._seg_reduce_raw(mode, torch.as_tensor(X, device=gpu_device), plan.rowptr, plan.stride, plan.col, plan.w,
                              plan.num_out, acc64=True).cpu().numpy()
    rows = np.concatenate([a[:, 0].astype(np.int64) * L + l for l, a in enumerate(adj)])
    tg = np.concatenate([a[:, 1] for a in adj]); ty = np.concatenate([np.full(len(a), l) for l, a in enumerate(adj)])
    w_msg = (np.float32(1.0) / (deg[ty, tg] + np.float32(1e-7))).astype(np.float32)
    wide = np.zeros((V, D), np.float64)
    np.add.at(wide, tg, w_msg.astype(np.float64)[:, None] * X[rows].astype(np.float64))     # in-order, exact products
    want = wide.astype(np.float32)
    n = np.maximum(np.bincount(tg, minlength=V), 1).astype(np.float32)[:, None]
    if agg == "mean":
        want = want / n
    elif agg == "sqrt_n":
        want = want / np.sqrt(n)
    np.testing.assert_array_equal(out, want)
    narrow = torch.zeros((V * L, 64), device=gpu_device)
    assert not ops.acc64_supported(64)
    np.testing.assert_array_equal(
        ops._seg_reduce_raw(_lib.AGG_SUM, narrow, plan.rowptr, plan.stride, plan.col, plan.w, plan.num_out, acc64=True).cpu().numpy(),
        np.zeros((V, 64), np.float32))
