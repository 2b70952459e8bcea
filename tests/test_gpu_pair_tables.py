"""Compact (node, type) pair tables for many-type graphs (graph.PairTables, ops.typed_linear, the bucket_row
indirection of the FiLM kernels): bit-exact index bookkeeping vs NumPy, and the FiLM layer on a VarMisuse-shaped sparse
graph against the oracle, compact path vs dense path."""
import os

import numpy as np
import pytest
import torch

from oracle import gnns as G, torch_ref as R
from helpers import degree_table, glorot, layer_norm_weights, random_relational_graph, rgcn_weights, set_switch

pytestmark = pytest.mark.gpu


def _sparse_many_type_graph(seed, V=300, L=12):
    """type 0: chain edges on all nodes, type 1: self loops; the other types touch few nodes; one type empty."""
    rng = np.random.default_rng(seed)
    adj = [np.stack([np.arange(V - 1), np.arange(1, V)], 1), np.stack([np.arange(V), np.arange(V)], 1)]
    for l in range(2, L):
        e = 0 if l == 5 else int(rng.integers(5, 80))
        nodes = rng.choice(V, size=max(2, V // 10), replace=False)
        adj.append(np.stack([rng.choice(nodes, e), rng.choice(nodes, e)], 1).reshape(-1, 2))
    adj = [a.astype(np.int32) for a in adj]
    return rng, adj, degree_table(adj, V)


def _np_side(adj, V, L, col, chunk):
    """NumPy restatement of graph.SidePairs: type-major rows, ascending node inside a type, every type's block padded
    to a multiple of `chunk` rows."""
    nonempty = np.zeros((V, L), bool)
    for l, a in enumerate(adj):
        nonempty[a[:, col], l] = True
    counts = nonempty.sum(0)
    padded = (counts + chunk - 1) // chunk * chunk
    offsets = np.concatenate([[0], np.cumsum(padded)])
    bucket_row = np.full((V, L), -1, np.int64)
    node = np.full(offsets[-1], V, np.int64)
    for l in range(L):
        nodes = np.nonzero(nonempty[:, l])[0]
        bucket_row[nodes, l] = offsets[l] + np.arange(len(nodes))
        node[offsets[l]:offsets[l] + len(nodes)] = nodes
    node_rowptr = np.concatenate([[0], np.cumsum(nonempty.sum(1))])
    node_col = bucket_row.reshape(-1)[nonempty.reshape(-1)]
    chunk_type = np.repeat(np.arange(L), padded // chunk)
    return bucket_row.reshape(-1), node, offsets, node_rowptr, node_col, chunk_type, counts


def test_pair_tables_bookkeeping_is_bit_exact(gpu_device):
    from tf_gnn_samples_amd.graph import PAIR_CHUNK, RelGraph
    rng, adj, _ = _sparse_many_type_graph(0)
    V, L = 300, 12
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    pt = g.pair_tables()
    for side, col in ((pt.tgt, 1), (pt.src, 0)):
        bucket_row, node, offsets, node_rowptr, node_col, chunk_type, counts = _np_side(adj, V, L, col, PAIR_CHUNK)
        assert np.array_equal(side.bucket_row.cpu().numpy(), bucket_row)
        assert np.array_equal(side.node.cpu().numpy(), node)
        assert side.offsets == offsets.tolist() and side.P == offsets[-1] and side.num_pairs == counts.sum()
        assert np.array_equal(side.node_rowptr.cpu().numpy(), node_rowptr)
        assert np.array_equal(side.node_col.cpu().numpy(), node_col)
        assert np.array_equal(side.chunk_type.cpu().numpy(), chunk_type)
    # message -> table row maps
    src_rows = _np_side(adj, V, L, 0, PAIR_CHUNK)[0]
    tgt_rows = _np_side(adj, V, L, 1, PAIR_CHUNK)[0]
    assert np.array_equal(pt.col_t.cpu().numpy(), src_rows[g.col_t.cpu().numpy()])
    assert np.array_equal(pt.frow_s.cpu().numpy(), tgt_rows[g.frow_s.cpu().numpy()])
    assert (pt.col_t >= 0).all() and (pt.frow_s >= 0).all()
    assert g.wants_pair_tables()                      # 12 types, most buckets empty


def test_few_type_graphs_keep_dense_tables(gpu_device):
    from tf_gnn_samples_amd.graph import RelGraph
    rng = np.random.default_rng(1)
    adj = random_relational_graph(rng, 200, 3, [2000, 300, 100])
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], 200)
    assert not g.wants_pair_tables()


@pytest.mark.parametrize("typed", ["panel", "bmm"])
def test_typed_linear_matches_per_row_matmul(gpu_device, monkeypatch, typed):
    """RELGNN_TYPED: one gathered-row MFMA launch per product (panel) | index_select + torch.bmm (bmm)."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    set_switch(monkeypatch, "RELGNN_TYPED", typed)
    rng, adj, _ = _sparse_many_type_graph(2)
    V, L, Din, Dout = 300, 12, 64, 96
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    side = g.pair_tables().src
    H = rng.standard_normal((V, Din)).astype(np.float32)
    Ws = [glorot(rng, (Din, Dout)) for _ in range(L)]
    Hd = torch.as_tensor(H, device=gpu_device).requires_grad_(True)
    Wd = [torch.as_tensor(w, device=gpu_device).requires_grad_(True) for w in Ws]
    Y = ops.typed_linear(Hd, side, Wd)
    gY = rng.standard_normal(Y.shape).astype(np.float32)
    Y.backward(torch.as_tensor(gY, device=gpu_device))
    node = side.node.cpu().numpy()
    types = np.repeat(np.arange(L), np.diff(side.offsets))
    Hz = np.concatenate([H, np.zeros((1, Din), np.float32)])          # padding rows read an all-zero input row
    ref = np.stack([Hz[n].astype(np.float64) @ Ws[t].astype(np.float64) for n, t in zip(node, types)])
    assert np.abs(Y.detach().cpu().numpy() - ref).max() < 1e-5
    assert float(Y.detach()[torch.as_tensor(node == V, device=gpu_device)].abs().max()) == 0.0
    gH = np.zeros((V + 1, Din)); gW = [np.zeros((Din, Dout)) for _ in range(L)]
    for r, (n, t) in enumerate(zip(node, types)):
        if n == V:
            continue                                                   # padding rows carry no gradient
        gH[n] += gY[r].astype(np.float64) @ Ws[t].T.astype(np.float64)
        gW[t] += np.outer(Hz[n], gY[r])
    gH = gH[:V]
    assert np.abs(Hd.grad.cpu().numpy() - gH).max() < 2e-5
    for t in range(L):
        assert np.abs(Wd[t].grad.cpu().numpy() - gW[t]).max() < 2e-5 * max(1.0, np.abs(gW[t]).max())


def test_typed_linear_odd_shape_sums_its_tile_partials_per_type(gpu_device, monkeypatch):
    """Din * Dout = 1200 is neither a multiple of 1024 nor at most 1024: the per-tile weight-gradient partials of the bmm route are
    summed per edge type by torch (ops.typed._sum_tiles_per_type's fallback), not by the gather-reduce kernel."""
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    set_switch(monkeypatch, "RELGNN_TYPED", "bmm")
    V, L, Din, Dout = 50, 3, 12, 100
    rng, adj, _ = _sparse_many_type_graph(5, V=V, L=L)
    side = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V).pair_tables().src
    H = rng.standard_normal((V, Din)).astype(np.float32)
    Ws = [glorot(rng, (Din, Dout)) for _ in range(L)]
    Wd = [torch.as_tensor(w, device=gpu_device).requires_grad_(True) for w in Ws]
    Y = ops.typed_linear(torch.as_tensor(H, device=gpu_device), side, Wd)
    gY = rng.standard_normal(Y.shape).astype(np.float32)
    Y.backward(torch.as_tensor(gY, device=gpu_device))
    node = side.node.cpu().numpy()
    types = np.repeat(np.arange(L), np.diff(side.offsets))
    real = node != V                                                   # padding rows carry no gradient
    for t in range(L):
        rows = real & (types == t)
        gW = H[node[rows]].astype(np.float64).T @ gY[rows].astype(np.float64)
        assert np.abs(Wd[t].grad.cpu().numpy() - gW).max() < 2e-5 * max(1.0, np.abs(gW).max())


def test_typed_weight_gradient_on_the_side_stream_is_the_same_bits(gpu_device):
    """bwd_overlap: the typed products' weight gradient (panel TN + per-type sum of the tile partials) runs on the side stream next to
    the input gradient — joined inside backward(), or behind it under deferred_weight_gradient_join (train_step).  Same kernels,
    same operands: the same bits as the one-stream order."""
    from tf_gnn_samples_amd import config, ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng, adj, _ = _sparse_many_type_graph(7)
    V, L, Din, Dout = 300, 12, 128, 256
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    side = g.pair_tables().tgt
    H = torch.as_tensor(rng.standard_normal((V, Din)).astype(np.float32), device=gpu_device)
    Ws = [torch.as_tensor(glorot(rng, (Din, Dout)), device=gpu_device) for _ in range(L)]
    gY = None

    def grads(overlap, deferred):
        nonlocal gY
        Hd = H.clone().requires_grad_(True)
        Wd = [w.clone().requires_grad_(True) for w in Ws]
        with config.override(bwd_overlap=overlap):
            assert ops._typed_panel_ok(Hd, side, Wd)
            Y = ops.typed_linear(Hd, side, Wd)
            if gY is None:
                gY = torch.as_tensor(rng.standard_normal(tuple(Y.shape)).astype(np.float32), device=gpu_device)
            if deferred:
                with ops.deferred_weight_gradient_join():
                    Y.backward(gY)
                ops.join_deferred()
            else:
                Y.backward(gY)
        torch.cuda.synchronize()
        return [Hd.grad.clone()] + [w.grad.clone() for w in Wd]

    want = grads("0", False)
    for overlap, deferred in (("1", False), ("1", True), ("auto", True)):
        got = grads(overlap, deferred)
        for a, b in zip(want, got):
            assert torch.equal(a, b), (overlap, deferred)
    assert float(want[1].abs().max()) > 0


@pytest.mark.parametrize("agg,norm,act,D", [("sum", False, "ReLU", 128), ("mean", True, "tanh", 64), ("sqrt_n", False, "elu", 256)])
def test_film_layer_compact_vs_oracle_and_dense(gpu_device, monkeypatch, agg, norm, act, D):
    from tf_gnn_samples_amd.gnns import sparse_gnn_film_layer
    from tf_gnn_samples_amd.graph import clear_graph_cache
    rng, adj, deg = _sparse_many_type_graph(3)
    V, L = 300, 12
    w = rgcn_weights(rng, L, D, D)
    for l in range(L):
        w["Edge_%i_FiLM_Computations/kernel" % l] = glorot(rng, (D, 2 * D))
    w.update(layer_norm_weights(D, 2, rng))
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    ref = G.sparse_gnn_film_layer(h, adj, deg, D, 2, act, agg, norm, weights=w)
    dev = lambda x: torch.as_tensor(x, device=gpu_device)
    adj_d, deg_d = [dev(a) for a in adj], dev(deg)
    outs = {}
    for flag in ("1", "0"):
        set_switch(monkeypatch, "RELGNN_PAIR_TABLES", flag)
        clear_graph_cache()
        hd = dev(h).requires_grad_(True)
        wd = {k: dev(v).requires_grad_(True) for k, v in w.items()}
        out = sparse_gnn_film_layer(hd, adj_d, deg_d, D, 2, act, agg, norm, weights=wd)
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(out.detach().cpu().numpy() - ref).max() < 1e-5 * scale, flag
        gout = np.random.default_rng(9).standard_normal(out.shape).astype(np.float32)
        out.backward(dev(gout))
        outs[flag] = (hd.grad.cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in wd.items()})
    # fp64 autograd reference for the gradients
    hr = torch.as_tensor(h, dtype=torch.float64).requires_grad_(True)
    wr = {k: torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in w.items()}
    r = R.sparse_gnn_film_layer(hr, [torch.as_tensor(a) for a in adj], torch.as_tensor(deg), D, 2, act, agg, norm, weights=wr)
    r.backward(torch.as_tensor(gout, dtype=torch.float64))
    for flag in ("1", "0"):
        gh, gw = outs[flag]
        s = max(1.0, float(hr.grad.abs().max()))
        assert np.abs(gh - hr.grad.numpy()).max() < 1e-4 * s, flag
        for k in w:
            s = max(1.0, float(wr[k].grad.abs().max()))
            assert np.abs(gw[k] - wr[k].grad.numpy()).max() < 1e-4 * s, (flag, k)


def test_film_model_trains_with_pair_tables(gpu_device, monkeypatch):
    """VarMisuse-shaped synthetic batch (23 edge types) through GNN_FiLM_Model: the compact path is picked by itself
    and gives the dense path's losses."""
    from tf_gnn_samples_amd.graph import as_rel_graph, clear_graph_cache
    from tf_gnn_samples_amd.models import name_to_model_class
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    from tf_gnn_samples_amd.tasks.synthetic import make_varmisuse_shaped_graphs
    graphs = make_varmisuse_shaped_graphs(3, seed=0, mean_nodes=300.0, std_nodes=50.0, min_nodes=100, max_nodes=500)
    losses = {}
    for flag in (None, "0"):
        if flag is None:
            set_switch(monkeypatch, "RELGNN_PAIR_TABLES", None)
        else:
            set_switch(monkeypatch, "RELGNN_PAIR_TABLES", flag)
        clear_graph_cache()
        task = PPI_Task(PPI_Task.default_params())
        task._PPI_Task__num_edge_types = 23; task._PPI_Task__initial_node_feature_size = 128; task._PPI_Task__num_labels = 1
        mb = next(task.make_minibatch_iterator(list(graphs), DataFold.VALIDATION, 10 ** 9))
        batch = DeviceBatch(mb, gpu_device)
        if flag is None:
            assert as_rel_graph(batch.adjacency_lists, batch.num_nodes).wants_pair_tables()
        cls, extra = name_to_model_class("GNN-FiLM")
        p = cls.default_params(); p.update(extra)
        p.update(hidden_size=64, graph_num_layers=3, random_seed=0)
        model = cls(p, task, device=gpu_device)
        losses[flag] = [float(model.train_step(batch)['loss'].detach()) for _ in range(4)]
    assert np.allclose(losses[None], losses["0"], rtol=2e-4, atol=1e-5), losses
    assert losses[None][-1] < losses[None][0]


@pytest.mark.parametrize("agg", ["sum", "mean", "max", "sqrt_n"])
def test_rgcn_layer_compact_vs_oracle(gpu_device, monkeypatch, agg):
    from tf_gnn_samples_amd.gnns import sparse_rgcn_layer
    from tf_gnn_samples_amd.graph import clear_graph_cache
    rng, adj, deg = _sparse_many_type_graph(5)
    V, L, D = 300, 12, 64
    w = rgcn_weights(rng, L, D, D)
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    ref = G.sparse_rgcn_layer(h, adj, deg, D, 2, "tanh", agg, True, weights=w)
    dev = lambda x: torch.as_tensor(x, device=gpu_device)
    adj_d, deg_d = [dev(a) for a in adj], dev(deg)
    grads = {}
    for flag in ("1", "0"):
        set_switch(monkeypatch, "RELGNN_PAIR_TABLES", flag)
        clear_graph_cache()
        hd = dev(h).requires_grad_(True)
        wd = {k: dev(v).requires_grad_(True) for k, v in w.items()}
        out = sparse_rgcn_layer(hd, adj_d, deg_d, D, 2, "tanh", agg, True, weights=wd)
        assert np.abs(out.detach().cpu().numpy() - ref).max() < 1e-5, flag
        gout = np.random.default_rng(1).standard_normal(out.shape).astype(np.float32)
        out.backward(dev(gout))
        grads[flag] = (hd.grad.cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in wd.items()})
    hr = torch.as_tensor(h, dtype=torch.float64).requires_grad_(True)
    wr = {k: torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in w.items()}
    r = R.sparse_rgcn_layer(hr, [torch.as_tensor(a) for a in adj], torch.as_tensor(deg), D, 2, "tanh", agg, True, weights=wr)
    r.backward(torch.as_tensor(gout, dtype=torch.float64))
    for flag in ("1", "0"):
        gh, gw = grads[flag]
        assert np.abs(gh - hr.grad.numpy()).max() < 5e-5 * max(1.0, float(hr.grad.abs().max())), flag
        for k in w:
            assert np.abs(gw[k] - wr[k].grad.numpy()).max() < 5e-5 * max(1.0, float(wr[k].grad.abs().max())), (flag, k)


@pytest.mark.parametrize("agg", ["sum", "max"])
def test_ggnn_layer_compact_vs_oracle(gpu_device, monkeypatch, agg):
    from tf_gnn_samples_amd.gnns import sparse_ggnn_layer
    from tf_gnn_samples_amd.graph import clear_graph_cache
    rng, adj, deg = _sparse_many_type_graph(6)
    V, L, D = 300, 12, 32
    w = rgcn_weights(rng, L, D, D)
    w["gru_cell/kernel"] = glorot(rng, (D, 3 * D))
    w["gru_cell/recurrent_kernel"] = glorot(rng, (D, 3 * D))
    w["gru_cell/bias"] = (0.1 * rng.standard_normal(3 * D)).astype(np.float32)
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    ref = G.sparse_ggnn_layer(h, adj, D, 2, "gru", "tanh", agg, weights=w)
    dev = lambda x: torch.as_tensor(x, device=gpu_device)
    for flag in ("1", "0"):
        set_switch(monkeypatch, "RELGNN_PAIR_TABLES", flag)
        clear_graph_cache()
        out = sparse_ggnn_layer(dev(h), [dev(a) for a in adj], D, 2, "gru", "tanh", agg, weights={k: dev(v) for k, v in w.items()})
        assert np.abs(out.cpu().numpy() - ref).max() < 1e-5, flag


@pytest.mark.parametrize("Dout", [128, 256])
def test_typed_weight_gradient_routes_agree(gpu_device, Dout):
    """config typed_tn: the per-edge-type weight gradients of ops.typed_linear from the gathered three-limb TN kernel (limb) and from
    the exact-fp32 panel TN (panel) — the FiLM layer's two products at hidden 128: [128, 128] message kernels, [128, 256] FiLM
    kernels — against float64; `auto` picks limb for the 256-column one."""
    from tf_gnn_samples_amd import config, ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng, adj, _ = _sparse_many_type_graph(5)
    V, L, Din = 300, 12, 128
    g = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V)
    side = g.pair_tables().src
    H = rng.standard_normal((V, Din)).astype(np.float32)
    Ws = [glorot(rng, (Din, Dout)) for _ in range(L)]
    gY = None
    grads = {}
    for route in ("limb", "panel", "auto"):
        with config.override(typed_tn=route):
            Hd = torch.as_tensor(H, device=gpu_device).requires_grad_(True)
            Wd = [torch.as_tensor(w, device=gpu_device).requires_grad_(True) for w in Ws]
            assert ops._typed_panel_ok(Hd, side, Wd)
            Y = ops.typed_linear(Hd, side, Wd)
            if gY is None:
                gY = torch.as_tensor(rng.standard_normal(tuple(Y.shape)).astype(np.float32), device=gpu_device)
            Y.backward(gY)
            torch.cuda.synchronize()
            grads[route] = [w.grad.detach().cpu().numpy().astype(np.float64) for w in Wd]
    node = side.node.cpu().numpy()
    types = np.repeat(np.arange(L), np.diff(side.offsets))
    Hz = np.concatenate([H, np.zeros((1, Din), np.float32)]).astype(np.float64)
    gYn = gY.cpu().numpy().astype(np.float64)
    for t in range(L):
        rows = np.nonzero((types == t) & (node != V))[0]
        want = Hz[node[rows]].T @ gYn[rows]
        scale = max(1.0, np.abs(want).max())
        for route in ("limb", "panel", "auto"):
            assert np.abs(grads[route][t] - want).max() <= 5e-6 * scale, (route, t)
        same = "limb" if Dout % 256 == 0 else "panel"
        assert np.array_equal(grads["auto"][t], grads[same][t])


def test_fill_rows_zeroes_the_listed_rows_only(gpu_device):
    """relgnn_fill_rows_f32 (the padding rows of a compact table in front of the typed weight-gradient product): the listed rows, whole,
    nothing else; a list padded with -1 is tolerated; strided rows."""
    from tf_gnn_samples_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    wide = torch.randn((300, 260), generator=g).to(gpu_device)
    X = wide[:, 4:260]                                                   # row stride 260, 256 columns
    before = wide.clone()
    rows = torch.tensor([0, 7, 299, 150, -1, -1], dtype=torch.int64, device=gpu_device)
    ops._fill_rows(X, rows, 0.0)
    torch.cuda.synchronize()
    want = before.clone()
    want[[0, 7, 299, 150], 4:260] = 0.0
    assert torch.equal(wide, want)
    ops._fill_rows(X, rows[:0], 1.0)                                     # empty list: nothing
    assert torch.equal(wide, want)
