"""The fused first product of an edge MLP (config edge_mlp = fused; csrc/edge_mlp_fused.hip, ops.edge_mlp_first_product):

    C[m] = out_act( in_act( P[row_src[m]] + Q[row_tgt[m]] ) @ W_type(m) )

against the composition it replaces (relgnn_pair_materialize + the 128-column panel product per type block: the same bits), against
float64, through autograd, through the two layers that use it, through whole models, and for what it exists for: the [M, Dh] hidden
tensor is neither written nor kept."""
import numpy as np
import pytest
import torch

from oracle import gnns as G, torch_ref as R
from helpers import assert_parity, degree_table, glorot, layer_norm_weights, random_relational_graph

pytestmark = pytest.mark.gpu

ACT = {"linear": 0, "tanh": 1, "relu": 2, "leaky_relu": 3, "elu": 4, "selu": 5, "gelu": 6}
V6, L6, COUNTS6 = 150, 6, (900, 300, 0, 128, 1, 129)          # type blocks: 7 panels + 4 rows, 2 + 44, none, one full, one row, 128 + 1
SENTINEL = -777.25


# ---- builders (as in tests/test_gpu_layers.py) ----------------------------------------------------------------------------------------
def _close(out, ref, tol, what=""):
    try:
        assert_parity(out, ref, strict_abs=False, what=what, tol=tol)
    except AssertionError:
        return False
    return True


def _dev(x, dev):
    if isinstance(x, dict):
        return {k: _dev(v, dev) for k, v in x.items()}
    if isinstance(x, list):
        return [_dev(v, dev) for v in x]
    return torch.as_tensor(x, device=dev)


def _graph(seed, V=150, L=3, E=(900, 150, 0)):
    """type 0: random heavy-tailed edges; type 1: self loops on every node plus some random edges (every node has >= 1 incoming
    message); type 2: empty.  Message blocks: 900, 300, 0."""
    rng = np.random.default_rng(seed)
    adj = random_relational_graph(rng, V, L, list(E))
    loops = np.stack([np.arange(V), np.arange(V)], 1).astype(np.int32)
    adj[1] = np.concatenate([loops, adj[1]]).astype(np.int32)
    return rng, adj, degree_table(adj, V)


def _grad_check(hip_fn, ref_fn, h, weights, dev, tol):
    """d(sum(out * G))/d(h, weights) for a fixed random G: HIP autograd vs fp64 torch-CPU autograd."""
    hd = torch.as_tensor(h, device=dev).requires_grad_(True)
    wd = {k: torch.as_tensor(v, device=dev).requires_grad_(True) for k, v in weights.items()}
    out = hip_fn(hd, wd)
    gout = np.random.default_rng(0).standard_normal(out.shape).astype(np.float32)
    out.backward(torch.as_tensor(gout, device=dev))
    hr = torch.as_tensor(h, dtype=torch.float64).requires_grad_(True)
    wr = {k: torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in weights.items()}
    ref = ref_fn(hr, wr)
    ref.backward(torch.as_tensor(gout, dtype=torch.float64))
    assert np.abs(out.detach().cpu().numpy() - ref.detach().numpy()).max() < tol
    pairs = [("h", hd.grad, hr.grad)] + [(k, wd[k].grad, wr[k].grad) for k in weights]
    for name, a, b in pairs:
        if b is None:
            continue
        scale = max(1.0, float(b.abs().max()))
        err = float(np.abs(a.cpu().numpy() - b.numpy()).max())
        assert err < tol * scale * 4, (name, err, scale)


LN = lambda D: layer_norm_weights(D, 2)


def _mlp_weights(rng, name, d_in, d_out, hidden, scale=1.0):
    dims = [d_in] + [d_out] * hidden + [d_out]
    names = ["dense" if i == 0 else "dense_%i" % i for i in range(hidden + 1)]
    return {"%s/%s/kernel" % (name, n): glorot(rng, (dims[i], dims[i + 1])) * np.float32(scale) for i, n in enumerate(names)}


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def _act64(name, x):
    return {"linear": lambda t: t, "elu": torch.nn.functional.elu, "relu": torch.relu, "tanh": torch.tanh,
            "gelu": torch.nn.functional.gelu}[name](x)


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the launches of the fused route: a layer that silently took the materialised route must not pass as 'fused'."""
    from tf_gnn_samples_amd import ops
    calls = []
    real = ops.edge_mlp_first_product

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "edge_mlp_first_product", counting)
    return calls


# ---- 1. the launch --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def messages(gpu_device):
    """V = 150, L = 6, random endpoints; rows of the [V*L, K] tables per message in the type-major order, and the panel table."""
    from tf_gnn_samples_amd.graph import edge_mlp_panel_table
    rng = np.random.default_rng(21)
    offs = np.concatenate([[0], np.cumsum(COUNTS6)]).tolist()
    src = np.concatenate([rng.integers(0, V6, n) for n in COUNTS6])
    tgt = np.concatenate([rng.integers(0, V6, n) for n in COUNTS6])
    typ = np.concatenate([np.full(n, l) for l, n in enumerate(COUNTS6)])
    rs = torch.as_tensor((src * L6 + typ).astype(np.int32), device=gpu_device)
    rt = torch.as_tensor((tgt * L6 + typ).astype(np.int32), device=gpu_device)
    panels = torch.as_tensor(edge_mlp_panel_table(offs), device=gpu_device)
    return offs, rs, rt, panels


def _raw_launch(in_act, out_act, P, Q, rs, rt, image, num_w, panels, C, M, N, K):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    _lib.check(lib.relgnn_edge_mlp_fwd_xf32(in_act, out_act, P.data_ptr(), P.stride(0), Q.data_ptr() if Q is not None else None,
                                            Q.stride(0) if Q is not None else 0, rs.data_ptr(), rt.data_ptr(), image.data_ptr(), num_w,
                                            panels.data_ptr(), panels.shape[0], C.data_ptr(), C.stride(0), M, N, K,
                                            _lib.current_stream()), "relgnn_edge_mlp_fwd_xf32")


def _materialize(in_act, P, Q, rs, rt, M, K):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    hidden = torch.empty((M, K), dtype=torch.float32, device=P.device)
    _lib.check(lib.relgnn_pair_materialize(in_act, _lib.ptr(P), K, _lib.ptr(Q), K, K, _lib.ptr(rs), _lib.ptr(rt), M, None,
                                           _lib.ptr(hidden), K, _lib.current_stream()), "relgnn_pair_materialize")
    return hidden


CASES = [(16, 128, True, "elu", "linear"), (16, 128, False, "relu", "elu"), (48, 128, True, "tanh", "linear"),
         (48, 128, False, "gelu", "elu"), (128, 128, True, "elu", "elu"), (128, 128, False, "linear", "linear"),
         (128, 128, True, "gelu", "linear"), (128, 256, True, "relu", "linear"), (128, 256, False, "elu", "elu"),
         (256, 256, True, "elu", "linear"), (256, 256, False, "tanh", "elu"), (256, 256, True, "linear", "elu")]


@pytest.mark.parametrize("K,N,has_q,in_act,out_act", CASES)
def test_launch_equals_materialize_then_panel_products(gpu_device, messages, K, N, has_q, in_act, out_act):
    """Bit for bit the composition (the hidden values come from the same helper, the k order and the limb-product order are those
    of the panel kernel, a row's result does not depend on its panel), float64 within the bar of the panel kernels
    (tests/test_gpu_limb_gemm.py: e <= max(3 e32, 8e-7 max(1, max|truth|))), and nothing outside [0, M) x [0, N) is written."""
    from tf_gnn_samples_amd import dense as DN
    offs, rs, rt, panels = messages
    M = offs[-1]
    P = _rand((V6 * L6, K), gpu_device, 1 + K)
    Q = _rand((V6 * L6, K), gpu_device, 2 + K) if has_q else None
    W = [_rand((K, N), gpu_device, 10 + l + N, 0.1) for l in range(L6)]
    image = DN.weight_image(W, DN.WEIGHT_NN, separate=True)
    buf = torch.full((M + 1, N + 8), SENTINEL, dtype=torch.float32, device=gpu_device)
    C = buf[:M, 4:4 + N]
    _raw_launch(ACT[in_act], ACT[out_act], P, Q, rs, rt, image.buf, L6, panels, C, M, N, K)
    torch.cuda.synchronize()
    assert bool((buf[M] == SENTINEL).all()) and bool((buf[:M, :4] == SENTINEL).all()) and bool((buf[:M, 4 + N:] == SENTINEL).all())

    hidden = _materialize(ACT[in_act], P, Q, rs, rt, M, K)
    ref = torch.full((M, N), SENTINEL, dtype=torch.float32, device=gpu_device)
    truth = torch.empty((M, N), dtype=torch.float64, device=gpu_device)
    plain = torch.empty((M, N), dtype=torch.float32, device=gpu_device)
    for l in range(L6):
        a, b = offs[l], offs[l + 1]
        if b > a:
            ref[a:b] = DN.limb_dense_sel(DN.GEMM_NN, hidden[a:b], W[l], None, ACT[out_act])
            truth[a:b] = _act64(out_act, hidden[a:b].double() @ W[l].double())
            plain[a:b] = _act64(out_act, torch.mm(hidden[a:b], W[l]))
    assert torch.equal(C, ref), float((C - ref).abs().max())
    e, e32 = float((C.double() - truth).abs().max()), float((plain.double() - truth).abs().max())
    print("K=%d N=%d e=%.3g e32=%.3g" % (K, N, e, e32))
    assert e <= max(3.0 * e32, 8e-7 * max(1.0, float(truth.abs().max()))), (e, e32)


def test_launch_refuses_what_the_kernel_does_not_take(gpu_device, messages):
    from tf_gnn_samples_amd import _lib
    offs, rs, rt, panels = messages
    M = offs[-1]
    lib = _lib.load_library()
    image = torch.zeros(L6 * int(lib.relgnn_limb_elements(256, 256)), dtype=torch.bfloat16, device=gpu_device)
    C = torch.full((M, 256), SENTINEL, dtype=torch.float32, device=gpu_device)

    def call(K, N, P=None, M_=M):
        P = torch.zeros((V6 * L6, K), dtype=torch.float32, device=gpu_device) if P is None else P
        _raw_launch(ACT["elu"], 0, P, None, rs, rt, image, L6, panels, C[:, :max(N, 4)], M_, N, K)

    assert not lib.relgnn_edge_mlp_fwd_supported(4, 0, 128, 24) and not lib.relgnn_edge_mlp_fwd_supported(4, 0, 64, 128)
    assert lib.relgnn_edge_mlp_fwd_supported(4, 0, 128, 16) and lib.relgnn_edge_mlp_fwd_supported(6, 4, 256, 1024)
    assert not lib.relgnn_edge_mlp_fwd_supported(4, 0, 128, 1040) and not lib.relgnn_edge_mlp_fwd_supported(7, 0, 128, 128)
    with pytest.raises(ValueError, match="relgnn_edge_mlp_fwd_xf32"):
        call(24, 128)
    with pytest.raises(ValueError, match="relgnn_edge_mlp_fwd_xf32"):
        call(128, 64)
    flat = torch.zeros(V6 * L6 * 128 + 4, dtype=torch.float32, device=gpu_device)
    with pytest.raises(ValueError, match="relgnn_edge_mlp_fwd_xf32"):
        call(128, 128, P=flat[1:1 + V6 * L6 * 128].view(V6 * L6, 128))            # base 4 bytes off a 16-byte boundary
    call(128, 128, M_=0)                                                         # no messages: OK, nothing launched
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())


# ---- 2. the autograd op ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_act", ["linear", "elu"])
@pytest.mark.parametrize("has_q", [True, False])
def test_first_product_gradients_against_float64(gpu_device, has_q, out_act):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import as_rel_graph
    K = N = 128
    rng = np.random.default_rng(31)
    adj = [np.stack([rng.integers(0, V6, n), rng.integers(0, V6, n)], 1).astype(np.int32) for n in COUNTS6]
    graph = as_rel_graph(_dev(adj, gpu_device), V6)
    ks = torch.as_tensor(np.concatenate([a[:, 0] * L6 + l for l, a in enumerate(adj)]).astype(np.int64))
    kt = torch.as_tensor(np.concatenate([a[:, 1] * L6 + l for l, a in enumerate(adj)]).astype(np.int64))
    offs = np.concatenate([[0], np.cumsum(COUNTS6)]).tolist()
    P0, Q0 = _rand((V6 * L6, K), "cpu", 3, 0.7), _rand((V6 * L6, K), "cpu", 4, 0.7)
    W0 = [_rand((K, N), "cpu", 50 + l, 0.1) for l in range(L6)]
    Gout = _rand((offs[-1], N), "cpu", 5)

    P = P0.to(gpu_device).requires_grad_(True)
    Q = Q0.to(gpu_device).requires_grad_(True) if has_q else None
    W = [w.to(gpu_device).requires_grad_(True) for w in W0]
    out = ops.edge_mlp_first_product(P, Q, graph, "elu", W, out_act)
    (out * Gout.to(gpu_device)).sum().backward()

    P64 = P0.double().requires_grad_(True)
    Q64 = Q0.double().requires_grad_(True) if has_q else None
    W64 = [w.double().requires_grad_(True) for w in W0]
    hid = torch.nn.functional.elu(P64[ks] + (Q64[kt] if has_q else 0.0))
    ref = _act64(out_act, torch.cat([hid[offs[l]:offs[l + 1]] @ W64[l] for l in range(L6)]))
    (ref * Gout.double()).sum().backward()

    tol = 3e-5
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < tol
    pairs = [("P", P.grad, P64.grad)] + ([("Q", Q.grad, Q64.grad)] if has_q else []) + \
            [("W%d" % l, W[l].grad, W64[l].grad) for l in range(L6)]
    for name, a, b in pairs:
        scale = max(1.0, float(b.abs().max()))
        err = float((a.cpu().double() - b).abs().max())
        assert err < 4 * tol * scale, (name, err, scale)
    assert COUNTS6[2] == 0 and W[2].grad is not None and not bool(W[2].grad.any())      # the type without messages


# ---- 3. layers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("hidden", [1, 2])
@pytest.mark.parametrize("use_target,norm,agg", [(True, False, "sum"), (True, True, "mean"), (False, False, "sum"),
                                                   (True, False, "max")])
def test_gnn_edge_mlp_layer_on_the_fused_route(gpu_device, fused_calls, D, hidden, use_target, norm, agg):
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.gnns import sparse_gnn_edge_mlp_layer
    rng, adj, deg = _graph(14)
    V, L = 150, 3
    w = dict(LN(D))
    for l in range(L):
        w.update(_mlp_weights(rng, "Edge_%i_MLP" % l, 2 * D if use_target else D, D, hidden))
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    ref = G.sparse_gnn_edge_mlp_layer(h, adj, deg, D, 2, "gelu", agg, norm, use_target, hidden, weights=w)
    adj_d, deg_d = _dev(adj, gpu_device), _dev(deg, gpu_device)
    adj_c, deg_c = [torch.as_tensor(a) for a in adj], torch.as_tensor(deg)
    with config.override(edge_mlp="fused"):
        out = sparse_gnn_edge_mlp_layer(_dev(h, gpu_device), adj_d, deg_d, D, 2, "gelu", agg, norm, use_target, hidden,
                                        weights=_dev(w, gpu_device))
        assert len(fused_calls) == 2                                        # one launch per timestep
        assert _close(out, ref, 2e-5)
        _grad_check(lambda x, ww: sparse_gnn_edge_mlp_layer(x, adj_d, deg_d, D, 1, "gelu", agg, norm, use_target, hidden, weights=ww),
                    lambda x, ww: R.sparse_gnn_edge_mlp_layer(x, adj_c, deg_c, D, 1, "gelu", agg, norm, use_target, hidden, weights=ww),
                    h, w, gpu_device, tol=3e-5)
    assert len(fused_calls) == 3


@pytest.mark.parametrize("agg", ["sum", "mean"])
def test_rgin_layer_on_the_fused_route(gpu_device, fused_calls, agg):
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.gnns import sparse_rgin_layer
    rng, adj, deg = _graph(15)
    V, L, D = 150, 3, 128
    w = dict(LN(D))
    for l in range(L):
        w.update(_mlp_weights(rng, "Edge_%i_MLP" % l, 2 * D, D, 1, 0.5))
    w.update(_mlp_weights(rng, "Aggregation_MLP", D, D, 0, 0.5))
    h = np.tanh(rng.standard_normal((V, D))).astype(np.float32)
    kw = dict(use_target_state_as_input=True, num_edge_MLP_hidden_layers=1, num_aggr_MLP_hidden_layers=0)
    ref = G.sparse_rgin_layer(h, adj, D, 2, "ReLU", agg, weights=w, **kw)
    adj_d, adj_c = _dev(adj, gpu_device), [torch.as_tensor(a) for a in adj]
    with config.override(edge_mlp="fused"):
        out = sparse_rgin_layer(_dev(h, gpu_device), adj_d, D, 2, "ReLU", agg, weights=_dev(w, gpu_device), **kw)
        assert len(fused_calls) == 2
        assert _close(out, ref, 2e-5)
        _grad_check(lambda x, ww: sparse_rgin_layer(x, adj_d, D, 1, "tanh", agg, weights=ww, **kw),
                    lambda x, ww: R.sparse_rgin_layer(x, adj_c, D, 1, "tanh", agg, weights=ww, **kw), h, w, gpu_device, tol=3e-5)
    assert len(fused_calls) == 3


# ---- 4. fallbacks ---------------------------------------------------------------------------------------------------------------------
def _layer_run(dev, D, seed=14):
    """Output and every gradient of one Edge-MLP1 layer (use_target, sum, 1 timestep) for a fixed upstream gradient."""
    from tf_gnn_samples_amd.gnns import sparse_gnn_edge_mlp_layer
    from tf_gnn_samples_amd.graph import clear_graph_cache
    clear_graph_cache()
    rng, adj, deg = _graph(seed)
    w = dict(LN(D))
    for l in range(3):
        w.update(_mlp_weights(rng, "Edge_%i_MLP" % l, 2 * D, D, 1))
    h = torch.as_tensor(np.tanh(rng.standard_normal((150, D))).astype(np.float32), device=dev).requires_grad_(True)
    wd = {k: torch.as_tensor(v, device=dev).requires_grad_(True) for k, v in w.items()}
    out = sparse_gnn_edge_mlp_layer(h, _dev(adj, dev), _dev(deg, dev), D, 1, "gelu", "sum", False, True, 1, weights=wd)
    out.backward(_rand(tuple(out.shape), dev, 9))
    torch.cuda.synchronize()
    return [out.detach(), h.grad] + [wd[k].grad for k in sorted(wd) if wd[k].grad is not None]


@pytest.mark.parametrize("D,switches", [(64, {}), (320, {}), (128, dict(gemm="lib")), (128, dict(weight_limb_cache="0"))],
                         ids=["D=64", "D=320", "gemm=lib", "weight_limb_cache=0"])
def test_what_the_kernel_does_not_take_runs_the_old_route_bit_for_bit(gpu_device, fused_calls, D, switches):
    from tf_gnn_samples_amd import config
    if config.current() != {name: config.default_of(name) for name in config.current()}:
        pytest.skip("compares against the DEFAULT settings: RELGNN_* variables are set in this run")
    base = _layer_run(gpu_device, D)
    with config.override(edge_mlp="fused", **switches):
        got = _layer_run(gpu_device, D)
    assert len(fused_calls) == 0
    assert len(got) == len(base)
    for a, b in zip(got, base):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D,has_q", [(256, True), (128, True), (128, False)])
def test_pair_materialize_gradients_are_those_of_the_raw_calls(gpu_device, D, has_q):
    """_PairMaterialize.backward moved into a helper that the fused op shares: its results are still, bit for bit, those of the raw
    calls (D > 128 with Q under the default edge_bwd: two relgnn_pair_bwd_p passes; otherwise the pre-activation gradient from
    relgnn_pair_materialize, gather-reduced by source row and by target row)."""
    from tf_gnn_samples_amd import _lib, config, ops
    from tf_gnn_samples_amd.graph import as_rel_graph
    if config.settings.edge_bwd != "auto":
        pytest.skip("written for the default edge_bwd")
    lib = _lib.load_library()
    _, adj, _ = _graph(17)
    V, L, act = 150, 3, ACT["elu"]
    graph = as_rel_graph(_dev(adj, gpu_device), V)
    M, S = graph.M, V * L
    P = _rand((S, D), gpu_device, 1).requires_grad_(True)
    Q = _rand((S, D), gpu_device, 2).requires_grad_(True) if has_q else None
    g = _rand((M, D), gpu_device, 3)
    hidden = ops.pair_materialize(P, Q, graph, "elu")
    hidden.backward(g)
    st = _lib.current_stream()
    Pd, Qd = P.detach(), (Q.detach() if has_q else None)
    if has_q and D > 128:
        gP, gQ = torch.empty_like(Pd), torch.empty_like(Qd)
        _lib.check(lib.relgnn_pair_bwd_p(act, _lib.ptr(Pd), D, _lib.ptr(Qd), D, D, _lib.ptr(graph.rowptr_s), S, _lib.ptr(graph.perm_s),
                                         _lib.ptr(graph.frow_s), None, _lib.ptr(g), D, _lib.ptr(gP), D, st), "relgnn_pair_bwd_p")
        _lib.check(lib.relgnn_pair_bwd_p(act, _lib.ptr(Qd), D, _lib.ptr(Pd), D, D, _lib.ptr(graph.rowptr_t), S, _lib.ptr(graph.perm_t),
                                         _lib.ptr(graph.col_t), None, _lib.ptr(g), D, _lib.ptr(gQ), D, st), "relgnn_pair_bwd_p")
    else:
        gpre = torch.empty_like(g)
        _lib.check(lib.relgnn_pair_materialize(act, _lib.ptr(Pd), D, _lib.ptr(Qd), D, D, _lib.ptr(graph.key_by_source),
                                               _lib.ptr(graph.key_by_target), M, _lib.ptr(g), _lib.ptr(gpre), D, st),
                   "relgnn_pair_materialize")
        gP = ops._seg_reduce_raw(_lib.AGG_SUM, gpre, graph.rowptr_s, 1, graph.perm_s, None, S)
        gQ = ops._seg_reduce_raw(_lib.AGG_SUM, gpre, graph.rowptr_t, 1, graph.perm_t, None, S) if has_q else None
    assert torch.equal(P.grad, gP)
    if has_q:
        assert torch.equal(Q.grad, gQ)


# ---- 5. models ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ppi_batch(gpu_device):
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(2, 1, seed=7, mean_nodes=200, std_nodes=30, min_nodes=80, max_nodes=300, fwd_edges_per_node=6.0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 6))
    return task, mb


def _model_step(task, mb, dev, model_name, **more):
    from tf_gnn_samples_amd.graph import clear_graph_cache
    from tf_gnn_samples_amd.models import name_to_model_class
    from tf_gnn_samples_amd.tasks import DeviceBatch
    clear_graph_cache()
    cls, extra = name_to_model_class(model_name)
    p = cls.default_params()
    p.update(extra)
    p.update(hidden_size=128, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=0, **more)
    model = cls(p, task, device=str(dev))
    batch = DeviceBatch(mb, dev)
    model.optimizer.zero_grad()
    m = model.forward_batch(batch, training=True)
    m['loss'].backward()
    torch.cuda.synchronize()
    return float(m['loss'].detach()), {n: model.variables[n].grad.detach().clone() for n in model.variables.names()}


# (RGIN's per-edge MLP exists where the target state is an input; on the source state alone its MLP runs on the nodes)
@pytest.mark.parametrize("model_name,more", [("GNN-Edge-MLP1", {}), ("RGIN", dict(use_target_state_as_input=True))],
                         ids=["GNN-Edge-MLP1", "RGIN-edge-MLP"])
def test_models_compute_the_same_step_on_the_fused_route(gpu_device, ppi_batch, fused_calls, model_name, more):
    """Loss and every gradient of one training step, fused against default, within the bars tests/test_gpu_switches.py applies to
    another arithmetic of the same step (there: why a gradient is compared against its largest entry and in Frobenius norm)."""
    from tf_gnn_samples_amd import config
    if config.current() != {name: config.default_of(name) for name in config.current()}:
        pytest.skip("compares against the DEFAULT settings: RELGNN_* variables are set in this run")
    task, mb = ppi_batch
    loss0, grads0 = _model_step(task, mb, gpu_device, model_name, **more)
    assert len(fused_calls) == 0
    with config.override(edge_mlp="fused"):
        loss, grads = _model_step(task, mb, gpu_device, model_name, **more)
    assert len(fused_calls) >= 2                                              # every layer took the fused route
    assert abs(loss - loss0) <= 2e-6 * max(1.0, abs(loss0)), (loss, loss0)
    assert set(grads) == set(grads0)
    for n, g0 in grads0.items():
        diff = (grads[n] - g0).double()
        gmax = max(float(g0.abs().max()), 1e-12)
        assert float(diff.abs().max()) <= 2e-3 * gmax, (n, float(diff.abs().max()), gmax)
        assert float(diff.norm()) <= 1e-3 * max(float(g0.double().norm()), 1e-12), (n, float(diff.norm()), float(g0.double().norm()))


# ---- 6. the hidden tensor is not kept -------------------------------------------------------------------------------------------------
def test_fused_route_keeps_one_message_tensor_less(gpu_device, fused_calls):
    """A condition, not a measurement: with the output alive and the backward pending, the default route holds exactly one
    [M, D] fp32 tensor more (the hidden states, saved by _PairMaterialize's consumer); 10 % allows for allocator rounding and the
    panel table."""
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.gnns import sparse_gnn_edge_mlp_layer
    V, L, D, counts = 20000, 3, 128, (120000, 60000, 20000)
    M = sum(counts)
    rng = np.random.default_rng(41)
    adj = [np.stack([rng.integers(0, V, n), rng.integers(0, V, n)], 1).astype(np.int32) for n in counts]
    adj_d, deg_d = _dev(adj, gpu_device), _dev(degree_table(adj, V), gpu_device)
    w = dict(layer_norm_weights(D, 1))
    for l in range(L):
        w.update(_mlp_weights(rng, "Edge_%i_MLP" % l, 2 * D, D, 1))
    wd = {k: torch.as_tensor(v, device=gpu_device).requires_grad_(True) for k, v in w.items()}
    h = torch.as_tensor(np.tanh(rng.standard_normal((V, D))).astype(np.float32), device=gpu_device).requires_grad_(True)

    def forward():
        return sparse_gnn_edge_mlp_layer(h, adj_d, deg_d, D, 1, "gelu", "sum", False, True, 1, weights=wd)

    held = {}
    for route in ("materialize", "fused"):
        with config.override(edge_mlp=route):
            forward()                                                       # fills the graph's plan caches and the image cache
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = forward()
            torch.cuda.synchronize()
            held[route] = torch.cuda.memory_allocated() - before
            del out
    assert len(fused_calls) == 2
    print("held after the forward: materialize %d, fused %d, [M, D] fp32 = %d bytes" % (held["materialize"], held["fused"], 4 * M * D))
    assert held["materialize"] - held["fused"] >= 0.9 * 4 * M * D, held


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------
def test_fused_layer_forward_replays_from_a_captured_graph(gpu_device, fused_calls):
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.gnns import sparse_gnn_edge_mlp_layer
    rng, adj, deg = _graph(14)
    V, L, D = 150, 3, 128
    w = dict(layer_norm_weights(D, 1))
    for l in range(L):
        w.update(_mlp_weights(rng, "Edge_%i_MLP" % l, 2 * D, D, 1))
    wd, adj_d, deg_d = _dev(w, gpu_device), _dev(adj, gpu_device), _dev(deg, gpu_device)
    h1 = torch.as_tensor(np.tanh(rng.standard_normal((V, D))).astype(np.float32), device=gpu_device)
    h2 = torch.as_tensor(np.tanh(rng.standard_normal((V, D))).astype(np.float32), device=gpu_device)
    static = h1.clone()

    def forward(x):
        return sparse_gnn_edge_mlp_layer(x, adj_d, deg_d, D, 1, "gelu", "sum", False, True, 1, weights=wd)

    with config.override(edge_mlp="fused"), torch.no_grad():
        forward(static)
        forward(static)                                                     # warm-up: graph plans, panel table, library handles
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = forward(static)
        static.copy_(h2)
        graph.replay()
        torch.cuda.synchronize()
        replayed = captured.clone()
        eager = forward(h2)
        torch.cuda.synchronize()
    assert len(fused_calls) == 4
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, forward(h1))
