"""weight_grad_stream.fork through its users: every mode of this tree — bwd_overlap 0 (one stream), 1 joined inside backward(), 1
with the join deferred behind the backward (train_step) — launches the same kernels on the same operands, so the gradients are the
same bits; and exactly the backward nodes that may go aside do (one _DEFER["pending"] entry each)."""
import numpy as np
import pytest
import torch

from helpers import glorot, random_relational_graph
from test_gpu_pair_tables import _sparse_many_type_graph

pytestmark = pytest.mark.gpu

MODES = (("0", False), ("1", False), ("1", True))


def _backward(out, gout, overlap, deferred):
    """The backward of `out` (a tensor or several) in one mode -> the number of pending joins the deferred pass left (None when not
    deferred)."""
    from tf_gnn_samples_amd import config, ops, weight_grad_stream
    pending = None
    with config.override(bwd_overlap=overlap):
        if deferred:
            with ops.deferred_weight_gradient_join():
                torch.autograd.backward(out, gout)
            pending = len(weight_grad_stream._DEFER["pending"])
            ops.join_deferred()
            assert not weight_grad_stream._DEFER["pending"] and not weight_grad_stream._DEFER["targets"] and not weight_grad_stream._DEFER["handed"]
        else:
            torch.autograd.backward(out, gout)
    torch.cuda.synchronize()
    return pending


def _same_bits(want, got, what):
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (what, i)


def test_typed_linear_pair_is_the_same_bits_in_every_mode(gpu_device):
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.graph import RelGraph
    rng, adj, _ = _sparse_many_type_graph(7)
    V, L, Din, Dout = 300, 12, 128, 256
    pairs = RelGraph([torch.as_tensor(a, device=gpu_device) for a in adj], V).pair_tables()
    H = torch.as_tensor(rng.standard_normal((V, Din)).astype(np.float32), device=gpu_device)
    Ws = [torch.as_tensor(glorot(rng, (Din, Dout)), device=gpu_device) for _ in range(2 * L)]
    gYs = None
    results = []
    for overlap, deferred in MODES:
        Hd = H.clone().requires_grad_(True)
        Wd = [w.clone().requires_grad_(True) for w in Ws]
        Ya, Yb = ops.typed_linear_pair(Hd, pairs, Wd[:L], Wd[L:])
        assert type(Ya.grad_fn).__name__ == "_TypedLinearPanelBackward" and Yb.grad_fn is Ya.grad_fn
        if gYs is None:
            gYs = [torch.as_tensor(rng.standard_normal(tuple(Y.shape)).astype(np.float32), device=gpu_device) for Y in (Ya, Yb)]
        pending = _backward([Ya, Yb], gYs, overlap, deferred)
        assert pending == (1 if deferred else None)
        results.append([Ya.detach(), Yb.detach(), Hd.grad] + [w.grad for w in Wd])
    assert len(results[0]) == 3 + 24 and all(float(results[0][i].abs().max()) > 0 for i in (2, 3, 3 + L))
    for got, mode in zip(results[1:], MODES[1:]):
        _same_bits(results[0], got, mode)


def _aggregate_case(dev, seed):
    from tf_gnn_samples_amd.graph import RelGraph
    rng = np.random.default_rng(seed)
    V, L, D = 4200, 3, 256                           # the smallest height on the limb route (4096 rows), not a multiple of a tile
    adj = random_relational_graph(rng, V, L, [40000, 4000, 20000])
    g = RelGraph([torch.as_tensor(a, device=dev) for a in adj], V)
    H = torch.as_tensor(rng.standard_normal((V, D)).astype(np.float32), device=dev)
    Ws = [torch.as_tensor((rng.standard_normal((D, D)) * 0.05).astype(np.float32), device=dev) for _ in range(L)]
    gout = torch.as_tensor(rng.standard_normal((V, D)).astype(np.float32), device=dev)
    return g, H, Ws, gout


def test_aggregate_then_transform_with_a_side_stream_intermediate_is_the_same_bits_in_every_mode(gpu_device):
    """mean aggregation: the scaled gradient gout * f is allocated inside run(), i.e. on the side stream — the caching allocator must
    not hand it (or the gradients) out early: ten rounds with fresh tensors and churn between them."""
    from tf_gnn_samples_amd import ops
    g, H0, W0, gout = _aggregate_case(gpu_device, 11)

    def grads(overlap, deferred):
        H = H0.clone().requires_grad_(True)
        Ws = [w.clone().requires_grad_(True) for w in W0]
        out = ops.aggregate_then_transform(H, Ws, g, None, "mean", "tanh")
        pending = _backward(out, gout, overlap, deferred)
        assert pending == (1 if deferred else None)
        return [out.detach().clone(), H.grad.clone()] + [w.grad.clone() for w in Ws]

    want = grads(*MODES[0])
    assert all(float(t.abs().max()) > 0 for t in want)
    for _ in range(10):
        for mode in MODES[1:]:
            _same_bits(want, grads(*mode), mode)
        junk = [torch.empty((4200, 256), device=gpu_device).normal_() for _ in range(3)]      # churn the allocator between rounds
        del junk


def test_kernels_shared_by_two_aggregate_then_transform_calls_go_aside_once(gpu_device):
    """The shared weights of a second timestep: the backward sees the kernels twice, the second sight stays on the main stream (and
    makes it wait for the first), the two contributions are summed there in the one-stream order."""
    from tf_gnn_samples_amd import ops, weight_grad_stream
    g, H0, W0, gout = _aggregate_case(gpu_device, 12)

    def grads(overlap, deferred):
        H = H0.clone().requires_grad_(True)
        Ws = [w.clone().requires_grad_(True) for w in W0]
        out = ops.aggregate_then_transform(ops.aggregate_then_transform(H, Ws, g, None, "mean", "tanh"), Ws, g, None, "mean", "tanh")
        pending = _backward(out, gout, overlap, deferred)
        return pending, [out.detach().clone(), H.grad.clone()] + [w.grad.clone() for w in Ws]

    _, want = grads("0", False)
    pending, got = grads("1", True)
    assert pending == 1
    _same_bits(want, got, "deferred")
    assert not weight_grad_stream._DEFER["on"] and not weight_grad_stream._DEFER["pending"] and not weight_grad_stream._DEFER["targets"] and not weight_grad_stream._DEFER["handed"]


def test_gru_cell_under_a_deferred_join_is_the_same_bits(gpu_device):
    from tf_gnn_samples_amd import _lib, config, utils
    if not config.settings.limb_gemm:
        pytest.skip("the cell kernels belong to the limb route (RELGNN_GEMM is set to another route in this run)")
    from test_gpu_gru_cell import U, _states, _weights
    V = 2250
    K, R, b = _weights(gpu_device, 61)
    x, h = _states(gpu_device, V, 62)
    gout = torch.randn((V, U), generator=torch.Generator(device="cpu").manual_seed(63)).to(gpu_device)
    assert utils._gru_cell_kernel_ok(x, h, K, R, b, _lib.ACT_TANH)

    def grads(deferred):
        leaves = [t.clone().requires_grad_(True) for t in (x, h, K, R, b)]
        pending = _backward(utils._GRUCellFn.apply(*leaves, _lib.ACT_TANH), gout, "1", deferred)
        return pending, [t.grad.clone() for t in leaves]

    _, want = grads(False)
    pending, got = grads(True)
    assert pending == 1 and all(float(t.abs().max()) > 0 for t in want)
    _same_bits(want, got, "deferred")
