"""Layer-input dropout on the fused route (csrc/dropout.hip, include/relgnn_dropout.h, config.settings.layer_dropout == "fused"):
the kernels bit for bit against the NumPy restatement of Philox4x32-10 and of the reference's arithmetic (tests/philox_reference.py),
the driver loop against the oracle and against the torch route on the same masks, a captured step, and the step's memory."""
import functools

import numpy as np
import pytest
import torch

from philox_reference import dropout_f32, keep_mask, threshold

pytestmark = pytest.mark.gpu

SEED, STEP, STREAM = 7, 1, 3
BIG = (1 << 20) + 3               # 1024 blocks x 256 threads x 4 elements is one grid pass: one more group, which is a scalar tail
COUNTS = [1, 3, 4, 5, 130, BIG]
SHAPES = [(3, 5), (100, 320)]


@functools.lru_cache(maxsize=None)
def _mask(n, keep, seed=SEED, step=STEP, stream=STREAM, offset=0):
    m = keep_mask(n, keep, seed, 0, step, stream, element_offset=offset)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _values(n, salt=0):
    x = np.random.default_rng(100 + salt).standard_normal(n).astype(np.float32)
    x.setflags(write=False)
    return x


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)).reshape(-1).view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (
        what, bad.size, g.size, bad[0], g.view(np.float32)[bad[0]], w.view(np.float32)[bad[0]])


def _state(dev, seed=SEED, step=STEP):
    from tf_gnn_samples_amd import ops
    return ops.dropout_state(dev, seed, 0, step)


def _inputs(case, dev):
    """(tensor on the device, its values as a flat array) for an element count, a shape, or the 4-byte aligned view."""
    if case == "view":
        buf = torch.tensor(_values(131), device=dev)
        x = buf[1:]
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        return x, _values(131)[1:]
    n = int(np.prod(case))
    return torch.tensor(_values(n), device=dev).reshape(case), _values(n)


# ---- 1. forward bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.8, 0.5])
@pytest.mark.parametrize("case", COUNTS + SHAPES + ["view"], ids=str)
def test_forward_bits(gpu_device, case, keep):
    from tf_gnn_samples_amd import ops
    x, values = _inputs(case, gpu_device)
    y = ops.dropout(x, keep, _state(gpu_device), STREAM)
    assert y.shape == x.shape and y.is_contiguous()
    _same_bits(y, dropout_f32(values, keep, _mask(values.size, keep)), "dropout %s keep %s" % (case, keep))


def _raw_forward(x, keep, state, stream, offset):
    from tf_gnn_samples_amd import _lib
    y = torch.full_like(x, 123.0)
    _lib.launch("relgnn_dropout_fwd", _lib.ptr(x), x.numel(), offset, _lib.ptr(state), stream, threshold(keep), keep, _lib.ptr(y))
    return y


def test_element_offset_reaches_the_high_counter_word(gpu_device):
    x = torch.tensor(_values(130), device=gpu_device)
    y = _raw_forward(x, 0.8, _state(gpu_device), STREAM, 1 << 34)
    want_mask = _mask(130, 0.8, offset=1 << 34)
    assert not np.array_equal(want_mask, _mask(130, 0.8))
    _same_bits(y, dropout_f32(_values(130), 0.8, want_mask), "element_offset 2^34")
    with pytest.raises(ValueError):
        _raw_forward(x, 0.8, _state(gpu_device), STREAM, 2)
    torch.cuda.synchronize()


def test_replica_is_the_second_word_of_the_key(gpu_device):
    from tf_gnn_samples_amd import ops
    x = torch.tensor(_values(130), device=gpu_device)
    y = ops.dropout(x, 0.8, ops.dropout_state(gpu_device, SEED, 3, STEP), STREAM)
    want_mask = keep_mask(130, 0.8, SEED, 3, STEP, STREAM)
    assert not np.array_equal(want_mask, _mask(130, 0.8))
    _same_bits(y, dropout_f32(_values(130), 0.8, want_mask), "replica 3")


# ---- 2. backward bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [5, 130, (100, 320), "view"], ids=str)
def test_backward_bits_and_nothing_but_the_state_is_saved(gpu_device, case):
    from tf_gnn_samples_amd import ops
    x, values = _inputs(case, gpu_device)
    x = x.detach().requires_grad_(True)
    g = _values(values.size, salt=1)
    y = ops.dropout(x, 0.8, _state(gpu_device), STREAM)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.int64 and saved[0].numel() == 3       # 24 bytes: no mask
    (gx,) = torch.autograd.grad(y, x, torch.tensor(g, device=gpu_device).reshape(y.shape))
    _same_bits(gx, dropout_f32(g, 0.8, _mask(values.size, 0.8)), "dropout backward %s" % (case,))


def test_a_backward_uses_the_mask_of_its_own_forward(gpu_device):
    """The driver loop's protocol: bump the step on the device, clone the state for the pass.  A second forward in between does not
    change the mask the first one's backward regenerates."""
    from tf_gnn_samples_amd import ops
    n = 1000
    x = torch.tensor(_values(n), device=gpu_device).requires_grad_(True)
    state = _state(gpu_device, step=0)
    passes = []
    for _ in range(2):
        state[2].add_(1)
        passes.append(ops.dropout(x, 0.8, state.clone(), STREAM))
    g = _values(n, salt=1)
    m1, m2 = _mask(n, 0.8, step=1), _mask(n, 0.8, step=2)
    assert not np.array_equal(m1, m2)
    _same_bits(passes[0], dropout_f32(_values(n), 0.8, m1), "forward at step 1")
    _same_bits(passes[1], dropout_f32(_values(n), 0.8, m2), "forward at step 2")
    (gx,) = torch.autograd.grad(passes[0], x, torch.tensor(g, device=gpu_device))
    _same_bits(gx, dropout_f32(g, 0.8, m1), "backward of the step-1 forward")


# ---- 3. residual form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_g_t", [False, True], ids=["g_t_absent", "g_t_present"])
@pytest.mark.parametrize("case", COUNTS + SHAPES + ["view"], ids=str)
def test_residual_form_gives_the_composition_s_bits(gpu_device, case, with_g_t):
    from tf_gnn_samples_amd import ops
    x0, values = _inputs(case, gpu_device)
    n = values.size
    last0 = torch.tensor(_values(n, salt=2), device=gpu_device).reshape(x0.shape)
    g_cur = torch.tensor(_values(n, salt=3), device=gpu_device).reshape(x0.shape)
    g_t = torch.tensor(_values(n, salt=4), device=gpu_device).reshape(x0.shape)
    results = []
    for fused in (True, False):
        x, last = x0.detach().requires_grad_(True), last0.detach().requires_grad_(True)
        if fused:
            t, cur = ops.dropout_residual(x, last, 0.8, _state(gpu_device), STREAM)
        else:
            t = ops.dropout(x, 0.8, _state(gpu_device), STREAM)
            cur = (t + last) / 2
        outs, gs = ([t, cur], [g_t, g_cur]) if with_g_t else ([cur], [g_cur])
        g_x, g_last = torch.autograd.grad(outs, [x, last], gs)
        results.append((t, cur, g_x, g_last))
    for name, a, b in zip(("t", "cur", "g_x", "g_last"), *results):
        _same_bits(a, b, "%s of %s" % (name, case))
    # and against NumPy, so that the two routes are not merely wrong together
    mask = _mask(n, 0.8)
    t_np = dropout_f32(values, 0.8, mask)
    _same_bits(results[0][0], t_np, "t vs NumPy")
    _same_bits(results[0][1], (t_np + _values(n, salt=2)) / np.float32(2), "cur vs NumPy")
    half = _values(n, salt=3) / np.float32(2)
    _same_bits(results[0][2], dropout_f32(_values(n, salt=4) + half if with_g_t else half, 0.8, mask), "g_x vs NumPy")
    _same_bits(results[0][3], half, "g_last vs NumPy")


@pytest.mark.parametrize("case", [5, 130, "view"], ids=str)
def test_residual_backward_when_only_t_is_used(gpu_device, case):
    """g_cur absent (nothing read cur): the gradient of x is the plain dropout's, g_last is None."""
    from tf_gnn_samples_amd import ops
    x0, values = _inputs(case, gpu_device)
    n = values.size
    x = x0.detach().requires_grad_(True)
    last = torch.tensor(_values(n, salt=2), device=gpu_device).reshape(x0.shape).requires_grad_(True)
    t, _ = ops.dropout_residual(x, last, 0.8, _state(gpu_device), STREAM)
    g_x, g_last = torch.autograd.grad([t], [x, last], [torch.tensor(_values(n, salt=4), device=gpu_device).reshape(x0.shape)],
                                      allow_unused=True)
    assert g_last is None
    _same_bits(g_x, dropout_f32(_values(n, salt=4), 0.8, _mask(n, 0.8)), "g_x from g_t alone")


# ---- 4. non-finite and extreme inputs --------------------------------------------------------------------------------------------
def _same_bits_nan_aware(got, want, what):
    g, w = np.asarray(got.detach().cpu().numpy(), np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: NaN positions differ" % what
    ok = ~np.isnan(w)
    assert np.array_equal(g[ok].view(np.int32), w[ok].view(np.int32)), what


def test_non_finite_and_extreme_inputs(gpu_device):
    """A dropped +-inf / NaN is NaN (inf * 0), denormals and the largest floats go through a true division: the NumPy composition's
    bits (a NaN's payload is the platform's: positions are compared)."""
    from tf_gnn_samples_amd import ops
    fmax, tiny = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    special = np.array([np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -3e-39, tiny, -tiny, tiny * 0.8, fmax, -fmax, fmax * 0.8,
                        fmax * 0.81, 0.0, -0.0, 1.0, -1.5], np.float32)
    x_np = np.tile(special, 40)                        # every value meets kept and dropped elements
    mask = _mask(x_np.size, 0.8)
    for v in range(special.size):
        assert mask[v::special.size].any() and not mask[v::special.size].all()
    last_np = np.roll(x_np, 7)
    x, last = torch.as_tensor(x_np, device=gpu_device), torch.as_tensor(last_np, device=gpu_device)
    with np.errstate(all="ignore"):
        t_np = dropout_f32(x_np, 0.8, mask)
        cur_np = (t_np + last_np) / np.float32(2)
        half = x_np / np.float32(2)
        gx_np = dropout_f32(last_np + half, 0.8, mask)
    assert np.isnan(t_np[np.isinf(x_np) & ~mask]).all()
    _same_bits_nan_aware(ops.dropout(x, 0.8, _state(gpu_device), STREAM), t_np, "dropout")
    t, cur = ops.dropout_residual(x, last, 0.8, _state(gpu_device), STREAM)
    _same_bits_nan_aware(t, t_np, "residual t")
    _same_bits_nan_aware(cur, cur_np, "residual cur")
    xr, lr = x.clone().requires_grad_(True), last.clone().requires_grad_(True)
    t, cur = ops.dropout_residual(xr, lr, 0.8, _state(gpu_device), STREAM)
    g_x, g_last = torch.autograd.grad([t, cur], [xr, lr], [last, x])          # g_t = last's values, g_cur = x's values
    _same_bits_nan_aware(g_last, half, "residual g_last")
    _same_bits_nan_aware(g_x, gx_np, "residual g_x")


# ---- 5. streams do not collide ---------------------------------------------------------------------------------------------------
def test_streams_steps_and_seeds_draw_independent_masks(gpu_device):
    from tf_gnn_samples_amd import ops
    n, keep = 1 << 20, 0.8
    ones = torch.ones(n, device=gpu_device)

    def kept(seed, step, stream):
        return ops.dropout(ones, keep, _state(gpu_device, seed=seed, step=step), stream) != 0

    base = kept(0, 1, 0)
    assert torch.equal(base, kept(0, 1, 0))                                    # the same (seed, step, stream): the same bits
    p = threshold(keep) / float(1 << 24)
    sigma, sigma_joint = (p * (1 - p) / n) ** 0.5, (0.64 * 0.36 / n) ** 0.5      # 3.9e-4, 4.7e-4
    others = {"stream": kept(0, 1, 1), "step": kept(0, 2, 0), "seed": kept(1, 1, 0)}
    for name, m in [("base", base)] + list(others.items()):
        share = float(m.float().mean())
        print("%s: share kept %.6f (%.2f sigma)" % (name, share, (share - p) / sigma))
        assert abs(share - p) <= 6 * sigma, name
    for name, m in others.items():
        joint = float((base & m).float().mean())
        print("base and another %s: share kept by both %.6f (%.2f sigma)" % (name, joint, (joint - 0.64) / sigma_joint))
        assert abs(joint - 0.64) <= 6 * sigma_joint, name


# ---- 6. placement against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual_every", [2, 10000])
def test_fused_route_sits_where_the_reference_puts_dropout(gpu_device, monkeypatch, residual_every):
    """tests/test_gpu_configs.py::test_driver_loop_dropout_sits_where_the_reference_puts_it with nothing patched: the masks of the
    fused route are known in advance (seed = random_seed, replica 0, step 1, stream = layer), so the oracle takes them as its
    argument.  Node states within 1e-5 abs (that test's bar)."""
    from oracle import model as OM
    from tf_gnn_samples_amd import _lib, config
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(2, 1, seed=4, mean_nodes=300, std_nodes=40, min_nodes=100, max_nodes=400, fwd_edges_per_node=5.0)
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=4, graph_residual_connection_every_num_layers=residual_every,
             graph_dense_between_every_num_gnn_layers=2, graph_layer_input_dropout_keep_prob=0.8)
    model = RGCN_Model(p, task, device=str(gpu_device))
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 6))
    batch = DeviceBatch(mb, gpu_device)
    assert model.dropout_state.tolist() == [p['random_seed'], 0, 0]
    masks = [keep_mask(mb.num_nodes * 64, 0.8, p['random_seed'], 0, 1, layer).reshape(mb.num_nodes, 64) for layer in range(4)]
    x = batch.initial_node_features.clone().requires_grad_(True)
    with config.override(layer_dropout="fused"):
        final = model.compute_final_node_representations(x, batch.adjacency_lists, batch.type_to_num_incoming_edges, dropout_keep_prob=0.8)
        assert int(model.dropout_state[2]) == 1
        W = {n[len("graph_model/"):]: model.variables[n].detach().cpu().numpy() for n in model.variables.names() if n.startswith("graph_model/")}
        fd = mb.feed_dict
        want = OM.graph_propagation(fd['initial_node_features'].astype(np.float32), fd['adjacency_lists'],
                                    fd['type_to_num_incoming_edges'].astype(np.float32), p, W, OM.rgcn_apply(p), dropout=(0.8, masks))
        err = float(np.abs(final.detach().cpu().numpy() - want).max())
        print("max |fused route - oracle| = %.3g" % err)
        assert err <= 1e-5
        final.square().sum().backward()
        assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
        # evaluation: keep-prob 1 launches no dropout kernel and leaves the step alone
        launched = []
        real = _lib.launch
        monkeypatch.setattr(_lib, "launch", lambda name, *args: (launched.append(name), real(name, *args))[1])
        with torch.no_grad():
            model.compute_final_node_representations(batch.initial_node_features, batch.adjacency_lists, batch.type_to_num_incoming_edges)
        assert launched and not [name for name in launched if "dropout" in name]
        assert int(model.dropout_state[2]) == 1


# ---- 7. the torch route on the same masks ----------------------------------------------------------------------------------------
def _both_routes(make_model, batch, monkeypatch):
    """One forward (step 1) and one training step (step 2) per route -> [(final states, {variable: gradient}, {variable: value})]."""
    import torch.nn.functional as F
    from tf_gnn_samples_amd import config
    out = []
    for route in ("torch", "fused"):
        model = make_model()
        seed = model.params['random_seed']
        pos = {"step": 0, "layer": 0}

        def helper_dropout(x, p=0.5, training=True, inplace=False):
            keep = 1.0 - p
            assert training and abs(keep - 0.8) < 1e-12
            m = keep_mask(x.numel(), 0.8, seed, 0, pos["step"], pos["layer"]).reshape(tuple(x.shape))
            pos["layer"] += 1
            # a true division (a 0-dim device tensor as the divisor; a Python scalar would be multiplied by its reciprocal)
            return torch.div(x, torch.tensor(0.8, dtype=x.dtype, device=x.device)) * torch.as_tensor(m, dtype=x.dtype, device=x.device)

        with monkeypatch.context() as mp, config.override(layer_dropout=route):
            if route == "torch":
                mp.setattr(F, "dropout", helper_dropout)
            pos.update(step=1, layer=0)
            with torch.no_grad():
                final = model.compute_final_node_representations(
                    model.task.compute_initial_node_features(batch, model.variables.scope("")), batch.adjacency_lists,
                    batch.type_to_num_incoming_edges, dropout_keep_prob=0.8).clone()
            pos.update(step=2, layer=0)
            model.train_step(batch)
            torch.cuda.synchronize()
            if route == "torch":
                assert pos["layer"] == model.params['graph_num_layers'] and int(model.dropout_state[2]) == 0
            else:
                assert int(model.dropout_state[2]) == 2
        names = model.variables.names()
        out.append((final, {n: model.variables[n].grad for n in names}, {n: model.variables[n].detach() for n in names}))
    return out


def _assert_routes_agree(results):
    (final_t, grads_t, vars_t), (final_f, grads_f, vars_f) = results
    assert torch.equal(final_t.view(torch.int32), final_f.view(torch.int32))
    assert float(final_t.abs().max()) > 0
    for n in grads_t:
        assert (grads_t[n] is None) == (grads_f[n] is None), n
        if grads_t[n] is not None:
            assert torch.equal(grads_t[n].contiguous().view(torch.int32), grads_f[n].contiguous().view(torch.int32)), "gradient of " + n
        assert torch.equal(vars_t[n].view(torch.int32), vars_f[n].view(torch.int32)), n
    assert any(g is not None and float(g.abs().max()) > 0 for g in grads_t.values())


def test_same_bits_as_the_torch_route_rgcn_residual_every_2(gpu_device, monkeypatch):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(2, 1, seed=4, mean_nodes=300, std_nodes=40, min_nodes=100, max_nodes=400, fwd_edges_per_node=5.0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 6))
    batch = DeviceBatch(mb, gpu_device)

    def make_model():
        p = RGCN_Model.default_params()
        p.update(hidden_size=64, graph_num_layers=5, graph_residual_connection_every_num_layers=2,
                 graph_dense_between_every_num_gnn_layers=2, graph_layer_input_dropout_keep_prob=0.8, random_seed=5)
        return RGCN_Model(p, task, device=str(gpu_device))

    _assert_routes_agree(_both_routes(make_model, batch, monkeypatch))


def test_same_bits_as_the_torch_route_gnn_film_23_edge_types(gpu_device, monkeypatch, tmp_path):
    from varmisuse_cases import build_task, one_batch
    from tf_gnn_samples_amd.models import GNN_FiLM_Model
    from tf_gnn_samples_amd.tasks import DeviceBatch
    task, folds = build_task(tmp_path, 1)
    assert task.num_edge_types == 23
    batch = DeviceBatch(one_batch(task, folds["valid"]), gpu_device)          # the smallest fold: three graphs

    def make_model():
        p = GNN_FiLM_Model.default_params()
        p.update(hidden_size=128, graph_num_layers=4, graph_layer_input_dropout_keep_prob=0.8, random_seed=2)
        return GNN_FiLM_Model(p, task, device=str(gpu_device))

    _assert_routes_agree(_both_routes(make_model, batch, monkeypatch))


# ---- 8. captured step ------------------------------------------------------------------------------------------------------------
def test_captured_step_draws_new_masks_on_every_replay(gpu_device):
    """capture_train_step with SGD, keep 0.8, fused: three warm-up steps and three replays against six eager steps from the same
    weights and the same dropout_state, compared the way tests/test_gpu_optimizer_fused.py compares captured and eager SGD steps.
    Recording a hipGraph runs nothing, so the device step count stands at warmup_steps + 3 afterwards, like the optimizer's."""
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(3, 1, seed=4, mean_nodes=300, std_nodes=50, min_nodes=100, max_nodes=500, fwd_edges_per_node=6.0)
    mb = next(task.make_minibatch_iterator(list(task._loaded_data[DataFold.TRAIN]), DataFold.VALIDATION, 3000))

    def fresh():
        p = RGCN_Model.default_params()
        p.update(hidden_size=128, graph_num_layers=4, graph_layer_input_dropout_keep_prob=0.8, random_seed=3, optimizer="SGD")
        return RGCN_Model(p, task, device=str(gpu_device)), DeviceBatch(mb, gpu_device)

    with config.override(layer_dropout="fused"):
        eager, batch_e = fresh()
        losses_e = [float(eager.train_step(batch_e)['loss'].detach()) for _ in range(6)]
        captured, batch_c = fresh()
        assert torch.equal(captured.dropout_state, torch.tensor([3, 0, 0], device=gpu_device))
        step = captured.capture_train_step(batch_c, warmup_steps=3)
        losses_c = [float(step.replay()['loss'].detach()) for _ in range(3)]
        torch.cuda.synchronize()
    assert step.handover_status() == 0
    assert captured.optimizer.t == eager.optimizer.t == 6
    assert int(captured.dropout_state[2]) == int(eager.dropout_state[2]) == 3 + 3
    print("eager", losses_e, "replayed", losses_c)
    np.testing.assert_allclose(losses_c, losses_e[3:], rtol=2e-5)
    for n in eager.variables.names():
        a, b = eager.variables[n].detach().cpu().numpy(), captured.variables[n].detach().cpu().numpy()
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=5e-5, err_msg=n)
        assert float(np.mean(np.abs(b - a) > 1e-6)) < 0.01, n
    assert len(set(losses_c)) == 3                       # the masks moved from replay to replay


# ---- 9. memory -------------------------------------------------------------------------------------------------------------------
def test_fused_step_needs_no_more_memory_than_the_torch_route(gpu_device):
    """One training step at hidden 256, 4 layers, about 20 000 nodes: the torch route keeps one mask per layer for the backward
    (V x 256 bytes each); the fused route keeps 24 bytes."""
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(10, 1, seed=6, mean_nodes=2000, std_nodes=100, min_nodes=1700, max_nodes=2300, fwd_edges_per_node=4.0)
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 6))
    assert 17000 <= mb.num_nodes <= 23000
    batch = DeviceBatch(mb, gpu_device)
    p = RGCN_Model.default_params()
    p.update(hidden_size=256, graph_num_layers=4, graph_layer_input_dropout_keep_prob=0.8)
    model = RGCN_Model(p, task, device=str(gpu_device))
    peak = {}
    for route in ("torch", "fused"):
        with config.override(layer_dropout=route):
            model.train_step(batch)                        # plans, caches, optimizer state
            model.optimizer.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(gpu_device)
            model.train_step(batch)
            torch.cuda.synchronize()
            peak[route] = torch.cuda.max_memory_allocated(gpu_device)
            model.optimizer.zero_grad()
    print("peak allocated bytes of the step: torch %d, fused %d (the masks alone: %d)" % (
        peak["torch"], peak["fused"], 4 * mb.num_nodes * 256))
    assert peak["fused"] <= peak["torch"]


# ---- 10. data parallelism: the replica is the rank ---------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    import os
    import sys
    from pathlib import Path
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import torch.distributed as dist
    from tf_gnn_samples_amd import ops
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.parallel import init_distributed
    from tf_gnn_samples_amd.tasks import PPI_Task
    init_distributed(backend="gloo")                    # (both ranks share cuda:0, as in tests/test_gpu_dp.py)
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(1, 1, seed=3, mean_nodes=80, std_nodes=1, min_nodes=60, max_nodes=100)
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, random_seed=5)
    model = RGCN_Model(p, task, device="cuda:0")
    kept = ops.dropout(torch.ones(4096, device="cuda:0"), 0.8, model.dropout_state, 0) != 0
    q.put((rank, model.dropout_state.tolist(), kept.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_a_model_built_in_a_process_group_takes_its_rank_as_replica(gpu_device):
    """Two ranks (one GPU, gloo): dropout_state[1] is the rank, and the ranks draw different masks from the same seed and step."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, state, kept in results:
        assert state == [5, rank, 0]
        assert np.array_equal(kept, keep_mask(4096, 0.8, 5, rank, 0, 0)), rank
    assert not np.array_equal(results[0][2], results[1][2])
