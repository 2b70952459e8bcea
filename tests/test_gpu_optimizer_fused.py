"""The fused multi-tensor RMSProp / SGD update (relgnn_mt_rmsprop_clip, relgnn_mt_sgd_clip in csrc/train_utils.hip) behind
TFStyleOptimizer.clip_and_step, and training steps captured as a hipGraph with those optimizers."""
import ctypes
import functools
import pickle
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, CLIP, DECAY, MOMENTUM = 1e-3, 1.0, 0.98, 0.85
# one element, the 4096-element chunk edge on both sides, a tail of one behind two chunks, two shapes of the models
SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (8193,), (3, 5, 7), (256, 121)]
NO_GRAD_VAR, ZERO_GRAD_VAR = 2, 5          # grad None in step 1 / an all-zero gradient in step 2


def _slots(opt):
    return [tensors for _, tensors in opt._slots()]


def _ref_slots(ref):
    return [ref.ms, ref.mom] if hasattr(ref, "ms") else []


def _assert_matches_oracle(params, opt, ref, what):
    """The bars of the issue: variables rtol 3e-6 / atol 3e-7 (the bar of tests/test_gpu_train_utils.py for this comparison), the two
    RMSProp slots 3e-6 x max|reference slot| per variable."""
    for i, (p, r) in enumerate(zip(params, ref.vars)):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=3e-6, atol=3e-7, err_msg="%s: variable %d" % (what, i))
    for k, (mine, theirs) in enumerate(zip(_slots(opt), _ref_slots(ref))):
        for i, (s, r) in enumerate(zip(mine, theirs)):
            err = float(np.abs(s.cpu().numpy() - r).max())
            assert err <= 3e-6 * float(np.abs(r).max()), "%s: slot %d of variable %d off by %g" % (what, k, i, err)


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """Five steps of oracle/optim.py on SHAPES: (initial values, per-step gradients, per-step lr_scale, per-step copies of the
    oracle's variables and slots).  Computed once per optimizer; nobody writes to it."""
    from oracle import optim as O
    rng = np.random.default_rng(11)
    vs = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    ref = O.make_optimizer(name, vs, LR, decay=DECAY, momentum=MOMENTUM)
    steps = []
    for step in range(5):
        gs = [(rng.standard_normal(s) * (5.0 if (i + step) % 2 == 0 else 0.01)).astype(np.float32) for i, s in enumerate(SHAPES)]
        if step == 1:
            gs[NO_GRAD_VAR] = None
        if step == 2:
            gs[ZERO_GRAD_VAR] = np.zeros(SHAPES[ZERO_GRAD_VAR], np.float32)
        scale = 0.5 if step == 3 else 1.0
        O.train_step(ref, gs, CLIP, scale)
        snapshot = types.SimpleNamespace(vars=[v.copy() for v in ref.vars])
        if name == "RMSProp":
            snapshot.ms, snapshot.mom = [v.copy() for v in ref.ms], [v.copy() for v in ref.mom]
        steps.append((gs, scale, snapshot))
    return vs, steps


@pytest.mark.parametrize("name", ["RMSProp", "SGD"])
def test_rule_against_the_numpy_restatement_of_the_tf_rules(gpu_device, name):
    from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
    vs, steps = _oracle_run(name)
    params = [torch.nn.Parameter(torch.as_tensor(v, device=gpu_device)) for v in vs]
    opt = TFStyleOptimizer(params, name, LR, CLIP, decay=DECAY, momentum=MOMENTUM)
    assert opt._fused_update_available()
    for step, (gs, scale, ref) in enumerate(steps):
        for p, g in zip(params, gs):
            p.grad = None if g is None else torch.as_tensor(g, device=gpu_device)
        before = [t[NO_GRAD_VAR].detach().clone() for t in [params] + _slots(opt)]
        opt.clip_and_step(scale)
        if step == 1:                                  # no gradient: the value and both slots keep their bits
            for b, t in zip(before, [params] + _slots(opt)):
                assert torch.equal(b, t[NO_GRAD_VAR].detach())
        _assert_matches_oracle(params, opt, ref, "%s step %d" % (name, step))
        for t in [params] + _slots(opt):
            assert all(bool(torch.isfinite(x).all()) for x in t)
    assert opt.t == 5


@pytest.mark.parametrize("name", ["RMSProp", "SGD"])
def test_fused_update_matches_the_foreach_restatement(gpu_device, name):
    """The bar of test_fused_clip_adam_matches_unfused_tf_rules (tests/test_gpu_train_utils.py)."""
    from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
    torch.manual_seed(0)
    shapes = [(50, 256), (256, 768), (256, 256), (121,), (1,), (256, 121), (3, 5, 7)]
    pa = [torch.nn.Parameter(torch.randn(*s, device=gpu_device)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = TFStyleOptimizer(pa, name, LR, CLIP, decay=DECAY, momentum=MOMENTUM)
    ob = TFStyleOptimizer(pb, name, LR, CLIP, decay=DECAY, momentum=MOMENTUM)
    for step in range(4):
        for i, (a, b) in enumerate(zip(pa, pb)):
            g = torch.randn_like(a) * (5.0 if i % 2 == 0 else 0.01)
            a.grad, b.grad = g.clone(), g.clone()
        pa[4].grad = pb[4].grad = None
        oa.clip_and_step(lr_scale=0.5)                                 # fused
        ob.clip_gradients(); ob.step(lr_scale=0.5)                     # foreach restatement
        for a, b in zip(pa, pb):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)
        for sa, sb in zip(_slots(oa), _slots(ob)):
            for a, b in zip(sa, sb):
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)
    assert oa.t == ob.t == 4


@pytest.mark.parametrize("name", ["RMSProp", "SGD"])
def test_more_variables_than_one_launch_takes(gpu_device, name):
    """100 tensors of 1 to 300 elements: three launches of the update, the last one partial (4 of RELGNN_MT_MAX = 48)."""
    from oracle import optim as O
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
    rng = np.random.default_rng(5)
    sizes = [1, 300] + [int(n) for n in rng.integers(1, 301, 98)]
    assert len(sizes) == 100 > 2 * _lib.MT_MAX and len(sizes) % _lib.MT_MAX != 0
    vs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    params = [torch.nn.Parameter(torch.as_tensor(v, device=gpu_device)) for v in vs]
    opt = TFStyleOptimizer(params, name, LR, CLIP, decay=DECAY, momentum=MOMENTUM)
    ref = O.make_optimizer(name, vs, LR, decay=DECAY, momentum=MOMENTUM)
    for step in range(3):
        gs = [(rng.standard_normal(n) * (5.0 if (i + step) % 2 == 0 else 0.01)).astype(np.float32) for i, n in enumerate(sizes)]
        for p, g in zip(params, gs):
            p.grad = torch.as_tensor(g, device=gpu_device)
        opt.clip_and_step()
        O.train_step(ref, gs, CLIP)
        _assert_matches_oracle(params, opt, ref, "%s step %d" % (name, step))


@pytest.mark.parametrize("name", ["RMSProp", "SGD"])
def test_an_element_s_bits_do_not_depend_on_its_place_or_its_tensor_s_alignment(gpu_device, name):
    """The same 4097 (p, g) values as a tensor of their own, as the head of a 10 000-element tensor and as a view that starts at
    element 1 of a larger buffer (4-byte aligned: the scalar path).  No gradient is clipped (scale exactly 1), the slots start
    equal: after three steps those elements and their slots hold the same bits in all three places, run after run."""
    from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
    N, BIG = 4097, 10000
    rng = np.random.default_rng(9)
    p0 = rng.standard_normal(BIG).astype(np.float32)
    gs = [(rng.standard_normal(BIG) * 1e-3).astype(np.float32) for _ in range(3)]
    assert all(float(np.linalg.norm(g.astype(np.float64))) < 0.5 * CLIP for g in gs)

    def run():
        to = lambda a: torch.as_tensor(a, device=gpu_device)
        buf = torch.zeros(N + 7, device=gpu_device)
        buf[1:N + 1] = to(p0[:N])
        params = [torch.nn.Parameter(to(p0[:N].copy())), torch.nn.Parameter(to(p0)), torch.nn.Parameter(buf[1:N + 1])]
        assert params[0].data_ptr() % 16 == 0 and params[1].data_ptr() % 16 == 0 and params[2].data_ptr() % 16 == 4
        opt = TFStyleOptimizer(params, name, LR, CLIP, decay=DECAY, momentum=MOMENTUM)
        for g in gs:
            params[0].grad, params[1].grad, params[2].grad = to(g[:N].copy()), to(g), to(g[:N].copy())
            opt.clip_and_step()
        torch.cuda.synchronize()
        assert float(buf[0]) == 0.0 and bool((buf[N + 1:] == 0).all())       # nothing written around the view
        return [[t[k].detach()[:N].clone() for k in range(3)] for t in [params] + _slots(opt)]

    first, second = run(), run()
    for own, head, view in first:
        assert torch.equal(own, head) and torch.equal(own, view)
    for a, b in zip(first, second):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(first[0][0], torch.as_tensor(p0[:N], device=gpu_device))      # (the steps did move the values)


def test_direct_calls_refuse_too_many_tensors_and_accept_none(gpu_device):
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    st = _lib.current_stream()
    n = _lib.MT_MAX + 1
    t = {k: torch.full((n, 8), v, device=gpu_device) for k, v in (("p", 1.5), ("g", 0.25), ("ms", 1.0), ("mom", 0.125))}
    want = {k: v.clone() for k, v in t.items()}
    norms = torch.full((n,), 2.0, device=gpu_device)
    arr = ctypes.c_void_p * n
    h = {k: arr(*[v[i].data_ptr() for i in range(n)]) for k, v in t.items()}
    h_n = (ctypes.c_int64 * n)(*([8] * n))
    einval = 1
    assert "argument" in _lib.status_string(einval)
    for count, status in ((n, einval), (0, 0)):
        assert lib.relgnn_mt_rmsprop_clip(h["p"], h["g"], h["ms"], h["mom"], h_n, count, _lib.ptr(norms), 1.0, 1e-3, 0.98, 0.85,
                                          1e-10, st) == status
        assert lib.relgnn_mt_sgd_clip(h["p"], h["g"], h_n, count, _lib.ptr(norms), 1.0, 1e-3, st) == status
    assert lib.relgnn_mt_rmsprop_clip(h["p"], h["g"], h["ms"], h["mom"], h_n, -1, _lib.ptr(norms), 1.0, 1e-3, 0.98, 0.85, 1e-10,
                                      st) == einval
    assert lib.relgnn_mt_sgd_clip(h["p"], h["g"], h_n, -1, _lib.ptr(norms), 1.0, 1e-3, st) == einval
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], want[k]), k


def _ppi_task():
    from tf_gnn_samples_amd.tasks import DataFold, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(3, 1, seed=4, mean_nodes=300, std_nodes=50, min_nodes=100, max_nodes=500, fwd_edges_per_node=6.0)
    return task, task._loaded_data[DataFold.TRAIN]


@pytest.mark.parametrize("which,optimizer,lr_n", [("ggnn_qm9", "RMSProp", None), ("rgcn_ppi", "RMSProp", None),
                                                  ("rgcn_ppi", "SGD", None), ("rgcn_ppi", "RMSProp", 4)])
def test_captured_rmsprop_and_sgd_steps_match_eager_steps(gpu_device, which, optimizer, lr_n):
    """The cases of test_captured_train_step_matches_eager_steps (tests/test_gpu_streams_graphs.py) with the optimizers that
    could not be captured before; ggnn_qm9 with RMSProp is the pairing the QM9 defaults ship.  With lr_for_num_graphs_per_batch the
    learning rate of the recorded update is lr * num_graphs / 4 of the fixed batch."""
    from tf_gnn_samples_amd.models import GGNN_Model, RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, QM9_Task
    if which == "rgcn_ppi":
        task, data = _ppi_task()
        cls, extra = RGCN_Model, dict(hidden_size=128, graph_num_layers=2)
    else:
        from test_golden_cpu import read_qm9_fixture
        task = QM9_Task(QM9_Task.default_params())
        data = task.load_raw(read_qm9_fixture())
        cls, extra = GGNN_Model, dict(hidden_size=64, graph_num_layers=2, graph_rnn_cell="GRU",
                                      message_aggregation_function="mean")
    mb = next(task.make_minibatch_iterator(list(data), DataFold.VALIDATION, 3000))
    if lr_n is not None:
        assert mb.num_graphs != lr_n                    # (the scale is not 1)

    def fresh():
        p = cls.default_params()
        p.update(extra)
        p.update(graph_layer_input_dropout_keep_prob=1.0, random_seed=3, optimizer=optimizer, lr_for_num_graphs_per_batch=lr_n)
        return cls(p, task, device=str(gpu_device)), DeviceBatch(mb, gpu_device)

    eager, batch_e = fresh()
    losses_e = [float(eager.train_step(batch_e)['loss'].detach()) for _ in range(6)]
    captured, batch_c = fresh()
    step = captured.capture_train_step(batch_c, warmup_steps=3)
    losses_c = [float(step.replay()['loss'].detach()) for _ in range(3)]
    torch.cuda.synchronize()
    assert step.handover_status() == 0
    assert captured.optimizer.t == eager.optimizer.t == 6
    np.testing.assert_allclose(losses_c, losses_e[3:], rtol=2e-5)
    for n in eager.variables.names():
        a, b = eager.variables[n].detach().cpu().numpy(), captured.variables[n].detach().cpu().numpy()
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=5e-5, err_msg=n)
        assert float(np.mean(np.abs(b - a) > 1e-6)) < 0.01, n
    assert losses_e[-1] < losses_e[0]


def test_rmsprop_checkpoint_round_trip_continues_with_the_same_bits(gpu_device, tmp_path):
    from tf_gnn_samples_amd import models
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch
    task, data = _ppi_task()
    mb = next(task.make_minibatch_iterator(list(data), DataFold.VALIDATION, 3000))
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=3, optimizer="RMSProp")
    model = RGCN_Model(p, task, device=str(gpu_device))
    assert model.optimizer._fused_update_available()
    batch = DeviceBatch(mb, gpu_device)
    for _ in range(2):
        model.train_step(batch)
    path = tmp_path / "rmsprop.pickle"
    model.save_model(str(path))
    with open(path, "rb") as f:
        weights = pickle.load(f)["weights"]
    trainable = model._trainable_names()
    assert trainable
    for n in trainable:
        assert "%s/RMSProp:0" % n in weights and "%s/RMSProp_1:0" % n in weights, n
        assert weights["%s/RMSProp:0" % n].shape == tuple(model.variables[n].shape)
    restored = models.restore(str(path), str(tmp_path), device=str(gpu_device))
    assert restored.optimizer.name == "rmsprop"
    model.train_step(batch)
    restored.train_step(DeviceBatch(mb, gpu_device))
    torch.cuda.synchronize()
    for n in model.variables.names():
        assert torch.equal(model.variables[n].detach(), restored.variables[n].detach()), n
    for sa, sb in zip(_slots(model.optimizer), _slots(restored.optimizer)):
        assert all(torch.equal(a, b) for a, b in zip(sa, sb))
