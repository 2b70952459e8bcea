"""The fused RMSProp / SGD update (csrc/train_utils.hip) as seen without a GPU: the two entries are declared and bound, CPU
parameters keep the foreach path bit for bit, and a CPU model cannot be captured."""
import re

import pytest
import torch

from abi_reference import declared_names, stripped

NEW_ENTRIES = ("relgnn_mt_rmsprop_clip", "relgnn_mt_sgd_clip")


def test_header_and_ctypes_table_carry_the_two_entries():
    from tf_gnn_samples_amd import _lib
    text, declared = stripped("relgnn.h"), declared_names("relgnn.h")
    sigs = _lib.signatures("relgnn.h")
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in sigs, name
    # the argument counts of the declarations: 13 for RMSProp (four pointer tables, sizes, n, norms, five scalars, stream), 8 for SGD
    for name, nargs in zip(NEW_ENTRIES, (13, 8)):
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs == len(sigs[name][1]), name


@pytest.mark.parametrize("name", ["RMSProp", "SGD"])
def test_cpu_parameters_keep_the_foreach_path_bit_for_bit(name):
    from tf_gnn_samples_amd.models.sparse_graph_model import TFStyleOptimizer
    torch.manual_seed(0)
    shapes = [(7, 5), (33,), (1,), (3, 5, 7)]
    pa = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = TFStyleOptimizer(pa, name, 1e-3, 1.0, decay=0.98, momentum=0.85)
    ob = TFStyleOptimizer(pb, name, 1e-3, 1.0, decay=0.98, momentum=0.85)
    assert not oa._fused_update_available()
    for step in range(3):
        for i, (a, b) in enumerate(zip(pa, pb)):
            g = torch.randn_like(a) * (5.0 if (i + step) % 2 == 0 else 0.01)
            a.grad, b.grad = g.clone(), g.clone()
        if step == 1:
            pa[2].grad = pb[2].grad = None
        oa.clip_and_step(lr_scale=0.5)
        ob.clip_gradients(); ob.step(lr_scale=0.5)
        for a, b in zip(pa, pb):
            assert torch.equal(a, b)
        for sa, sb in zip(oa._slots(), ob._slots()):
            assert all(torch.equal(x, y) for x, y in zip(sa[1], sb[1]))
    assert oa.t == ob.t == 3
    with pytest.raises(RuntimeError):
        oa.clip_and_step(device_step_count=True)         # a captured step never takes the foreach path


@pytest.mark.parametrize("optimizer", ["Adam", "RMSProp", "SGD"])
def test_a_cpu_model_cannot_be_captured(optimizer):
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import DataFold, DeviceBatch, PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(1, 1, seed=2, mean_nodes=30, std_nodes=3, min_nodes=20, max_nodes=40, fwd_edges_per_node=3.0)
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1, optimizer=optimizer)
    model = RGCN_Model(p, task, device="cpu")
    mb = next(task.make_minibatch_iterator(task._loaded_data[DataFold.TRAIN], DataFold.VALIDATION, 10 ** 6))
    with pytest.raises(RuntimeError, match="GPU"):
        model.capture_train_step(DeviceBatch(mb, "cpu"))
