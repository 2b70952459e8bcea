"""Layer-input dropout, the parts that need no GPU: the Philox restatement the GPU tests lean on, the layer_dropout switch and the
CPU model's route.  (Its header of the C ABI, include/relgnn_dropout.h, is held by tests/test_abi.py.)"""
from pathlib import Path

import numpy as np
import pytest

from philox_reference import keep_mask, philox4x32_10, threshold

ROOT = Path(__file__).resolve().parent.parent

# Random123's known-answer vectors for philox4x32_10 (kat_vectors): counter, key -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_restatement_reproduces_the_known_answer_vectors(counter, key, want):
    assert tuple(int(w) for w in philox4x32_10(counter, key)) == want
    # and element for element on arrays (the form keep_mask uses)
    got = philox4x32_10([np.full(3, c) for c in counter], key)
    assert all((np.asarray(g) == w).all() for g, w in zip(got, want))


def test_keep_rule_of_the_restatement():
    assert threshold(0.8) == 13421773 and threshold(0.5) == 1 << 23 and threshold(1.0) == 1 << 24
    words = philox4x32_10((0, 0, 7, 3), (5, 1))
    m = keep_mask(4, 0.8, seed=5, replica=1, step=3, stream=7)
    assert m.tolist() == [(int(w) >> 8) < threshold(0.8) for w in words]
    # an offset moves the tensor through the counter space: elements 4 .. 7 of a long tensor are elements 0 .. 3 at offset 4
    assert np.array_equal(keep_mask(8, 0.8, 5, 1, 3, 7)[4:], keep_mask(4, 0.8, 5, 1, 3, 7, element_offset=4))
    # the high counter word
    hi = philox4x32_10((1, 1, 7, 3), (5, 1))
    assert keep_mask(8, 0.5, 5, 1, 3, 7, element_offset=2 ** 34)[4:].tolist() == [(int(w) >> 8) < (1 << 23) for w in hi]
    assert keep_mask(1 << 12, 1.0, 0, 0, 0, 0).all()


def test_the_switch_is_in_the_table_and_in_the_readme():
    from tf_gnn_samples_amd import config
    rows = {row[0]: row for row in config.describe()}
    env, name, default, allowed, doc = rows["RELGNN_LAYER_DROPOUT"]
    assert (name, default, allowed) == ("layer_dropout", "torch", "torch | fused") and "csrc/dropout.hip" in doc
    assert config.settings.layer_dropout == config.default_of("layer_dropout") == "torch"
    with config.override(layer_dropout="fused") as s:
        assert s.layer_dropout == "fused"
    assert config.settings.layer_dropout == "torch"
    with pytest.raises(ValueError, match="RELGNN_LAYER_DROPOUT must be one of"):
        with config.override(layer_dropout="hip"):
            pass
    text = (ROOT / "README.md").read_text()
    assert "`RELGNN_LAYER_DROPOUT`" in text[text.index("## Switches"):]


def test_a_cpu_model_keeps_the_torch_call_under_the_fused_switch(monkeypatch):
    """No GPU tensor, no kernel: with layer_dropout=fused a CPU model still calls torch.nn.functional.dropout once per layer."""
    import torch
    import torch.nn.functional as F
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.models import RGCN_Model
    from tf_gnn_samples_amd.tasks import PPI_Task
    task = PPI_Task(PPI_Task.default_params())
    task.load_synthetic(2, 1, mean_nodes=60, std_nodes=5, min_nodes=40, max_nodes=80)
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=3, graph_layer_input_dropout_keep_prob=0.8)
    model = RGCN_Model(p, task, device="cpu")
    assert getattr(model, "dropout_state", None) is None
    calls = []
    real = F.dropout

    def recorder(x, p=0.5, training=True, inplace=False):
        calls.append((tuple(x.shape), p, training))
        return real(x, p=p, training=training, inplace=inplace)

    monkeypatch.setattr(F, "dropout", recorder)
    # (bucketing and the layer kernels are GPU-only: the driver loop around them is what runs here)
    from tf_gnn_samples_amd.models import sparse_graph_model
    monkeypatch.setattr(sparse_graph_model, "as_rel_graph", lambda adjacency_lists, num_nodes, validate=True: None)
    monkeypatch.setattr(RGCN_Model, "_apply_gnn_layer", lambda self, h, *a, **k: h)
    x = torch.randn(7, task.initial_node_feature_size)
    with config.override(layer_dropout="fused"):
        out = model.compute_final_node_representations(x, [torch.zeros((0, 2), dtype=torch.int64)] * 3, torch.zeros((7, 3)),
                                                       dropout_keep_prob=0.8)
    assert out.shape == (7, 16)
    assert len(calls) == 3 and all(abs(p_ - 0.2) < 1e-12 and training for _, p_, training in calls)
