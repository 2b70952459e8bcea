"""The qm9_head switch (config.py), the route QM9_Task takes without a GPU, and the names the new C entries go by."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["relgnn_qm9_head_bwd", "relgnn_qm9_head_fwd", "relgnn_qm9_head_supported", "relgnn_qm9_head_workspace_bytes"]


def test_the_switch_exists_and_validates_its_values():
    from tf_gnn_samples_amd import config
    assert config.default_of("qm9_head") == "compose" and config.attribute_of("RELGNN_QM9_HEAD") == "qm9_head"
    assert config.settings.qm9_head in ("compose", "fused")
    before = config.current()
    with config.override(qm9_head="fused") as s:
        assert s.qm9_head == "fused"
    assert config.current() == before
    with pytest.raises(ValueError, match="RELGNN_QM9_HEAD must be one of compose, fused"):
        with config.override(qm9_head="hip"):
            pass


class _Weights(dict):
    def scope(self, prefix):
        return {k[len(prefix) + 1:]: v for k, v in self.items() if k.startswith(prefix + "/")}


def test_cpu_tensors_take_the_composition_whatever_the_switch_says(monkeypatch):
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.tasks import QM9_Task, qm9_task
    rng = np.random.default_rng(0)
    V, G, hidden, A, task_ids = 23, 4, 8, 3, [1, 4]
    p = QM9_Task.default_params()
    p.update(task_ids=task_ids)
    task = QM9_Task(p)
    weights = _Weights()
    for t in task_ids:
        s = "out_layer_task%i" % t
        weights[s + "/regression/dense/kernel"] = torch.tensor(rng.uniform(-1, 1, (hidden, 1)).astype(np.float32))
        weights[s + "/regression/dense/bias"] = torch.tensor(rng.uniform(-1, 1, (1,)).astype(np.float32))
        weights[s + "/regression_gate/dense/kernel"] = torch.tensor(rng.uniform(-1, 1, (hidden + A, 1)).astype(np.float32))
        weights[s + "/regression_gate/dense/bias"] = torch.tensor(rng.uniform(-1, 1, (1,)).astype(np.float32))
    states = torch.tensor(rng.uniform(-1, 1, (V, hidden)).astype(np.float32))
    batch = types.SimpleNamespace(num_graphs=G, initial_node_features=torch.tensor(rng.uniform(-1, 1, (V, A)).astype(np.float32)),
                                  graph_nodes_list=torch.tensor(np.sort(rng.integers(0, G, V)).astype(np.int32)),
                                  extra={'target_values': torch.tensor(rng.uniform(-1, 1, (len(task_ids), G)).astype(np.float32))})
    from tf_gnn_samples_amd import _lib, ops
    # the composition's segment sum is a HIP kernel and the package has no CPU fallback: on CPU tensors both switch values end in
    # the same refusal, at the same call
    for route in ("compose", "fused"):
        qm9_task.ROUTES["head"] = None
        with config.override(qm9_head=route), pytest.raises(_lib.RelGnnLibraryError, match="no CPU fallback"):
            task.compute_task_metrics(states, batch, weights)
        assert qm9_task.ROUTES["head"] == "composition"

    def segment_sum(data, segment_ids, num_segments):    # a stand-in for that one kernel, so that the rest of the chain runs here
        return torch.zeros((num_segments, data.shape[1]), dtype=data.dtype).index_add(0, segment_ids.long(), data)
    monkeypatch.setattr(ops, "unsorted_segment_sum", segment_sum)
    got = {}
    for route in ("compose", "fused"):
        qm9_task.ROUTES["head"] = None
        with config.override(qm9_head=route):
            got[route] = task.compute_task_metrics(states, batch, weights)
        assert qm9_task.ROUTES["head"] == "composition"
    assert sorted(got["fused"]) == ["abs_err_task1", "abs_err_task4", "loss", "total_loss"]
    for name, value in got["compose"].items():
        assert torch.equal(got["fused"][name], value), name


def test_header_binding_and_readme_agree_on_the_new_names():
    from tf_gnn_samples_amd import _lib, config
    header = (ROOT / "include" / "relgnn.h").read_text()
    declared = sorted(set(re.findall(r"\b(relgnn_qm9_head_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == ENTRIES
    assert sorted(n for n in _lib.signatures("relgnn.h") if n.startswith("relgnn_qm9_head")) == ENTRIES
    assert "RELGNN_ERRFLAG_NOT_SORTED 2u" in header and _lib.ERRFLAG_NOT_SORTED == 2
    assert "tasks/qm9_task.py:163-197" in header
    readme = (ROOT / "README.md").read_text()
    switches = readme[readme.index("## Switches"):]
    assert "`RELGNN_QM9_HEAD`" in switches and "`qm9_head`" in switches and "qm9_head.hip" in readme
    row = next(r for r in config.describe() if r[1] == "qm9_head")
    assert row[0] == "RELGNN_QM9_HEAD" and row[2] == "compose" and row[3] == "compose | fused"
    assert (ROOT / "tf_gnn_samples_amd" / "csrc" / "qm9_head.hip").exists()
