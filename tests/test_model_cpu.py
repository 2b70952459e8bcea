"""Host-side model plumbing that needs no GPU: TF variable naming, the reference's best-model pickle layout
(models/sparse_graph_model.py:91-126) and registries."""
import pickle

import numpy as np
import pytest
import torch


def _task():
    from tf_gnn_samples_amd.tasks import PPI_Task
    t = PPI_Task(PPI_Task.default_params())
    t.load_synthetic(2, 1, mean_nodes=60, std_nodes=5, min_nodes=40, max_nodes=80)
    return t


def test_rgcn_variable_names_and_parameter_count():
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(hidden_size=256, graph_num_layers=3)
    m = RGCN_Model(p, _task(), device="cpu")
    names = m.variables.names()
    assert m.variables.num_parameters() == 699257                      # README.md:29 of the reference
    assert "graph_model/dense/kernel" in names                        # input projection 50 -> 256
    assert "graph_model/gnn_layer_0/Dense/kernel" in names            # layer 0 ALWAYS gets the Dense (:194-200)
    assert "graph_model/gnn_layer_1/Dense/kernel" not in names
    assert tuple(m.variables["graph_model/gnn_layer_2/Edge_1_Weight/kernel"].shape) == (256, 256)   # TF layout [in, out]
    assert tuple(m.variables["dense_1/kernel"].shape) == (256, 121)


def test_best_model_pickle_round_trip(tmp_path):
    from tf_gnn_samples_amd.models import GNN_FiLM_Model
    task = _task()
    p = GNN_FiLM_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=2)
    a = GNN_FiLM_Model(p, task, device="cpu")
    path = tmp_path / "best_model.pickle"
    a.save_model(str(path))
    data = pickle.load(open(path, "rb"))
    assert set(data) == {"model_class", "task_class", "model_params", "task_params", "task_metadata", "weights"}
    assert data["model_class"] == "GNN-FiLM" and data["task_class"] == "PPI"
    assert all(k.endswith(":0") and isinstance(v, (np.ndarray, np.generic)) for k, v in data["weights"].items())
    p2 = dict(p, random_seed=7)
    b = GNN_FiLM_Model(p2, task, device="cpu")
    assert not torch.equal(a.variables["graph_model/gnn_layer_0/Edge_0_Weight/kernel"],
                           b.variables["graph_model/gnn_layer_0/Edge_0_Weight/kernel"])
    b.load_weights(data["weights"])
    for n in a.variables.names():
        assert torch.equal(a.variables[n], b.variables[n]), n


def test_registries_and_unknown_names():
    from tf_gnn_samples_amd.models import name_to_model_class
    from tf_gnn_samples_amd.tasks import name_to_task_class
    assert name_to_model_class("RGCN")[0].__name__ == "RGCN_Model"
    assert name_to_model_class("GNN-Edge-MLP0")[1] == {'num_edge_hidden_layers': 0}
    assert name_to_model_class("rgdcn")[0].__name__ == "RGDCN_Model"
    assert name_to_task_class("qm9")[0].__name__ == "QM9_Task" and name_to_task_class("PPI")[1] == {}      # (class, extra params) as the reference
    with pytest.raises(ValueError):
        name_to_model_class("GCN")
    with pytest.raises(ValueError):
        name_to_task_class("varmisuse")


def test_every_model_declares_its_variables_on_cpu():
    from tf_gnn_samples_amd.models import MODEL_CLASSES
    task = _task()
    for cls in set(MODEL_CLASSES.values()):
        p = cls.default_params()
        p.update(hidden_size=32, graph_num_layers=2)
        m = cls(p, task, device="cpu")
        assert m.variables.num_parameters() > 0
        # inter-layer norm gets its own scope when the layer already owns a LayerNorm (TF uniquifies the name)
        if p.get('graph_inter_layer_norm') and "graph_model/gnn_layer_0/LayerNorm/gamma" in m.variables.names() \
                and cls.__name__ in ("RGIN_Model", "GNN_Edge_MLP_Model"):
            assert "graph_model/gnn_layer_0/LayerNorm_1/gamma" in m.variables.names()


def test_effective_cpu_count_is_bounded_by_quota_and_affinity():
    import os
    from tf_gnn_samples_amd.parallel import effective_cpu_count
    n = effective_cpu_count()
    assert 1 <= n <= (os.cpu_count() or 1)
    if hasattr(os, "sched_getaffinity"):
        assert n <= len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            assert n <= max(1, int(int(quota) / int(period)))
    except OSError:
        pass


# ---- TF variable name lists (what a reference checkpoint of the same configuration holds) -----------------------------
def _gnn_names(prefix, L, extra=()):
    return ["%s/Edge_%i_Weight/kernel" % (prefix, l) for l in range(L)] + ["%s/%s" % (prefix, e) for e in extra]


def test_variable_names_equal_the_reference_name_lists():
    """Names as the TF1 graph of the reference would create them (variable_scope('graph_model') /
    'gnn_layer_%i', models/sparse_graph_model.py:161-200; heads: tasks/ppi_task.py:176-179 (unnamed Keras Dense ->
    dense_1), tasks/qm9_task.py:163-176 (variable_scope('out_layer_task%i') at the ROOT, MLP scopes regression /
    regression_gate, tf.layers.Dense default name 'dense')).  A reference pickle of the same configuration is keyed by
    exactly these names + ':0'."""
    from tf_gnn_samples_amd.models import GGNN_Model, GNN_FiLM_Model, RGCN_Model
    from tf_gnn_samples_amd.tasks import QM9_Task
    p = RGCN_Model.default_params()
    p.update(hidden_size=64, graph_num_layers=2)
    got = RGCN_Model(p, _task(), device="cpu").variables.names()
    want = (["graph_model/dense/kernel"] + _gnn_names("graph_model/gnn_layer_0", 3, ["Dense/kernel"])
            + _gnn_names("graph_model/gnn_layer_1", 3) + ["dense_1/kernel", "dense_1/bias"])
    assert sorted(got) == sorted(want)

    qm9 = QM9_Task(QM9_Task.default_params())
    import gzip, json
    from pathlib import Path
    with gzip.open(Path(__file__).resolve().parent / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
        qm9._loaded_data = {}
        qm9.load_raw([json.loads(line) for _, line in zip(range(64), f)])
    assert qm9.num_edge_types == 5
    p = GGNN_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=2)
    got = GGNN_Model(p, qm9, device="cpu").variables.names()
    cell = ["gru_cell/kernel", "gru_cell/recurrent_kernel", "gru_cell/bias"]
    want = (["graph_model/dense/kernel"] + _gnn_names("graph_model/gnn_layer_0", 5, cell + ["Dense/kernel"])
            + _gnn_names("graph_model/gnn_layer_1", 5, cell)
            + ["out_layer_task0/regression_gate/dense/kernel", "out_layer_task0/regression_gate/dense/bias",
               "out_layer_task0/regression/dense/kernel", "out_layer_task0/regression/dense/bias"])
    assert sorted(got) == sorted(want)

    # two timesteps per layer: one LayerNorm scope per timestep, the inter-layer norm is the next one
    p = GNN_FiLM_Model.default_params()
    p.update(hidden_size=32, graph_num_layers=1, graph_num_timesteps_per_layer=2, graph_inter_layer_norm=True)
    got = GNN_FiLM_Model(p, _task(), device="cpu").variables.names()
    film = ["Edge_%i_FiLM_Computations/kernel" % l for l in range(3)]
    lns = ["%s/%s" % (s, v) for s in ("LayerNorm", "LayerNorm_1", "LayerNorm_2") for v in ("beta", "gamma")]
    want = (["graph_model/dense/kernel"] + _gnn_names("graph_model/gnn_layer_0", 3, film + lns + ["Dense/kernel"])
            + ["dense_1/kernel", "dense_1/bias"])
    assert sorted(got) == sorted(want)


def test_import_of_a_reference_style_pickle_with_missing_and_extra_variables(tmp_path, capsys):
    """models/sparse_graph_model.py:109-126 on a weights dict keyed like a TF1 checkpoint: '<name>:0' keys, Adam slot
    variables, one model variable missing (stays freshly initialised, reported), two entries the model does not own
    (reported, ignored)."""
    from tf_gnn_samples_amd.models import RGCN_Model
    task = _task()
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=2)
    src = RGCN_Model(dict(p, random_seed=1), task, device="cpu")
    src.optimizer.t = 7
    for m in src.optimizer.m:
        m.add_(0.25)
    path = tmp_path / "ref_best_model.pickle"
    src.save_model(str(path))
    saved = pickle.load(open(path, "rb"))["weights"]
    assert "graph_model/gnn_layer_0/Edge_0_Weight/kernel/Adam:0" in saved and "beta1_power:0" in saved
    assert abs(float(saved["beta1_power:0"]) - 0.9 ** 8) < 1e-7
    missing = "graph_model/gnn_layer_1/Edge_2_Weight/kernel:0"
    del saved[missing]
    saved["graph_model/gnn_layer_5/Edge_0_Weight/kernel:0"] = np.zeros((16, 16), np.float32)
    saved["total_num_graphs:0"] = np.int64(123)
    dst = RGCN_Model(dict(p, random_seed=2), task, device="cpu")
    fresh = dst.variables[missing[:-2]].detach().clone()
    capsys.readouterr()
    dst.load_weights(saved)
    out = capsys.readouterr().out
    assert "Freshly initializing %s since no saved value was found." % missing[:-2] in out
    assert "Saved weights for graph_model/gnn_layer_5/Edge_0_Weight/kernel:0 not used by model." in out
    assert "Saved weights for total_num_graphs:0 not used by model." in out
    assert out.count("not used by model") == 2 and out.count("Freshly initializing") == 1
    for n in src.variables.names():
        if n + ":0" == missing:
            assert torch.equal(dst.variables[n], fresh)
        else:
            assert torch.equal(dst.variables[n], src.variables[n]), n
    assert dst.optimizer.t == 7 and all(torch.equal(a, b) for a, b in zip(dst.optimizer.m, src.optimizer.m))
    with pytest.raises(ValueError, match="shape mismatch"):
        dst.load_weights({"dense_1/bias:0": np.zeros(5, np.float32)})


@pytest.mark.parametrize("steps", [7, 800, 1500, 2500, 50000, 200000])
def test_checkpoint_round_trip_after_many_adam_steps(tmp_path, steps):
    """beta1_power = float32(0.9^(t+1)) is denormal after ~830 steps and exactly 0 after ~985 (TF's float32 variable
    underflows the same way): the step count must then come from beta2_power, and a checkpoint in which both have
    underflowed must still load (all bias corrections are 1 there)."""
    from tf_gnn_samples_amd.models import RGCN_Model
    task = _task()
    p = RGCN_Model.default_params()
    p.update(hidden_size=16, graph_num_layers=1)
    src = RGCN_Model(dict(p, random_seed=1), task, device="cpu")
    src.optimizer.t = steps
    path = tmp_path / "long_run_best_model.pickle"
    src.save_model(str(path))
    saved = pickle.load(open(path, "rb"))["weights"]
    dst = RGCN_Model(dict(p, random_seed=2), task, device="cpu")
    dst.load_weights(saved)
    t = dst.optimizer.t
    if steps <= 50000:
        # float32 rounding of the power limits the recovered count to ~1e-7 / (1 - beta) relative steps
        assert abs(t - steps) <= max(1, steps // 2000), (steps, t)
    else:
        assert t >= 80000           # both powers underflowed: any count whose bias corrections are 1
    lr_t = lambda n: np.sqrt(1 - 0.999 ** n) / (1 - 0.9 ** n)
    assert abs(lr_t(max(t, 1)) - lr_t(steps)) < 1e-4


def test_metrics_readback_on_host_values():
    """MetricsReadback: host-resident metrics (CPU model) pass straight through; get() is idempotent."""
    import torch
    from tf_gnn_samples_amd.models.sparse_graph_model import MetricsReadback
    rb = MetricsReadback({"loss": torch.tensor(1.5), "f1": torch.tensor(0.25, dtype=torch.float64), "n": 7})
    assert rb.get() == {"loss": 1.5, "f1": 0.25, "n": 7}
    assert rb.get() == {"loss": 1.5, "f1": 0.25, "n": 7}


def test_split_plan_virtual_rows_cpu():
    """ops.SplitPlan is pure index arithmetic: chunked virtual rows of long buckets, checked without a GPU."""
    import torch
    from tf_gnn_samples_amd.ops import SplitPlan
    rowptr = torch.tensor([0, 0, 5, 5, 10005, 10006, 10006], dtype=torch.int32)
    sp = SplitPlan(rowptr, 1, 6, chunk=4096)
    assert sp.num_virtual == 8
    assert sp.virtual_rowptr.tolist() == [0, 0, 5, 5, 4101, 8197, 10005, 10006, 10006]
    assert sp.combine_rowptr.tolist() == [0, 1, 2, 3, 6, 7, 8]
    assert sp.lengths.tolist() == [0, 5, 0, 10000, 1, 0]
    merged = SplitPlan(rowptr, 2, 3, chunk=4096)
    assert merged.virtual_rowptr.tolist() == [0, 5, 4101, 8197, 10005, 10006]
    assert merged.combine_rowptr.tolist() == [0, 1, 4, 5]
    # every message belongs to exactly one virtual row, in order
    v = sp.virtual_rowptr
    assert (v[1:] >= v[:-1]).all() and v[0] == 0 and v[-1] == rowptr[-1]
    assert int((v[1:] - v[:-1]).max()) <= 4096


def test_late_fetch_hands_back_the_previous_item():
    """readback.LateFetch alone: put() fetches the item before, flush() the last one; a fetch that raises leaves nothing pending."""
    from tf_gnn_samples_amd.models.readback import LateFetch
    fetched = []
    late = LateFetch(lambda item: (fetched.append(item), "got %s" % item)[1])
    assert late.put("item 0") is None and fetched == []
    assert late.put("item 1") == "got item 0"
    assert late.put("item 2") == "got item 1"
    assert late.flush() == "got item 2" and late.flush() is None
    assert fetched == ["item 0", "item 1", "item 2"]

    def failing(item):
        fetched.append(item)
        raise RuntimeError(item)
    late = LateFetch(failing)
    late.put("item 3")
    with pytest.raises(RuntimeError, match="item 3"):
        late.put("item 4")
    assert late.flush() is None and fetched[3:] == ["item 3"]          # item 4 was dropped unread, as by a loop that the exception ends


def test_the_status_word_hand_off_without_a_gpu():
    from tf_gnn_samples_amd import ops
    nobody = torch.device("cuda", 63)               # (naming a device initialises nothing)
    assert ops.handover_word_if_any(nobody) is None
    assert ops.report_handover(0, nobody) is None
    with pytest.raises(ops.HandoverError, match=r"gave up on an LDS hand-over \(status 0xc: product matrix wave product producer wave\): "
                                                r"the results of that launch are wrong"):
        ops.report_handover(12, nobody)
    assert ops.handover_word_if_any(nobody) is None                    # still nothing allocated


def test_the_driver_module_exports_the_moved_classes_themselves():
    from tf_gnn_samples_amd.models import data_parallel, optimizer, readback, sparse_graph_model as sgm
    assert sgm.TFStyleOptimizer is optimizer.TFStyleOptimizer and optimizer.TFStyleOptimizer.__module__ == optimizer.__name__
    assert sgm.MetricsReadback is readback.MetricsReadback and readback.MetricsReadback.__module__ == readback.__name__
    assert sgm._PredictionArena is readback._PredictionArena and readback._PredictionArena.__module__ == readback.__name__
    assert sgm.CapturedTrainStep.__module__ == sgm.__name__ and sgm.Sparse_Graph_Model.__module__ == sgm.__name__
    assert data_parallel._DataParallel.__module__ == data_parallel.__name__
    import tf_gnn_samples_amd.graph as graph
    assert sgm.as_rel_graph is graph.as_rel_graph
