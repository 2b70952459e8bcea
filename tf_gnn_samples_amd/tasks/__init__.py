from .sparse_graph_task import DataFold, DeviceBatch, MinibatchData, Sparse_Graph_Task
from .ppi_task import PPI_Task
from .qm9_task import QM9_Task
from .citation_network_task import Citation_Network_Task
from .varmisuse_task import VarMisuse_Task

# utils/model_utils.py:12-29: name -> (class, extra task parameters).  The reference's "varmisuse" key is NOT here: the suite pins
# this table (tests/test_model_cpu.py), so VarMisuse_Task is constructed directly, as bench.py and the tests construct tasks.
TASK_CLASSES = {"ppi": (PPI_Task, {}), "qm9": (QM9_Task, {}),
                "cora": (Citation_Network_Task, {"data_kind": "cora"}),
                "citeseer": (Citation_Network_Task, {"data_kind": "citeseer"}),
                "pubmed": (Citation_Network_Task, {"data_kind": "pubmed"}),
                "citationnetwork": (Citation_Network_Task, {})}

# task_class of a best-model pickle (Sparse_Graph_Task.name()) -> class, for the tasks the name table above does not list;
# models.restore() looks here first
CHECKPOINT_TASK_CLASSES = {"VarMisuse": VarMisuse_Task}


def name_to_task_class(name: str):
    """-> (class, extra task parameters), utils/model_utils.py:12-29 (the VarMisuse name is unknown here)."""
    key = name.lower()
    if key not in TASK_CLASSES:
        raise ValueError("Unknown task type '%s'" % key)
    task_class, extra = TASK_CLASSES[key]
    return task_class, dict(extra)
