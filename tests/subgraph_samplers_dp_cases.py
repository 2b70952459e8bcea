"""What tests/test_gpu_subgraph_samplers.py shares with the two ranks it spawns: the `subgraph_batches` cases of the node, edge and
partition samplers under "data_parallel", added to the cases of tests/single_graph_dp_cases.py (its graph, its model and its worker are
used as they are), and the partition file both ranks and the replay read."""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import single_graph_dp_cases as C  # noqa: E402

NUM_TRAIN = 200                 # of 600 nodes: a batch of 64 degree-proportional draws without a TRAIN node is out of the question
PARTS = 12
NORMALISATION = {"presample_epochs": 2}
BATCHES = {"node": 4, "edge": 4, "parts": 4}          # ceil(200 / 64), ceil(200 / 64), ceil(12 / 3)


def parts_path(result_dir) -> str:
    return str(Path(result_dir) / "parts.npy")


def write_parts(result_dir) -> None:
    np.save(parts_path(result_dir), (np.random.default_rng(12).permutation(C.V) % PARTS).astype(np.int32))


def register(result_dir) -> None:
    """The three cases under the names "node", "edge" and "parts" (the partition file lies in result_dir)."""
    C.TASK_PARAMS.update({
        "node": {"subgraph_batches": {"sampler": "node", "roots_per_batch": 64, "seed": 3, "normalisation": dict(NORMALISATION)}},
        "edge": {"subgraph_batches": {"sampler": "edge", "roots_per_batch": 64, "seed": 3, "normalisation": dict(NORMALISATION)}},
        "parts": {"subgraph_batches": {"sampler": "parts", "parts_path": parts_path(result_dir), "parts_per_batch": 3, "seed": 3,
                                       "normalisation": dict(NORMALISATION)}},
    })


def worker(rank, world, port, q, kind, num_train, result_dir, refusals):
    """One rank of single_graph_dp_cases.worker over one of the cases above."""
    register(result_dir)
    C.worker(rank, world, port, q, kind, num_train, result_dir, refusals)
