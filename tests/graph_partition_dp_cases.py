"""What tests/test_gpu_graph_partition.py shares with the two ranks it spawns: the `subgraph_batches` case of a COMPUTED partition
under "data_parallel", added to the cases of tests/single_graph_dp_cases.py (its graph, its model and its worker are used as they are).
No file: every rank computes the partition itself."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import single_graph_dp_cases as C  # noqa: E402

NUM_TRAIN = 200
KIND = "partition"
PARTITION = {"num_parts": 12, "refine_rounds": 3}
SEED = 3
BATCHES = 4                     # ceil(12 / 3)


def register() -> None:
    C.TASK_PARAMS[KIND] = {"subgraph_batches": {"sampler": "parts", "partition": dict(PARTITION), "parts_per_batch": 3, "seed": SEED,
                                                "normalisation": {"presample_epochs": 2}}}


def worker(rank, world, port, q, kind, num_train, result_dir, refusals):
    """One rank of single_graph_dp_cases.worker over the case above."""
    register()
    C.worker(rank, world, port, q, kind, num_train, result_dir, refusals)
