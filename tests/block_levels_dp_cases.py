"""What tests/test_gpu_block_levels.py shares with the two ranks it spawns (a spawned process imports its target by module name, so the
worker lives in a module of its own): the case "blocks" beside the cases of tests/single_graph_dp_cases.py, and that module's worker."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import single_graph_dp_cases as C  # noqa: E402

KIND = "blocks"
# layered TRAIN batches with derived levels, exact evaluation fields with derived levels: every batch of the run brings its graphs
C.TASK_PARAMS.setdefault(KIND, {"sampled_batches": dict(C.SAMPLED, layered=True, evaluation=dict(C.EVALUATION), blocks=True)})


def worker(*args):
    """single_graph_dp_cases.worker in a process that knows the case (the line above ran when the child imported this module)."""
    return C.worker(*args)
