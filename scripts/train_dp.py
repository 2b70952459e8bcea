#!/usr/bin/env python
"""Data-parallel training by graph, one process per GPU (Sparse_Graph_Model.train(group=...)):

    python -m torch.distributed.run --nproc-per-node N scripts/train_dp.py MODEL TASK
        [--data-path P | --synthetic] [--model-param-overrides JSON] [--task-param-overrides JSON] [--max-epochs E]
        [--result-dir D] [--backend nccl|gloo] [--share-gpu]

init_distributed(), the task and the model through the registries, train(group=WORLD), then test(validation fold, group=WORLD).
--synthetic fills the folds of PPI / VarMisuse / the citation networks with generated graphs and those of QM9 with the 256 committed
molecules.  The citation task (cora, citeseer, pubmed) trains on ONE graph: it is accepted with sampled epochs and the key
"data_parallel", which deals the batches of an epoch out to the ranks, e.g.
    --task-param-overrides '{"sampled_batches": {"fanouts": [10, 10], "seeds_per_batch": 1024, "data_parallel": true}}'
(or "subgraph_batches": {"roots_per_batch": R, "walk_length": h, "data_parallel": true}); without the key it is refused before
anything is loaded, with the reason.
--share-gpu puts every rank on cuda:0 over gloo: a rehearsal of the protocol on a box with one GPU, not a speed.
An example and the thing a leased node runs, not a command-line interface of the package."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import torch.distributed as dist

from tf_gnn_samples_amd.models import name_to_model_class
from tf_gnn_samples_amd.parallel import init_distributed
from tf_gnn_samples_amd.tasks import DataFold, name_to_task_class

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("model")
ap.add_argument("task")
ap.add_argument("--data-path")
ap.add_argument("--synthetic", action="store_true")
ap.add_argument("--model-param-overrides", default="{}")
ap.add_argument("--task-param-overrides", default="{}")
ap.add_argument("--max-epochs", type=int)
ap.add_argument("--result-dir", default="trained_models")
ap.add_argument("--backend", choices=["nccl", "gloo"])
ap.add_argument("--share-gpu", action="store_true")
args = ap.parse_args()

if args.share_gpu:
    os.environ["LOCAL_RANK"] = "0"
rank, local_rank, world = init_distributed(backend="gloo" if args.share_gpu else args.backend)
device = torch.device("cuda", local_rank)
torch.cuda.set_device(device)

try:
    task_cls, task_extra = name_to_task_class(args.task)
except ValueError:                                         # (the name table is the reference's: VarMisuse is constructed directly)
    from tf_gnn_samples_amd.tasks import CHECKPOINT_TASK_CLASSES
    by_name = {k.lower(): v for k, v in CHECKPOINT_TASK_CLASSES.items()}
    if args.task.lower() not in by_name:
        raise
    task_cls, task_extra = by_name[args.task.lower()], {}
task_params = task_cls.default_params()
task_params.update(task_extra)
task_params.update(json.loads(args.task_param_overrides))
task = task_cls(task_params)
if world > 1 and task.name() == "CitationNetwork" and not task.single_graph_data_parallel():
    raise SystemExit('the citation task trains on ONE graph: under %d ranks it needs sampled epochs with the key "data_parallel", e.g. '
                     '--task-param-overrides \'{"sampled_batches": {"fanouts": [10, 10], "seeds_per_batch": 1024, "data_parallel": true}}\''
                     % world)
if args.synthetic:
    if hasattr(task, "load_synthetic"):
        task.load_synthetic()
    else:                                                  # QM9: the committed molecules, 192 to train on and 64 to validate
        import gzip
        with gzip.open(ROOT / "tests" / "golden" / "qm9_valid_256.jsonl.gz", "rt") as f:
            raw = [json.loads(line) for line in f]
        task._loaded_data[DataFold.TRAIN] = task.load_raw(raw[:192])
        task._loaded_data[DataFold.VALIDATION] = task.load_raw(raw[192:])
else:
    task.load_data(args.data_path or task.default_data_path())

model_cls, model_extra = name_to_model_class(args.model)
model_params = model_cls.default_params()
model_params.update(model_extra)
model_params.update(json.loads(args.model_param_overrides))
os.makedirs(args.result_dir, exist_ok=True)
run_id = "%s_%s_dp%d" % (task_cls.name(), model_cls.name(model_params), world)
model = model_cls(model_params, task, run_id=run_id, result_dir=args.result_dir, device=str(device))      # (after init_distributed)

group = dist.group.WORLD if world > 1 else None
model.train(quiet=True, max_epochs=args.max_epochs, group=group)
model.test(task._loaded_data[DataFold.VALIDATION], quiet=True, group=group)
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
