"""What tests/test_gpu_single_graph_dp.py shares with the ranks it spawns (a spawned process imports its target by module name, so
the worker lives in a module of its own): the synthetic citation graph, the model, and the worker of one rank."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
V, FEATURES, CLASSES, HIDDEN, NUM_VALID, NUM_TEST = 600, 16, 4, 32, 150, 100
REPLAY_GEMM = "torch"          # as in tests/test_gpu_dp_train.py: the route on which a batch's bits do not depend on the process's earlier batches

SAMPLED = {"fanouts": [3, 3], "seeds_per_batch": 16, "seed": 3}
EVALUATION = {"fanouts": [0, 0], "seeds_per_batch": 64}
SUBGRAPH = {"roots_per_batch": 16, "walk_length": 2, "seed": 3}
TASK_PARAMS = {
    "sampled": {"sampled_batches": dict(SAMPLED)},
    "layered": {"sampled_batches": dict(SAMPLED, layered=True)},
    "sampled_evaluation": {"sampled_batches": dict(SAMPLED, evaluation=EVALUATION)},
    "subgraph": {"subgraph_batches": dict(SUBGRAPH)},
    "subgraph_normalisation": {"subgraph_batches": dict(SUBGRAPH, normalisation={"presample_epochs": 2})},
}


def citation_task(kind: str, num_train: int, data_parallel: bool = True):
    """600 nodes, 16 features, 4 classes, THREE edge types (the synthetic graph's self loops and citations, and 900 random
    edges of a third type that the three folds share like the other two)."""
    from tf_gnn_samples_amd.tasks import Citation_Network_Task, DataFold
    params = {name: dict(value, **({"data_parallel": True} if data_parallel else {})) for name, value in TASK_PARAMS[kind].items()}
    task = Citation_Network_Task(dict(Citation_Network_Task.default_params(), out_layer_dropout_keep_prob=1.0, **params))
    task.load_synthetic(num_nodes=V, num_features=FEATURES, num_classes=CLASSES, num_train=num_train, num_valid=NUM_VALID,
                        num_test=NUM_TEST, feature_density=0.25, seed=4)
    third = np.random.default_rng(9).integers(0, V, size=(900, 2)).astype(np.int32)
    first = task._loaded_data[DataFold.TRAIN][0]
    adjacency = list(first.adjacency_lists) + [third]
    degrees = np.concatenate([first.type_to_node_to_num_incoming_edges, np.bincount(third[:, 1], minlength=V).astype(np.int32)[None]])
    for folds in (task._loaded_data[DataFold.TRAIN], task._loaded_data[DataFold.VALIDATION], task.synthetic_test_data):
        folds[0] = folds[0]._replace(adjacency_lists=adjacency, type_to_node_to_num_incoming_edges=degrees)
    task._Citation_Network_Task__num_edge_types = 3
    return task


def citation_model(task, device, result_dir, run_id="dp"):
    """RGCN, 2 layers of hidden size 32, nothing dropped anywhere."""
    from tf_gnn_samples_amd.models import RGCN_Model
    p = RGCN_Model.default_params()
    p.update(hidden_size=HIDDEN, graph_num_layers=2, graph_layer_input_dropout_keep_prob=1.0, random_seed=5, optimizer="Adam")
    return RGCN_Model(p, task, run_id=run_id, result_dir=str(result_dir), device=str(device))


def model_state(model):
    """Parameters, optimizer slots and step count as host arrays."""
    torch.cuda.synchronize()
    opt = model.optimizer
    return ([p.detach().cpu().numpy().copy() for p in opt.params],
            [t.detach().cpu().numpy().copy() for _, slots in opt._slots() for t in slots], opt.t)


def host_metrics(m):
    return {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in m.items()}


def worker(rank, world, port, q, kind, num_train, result_dir, refusals):
    """One rank: two epochs of train(group=WORLD) and test(group=WORLD) on cuda:0 over gloo, every epoch's result recorded; then,
    when asked, what stays refused."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    import tf_gnn_samples_amd.parallel as par
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.models import data_parallel as drivers
    from tf_gnn_samples_amd.tasks import DataFold
    r, local_rank, w = par.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    config.settings.gemm = REPLAY_GEMM                        # (this process ends with the test)
    epochs, reduced = [], []
    run_epoch, reduce_call = drivers._SingleGraphDataParallel.run_epoch, par.PackedGradientAllReducer.__call__

    def recording_epoch(self, epoch_name, data, data_fold, quiet=False):
        out = run_epoch(self, epoch_name, data, data_fold, quiet)
        epochs.append((epoch_name, out[0], [host_metrics(m) for m in out[1]], out[2]))
        return out

    def recording_call(self, scale):
        reduce_call(self, scale)
        reduced.append(self.flat.detach().cpu().numpy().copy())

    drivers._SingleGraphDataParallel.run_epoch = recording_epoch
    par.PackedGradientAllReducer.__call__ = recording_call
    task = citation_task(kind, num_train)
    model = citation_model(task, device, result_dir)
    model.train(quiet=True, max_epochs=2, group=dist.group.WORLD)
    params, slots, t = model_state(model)
    model.test(task.synthetic_test_data, quiet=True, group=dist.group.WORLD)
    out = dict(rank=rank, epochs=epochs, reduced=reduced, params=params, slots=slots, t=t, history=model.validation_history,
               counters=(task.batches.epoch, task.batches.draw), refusals=[])
    if refusals:
        def refused(what, fn):
            try:
                fn()
                out["refusals"].append((what, None))
            except Exception as e:
                out["refusals"].append((what, "%s: %s" % (type(e).__name__, e)))

        without = citation_model(citation_task(kind, num_train, data_parallel=False), device, result_dir, run_id="without")
        refused("without the key", lambda: without.train(quiet=True, max_epochs=1, group=dist.group.WORLD))
        with config.override(allreduce="overlap"):
            refused("overlap", lambda: model.train(quiet=True, max_epochs=1, group=dist.group.WORLD))
        train = task._loaded_data[DataFold.TRAIN]
        batch = next(iter(task.batches.rank_train_batches(train[0], rank, world)))
        refused("capture_train_step", lambda: model.capture_train_step(batch))
        refused("predict", lambda: model.predict(task.synthetic_test_data))
        refused("predict nodes", lambda: model.predict(task.synthetic_test_data, nodes=[1, 2, 3]))
        refused("iterator", lambda: list(task.make_minibatch_iterator(train, DataFold.TRAIN, 10)))
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()
