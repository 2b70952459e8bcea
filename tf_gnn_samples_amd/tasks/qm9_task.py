"""QM9 task mirror (tasks/qm9_task.py): jsonl.gz loader (:86-147), batch builder (:200-261) and the
gated-regression head with per-graph unsorted_segment_sum pooling (:150-197) — the second user of the
segment-sum kernel in the reference.

Edge types (defaults add_self_loop_edges=True, tie_fwd_bkwd_edges=True): type 0 = self loops, types 1..4 = bond
types with both directions in one list (:114-133); each graph's adjacency lists are SORTED (:135).

The head has two routes (config.settings.qm9_head): `compose`, the reference's op chain per task id (any device, any shape), and
`fused`, one HIP kernel pair for all task ids of the batch (csrc/qm9_head.hip) on GPU tensors of a shape the kernels take; ROUTES
says which one the last call took."""
import gzip
import json
from typing import Any, Dict, Iterator, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib, config, ops
from ..dense import dense
from ..graph import _PENDING_CHECKS
from .sparse_graph_task import DataFold, MinibatchData, Sparse_Graph_Task


class QM9GraphSample(NamedTuple):
    adjacency_lists: List[np.ndarray]
    type_to_node_to_num_incoming_edges: np.ndarray
    node_features: List[List[float]]
    target_values: List[float]


ROUTES = {"head": None}                                 # which implementation the last call took: "hip" or "composition"

_NOT_SORTED = "graph_nodes_list is not non-decreasing (a node's graph id is smaller than its predecessor's)"


def _err_flag(device, num_graphs: int) -> torch.Tensor:
    """A fresh device word for the kernel's check of graph_nodes_list, read back with the graphs' own at the next metric fetch."""
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    _PENDING_CHECKS.append((flag, {_lib.ERRFLAG_INDEX_OUT_OF_RANGE: "graph_nodes_list holds a graph id outside [0, %d)" % num_graphs,
                                   _lib.ERRFLAG_NOT_SORTED: _NOT_SORTED}))
    return flag


def _pointer_table(tensors):
    """Host array of device pointers (the C ABI hands them to the kernel by value)."""
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[_lib.ptr(t) for t in tensors])


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().reshape(-1).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _Head(torch.autograd.Function):
    """(loss, total_loss, abs_err [T], y [T, G]) of one batch for all T tasks: csrc/qm9_head.hip, one wave per graph.
    loss and total_loss are differentiable.  abs_err and y are marked non-differentiable: nothing in the package back-propagates
    through them (the reference's train step differentiates `loss` alone), and a gradient asked of them is an error instead of a
    silent zero.  variables = w_reg, b_reg, w_gate, b_gate of task 0, then of task 1, ..."""

    @staticmethod
    def forward(ctx, states, features, graph_nodes_list, targets, num_graphs, *variables):
        num_tasks = len(variables) // 4
        if states.stride(1) != 1 or states.stride(0) % 4 != 0 or states.data_ptr() % 16 != 0:
            states = states.contiguous()
        if features.stride(1) != 1:
            features = features.contiguous()
        num_nodes, hidden = states.shape
        annotation_size = features.shape[1]
        ld = states.stride(0) if num_nodes > 1 else hidden
        ldf = features.stride(0) if num_nodes > 1 else annotation_size
        flat = [_aligned(v) for v in variables]
        tables = [_pointer_table(flat[k::4]) for k in range(4)]
        targets = targets.contiguous()
        device = states.device
        y = torch.empty((num_tasks, num_graphs), dtype=torch.float32, device=device)
        node_range = torch.empty((num_graphs, 2), dtype=torch.int32, device=device)
        stats = torch.empty(num_tasks + 2, dtype=torch.float32, device=device)
        _lib.launch("relgnn_qm9_head_fwd", _lib.ptr(states, rows_strided=True), ld, _lib.ptr(features, rows_strided=True), ldf,
                    _lib.ptr(graph_nodes_list), num_nodes, num_graphs, hidden, annotation_size, num_tasks, *tables, _lib.ptr(targets),
                    _lib.ptr(y), _lib.ptr(node_range), _lib.ptr(stats), _lib.ptr(_err_flag(device, num_graphs)))
        ctx.save_for_backward(states, features, graph_nodes_list, targets, y, node_range, *flat)
        ctx.shapes = [tuple(v.shape) for v in variables]
        ctx.num_graphs = num_graphs
        ctx.set_materialize_grads(False)
        loss, total_loss, abs_err = stats[num_tasks], stats[num_tasks + 1], stats[:num_tasks]
        ctx.mark_non_differentiable(abs_err, y)
        return loss, total_loss, abs_err, y

    @staticmethod
    def backward(ctx, g_loss, g_total, g_abs_err, g_y):
        lib = _lib.load_library()
        states, features, graph_nodes_list, targets, y, node_range, *flat = ctx.saved_tensors
        num_tasks = len(flat) // 4
        if g_loss is None and g_total is None:
            return (None,) * (5 + len(flat))

        def scalar(g):                                  # the incoming gradients stay on the device: the kernel reads them
            return None if g is None else g.reshape(1).to(torch.float32).contiguous()
        g_loss, g_total = scalar(g_loss), scalar(g_total)
        num_nodes, hidden = states.shape
        annotation_size = features.shape[1]
        ld = states.stride(0) if num_nodes > 1 else hidden
        ldf = features.stride(0) if num_nodes > 1 else annotation_size
        device = states.device
        d_states = torch.empty((num_nodes, hidden), dtype=torch.float32, device=device)
        d_features = torch.empty((num_nodes, annotation_size), dtype=torch.float32, device=device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(v) for v in flat]     # one buffer per variable: the kernel writes each gradient where it stays
        nbytes = lib.relgnn_qm9_head_workspace_bytes(num_nodes, num_tasks, hidden, annotation_size)
        ws = _lib.scratch(nbytes, device)
        _lib.launch("relgnn_qm9_head_bwd", _lib.ptr(states, rows_strided=True), ld, _lib.ptr(features, rows_strided=True), ldf,
                    _lib.ptr(graph_nodes_list), num_nodes, ctx.num_graphs, hidden, annotation_size, num_tasks,
                    *[_pointer_table(flat[k::4]) for k in range(4)], _lib.ptr(targets), _lib.ptr(y), _lib.ptr(node_range), _lib.ptr(g_loss),
                    _lib.ptr(g_total), _lib.ptr(d_states), hidden, _lib.ptr(d_features), *[_pointer_table(grads[k::4]) for k in range(4)],
                    _lib.ptr(ws), nbytes)
        return (d_states, d_features, None, None, None) + tuple(g.reshape(s) for g, s in zip(grads, ctx.shapes))


def head_supported(num_tasks: int, hidden: int, annotation_size: int) -> bool:
    return bool(_lib.load_library().relgnn_qm9_head_supported(int(num_tasks), int(hidden), int(annotation_size)))


def qm9_head(states: torch.Tensor, features: torch.Tensor, graph_nodes_list: torch.Tensor, targets: torch.Tensor, num_graphs: int,
             variables):
    """-> (loss, total_loss, abs_err [T], y [T, G]) on the HIP route: float32 device states [V, hidden] and features [V, A], int32
    non-decreasing graph_nodes_list [V], float32 targets [T, G]; variables = [(w_reg, b_reg, w_gate, b_gate), ...] per task."""
    return _Head.apply(states, features, graph_nodes_list, targets, int(num_graphs), *[v for task in variables for v in task])


class QM9_Task(Sparse_Graph_Task):
    # tasks/qm9_task.py:22-26
    CHEMICAL_ACC_NORMALISING_FACTORS = [0.066513725, 0.012235489, 0.071939046,
                                        0.033730778, 0.033486113, 0.004278493,
                                        0.001330901, 0.004165489, 0.004128926,
                                        0.00409976, 0.004527465, 0.012292586,
                                        0.037467458]

    @classmethod
    def default_params(cls):
        params = super().default_params()
        params.update({
            'task_ids': [0],
            'add_self_loop_edges': True,
            'tie_fwd_bkwd_edges': True,
            'use_graph': True,
            'activation_function': "tanh",
            'out_layer_dropout_keep_prob': 1.0,
        })
        return params

    @staticmethod
    def name() -> str:
        return "QM9"

    @staticmethod
    def default_data_path() -> str:
        return "data/qm9"

    def __init__(self, params: Dict[str, Any]):
        super().__init__(params)
        self.__num_edge_types = 0
        self.__annotation_size = 0

    def get_metadata(self) -> Dict[str, Any]:
        return {'num_edge_types': self.__num_edge_types, 'annotation_size': self.__annotation_size}

    def restore_from_metadata(self, metadata: Dict[str, Any]) -> None:
        self.__num_edge_types = metadata['num_edge_types']
        self.__annotation_size = metadata['annotation_size']

    @property
    def num_edge_types(self) -> int:
        return self.__num_edge_types

    @property
    def initial_node_feature_size(self) -> int:
        return self.__annotation_size

    # -------------------- Data Loading --------------------
    @staticmethod
    def read_jsonl_gz(path: str, max_graphs: Optional[int] = None) -> List[dict]:
        out = []
        with gzip.open(path, "rt") as f:
            for line in f:
                out.append(json.loads(line))
                if max_graphs is not None and len(out) >= max_graphs:
                    break
        return out

    def load_data(self, path: str, max_graphs: Optional[int] = None) -> None:
        import os
        for fold, fname in ((DataFold.TRAIN, "train.jsonl.gz"), (DataFold.VALIDATION, "valid.jsonl.gz")):
            p = os.path.join(path, fname)
            if os.path.exists(p):
                self._loaded_data[fold] = self.load_raw(self.read_jsonl_gz(p, max_graphs))

    def load_eval_data_from_path(self, path: str):
        return self.load_raw(self.read_jsonl_gz(path))

    def load_raw(self, data: List[dict]) -> List[QM9GraphSample]:
        """tasks/qm9_task.py:86-112."""
        num_fwd_edge_types = 0
        for g in data:
            num_fwd_edge_types = max(num_fwd_edge_types, max([e[1] for e in g['graph']]))
        if self.params['add_self_loop_edges']:
            num_fwd_edge_types += 1
        self.__num_edge_types = max(self.__num_edge_types,
                                    num_fwd_edge_types * (1 if self.params['tie_fwd_bkwd_edges'] else 2))
        self.__annotation_size = max(self.__annotation_size, len(data[0]["node_features"][0]))
        return [QM9GraphSample(*self._graph_to_adjacency_lists(d['graph'], len(d["node_features"])),
                               node_features=d["node_features"],
                               target_values=[d["targets"][task_id][0] for task_id in self.params['task_ids']])
                for d in data]

    def _graph_to_adjacency_lists(self, graph, num_nodes: int):
        """tasks/qm9_task.py:114-147: raw triples (src, bond type e in 1..4, dst)."""
        L = self.__num_edge_types
        lists = [[] for _ in range(L)]
        deg = np.zeros((L, num_nodes))
        for src, e, dest in graph:
            t = e if self.params['add_self_loop_edges'] else e - 1
            lists[t].append((src, dest))
            deg[t, dest] += 1
            if self.params['tie_fwd_bkwd_edges']:
                lists[t].append((dest, src))
                deg[t, src] += 1
        if self.params['add_self_loop_edges']:
            for node in range(num_nodes):
                deg[0, node] = 1
                lists[0].append((node, node))
        adj = [np.array(sorted(a), dtype=np.int32) if len(a) > 0 else np.zeros((0, 2), dtype=np.int32) for a in lists]
        if not self.params['tie_fwd_bkwd_edges']:
            half = L // 2
            adj = adj[:half]
            for t, a in enumerate(list(adj)):
                adj.append(np.array(sorted((y, x) for (x, y) in a), dtype=np.int32).reshape(-1, 2))
                for (x, y) in a:
                    # Reference behaviour kept bit for bit (tasks/qm9_task.py:144-145): the count goes to y, the target
                    # of the FORWARD edge, although the reversed edge (y -> x) lands on x.  So with
                    # tie_fwd_bkwd_edges=False the backward types' table is NOT the true in-degree of their adjacency
                    # lists; it only reaches layers that normalise by it (RGCN default, FiLM/Edge-MLP when asked).
                    deg[half + t][y] += 1
        return adj, deg

    # -------------------- Output head (tasks/qm9_task.py:150-197) --------------------
    def output_variables(self, hidden_size: int):
        specs = {}
        for task_id in self.params['task_ids']:
            s = "out_layer_task%i" % task_id
            specs[s + "/regression_gate/dense/kernel"] = ((hidden_size + self.__annotation_size, 1), "glorot_uniform")
            specs[s + "/regression_gate/dense/bias"] = ((1,), "zeros")
            specs[s + "/regression/dense/kernel"] = ((hidden_size, 1), "glorot_uniform")
            specs[s + "/regression/dense/bias"] = ((1,), "zeros")
        return specs

    def _fused_head_applies(self, final_node_representations: torch.Tensor, batch, targets) -> bool:
        features = batch.initial_node_features
        return (config.settings.qm9_head == "fused" and final_node_representations.is_cuda and features.is_cuda
                and final_node_representations.dtype == torch.float32 and features.dtype == torch.float32
                and torch.is_tensor(targets) and targets.dtype == torch.float32
                and batch.graph_nodes_list.dtype == torch.int32 and batch.num_graphs >= 1 and final_node_representations.dim() == 2
                and head_supported(len(self.params['task_ids']), final_node_representations.shape[1], features.shape[1]))

    def _fused_head_variables(self, weights):
        variables = []
        for task_id in self.params['task_ids']:
            w = weights.scope("out_layer_task%i" % task_id) if hasattr(weights, "scope") else weights
            variables.append((w["regression/dense/kernel"], w["regression/dense/bias"],
                              w["regression_gate/dense/kernel"], w["regression_gate/dense/bias"]))
        return variables

    def _per_graph_outputs(self, final_node_representations: torch.Tensor, batch, w) -> torch.Tensor:
        """The composition's readout of ONE task (:163-187): gated per-node regression, summed per graph -> [G]."""
        # (dense(): the [hidden, 1] weight gradients go through the streaming kernel — as plain `@` autograd handed
        # them to the library as [V, hidden]^T @ [V, 1] products, 191 us each on a 50 k-node batch)
        per_node_outputs = dense(final_node_representations, w["regression/dense/kernel"], w["regression/dense/bias"])
        gate_input = torch.cat([final_node_representations, batch.initial_node_features], dim=-1)
        gate = torch.sigmoid(dense(gate_input, w["regression_gate/dense/kernel"], w["regression_gate/dense/bias"]))
        per_node_gated_outputs = gate * per_node_outputs
        # Sum up all nodes per graph: the HIP segment-sum kernel (2nd call-site family, :185-187)
        return ops.unsorted_segment_sum(per_node_gated_outputs, batch.graph_nodes_list, batch.num_graphs).squeeze(-1)

    # -------------------- Predictions: the molecule's value per task id --------------------
    def prediction_layout(self, batch, hidden_size: int):
        return {"values": ((int(batch.num_graphs), len(self.params['task_ids'])), torch.float32)}

    def compute_task_predictions(self, final_node_representations: torch.Tensor, batch, weights, out=None) -> Dict[str, torch.Tensor]:
        """values float32 [G, len(task_ids)] in task_ids order: the per-graph outputs the head's errors are taken of, on the route
        compute_task_metrics takes (config.settings.qm9_head).  The batch's targets are not read: the fused kernel pair computes its
        outputs next to a loss against zeros, which is dropped."""
        num_graphs, task_ids = batch.num_graphs, self.params['task_ids']
        device = final_node_representations.device
        zeros = torch.zeros((len(task_ids), num_graphs), dtype=torch.float32, device=device)
        use_hip = self._fused_head_applies(final_node_representations, batch, zeros)
        ROUTES["head"] = "hip" if use_hip else "composition"
        if use_hip:
            y = qm9_head(final_node_representations.detach(), batch.initial_node_features, batch.graph_nodes_list, zeros, num_graphs,
                         [tuple(v.detach() for v in task) for task in self._fused_head_variables(weights)])[3]
        else:
            y = torch.stack([self._per_graph_outputs(final_node_representations,
                                                     batch, weights.scope("out_layer_task%i" % t) if hasattr(weights, "scope") else weights)
                             for t in task_ids]).detach()
        values = y.t()                                                           # [G, tasks]
        if out is not None and out.get("values") is not None:
            out["values"].copy_(values)
            values = out["values"]
        return {"values": values}

    def compute_task_metrics(self, final_node_representations: torch.Tensor, batch, weights) -> Dict[str, torch.Tensor]:
        metrics = {}
        losses = []
        num_graphs = batch.num_graphs
        targets = batch.extra['target_values']                                   # [tasks, G]
        task_ids = self.params['task_ids']
        features = batch.initial_node_features
        use_hip = self._fused_head_applies(final_node_representations, batch, targets)
        ROUTES["head"] = "hip" if use_hip else "composition"
        if use_hip:
            variables = self._fused_head_variables(weights)
            loss, total_loss, abs_err, _ = qm9_head(final_node_representations, features, batch.graph_nodes_list, targets, num_graphs,
                                                    variables)
            for internal_id, task_id in enumerate(task_ids):
                metrics['abs_err_task%i' % task_id] = abs_err[internal_id]
            metrics['loss'] = loss
            metrics['total_loss'] = total_loss
            return metrics
        for internal_id, task_id in enumerate(self.params['task_ids']):
            w = weights.scope("out_layer_task%i" % task_id) if hasattr(weights, "scope") else weights
            per_graph_outputs = self._per_graph_outputs(final_node_representations, batch, w)
            per_graph_errors = per_graph_outputs - targets[internal_id, :]
            metrics['abs_err_task%i' % task_id] = per_graph_errors.abs().sum()
            losses.append((0.5 * per_graph_errors ** 2).mean())
        metrics['loss'] = torch.stack(losses).sum()
        metrics['total_loss'] = metrics['loss'] * float(num_graphs)
        return metrics

    NODE_PAYLOADS = {"initial_node_features": ("node_features", np.float32)}
    GRAPH_PAYLOADS = {"target_values": ("target_values", np.float32)}

    def _finish_native_batch(self, batch):
        batch.extra['target_values'] = batch.extra['target_values'].t()          # [tasks, G] (:254)
        return batch

    # -------------------- Minibatching (tasks/qm9_task.py:200-261) --------------------
    def make_minibatch_iterator(self, data: List[QM9GraphSample], data_fold: DataFold, max_nodes_per_batch: int,
                                rng: Optional[np.random.RandomState] = None) -> Iterator[MinibatchData]:
        if data_fold == DataFold.TRAIN:
            (rng or np.random).shuffle(data)
            out_keep = self.params['out_layer_dropout_keep_prob']
        else:
            out_keep = 1.0
        i = 0
        while i < len(data):
            start, node_offset, offsets = i, 0, []
            while i < len(data) and node_offset + len(data[i].node_features) < max_nodes_per_batch:
                offsets.append(node_offset)
                node_offset += len(data[i].node_features)
                i += 1
            if i == start:
                raise ValueError("graph %d does not fit max_nodes_per_batch=%d" % (i, max_nodes_per_batch))
            chunk = data[start:i]
            adjacency, num_edges = [], 0
            for l in range(self.num_edge_types):
                a = np.concatenate([np.asarray(g.adjacency_lists[l]).reshape(-1, 2) + off for g, off in zip(chunk, offsets)])
                a = a.astype(np.int32) if a.shape[0] else np.zeros((0, 2), dtype=np.int32)
                num_edges += a.shape[0]
                adjacency.append(a)
            feed = {
                'initial_node_features': np.concatenate([np.asarray(g.node_features, dtype=np.float32) for g in chunk], axis=0),
                'type_to_num_incoming_edges': np.concatenate([g.type_to_node_to_num_incoming_edges for g in chunk], axis=1),
                'graph_nodes_list': np.concatenate([np.full([len(g.node_features)], k, dtype=np.int32)
                                                    for k, g in enumerate(chunk)]),
                'target_values': np.transpose(np.array([g.target_values for g in chunk], dtype=np.float32), axes=[1, 0]),
                'out_layer_dropout_keep_prob': out_keep,
                'adjacency_lists': adjacency,
            }
            yield MinibatchData(feed_dict=feed, num_graphs=len(chunk), num_nodes=node_offset, num_edges=num_edges)

    def loss_weight(self, num_graphs: int, num_nodes: int) -> float:
        return float(num_graphs)             # the loss is a mean over the batch's graphs (compute_task_metrics)

    def early_stopping_metric(self, task_metric_results, num_graphs: int) -> float:
        return float(np.sum([float(m['total_loss']) for m in task_metric_results]) / num_graphs)

    def pretty_print_epoch_task_metrics(self, task_metric_results, num_graphs: int) -> str:
        maes = {t: 0.0 for t in self.params['task_ids']}
        for r in task_metric_results:
            for t in self.params['task_ids']:
                maes[t] += float(r['abs_err_task%i' % t]) / float(num_graphs)
        maes_str = " ".join("%i:%.5f" % (t, maes[t]) for t in self.params['task_ids'])
        err_str = " ".join("%i:%.5f" % (t, maes[t] / self.CHEMICAL_ACC_NORMALISING_FACTORS[t]) for t in self.params['task_ids'])
        return "MAEs: %s | Error Ratios: %s" % (maes_str, err_str)
