"""Input contract of the hot path (mirror of tasks/sparse_graph_task.py:10-20,139-149).

A minibatch is ONE disjoint-union graph:
  initial_node_features       float32 [V, F]
  adjacency_lists             L x int32 [E_l, 2], rows = [source, target]
  type_to_num_incoming_edges  float32 [L, V]   (float despite the reference docstring, :144-145)
"""
from enum import Enum
from typing import Any, Dict, NamedTuple, Optional

import numpy as np
import torch


class DataFold(Enum):
    TRAIN = 0
    VALIDATION = 1
    TEST = 2


class MinibatchData(NamedTuple):
    feed_dict: Dict[str, Any]
    num_graphs: int
    num_nodes: int
    num_edges: int


class DeviceBatch:
    """The feed dict of one minibatch, resident in HBM (the reference copies host->device on every
    sess.run, models/sparse_graph_model.py:293; here it is done once, explicitly)."""

    def __init__(self, mb: MinibatchData, device, pin: bool = False):
        fd = mb.feed_dict
        self.num_graphs, self.num_nodes, self.num_edges = mb.num_graphs, mb.num_nodes, mb.num_edges

        def put(a, dtype):
            t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
            if pin and device != "cpu":
                t = t.pin_memory()
            return t.to(device, non_blocking=pin)

        # (a task with an input model of its own, tasks/varmisuse_task.py, feeds what that model reads instead)
        self.initial_node_features = put(fd['initial_node_features'], torch.float32) if 'initial_node_features' in fd else None
        self.adjacency_lists = [put(np.asarray(a).reshape(-1, 2), torch.int32) for a in fd['adjacency_lists']]
        self.type_to_num_incoming_edges = put(fd['type_to_num_incoming_edges'], torch.float32)
        self.graph_nodes_list = put(fd['graph_nodes_list'], torch.int32) if fd.get('graph_nodes_list') is not None else None
        self.extra = {k: v for k, v in fd.items() if k not in (
            'initial_node_features', 'adjacency_lists', 'type_to_num_incoming_edges', 'graph_nodes_list')}
        for k, v in list(self.extra.items()):
            if isinstance(v, np.ndarray):
                self.extra[k] = put(v, torch.float32 if v.dtype.kind == 'f' else torch.int64)

    @classmethod
    def from_tensors(cls, num_graphs, num_nodes, num_edges, initial_node_features, adjacency_lists,
                     type_to_num_incoming_edges, graph_nodes_list=None, extra=None) -> "DeviceBatch":
        """A batch whose tensors already live on the device (tasks/batcher.py: views of one uploaded arena)."""
        self = cls.__new__(cls)
        self.num_graphs, self.num_nodes, self.num_edges = int(num_graphs), int(num_nodes), int(num_edges)
        self.initial_node_features = initial_node_features
        # a zero-argument callable defers the lists (tasks/resident.py: the layers get the batch's bucketing, the lists are
        # gathered only if something reads them)
        self._adjacency = adjacency_lists if callable(adjacency_lists) else list(adjacency_lists)
        self.type_to_num_incoming_edges = type_to_num_incoming_edges
        self.graph_nodes_list = graph_nodes_list
        self.extra = dict(extra or {})
        return self

    @property
    def adjacency_lists(self):
        if callable(self._adjacency):
            self._adjacency = list(self._adjacency())
        return self._adjacency

    @adjacency_lists.setter
    def adjacency_lists(self, value):
        self._adjacency = value

    ready_event = None

    def wait_ready(self) -> "DeviceBatch":
        """A batch assembled on a side stream (tasks/resident.py) carries the event recorded behind its last kernel: make
        the CURRENT stream wait for it (no host sync) and tell the caching allocator that the batch's tensors are now
        used on this stream."""
        ev, self.ready_event = self.ready_event, None
        if ev is None:
            return self
        cur = torch.cuda.current_stream(self.initial_node_features.device)
        cur.wait_event(ev)
        tensors = [self.initial_node_features, self.type_to_num_incoming_edges, self.graph_nodes_list,
                   *([] if callable(self._adjacency) else self._adjacency),
                   *[v for v in self.extra.values() if torch.is_tensor(v)]]
        for t in tensors:
            if t is not None and t.is_cuda:
                t.record_stream(cur)
        for v in self.extra.values():                    # a feature container (tasks/sparse_features.py): a per-batch one records its tensors
            if not torch.is_tensor(v) and hasattr(v, "record_stream"):
                v.record_stream(cur)
        return self


class ModelRequirements(NamedTuple):
    """What a task's batches need from the model that runs them (Sparse_Graph_Task.model_requirements); the model checks each and
    raises the task's text with what it lacks in the place of %s."""
    layered: tuple = ()                         # ((fanouts, text), ...): batches with one level graph per layer for these fanouts
    message_scale: Optional[str] = None         # the text, when batches bring a per-message scale in the degree scale's place
    deferred_projection_rows: bool = False      # the input projection's weight is updated by the rows a batch names
    compact_projection_gradient: bool = False   # ... and its gradient exists only as those rows
    layerwise: Optional[str] = None             # the text, when evaluation batches run layer by layer over windows of target rows


class Sparse_Graph_Task:
    """Minimal task interface used by Sparse_Graph_Model (tasks/sparse_graph_task.py:23-254)."""

    @classmethod
    def default_params(cls):
        return {}

    @staticmethod
    def name() -> str:
        raise NotImplementedError()

    def __init__(self, params: Dict[str, Any]):
        self.params = params
        self._loaded_data = {}  # type: Dict[DataFold, Any]

    @property
    def num_edge_types(self) -> int:
        raise NotImplementedError()

    @property
    def initial_node_feature_size(self) -> int:
        raise NotImplementedError()

    def get_metadata(self) -> Dict[str, Any]:
        return {}

    def output_variable_scope(self, model_has_input_projection: bool) -> str:
        """Absolute TF variable scope of the task's output variables ("" = the graph's root scope)."""
        return ""

    # ---- a task-owned input model (make_task_input_model, tasks/sparse_graph_task.py:139-149; only VarMisuse has variables there) ----
    def input_variables(self) -> Dict[str, tuple]:
        """Variable specs (absolute names, the graph's root scope) of the task's input model, created BEFORE graph_model/..."""
        return {}

    def compute_initial_node_features(self, batch: "DeviceBatch", weights) -> torch.Tensor:
        """model_ops['initial_node_features'] of one batch; `weights` maps the names of input_variables() to the parameters."""
        return batch.initial_node_features

    # ---- predictions (Sparse_Graph_Model.predict): what the task's metric counts, per node or per graph ----
    PER_NODE_PREDICTIONS: tuple = ()                    # keys of compute_task_predictions whose rows are the batch's nodes

    def prediction_layout(self, batch: "DeviceBatch", hidden_size: int) -> Dict[str, tuple]:
        """key -> (shape, torch dtype) of what compute_task_predictions returns for this batch: the model lays one packed arena out
        by it and hands its views to the hook as `out`."""
        raise NotImplementedError("the %s task defines no predictions" % type(self).__name__)

    def compute_task_predictions(self, final_node_representations: torch.Tensor, batch: "DeviceBatch", weights,
                                 out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Batch-level predictions on the tensors' device, decided by the rules the task's metric counts by (predict.py).  Reads no
        label, target or mask of the batch and applies no dropout.  `out`: tensors of prediction_layout() to write into (optional)."""
        raise NotImplementedError("the %s task defines no predictions" % type(self).__name__)

    @staticmethod
    def num_nodes_of(sample) -> int:
        """Nodes of one data sample (what the batch builders count it as)."""
        return len(sample.node_features)

    def split_predictions(self, host_arrays: Dict[str, np.ndarray], batch, samples) -> list:
        """One dict per graph of the batch, in the batch's order: per-node arrays (PER_NODE_PREDICTIONS and 'node_states') are cut
        by each sample's node count, every other array is indexed by the graph.  The pieces are views of host_arrays."""
        counts = [int(self.num_nodes_of(s)) for s in samples]
        if len(samples) != int(batch.num_graphs):
            raise ValueError("split_predictions: %d samples for a batch of %d graphs" % (len(samples), int(batch.num_graphs)))
        if sum(counts) != int(batch.num_nodes):
            raise ValueError("split_predictions: the samples hold %d nodes, the batch %d" % (sum(counts), int(batch.num_nodes)))
        per_node = set(self.PER_NODE_PREDICTIONS) | {"node_states"}
        for key, a in host_arrays.items():
            want = int(batch.num_nodes) if key in per_node else len(samples)
            if a.shape[0] != want:
                raise ValueError("split_predictions: %r has %d rows, expected %d" % (key, a.shape[0], want))
        out, offset = [], 0
        for g, n in enumerate(counts):
            out.append({key: (a[offset:offset + n] if key in per_node else a[g]) for key, a in host_arrays.items()})
            offset += n
        return out

    # ---- native batching (tasks/batcher.py); tasks override the payload tables / post-processing ----
    NODE_PAYLOADS = {"initial_node_features": ("node_features", np.float32)}
    GRAPH_PAYLOADS: Dict[str, tuple] = {}

    def make_graph_store(self, data):
        """Flatten one data fold once for the C++ batch builder (include/relgnn.h section 9)."""
        from .batcher import GraphStore           # (cycle: batcher imports DeviceBatch from this module at its top)
        return GraphStore(data, self.num_edge_types, self.NODE_PAYLOADS, self.GRAPH_PAYLOADS)

    def _finish_native_batch(self, batch: "DeviceBatch") -> "DeviceBatch":
        return batch

    def make_native_minibatch_iterator(self, batcher, data_fold: DataFold, max_nodes_per_batch: int,
                                       rng: Optional[np.random.RandomState] = None):
        """Same batches as make_minibatch_iterator, assembled by relgnn_batch_pack and already on the device.
        TRAIN shuffles the graph order (the reference shuffles the data list in place, tasks/ppi_task.py:204-206)."""
        ids = np.arange(batcher.store.num_graphs)
        if data_fold == DataFold.TRAIN:
            (rng or np.random).shuffle(ids)
            batcher.constants['out_layer_dropout_keep_prob'] = self.params.get('out_layer_dropout_keep_prob', 1.0)
        else:
            batcher.constants['out_layer_dropout_keep_prob'] = 1.0
        for batch in batcher.iterate(ids, max_nodes_per_batch):
            yield self._finish_native_batch(batch)

    # ---- what the model driver asks a task with batching modes of its own (the citation task); the defaults ask for nothing ----
    def model_requirements(self) -> ModelRequirements:
        return ModelRequirements()

    def epoch_batches(self, data, data_fold: DataFold, device, full_graph_route: bool, full_graph: bool = False):
        """The batches of one epoch on `device` when the task cuts them itself, None for the general input pipelines.
        full_graph_route: would the model's full-graph batch of a single-graph fold be a resident one?  full_graph: predict(data)."""
        return None

    def epoch_result(self, result, data_fold: DataFold):
        """The result of an epoch (EpochTally.result) as the task reports it."""
        return result

    def check_prediction_nodes(self, data, nodes):
        raise ValueError("predict(nodes=...) is not defined for the %s task: its predictions are per graph of `data`, and only a "
                         "task whose data is ONE graph names single nodes" % self.name())

    def loss_weight(self, num_graphs: int, num_nodes: int) -> float:
        """The normaliser of the task's loss for a batch of that many graphs and nodes: what the batch weighs in the mean over a
        data-parallel step (parallel.dp_schedule).  A task that trains under train(group=...) says which one it divides by."""
        raise NotImplementedError("the %s task does not say what its loss is normalised by (loss_weight): it cannot be trained "
                                  "data-parallel" % type(self).__name__)

    def single_graph_data_parallel(self) -> bool:
        """Does the task train its ONE graph data-parallel, by handing the sampled batches of an epoch out to the ranks (the citation
        task's key "data_parallel")?  models/data_parallel.py asks this before loss_weight and then drives the epochs through the
        task's rank_epoch_batches, train_schedule and data_parallel_fingerprint."""
        return False

    def restore_from_metadata(self, metadata: Dict[str, Any]) -> None:
        pass
