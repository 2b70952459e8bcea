"""Citation-network task mirror (tasks/citation_network_task.py, utils/citation_network_utils.py): full-graph masked node
classification on Cora / CiteSeer / PubMed in the Planetoid file layout.

ONE graph is always the whole batch: the three folds share the graph and the row-normalised features and differ in the per-node
class labels and the 0/1 node mask.  The output head is a bias-free Dense followed by a masked sparse softmax cross-entropy and an
accuracy count; on the GPU that is one kernel pair (csrc/train_utils.hip: relgnn_softmax_ce_stats / relgnn_softmax_ce_bwd).
Without the datasets `load_synthetic` fills the folds with a Cora-shaped graph.

Task parameter `sparse_node_features` (False by default; read with params.get, not part of default_params(), which is pinned against
the reference's): the features stay sparse from the file to the input projection.  The folds then share ONE tasks.sparse_features
.SparseRows under `node_features` (no dense [V, F] array is ever built), every device holds one copy of it, the input pipelines
carry a float32 [V, 1] stand-in under `initial_node_features`, and compute_initial_node_features hands the model the device's
SparseRows, which its input projection takes through ops.csr_rows_project (csrc/csr_project.hip).

The batching modes live in tasks/single_graph_batches.py (`self.batches`), which describes every parameter and key:
  `sampled_batches` {"fanouts", "seeds_per_batch", "seed"; optional "sparse_features", "sparse_update", "sparse_gradient", "layered",
      "evaluation", "blocks"}: TRAIN epochs of neighbour-sampled receptive fields; "evaluation": VALIDATION, TEST and predict(nodes=...) on them too.
  `subgraph_batches` {"roots_per_batch", "walk_length", "seed"; optional "sparse_features", "normalisation", "sampler"}: TRAIN epochs of
      random-walk induced subgraphs; "normalisation": GraphSAINT's loss and aggregation weights; "sampler": the node set from a node, edge
      or partition sampler instead of walks.
  Either takes the optional key "data_parallel": train(group=...) / test(group=...) deal the batches of an epoch out to the ranks.
"""
import os
import pickle
import weakref
from typing import Any, Dict, Iterator, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib, config as _cfg
from ..dense import dense, mark_zero_padded
from ..parallel import refuse_single_graph_task, single_graph_schedule
from ..predict import predict_softmax
from .layerwise import KeptBlocks, LayerwisePlan, check_layerwise_evaluation, parse_layerwise_evaluation
from .neighbour_sampling import PREDICT_SEEDS_PER_BATCH, check_prediction_nodes, check_sparse_node_features, parse_sampled_batches
from .subgraph_sampling import parse_subgraph_batches
from .resident import ResidentDataset
from .single_graph_batches import SingleGraphBatches
from .sparse_features import SparseRows, node_stand_in, random_rows, resident_copy
from .sparse_graph_task import DataFold, MinibatchData, ModelRequirements, Sparse_Graph_Task


class CitationData(NamedTuple):
    """One fold = the whole graph (the reference's CitationData, :12, under the attribute names tasks/batcher.py flattens)."""
    adjacency_lists: List[np.ndarray]                      # [self loops, both directions of every (node, neighbour)], int32 [E_l, 2]
    type_to_node_to_num_incoming_edges: np.ndarray         # int32 [2, V]
    node_features: Any                                     # float32 [V, F], row-normalised (sparse_node_features: a SparseRows)
    labels: np.ndarray                                     # int32 [V]
    mask: np.ndarray                                       # float32 [V], 1 = the node counts in this fold


class _SoftmaxCEStats(torch.autograd.Function):
    """(loss, total_loss, accuracy, [total_loss, sum of mask, masked correct count]) of the whole graph in one pass over the logits
    (csrc/train_utils.hip).  log_softmax, gather, mul, sum, argmax, eq, sum, div and their autograd mirrors would be a dozen ~5 us
    launches around a step that is launch-bound by construction (a few thousand nodes); see _SigmoidCEStats in ppi_task.py.
    With `weights` and `denominator` (relgnn_softmax_ce_weighted_stats / _bwd, include/relgnn_subgraph_norm.h): a weight per row and
    a denominator the caller names, loss = sum(mask * weight * loss_v) / denominator, total_loss the numerator; the accuracy and the
    counts behind it stay unweighted."""

    @staticmethod
    def forward(ctx, logits, labels, mask, weights=None, denominator=None):
        lib = _lib.load_library()
        if logits.dim() != 2 or logits.stride(1) != 1:
            logits = logits.contiguous()
        labels, mask = labels.contiguous(), mask.contiguous()
        rows, cols = logits.shape
        weighted = weights is not None
        name = "relgnn_softmax_ce_weighted_stats" if weighted else "relgnn_softmax_ce_stats"
        stats = torch.empty(6 if weighted else 5, dtype=torch.float32, device=logits.device)
        nbytes = getattr(lib, name + "_workspace_bytes")()
        ws = _lib.scratch(nbytes, logits.device)
        weights = weights.contiguous() if weighted else None
        _lib.launch(name, _lib.ptr(logits, rows_strided=True), logits.stride(0) if rows > 1 else cols, _lib.ptr(labels), _lib.ptr(mask),
                    *((_lib.ptr(weights), float(denominator)) if weighted else ()), rows, cols, _lib.ptr(stats), _lib.ptr(ws), nbytes)
        # (the plain backward divides by the sum of the mask, stats[1]; the weighted one takes the denominator as a launch scalar)
        ctx.save_for_backward(logits, labels, mask, weights if weighted else stats)
        ctx.denominator = float(denominator) if weighted else None
        ctx.set_materialize_grads(False)          # an unused output's gradient arrives as None, not as a zero tensor
        loss, total, accuracy = stats[3], stats[0], stats[4]
        counts = stats[0:3]                       # total_loss, sum of mask, masked correct count (the last two unweighted)
        ctx.mark_non_differentiable(accuracy, counts)
        return loss, total, accuracy, counts

    @staticmethod
    def backward(ctx, g_loss, g_total, g_accuracy, g_counts):
        logits, labels, mask, stats_or_weights = ctx.saved_tensors
        if g_loss is None and g_total is None:
            return None, None, None, None, None

        def scalar(g):                            # the incoming gradients stay on the device: the kernel reads them (and sum of mask)
            return None if g is None else g.reshape(1).to(torch.float32).contiguous()
        g_loss, g_total = scalar(g_loss), scalar(g_total)
        rows, cols = logits.shape
        ld = logits.stride(0) if rows > 1 else cols
        # padded: rows of the next multiple of 16 floats, zeros behind the classes: the head's input-gradient product then runs on the
        # limb route with the activation gradient of the last GNN layer's Dense in its epilogue (dense.mark_zero_padded), as PPI's
        padded = cols % 16 and _cfg.settings.limb_gemm and _cfg.settings.head_pad == "1"
        ldg = (cols + 15) // 16 * 16 if padded else cols
        gl = torch.empty((rows, ldg), dtype=torch.float32, device=logits.device)
        if ctx.denominator is None:
            _lib.launch("relgnn_softmax_ce_bwd", _lib.ptr(logits, rows_strided=True), ld, _lib.ptr(labels), _lib.ptr(mask), rows, cols,
                        _lib.ptr(stats_or_weights), _lib.ptr(g_loss), _lib.ptr(g_total), _lib.ptr(gl), ldg)
        else:
            _lib.launch("relgnn_softmax_ce_weighted_bwd", _lib.ptr(logits, rows_strided=True), ld, _lib.ptr(labels), _lib.ptr(mask),
                        _lib.ptr(stats_or_weights), ctx.denominator, rows, cols, _lib.ptr(g_loss), _lib.ptr(g_total), _lib.ptr(gl), ldg)
        return (mark_zero_padded(gl[:, :cols], ldg) if padded else gl), None, None, None, None


def softmax_ce_stats(logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor):
    """-> (loss, total_loss, accuracy, counts) of float32 device logits [V, C], int32 labels [V], float32 mask [V]."""
    return _SoftmaxCEStats.apply(logits, labels, mask)


def softmax_ce_weighted_stats(logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor, weights: torch.Tensor, denominator: float):
    """-> (loss, total_loss, accuracy, counts) of float32 device logits [V, C], int32 labels [V], float32 mask and weights [V]."""
    return _SoftmaxCEStats.apply(logits, labels, mask, weights, denominator)


# ---------------------------------------------------------------------------------------------------------------------------------
# Planetoid files (utils/citation_network_utils.py:25-90, :114-121)
# ---------------------------------------------------------------------------------------------------------------------------------
def load_planetoid(directory: str, data_kind: str):
    """ind.<kind>.{x,y,tx,ty,allx,ally,graph} + ind.<kind>.test.index -> (graph dict, feature matrix (scipy LIL), the three
    one-hot label tables restricted to their fold, the three boolean node masks), utils/citation_network_utils.py:25-90.

    The test rows are stored in the order of the sorted test ids and put where test.index says; the train fold is the first len(y)
    nodes, the validation fold the next 500.  CiteSeer's test ids have holes (isolated nodes the files leave out): those become
    all-zero feature rows and all-zero label rows."""
    import scipy.sparse as sp           # (the pickles hold scipy matrices; nothing else in the package needs scipy)
    loaded = {}
    for part in ("x", "y", "tx", "ty", "allx", "ally", "graph"):
        with open(os.path.join(directory, "ind.%s.%s" % (data_kind, part)), "rb") as f:
            loaded[part] = pickle.load(f, encoding="latin1")
    with open(os.path.join(directory, "ind.%s.test.index" % data_kind)) as f:
        test_ids = [int(line.strip()) for line in f]
    test_sorted = np.sort(test_ids)
    tx, ty = loaded["tx"], loaded["ty"]
    if data_kind == "citeseer":
        first, span = min(test_ids), max(test_ids) - min(test_ids) + 1
        tx_full = sp.lil_matrix((span, loaded["x"].shape[1]))
        tx_full[test_sorted - first, :] = tx
        ty_full = np.zeros((span, loaded["y"].shape[1]))
        ty_full[test_sorted - first, :] = ty
        tx, ty = tx_full, ty_full
    features = sp.vstack((loaded["allx"], tx)).tolil()
    features[test_ids, :] = features[test_sorted, :]
    labels = np.vstack((loaded["ally"], ty))
    labels[test_ids, :] = labels[test_sorted, :]
    num_nodes, num_train = labels.shape[0], len(loaded["y"])
    folds = (np.arange(num_train), np.arange(num_train, num_train + 500), test_sorted)
    masks, tables = [], []
    for ids in folds:
        m = np.zeros(num_nodes, dtype=bool)
        m[ids] = True
        t = np.zeros(labels.shape)
        t[m, :] = labels[m, :]
        masks.append(m)
        tables.append(t)
    return loaded["graph"], features, tables, masks


def row_normalise(features) -> np.ndarray:
    """utils/citation_network_utils.py:114-121: every row divided by its sum, in the matrix's own dtype; the reciprocal of a zero
    row sum counts as 0 (the row stays zero).  Returns the dense array."""
    import scipy.sparse as sp
    row_sum = np.array(features.sum(1))
    with np.errstate(divide="ignore"):
        reciprocal = np.power(row_sum, -1).flatten()
    reciprocal[np.isinf(reciprocal)] = 0.
    return sp.diags(reciprocal).dot(features).toarray()


def graph_to_edge_lists(graph: Dict[int, List[int]]):
    """:90-109.  Type 0: one self loop per node, in the dict's iteration order.  Type 1: for every (node, neighbour) of the dict in
    iteration order the rows (node, neighbour) and (neighbour, node); duplicates stay (the segment sums follow this order).
    -> ([self loops, edges] as int32 [E, 2], in-degree table int32 [2, V] = [ones, counts])."""
    num_nodes = len(graph)
    nodes = np.fromiter(graph.keys(), dtype=np.int64, count=num_nodes)
    lengths = np.fromiter((len(v) for v in graph.values()), dtype=np.int64, count=num_nodes)
    src = np.repeat(nodes, lengths)
    dst = np.fromiter((n for v in graph.values() for n in v), dtype=np.int64, count=int(lengths.sum()))
    edges = np.empty((2 * len(src), 2), dtype=np.int32)
    edges[0::2, 0], edges[0::2, 1] = src, dst
    edges[1::2, 0], edges[1::2, 1] = dst, src
    self_loops = np.stack([nodes, nodes], axis=1).astype(np.int32)
    counts = np.bincount(edges[:, 1], minlength=num_nodes).astype(np.int32)       # every pair adds one to either end
    return [self_loops, edges], np.stack([np.ones_like(counts), counts])


class Citation_Network_Task(Sparse_Graph_Task):
    @classmethod
    def default_params(cls):
        # :16-25
        params = super().default_params()
        params.update({
            'add_self_loop_edges': True,
            'use_graph': True,
            'activation_function': "tanh",
            'out_layer_dropout_keep_prob': 1.0,
        })
        return params

    @staticmethod
    def name() -> str:
        return "CitationNetwork"

    @staticmethod
    def default_data_path() -> str:
        return "data/citation-networks"

    def __init__(self, params: Dict[str, Any]):
        super().__init__(params)
        self._resident_batches = weakref.WeakKeyDictionary()      # resident fold -> its one assembled batch (released with the fold)
        self._device_rows = weakref.WeakKeyDictionary()           # host SparseRows -> {device: its one copy there}
        self.batches = SingleGraphBatches(self)                   # the sampled batches of every mode, their device, counters and caches
        self.subgraph_batches                                     # (a malformed parameter fails here, not in the first epoch)
        self.sampled_batches
        self.layerwise_evaluation
        self.__num_edge_types = 2
        self.__initial_node_feature_size = 0
        self.__num_output_classes = 0

    def get_metadata(self) -> Dict[str, Any]:
        metadata = {'params': self.params}          # (the reference's base class stores the task parameters here, sparse_graph_task.py:46-59)
        metadata['initial_node_feature_size'] = self.__initial_node_feature_size
        metadata['num_output_classes'] = self.__num_output_classes
        return metadata

    def restore_from_metadata(self, metadata: Dict[str, Any]) -> None:
        self.params = metadata.get('params', self.params)
        self.__initial_node_feature_size = metadata['initial_node_feature_size']
        self.__num_output_classes = metadata['num_output_classes']

    @property
    def sparse_node_features(self) -> bool:
        return bool(self.params.get('sparse_node_features', False))

    @property
    def sampled_batches(self) -> Optional[Dict[str, Any]]:
        """The validated `sampled_batches` parameter, None when the TRAIN fold is one full-graph batch."""
        sampled = parse_sampled_batches(self.params.get('sampled_batches'))
        if sampled is None:
            return None
        check_sparse_node_features("sampled_batches", sampled, self.sparse_node_features)
        return sampled

    @property
    def subgraph_batches(self) -> Optional[Dict[str, Any]]:
        """The validated `subgraph_batches` parameter, None when the TRAIN fold is not cut into random-walk subgraphs."""
        subgraph = parse_subgraph_batches(self.params.get('subgraph_batches'))
        if subgraph is None:
            return None
        if self.params.get('sampled_batches') is not None:
            raise ValueError("subgraph_batches cannot be combined with sampled_batches: a TRAIN epoch is cut into induced subgraphs "
                             "or into neighbour-sampled receptive fields, not both")
        check_sparse_node_features("subgraph_batches", subgraph, self.sparse_node_features)
        return subgraph

    @property
    def sparse_update(self) -> bool:
        """Does `sampled_batches` ask for the row-deferred update of the input projection's weight?"""
        sampled = self.sampled_batches
        return bool(sampled is not None and sampled.get("sparse_update", False))

    @property
    def sparse_gradient(self) -> bool:
        """Does `sampled_batches` ask for the compact gradient of the input projection's weight (on top of sparse_update)?"""
        sampled = self.sampled_batches
        return bool(sampled is not None and sampled.get("sparse_gradient", False))

    @property
    def layered(self) -> bool:
        """Does `sampled_batches` ask for hop-ordered batches whose layers run on the hops they need?"""
        sampled = self.sampled_batches
        return bool(sampled is not None and sampled.get("layered", False))

    @property
    def blocks(self) -> bool:
        """Does `sampled_batches` ask for level graphs derived from the union graph's bucketing, target rows only?"""
        sampled = self.sampled_batches
        return bool(sampled is not None and sampled.get("blocks", False))

    def single_graph_data_parallel(self) -> bool:
        """Does `sampled_batches` or `subgraph_batches` carry "data_parallel": true?"""
        return bool((self.sampled_batches or self.subgraph_batches or {}).get("data_parallel", False))

    @property
    def evaluation(self) -> Optional[Dict[str, Any]]:
        """The "evaluation" key of `sampled_batches` ({"fanouts", "seeds_per_batch"}, "keep" when given), None when VALIDATION, TEST and
        test() run on the full graph."""
        sampled = self.sampled_batches
        return None if sampled is None else sampled.get("evaluation")

    @property
    def layerwise_evaluation(self) -> Optional[Dict[str, Any]]:
        """The validated `layerwise_evaluation` parameter ({"rows_per_batch", "keep"}; tasks/layerwise.py), None when VALIDATION, TEST,
        test() and predict(data) run the full graph as one batch."""
        return check_layerwise_evaluation(parse_layerwise_evaluation(self.params.get('layerwise_evaluation')),
                                          parse_sampled_batches(self.params.get('sampled_batches')))

    def _layerwise_plan(self, fold, data_fold: DataFold) -> Optional[LayerwisePlan]:
        """What a full-graph batch of an evaluation fold carries under extra['layerwise_evaluation'], None for a TRAIN batch and
        without the parameter."""
        asked = self.layerwise_evaluation
        if asked is None or data_fold == DataFold.TRAIN:
            return None
        kept = KeptBlocks(self.batches.kept_layerwise, fold.labels) if asked["keep"] and fold is not None else None
        return LayerwisePlan(asked["rows_per_batch"], kept)

    @property
    def num_edge_types(self) -> int:
        return self.__num_edge_types

    @property
    def initial_node_feature_size(self) -> int:
        return self.__initial_node_feature_size

    @property
    def num_output_classes(self) -> int:
        return self.__num_output_classes

    # -------------------- Data (:63-109) --------------------
    def load_data(self, path: str) -> None:
        train, valid, _ = self._load_folds(path)
        self._loaded_data[DataFold.TRAIN] = train
        self._loaded_data[DataFold.VALIDATION] = valid

    def load_eval_data_from_path(self, path: str):
        return self._load_folds(path)[2]

    def _load_folds(self, path):
        data_path = getattr(path, "path", path)                       # (a RichPath-like object or a plain string)
        print(" Loading CitationNetwork data from %s." % (data_path,))
        graph, features, label_tables, masks = load_planetoid(data_path, self.params['data_kind'])
        self.__initial_node_feature_size = features.shape[1]
        self.__num_output_classes = label_tables[0].shape[1]
        if self.sparse_node_features:
            features = SparseRows.row_normalised(features)            # one container for the three folds; never dense
        else:
            # the reference feeds its array into a float32 placeholder: the cast happens once, here
            features = np.ascontiguousarray(row_normalise(features), dtype=np.float32)
        adjacency, degrees = graph_to_edge_lists(graph)
        return tuple([self._fold(adjacency, degrees, features, np.argmax(table, axis=1), mask)]
                     for table, mask in zip(label_tables, masks))

    @staticmethod
    def _fold(adjacency, degrees, features, labels, mask) -> CitationData:
        # (the reference feeds a bool mask into a float32 placeholder, :117)
        return CitationData(adjacency_lists=adjacency, type_to_node_to_num_incoming_edges=degrees, node_features=features,
                            labels=np.ascontiguousarray(labels, dtype=np.int32), mask=np.ascontiguousarray(mask, dtype=np.float32))

    def load_synthetic(self, num_nodes: int = 2708, num_features: int = 1433, num_classes: int = 7, num_train: int = 140,
                       num_valid: int = 500, num_test: int = 1000, neighbours_per_node: float = 2.0, feature_density: float = 0.0127,
                       seed: int = 0, hub_nodes: int = 0, hub_share: float = 0.02) -> None:
        """Cora-shaped stand-in for load_data (no dataset on the machines): 2708 nodes, 1433 binary bag-of-words features at Cora's
        density, row-normalised, 7 classes, ~5.4 k neighbour-list entries = 10.8 k directed edges + self loops; folds of
        140 / 500 / 1000 nodes laid out as Planetoid's (first, next, last).  The test fold is kept as `synthetic_test_data`.
        sparse_node_features: the words of every row are drawn directly (a Binomial(num_features, feature_density) count of uniform
        draws per row, a word drawn twice counted once), no [V, F] array is built, and the folds share one SparseRows.
        hub_nodes > 0 (the benchmark graph of scripts/bench_neighbour_sampling.py): every neighbour-list entry is redirected with
        probability hub_share to one of the first hub_nodes nodes, node (Zipf(1.5) - 1) % hub_nodes: a heavy tail of in-degrees.  The
        redirection draws from a generator of its own; with hub_nodes == 0 nothing of what a seed gave before changes."""
        rng = np.random.default_rng(seed)
        graph = {}
        lengths = rng.poisson(neighbours_per_node, size=num_nodes)
        for node in range(num_nodes):
            graph[node] = rng.integers(0, num_nodes, size=int(lengths[node])).tolist()
        if hub_nodes > 0:
            hub_rng = np.random.default_rng([seed, 1])
            total = int(lengths.sum())
            flat = np.fromiter((n for v in graph.values() for n in v), dtype=np.int64, count=total)
            to_hub = hub_rng.random(total) < hub_share
            flat[to_hub] = (hub_rng.zipf(1.5, size=int(to_hub.sum())) - 1) % hub_nodes
            ends = np.cumsum(lengths).tolist()
            graph = {node: flat[end - int(n):end].tolist() for node, (end, n) in enumerate(zip(ends, lengths))}
        if self.sparse_node_features:
            rowptr, col = random_rows(rng, num_nodes, num_features, rng.binomial(num_features, feature_density, size=num_nodes))
            words = np.diff(rowptr)
            features = SparseRows(rowptr, col, np.repeat(np.float32(1.0) / np.maximum(words, 1).astype(np.float32), words),
                                  (num_nodes, num_features))
        else:
            bag = (rng.random((num_nodes, num_features)) < feature_density).astype(np.float32)
            row_sum = bag.sum(1, keepdims=True)
            features = np.divide(bag, row_sum, out=np.zeros_like(bag), where=row_sum > 0)
        labels = rng.integers(0, num_classes, size=num_nodes)
        adjacency, degrees = graph_to_edge_lists(graph)
        self.__initial_node_feature_size, self.__num_output_classes = num_features, num_classes
        folds = []
        for ids in (np.arange(num_train), np.arange(num_train, num_train + num_valid), np.arange(num_nodes - num_test, num_nodes)):
            mask = np.zeros(num_nodes, dtype=bool)
            mask[ids] = True
            folds.append([self._fold(adjacency, degrees, features, np.where(mask, labels, 0), mask)])
        self._loaded_data[DataFold.TRAIN], self._loaded_data[DataFold.VALIDATION], self.synthetic_test_data = folds

    # -------------------- Output head (:112-148) --------------------
    def output_variable_scope(self, model_has_input_projection: bool) -> str:
        # :127-131: a NAMED Keras Dense made outside the model's variable scope: its variable sits at the graph's root whatever the
        # model built before it
        return "OutputDenseLayer"

    def output_variables(self, hidden_size: int):
        return {"kernel": ((hidden_size, self.__num_output_classes), "glorot_uniform")}

    def compute_task_metrics(self, final_node_representations: torch.Tensor, batch, weights) -> Dict[str, torch.Tensor]:
        labels, mask = batch.extra['labels'], batch.extra['mask']
        keep = float(batch.extra.get('out_layer_dropout_keep_prob', 1.0))
        if keep < 1.0:                                                                    # :123-125
            final_node_representations = torch.nn.functional.dropout(final_node_representations, p=1.0 - keep, training=True)
        logits = dense(final_node_representations, weights["kernel"])                     # :126-131, [V, classes]
        if logits.is_cuda:
            if labels.dtype != torch.int32:           # (the numpy iterator's DeviceBatch widens integer arrays; the native one keeps int32)
                labels = labels.to(torch.int32)
            if 'loss_normalisation' in batch.extra:   # a normalised subgraph batch: (weight per node, denominator = n_train)
                node_weights, denominator = batch.extra['loss_normalisation']
                loss, total_loss, accuracy, counts = softmax_ce_weighted_stats(logits, labels, mask, node_weights, denominator)
            else:
                loss, total_loss, accuracy, counts = softmax_ce_stats(logits, labels, mask)
            metrics = {'loss': loss, 'total_loss': total_loss, 'accuracy': accuracy}
            if 'sampled_nodes' in batch.extra:        # one of several batches of an epoch: the counts the epoch's accuracy adds up
                metrics.update(num_masked=counts[1], num_correct=counts[2])
            return metrics
        # :133-148 in torch
        num_masked = mask.sum()
        losses = torch.nn.functional.cross_entropy(logits, labels.long(), reduction='none')
        total_loss = (losses * mask).sum()
        top = logits.detach().max(dim=1, keepdim=True).values
        columns = torch.arange(logits.shape[1], device=logits.device).expand_as(logits)
        first_max = torch.where(logits.detach() == top, columns, logits.shape[1]).min(dim=1).values   # the first of equal maxima, as tf.argmax
        accuracy = ((first_max == labels.long()).to(torch.float32) * mask).sum() / num_masked
        return {'loss': total_loss / num_masked, 'total_loss': total_loss, 'accuracy': accuracy}

    # -------------------- Predictions: the class of every node --------------------
    PER_NODE_PREDICTIONS = ("probabilities", "classes")

    @staticmethod
    def num_nodes_of(sample) -> int:
        return int(sample.node_features.shape[0])

    def prediction_layout(self, batch, hidden_size: int):
        # (a layered batch, predict(nodes=...): the head sees the seed rows only)
        num_nodes = int(batch.extra['layer_graphs'][-1].num_targets) if 'layer_graphs' in batch.extra else int(batch.num_nodes)
        return {"probabilities": ((num_nodes, self.__num_output_classes), torch.float32), "classes": ((num_nodes,), torch.int32)}

    def compute_task_predictions(self, final_node_representations: torch.Tensor, batch, weights, out=None) -> Dict[str, torch.Tensor]:
        """probabilities float32 [V, classes] = softmax(logits); classes int32 [V] = the first maximum of the logits, as the accuracy
        of _SoftmaxCEStats counts it (:134-138).  For EVERY node: the fold's mask is not read; no dropout."""
        out = out or {}
        logits = dense(final_node_representations, weights["kernel"])
        probabilities, classes = predict_softmax(logits, out.get("probabilities"), out.get("classes"))
        return {"probabilities": probabilities, "classes": classes}

    NODE_PAYLOADS = {"initial_node_features": ("node_features", np.float32), "labels": ("labels", np.int32),
                     "mask": ("mask", np.float32)}

    # -------------------- Minibatching (:151-177) --------------------
    def _out_keep(self, data_fold: DataFold) -> float:
        return self.params['out_layer_dropout_keep_prob'] if data_fold == DataFold.TRAIN else 1.0

    def make_minibatch_iterator(self, data, data_fold: DataFold, max_nodes_per_batch: int,
                                rng: Optional[np.random.RandomState] = None) -> Iterator[MinibatchData]:
        """Exactly one minibatch per epoch, the whole graph; max_nodes_per_batch is not consulted (:157-177)."""
        refuse_single_graph_task(self.name())
        fold = next(iter(data))
        sampled = self.batches.train_batches(fold) if data_fold == DataFold.TRAIN else None
        if sampled is not None:
            yield from sampled
            return
        sparse = isinstance(fold.node_features, SparseRows)
        feed = {
            'initial_node_features': node_stand_in(len(fold.node_features)) if sparse else fold.node_features,
            'adjacency_lists': list(fold.adjacency_lists),
            'type_to_num_incoming_edges': fold.type_to_node_to_num_incoming_edges,
            'num_graphs': 1,
            'labels': fold.labels,
            'mask': fold.mask,
            'out_layer_dropout_keep_prob': self._out_keep(data_fold),
        }
        plan = self._layerwise_plan(fold, data_fold)
        if plan is not None:
            feed['layerwise_evaluation'] = plan                       # (not an array either)
        if sparse:
            feed['sparse_node_features'] = fold.node_features       # (not an array: DeviceBatch keeps it as it is, in `extra`)
        yield MinibatchData(feed_dict=feed, num_graphs=1, num_nodes=fold.node_features.shape[0],
                            num_edges=sum(len(a) for a in fold.adjacency_lists))

    def make_graph_store(self, data):
        """A fold with sparse features is flattened with the per-node stand-in in the table's place; the store remembers the
        container (`sparse_rows`) for make_native_minibatch_iterator."""
        folds = list(data)
        rows = folds[0].node_features if folds and isinstance(folds[0].node_features, SparseRows) else None
        if rows is None:
            store = super().make_graph_store(folds)
            store.citation_fold = folds[0] if folds else None        # (what the sampled TRAIN batches are cut from)
            return store
        store = super().make_graph_store([f._replace(node_features=node_stand_in(len(f.node_features))) for f in folds])
        store.sparse_rows = rows
        store.citation_fold = folds[0]
        return store

    # -------------------- Sampled batches (tasks/single_graph_batches.py) and what the model is asked for them --------------------
    def bind_sampling_device(self, device) -> None:
        self.batches.bind(device)

    def evaluation_batches(self, data, data_fold: DataFold, full_graph_route: bool):
        return self.batches.evaluation_batches(data, data_fold, full_graph_route)

    def node_prediction_batches(self, data, distinct_nodes: np.ndarray, fanouts, seeds_per_batch: int, full_graph_route: bool):
        return self.batches.node_prediction_batches(data, distinct_nodes, fanouts, seeds_per_batch, full_graph_route)

    def resident_rows(self, rows: SparseRows, device) -> SparseRows:
        return resident_copy(self._device_rows, rows, device)

    def model_requirements(self) -> ModelRequirements:
        sampled, subgraph = self.sampled_batches or {}, self.subgraph_batches or {}
        layered = []
        if sampled.get("layered", False):         # one level graph per layer, one hop per level
            layered.append((sampled["fanouts"], 'sampled_batches: "layered": true requires %s: layer l runs on the nodes H - l + 1 hops '
                                                'from a seed, and the layer functions take one graph'))
        if sampled.get("evaluation") is not None:
            layered.append((sampled["evaluation"]["fanouts"], 'sampled_batches: "evaluation" requires %s: evaluation batches are '
                                                              'hop-ordered and run layer l on the nodes H - l + 1 hops from a seed'))
        message_scale = None
        if (subgraph.get("normalisation") or {}).get("aggregation", False):    # the per-edge weights reach a layer as its degree scale
            message_scale = ('subgraph_batches: normalisation: "aggregation": true requires %s: the per-edge weights take the place '
                             'of 1/(in-degree + 1e-7) in a sum over the messages; "aggregation": false (the loss normalisation '
                             'alone) works with every model')
        layerwise = None
        if self.layerwise_evaluation is not None:                              # a window's block is one hop under every layer
            layerwise = ('layerwise_evaluation requires %s: every layer runs on the blocks of its windows, one hop each, and the '
                         'layer functions take one graph')
        return ModelRequirements(tuple(layered), message_scale, self.sparse_update, self.sparse_gradient, layerwise)

    def epoch_batches(self, data, data_fold: DataFold, device, full_graph_route: bool, full_graph: bool = False):
        if data_fold == DataFold.TRAIN and (self.sampled_batches is not None or self.subgraph_batches is not None):
            self.bind_sampling_device(device)
            return self.make_minibatch_iterator(data, data_fold, 0)
        if data_fold != DataFold.TRAIN and not full_graph and self.evaluation is not None:
            self.bind_sampling_device(device)
            return self.evaluation_batches(data, data_fold, full_graph_route)
        if data_fold != DataFold.TRAIN and self.layerwise_evaluation is not None and torch.device(device).type != "cuda":
            raise RuntimeError("layerwise_evaluation needs a model on the GPU: the window block is a HIP kernel and there is no CPU "
                               "fallback (the model is on %s)" % (device,))
        return None

    def epoch_result(self, result, data_fold: DataFold):
        if data_fold != DataFold.TRAIN and self.evaluation is not None:
            return self.sampled_evaluation_epoch(result)      # the fold's batches add up to its one graph
        return result

    def node_prediction_settings(self) -> Dict[str, Any]:
        """Fanouts and batch size of predict(nodes=...): the "evaluation" key's, or (None: one 0 per layer) and 1024 without it."""
        evaluation = self.evaluation
        if evaluation is not None:
            return {"fanouts": list(evaluation["fanouts"]), "seeds_per_batch": evaluation["seeds_per_batch"]}
        return {"fanouts": None, "seeds_per_batch": PREDICT_SEEDS_PER_BATCH}

    def check_prediction_nodes(self, data, nodes):
        """-> (distinct ids ascending int32, position of every given node among them, the given nodes as int64) for the ONE graph
        of `data`; ValueError otherwise (neighbour_sampling.check_prediction_nodes)."""
        folds = list(data)
        if len(folds) != 1:
            raise ValueError("predict(nodes=...): the ids name nodes of ONE graph; data holds %d" % len(folds))
        return check_prediction_nodes(nodes, len(folds[0].labels))

    @staticmethod
    def sampled_evaluation_epoch(result):
        """The result of an epoch of evaluation batches as the fold's ONE graph: loss = sum of total_loss / sum of num_masked, one
        graph (early_stopping_metric then divides the sum of total_loss by 1: the full-graph value's definition)."""
        loss, results, graphs, graphs_per_s, nodes_per_s, edges_per_s = result
        masked = sum(float(m['num_masked']) for m in results)
        total = float(np.sum([float(m['total_loss']) for m in results]))
        return (total / masked if masked else float("nan"), results, 1, graphs_per_s / max(graphs, 1), nodes_per_s, edges_per_s)

    def compute_initial_node_features(self, batch, weights):
        """The batch's feature table, or in the sparse mode the SparseRows on the batch's device: one copy per device, kept weakly
        with the host container."""
        rows = batch.extra.get('sparse_node_features')
        if rows is None:
            return batch.initial_node_features
        return self.resident_rows(rows, batch.initial_node_features.device)

    def make_native_minibatch_iterator(self, batcher, data_fold: DataFold, max_nodes_per_batch: int,
                                       rng: Optional[np.random.RandomState] = None):
        """The same single batch from the flattened fold.  The packer's rule (graphs are taken while the node count stays BELOW
        max_nodes_per_batch) is not asked: the graph is the batch whatever its size.  A resident fold (tasks/resident.py) was
        bucketed once when it was made; its one assembled batch is kept and handed out again every epoch."""
        refuse_single_graph_task(self.name())
        if batcher.store.num_graphs != 1:
            raise ValueError("a citation-network fold is ONE graph; got %d" % batcher.store.num_graphs)
        sampled = self.batches.train_batches(batcher.store.citation_fold) if data_fold == DataFold.TRAIN else None
        if sampled is not None:
            yield from sampled
            return
        yield self._full_graph_batch(batcher, data_fold)

    def _full_graph_batch(self, batcher, data_fold: DataFold):
        """The fold's one full-graph batch from its input pipeline."""
        keep = self._out_keep(data_fold)
        batcher.constants['out_layer_dropout_keep_prob'] = keep
        rows = getattr(batcher.store, "sparse_rows", None)
        if rows is not None:
            batcher.constants['sparse_node_features'] = rows
        ids = np.zeros(1, dtype=np.int64)
        if isinstance(batcher, ResidentDataset):
            batch = self._resident_batches.get(batcher)
            if batch is None:
                batch = self._resident_batches[batcher] = batcher.assemble(ids)
            batch.extra['out_layer_dropout_keep_prob'] = keep
        else:
            batch = batcher.pack(ids)
        plan = self._layerwise_plan(getattr(batcher.store, "citation_fold", None), data_fold)
        if plan is not None:
            batch.extra['layerwise_evaluation'] = plan
        else:
            batch.extra.pop('layerwise_evaluation', None)             # (a resident fold's one batch is handed out again)
        return batch

    # -------------------- Data parallelism over the sampled batches of the ONE graph (the key "data_parallel"; models/data_parallel.py) ----
    def rank_epoch_batches(self, data, data_fold: DataFold, device, full_graph_route: bool, rank: int, world: int, pipeline):
        """-> (the batches rank `rank` of `world` runs in one epoch, are they its share of the fold's).  TRAIN: global batch j when
        j mod world == rank.  VALIDATION / TEST under "evaluation": batch i when i mod world == rank.  Without "evaluation" every
        rank runs the full graph itself from `pipeline()` (the model's input pipeline of the fold, built when asked for)."""
        if data_fold == DataFold.TRAIN:
            self.bind_sampling_device(device)
            return self.batches.rank_train_batches(next(iter(data)), rank, world), True
        if self.evaluation is not None:
            self.bind_sampling_device(device)
            return self.batches.rank_evaluation_batches(data, data_fold, full_graph_route, rank, world), True
        batcher = pipeline()
        if batcher.store.num_graphs != 1:
            raise ValueError("a citation-network fold is ONE graph; got %d" % batcher.store.num_graphs)
        return iter((self._full_graph_batch(batcher, data_fold),)), False

    def train_schedule(self, data, world: int):
        """Who runs which batch of the NEXT TRAIN epoch, with what share of its step (parallel.single_graph_schedule)."""
        return single_graph_schedule(self.batches.train_batch_weights(next(iter(data))), world, self.batches.epoch)

    def data_parallel_fingerprint(self) -> Dict[str, Any]:
        """Of the loaded TRAIN and VALIDATION folds (single_graph_batches.SingleGraphBatches.fingerprint)."""
        return self.batches.fingerprint({"train": self._loaded_data[DataFold.TRAIN][0], "validation": self._loaded_data[DataFold.VALIDATION][0]})

    def loss_weight(self, num_graphs: int, num_nodes: int) -> float:
        raise RuntimeError("the %s task trains on ONE graph that is the whole batch: it cannot be split by graph across ranks; "
                           "run it on a single GPU" % self.name())

    def early_stopping_metric(self, task_metric_results: List[Dict[str, Any]], num_graphs: int) -> float:
        # :179-181: average loss
        return float(np.sum([float(m['total_loss']) for m in task_metric_results]) / num_graphs)

    def pretty_print_epoch_task_metrics(self, task_metric_results: List[Dict[str, Any]], num_graphs: int) -> str:
        if len(task_metric_results) > 1 and all('num_masked' in m for m in task_metric_results):     # an epoch of sampled batches
            masked = sum(float(m['num_masked']) for m in task_metric_results)
            # (the graph-wide samplers of `subgraph_batches` may meet no TRAIN node in a whole epoch: 0 of 0 is printed as 0)
            return "Acc: %.2f%%" % (sum(float(m['num_correct']) for m in task_metric_results) / max(masked, 1.0) * 100,)
        return "Acc: %.2f%%" % (float(task_metric_results[0]['accuracy']) * 100,)
