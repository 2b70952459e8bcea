"""VarMisuse task mirror (tasks/varmisuse_task.py of the reference): pick, among at most five candidate variables, the one that
belongs into a slot of a program graph.

Two parts of the model belong to the task:
  * the INPUT model (:317-367), with variables of its own at the graph's root scope, created before `graph_model/...`: a 2-layer
    character CNN over the node labels (one_hot -> Conv1D(16, 5) -> MaxPool1D(5, 1) -> Conv1D(D, C - 8), leaky_relu 0.2), computed
    once per unique label of a graph and gathered per node;
  * the OUTPUT head (:369-448): slot row and candidate rows of the final node states, their inner product, optionally a bias-free
    Dense over [candidate | slot | inner product], `+ (1 - mask) * -1e7`, softmax cross-entropy against candidate 0.
On the GPU both are HIP kernels (csrc/varmisuse.hip); the torch compositions below serve the CPU, any shape the kernels do not
take, the `max-margin` loss, and as the yardstick the kernels are timed against.

Kept quirks of the reference:
  * the head applies NO dropout, in any fold: :490 writes the rate into the placeholder dict instead of the feed dict, so the
    placeholder keeps its default 0.0.  `out_layer_dropout_rate` is accepted and never used.
  * PAD (code 0) is a live one-hot column; the codes of '{' and '}' (68, 69) fall outside depth 68 and are all-zero rows.
Stated deviations:
  * `max-margin`: the reference reads self.parameters['loss_margin'], which does not exist (:434), so it cannot run that loss; here
    it is relu(max wrong log-prob - correct log-prob + params['max-margin_loss_margin']) in plain torch ops.
  * num_edge_types is per instance (22, or 23 with add_self_loop_edges); the reference mutates a module-global vocabulary, so one
    self-loop task makes every later task of the process report 23 (:243-247).
  * the loader runs in-process over the files in sorted order (the reference: a multiprocessing pool of cpu_count() workers, in
    completion order); a first graph that alone reaches max_nodes_per_batch raises ValueError (the reference concatenates an
    empty list).
  * `"varmisuse"` is NOT a key of tasks.TASK_CLASSES (tests/test_model_cpu.py pins the registry): construct VarMisuse_Task directly;
    models.restore() finds it through tasks.CHECKPOINT_TASK_CLASSES.
The native pipelines (host packer, resident fold) carry the per-node character table `unique[inverse]` as their
initial_node_features payload and run the CNN with an identity map: at 60 k nodes the CNN is ~1.5 GFLOP, de-duplication buys
nothing on the GPU.  So that the three pipelines produce the same bits, the numpy iterator's unique tables are expanded to the
per-node table on the GPU as well.
"""
import glob
import gzip
import json
import os
import re
from collections import defaultdict
from typing import Any, Dict, Iterable, Iterator, List, NamedTuple, Optional, Set

import numpy as np
import torch

from .. import _lib, ops
from ..graph import _PENDING_CHECKS
from ..predict import predict_candidates
from .sparse_graph_task import DataFold, MinibatchData, Sparse_Graph_Task
from .synthetic import make_varmisuse_shaped_graph

BIG_NUMBER = 1e7                                        # utils/utils.py of the reference
ALPHABET = "abcdefghijklmnopqrstuvwxyz0123456789,;.!?:'\"/\\|_@#$%^&*~`+-=<>()[]{}"      # :15, 68 characters
ALPHABET_DICT = {char: idx + 2 for (idx, char) in enumerate(ALPHABET)}                     # 0 is PAD, 1 is UNK
ONE_HOT_DEPTH = len(ALPHABET)                           # tf.one_hot(depth=len(ALPHABET)) over codes that start at 2 (:341-343)
USES_SUBTOKEN_EDGE_NAME = "UsesSubtoken"
SELF_LOOP_EDGE_NAME = "SelfLoop"
BACKWARD_EDGE_TYPE_NAME_SUFFIX = "_Bkwd"
PROGRAM_GRAPH_EDGES_TYPES = ["Child", "NextToken", "LastUse", "LastWrite", "LastLexicalUse", "ComputedFrom", "GuardedByNegation",
                             "GuardedBy", "FormalArgName", "ReturnsTo", USES_SUBTOKEN_EDGE_NAME]           # :22-23

ROUTES = {"charcnn": None, "head": None}                # which implementation the last call took: "hip" or "composition"


class GraphSample(NamedTuple):
    """The reference's seven fields (:31-38) and `node_features`: the per-node character table unique[inverse], uint8 [V, C]
    (tasks/batcher.py sizes a graph by len(node_features) and carries it as the initial_node_features payload)."""
    adjacency_lists: List[np.ndarray]
    type_to_node_to_num_incoming_edges: np.ndarray
    unique_labels_as_characters: np.ndarray
    node_labels_to_unique_labels: np.ndarray
    slot_node_id: int
    variable_candidate_nodes: np.ndarray
    variable_candidate_nodes_mask: np.ndarray
    node_features: np.ndarray


# ---------------------------------------------------------------------------------------------------------------------------------
# dpu_utils.codeutils, restated  [dpu_utils-internal, from memory, unpinned]: the package is on no machine this project has; the
# fixtures pin everything the reference does AROUND these two functions (they are injected into its module), not the functions.
# ---------------------------------------------------------------------------------------------------------------------------------
_CAMEL_PARTS = re.compile(r"[A-Z]+(?![a-z])|[A-Z]?[a-z]+|[0-9]+|[^A-Za-z0-9]+")


def split_identifier_into_parts(identifier: str) -> List[str]:
    """Split on '_' and on camelCase boundaries ('HTTPServer2x' -> http, server, 2, x), lower-cased; an identifier without any
    part is returned as it is.  [dpu_utils-internal, from memory, unpinned]"""
    parts = []
    for snake in identifier.split("_"):
        if snake:
            parts.extend(p.lower() for p in _CAMEL_PARTS.findall(snake))
    return parts if parts else [identifier]


_CSHARP_KEYWORDS = frozenset("""abstract as base bool break byte case catch char checked class const continue decimal default delegate do
double else enum event explicit extern false finally fixed float for foreach goto if implicit in int interface internal is lock long
namespace new null object operator out override params private protected public readonly ref return sbyte sealed short sizeof
stackalloc static string struct switch this throw true try typeof uint ulong unchecked unsafe ushort using virtual void volatile
while""".split())


def get_language_keywords(language: str) -> Set[str]:
    """The keyword set that keeps a node label from being split into subtokens.  [dpu_utils-internal, from memory, unpinned]"""
    if language.lower() != "csharp":
        raise ValueError("only the C# keyword set is restated here; got %r" % language)
    return _CSHARP_KEYWORDS


# ---------------------------------------------------------------------------------------------------------------------------------
# loader (:41-136)
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_type_vocabulary(add_self_loop_edges: bool) -> Dict[str, int]:
    """:24-28 and :243-247: 11 base types, their _Bkwd mirrors in the same order, SelfLoop last when asked for."""
    names = PROGRAM_GRAPH_EDGES_TYPES + [n + BACKWARD_EDGE_TYPE_NAME_SUFFIX for n in PROGRAM_GRAPH_EDGES_TYPES]
    if add_self_loop_edges:
        names = names + [SELF_LOOP_EDGE_NAME]
    return {name: idx for idx, name in enumerate(names)}


def _add_per_subtoken_nodes(unsplittable_node_names: Set[str], graph_dict: Dict[str, Any]) -> None:
    """:41-66, same containers (dict / set iteration orders are the reference's)."""
    graph_node_labels = graph_dict['NodeLabels']
    subtoken_to_using_nodes = defaultdict(set)
    max_used_node_id = 0
    for node_id, node_label in graph_node_labels.items():
        node_id = int(node_id)
        max_used_node_id = max(node_id, max_used_node_id)
        if node_label in unsplittable_node_names:       # AST nodes and punctuation
            continue
        for subtoken in split_identifier_into_parts(node_label):
            if re.search('[a-zA-Z0-9]', subtoken):
                subtoken_to_using_nodes[subtoken].add(node_id)
    subtoken_node_id = max_used_node_id
    new_edges = []
    for subtoken, using_nodes in subtoken_to_using_nodes.items():
        subtoken_node_id += 1
        graph_node_labels[str(subtoken_node_id)] = subtoken
        new_edges.extend([(using_node_id, subtoken_node_id) for using_node_id in using_nodes])
    graph_dict['Edges'][USES_SUBTOKEN_EDGE_NAME] = new_edges


def encode_labels(node_labels: Dict[str, str], num_nodes: int, max_num_chars: int) -> np.ndarray:
    """:77-81: lower-cased, cut to max_num_chars, alphabet index + 2, unknown characters 1, padding 0; uint8 [V, C]."""
    node_label_chars = np.zeros(shape=(num_nodes, max_num_chars), dtype=np.uint8)
    for (node, label) in node_labels.items():
        for (char_idx, label_char) in enumerate(label[:max_num_chars].lower()):
            node_label_chars[int(node), char_idx] = ALPHABET_DICT.get(label_char, 1)
    return node_label_chars


def load_single_sample(raw_sample: Dict[str, Any], unsplittable_node_names: Set[str], graph_node_label_max_num_chars: int,
                       max_variable_candidates: int, edge_type_vocab: Dict[str, int]) -> GraphSample:
    """:69-136.  raw_sample is changed in place (subtoken nodes and edges are added), as the reference changes it."""
    _add_per_subtoken_nodes(unsplittable_node_names, raw_sample['ContextGraph'])
    num_nodes = len(raw_sample['ContextGraph']['NodeLabels'])
    node_label_chars = encode_labels(raw_sample['ContextGraph']['NodeLabels'], num_nodes, graph_node_label_max_num_chars)
    node_label_chars_unique, node_label_chars_indices = np.unique(node_label_chars, axis=0, return_inverse=True)
    node_label_chars_indices = node_label_chars_indices.reshape(-1)

    num_edge_types = len(edge_type_vocab)
    adjacency_lists = [np.zeros((0, 2), dtype=np.int32) for _ in range(num_edge_types)]
    num_incoming_edges_per_type = np.zeros((num_edge_types, num_nodes), dtype=np.uint16)
    for e_type, e_type_edges in raw_sample['ContextGraph']['Edges'].items():
        if len(e_type_edges) > 0:
            e_type_idx = edge_type_vocab[e_type]
            e_type_bkwd_idx = edge_type_vocab[e_type + BACKWARD_EDGE_TYPE_NAME_SUFFIX]
            fwd_edges = np.array(e_type_edges, dtype=np.int32)
            bkwd_edges = np.flip(fwd_edges, axis=1)
            adjacency_lists[e_type_idx] = fwd_edges
            adjacency_lists[e_type_bkwd_idx] = bkwd_edges
            num_incoming_edges_per_type[e_type_idx, :] = np.bincount(fwd_edges[:, 1], minlength=num_nodes)
            num_incoming_edges_per_type[e_type_bkwd_idx, :] = np.bincount(bkwd_edges[:, 1], minlength=num_nodes)
    if SELF_LOOP_EDGE_NAME in edge_type_vocab:
        self_loop_edge_type_idx = edge_type_vocab[SELF_LOOP_EDGE_NAME]
        adjacency_lists[self_loop_edge_type_idx] = np.stack([np.arange(num_nodes), np.arange(num_nodes)], axis=1)
        num_incoming_edges_per_type[self_loop_edge_type_idx, :] = np.ones(shape=(num_nodes,))

    # the correct candidate first, then at most max - 1 distractors in file order, padded with node 0 / mask False (:114-127)
    correct_candidate_id = None
    distractor_candidate_ids = []
    for candidate in raw_sample['SymbolCandidates']:
        if candidate['IsCorrect']:
            correct_candidate_id = candidate['SymbolDummyNode']
        else:
            distractor_candidate_ids.append(candidate['SymbolDummyNode'])
    assert correct_candidate_id is not None
    candidate_node_ids = [correct_candidate_id] + distractor_candidate_ids[:max_variable_candidates - 1]
    num_scope_padding = max_variable_candidates - len(candidate_node_ids)
    candidate_node_ids_mask = [True] * len(candidate_node_ids) + [False] * num_scope_padding
    candidate_node_ids = candidate_node_ids + [0] * num_scope_padding
    return GraphSample(adjacency_lists=adjacency_lists,
                       type_to_node_to_num_incoming_edges=num_incoming_edges_per_type,
                       unique_labels_as_characters=node_label_chars_unique,
                       node_labels_to_unique_labels=node_label_chars_indices,
                       slot_node_id=raw_sample['SlotDummyNode'],
                       variable_candidate_nodes=np.array(candidate_node_ids),
                       variable_candidate_nodes_mask=np.array(candidate_node_ids_mask),
                       node_features=node_label_chars)


def read_by_file_suffix(path: str) -> List[Dict[str, Any]]:
    """The two forms dpu_utils' RichPath.read_by_file_suffix decodes for these files: one JSON document per line (.jsonl.gz) or one
    JSON list (.json.gz)."""
    if path.endswith(".jsonl.gz"):
        with gzip.open(path, "rt") as f:
            return [json.loads(line) for line in f if line.strip()]
    if path.endswith(".json.gz"):
        with gzip.open(path, "rt") as f:
            return json.load(f)
    raise ValueError("unsupported suffix of %r (expected .jsonl.gz or .json.gz)" % path)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two task-owned model parts as torch compositions (any device, any float dtype)
# ---------------------------------------------------------------------------------------------------------------------------------
def charcnn_composition(chars: torch.Tensor, label_of_node: Optional[torch.Tensor], w1: torch.Tensor, b1: torch.Tensor,
                        w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """:337-367 with Keras kernels [k, in, out]: chars integer [U, C] -> [V, D] (label_of_node None: V = U)."""
    depth = w1.shape[1]
    codes = chars.long().clamp(max=depth)                                                   # codes >= depth: an all-zero row
    one_hot = torch.nn.functional.one_hot(codes, depth + 1)[..., :depth].to(w1.dtype)       # [U, C, A]
    x = one_hot.transpose(1, 2)                                                             # channels first
    conv1 = torch.nn.functional.leaky_relu(torch.nn.functional.conv1d(x, w1.permute(2, 1, 0), b1), 0.2)
    pool1 = torch.nn.functional.max_pool1d(conv1, kernel_size=w1.shape[0], stride=1)
    conv2 = torch.nn.functional.leaky_relu(torch.nn.functional.conv1d(pool1, w2.permute(2, 1, 0), b2), 0.2)
    unique_label_representations = conv2.squeeze(2)                                         # [U, D]
    if label_of_node is None:
        return unique_label_representations
    return unique_label_representations.index_select(0, label_of_node.long())


def head_logits_composition(states: torch.Tensor, slot_ids: torch.Tensor, cand_ids: torch.Tensor, mask: torch.Tensor,
                            w: Optional[torch.Tensor]) -> torch.Tensor:
    """:389-420: absolute slot ids [G], candidate ids [G, Cn], mask [G, Cn], w [2 D + 1, 1] or None -> logits [G, Cn]."""
    num_graphs, num_cands = cand_ids.shape
    slot = states.index_select(0, slot_ids.long())                                          # [G, D]
    cands = states.index_select(0, cand_ids.reshape(-1).long()).reshape(num_graphs, num_cands, states.shape[1])
    inner = torch.einsum('sd,scd->sc', slot, cands)
    if w is not None:
        comb = torch.cat([cands, slot.unsqueeze(1).expand(-1, num_cands, -1), inner.unsqueeze(-1)], dim=2)
        logits = (comb @ w.reshape(-1, 1)).squeeze(-1)
    else:
        logits = inner
    return logits + (1.0 - mask.to(logits.dtype)) * -BIG_NUMBER


def head_metrics_composition(logits: torch.Tensor, loss_function: str, margin: float) -> Dict[str, torch.Tensor]:
    """:422-448; the first candidate is the correct one."""
    log_probs = torch.log_softmax(logits, dim=1)
    if loss_function == 'max-likelihood':
        per_graph_loss = -log_probs[:, 0]
    elif loss_function == 'max-margin':
        if logits.shape[1] < 2:
            raise ValueError("the max-margin loss needs at least two candidates")
        per_graph_loss = torch.relu(log_probs[:, 1:].max(dim=1).values - log_probs[:, 0] + margin)
    else:
        raise Exception('Invalid loss function option: "%s"' % loss_function)
    probs = torch.softmax(logits.detach(), dim=1)
    columns = torch.arange(logits.shape[1], device=logits.device).expand_as(probs)
    first_max = torch.where(probs == probs.max(dim=1, keepdim=True).values, columns, logits.shape[1]).min(dim=1).values
    correct = (first_max == 0).to(torch.float32)
    return {'loss': per_graph_loss.mean(), 'total_loss': per_graph_loss.sum(), 'accuracy': correct.mean(),
            'num_correct_predictions': correct.sum()}


# ---------------------------------------------------------------------------------------------------------------------------------
# the HIP route (csrc/varmisuse.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def _err_flag(device, what: str) -> torch.Tensor:
    """A fresh device word for the kernels' index check, read back with the graphs' own at the next metric fetch."""
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    _PENDING_CHECKS.append((flag, what))
    return flag


class _CharCNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chars, label_of_node, w1, b1, w2, b2):
        lib = _lib.load_library()
        chars = chars.contiguous()
        w1c, b1c, w2c, b2c = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        num_labels, num_chars = chars.shape
        out_dim = w2.shape[2]
        num_nodes = num_labels if label_of_node is None else label_of_node.shape[0]
        out = torch.empty((num_nodes, out_dim), dtype=torch.float32, device=chars.device)
        nbytes = lib.relgnn_charcnn_fwd_workspace_bytes(num_labels, out_dim, 0 if label_of_node is None else 1)
        ws = _lib.scratch(nbytes, chars.device)
        flag = None if label_of_node is None else _err_flag(chars.device, "node_labels_to_unique_labels holds an id outside [0, %d)" % num_labels)
        _lib.launch("relgnn_charcnn_fwd", _lib.ptr(chars), num_labels, num_chars, _lib.ptr(label_of_node), num_nodes, _lib.ptr(w1c),
                    _lib.ptr(b1c), _lib.ptr(w2c), _lib.ptr(b2c), out_dim, _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.ptr(flag))
        ctx.save_for_backward(chars, label_of_node, w1c, b1c, w2c, b2c)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load_library()
        chars, label_of_node, w1, b1, w2, b2 = ctx.saved_tensors
        num_labels, num_chars = chars.shape
        out_dim = w2.shape[2]
        g = g.contiguous()
        if label_of_node is not None:                   # the gather's gradient: the deterministic segment sum by label
            g = ops.unsorted_segment_sum(g, label_of_node, num_labels).contiguous()
        dw1, db1, dw2, db2 = (torch.empty_like(t) for t in (w1, b1, w2, b2))
        nbytes = lib.relgnn_charcnn_bwd_workspace_bytes(num_labels, num_chars, out_dim)
        ws = _lib.scratch(nbytes, chars.device)
        _lib.launch("relgnn_charcnn_bwd", _lib.ptr(chars), num_labels, num_chars, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2),
                    out_dim, _lib.ptr(g), _lib.ptr(dw1), _lib.ptr(db1), _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(ws), nbytes)
        return None, None, dw1, db1, dw2, db2


def charcnn_supported(num_chars: int, out_dim: int, w1: torch.Tensor) -> bool:
    return tuple(w1.shape) == (5, ONE_HOT_DEPTH, 16) and bool(_lib.load_library().relgnn_charcnn_supported(int(num_chars), int(out_dim)))


def node_label_embeddings(chars: torch.Tensor, label_of_node: Optional[torch.Tensor], w1, b1, w2, b2) -> torch.Tensor:
    """The input model on chars [U, C] (uint8 on the HIP route) and an optional int32 map [V]: the kernels on a GPU for the shapes
    they take, the composition otherwise; ROUTES['charcnn'] says which."""
    if chars.is_cuda and w1.dtype == torch.float32 and w2.shape[0] == chars.shape[1] - 8 \
            and charcnn_supported(chars.shape[1], w2.shape[2], w1):
        ROUTES["charcnn"] = "hip"
        if chars.dtype != torch.uint8:
            chars = chars.to(torch.uint8)
        if label_of_node is not None and label_of_node.dtype != torch.int32:
            label_of_node = label_of_node.to(torch.int32)
        return _CharCNN.apply(chars, label_of_node, w1, b1, w2, b2)
    ROUTES["charcnn"] = "composition"
    return charcnn_composition(chars, label_of_node, w1, b1, w2, b2)


class _Head(torch.autograd.Function):
    """(loss, total_loss, accuracy, num_correct_predictions, logits) of one batch: csrc/varmisuse.hip, one wave per graph."""

    @staticmethod
    def forward(ctx, states, slot_ids, cand_ids, mask, first_node, w):
        lib = _lib.load_library()
        if states.dim() != 2 or states.stride(1) != 1:
            states = states.contiguous()
        num_nodes, hidden = states.shape
        num_graphs, num_cands = cand_ids.shape
        wv = None if w is None else w.detach().reshape(-1).contiguous()
        logits = torch.empty((num_graphs, num_cands), dtype=torch.float32, device=states.device)
        stats = torch.empty(4, dtype=torch.float32, device=states.device)
        nbytes = lib.relgnn_varmisuse_head_workspace_bytes(num_graphs, hidden)
        ws = _lib.scratch(nbytes, states.device)
        ld = states.stride(0) if num_nodes > 1 else hidden
        _lib.launch("relgnn_varmisuse_head_fwd", _lib.ptr(states, rows_strided=True), ld, num_nodes, hidden, _lib.ptr(slot_ids),
                    _lib.ptr(cand_ids), _lib.ptr(mask), _lib.ptr(first_node), num_graphs, num_cands, _lib.ptr(wv), _lib.ptr(logits),
                    _lib.ptr(stats), _lib.ptr(ws), nbytes,
                    _lib.ptr(_err_flag(states.device, "a slot or candidate node id lies outside [0, %d)" % num_nodes)))
        ctx.save_for_backward(states, slot_ids, cand_ids, mask, first_node, wv)
        ctx.w_shape = None if w is None else tuple(w.shape)
        ctx.set_materialize_grads(False)
        loss, total, accuracy, correct = stats[2], stats[0], stats[3], stats[1]
        ctx.mark_non_differentiable(accuracy, correct, logits)
        return loss, total, accuracy, correct, logits

    @staticmethod
    def backward(ctx, g_loss, g_total, g_accuracy, g_correct, g_logits):
        lib = _lib.load_library()
        states, slot_ids, cand_ids, mask, first_node, wv = ctx.saved_tensors
        if g_loss is None and g_total is None:
            return None, None, None, None, None, None

        def scalar(g):                                  # the incoming gradients stay on the device: the kernel reads them
            return None if g is None else g.reshape(1).to(torch.float32).contiguous()
        g_loss, g_total = scalar(g_loss), scalar(g_total)
        num_nodes, hidden = states.shape
        num_graphs, num_cands = cand_ids.shape
        d_states = torch.empty((num_nodes, hidden), dtype=torch.float32, device=states.device)
        dw = None if wv is None else torch.empty_like(wv)
        nbytes = lib.relgnn_varmisuse_head_workspace_bytes(num_graphs, hidden)
        ws = _lib.scratch(nbytes, states.device)
        ld = states.stride(0) if num_nodes > 1 else hidden
        _lib.launch("relgnn_varmisuse_head_bwd", _lib.ptr(states, rows_strided=True), ld, num_nodes, hidden, _lib.ptr(slot_ids),
                    _lib.ptr(cand_ids), _lib.ptr(mask), _lib.ptr(first_node), num_graphs, num_cands, _lib.ptr(wv), _lib.ptr(g_loss),
                    _lib.ptr(g_total), _lib.ptr(d_states), hidden, _lib.ptr(dw), _lib.ptr(ws), nbytes)
        return d_states, None, None, None, None, (None if dw is None else dw.reshape(ctx.w_shape))


def head_supported(num_candidates: int, hidden: int) -> bool:
    return bool(_lib.load_library().relgnn_varmisuse_head_supported(int(num_candidates), int(hidden)))


def varmisuse_head(states: torch.Tensor, slot_ids: torch.Tensor, cand_ids: torch.Tensor, mask: torch.Tensor,
                   first_node: Optional[torch.Tensor], w: Optional[torch.Tensor]):
    """-> (loss, total_loss, accuracy, num_correct_predictions, logits) on the HIP route: float32 device states [V, D], int32
    slot ids [G] and candidate ids [G, Cn], float32 mask [G, Cn]; ids absolute (first_node None) or graph-local with int32
    first_node [G]."""
    return _Head.apply(states, slot_ids.contiguous(), cand_ids.contiguous(), mask.contiguous(), first_node, w)


def _device_tensor(value, dtype, device) -> torch.Tensor:
    if torch.is_tensor(value):
        return value if value.dtype == dtype else value.to(dtype)
    return torch.as_tensor(np.asarray(value), dtype=dtype, device=device)


class VarMisuse_Task(Sparse_Graph_Task):
    @classmethod
    def default_params(cls):
        # :216-230
        params = super().default_params()
        params.update({
            'max_variable_candidates': 5,
            'graph_node_label_max_num_chars': 19,
            'graph_node_label_representation_size': 64,
            'slot_score_via_linear_layer': True,
            'loss_function': 'max-likelihood',  # max-likelihood or max-margin
            'max-margin_loss_margin': 0.2,
            'out_layer_dropout_rate': 0.2,      # accepted, never applied (module docstring)
            'add_self_loop_edges': False,
            # 'max_num_data_files': 3,
        })
        return params

    @staticmethod
    def name() -> str:
        return "VarMisuse"

    @staticmethod
    def default_data_path() -> str:
        return "data/varmisuse"

    def __init__(self, params: Dict[str, Any]):
        super().__init__(params)
        self._edge_type_vocab = edge_type_vocabulary(bool(params.get('add_self_loop_edges')))

    def get_metadata(self) -> Dict[str, Any]:
        return {'params': self.params}                  # (the reference's base class stores the task parameters, sparse_graph_task.py:46-59)

    def restore_from_metadata(self, metadata: Dict[str, Any]) -> None:
        self.params = metadata.get('params', self.params)
        self._edge_type_vocab = edge_type_vocabulary(bool(self.params.get('add_self_loop_edges')))

    @property
    def num_edge_types(self) -> int:
        return len(self._edge_type_vocab)

    @property
    def initial_node_feature_size(self) -> int:
        return self.params['graph_node_label_representation_size']

    # -------------------- Data Loading (:265-293) --------------------
    def load_data(self, path) -> None:
        path = getattr(path, "path", path)
        self._loaded_data[DataFold.TRAIN] = list(self._load_fold(os.path.join(path, "graphs-train")))
        self._loaded_data[DataFold.VALIDATION] = list(self._load_fold(os.path.join(path, "graphs-valid")))

    def load_eval_data_from_path(self, path) -> Iterable[GraphSample]:
        path = getattr(path, "path", path)
        if path == self.default_data_path():
            path = os.path.join(path, "graphs-test")
        return iter(self._load_fold(path))

    def _load_fold(self, data_dir: str) -> List[GraphSample]:
        all_data_files = sorted(glob.glob(os.path.join(data_dir, "*.gz")))
        max_num_files = self.params.get('max_num_data_files', None)
        if max_num_files is not None:
            all_data_files = all_data_files[:max_num_files]
        print(" Loading VarMisuse data from %s [%i data files]." % (data_dir, len(all_data_files)))
        unsplittable_keywords = get_language_keywords('csharp')
        return [load_single_sample(raw_sample, unsplittable_keywords, self.params['graph_node_label_max_num_chars'],
                                   self.params['max_variable_candidates'], self._edge_type_vocab)
                for data_file in all_data_files for raw_sample in read_by_file_suffix(data_file)]

    def load_synthetic(self, num_graphs: int = 24, seed: int = 0, num_valid: Optional[int] = None, num_test: Optional[int] = None,
                       mean_nodes: float = 2500.0, std_nodes: float = 600.0, min_nodes: int = 500, max_nodes: int = 5000,
                       vocabulary_size: int = 300) -> None:
        """Stand-in for load_data (no dataset on the machines): the VarMisuse-shaped program-graph structure of tasks/synthetic.py,
        identifier-like node labels drawn from a vocabulary of `vocabulary_size` names, a slot node and 1 .. max_variable_candidates
        candidate nodes per graph (the correct one first, as the loader leaves them).  num_graphs train graphs; the validation and
        test folds hold num_valid / num_test graphs (default: a quarter each, at least one); the test fold is kept as
        `synthetic_test_data`."""
        rng = np.random.default_rng([seed, 0x5a])
        stems = ["get", "set", "is", "num", "index", "count", "value", "name", "list", "item", "node", "result", "buffer", "length",
                 "key", "current", "next", "total", "max", "min", "file", "path", "data", "id", "size", "temp", "source", "target"]
        punctuation = [";", "{", "}", "(", ")", "=", ".", ",", "[", "]", "==", "+", "return", "if", "new"]
        vocabulary = list(punctuation)
        while len(vocabulary) < vocabulary_size:
            parts = [stems[i] for i in rng.integers(0, len(stems), size=int(rng.integers(1, 4)))]
            name = parts[0] + "".join(p.capitalize() for p in parts[1:])
            if rng.random() < 0.2:
                name += str(int(rng.integers(0, 100)))
            vocabulary.append(name)
        num_chars = self.params['graph_node_label_max_num_chars']
        table = encode_labels({str(i): label for i, label in enumerate(vocabulary)}, len(vocabulary), num_chars)
        max_cands = self.params['max_variable_candidates']
        num_types = self.num_edge_types
        num_valid = max(1, num_graphs // 4) if num_valid is None else num_valid
        num_test = max(1, num_graphs // 4) if num_test is None else num_test

        def graph(index: int) -> GraphSample:
            s = make_varmisuse_shaped_graph(seed, index, feature_size=1, mean_nodes=mean_nodes, std_nodes=std_nodes,
                                            min_nodes=min_nodes, max_nodes=max_nodes)
            num_nodes = s.node_features.shape[0]
            g_rng = np.random.default_rng([seed, index, 0x5a])
            chars = table[g_rng.integers(0, len(vocabulary), size=num_nodes)]
            unique, inverse = np.unique(chars, axis=0, return_inverse=True)
            num_cands = int(g_rng.integers(1, max_cands + 1))
            picked = g_rng.choice(num_nodes, size=num_cands + 1, replace=False)
            cands = np.concatenate([picked[1:], np.zeros(max_cands - num_cands, dtype=picked.dtype)])
            return GraphSample(adjacency_lists=list(s.adjacency_lists[:num_types]),
                               type_to_node_to_num_incoming_edges=s.type_to_node_to_num_incoming_edges[:num_types].astype(np.uint16),
                               unique_labels_as_characters=unique, node_labels_to_unique_labels=inverse.reshape(-1),
                               slot_node_id=int(picked[0]), variable_candidate_nodes=cands.astype(np.int64),
                               variable_candidate_nodes_mask=np.arange(max_cands) < num_cands, node_features=chars)

        self._loaded_data[DataFold.TRAIN] = [graph(i) for i in range(num_graphs)]
        self._loaded_data[DataFold.VALIDATION] = [graph(num_graphs + i) for i in range(num_valid)]
        self.synthetic_test_data = [graph(num_graphs + num_valid + i) for i in range(num_test)]

    # -------------------- Input model (:296-367) --------------------
    def input_variables(self):
        """conv1d/{kernel, bias}, conv1d_1/{kernel, bias} at the root scope, created before graph_model/... [TF-internal: Keras
        auto-naming]."""
        num_chars = self.params['graph_node_label_max_num_chars']
        size = self.params['graph_node_label_representation_size']
        return {"conv1d/kernel": ((5, ONE_HOT_DEPTH, 16), "glorot_uniform"), "conv1d/bias": ((16,), "zeros"),
                "conv1d_1/kernel": ((num_chars - 2 * (5 - 1), 16, size), "glorot_uniform"), "conv1d_1/bias": ((size,), "zeros")}

    def compute_initial_node_features(self, batch, weights) -> torch.Tensor:
        w = [weights["conv1d/kernel"], weights["conv1d/bias"], weights["conv1d_1/kernel"], weights["conv1d_1/bias"]]
        chars, label_of_node = batch.initial_node_features, None
        if chars is None:                                # the numpy iterator's feed: unique tables and the shifted maps
            chars, label_of_node = batch.extra['unique_labels_as_characters'], batch.extra['node_labels_to_unique_labels']
            if chars.is_cuda:                            # the per-node table, as the native pipelines carry it (module docstring)
                chars, label_of_node = chars.to(torch.uint8).index_select(0, label_of_node.long()), None
        return node_label_embeddings(chars, label_of_node, *w)

    # -------------------- Output head (:369-448) --------------------
    def output_variable_scope(self, model_has_input_projection: bool) -> str:
        return ""                                        # a NAMED Keras Dense made outside every variable scope

    def output_variables(self, hidden_size: int):
        if self.params['slot_score_via_linear_layer']:
            return {"slot_score_linear_layer/kernel": ((2 * hidden_size + 1, 1), "glorot_uniform")}
        return {}

    # -------------------- Predictions: which candidate belongs into the slot --------------------
    @staticmethod
    def num_nodes_of(sample) -> int:
        return len(sample.node_labels_to_unique_labels)          # (the reference's seven fields: the numpy feed sizes a graph by this)

    def prediction_layout(self, batch, hidden_size: int):
        num_graphs, num_cands = int(batch.num_graphs), int(self.params['max_variable_candidates'])
        return {"probabilities": ((num_graphs, num_cands), torch.float32), "predicted": ((num_graphs,), torch.int32)}

    def compute_task_predictions(self, final_node_representations: torch.Tensor, batch, weights, out=None) -> Dict[str, torch.Tensor]:
        """probabilities float32 [G, max_variable_candidates] and predicted int32 [G], the candidate index tf.argmax(tf.nn.softmax(
        logits)) names (:438; 0 is the correct one): the arithmetic by which the head counts num_correct_predictions
        (csrc/common.h: candidate_choice).  Runs the head's forward on whichever route compute_task_metrics takes, for either loss
        function, and drops its metrics; the logits do not depend on the loss.  A padded candidate has probability exactly 0."""
        out = out or {}
        with torch.no_grad():
            self.compute_task_metrics(final_node_representations, batch, weights)
        probabilities, predicted = predict_candidates(self.last_logits, out.get("probabilities"), out.get("predicted"))
        return {"probabilities": probabilities, "predicted": predicted}

    def compute_task_metrics(self, final_node_representations: torch.Tensor, batch, weights) -> Dict[str, torch.Tensor]:
        """No dropout on the final states in any fold (module docstring).  Metrics: loss (mean over the graphs), total_loss,
        accuracy, num_correct_predictions (float32 here; an int32 count in the reference).  `last_logits` keeps the batch's
        logits [G, candidates] (detached), which compute_task_predictions reads."""
        device = final_node_representations.device
        w = weights["slot_score_linear_layer/kernel"] if self.params['slot_score_via_linear_layer'] else None
        slot = _device_tensor(batch.extra['slot_node_ids'], torch.int32, device).reshape(-1)
        cands = _device_tensor(batch.extra['candidate_node_ids'], torch.int32, device)
        mask = _device_tensor(batch.extra['candidate_node_ids_mask'], torch.float32, device)
        first_node = None
        if batch.extra.get('ids_are_graph_local'):
            # each graph's first node, from the batch's node -> graph list (ascending), on the device
            graphs = torch.arange(cands.shape[0], dtype=torch.int32, device=device)
            first_node = torch.searchsorted(batch.graph_nodes_list, graphs).to(torch.int32)
        use_hip = (final_node_representations.is_cuda and final_node_representations.dtype == torch.float32
                   and self.params['loss_function'] == 'max-likelihood'
                   and head_supported(cands.shape[1], final_node_representations.shape[1]))
        ROUTES["head"] = "hip" if use_hip else "composition"
        if use_hip:
            loss, total_loss, accuracy, correct, logits = varmisuse_head(final_node_representations, slot, cands, mask, first_node, w)
            self.last_logits = logits
            return {'loss': loss, 'total_loss': total_loss, 'accuracy': accuracy, 'num_correct_predictions': correct}
        if first_node is not None:
            slot, cands = slot + first_node, cands + first_node.unsqueeze(1)
        logits = head_logits_composition(final_node_representations, slot, cands, mask, w)
        self.last_logits = logits.detach()
        return head_metrics_composition(logits, self.params['loss_function'], self.params['max-margin_loss_margin'])

    # -------------------- Minibatching (:451-538) --------------------
    NODE_PAYLOADS = {"initial_node_features": ("node_features", np.uint8)}
    GRAPH_PAYLOADS = {"slot_node_ids": ("slot_node_id", np.int32), "candidate_node_ids": ("variable_candidate_nodes", np.int32),
                      "candidate_node_ids_mask": ("variable_candidate_nodes_mask", np.float32)}

    def _finish_native_batch(self, batch):
        batch.extra['ids_are_graph_local'] = True        # the per-graph payloads hold graph-local ids; the head adds first-node offsets
        return batch

    def make_native_minibatch_iterator(self, batcher, data_fold: DataFold, max_nodes_per_batch: int,
                                       rng: Optional[np.random.RandomState] = None):
        ids = np.arange(batcher.store.num_graphs)
        if data_fold == DataFold.TRAIN:
            (rng or np.random).shuffle(ids)
        for batch in batcher.iterate(ids, max_nodes_per_batch):
            yield self._finish_native_batch(batch)

    def make_minibatch_iterator(self, data: Iterable[Any], data_fold: DataFold, max_nodes_per_batch: int,
                                rng: Optional[np.random.RandomState] = None) -> Iterator[MinibatchData]:
        """The reference's feed (:479-505) under its placeholder names and dtypes: unique-label tables concatenated (labels are
        unique per graph, not per batch), maps shifted by the running unique-label offset, adjacency lists, slot and candidate ids
        shifted by the node offset.  A batch is flushed when node_offset + n >= max_nodes_per_batch."""
        if data_fold == DataFold.TRAIN:
            (rng or np.random).shuffle(data)
        num_types = self.num_edge_types

        def finalise(graphs: List[GraphSample]) -> MinibatchData:
            node_offsets = np.concatenate([[0], np.cumsum([len(g.node_labels_to_unique_labels) for g in graphs])])
            label_offsets = np.concatenate([[0], np.cumsum([g.unique_labels_as_characters.shape[0] for g in graphs])])
            adjacency, num_edges = [], 0
            for l in range(num_types):
                parts = [np.asarray(g.adjacency_lists[l]).reshape(-1, 2) + off for g, off in zip(graphs, node_offsets)]
                a = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 2), dtype=np.int32)
                num_edges += a.shape[0]
                adjacency.append(a)
            feed = {
                'unique_labels_as_characters': np.concatenate([g.unique_labels_as_characters for g in graphs], axis=0).astype(np.int32),
                'node_labels_to_unique_labels': np.concatenate([g.node_labels_to_unique_labels + off
                                                                for g, off in zip(graphs, label_offsets)], axis=0).astype(np.int32),
                'type_to_num_incoming_edges': np.concatenate([g.type_to_node_to_num_incoming_edges for g in graphs],
                                                             axis=1).astype(np.float32),
                'slot_node_ids': np.array([g.slot_node_id + off for g, off in zip(graphs, node_offsets)], dtype=np.int32),
                'candidate_node_ids': np.stack([g.variable_candidate_nodes + off for g, off in zip(graphs, node_offsets)]).astype(np.int32),
                'candidate_node_ids_mask': np.stack([g.variable_candidate_nodes_mask for g in graphs]).astype(np.float32),
                'adjacency_lists': adjacency,
            }
            return MinibatchData(feed_dict=feed, num_graphs=len(graphs), num_nodes=int(node_offsets[-1]), num_edges=num_edges)

        current, node_offset = [], 0
        for graph in data:
            num_nodes = len(graph.node_labels_to_unique_labels)
            if node_offset + num_nodes >= max_nodes_per_batch:
                if not current:
                    raise ValueError("a graph of %d nodes does not fit max_nodes_per_batch=%d" % (num_nodes, max_nodes_per_batch))
                yield finalise(current)
                current, node_offset = [], 0
            current.append(graph)
            node_offset += num_nodes
        if current:
            yield finalise(current)

    def loss_weight(self, num_graphs: int, num_nodes: int) -> float:
        return float(num_graphs)             # the loss is a mean over the batch's graphs (compute_task_metrics)

    def early_stopping_metric(self, task_metric_results: List[Dict[str, Any]], num_graphs: int) -> float:
        # :540-543: accuracy, negated (the loop minimises)
        return -(sum(float(m['num_correct_predictions']) for m in task_metric_results) / float(num_graphs))

    def pretty_print_epoch_task_metrics(self, task_metric_results: List[Dict[str, Any]], num_graphs: int) -> str:
        acc = sum(float(m['num_correct_predictions']) for m in task_metric_results) / float(num_graphs)
        return "Accuracy: %.3f" % (acc,)
