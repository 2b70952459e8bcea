"""Model driver mirror (models/sparse_graph_model.py of the reference).

Hot-path scope: the per-layer loop of __build_graph_propagation_model
(:162-202) and the abstract hook _apply_gnn_layer (:204-225), same names and argument meaning.
The training-step plumbing around it (optimizer with per-variable clip_by_norm :227-260, epoch
loop with throughput counters :263-311) is restated minimally so that the reference's own
"edges/sec" number (README.md:34-35) can be measured end to end.

TF1 builds a static graph once and feeds numpy batches through sess.run; here the variables
live in a VariableStore under the reference's TF names, batches live in HBM (DeviceBatch), and a
step is eager PyTorch-ROCm around the librelgnn HIP kernels.
"""
import os
import pickle
import time
from abc import ABC, abstractmethod
from contextlib import nullcontext
from typing import Any, Dict, Iterable, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from .. import ops
from ..dense import capture_image_cache, dense_act, vouch_sole_consumer, weights_changed
from ..graph import as_rel_graph, check_pending_graph_errors
from ..tasks import DataFold, DeviceBatch, Sparse_Graph_Task
from ..tasks.batcher import NativeBatcher
from ..tasks.layerwise import target_windows, window_blocker
from ..tasks.resident import ResidentDataset
from ..tasks.sparse_features import SparseRows
from ..utils import get_activation, layer_norm, layer_norm_scope
from ..variables import VariableStore
from .data_parallel import data_parallel
from .optimizer import TFStyleOptimizer
from .readback import EpochTally, LateFetch, MetricsReadback, _PredictionArena


class CapturedTrainStep:
    """A training step recorded as a hipGraph on one fixed batch (Sparse_Graph_Model.capture_train_step), with any of the
    three optimizers.  Adam's step count is device state that every replay advances; the learning rate of an RMSProp or SGD
    step is a launch scalar of the recorded update."""

    def __init__(self, model, graph, metrics, batch):
        self.model, self.graph, self.metrics, self.batch = model, graph, metrics, batch
        self._expected_t = model.optimizer.t

    def replay(self) -> Dict[str, torch.Tensor]:
        """One more training step: a single graph launch.  The returned tensors are overwritten by the next replay.
        With Adam the graph reads the step count from device memory; if the host count moved since the last replay (an eager
        train_step(), load_weights()), the device copy is re-seeded first, so lr_t never comes from a stale count.  RMSProp and
        SGD keep no device state (the re-seeding is a no-op): their update does not depend on the step count.
        (lr_t of a replayed step is computed in float32 on the device, of an eager step in double on the host: the two
        agree to ~1e-7 relative, not bit for bit.)"""
        opt = self.model.optimizer
        if opt.t != self._expected_t:
            opt.sync_device_step_count()
        self.graph.replay()
        weights_changed()                  # the replayed update rewrote the parameters: limb images kept by eager code are stale
        opt.t += 1
        self._expected_t = opt.t
        return self.metrics

    def handover_status(self) -> int:
        """The device's hand-over status word (ops.handover_status: synchronises).  A replay loop that reads the metric tensors
        itself instead of going through MetricsReadback checks this where it syncs anyway."""
        return ops.handover_status(device=self.model.device)


class Sparse_Graph_Model(ABC):
    """Abstract superclass of all graph models (reference docstring: models/sparse_graph_model.py:16-20)."""

    @classmethod
    def default_params(cls):
        # models/sparse_graph_model.py:22-45
        return {
            'max_nodes_in_batch': 50000,
            'graph_num_layers': 8,
            'graph_num_timesteps_per_layer': 1,
            'graph_layer_input_dropout_keep_prob': 0.8,
            'graph_dense_between_every_num_gnn_layers': 1,
            'graph_model_activation_function': 'tanh',
            'graph_residual_connection_every_num_layers': 2,
            'graph_inter_layer_norm': False,
            'max_epochs': 10000,
            'patience': 25,
            'optimizer': 'Adam',
            'learning_rate': 0.001,
            'learning_rate_decay': 0.98,
            'lr_for_num_graphs_per_batch': None,
            'momentum': 0.85,
            'clamp_gradient_norm': 1.0,
            'random_seed': 0,
        }

    @staticmethod
    @abstractmethod
    def name(params: Dict[str, Any]) -> str:
        raise NotImplementedError()

    def __init__(self, params: Dict[str, Any], task: Sparse_Graph_Task, run_id: str = "run",
                 result_dir: str = ".", device: Optional[str] = None) -> None:
        self.params = params
        self.task = task
        self.run_id = run_id
        self.result_dir = result_dir
        self.device = torch.device(device if device is not None else "cuda")
        self._native_batchers = {}
        self.training = False
        # under a process group only rank 0 logs (the drivers form the group before they build the model; train(group=...) /
        # test(group=...) go by the rank within THEIR group)
        self._log_rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        torch.manual_seed(params['random_seed'])
        np.random.seed(params['random_seed'])
        if self.device.type == "cuda":
            # the hand-over status block of this device (ops.handover_word): exists before any step can be captured into a hipGraph;
            # read back with every step's metrics (MetricsReadback) and by handover_status()
            self.handover_word = ops.handover_word(self.device)
            # the state block of the fused layer-input dropout (ops.dropout): {seed, replica, step} in HBM, next to the hand-over
            # word for the same reason (a captured step needs a live pointer).  replica = the data-parallel rank (the drivers form
            # their process group before they build the model), so that ranks do not share masks
            self.dropout_state = ops.dropout_state(self.device, params['random_seed'], self._log_rank, 0)
        self.variables = VariableStore(seed=params['random_seed'])
        self.__make_model()
        self.variables.to(self.device)
        self.__make_train_step()

    @property
    def log_file(self):
        return os.path.join(self.result_dir, "%s.log" % self.run_id)

    @property
    def best_model_file(self):
        return os.path.join(self.result_dir, "%s_best_model.pickle" % self.run_id)

    def log_line(self, msg):
        if self._log_rank != 0:
            return
        try:
            with open(self.log_file, 'a') as log_fh:
                log_fh.write(msg + '\n')
        except OSError:
            pass
        print(msg)

    # -------------------- Model Saving/Loading (reference pickle layout :91-126) --------------------
    def save_model(self, path: str) -> None:
        self.optimizer.flush_deferred()    # (a row-deferred parameter, `sparse_update`: its tensor holds stale rows between training steps)
        data_to_save = {
            "model_class": self.name(self.params),
            "task_class": self.task.name(),
            "model_params": self.params,
            "task_params": self.task.params,
            "task_metadata": self.task.get_metadata(),
            # every GLOBAL_VARIABLE of the TF graph: the model variables and the optimizer's slots
            "weights": dict(self.variables.tf_weights(), **self.optimizer.tf_slot_weights(self._trainable_names())),
        }
        with open(path, 'wb') as out_file:
            pickle.dump(data_to_save, out_file, pickle.HIGHEST_PROTOCOL)

    def _trainable_names(self) -> List[str]:
        return [n for n in self.variables.names() if self.variables[n].requires_grad]

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """:109-126: assign every variable the pickle names (model variables and optimizer slots), freshly initialise
        (= keep the initial value of) the ones it does not, report saved entries nothing consumed."""
        self.optimizer.flush_deferred()    # (before anything is overwritten: a replay behind it would run on the loaded values)
        used = self.variables.load_tf_weights(weights, report_unused=False)
        used |= self.optimizer.load_tf_slots(weights, self._trainable_names())
        weights_changed()                  # (copy_ moves the version counters too; said once more for limb images kept per step)
        for var_name in weights:
            if var_name not in used:
                print('Saved weights for %s not used by model.' % var_name)

    # -------------------- Model Construction --------------------
    @abstractmethod
    def _gnn_layer_variables(self, in_dim: int) -> Dict[str, Any]:
        """TF-relative variable specs of ONE gnn layer (what the reference's layer function would
        create under variable_scope('gnn_layer_%i'))."""
        raise NotImplementedError()

    def __make_model(self):
        p = self.params
        h_dim = p['hidden_size']
        vs = self.variables
        vs.create_all("", self.task.input_variables())            # :138 make_task_input_model runs before the propagation model
        if self.task.initial_node_feature_size != h_dim:          # :165-170, unnamed Keras Dense
            vs.create("graph_model/dense/kernel", (self.task.initial_node_feature_size, h_dim))
        self._inter_norm_name = []
        for layer_idx in range(p['graph_num_layers']):            # :176-200
            scope = "graph_model/gnn_layer_%i" % layer_idx
            specs = dict(self._gnn_layer_variables(h_dim))
            if p['graph_inter_layer_norm']:
                own = sum(1 for k in specs if k.startswith("LayerNorm") and k.endswith("/gamma"))
                ln = layer_norm_scope(own)          # TF uniquifies: the scope after the layer's own per-timestep norms
                specs[ln + "/beta"] = ((h_dim,), "zeros")
                specs[ln + "/gamma"] = ((h_dim,), "ones")
                self._inter_norm_name.append(ln)
            else:
                self._inter_norm_name.append(None)
            if layer_idx % p['graph_dense_between_every_num_gnn_layers'] == 0:
                specs["Dense/kernel"] = ((h_dim, h_dim), "glorot_uniform")
            vs.create_all(scope, specs)
        # The task names its own output variables (absolute TF scope): PPI's head is an UNNAMED Keras Dense, which TF
        # auto-names after the model's unnamed input projection ("dense" -> "dense_1", tasks/ppi_task.py:176-179);
        # QM9's heads live under variable_scope("out_layer_task%i") at the root (tasks/qm9_task.py:163-176).
        has_projection = self.task.initial_node_feature_size != h_dim
        self._task_scope = self.task.output_variable_scope(has_projection)
        vs.create_all(self._task_scope, self.task.output_variables(h_dim))
        self.log_line("Model has %i parameters." % vs.num_parameters())

    def _project_input(self, initial_node_features, w, act_id: int, sole_consumer: bool) -> torch.Tensor:
        """:165-170: the unnamed Dense in front of the first layer, when the feature size differs from hidden_size.  Features that
        a task keeps sparse (tasks/sparse_features.py, the citation task's sparse_node_features mode) gather rows of the same
        `dense/kernel` instead (ops.csr_rows_project); without a projection they are densified on the device.  With the citation
        task's `"sparse_gradient": true` the optimizer's sink goes along: the backward leaves the weight's gradient there as the
        rows the batch names, not in `.grad`."""
        has_projection = self.task.initial_node_feature_size != self.params['hidden_size']
        if isinstance(initial_node_features, SparseRows):
            if has_projection:
                optimizer = getattr(self, "optimizer", None)
                sink = optimizer.row_gradient_sink if optimizer is not None and torch.is_grad_enabled() else None
                return ops.csr_rows_project(initial_node_features, w["dense/kernel"], act_id, row_gradient_sink=sink)
            return initial_node_features.to_dense()
        if has_projection:
            return dense_act(initial_node_features, w["dense/kernel"], None, act_id, sole_consumer=sole_consumer)
        return initial_node_features

    def compute_final_node_representations(self, initial_node_features: torch.Tensor,
                                           adjacency_lists, type_to_num_incoming_edges: torch.Tensor,
                                           dropout_keep_prob: float = 1.0, layer_graphs=None) -> torch.Tensor:
        """__build_graph_propagation_model, models/sparse_graph_model.py:162-202.

        layer_graphs (the citation task's `"layered": true`; tasks/neighbour_sampling.py, LevelGraph): one entry per layer.  Layer
        l then runs on its level's graph and degree table over num_sources input rows, and its output is cut to num_targets rows
        before the inter-layer norm and the Dense (both row-wise) read it; at a residual step the kept tensor is cut to the current
        row count.  The result has the last level's num_targets rows: the seeds.  The row cut sits between a producer and its
        consumer, which is what the folding of activation gradients (dense.py) must not straddle: in this mode the driver vouches
        for nothing, the route a keep-probability below 1 takes.

        Dropout on the layer inputs (keep-prob < 1) is torch.nn.functional.dropout by default.  With
        config.settings.layer_dropout == "fused" a contiguous fp32 GPU input takes ops.dropout / ops.dropout_residual instead (one
        kernel per layer, the residual average included; no mask stored): the masks are Philox4x32-10 draws keyed by
        self.dropout_state = {random_seed, replica, step} with the layer index as the stream.  The step is bumped here, on the
        device, once per call that drops anything, so every pass (and every replay of a captured step) draws new masks; each pass
        works on its own 24-byte copy of the state, which its backward reads again.  The step is NOT written to checkpoints (the
        reference's pickle layout has no place for it): a restored model starts at step 0."""
        p = self.params
        activation_fn = get_activation(p['graph_model_activation_function'])
        w = self.variables.scope("graph_model")
        num_nodes = initial_node_features.shape[0]
        # bucketed once, shared by every layer; the index range check is read back at the next fetch
        graph = as_rel_graph(adjacency_lists, num_nodes, validate="deferred")
        layered = layer_graphs is not None
        if layered and (len(layer_graphs) != p['graph_num_layers'] or layer_graphs[0].num_sources != num_nodes):
            raise ValueError("layer_graphs: %d levels, the first over %d nodes, for a model of %d layers and %d input rows"
                             % (len(layer_graphs), layer_graphs[0].num_sources if layer_graphs else 0, p['graph_num_layers'], num_nodes))
        act_id = ops.activation_id(p['graph_model_activation_function'])
        num_layers, res_every = p['graph_num_layers'], p['graph_residual_connection_every_num_layers']

        def only_the_next_layer_reads(next_layer_idx: int) -> bool:
            """Is the layer function of iteration `next_layer_idx` the only reader of the tensor handed to it?  (One of the two words
            that let a layer fold a non-idempotent activation gradient — tanh' of the Dense below it — into its input-gradient
            product: dense.py, "activation gradients folded into the product that feeds them"; the other one is the layer's own:
            that it reads its input once.)  At a residual step the tensor is read by the average instead (and kept for the next
            residual step); at layer 0 it is kept for the first residual step too."""
            if next_layer_idx >= num_layers or dropout_keep_prob < 1.0 or layered:
                return False
            if next_layer_idx % res_every == 0:
                return next_layer_idx == 0 and res_every >= num_layers
            return True

        cur_node_representations = self._project_input(initial_node_features, w, act_id, only_the_next_layer_reads(0))
        last_residual_representations = None          # (the reference's zeros_like is overwritten at layer 0 before any use)
        pass_state = None
        if ops.fused_dropout_on(dropout_keep_prob) and getattr(self, "dropout_state", None) is not None:
            with torch.no_grad():
                self.dropout_state[2].add_(1)                  # on the device, stream-ordered: every replay of a captured step advances it
                pass_state = self.dropout_state.clone()        # this pass's 24 bytes: read by its forward kernels and by its backward
        for layer_idx in range(p['graph_num_layers']):
            cur_node_representations, last_residual_representations = self._layer_step(
                layer_idx, cur_node_representations, last_residual_representations, graph, type_to_num_incoming_edges,
                layer_graphs[layer_idx] if layered else None, dropout_keep_prob, pass_state, only_the_next_layer_reads(layer_idx + 1),
                w, act_id)
        return vouch_sole_consumer(cur_node_representations, False)     # (a task head may read it more than once)

    def _layer_step(self, layer_idx: int, cur_node_representations: torch.Tensor, last_residual_representations, graph,
                    type_to_num_incoming_edges: torch.Tensor, level, dropout_keep_prob: float, pass_state,
                    next_layer_reads_alone: bool, w, act_id: int):
        """One iteration of the layer loop (:176-200): the residual average, the layer function on a graph, the cut to the level's
        num_targets, the inter-layer norm and the Dense.  -> (the layer's output, the tensor kept for the next residual step).
        level (a LevelGraph, or a WindowBlock of the layer-wise pass; None: the batch's own `graph` and degree table): the layer runs on
        the level's graph and degree table over its num_sources rows.  Both compute_final_node_representations and
        layerwise_final_node_representations run their layers through here; w is the scope "graph_model", act_id the model's
        activation."""
        p = self.params
        layered = level is not None
        self._layer_weights = w.scope('gnn_layer_%i' % layer_idx)
        residual_step = layer_idx % p['graph_residual_connection_every_num_layers'] == 0
        layer_degrees = type_to_num_incoming_edges
        if layered:
            if cur_node_representations.shape[0] != level.num_sources:
                raise ValueError("layer_graphs: level %d takes %d rows, the layer below it left %d"
                                 % (layer_idx + 1, level.num_sources, cur_node_representations.shape[0]))
            # (level 1 is the union graph: the same key, the same cached bucketing)
            # (an evaluation batch brings every level's bucketing along, routed as the full graph's)
            graph = as_rel_graph(level.graph if getattr(level, "graph", None) is not None else level.adjacency_lists,
                                 level.num_sources, validate="deferred")
            layer_degrees = level.type_to_num_incoming_edges
            if residual_step and layer_idx > 0 and last_residual_representations.shape[0] > level.num_sources:
                last_residual_representations = last_residual_representations[:level.num_sources]
        if pass_state is not None and ops.dropout_tensor_ok(cur_node_representations):
            # csrc/dropout.hip: one kernel for the whole layer-input stage; the layer index is the Philox stream
            if residual_step and layer_idx > 0:
                last_residual_representations, cur_node_representations = ops.dropout_residual(
                    cur_node_representations, last_residual_representations, dropout_keep_prob, pass_state, layer_idx)
            else:
                cur_node_representations = ops.dropout(cur_node_representations, dropout_keep_prob, pass_state, layer_idx)
                if residual_step:
                    last_residual_representations = cur_node_representations
        else:
            if dropout_keep_prob < 1.0:
                cur_node_representations = torch.nn.functional.dropout(
                    cur_node_representations, p=1.0 - dropout_keep_prob, training=True)
            if residual_step:
                t = cur_node_representations
                if layer_idx > 0:
                    cur_node_representations = (cur_node_representations + last_residual_representations) / 2
                last_residual_representations = t
        cur_node_representations = self._apply_gnn_layer(
            cur_node_representations, graph, layer_degrees, p['graph_num_timesteps_per_layer'])
        if layered and level.num_targets < cur_node_representations.shape[0]:
            cur_node_representations = cur_node_representations[:level.num_targets]      # (a view: it carries no activation tag)
        if p['graph_inter_layer_norm']:
            ln = self._inter_norm_name[layer_idx]
            cur_node_representations = layer_norm(cur_node_representations,
                                                  self._layer_weights[ln + "/gamma"], self._layer_weights[ln + "/beta"])
        if layer_idx % p['graph_dense_between_every_num_gnn_layers'] == 0:
            # (the layer's / the norm's output is referenced nowhere else: this Dense is its only reader)
            cur_node_representations = dense_act(vouch_sole_consumer(cur_node_representations, not layered),
                                                 self._layer_weights["Dense/kernel"], None, act_id,
                                                 sole_consumer=next_layer_reads_alone, sole_reader=True)
        else:
            vouch_sole_consumer(cur_node_representations, next_layer_reads_alone)
        return cur_node_representations, last_residual_representations

    def layerwise_final_node_representations(self, batch: DeviceBatch, rows_per_batch: int, blocks=None) -> torch.Tensor:
        """The final node states of a full-graph batch, computed layer by layer over windows of `rows_per_batch` target rows (the
        citation task's `layerwise_evaluation`; tasks/layerwise.py): layer l for ALL nodes from the [V, hidden] table of layer l - 1,
        then layer l + 1.  Under torch.no_grad() and keep-probability 1.

        The input projection runs over the whole graph as the full-graph path runs it; its result is table 0.  Per layer and window
        the input rows are table[block.nodes], the layer step is _layer_step on the block's graph and degree table, and its T output
        rows are rows [a, b) of the next table.  The residual average is row-wise: it is taken over the rows gathered from the kept
        residual table; a residual step keeps its input table.  At most three [V, hidden] tables are alive (current, next, the last
        residual step's input), two when no residual step lies ahead.
        blocks (tasks/layerwise.KeptBlocks; `"keep": true`): the windows' blocks are built once per (device, B, route) and kept there;
        None: they are built again for every layer and dropped.  A window's block is the same for every layer."""
        p = self.params
        if self.device.type != "cuda":
            raise RuntimeError("layerwise_evaluation needs a model on the GPU: the window block is a HIP kernel and there is no CPU "
                               "fallback (the model is on %s)" % self.device)
        problem = self._layerwise_prerequisites()
        if problem is not None:
            raise ValueError("layerwise_evaluation requires %s" % problem)
        num_layers, res_every = p['graph_num_layers'], p['graph_residual_connection_every_num_layers']
        act_id = ops.activation_id(p['graph_model_activation_function'])
        with torch.no_grad():
            batch.wait_ready()
            features = self.task.compute_initial_node_features(batch, self.variables.scope(""))
            num_nodes = features.shape[0]
            own = getattr(batch, "graph", None)
            full = as_rel_graph(own if own is not None else batch.adjacency_lists, num_nodes, validate="deferred")
            key = (str(full.device), int(rows_per_batch), bool(full.has_long_buckets))
            kept = blocks.get(key) if blocks is not None else None

            def window_blocks():
                if kept is not None:
                    return kept
                blocker = window_blocker(full)
                ends = blocker.boundaries(rows_per_batch)         # (the host copy of rowptr_t at the window boundaries: one read per (graph, B))
                return (blocker.block(a, b, full, (ends[a], ends[b])) for a, b in target_windows(num_nodes, rows_per_batch))

            w = self.variables.scope("graph_model")
            table = self._project_input(features, w, act_id, False)
            if table is features:                 # (no projection: the batch's own feature table is not ours to drop or overwrite)
                features = None
            del features
            residual = None
            for layer_idx in range(num_layers):
                residual_step = layer_idx % res_every == 0
                following = torch.empty((num_nodes, p['hidden_size']), dtype=table.dtype, device=table.device)
                built = []
                for block in window_blocks():
                    index = block.nodes.long()
                    rows = table.index_select(0, index)
                    kept_rows = residual.index_select(0, index) if residual_step and layer_idx > 0 else None
                    out, _ = self._layer_step(layer_idx, rows, kept_rows, None, None, block, 1.0, None, False, w, act_id)
                    following[block.first:block.last] = out
                    if blocks is not None and kept is None:
                        built.append(block)
                    del block, index, rows, kept_rows, out
                if blocks is not None and kept is None:
                    kept = blocks.put(key, built)         # (only a whole layer's list is kept)
                if residual_step:
                    residual = table              # a residual step keeps its input table
                if not any(later % res_every == 0 for later in range(layer_idx + 1, num_layers)):
                    residual = None               # no residual step lies ahead: two tables
                table = following
                del following
            return table

    def _layerwise_prerequisites(self) -> Optional[str]:
        """What the layer-wise pass needs and this model lacks, None when it can run it: _layered_prerequisites with one hop per
        layer, which leaves its check of the timesteps (a window's block is one hop, and a layer of several timesteps reads
        neighbours of neighbours)."""
        return self._layered_prerequisites([0] * self.params['graph_num_layers'])

    @abstractmethod
    def _apply_gnn_layer(self,
                         node_representations: torch.Tensor,
                         adjacency_lists: List[torch.Tensor],
                         type_to_num_incoming_edges: torch.Tensor,
                         num_timesteps: int) -> torch.Tensor:
        """Run a GNN layer on a graph (models/sparse_graph_model.py:204-225; same arguments).
        The current layer's variables are available as self._layer_weights."""
        raise Exception("Models have to implement _apply_gnn_layer!")

    def __make_train_step(self):
        p = self.params
        self.optimizer = TFStyleOptimizer(list(self.variables.parameters()), p['optimizer'], p['learning_rate'],
                                          p['clamp_gradient_norm'], decay=p['learning_rate_decay'],
                                          momentum=p['momentum'])
        need = self.task.model_requirements()
        for fanouts, refusal in need.layered:
            problem = self._layered_prerequisites(fanouts)
            if problem is not None:
                raise ValueError(refusal % problem)
        if need.layerwise is not None:
            problem = self._layerwise_prerequisites()
            if problem is not None:
                raise ValueError(need.layerwise % problem)
        if need.message_scale is not None:
            problem = self._message_scale_prerequisites()
            if problem is not None:
                raise ValueError(need.message_scale % problem)
        if need.deferred_projection_rows:
            # the citation task's `sampled_batches` key "sparse_update": the weight of the sparse input projection is updated by rows.
            # CONTRACT: between training steps that parameter's tensor (and its two Adam slots) hold stale rows; everything here that
            # reads them outside a training step calls self.optimizer.flush_deferred() first (forward_batch(training=False),
            # predict_iter, save_model, load_weights), and so must anyone who reads self.variables directly.
            if self.optimizer.name != 'adam':
                raise ValueError('sampled_batches: "sparse_update": true requires the optimizer Adam (got %r): the row-deferred update '
                                 'replays Adam steps' % (p['optimizer'],))
            if "graph_model/dense/kernel" not in self.variables:
                raise ValueError('sampled_batches: "sparse_update": true requires a model with the input projection '
                                 'graph_model/dense/kernel (hidden_size %d equals the feature size: there is none)' % p['hidden_size'])
            self.optimizer.defer_rows(self.variables["graph_model/dense/kernel"])
            if need.compact_projection_gradient:
                # "sparse_gradient": that weight's gradient exists only as the rows a batch names (_project_input hands the sink on)
                self.optimizer.compact_row_gradient()

    def _message_scale_prerequisites(self) -> Optional[str]:
        """What a batch whose degree scale is a weight per message (the citation task's `subgraph_batches` key "normalisation" with
        "aggregation": true) needs and this model lacks, None when its layers take that scale: the layer function reads the degree
        table, normalises by it, and SUMS the scaled messages.  The adapters answer from their spec (models/adapters.py)."""
        return "a model whose layers read the in-degree scale (this one says nothing about its layers)"

    def _layered_prerequisites(self, fanouts) -> Optional[str]:
        """What a layered batch of these fanouts needs and this model lacks, None when it can run one."""
        p = self.params
        if len(fanouts) != p['graph_num_layers']:
            return "as many fanouts as graph_num_layers (got %d fanouts for %d layers)" % (len(fanouts), p['graph_num_layers'])
        if p['graph_num_timesteps_per_layer'] != 1:
            return "graph_num_timesteps_per_layer 1 (got %r)" % (p['graph_num_timesteps_per_layer'],)
        return None

    # -------------------- Training Loop --------------------
    def _final_node_states(self, batch: DeviceBatch, training: bool) -> torch.Tensor:
        keep = self.params['graph_layer_input_dropout_keep_prob'] if training else 1.0
        batch.wait_ready()               # assembled on a side stream (tasks/resident.py)? wait on the GPU, not the host
        plan = None if training else batch.extra.get('layerwise_evaluation')
        if plan is not None:             # a full-graph evaluation batch of a task that asks for the layer-wise pass (tasks/layerwise.py)
            return self.layerwise_final_node_representations(batch, plan.rows_per_batch, blocks=plan.blocks)
        # a batch from the input pipeline may carry its bucketing, built on a side stream (tasks/batcher.py)
        graph = getattr(batch, "graph", None)
        return self.compute_final_node_representations(
            self.task.compute_initial_node_features(batch, self.variables.scope("")),
            graph if graph is not None else batch.adjacency_lists,
            batch.type_to_num_incoming_edges, keep, layer_graphs=batch.extra.get('layer_graphs'))

    def forward_batch(self, batch: DeviceBatch, training: bool):
        """training=False with a row-deferred parameter (`sparse_update`): every row is brought up to date first; a training forward
        relies on train_step's rows_touched()."""
        if not training:
            self.optimizer.flush_deferred()
        final = self._final_node_states(batch, training)
        return self.task.compute_task_metrics(final, batch, self.variables.scope(self._task_scope))

    def capture_train_step(self, batch: DeviceBatch, warmup_steps: int = 3):
        """One full training step on a FIXED batch as a hipGraph (forward, backward, clip, update with Adam, RMSProp or SGD:
        ~150 launches replayed with one host call).  For workloads whose step is host-enqueue bound (C3: 153 k messages per
        batch) and whose batch shapes repeat.  Runs `warmup_steps` real steps first (allocator / plan caches), then captures;
        returns a CapturedTrainStep whose replay() performs exactly one more step and returns the (static) metric tensors.
        The learning rate of a captured RMSProp or SGD step is a launch scalar.  With lr_for_num_graphs_per_batch set it is
        learning_rate * num_graphs / lr_for_num_graphs_per_batch of THIS batch: constant for the fixed batch, so freezing it
        into the graph is correct (Adam's lr_t changes per step and is computed on the device instead)."""
        if 'sampled_nodes' in batch.extra:
            raise RuntimeError("capture_train_step records ONE fixed batch; a sampled batch (tasks/neighbour_sampling.py) has another "
                               "shape every step")
        if self.task.model_requirements().layerwise is not None:
            raise RuntimeError("capture_train_step records ONE fixed batch; a task with layerwise_evaluation (tasks/layerwise.py) runs "
                               "its evaluation window by window, with a read-back per window")
        if self.device.type != "cuda":
            raise RuntimeError("capture_train_step needs a model on the GPU (a hipGraph records GPU work)")
        batch.wait_ready()
        if getattr(batch, "graph", None) is None:           # the bucketing is part of the fixed batch, not of the step
            batch.graph = as_rel_graph(batch.adjacency_lists, batch.num_nodes, validate=True)
        opt = self.optimizer
        opt.sync_device_step_count()
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup_steps):
                self.train_step(batch, device_step_count=True)
                opt.t += 1
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad()
        with capture_image_cache(), torch.cuda.graph(graph):      # (limb images of the weights: split once per captured step)
            metrics = self.train_step(batch, device_step_count=True)
        return CapturedTrainStep(self, graph, {k: v for k, v in metrics.items() if torch.is_tensor(v)}, batch)

    _backward_seed: Dict[Any, torch.Tensor] = {}

    def train_step(self, batch: DeviceBatch, grad_hook=None, device_step_count: bool = False,
                   pre_backward=None, lr_num_graphs: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """forward + backward + per-variable clip + optimizer update == one sess.run with train_step (:287-293).
        pre_backward(): called between the forward and the backward (a bucketed gradient all-reduce arms its hooks there);
        grad_hook(params): between the backward and the clipping (the data-parallel reduction);
        lr_num_graphs: the graph count lr_for_num_graphs_per_batch scales by (data-parallel: the step's global count)."""
        self.optimizer.zero_grad()
        self._name_touched_rows(batch)
        metrics = self.forward_batch(batch, training=True)
        if pre_backward is not None:
            pre_backward()
        # one process drives one GPU: running the backward on the calling thread instead of the autograd engine's
        # device thread saves the hand-off per node (host enqueue 1.56 -> 1.29 ms per C2 step) and a busy CPU thread
        # (the weight gradients of the aggregate-first layers run on a side stream; nothing reads them before the reduction / the
        #  optimizer, so their joins move behind the whole backward — not with a reducer that packs gradients from hooks DURING it)
        # (measured on the C2 step, alternated three times: 1.812 / 1.812 / 1.814 ms with the joins per layer, 1.804 / 1.806 / 1.806 deferred)
        defer = ops.deferred_weight_gradient_join() if pre_backward is None else nullcontext()
        with torch.autograd.set_multithreading_enabled(False), defer:
            loss = metrics['loss']
            one = self._backward_seed.get((loss.device, loss.dtype, loss.shape))
            if one is None:       # (loss.backward() would fill a fresh ones_like every step)
                one = self._backward_seed[(loss.device, loss.dtype, loss.shape)] = torch.ones_like(loss)
            loss.backward(gradient=one)
        ops.join_deferred()
        if grad_hook is not None:  # data-parallel gradient all-reduce goes here (before clipping)
            grad_hook(self.optimizer.params)
        lr_scale = self._lr_scale(batch.num_graphs if lr_num_graphs is None else lr_num_graphs)
        self.optimizer.clip_and_step(lr_scale, device_step_count=device_step_count)
        return metrics

    def _name_touched_rows(self, batch: DeviceBatch) -> None:
        """With a row-deferred projection weight (`sparse_update`): the rows this step's forward reads and its update writes are the
        non-empty rows of the transposed structure of the batch's SparseRows (a sampled batch's own container, or the fold's for a
        full-graph sparse batch); they catch up before the forward.  Nothing otherwise."""
        if getattr(self.optimizer, "_deferred", None) is None:
            return
        batch.wait_ready()                 # (a batch assembled on a side stream: a per-batch container records its tensors for this one)
        rows = self.task.compute_initial_node_features(batch, self.variables.scope(""))
        if not isinstance(rows, SparseRows):
            raise RuntimeError("sparse_update: a training batch without sparse node features cannot name the rows it touches")
        if self.optimizer.row_gradient_sink is not None:
            rows.named_rows()              # (`sparse_gradient`: a sampled batch's container brought them along; any other builds them now)
        self.optimizer.rows_touched(rows.transposed.rowptr)

    def _lr_scale(self, num_graphs: int) -> float:
        lr_n = self.params.get('lr_for_num_graphs_per_batch')
        return 1.0 if lr_n is None else float(num_graphs) / float(lr_n)

    def _native_batching(self) -> bool:
        return bool(self.params.get('native_batching', True) and torch.device(self.device).type == "cuda"
                    and hasattr(self.task, "make_graph_store"))

    def _batches(self, data, data_fold: DataFold, full_graph: bool = False):
        """Batches of one epoch.  On the GPU the data fold is flattened once and batches come from the C++ builder
        (tasks/batcher.py: packed in pinned memory on a background thread, one async upload each), the stand-in for
        the reference's ThreadedIterator (:272); `native_batching: false` keeps the numpy iterator.  full_graph: the task's
        "evaluation" key is not consulted (predict(data) without nodes)."""
        native = self._native_batching()
        # a single-graph task draws its sampled batches itself, on this device: no flattened or resident copy of the fold is built
        own = self.task.epoch_batches(data, data_fold, self.device, self._full_graph_route(native), full_graph)
        if own is not None:
            return own
        if not native:
            return self.task.make_minibatch_iterator(data, data_fold, self.params['max_nodes_in_batch'])
        return self.task.make_native_minibatch_iterator(self._native_pipeline(data), data_fold, self.params['max_nodes_in_batch'])

    def _full_graph_route(self, native: bool) -> bool:
        """Would this model's full-graph batch of a single-graph fold be a resident one?  (tasks/resident.py splits the hub buckets
        of such a batch; the graph the model buckets itself keeps one wave per bucket.)  A batch of receptive fields routes its
        reductions the same way, so that an exact field reproduces the full-graph rows."""
        return bool(native and self.params.get('resident_dataset', 'auto') is not False)

    def _native_pipeline(self, data):
        """The input pipeline of one data fold (ResidentDataset or NativeBatcher over its GraphStore), built once and kept."""
        key = (id(data), len(data))
        cached = self._native_batchers.get(key)
        if cached is not None and cached[0] is data:
            self._native_batchers[key] = self._native_batchers.pop(key)      # most recently used last
        if cached is None or cached[0] is not data:
            store = self.task.make_graph_store(data)
            pipeline = None
            # small enough folds simply live in HBM, bucketed once (tasks/resident.py); `resident_dataset: false`
            # keeps the host packer, `true` insists
            want = self.params.get('resident_dataset', 'auto')
            if want is True or (want == 'auto' and self._fold_fits_hbm(store)):
                try:
                    pipeline = ResidentDataset(store, self.device)
                except ValueError:
                    if want is True:
                        raise
            if pipeline is None:
                pipeline = NativeBatcher(store, self.device)
            cached = (data, pipeline)
            self._native_batchers[key] = cached
            # train + validation folds (and one more) stay; anything older — e.g. the fresh list every test() call
            # passes — is dropped so that its resident copy of the fold and its pinned arenas are released
            while len(self._native_batchers) > 3:
                self._native_batchers.pop(next(iter(self._native_batchers)))
        return cached[1]

    @staticmethod
    def _fold_fits_hbm(store, budget_bytes: int = 32 << 30) -> bool:
        """Flat arrays + fold-level bucketing (~9 int32 per message) well inside the 288 GB of an MI355X."""
        nbytes = sum(a.nbytes for a in store.payload) + sum(a.nbytes for a in store.adj) + sum(a.nbytes for a in store.deg)
        messages = sum(int(o[-1]) for o in store.edge_off)
        nodes = int(store.node_off[-1])
        if nodes * max(store.num_edge_types, 1) >= 2 ** 31 - 1 or messages >= 2 ** 31 - 1:
            return False
        return nbytes + 40 * messages + 8 * nodes * max(store.num_edge_types, 1) < budget_bytes

    def _run_epoch(self, epoch_name: str, data: Iterable[Any], data_fold: DataFold, quiet: bool = False):
        """__run_epoch, :263-311: returns (avg loss, task metric results, graphs, graphs/s, nodes/s, edges/s)."""
        batch_iterator = iter(self._batches(data, data_fold))
        tally = EpochTally(epoch_name, quiet)
        late = LateFetch(tally.fetch)
        upcoming = next(batch_iterator, None)
        while upcoming is not None:
            mb = upcoming
            batch = mb if isinstance(mb, DeviceBatch) else DeviceBatch(mb, self.device)
            if data_fold == DataFold.TRAIN:
                m = self.train_step(batch)
            else:
                with torch.no_grad():
                    m = self.forward_batch(batch, training=False)
            # (the order of readback.LateFetch: every step's metrics are fetched, one step late, after the next batch is requested)
            readback = MetricsReadback(m)          # (also drops the autograd graph: values are detached)
            upcoming = next(batch_iterator, None)
            late.put((readback, mb))
        late.flush()
        return self.task.epoch_result(tally.result(), data_fold)

    def train(self, quiet: bool = False, max_epochs: Optional[int] = None, group=None):
        """:318-371 without TensorBoard: early stopping on the task's validation metric.
        group: a torch.distributed process group of W > 1 ranks (one process per GPU, the model built after init_distributed())
        trains data-parallel by graph (data_parallel.py); None or a group of one rank is the single-GPU loop."""
        total_time_start = time.time()
        dp = data_parallel(self, group)
        train_data = self.task._loaded_data[DataFold.TRAIN]
        valid_data = self.task._loaded_data[DataFold.VALIDATION]
        # The loaded folds are millions of long-lived Python objects: frozen for the duration of the loop they cost the cyclic
        # collector nothing, and a step's own cyclic garbage (autograd graphs hold device tensors) is collected by cheap, frequent
        # full collections instead of waiting for a quarter as many survivors as there are tracked objects.
        import gc
        gc.collect()
        gc.freeze()
        try:
            if dp is not None:
                dp.begin_training()
            return self._train_loop(train_data, valid_data, total_time_start, quiet, max_epochs, dp)
        finally:
            gc.unfreeze()
            if dp is not None:
                dp.end()

    def _train_loop(self, train_data, valid_data, total_time_start, quiet, max_epochs, dp=None):
        best_valid_metric, best_epoch = float("+inf"), 0
        self.validation_history = []       # (epoch, early-stopping metric); under a group the same list on every rank
        run_epoch = self._run_epoch if dp is None else dp.run_epoch
        for epoch in range(1, (max_epochs or self.params['max_epochs']) + 1):
            if dp is not None:
                dp.epoch = epoch
            self.log_line("== Epoch %i" % epoch)
            loss, res, n, gs, ns, es = run_epoch("epoch %i (training)" % epoch, train_data, DataFold.TRAIN, quiet)
            self.log_line(" Train: loss: %.5f || %s || graphs/sec: %.2f | nodes/sec: %.0f | edges/sec: %.0f"
                          % (loss, self.task.pretty_print_epoch_task_metrics(res, n), gs, ns, es))
            loss, res, n, gs, ns, es = run_epoch("epoch %i (validation)" % epoch, valid_data, DataFold.VALIDATION, quiet)
            metric = self.task.early_stopping_metric(res, n)
            self.validation_history.append((epoch, metric))
            self.log_line(" Valid: loss: %.5f || %s || graphs/sec: %.2f | nodes/sec: %.0f | edges/sec: %.0f"
                          % (loss, self.task.pretty_print_epoch_task_metrics(res, n), gs, ns, es))
            if metric < best_valid_metric:
                if dp is None or dp.rank == 0:     # (the parameters are identical on every rank: rank 0's pickle is the model)
                    self.save_model(self.best_model_file)
                best_valid_metric, best_epoch = metric, epoch
            elif epoch - best_epoch >= self.params['patience']:
                self.log_line("Stopping training after %i epochs without improvement." % self.params['patience'])
                break
        self.best_epoch = best_epoch
        if dp is not None:
            dp.barrier()                   # nobody leaves (and reads rank 0's files) before everyone is done
        self.log_line("Training took %is." % (time.time() - total_time_start))

    # -------------------- Predictions --------------------
    def predict_iter(self, data, return_states: bool = False, nodes=None):
        """Generator over (samples of the batch, their predictions): one dict of NumPy arrays per graph, in the order of `data`
        (the task's split_predictions says which keys; return_states adds 'node_states' float32 [n, hidden], the rows of
        compute_final_node_representations).

        The forward runs under torch.no_grad() with training=False over self._batches(data, DataFold.TEST): whichever input pipeline
        the model's parameters select.  A batch's outputs are written into ONE packed device arena (the task's kernels write their
        slices in place) that leaves the device as one asynchronous copy into pinned memory, and are read one batch late, as
        _run_epoch reads metrics (readback.LateFetch): batch i is yielded once batch i + 1 is enqueued and batch i + 2 requested; two
        pinned arenas exist at most.  The fetch
        reports what a metric fetch reports: check_pending_graph_errors() and the hand-over status word (ops.HandoverError): the
        predictions of a product kernel that gave up are never handed out.

        Nothing a later training step can see is touched: no .grad, no optimizer state, no torch / NumPy random state, and
        dropout_state does not advance (nothing is dropped).  No collective: under data parallelism each rank predicts its own data.

        nodes (the citation task): int32 / int64 ids of nodes of the ONE graph in `data`, any order, repeats allowed (validated here, on
        the host, before the generator is made).  The distinct ids, ascending, are cut into batches; each batch is the receptive field
        of its ids (the fanouts and batch size of the task's "evaluation" key, or every neighbour and 1024 without it) and the
        generator yields (the batch's ids as an int32 array, [one dict whose rows are those ids']).  Everything above holds."""
        data = data if isinstance(data, list) else list(data)
        plan = None
        if nodes is not None:
            plan = self._node_prediction_plan(data, nodes)
        return self._predict_iter(data, return_states, plan)

    def _node_prediction_plan(self, data, nodes):
        distinct, inverse, given = self.task.check_prediction_nodes(data, nodes)
        settings = self.task.node_prediction_settings()
        if settings["fanouts"] is None:
            settings["fanouts"] = [0] * self.params['graph_num_layers']
        problem = self._layered_prerequisites(settings["fanouts"])
        if problem is not None:
            raise ValueError("predict(nodes=...) runs layered batches and requires %s" % problem)
        self.task.bind_sampling_device(self.device)
        return dict(settings, distinct=distinct, inverse=inverse, given=given)

    def _predict_iter(self, data, return_states, plan):
        # two pinned host arenas, taken in turn (batch i + 1's copy runs while batch i is read); kept with the model between calls
        # (pinning memory costs more than a small batch's forward) and taken out of it while this generator runs, so that a second
        # generator on the same model pins its own
        pinned, self._prediction_pinned = getattr(self, "_prediction_pinned", None) or [None, None], None
        try:
            yield from self._predict_batches(data, return_states, pinned, plan)
        finally:
            self._prediction_pinned = pinned

    def _predict_batches(self, data, return_states, pinned, plan=None):
        cursor, turn = 0, 0
        self.optimizer.flush_deferred()    # (`sparse_update`: the projection's weight holds stale rows between training steps)
        late = LateFetch(self._fetch_predictions)
        if plan is None:
            # (predict(data) stays on the full graph whatever the task's "evaluation" key says)
            batch_iterator = iter(self._batches(data, DataFold.TEST, full_graph=True))
        else:
            batch_iterator = iter(self.task.node_prediction_batches(data, plan["distinct"], plan["fanouts"], plan["seeds_per_batch"],
                                                                    self._full_graph_route(self._native_batching())))
        upcoming = next(batch_iterator, None)
        while upcoming is not None:
            with torch.no_grad():      # (around the device work only: a generator suspended inside it would leave the grad mode of
                #                         the CONSUMER's code switched off between two batches)
                batch = upcoming if isinstance(upcoming, DeviceBatch) else DeviceBatch(upcoming, self.device)
                if plan is None:
                    samples = data[cursor:cursor + batch.num_graphs]
                    cursor += batch.num_graphs
                else:
                    samples = None     # (one graph; the batch names its rows itself: extra['prediction_seeds'])
                final = self._final_node_states(batch, training=False)
                layout = dict(self.task.prediction_layout(batch, final.shape[1]))
                if return_states:
                    layout["node_states"] = (tuple(final.shape), torch.float32)
                arena = _PredictionArena(layout, final.device, pinned, turn)
                turn ^= 1
                outputs = self.task.compute_task_predictions(final, batch, self.variables.scope(self._task_scope), out=arena.views)
                if return_states:
                    outputs = dict(outputs, node_states=final)
                arena.send(outputs)
            upcoming = next(batch_iterator, None)          # (the order of readback.LateFetch: requested before the previous batch is read)
            fetched = late.put((arena, batch, samples))
            if fetched is not None:
                yield fetched
        fetched = late.flush()
        if fetched is not None:
            yield fetched

    def _fetch_predictions(self, pending):
        arena, batch, samples = pending
        host = arena.fetch()
        check_pending_graph_errors()
        if samples is None:                # predict(nodes=...): the rows are the batch's seeds
            return batch.extra['prediction_seeds'], [host]
        return samples, self.task.split_predictions(host, batch, samples)

    def predict(self, data, return_states: bool = False, quiet: bool = True, nodes=None):
        """One entry per graph of `data`, in its order (predict_iter, collected).  nodes (predict_iter): ONE dict instead, `nodes` as
        given (int64) and one row per entry of it under every other key; a node named twice has two equal rows."""
        if nodes is not None:
            data = data if isinstance(data, list) else list(data)
            plan = self._node_prediction_plan(data, nodes)
            parts = [rows for _, (rows,) in self._predict_iter(data, return_states, plan)]
            out = {"nodes": plan["given"]}
            for key in parts[0]:
                out[key] = np.concatenate([part[key] for part in parts])[plan["inverse"]]
            return out
        results = []
        for step, (samples, predictions) in enumerate(self.predict_iter(data, return_states)):
            results.extend(predictions)
            if not quiet:
                print("Predicting, batch %i (has %i graphs). %i graphs so far." % (step, len(samples), len(results)), end='\r')
        return results

    def test(self, data, quiet: bool = False, group=None):
        """Loss and task metrics of `data`.  group: as in train(); every rank passes the SAME data, evaluates its shard of it, and
        rank 0 logs the metrics of the whole."""
        dp = data_parallel(self, group)
        if dp is None:
            loss, res, n, gs, ns, es = self._run_epoch("Test", list(data), DataFold.TEST, quiet)
        else:
            try:
                loss, res, n, gs, ns, es = dp.run_epoch("Test", list(data), DataFold.TEST, quiet)
            finally:
                dp.end()
        self.log_line("Loss %.5f on %i graphs" % (loss, n))
        self.log_line("Metrics: %s" % self.task.pretty_print_epoch_task_metrics(res, n))
