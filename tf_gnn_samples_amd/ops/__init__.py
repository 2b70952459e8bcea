"""torch.autograd wrappers over the librelgnn C ABI (include/relgnn.h), one module per kernel family.  This file only re-exports:
callers outside the package say ops.<name>."""
from ..activations import FUSABLE_ACTS as _FUSABLE_ACTS, activation_id  # noqa: F401
from ..graph import LONG_SEGMENT, SplitPlan  # noqa: F401
from ..handover import HandoverError, handover_status, handover_word, handover_word_if_any, raise_on_handover, report_handover  # noqa: F401
from ..weight_grad_stream import (deferred_targets_ok, deferred_weight_gradient_join, fork, hand_over_deferred, join_deferred,  # noqa: F401
                                  wait_if_in_flight)
from .dropout import dropout, dropout_residual, dropout_state, dropout_tensor_ok, dropout_threshold, fused_dropout_on  # noqa: F401
from .edge import (_BlockedLinear, _fill_rows, _FusedEdgeMessages, _PairMaterialize, blocked_linear, edge_mlp_first_product,  # noqa: F401
                   film_messages_reduce, pair_materialize, pair_messages_reduce_fused)
from .rgat import rgat_attention, rgat_layer_attention, rgat_scores_supported  # noqa: F401
from .rgcn import _AggregateThenTransform, _rgcn_fused, _weight_gradient, aggregate_acc64, aggregate_then_transform  # noqa: F401
from .rgdcn import rgdcn_apply, rgdcn_apply_supported  # noqa: F401
from .segment import (ROUTES, SegmentPlanCache, _csr_project_raw, _seg_reduce_raw, acc64_supported, aggregation_mode_id,  # noqa: F401
                      csr_project_supported, csr_rows_project, message_act_reduce, rowmax_supported, seg_gather_reduce,
                      unsorted_segment_max, unsorted_segment_mean, unsorted_segment_sqrt_n, unsorted_segment_sum)
from .typed import _typed_panel_ok, _TypedLinearPanel, typed_linear, typed_linear_pair  # noqa: F401
