"""ctypes binding of librelgnn.so (C ABI: the headers include/relgnn*.h, one table of `ABI` each).

This is the ONLY compute backend of the package.  There is no CPU / eager-PyTorch fallback:
if the HIP library is missing, or a tensor is not a float32/int32 CUDA(HIP) tensor, the
call fails loudly.  (The NumPy oracle under oracle/ is test infrastructure and is never
imported from here.)
"""
import ctypes
from pathlib import Path

import torch  # imported first on purpose: makes torch's libamdhip64.so.7 the process-wide HIP runtime

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = _PKG_DIR / "librelgnn.so"

OK, EINVAL, ENOSPC, EHIP, EUNSUPPORTED = 0, 1, 2, 3, 4
ERRFLAG_INDEX_OUT_OF_RANGE = 1
ERRFLAG_NOT_SORTED = 2

AGG_SUM, AGG_MEAN, AGG_SQRT_N, AGG_MAX = 0, 1, 2, 3
MT_MAX = 48
ACT_LINEAR, ACT_TANH, ACT_RELU, ACT_LEAKY_RELU, ACT_ELU, ACT_SELU, ACT_GELU = range(7)

_c_i32, _c_i64, _c_f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
_c_u32 = ctypes.c_uint32
_ptr = ctypes.c_void_p

# header file name -> {name: (restype, argtypes)}: one table per header of include/, each listing every function its header declares
# (tests/test_abi.py holds every table to its header, to the library's exports and to what load_library() sets)
ABI = {}

# include/relgnn.h (the kernels behind the layer functions, the heads, the optimizers and the batch builder)
ABI["relgnn.h"] = {
    "relgnn_abi_version": (ctypes.c_int, []),
    "relgnn_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "relgnn_relational_keys": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _c_i32, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_relational_keys2": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _c_i32, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_relational_keys_all": (ctypes.c_int, [_ptr, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_relational_plan_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "relgnn_relational_plan": (ctypes.c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_segment_plan_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "relgnn_segment_plan": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_gather_i32": (ctypes.c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_gather_div_i32": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr]),
    "relgnn_gather_f32": (ctypes.c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_invert_perm": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr]),
    "relgnn_degree_scale": (ctypes.c_int, [_ptr, _ptr, _c_i32, _c_i32, _c_f32, _ptr, _ptr]),
    "relgnn_segment_counts_scale": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr]),
    "relgnn_seg_reduce_fwd": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr]),
    "relgnn_seg_reduce_acc64_fwd": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr]),
    "relgnn_seg_reduce_fwd_rowmax": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_seg_reduce_msgact_fwd": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_msg_act_bwd": (ctypes.c_int, [_c_i32, _ptr, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_seg_max_count": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_seg_max_bwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_act_bwd_from_output": (ctypes.c_int, [_c_i32, _ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_film_fwd": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_film_bwd_film": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_film_bwd_msg_masked": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_film_bwd_msg": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_rgat_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i32, _c_i32, _ptr, _c_f32, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_rgat_bwd_logits": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i32, _c_i32, _ptr, _c_f32, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_rgat_bwd_msg": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_rgat_alpha": (ctypes.c_int, [_ptr, _ptr, _c_i32, _ptr, _c_i32, _c_i32, _ptr, _c_f32, _ptr, _ptr]),
    "relgnn_headw_reduce": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _c_i32, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_rgat_dz": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i32, _c_i32, _ptr, _c_f32, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_pair_fwd": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_pair_bwd_q": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_pair_bwd_p": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_column_sum_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "relgnn_column_sum": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i64, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_mt_l2norm_workspace_bytes": (ctypes.c_size_t, []),
    "relgnn_mt_l2norm": (ctypes.c_int, [_ptr, _ptr, _c_i32, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_mt_adam_clip": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr]),
    "relgnn_adam_step_size": (ctypes.c_int, [_ptr, _c_f32, _c_f32, _c_f32, _ptr]),
    "relgnn_mt_adam_clip_devlr": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_f32, _ptr, _c_f32, _c_f32, _c_f32, _ptr]),
    "relgnn_mt_rmsprop_clip": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr]),
    "relgnn_mt_sgd_clip": (ctypes.c_int, [_ptr, _ptr, _ptr, _c_i32, _ptr, _c_f32, _c_f32, _ptr]),
    "relgnn_sigmoid_ce_stats_workspace_bytes": (ctypes.c_size_t, []),
    "relgnn_sigmoid_ce_stats": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_f32, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_sigmoid_ce_bwd": (ctypes.c_int, [_ptr, _ptr, _c_i64, _ptr, _c_f32, _ptr, _ptr, _ptr]),
    "relgnn_sigmoid_ce_bwd_padded": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _c_f32, _ptr, _ptr, _c_i32, _ptr]),
    "relgnn_softmax_ce_stats_workspace_bytes": (ctypes.c_size_t, []),
    "relgnn_softmax_ce_stats": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_softmax_ce_bwd": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_charcnn_supported": (ctypes.c_int, [_c_i32, _c_i32]),
    "relgnn_charcnn_range_labels": (_c_i64, [_c_i32]),
    "relgnn_charcnn_fwd_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "relgnn_charcnn_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr, ctypes.c_size_t,
                                          _ptr, _ptr]),
    "relgnn_charcnn_bwd_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "relgnn_charcnn_bwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                          ctypes.c_size_t, _ptr]),
    "relgnn_varmisuse_head_supported": (ctypes.c_int, [_c_i32, _c_i32]),
    "relgnn_varmisuse_head_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "relgnn_varmisuse_head_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr,
                                                 ctypes.c_size_t, _ptr, _ptr]),
    "relgnn_varmisuse_head_bwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr,
                                                 _c_i64, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_qm9_head_supported": (ctypes.c_int, [_c_i32, _c_i32, _c_i32]),
    "relgnn_qm9_head_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32, _c_i32]),
    "relgnn_qm9_head_fwd": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr,
                                           _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_qm9_head_bwd": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr,
                                           _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, ctypes.c_size_t,
                                           _ptr]),
    "relgnn_gru_gates_fwd": (ctypes.c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_gru_cell_fwd_supported": (ctypes.c_int, [_c_i32, _c_i32, _c_i32]),
    "relgnn_gru_cell_fwd_xf32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                                _c_i64, _c_i32, _c_i32, _ptr, _ptr]),
    "relgnn_gru_cell_bwd_xf32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr, _ptr, _c_i64,
                                                _c_i32, _c_i32, _ptr, _ptr]),
    "relgnn_gru_out_fwd": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr]),
    "relgnn_gru_out_bwd": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_gru_gates_bwd": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr]),
    "relgnn_pair_materialize": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_rgat_scores_groups": (_c_i64, [_c_i64]),
    "relgnn_rgat_scores_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _c_i32, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_rgat_scores_bwd": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _c_i32, _c_i64, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_layer_norm_groups": (_c_i64, [_c_i64, _c_i32]),
    "relgnn_layer_norm_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _c_f32, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_layer_norm_bwd": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_panel_gemm_zeros_floats": (ctypes.c_int, []),
    "relgnn_panel_gemm_f32": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr, _c_i32, _c_i64, _ptr, _ptr, _ptr,
                                             _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i64, _c_i64, _c_i64, _c_i32, _ptr]),
    "relgnn_limb_elements": (_c_i64, [_c_i64, _c_i64]),
    "relgnn_limb_split_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _c_i32, _ptr, _ptr]),
    "relgnn_limb_gemm_f32": (ctypes.c_int, [_c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_limb_gemm_xf32": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_limb_gemm_xf32_dact": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _c_i32,
                                                  _c_i32, _ptr]),
    "relgnn_limb16_gemm_xf32_dact": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr,
                                                    _c_i64, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_rgcn_fused_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr,
                                             _c_i64, _c_i32, _c_i32, _ptr, _ptr]),
    "relgnn_limb_gemm_xf32_pc": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _ptr, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _c_i32, _c_i32,
                                                _ptr, _ptr]),
    "relgnn_limb_gemm_xf32_pc_supported": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32]),
    "relgnn_limb_gemm_tn_chunks": (_c_i64, [_c_i32, _c_i32, _c_i32]),
    "relgnn_limb_gemm_tn_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_limb_gemm_tn_tiles_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i32, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_limb16_gemm_tn_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i32, _ptr, _c_i32, _ptr, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_col_absmax_workspace_bytes": (ctypes.c_int64, [_c_i32, _c_i32]),
    "relgnn_col_absmax_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _c_i32, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_absmax_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr]),
    "relgnn_limb16_elements": (_c_i64, [_c_i64, _c_i64]),
    "relgnn_limb16_split_multi_f32": (ctypes.c_int, [_c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr]),
    "relgnn_limb16_gemm_xf32": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i32,
                                               _c_i32, _ptr]),
    "relgnn_limb_split_multi_f32": (ctypes.c_int, [_c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_limb_split_batch_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _ptr, _ptr]),
    "relgnn_limb_dense_sel_f32": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _c_i32, _ptr, _ptr,
                                                 _ptr, _c_i64, _ptr, _c_i64, _c_i32, _c_i32, _c_i32, _ptr]),
    "relgnn_limb_gemm_sel_xf32": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _ptr, _c_i32, _ptr, _c_i32, _ptr, _ptr, _ptr, _c_i64, _c_i32,
                                                 _c_i32, _c_i32, _ptr]),
    "relgnn_limb_gemm_sel_pc_supported": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32]),
    "relgnn_limb_gemm_sel_pc_xf32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i32, _ptr, _c_i32, _ptr, _ptr, _c_i64, _c_i32, _c_i32,
                                                    _c_i32, _ptr, _ptr]),
    "relgnn_edge_mlp_fwd_supported": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32]),
    "relgnn_edge_mlp_fwd_xf32": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _c_i32, _ptr, _c_i32, _ptr,
                                                _c_i64, _c_i64, _c_i32, _c_i32, _ptr]),
    "relgnn_fill_rows_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _c_i64, ctypes.c_float, _ptr]),
    "relgnn_limb_dense_f32": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _c_i32,
                                             _c_i32, _c_i32, _ptr]),
    "relgnn_blaslt_gemm_f32": (ctypes.c_int, [_c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32,
                                              _c_i64, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _ptr]),
    "relgnn_gemm_tn_stream_workspace_bytes": (_c_i64, [_c_i32, _c_i32, _c_i64]),
    "relgnn_gemm_tn_stream_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _c_i32, _c_i64, _c_i32, _ptr, _c_i64, _ptr]),
    "relgnn_gemm_tn_stream_group_workspace_bytes": (_c_i64, [_c_i32, _ptr, _ptr, _c_i64, _c_i32]),
    "relgnn_gemm_tn_stream_group_f32": (ctypes.c_int, [_c_i32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64,
                                                       _ptr]),
    "relgnn_gemm_tn_stream_blocks_f32": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_i64,
                                                        _c_i32, _ptr, _c_i64, _ptr]),
    "relgnn_sum_slabs_tail_f32": (ctypes.c_int, [_ptr, _c_i32, _c_i32, _c_i32, _ptr, _c_i64, _ptr, _c_i64, _c_i32, _ptr, _ptr]),
    "relgnn_rgdcn_apply_fwd": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _ptr, _ptr, _ptr]),
    "relgnn_rgdcn_apply_bwd": (ctypes.c_int, [_c_i32, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_batch_gather": (ctypes.c_int, [_ptr, _c_i32, _c_i32, _c_i64] + [_ptr] * 6 + [_c_i64, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _ptr,
                                           _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_plan_assemble": (ctypes.c_int, [_ptr, _c_i32, _c_i32, _c_i64] + [_ptr] * 8 + [_c_i64, _c_i64] + [_ptr] * 16 + [_ptr] * 5 + [_ptr]),
    # host-side batch builder (section 9): host pointers only
    "relgnn_batch_layout_len": (_c_i64, [_c_i32, _c_i32]),
    "relgnn_batch_count": (_c_i64, [_ptr, _ptr, _c_i64, _c_i64, _c_i64]),
    "relgnn_batch_layout": (ctypes.c_int, [_c_i32, _c_i64, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr]),
    "relgnn_batch_pack": (ctypes.c_int, [_c_i32, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i32, _ptr, _ptr, _ptr, _ptr, ctypes.c_size_t, _c_i32]),
}

# include/relgnn_dropout.h (the opt-in layer-input dropout route)
ABI["relgnn_dropout.h"] = {
    "relgnn_dropout_fwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _c_i32, _c_u32, _c_f32, _ptr, _ptr]),
    "relgnn_dropout_bwd": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _c_i32, _c_u32, _c_f32, _ptr, _ptr]),
    "relgnn_dropout_residual_fwd": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _c_i32, _c_u32, _c_f32, _ptr, _ptr, _ptr]),
    "relgnn_dropout_residual_bwd": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _c_i32, _c_u32, _c_f32, _ptr, _ptr, _ptr]),
}

# include/relgnn_predict.h (probabilities and labels out of the heads' logits)
ABI["relgnn_predict.h"] = {
    "relgnn_predict_sigmoid_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_predict_softmax_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_predict_candidates_f32": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr]),
}

# include/relgnn_parallel.h (data-parallel training: the scaled pack in front of the gradient all-reduce)
ABI["relgnn_parallel.h"] = {
    "relgnn_mt_pack_scaled_f32": (ctypes.c_int, [_ptr, _ptr, _c_i32, _c_f32, _ptr, _ptr]),
}

# include/relgnn_sparse_features.h (CSR rows times a row table: the citation task's sparse node features)
ABI["relgnn_sparse_features.h"] = {
    "relgnn_csr_project_supported": (ctypes.c_int, [_c_i32]),
    "relgnn_csr_project_split_above": (_c_i64, []),
    "relgnn_csr_project_slab": (_c_i64, []),
    "relgnn_csr_project_f32": (ctypes.c_int, [_c_i32, _ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr, _c_i64, _c_i64, _ptr, _c_i64, _c_i32, _ptr,
                                              _c_i64, _ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
}

# include/relgnn_sampling.h (neighbour sampling from the by-target bucketing: the citation task's sampled batches)
ABI["relgnn_sampling.h"] = {
    "relgnn_neighbour_sample_supported": (ctypes.c_int, [_ptr, _c_i32, _c_i64, _c_i32]),
    "relgnn_neighbour_sample_max_fanout": (_c_i64, []),
    "relgnn_neighbour_sample_max_hops": (_c_i64, []),
    "relgnn_neighbour_sample_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "relgnn_neighbour_sample_begin": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_neighbour_sample_count": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _ptr, _ptr,
                                                     ctypes.c_size_t, _ptr]),
    "relgnn_neighbour_sample_take": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i64, _c_i32, _c_i32, _c_u32, _c_u32, _c_u32,
                                                    _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_neighbour_sample_compact": (ctypes.c_int, [_ptr, _c_i64, _c_i32, _ptr, _c_i64, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_neighbour_sample_relabel": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_neighbour_sample_degrees": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _ptr, _ptr, _c_i64, _ptr, _ptr]),
    "relgnn_neighbour_sample_finish": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr]),
}

# include/relgnn_layered_sampling.h (the hop-ordered numbering of a sampled subgraph: the citation task's layered batches)
ABI["relgnn_layered_sampling.h"] = {
    "relgnn_neighbour_sample_relabel_by_hop": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _c_i64, _ptr, _ptr, _c_i32, _ptr, _ptr]),
    "relgnn_neighbour_sample_degrees_by_hop": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _c_i32, _c_i64, _c_i64, _ptr, _ptr]),
}

# include/relgnn_sparse_subset.h (a row subset of sparse node features and its transpose, built on the device: sampled batches over
# sparse features)
ABI["relgnn_sparse_subset.h"] = {
    "relgnn_sparse_subset_supported": (ctypes.c_int, [_c_i64, _c_i64, _c_i64]),
    "relgnn_split_plan_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "relgnn_split_plan_count": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_split_plan_fill": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_sparse_subset_count_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "relgnn_sparse_subset_count": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                                  ctypes.c_size_t, _ptr]),
    "relgnn_sparse_subset_copy": (ctypes.c_int, [_ptr, _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    "relgnn_sparse_subset_transpose_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "relgnn_sparse_subset_transpose": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr, ctypes.c_size_t, _ptr]),
}

# include/relgnn_sparse_update.h (row-deferred Adam for a row table whose gradient is +0 outside the rows a batch names)
ABI["relgnn_sparse_update.h"] = {
    "relgnn_rows_adam_supported": (ctypes.c_int, [_c_i32]),
    "relgnn_rows_adam_catch_up": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32, _c_i32, _c_f32, _c_f32,
                                                 _c_f32, _ptr]),
    "relgnn_rows_adam_step": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32, _c_i32, _ptr,
                                             _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr]),
}

# include/relgnn_sparse_gradient.h (the compact gradient of that row table: named rows, the dense norm's bits over them, the row step
# on compact rows)
ABI["relgnn_sparse_gradient.h"] = {
    "relgnn_named_rows_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "relgnn_named_rows_count": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_named_rows_fill": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64, _ptr]),
    "relgnn_rows_l2norm_workspace_bytes": (ctypes.c_size_t, []),
    "relgnn_rows_l2norm": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_rows_adam_step_compact": (ctypes.c_int, [_ptr, _c_i64, _c_i64, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i32,
                                                     _c_i32, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr]),
}

# include/relgnn_subgraph.h (random-walk node sets and their induced subgraphs: the citation task's subgraph batches)
ABI["relgnn_subgraph.h"] = {
    "relgnn_subgraph_supported": (ctypes.c_int, [_c_i64, _c_i32, _c_i64, _c_i32]),
    "relgnn_subgraph_max_walk_length": (_c_i64, []),
    "relgnn_subgraph_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "relgnn_subgraph_walk": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _c_i64, _c_i32, _c_u32, _c_u32, _c_u32, _ptr, _ptr]),
    "relgnn_subgraph_number": (ctypes.c_int, [_ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
    "relgnn_subgraph_induced_count": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr,
                                                     ctypes.c_size_t, _ptr]),
    "relgnn_subgraph_induced_emit": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _ptr, _c_i64, _c_i64, _ptr, _ptr, _c_i64, _ptr, _ptr,
                                                    _ptr]),
    "relgnn_subgraph_clear": (ctypes.c_int, [_ptr, _c_i64, _ptr, _c_i64, _ptr]),
}

# include/relgnn_subgraph_norm.h (GraphSAINT normalisation of the subgraph batches: visit counts, per-edge weights, the weighted loss
# head)
ABI["relgnn_subgraph_norm.h"] = {
    "relgnn_subgraph_visit_count": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_subgraph_induced_emit_weighted": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr,
                                                             _ptr, _c_f32, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    "relgnn_softmax_ce_weighted_stats_workspace_bytes": (ctypes.c_size_t, []),
    "relgnn_softmax_ce_weighted_stats": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, _c_f32, _c_i64, _c_i32, _ptr, _ptr,
                                                        ctypes.c_size_t, _ptr]),
    "relgnn_softmax_ce_weighted_bwd": (ctypes.c_int, [_ptr, _c_i64, _ptr, _ptr, _ptr, _c_f32, _c_i64, _c_i32, _ptr, _ptr, _ptr, _c_i64,
                                                      _ptr]),
}

# csrc/<header> -> {name: (restype, argtypes)}: the package-internal entry points, declared beside the kernels and NOT under include/.
# load_library() types them too; signatures() neither returns nor merges them: they are not public ABI and may change with the package.
INTERNAL = {}

# csrc/graph_partition.h (the wish pass of the device graph partitioner: tasks/graph_partition.py)
INTERNAL["graph_partition.h"] = {
    "relgnn_partition_supported": (ctypes.c_int, [_c_i64, _c_i32, _c_i64, _c_i32, _c_i32]),
    "relgnn_partition_wave_row_max": (_c_i64, []),
    "relgnn_partition_wish": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _ptr, _c_i32, _ptr, _c_i32, _c_u32, _c_u32, _ptr, _ptr,
                                             _c_i64, _c_i32, _ptr, _ptr]),
}

# csrc/level_plan.h (the level bucketings of a hop-ordered sampled batch derived from its union graph's: tasks/neighbour_sampling.py)
INTERNAL["level_plan.h"] = {
    "relgnn_level_plan_max_levels": (_c_i32, []),
    "relgnn_level_plan_desc_stride": (_c_i64, [_c_i32]),
    "relgnn_level_plan_tile": (_c_i64, []),
    "relgnn_level_plan_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "relgnn_level_plan": (ctypes.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i32, _c_i64, _ptr, _c_i32, _c_i64,
                                         _c_i64, _ptr, _c_i64, _ptr, ctypes.c_size_t, _ptr]),
}

# csrc/window_block.h (the block of a window of target rows, cut from the full graph's by-target bucketing: tasks/layerwise.py)
INTERNAL["window_block.h"] = {
    "relgnn_window_block_supported": (ctypes.c_int, [_c_i64, _c_i32]),
    "relgnn_window_block_tile": (_c_i64, []),
    "relgnn_window_block_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "relgnn_window_block_count": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr,
                                                 _ptr, ctypes.c_size_t, _ptr]),
    "relgnn_window_block_emit": (ctypes.c_int, [_ptr, _ptr, _c_i64, _c_i32, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _c_i64,
                                                _ptr, _ptr, _c_i64, _ptr, _c_i64, _ptr, _c_i64, _ptr]),
}

_lib = None


class RelGnnLibraryError(RuntimeError):
    pass


def load_library():
    """dlopen librelgnn.so and type every entry point.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RelGnnLibraryError(
            "%s not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (needs hipcc). There is no CPU fallback for this path." % LIB_PATH)
    lib = ctypes.CDLL(str(LIB_PATH))
    typed = signatures()
    for header, table in INTERNAL.items():
        for name in table:
            if name in typed:
                raise RelGnnLibraryError("%s of csrc/%s is bound twice" % (name, header))
        typed.update(table)
    for name, (restype, argtypes) in typed.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.relgnn_abi_version() != 1:
        raise RelGnnLibraryError("librelgnn.so ABI version mismatch")
    _lib = lib
    return lib


def signatures(header=None):
    """A copy of one header's table (`header` is its file name, a key of ABI), or with None the union of all of them: every entry
    point load_library() types.  Raises if two headers bind one name, where the later table would silently win."""
    if header is not None:
        return dict(ABI[header])
    union, owner = {}, {}
    for h, table in ABI.items():
        for name in table:
            if name in owner:
                raise RelGnnLibraryError("%s is bound by both %s and %s" % (name, owner[name], h))
            owner[name] = h
        union.update(table)
    return union


def status_string(code: int) -> str:
    return load_library().relgnn_status_string(code).decode()


def check(code: int, what: str):
    if code == OK:
        return
    msg = "%s failed: %s (status %d)" % (what, status_string(code), code)
    if code in (EINVAL, EUNSUPPORTED):
        raise ValueError(msg)
    raise RuntimeError(msg)


def ptr(t, rows_strided: bool = False):
    """Device pointer of a tensor (None -> NULL).  Refuses anything but HIP device memory.
    rows_strided=True accepts a 2-D tensor whose rows are dense (stride(1) == 1) but whose row
    stride exceeds its width (the C ABI takes the leading dimension separately)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RelGnnLibraryError(
            "librelgnn kernels only run on MI355X device tensors; got a %s tensor. "
            "There is no CPU fallback for this path." % t.device)
    if not t.is_contiguous():
        if not (rows_strided and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
            raise ValueError("librelgnn expects contiguous tensors")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream():
    """hipStream_t of torch's current stream on the current device (an int for ctypes).  The raw accessor avoids
    building a torch.cuda.Stream object per kernel launch (~10 us each, several launches per layer)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def launch(name: str, *args) -> None:
    """librelgnn's `name`(*args, the current stream); raises on a status other than OK."""
    check(getattr(load_library(), name)(*args, current_stream()), name)


def scratch(nbytes: int, device) -> torch.Tensor:
    """Workspace of at least `nbytes` bytes for one launch (the kernels take a pointer and a byte count; the caching allocator's
    alignment exceeds every element type they keep there).  A plain torch.empty: on the current stream, capturable."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
