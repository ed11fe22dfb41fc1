"""ctypes binding of ``libgnc_hip.so`` (C ABI: ``include/gnc_hip.h``).

PyTorch is used for device memory and streams only: every call below passes raw
``data_ptr()`` values and the current HIP stream to the library.  There is NO
fallback: if the shared library is missing or a call fails, a ``RuntimeError``
is raised -- the product path never silently routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes
import math
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

import torch

LIB_NAME = "libgnc_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

GNC_MAX_SEGMENTS = 4
GNC_MAX_LINEAR = 8
ABI_VERSION = 20
GRAD_NORM_BLOCKS = 256                      # workgroups of the gradient-norm pass: a constant, so the sum's order depends on n alone
GRAD_NORM_PASS = GRAD_NORM_BLOCKS * 256 * 4  # elements one grid pass of it covers (float4 per thread)
OPT_SCALARS = 8                             # float32 scalars of a controlled step: step_size, bc2_sqrt, decay, clip_coef, lr, grad_norm
OPT_RULES = {"adam": 0, "adamw": 1, "sgd": 2}
LR_SCHEDULES = {"constant": 0, "cosine": 1, "step": 2}
LOSS_KINDS = {"ce": 0, "bce": 1}            # GNC_LOSS_CE / GNC_LOSS_BCE
LOSS_REDUCTIONS = {"mean": 0, "sum": 1}     # GNC_LOSS_MEAN / GNC_LOSS_SUM
CLASS_LOSS_ONE_LAUNCH_ROWS = 64             # GNC_CLASS_LOSS_ONE_LAUNCH_ROWS: up to here the loss head is ONE kernel launch
CLASS_LOSS_WORKSPACE_DOUBLES = 2 * 256 + 1  # GNC_CLASS_LOSS_WORKSPACE_DOUBLES: the larger batches' partials and the gradient's factor

ACTIVATIONS = {  # nn.<Name> accepted by the reference's MLP(activation=...) (models/MLP.py:21)
    "ReLU": 0, "Identity": 1, "Tanh": 2, "Sigmoid": 3, "SiLU": 4, "GELU": 5, "LeakyReLU": 6, "ELU": 7,
}

# every symbol include/gnc_hip.h declares: (restype, argtypes)
_SIGNATURES = {
    "gnc_abi_version": (c_int32, []),
    "gnc_last_error_string": (c_char_p, []),
    "gnc_target_arch": (c_char_p, []),
    "gnc_mlp_agg_supported": (c_int32, [c_void_p]),
    "gnc_mlp_agg_only_supported": (c_int32, [c_void_p]),
    "gnc_mlp_forward_agg_only_f32": (c_int32, [c_void_p, c_void_p]),
    "gnc_mlp_edge_features_supported": (c_int32, [c_void_p]),
    "gnc_mlp_operands_in_place_supported": (c_int32, [c_void_p]),
    "gnc_mlp_save_act_supported": (c_int32, [c_void_p]),
    "gnc_mlp_agg_fix_len": (c_int32, []),
    "gnc_mlp_small_batch_supported": (c_int32, [c_void_p]),
    "gnc_mlp_small_batch_max_rows": (c_int64, []),
    "gnc_mlp_projection_t2_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                            c_int64, c_void_p]),
    "gnc_mlp_dual_projection_f32": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32,
                                              c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_mlp_backward_small_batch_supported": (c_int32, [c_void_p]),
    "gnc_readout_forward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32,
                                          c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnc_readout_backward_f32": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_void_p,
                                           c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "gnc_readout_batched_supported": (c_int32, [c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "gnc_readout_batched_forward_f32": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_void_p, c_int64, c_void_p,
                                                  c_int32, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_readout_batched_backward_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_void_p, c_int64,
                                                   c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_pad_graph_batch_supported": (c_int32, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int32, c_int32]),
    "gnc_pad_graph_batch": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnc_xty_small_max_rows": (c_int32, []),
    "gnc_xty_small_f32": (c_int32, [c_void_p, c_int32, c_void_p]),
    "gnc_agg_fixup_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int64,
                                    c_void_p]),
    "gnc_csr_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gnc_csr_build": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gnc_topology_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32]),
    "gnc_topology_build": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_int32, c_void_p]),
    "gnc_permute_index_i64_i32": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_permute_index_checked_i64_i32": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnc_scatter_sum_csr_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p,
                                          c_int64, c_void_p]),
    "gnc_gather_rows_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p]),
    "gnc_gather_rows_add_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64,
                                          c_void_p]),
    "gnc_poison_if_flagged_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    "gnc_edge_features_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "gnc_sizeof_mlp_desc": (c_size_t, []),
    "gnc_mlp_supported": (c_int32, [c_void_p]),
    "gnc_mlp_forward_f32": (c_int32, [c_void_p, c_void_p]),
    "gnc_sizeof_mlp_bwd_desc": (c_size_t, []),
    "gnc_mlp_backward_supported": (c_int32, [c_void_p]),
    "gnc_mlp_backward_dx_add_honoured": (c_int32, [c_void_p]),
    "gnc_mlp_backward_grad_gather_honoured": (c_int32, [c_void_p]),
    "gnc_mlp_backward_saved_act_honoured": (c_int32, [c_void_p]),
    "gnc_mlp_backward_ln_partial_rows": (c_int32, [c_void_p]),
    "gnc_mlp_backward_fused_rows": (c_int32, [c_void_p]),
    "gnc_mlp_backward_f32": (c_int32, [c_void_p, c_void_p]),
    "gnc_xty_partials": (c_int32, [c_int64]),
    "gnc_xty_partials_for": (c_int32, [c_int64, c_int32, c_int32]),
    "gnc_xty_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "gnc_grid_num_edges": (c_int64, [c_int32, c_int32, c_int32]),
    "gnc_grid_edges_i64": (c_int32, [c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "gnc_pixel_nodes_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "gnc_patch_nodes_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "gnc_rag_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "gnc_rag_build": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "gnc_rag_batched_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gnc_rag_build_batched": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gnc_region_descriptors_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "gnc_region_descriptors_rgb_u8": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    "gnc_slic_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "gnc_slic_rgb_u8": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_int32, c_int32, c_double, c_double,
                                  c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gnc_resize_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gnc_resize_rgb_u8": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "gnc_crop_resize_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gnc_crop_resize_rgb_u8": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
    "gnc_color_jitter_resident_pixels": (c_int64, []),
    "gnc_color_jitter_rgb_u8": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "gnc_u8_hwc_to_f32_chw": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "gnc_wide_linear_supported": (c_int32, [c_void_p, c_void_p]),
    "gnc_wide_linear_workspace_floats": (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    "gnc_wide_linear_forward_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_float,
                                              c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "gnc_wide_linear_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32,
                                               c_float, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_colsum_pair_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int32, c_void_p]),
    "gnc_reduce_partials_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_activation_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_float, c_void_p, c_int64, c_void_p]),
    "gnc_activation_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_float, c_void_p, c_int64,
                                              c_void_p]),
    "gnc_layer_norm_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_float, c_void_p, c_int64,
                                              c_void_p, c_int64, c_void_p]),
    "gnc_bn_partials": (c_int32, [c_int64, c_int32]),
    "gnc_bn_stats_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int32, c_void_p]),
    "gnc_bn_finalize_f32": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "gnc_bn_apply_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32,
                                   c_void_p, c_int64, c_void_p]),
    "gnc_bn_backward_sums_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32,
                                           c_void_p]),
    "gnc_bn_backward_dz_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_int32, c_void_p, c_int64, c_void_p]),
    "gnc_bn_small_max_rows": (c_int32, []),
    "gnc_bn_forward_small_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_float, c_float,
                                           c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnc_bn_backward_small_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                            c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnc_bn_fold_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32,
                                  c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_graph_pool_plan": (c_int32, [c_int64, c_int64, c_int64, c_void_p]),
    "gnc_graph_pool_forward_f32": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int64, c_void_p, c_int64, c_void_p]),
    "gnc_graph_pool_backward_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                              c_void_p]),
    "gnc_graph_attention_pool_workspace_floats": (c_int64, [c_int64, c_int64, c_int64]),
    "gnc_graph_attention_pool_forward_f32": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                                       c_void_p, c_int64, c_void_p]),
    "gnc_graph_attention_pool_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                        c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnc_graph_attention_weights_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "gnc_topk_pool_select_f32": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnc_topk_pool_edge_workspace_ints": (c_int64, [c_int64]),
    "gnc_topk_pool_filter_edges": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_topk_pool_select_padded_f32": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p]),
    "gnc_topk_pool_filter_edges_padded": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_topk_pool_rows_forward_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnc_topk_pool_rows_backward_f32": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                                  c_int64, c_void_p, c_void_p]),
    "gnc_segment_reduce_csr_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64,
                                             c_void_p, c_void_p]),
    "gnc_segment_reduce_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32,
                                                  c_void_p, c_int64, c_void_p]),
    "gnc_rows_div_degree_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    "gnc_segment_softmax_csr_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64,
                                              c_void_p, c_void_p]),
    "gnc_segment_softmax_backward_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                   c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_segment_softmax_weights_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_adam_step_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                    c_void_p, c_void_p, c_void_p]),
    "gnc_adam_step_hp64_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_float, c_float,
                                         c_void_p, c_void_p, c_void_p]),
    "gnc_sizeof_opt_ctl": (c_int32, []),
    "gnc_grad_norm_pass": (c_int64, []),
    "gnc_grad_norm_blocks": (c_int32, []),
    "gnc_grad_sumsq_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p]),
    "gnc_optimizer_ctl_step_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p]),
    "gnc_class_loss_workspace_doubles": (c_int32, []),
    "gnc_class_loss_launches": (c_int32, [c_int64, c_int32]),
    "gnc_class_loss_f32": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_double, c_double, c_int32, c_double,
                                     c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnc_knn_graph_f32": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p,
                                    c_void_p, c_void_p]),
    "gnc_knn_graph_padded_f32": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "gnc_knn_graph_constants": (None, [c_void_p, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class MlpSegment(Structure):
    _fields_ = [("ptr", c_void_p), ("index", c_void_p), ("width", c_int32), ("ld", c_int32), ("mode", c_int32),
                ("wcol", c_int32), ("table_rows", c_int64)]


class MlpDesc(Structure):
    _fields_ = [
        ("num_segments", c_int32), ("num_linear", c_int32), ("activation", c_int32), ("act_param", c_float),
        ("seg", MlpSegment * GNC_MAX_SEGMENTS),
        ("weight", c_void_p * GNC_MAX_LINEAR), ("ld_weight", c_int32 * GNC_MAX_LINEAR),
        ("bias", c_void_p * GNC_MAX_LINEAR),
        ("in_dim", c_int32 * GNC_MAX_LINEAR), ("out_dim", c_int32 * GNC_MAX_LINEAR),
        ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_eps", c_float),
        ("residual", c_void_p), ("ld_residual", c_int32),
        ("out", c_void_p), ("ld_out", c_int32),
        ("rows", c_int64),
        ("agg_out", c_void_p), ("ld_agg", c_int32), ("agg_index", c_void_p), ("agg_fix", c_void_p),
        ("save_act", c_void_p * GNC_MAX_LINEAR),
        ("ef_pos", c_void_p), ("ef_src", c_void_p), ("ef_dst", c_void_p), ("ef_nodes", c_int64), ("ef_space_dim", c_int32),
    ]


class MlpBwdDesc(Structure):
    _fields_ = [
        ("fwd", MlpDesc), ("grad_out", c_void_p), ("ld_grad_out", c_int32),
        ("act", c_void_p * GNC_MAX_LINEAR), ("dz", c_void_p * GNC_MAX_LINEAR),
        ("dx", c_void_p), ("ld_dx", c_int32), ("yhat", c_void_p), ("dx_add_grad_out", c_int32), ("ln_partial", c_void_p),
        ("dw_partial", c_void_p * GNC_MAX_LINEAR),
        ("grad_gather", c_void_p), ("ld_grad_gather", c_int32), ("grad_gather_index", c_void_p), ("grad_gather_rows", c_int64),
        ("grad_sum", c_void_p), ("ld_grad_sum", c_int32), ("act_given", c_int32),
    ]


class XtyJob(Structure):
    _fields_ = [("a", c_void_p), ("lda", c_int64), ("b", c_void_p), ("ldb", c_int64), ("rows", c_int64), ("m", c_int32),
                ("k", c_int32), ("dw", c_void_p), ("ld_dw", c_int64), ("db", c_void_p), ("kind", c_int32)]


class ReadoutBatchedPlan(Structure):
    _fields_ = [(name, c_int64) for name in ("f_slices", "f_slice_len", "tail_rows", "small_parts", "dw1_parts", "dw1_graph_range",
                                              "dy_groups", "forward_workspace_floats", "backward_workspace_floats")]


class GraphPoolPlan(Structure):
    _fields_ = [(name, c_int64) for name in ("chunk_rows", "split", "slots", "vec", "col_lanes", "row_lanes", "col_tiles",
                                              "workspace_floats")]


class WideLinearPlan(Structure):
    _fields_ = [(name, c_int64) for name in ("k_slices", "k_slice_len", "dw_parts", "dw_row_range", "forward_workspace_floats",
                                              "backward_workspace_floats")]


class OptCtl(Structure):
    """gnc_opt_ctl_t: the hyper-parameters of a controlled optimizer step (``optimizer_ctl_step``), constants of a run."""
    _fields_ = ([(name, c_int32) for name in ("rule", "schedule", "nesterov", "clip", "check_nonfinite", "reserved")]
                + [(name, c_int64) for name in ("warmup_steps", "total_steps", "every")]
                + [(name, c_double) for name in ("lr", "min_lr", "gamma", "max_grad_norm", "beta1", "beta2", "eps", "weight_decay",
                                                 "momentum")])


GNC_XTY_MAX_JOBS = 8

_lib = None


def load_library() -> ctypes.CDLL:
    """Load the in-tree shared library (torch is imported first so that its HIP runtime is
    the one already mapped).  Raises RuntimeError when it is missing or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("GNC_LIB_PATH", LIB_PATH)  # developer override: A/B builds and the phase-probe build
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C graphnet_classifier_amd/csrc`.  There is no CPU/PyTorch fallback for the hot path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.gnc_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_NAME}: ABI version {lib.gnc_abi_version()} != expected {ABI_VERSION}")
    if lib.gnc_sizeof_mlp_bwd_desc() != ctypes.sizeof(MlpBwdDesc):
        raise RuntimeError(f"{LIB_NAME}: gnc_mlp_bwd_desc_t is {lib.gnc_sizeof_mlp_bwd_desc()} bytes in C but "
                           f"{ctypes.sizeof(MlpBwdDesc)} in the ctypes binding")
    if lib.gnc_sizeof_mlp_desc() != ctypes.sizeof(MlpDesc):
        raise RuntimeError(f"{LIB_NAME}: gnc_mlp_desc_t is {lib.gnc_sizeof_mlp_desc()} bytes in C but "
                           f"{ctypes.sizeof(MlpDesc)} in the ctypes binding")
    if lib.gnc_sizeof_opt_ctl() != ctypes.sizeof(OptCtl):
        raise RuntimeError(f"{LIB_NAME}: gnc_opt_ctl_t is {lib.gnc_sizeof_opt_ctl()} bytes in C but {ctypes.sizeof(OptCtl)} in the "
                           f"ctypes binding")
    if lib.gnc_grad_norm_pass() != GRAD_NORM_PASS or lib.gnc_grad_norm_blocks() != GRAD_NORM_BLOCKS:
        raise RuntimeError(f"{LIB_NAME}: the gradient-norm grid is {lib.gnc_grad_norm_blocks()} workgroups of "
                           f"{lib.gnc_grad_norm_pass()} elements per pass in C, not {GRAD_NORM_BLOCKS} / {GRAD_NORM_PASS}")
    if lib.gnc_class_loss_workspace_doubles() != CLASS_LOSS_WORKSPACE_DOUBLES or lib.gnc_class_loss_launches(CLASS_LOSS_ONE_LAUNCH_ROWS, 1) != 1:
        raise RuntimeError(f"{LIB_NAME}: the loss head's workspace is {lib.gnc_class_loss_workspace_doubles()} doubles in C, not "
                           f"{CLASS_LOSS_WORKSPACE_DOUBLES}, or {CLASS_LOSS_ONE_LAUNCH_ROWS} rows are not one launch")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().gnc_last_error_string()
        raise RuntimeError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _require_cuda(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("graphnet_classifier_amd: the hot path runs on the GPU only; got a CPU tensor "
                               "(there is deliberately no CPU fallback)")


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    """2-D fp32 tensor with unit column stride (row stride may exceed the width)."""
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"expected a 2-D tensor, got shape {tuple(t.shape)}")
    if t.size(1) > 0 and t.stride(1) != 1 or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        t = t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    if t.size(0) > 1 or t.stride(0) >= t.size(1):
        return max(t.stride(0), 1)
    return max(t.size(1), 1)  # a single row whose stride says nothing


# --------------------------------------------------------------------------- kernel timers
class KernelTimers:
    """Optional HIP-event timing of individual launches (bench.py uses it for the roofline
    object).  Events are recorded on the stream the kernel is launched on (torch's current
    stream); nothing is synchronised until ``summary()`` is called after the timed region."""

    def __init__(self, only: str | None = None):
        self.events = {}
        self.work = {}
        self._pool = []
        self.only = only  # time launches of this name alone (every event record is a few microseconds of GPU time)

    def reserve(self, launches: int) -> None:
        """Create (and record once, which is what makes the runtime allocate them) the events of ``launches``
        launches ahead of a timed region: growing the runtime's event pool costs tens of milliseconds each time
        it happens (seen as one 50-70 ms step in every fresh process around the 900th event)."""
        stream = torch.cuda.current_stream()
        for _ in range(2 * launches):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream)
            self._pool.append(ev)

    def num_launches(self) -> int:
        return sum(len(v) for v in self.events.values())

    def launch(self, name: str, stream_tensor: torch.Tensor, fn, work: float = 0.0):
        if self.only is not None and name != self.only:
            return fn()
        start = self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)
        end = self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)
        start.record(torch.cuda.current_stream(stream_tensor.device))
        rc = fn()
        end.record(torch.cuda.current_stream(stream_tensor.device))
        self.events.setdefault(name, []).append((start, end))
        self.work.setdefault(name, []).append(work)
        return rc

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = {"launches": len(ms), "avg_ms": sum(ms) / len(ms), "min_ms": min(ms),
                         "avg_work": sum(self.work[name]) / len(ms)}
        return out


_timers: KernelTimers | None = None


def set_kernel_timers(timers: KernelTimers | None) -> None:
    global _timers
    _timers = timers


def _launch(name: str, t: torch.Tensor, fn, work: float = 0.0):
    return _timers.launch(name, t, fn, work) if _timers is not None else fn()


# --------------------------------------------------------------------------- topology
def csr_build(index: torch.Tensor, num_nodes: int):
    """index [E] int64 (device) -> (rowptr int32 [N+1], perm int32 [E], status int32 [2]: [0] = out-of-range flag of the build, [1] = scratch flag for a checked permute)."""
    lib = load_library()
    _require_cuda(index)
    if index.dtype != torch.int64:
        index = index.long()
    index = index.contiguous()
    e = index.numel()
    dev = index.device
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)  # [0]: written by the build, [1]: free for a checked permute
    with torch.cuda.device(dev):
        nbytes = lib.gnc_csr_workspace_bytes(num_nodes, e)
        if nbytes == 0:
            _check(-1, "gnc_csr_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _check(lib.gnc_csr_build(index.data_ptr(), e, num_nodes, rowptr.data_ptr(), perm.data_ptr(), status.data_ptr(),
                                 ws.data_ptr(), nbytes, _stream(index)), "gnc_csr_build")
    return rowptr, perm, status


def topology_build(src: torch.Tensor | None, dst: torch.Tensor, num_nodes: int, gated_fallback: bool = True):
    """(rowptr int32 [N+1], perm int32 [E], src_sorted int32 [E] | None, dst_sorted int32 [E] | None, status int32 [3]) of
    one edge list in ONE call (include/gnc_hip.h, gnc_topology_build): graph-ordered batches are sorted range by range in
    LDS; anything else raises status[2] on the device and - with ``gated_fallback`` - is sorted by the general kernels
    enqueued behind it.  ``src`` / ``dst``: int64 or int32 [E] on the device; ``src=None`` gives rowptr and perm only."""
    lib = load_library()
    _require_cuda(dst, src)
    if dst.dtype not in (torch.int64, torch.int32):
        dst = dst.long()
    dst = dst.contiguous()
    if src is not None:
        src = src.to(dst.dtype).contiguous()
    e, dev = dst.numel(), dst.device
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    ends = torch.empty(2, e, dtype=torch.int32, device=dev) if src is not None else None
    status = torch.empty(3, dtype=torch.int32, device=dev)  # zeroed by the call
    with torch.cuda.device(dev):
        nbytes = lib.gnc_topology_workspace_bytes(num_nodes, e, 1 if gated_fallback else 0)
        if nbytes == 0:
            _check(-1, "gnc_topology_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _check(lib.gnc_topology_build(src.data_ptr() if src is not None else None, dst.data_ptr(), dst.element_size(), e, num_nodes,
                                      rowptr.data_ptr(), perm.data_ptr(), ends[0].data_ptr() if ends is not None else None,
                                      ends[1].data_ptr() if ends is not None else None, status.data_ptr(), ws.data_ptr(), nbytes,
                                      1 if gated_fallback else 0, _stream(dst)), "gnc_topology_build")
    return rowptr, perm, (ends[0] if ends is not None else None), (ends[1] if ends is not None else None), status


def permute_index_checked(src: torch.Tensor, perm: torch.Tensor | None, num_nodes: int, status: torch.Tensor) -> torch.Tensor:
    """``permute_index`` that also flags ids outside [0, num_nodes) in ``status`` (int32 [1] on the device, zero
    before the call) and stores them as 0."""
    lib = load_library()
    _require_cuda(src, status)
    src = src.contiguous()
    out = torch.empty(src.numel(), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _check(lib.gnc_permute_index_checked_i64_i32(src.data_ptr(), perm.data_ptr() if perm is not None else None, src.numel(),
                                                     num_nodes, out.data_ptr(), status.data_ptr(), _stream(src)),
               "gnc_permute_index_checked_i64_i32")
    return out


def permute_index(src: torch.Tensor, perm: torch.Tensor | None) -> torch.Tensor:
    """int64 [E] -> int32 [E], reordered by perm (sorted position -> original edge)."""
    lib = load_library()
    _require_cuda(src)
    src = src.contiguous()
    out = torch.empty(src.numel(), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _check(lib.gnc_permute_index_i64_i32(src.data_ptr(), perm.data_ptr() if perm is not None else None, src.numel(),
                                             out.data_ptr(), _stream(src)), "gnc_permute_index_i64_i32")
    return out


# --------------------------------------------------------------------------- K1 / K2 / K6
def scatter_sum_csr(src: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor | None, num_nodes: int,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    lib = load_library()
    _require_cuda(src, rowptr)
    src = _rowmajor(src)
    e, d = src.shape
    if out is None:
        out = torch.empty(num_nodes, d, dtype=torch.float32, device=src.device)
    # algorithmic bytes of this launch: messages once, output once, row pointers,
    # and one int32 per edge only when the kernel has to go through the permutation
    work = 4.0 * d * e + 4.0 * d * num_nodes + 4.0 * (num_nodes + 1) + (4.0 * e if perm is not None else 0.0)
    with torch.cuda.device(src.device):
        _check(_launch("scatter_sum_csr" + ("_perm" if perm is not None else "_sorted"), src,
                       lambda: lib.gnc_scatter_sum_csr_f32(src.data_ptr(), _ld(src), rowptr.data_ptr(),
                                                           perm.data_ptr() if perm is not None else None, num_nodes,
                                                           e, d, out.data_ptr(), _ld(out), _stream(src)), work),
               "gnc_scatter_sum_csr_f32")
    return out


def gather_rows(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    _require_cuda(table, index)
    table = _rowmajor(table)
    if index.dtype != torch.int32:
        raise TypeError("gather_rows expects an int32 index")
    n, d = index.numel(), table.size(1)
    out = torch.empty(n, d, dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _check(lib.gnc_gather_rows_f32(table.data_ptr(), _ld(table), index.data_ptr(), n, d, out.data_ptr(), _ld(out),
                                       _stream(table)), "gnc_gather_rows_f32")
    return out


def gather_rows_add(table: torch.Tensor, index: torch.Tensor, addend: torch.Tensor) -> torch.Tensor:
    """out[r] = table[index[r]] + addend[r] in one pass."""
    lib = load_library()
    _require_cuda(table, index, addend)
    table, addend = _rowmajor(table), _rowmajor(addend)
    if index.dtype != torch.int32:
        raise TypeError("gather_rows_add expects an int32 index")
    n, d = index.numel(), table.size(1)
    if addend.shape != (n, d):
        raise ValueError(f"addend must be [{n}, {d}], got {tuple(addend.shape)}")
    out = torch.empty(n, d, dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _check(lib.gnc_gather_rows_add_f32(table.data_ptr(), _ld(table), index.data_ptr(), addend.data_ptr(), _ld(addend), n, d,
                                           out.data_ptr(), _ld(out), _stream(table)), "gnc_gather_rows_add_f32")
    return out



# --------------------------------------------------------------------------- K18: mean / max aggregation
SEGMENT_MEAN, SEGMENT_MAX = 1, 2  # GNC_SEGMENT_* of include/gnc_hip.h
SEGMENT_MODES = {"mean": SEGMENT_MEAN, "max": SEGMENT_MAX}


def _segment_mode(mode) -> int:
    mode = SEGMENT_MODES.get(mode, mode)
    if mode not in (SEGMENT_MEAN, SEGMENT_MAX):
        raise ValueError(f"segment_reduce: mode {mode!r} is not one of {sorted(SEGMENT_MODES)}")
    return mode


def segment_reduce_csr(src: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor | None, num_nodes: int, mode,
                       with_argmax: bool = False):
    """K1 with another reducer (csrc/segment_reduce.hip): ``(out [num_nodes, D], argmax)``.  ``mode``: ``"mean"`` / ``"max"``;
    ``argmax`` int32 [num_nodes, D] - the row of ``src`` that won each column, -1 for a destination without rows - comes only
    with ``with_argmax`` (max), else None and the launch stores nothing for it."""
    lib = load_library()
    _require_cuda(src, rowptr, perm)
    mode = _segment_mode(mode)
    if with_argmax and mode != SEGMENT_MAX:
        raise ValueError("segment_reduce_csr: argmax comes with mode 'max' only")
    if rowptr.dtype != torch.int32 or (perm is not None and perm.dtype != torch.int32):
        raise TypeError("segment_reduce_csr expects int32 rowptr / perm")
    if rowptr.numel() != num_nodes + 1:
        raise ValueError(f"segment_reduce_csr: rowptr has {rowptr.numel()} entries for {num_nodes} nodes")
    src = _rowmajor(src)
    e, d = src.shape
    out = torch.empty(num_nodes, d, dtype=torch.float32, device=src.device)
    argmax = torch.empty(num_nodes, d, dtype=torch.int32, device=src.device) if with_argmax else None
    # algorithmic bytes: K1's, plus one int32 per output element when the winners are stored
    work = (4.0 * d * e + 4.0 * d * num_nodes + 4.0 * (num_nodes + 1) + (4.0 * e if perm is not None else 0.0)
            + (4.0 * d * num_nodes if with_argmax else 0.0))
    name = "segment_" + ("mean" if mode == SEGMENT_MEAN else "max_argmax" if with_argmax else "max") + "_csr"
    with torch.cuda.device(src.device):
        _check(_launch(name, src,
                       lambda: lib.gnc_segment_reduce_csr_f32(src.data_ptr(), _ld(src), rowptr.data_ptr(),
                                                              perm.data_ptr() if perm is not None else None, num_nodes, e, d, mode,
                                                              out.data_ptr(), _ld(out),
                                                              argmax.data_ptr() if argmax is not None else None, _stream(src)), work),
               "gnc_segment_reduce_csr_f32")
    return out, argmax


def segment_reduce_backward(grad_out: torch.Tensor, dst_of_row: torch.Tensor, rowptr: torch.Tensor, argmax: torch.Tensor | None,
                            mode) -> torch.Tensor:
    """``grad_src`` [E, D] of ``segment_reduce_csr`` in one pass over its rows: ``dst_of_row`` int32 [E] is the destination of
    each row of the forward's ``src``; mean needs ``rowptr``, max the forward's ``argmax``."""
    lib = load_library()
    _require_cuda(grad_out, dst_of_row, rowptr, argmax)
    mode = _segment_mode(mode)
    grad_out = _rowmajor(grad_out)
    n, d = grad_out.shape
    if dst_of_row.dtype != torch.int32 or rowptr.dtype != torch.int32:
        raise TypeError("segment_reduce_backward expects int32 dst_of_row / rowptr")
    if rowptr.numel() != n + 1:
        raise ValueError(f"segment_reduce_backward: rowptr has {rowptr.numel()} entries for {n} rows of grad_out")
    if mode == SEGMENT_MAX and (argmax is None or argmax.dtype != torch.int32 or tuple(argmax.shape) != (n, d)
                                or not argmax.is_contiguous()):
        raise ValueError("segment_reduce_backward: max needs the forward's contiguous int32 argmax [N, D]")
    e = dst_of_row.numel()
    grad_src = torch.empty(e, d, dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _check(_launch("segment_" + ("mean" if mode == SEGMENT_MEAN else "max") + "_backward", grad_out,
                       lambda: lib.gnc_segment_reduce_backward_f32(grad_out.data_ptr(), _ld(grad_out), dst_of_row.data_ptr(),
                                                                   rowptr.data_ptr(),
                                                                   argmax.data_ptr() if mode == SEGMENT_MAX else None, n, e, d, mode,
                                                                   grad_src.data_ptr(), _ld(grad_src), _stream(grad_out)),
                       4.0 * d * e + 4.0 * e + (8.0 if mode == SEGMENT_MAX else 4.0) * d * n),
               "gnc_segment_reduce_backward_f32")
    return grad_src


def rows_div_degree_(table: torch.Tensor, rowptr: torch.Tensor) -> torch.Tensor:
    """In place: row v of ``table`` [N, D] divided by ``float(rowptr[v + 1] - rowptr[v])``, rows of degree 0 left alone."""
    lib = load_library()
    _require_cuda(table, rowptr)
    if table.dtype != torch.float32 or table.dim() != 2 or (table.size(1) > 0 and table.stride(1) != 1):
        raise ValueError("rows_div_degree_: a 2-D float32 table with unit column stride expected")
    if rowptr.dtype != torch.int32 or rowptr.numel() != table.size(0) + 1:
        raise ValueError(f"rows_div_degree_: int32 rowptr with {table.size(0) + 1} entries expected")
    n, d = table.shape
    with torch.cuda.device(table.device):
        _check(_launch("rows_div_degree", table,
                       lambda: lib.gnc_rows_div_degree_f32(table.data_ptr(), _ld(table), rowptr.data_ptr(), n, d, _stream(table)),
                       8.0 * d * n + 4.0 * (n + 1)), "gnc_rows_div_degree_f32")
    return table


# --------------------------------------------------------------------------- K21: attention aggregation
def _scores_of(scores: torch.Tensor, rows: int, who: str) -> torch.Tensor:
    if scores.dtype != torch.float32 or scores.numel() != rows:
        raise ValueError(f"{who}: float32 scores with one entry per row of src ({rows}) expected, got {scores.dtype} "
                         f"{tuple(scores.shape)}")
    return scores.reshape(-1).contiguous()


def segment_softmax_csr(src: torch.Tensor, scores: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor | None, num_nodes: int):
    """K21 forward (csrc/segment_softmax.hip): ``(out [num_nodes, D], saved [num_nodes, 2])`` - per destination the softmax of the
    ``scores`` of its rows weighting the sum of those rows of ``src``; ``saved[v] = (max score, sum of exp)`` is what the backward and
    ``segment_softmax_weights`` rebuild the weights from.  ``perm`` (sorted position -> row) indexes ``src`` and ``scores`` alike."""
    lib = load_library()
    _require_cuda(src, scores, rowptr, perm)
    if rowptr.dtype != torch.int32 or (perm is not None and perm.dtype != torch.int32):
        raise TypeError("segment_softmax_csr expects int32 rowptr / perm")
    if rowptr.numel() != num_nodes + 1:
        raise ValueError(f"segment_softmax_csr: rowptr has {rowptr.numel()} entries for {num_nodes} nodes")
    src = _rowmajor(src)
    e, d = src.shape
    scores = _scores_of(scores, e, "segment_softmax_csr")
    out = torch.empty(num_nodes, d, dtype=torch.float32, device=src.device)
    saved = torch.empty(num_nodes, 2, dtype=torch.float32, device=src.device)
    # algorithmic bytes: K18's, plus the scores twice and (m, Z) per destination
    work = (4.0 * d * e + 8.0 * e + 4.0 * d * num_nodes + 8.0 * num_nodes + 4.0 * (num_nodes + 1)
            + (4.0 * e if perm is not None else 0.0))
    with torch.cuda.device(src.device):
        _check(_launch("segment_softmax_csr", src,
                       lambda: lib.gnc_segment_softmax_csr_f32(src.data_ptr(), _ld(src), scores.data_ptr(), rowptr.data_ptr(),
                                                               perm.data_ptr() if perm is not None else None, num_nodes, e, d,
                                                               out.data_ptr(), _ld(out), saved.data_ptr(), _stream(src)), work),
               "gnc_segment_softmax_csr_f32")
    return out, saved


def segment_softmax_backward(grad_out: torch.Tensor, src: torch.Tensor, scores: torch.Tensor, out: torch.Tensor, saved: torch.Tensor,
                             dst_of_row: torch.Tensor):
    """``(grad_src [E, D], grad_scores [E])`` of ``segment_softmax_csr`` in one pass over its rows; ``dst_of_row`` int32 [E] is the
    destination of each row of the forward's ``src``."""
    lib = load_library()
    _require_cuda(grad_out, src, scores, out, saved, dst_of_row)
    grad_out, src, out = _rowmajor(grad_out), _rowmajor(src), _rowmajor(out)
    n, d = out.shape
    e = src.size(0)
    if dst_of_row.dtype != torch.int32 or dst_of_row.numel() != e:
        raise TypeError(f"segment_softmax_backward expects an int32 dst_of_row with {e} entries")
    if tuple(grad_out.shape) != (n, d) or src.size(1) != d:
        raise ValueError(f"segment_softmax_backward: grad_out {tuple(grad_out.shape)}, src {tuple(src.shape)}, out {(n, d)} disagree")
    if saved.dtype != torch.float32 or tuple(saved.shape) != (n, 2) or not saved.is_contiguous():
        raise ValueError("segment_softmax_backward: the forward's contiguous float32 saved [N, 2] expected")
    scores = _scores_of(scores, e, "segment_softmax_backward")
    grad_src = torch.empty(e, d, dtype=torch.float32, device=src.device)
    grad_scores = torch.empty(e, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _check(_launch("segment_softmax_backward", src,
                       lambda: lib.gnc_segment_softmax_backward_f32(grad_out.data_ptr(), _ld(grad_out), src.data_ptr(), _ld(src),
                                                                    scores.data_ptr(), out.data_ptr(), _ld(out), saved.data_ptr(),
                                                                    dst_of_row.data_ptr(), n, e, d, grad_src.data_ptr(),
                                                                    _ld(grad_src), grad_scores.data_ptr(), _stream(src)),
                       8.0 * d * e + 12.0 * e + 8.0 * d * n + 8.0 * n), "gnc_segment_softmax_backward_f32")
    return grad_src, grad_scores


def segment_softmax_weights(scores: torch.Tensor, saved: torch.Tensor, dst_of_row: torch.Tensor) -> torch.Tensor:
    """``alpha`` [E]: the softmax weight of every row, rebuilt from the forward's ``saved``."""
    lib = load_library()
    _require_cuda(scores, saved, dst_of_row)
    e = dst_of_row.numel()
    if dst_of_row.dtype != torch.int32:
        raise TypeError("segment_softmax_weights expects an int32 dst_of_row")
    if saved.dtype != torch.float32 or saved.dim() != 2 or saved.size(1) != 2 or not saved.is_contiguous():
        raise ValueError("segment_softmax_weights: the forward's contiguous float32 saved [N, 2] expected")
    scores = _scores_of(scores, e, "segment_softmax_weights")
    alpha = torch.empty(e, dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        _check(lib.gnc_segment_softmax_weights_f32(scores.data_ptr(), saved.data_ptr(), dst_of_row.data_ptr(), e, alpha.data_ptr(),
                                                   _stream(scores)), "gnc_segment_softmax_weights_f32")
    return alpha


def edge_features(pos: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    _require_cuda(pos, src, dst)
    pos = pos.float().contiguous()
    e, sd = src.numel(), pos.size(1)
    ld = (sd + 1 + 3) // 4 * 4  # rows padded to a multiple of 16 B (zeros) for the MLP kernels' vector loads
    buf = torch.empty(e, ld, dtype=torch.float32, device=pos.device)
    with torch.cuda.device(pos.device):
        _check(lib.gnc_edge_features_f32(pos.data_ptr(), sd, src.data_ptr(), dst.data_ptr(), e, buf.data_ptr(), ld,
                                         _stream(pos)), "gnc_edge_features_f32")
    return buf[:, :sd + 1]


def poison_if_flagged_(out: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """In place: ``out`` (contiguous fp32) becomes NaN when any of the int32 device ``flags`` is set; one launch that returns
    at once otherwise (deferred topology validation)."""
    lib = load_library()
    _require_cuda(out, flags)
    if not out.is_contiguous() or out.dtype != torch.float32 or flags.dtype != torch.int32 or not flags.is_contiguous():
        raise TypeError("poison_if_flagged_: contiguous fp32 output and contiguous int32 flags expected")
    with torch.cuda.device(out.device):
        _check(lib.gnc_poison_if_flagged_f32(out.data_ptr(), out.numel(), flags.data_ptr(), flags.numel(), _stream(out)),
               "gnc_poison_if_flagged_f32")
    return out


# --------------------------------------------------------------------------- K4
def make_mlp_desc(segments, weights, biases, ln, activation: str, act_param: float, residual, out, rows: int):
    """Fill a gnc_mlp_desc_t.  ``segments`` = [(table, index_or_None, width, mode, wcol)], tensors must stay
    alive until the call returns (they are enqueued on the current stream)."""
    if len(segments) > GNC_MAX_SEGMENTS or not (1 <= len(weights) <= GNC_MAX_LINEAR):
        raise NotImplementedError(f"MLP with {len(segments)} segments / {len(weights)} Linear layers is outside the HIP kernel")
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f"activation nn.{activation} has no HIP kernel (supported: {sorted(ACTIVATIONS)})")
    d = MlpDesc()
    d.num_segments = len(segments)
    d.num_linear = len(weights)
    d.activation = ACTIVATIONS[activation]
    d.act_param = act_param
    for s, (table, index, width, mode, wcol) in enumerate(segments):
        d.seg[s].wcol = wcol
        d.seg[s].ptr = table.data_ptr()
        d.seg[s].index = index.data_ptr() if index is not None else None
        d.seg[s].width = width
        d.seg[s].ld = _ld(table)
        d.seg[s].mode = mode
        d.seg[s].table_rows = table.size(0) if index is not None else 0
    for l, (w, b) in enumerate(zip(weights, biases)):
        d.weight[l] = w.data_ptr()
        d.ld_weight[l] = _ld(w)
        d.bias[l] = b.data_ptr() if b is not None else None
        d.out_dim[l], d.in_dim[l] = w.shape
    if ln is not None:
        d.ln_gamma, d.ln_beta, d.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), ln[2]
    if residual is not None:
        d.residual, d.ld_residual = residual.data_ptr(), _ld(residual)
    d.out, d.ld_out = out.data_ptr(), _ld(out)
    d.rows = rows
    return d


SEG_MATMUL, SEG_ADD = 0, 1

def _vector_rows(t: torch.Tensor) -> torch.Tensor:
    """Rows the kernels can read with 16-B vector loads: row stride a multiple of 4 floats and a 16-B
    aligned base.  Anything else (the reference's 3-column inputs and [H, 3] first-layer weights) is
    copied into a zero-padded buffer (one pad launch) and handed over as a column slice of it.  Nothing is
    cached: the copy is made from the live tensor on every call, so in-place edits through ``.data``
    (which do not bump ``_version``), ``load_state_dict`` and optimizer steps are always seen, and a
    hipGraph capture records the pad itself instead of a pointer to a stale copy."""
    if t.data_ptr() % 16 == 0 and _ld(t) % 4 == 0:
        return t
    cols = (t.size(1) + 3) // 4 * 4
    if t.stride(1) != 1 or t.stride(0) != t.size(1):
        t = t.contiguous()
    if cols == t.size(1):  # only the base address was off (a column slice of a wider tensor): fresh, aligned copy
        return t.clone(memory_format=torch.contiguous_format)
    return torch.nn.functional.pad(t, (0, cols - t.size(1)))[:, :t.size(1)]


_SMALL_ROWS = None


def _small_batch_rows(lib) -> int:
    """Row limit of the small-batch forward kernel (asked once)."""
    global _SMALL_ROWS
    if _SMALL_ROWS is None:
        _SMALL_ROWS = int(lib.gnc_mlp_small_batch_max_rows())
    return _SMALL_ROWS


def _rows_of(segments, rows) -> int:
    if rows is not None:
        return int(rows)
    t0, i0 = segments[0]
    return int(i0.numel() if i0 is not None else t0.size(0))


def _prepare_mlp(segments, weights, biases, residual, rows, modes, vector_rows: bool = True):
    """Shared argument preparation of the forward and backward launches (see mlp_forward).  ``vector_rows=False`` hands
    tables and weights over as they are (row-major, any alignment): only for a launch whose kernel reads them in place
    (gnc_mlp_small_batch_supported, gnc_mlp_operands_in_place_supported)."""
    _vr = _vector_rows if vector_rows else (lambda t: t)
    _vw = _vr
    modes = list(modes) if modes is not None else [SEG_MATMUL] * len(segments)
    segs, wcol = [], 0
    for (table, index), mode in zip(segments, modes):
        _require_cuda(table, index)
        table = _vr(_rowmajor(table))
        if index is not None and index.dtype != torch.int32:
            raise TypeError("segment index must be int32")
        segs.append((table, index, table.size(1), mode, wcol if mode == SEG_MATMUL else 0))
        if mode == SEG_MATMUL:
            wcol += table.size(1)
    # kernel-side order: MATMUL segments first (the one that is also the residual last among them, so
    # its rows can stay in registers for the residual add), then the additive segments
    def _rank(sg):
        is_res = (residual is not None and sg[1] is None and sg[0].data_ptr() == residual.data_ptr()
                  and sg[0].shape == residual.shape)
        return (sg[3] == SEG_ADD, is_res)
    segs.sort(key=_rank)
    if rows is None:
        t0, i0 = segments[0]
        rows = i0.numel() if i0 is not None else t0.size(0)
    weights = [_vw(_rowmajor(w.detach())) for w in weights]
    biases = [b.contiguous() if b is not None else None for b in biases]
    if residual is not None:
        residual = _rowmajor(residual)
    return segs, weights, biases, residual, rows, modes


SAVE_ACT = os.environ.get("GNC_NO_SAVED_ACT") is None  # A/B switch: training forwards keep nothing, backwards recompute


def _saved_act_honoured(lib, desc, act_ptrs, need_dx: bool, fused: bool) -> bool:
    """gnc_mlp_backward_saved_act_honoured for the forward description ``desc`` with post-activations at ``act_ptrs``:
    ``need_dx`` - the backward will be asked for the input gradient, ``fused`` - and for weight-gradient partials (the
    kernel choice, and with it the answer, depends on both).  The query looks at the addresses' alignment only."""
    bd = MlpBwdDesc()
    ctypes.memmove(ctypes.byref(bd.fwd), ctypes.byref(desc), ctypes.sizeof(MlpDesc))
    for l, ptr in enumerate(act_ptrs):
        bd.act[l] = ptr
    bd.act_given, bd.dx = 1, (act_ptrs[0] if need_dx else None)
    bd.dw_partial[0] = act_ptrs[0] if fused else None
    return lib.gnc_mlp_backward_saved_act_honoured(ctypes.byref(bd)) == 1


def _backward_reads_saved_act(lib, desc, any_tensor, need_dx: bool = True) -> bool:
    """Would gnc_mlp_backward_f32 read saved post-activations for this description?  (Shape question only: the K8 kernel
    of some shapes - the weights-resident data kernel of the node processors - recomputes regardless, and a forward that
    saved for it would write tensors nobody reads.)  ``any_tensor``: any 16-B aligned device tensor."""
    fused = lib.gnc_mlp_backward_fused_rows(ctypes.byref(desc)) > 0
    return _saved_act_honoured(lib, desc, [any_tensor.data_ptr()] * (desc.num_linear - 1), need_dx, fused)


def mlp_forward(segments, weights, biases, ln=None, activation: str = "ReLU", act_param: float = 0.0,
                residual: torch.Tensor | None = None, rows: int | None = None, modes=None, aggregate=None,
                save_act: list | None = None, save_need_dx: bool = True, agg_only: bool = False):
    """Fused MLP.  segments (in CONCAT order): list of (table [*, w] fp32, index int32 [rows] | None);
    ``modes[s]`` is SEG_MATMUL (default) or SEG_ADD.  Weights may be column slices of a larger
    matrix.  The segment that is also the residual is listed last for the kernel (its weight
    columns are carried in ``wcol``), so the residual comes from the staged rows.

    ``aggregate=(dst_of_row int32 [rows] non-decreasing, rowptr int32 [N+1], N)`` asks for the fused aggregation
    epilogue: returns ``(out, agg)`` with ``agg[v] = sum of out rows with dst v`` in row order,
    bit-identical to ``scatter_sum_csr(out, rowptr)``; returns ``(out, None)`` when the launch shape cannot
    carry it (the caller then runs K1).  With ``agg_only`` as well, the output rows are not wanted: where
    gnc_mlp_agg_only_supported says so the launch stores only the rows the fix-up reads and ``(None, agg)`` comes back
    (``agg`` bit-identical to the storing launch's); otherwise the storing launch runs and ``(out, agg)`` comes back.

    ``save_act`` (training forward): an empty list; when the kernel that serves the call can write the post-activation
    outputs of its hidden layers (gnc_mlp_save_act_supported) they are appended to it ([rows, H] each) for
    ``mlp_backward(saved_act=...)``, which then reads them instead of recomputing the forward of every tile;
    ``save_need_dx`` says whether that backward will want the input gradient (``need_dx``)."""
    lib = load_library()
    given = (segments, weights, biases, residual, rows, modes)
    small = _rows_of(segments, rows) <= _small_batch_rows(lib)
    # inference launches without extras: tables and weights go over as they lie first ([N, 3] inputs and [H, 3] first-layer
    # matrices cost a pad launch pair each per call otherwise) and are padded only when the kernel that will serve the launch
    # reads rows of 16-B pieces
    raw = not small and save_act is None and aggregate is None
    segs, weights, biases, residual, rows, modes = _prepare_mlp(*given, vector_rows=not (small or raw))
    dev = segs[0][0].device
    out = torch.empty(rows, weights[-1].size(0), dtype=torch.float32, device=dev)
    desc = make_mlp_desc(segs, weights, biases, ln, activation, act_param, residual, out, rows)
    if raw and any(t.data_ptr() % 16 or _ld(t) % 4 for t in [sg[0] for sg in segs] + weights) and \
            lib.gnc_mlp_operands_in_place_supported(ctypes.byref(desc)) != 0:
        segs, weights, biases, residual, rows, modes = _prepare_mlp(*given)  # a streaming kernel: rows of 16-B pieces
        desc = make_mlp_desc(segs, weights, biases, ln, activation, act_param, residual, out, rows)
    if small and lib.gnc_mlp_small_batch_supported(ctypes.byref(desc)) != 0:
        # every other kernel reads rows as 16-B pieces: 3-column inputs / [H, 3] weights go through a zero-padded copy
        # (one pad launch each); the small-batch kernel reads them where they lie
        segs, weights, biases, residual, rows, modes = _prepare_mlp(*given)
        desc = make_mlp_desc(segs, weights, biases, ln, activation, act_param, residual, out, rows)
    if (save_act is not None and SAVE_ACT and rows > 0 and len(weights) >= 2
            and lib.gnc_mlp_save_act_supported(ctypes.byref(desc)) == 0 and _backward_reads_saved_act(lib, desc, out, save_need_dx)):
        for l in range(len(weights) - 1):
            a = torch.empty(rows, weights[l].size(0), dtype=torch.float32, device=dev)
            desc.save_act[l] = a.data_ptr()
            save_act.append(a)
    agg = fix = None
    if aggregate is not None:
        dst_of_row, rowptr, num_nodes = aggregate
        _require_cuda(dst_of_row, rowptr)
        if rows > 0 and lib.gnc_mlp_agg_supported(ctypes.byref(desc)) == 0:
            agg = torch.empty(num_nodes, out.size(1), dtype=torch.float32, device=dev)  # fully defined after the fix-up
            fix = torch.empty(lib.gnc_mlp_agg_fix_len(), dtype=torch.int32, device=dev)
            desc.agg_out, desc.ld_agg = agg.data_ptr(), _ld(agg)
            desc.agg_index, desc.agg_fix = dst_of_row.contiguous().data_ptr(), fix.data_ptr()
    agg_only = agg_only and agg is not None and lib.gnc_mlp_agg_only_supported(ctypes.byref(desc)) == 0
    forward = lib.gnc_mlp_forward_agg_only_f32 if agg_only else lib.gnc_mlp_forward_f32
    # executed FLOPs of this launch: 2 * rows * sum(in*out) over the Linear layers
    flops = 2.0 * rows * sum(w.size(0) * w.size(1) for w in weights)
    with torch.cuda.device(dev):
        nadd = sum(1 for m in modes if m == SEG_ADD)
        _check(_launch(f"mlp_fused_in{weights[0].size(1)}{'+%dadd' % nadd if nadd else ''}_h{weights[0].size(0)}"
                       f"_out{weights[-1].size(0)}_L{len(weights)}", out,
                       lambda: forward(ctypes.byref(desc), _stream(out)), flops),
               forward.__name__)
        if agg is not None:  # the destinations cut by a wave-range boundary, from the stored rows (same stream)
            _check(lib.gnc_agg_fixup_f32(out.data_ptr(), _ld(out), rowptr.data_ptr(), fix.data_ptr(), fix.numel(), num_nodes,
                                         out.size(1), agg.data_ptr(), _ld(agg), _stream(out)), "gnc_agg_fixup_f32")
    return (None if agg_only else out, agg) if aggregate is not None else out


FOLD_EDGE_FEATURES = os.environ.get("GNC_NO_K6_FOLD") is None  # A/B switch: K6 as its own launch + a [E, 4] table


def mlp_forward_edge_features(pos: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, weights, biases, ln=None,
                              activation: str = "ReLU", act_param: float = 0.0):
    """The edge encoder on edge features that are never stored (models/GNN.py:299-302 feeding :306): K6 runs as the
    prologue of the K4 launch (gnc_mlp_desc_t.ef_pos, ABI 19).  ``pos`` [N, 2] fp32, ``src`` / ``dst`` int32 [E] (the
    topology's sorted endpoint vectors).  Inference only.  Returns None when no kernel serves the shape this way
    (gnc_mlp_edge_features_supported): the caller then runs ``edge_features`` + ``mlp_forward``; bit-identical either way."""
    lib = load_library()
    if not FOLD_EDGE_FEATURES or pos.dim() != 2 or pos.size(1) != 2 or src.numel() == 0:
        return None
    _require_cuda(pos, src, dst)
    if src.dtype != torch.int32 or dst.dtype != torch.int32:
        raise TypeError("edge endpoint ids must be int32")
    pos = pos.float().contiguous()
    src, dst = src.contiguous(), dst.contiguous()
    rows, sd = src.numel(), pos.size(1)
    if weights[0].size(1) != sd + 1 or rows <= _small_batch_rows(lib):
        return None
    weights = [_rowmajor(w.detach()) for w in weights]  # read where they lie: only the weights-resident kernel serves this form
    biases = [b.contiguous() if b is not None else None for b in biases]
    dev = pos.device
    out = torch.empty(rows, weights[-1].size(0), dtype=torch.float32, device=dev)
    desc = make_mlp_desc([(pos, None, sd + 1, SEG_MATMUL, 0)], weights, biases, ln, activation, act_param, None, out, rows)
    desc.seg[0].ld = 4  # the segment's table is never read (computed rows); ld only has to cover the width
    desc.ef_pos, desc.ef_src, desc.ef_dst = pos.data_ptr(), src.data_ptr(), dst.data_ptr()
    desc.ef_nodes, desc.ef_space_dim = pos.size(0), sd
    if lib.gnc_mlp_edge_features_supported(ctypes.byref(desc)) != 0:
        return None
    flops = 2.0 * rows * sum(w.size(0) * w.size(1) for w in weights)
    with torch.cuda.device(dev):
        _check(_launch(f"mlp_fused_in{weights[0].size(1)}_h{weights[0].size(0)}_out{weights[-1].size(0)}_L{len(weights)}", out,
                       lambda: lib.gnc_mlp_forward_f32(ctypes.byref(desc), _stream(out)), flops), "gnc_mlp_forward_f32")
    return out


READOUT_MAX_HIDDEN, READOUT_MAX_CLASSES = 1024, 64
_readout_tickets: dict = {}


def _readout_ticket(dev) -> torch.Tensor:
    """One zeroed device counter per device AND stream (every launch leaves it at 0; launches on one stream are ordered, launches
    on different streams must not share a counter)."""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    if key not in _readout_tickets:
        _readout_tickets[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _readout_tickets[key]


def readout_forward(y, w1, b1, w2, b2, w3, b3):
    """logits [C] = fc3(relu(fc2(relu(fc1(y))))) for ONE flattened graph output y [F] in one launch (gnc_readout_forward_f32);
    also returns the two post-ReLU hidden vectors for the backward."""
    lib = load_library()
    _require_cuda(y, w1, w2, w3)
    y = y.contiguous()
    w1, w2, w3 = _rowmajor(w1.detach()), _rowmajor(w2.detach()), _rowmajor(w3.detach())
    dev = y.device
    h1 = torch.empty(w1.size(0), dtype=torch.float32, device=dev)
    h2 = torch.empty(w2.size(0), dtype=torch.float32, device=dev)
    logits = torch.empty(w3.size(0), dtype=torch.float32, device=dev)
    bp = [b.detach().contiguous() if b is not None else None for b in (b1, b2, b3)]
    with torch.cuda.device(dev):
        _check(_launch("readout_forward", y,
                       lambda: lib.gnc_readout_forward_f32(y.data_ptr(), y.numel(), w1.data_ptr(), _ld(w1), bp[0].data_ptr() if bp[0] is not None else None,
                                                           w1.size(0), w2.data_ptr(), _ld(w2), bp[1].data_ptr() if bp[1] is not None else None, w2.size(0),
                                                           w3.data_ptr(), _ld(w3), bp[2].data_ptr() if bp[2] is not None else None, w3.size(0),
                                                           h1.data_ptr(), h2.data_ptr(), logits.data_ptr(), _readout_ticket(dev).data_ptr(), _stream(y)),
                       2.0 * (w1.numel() + w2.numel() + w3.numel())), "gnc_readout_forward_f32")
    return logits, h1, h2


def readout_backward(grad_logits, y, w1, w2, w3, h1, h2, need_dy: bool = True):
    """All gradients of ``readout_forward`` in one launch: (dy or None, dW1, db1, dW2, db2, dW3, db3)."""
    lib = load_library()
    g = grad_logits.contiguous()
    y = y.contiguous()
    w1, w2, w3 = _rowmajor(w1.detach()), _rowmajor(w2.detach()), _rowmajor(w3.detach())
    dev = y.device
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)  # noqa: E731
    dw1, db1, dw2, db2, dw3, db3 = e(*w1.shape), e(w1.size(0)), e(*w2.shape), e(w2.size(0)), e(*w3.shape), e(w3.size(0))
    dy = e(y.numel()) if need_dy else None
    with torch.cuda.device(dev):
        _check(_launch("readout_backward", y,
                       lambda: lib.gnc_readout_backward_f32(g.data_ptr(), y.data_ptr(), y.numel(), w1.data_ptr(), _ld(w1), w1.size(0), w2.data_ptr(),
                                                            _ld(w2), w2.size(0), w3.data_ptr(), _ld(w3), w3.size(0), h1.data_ptr(), h2.data_ptr(),
                                                            dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), dw3.data_ptr(),
                                                            db3.data_ptr(), dy.data_ptr() if dy is not None else None, _stream(y)),
                       4.0 * w1.numel()), "gnc_readout_backward_f32")
    return dy, dw1, db1, dw2, db2, dw3, db3


def readout_batched_plan(num_graphs: int, features: int, h1: int, h2: int, classes: int) -> dict | None:
    """The library's decision for the batched read-out of ``num_graphs`` graphs with ``features`` fc1 inputs each (host only, no
    GPU needed): None when the shape is left to the torch path, otherwise the split the launches will use - ``f_slices`` x
    ``f_slice_len`` of F in the forward, the graph chunks of the backward - and the workspace sizes in floats."""
    plan = ReadoutBatchedPlan()
    if not load_library().gnc_readout_batched_supported(int(num_graphs), int(features), int(h1), int(h2), int(classes), ctypes.byref(plan)):
        return None
    return {name: int(getattr(plan, name)) for name, _ in ReadoutBatchedPlan._fields_}


def readout_batched_supported(num_graphs: int, features: int, h1: int, h2: int, classes: int) -> bool:
    return bool(load_library().gnc_readout_batched_supported(int(num_graphs), int(features), int(h1), int(h2), int(classes), None))


def _graph_ptr_arg(graph_ptr, num_graphs: int, dev):
    if graph_ptr is None:
        return None
    if graph_ptr.dtype != torch.int64 or graph_ptr.device != dev or graph_ptr.numel() != num_graphs + 1:
        raise ValueError("readout_batched: graph_ptr must be int64 [num_graphs + 1] on the device of y")
    return graph_ptr.contiguous()


def readout_batched_forward(y, graph_ptr, num_graphs: int, num_nodes: int, w1, b1, w2, b2, w3, b3):
    """logits [G, C] = fc3(relu(fc2(relu(fc1(feats))))) for the G graphs of a block-diagonal batch, ``y`` [N_total, out_dim] being
    the GraphNet output (gnc_readout_batched_forward_f32: fc1 with the gather fused into its operand load, then the tail).
    ``graph_ptr`` int64 [G + 1] on the device, or None for G graphs of exactly ``num_nodes`` rows.  Also returns the post-ReLU
    ``h1`` [G, 128] and ``h2`` [G, H2] for the backward."""
    lib = load_library()
    _require_cuda(y, w1, w2, w3)
    y = _rowmajor(y).contiguous()
    w1, w2, w3 = _rowmajor(w1.detach()), _rowmajor(w2.detach()), _rowmajor(w3.detach())
    dev, G, od = y.device, int(num_graphs), y.size(1)
    gp = _graph_ptr_arg(graph_ptr, G, dev)
    plan = readout_batched_plan(G, int(num_nodes) * od, w1.size(0), w2.size(0), w3.size(0))
    if plan is None:
        raise RuntimeError("readout_batched_forward: shape outside the kernel's set (ask readout_batched_supported first)")
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)  # noqa: E731
    h1, h2, logits = e(G, w1.size(0)), e(G, w2.size(0)), e(G, w3.size(0))
    ws = e(max(plan["forward_workspace_floats"], 1))
    bp = [b.detach().contiguous() if b is not None else None for b in (b1, b2, b3)]
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        _check(_launch("readout_batched_forward", y,
                       lambda: lib.gnc_readout_batched_forward_f32(
                           y.data_ptr(), ptr(gp), G, int(num_nodes), od, y.size(0), w1.data_ptr(), _ld(w1), ptr(bp[0]), w1.size(0),
                           w2.data_ptr(), _ld(w2), ptr(bp[1]), w2.size(0), w3.data_ptr(), _ld(w3), ptr(bp[2]), w3.size(0),
                           h1.data_ptr(), h2.data_ptr(), logits.data_ptr(), ws.data_ptr(), ws.numel(), _stream(y)),
                       2.0 * G * (int(num_nodes) * od * w1.size(0) + w2.numel() + w3.numel())), "gnc_readout_batched_forward_f32")
    return logits, h1, h2


def readout_batched_backward(grad_logits, y, graph_ptr, num_graphs: int, num_nodes: int, w1, w2, w3, h1, h2, need_dy: bool = True):
    """All gradients of ``readout_batched_forward``: (dy [N_total, out_dim] or None, dW1, db1, dW2, db2, dW3, db3).  ``dy`` is written
    for every row (exact zeros where a row does not reach fc1); the five small gradients are views of one buffer."""
    lib = load_library()
    g = grad_logits.contiguous()
    y = _rowmajor(y).contiguous()
    w1, w2, w3 = _rowmajor(w1.detach()), _rowmajor(w2.detach()), _rowmajor(w3.detach())
    dev, G, od = y.device, int(num_graphs), y.size(1)
    H1, H2, C = w1.size(0), w2.size(0), w3.size(0)
    gp = _graph_ptr_arg(graph_ptr, G, dev)
    plan = readout_batched_plan(G, int(num_nodes) * od, H1, H2, C)
    if plan is None:
        raise RuntimeError("readout_batched_backward: shape outside the kernel's set")
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)  # noqa: E731
    dw1 = e(H1, int(num_nodes) * od)
    small = e(H2 * H1 + H2 + C * H2 + C + H1)
    dy = e(y.size(0), od) if need_dy else None
    ws = e(max(plan["backward_workspace_floats"], 1))
    with torch.cuda.device(dev):
        _check(_launch("readout_batched_backward", y,
                       lambda: lib.gnc_readout_batched_backward_f32(
                           g.data_ptr(), y.data_ptr(), gp.data_ptr() if gp is not None else None, G, int(num_nodes), od, y.size(0),
                           w1.data_ptr(), _ld(w1), H1, w2.data_ptr(), _ld(w2), H2, w3.data_ptr(), _ld(w3), C, h1.data_ptr(),
                           h2.data_ptr(), dw1.data_ptr(), small.data_ptr(), dy.data_ptr() if dy is not None else None, ws.data_ptr(),
                           ws.numel(), _stream(y)),
                       4.0 * G * w1.numel()), "gnc_readout_batched_backward_f32")
    dw2, db2, dw3, db3, db1 = small.split([H2 * H1, H2, C * H2, C, H1])
    return dy, dw1, db1, dw2.view(H2, H1), db2, dw3.view(C, H2), db3


# --------------------------------------------------------------------------- K17: global pooling read-out
POOL_SUM, POOL_MEAN, POOL_MAX = 1, 2, 4
POOL_MODES = {"sum": POOL_SUM, "mean": POOL_MEAN, "max": POOL_MAX, "hybrid": POOL_SUM | POOL_MEAN | POOL_MAX}


def graph_pool_plan(rows: int, width: int, num_graphs: int) -> dict | None:
    """The library's decision for pooling ``num_graphs`` graphs out of ``rows`` rows of ``width`` columns (host only, no GPU
    needed): None outside the served set, otherwise ``chunk_rows`` (the chunk length of the fixed summation order), ``split`` (0:
    one workgroup per graph and column tile; 1: few large graphs, one workgroup per chunk and a merge launch), the workgroup's
    tiling and ``workspace_floats``."""
    plan = GraphPoolPlan()
    if not load_library().gnc_graph_pool_plan(int(rows), int(width), int(num_graphs), ctypes.byref(plan)):
        return None
    return {name: int(getattr(plan, name)) for name, _ in GraphPoolPlan._fields_}


def _pool_graph_ptr(graph_ptr: torch.Tensor, dev) -> torch.Tensor:
    if graph_ptr.dtype != torch.int64 or graph_ptr.device != dev or graph_ptr.dim() != 1 or graph_ptr.numel() < 2:
        raise ValueError("graph_pool: graph_ptr must be int64 [num_graphs + 1] (num_graphs >= 1) on the device of y")
    return graph_ptr.contiguous()


def graph_pool_forward(y: torch.Tensor, graph_ptr: torch.Tensor, modes: int):
    """One pass over ``y`` [rows, C] (float32): for the graphs ``graph_ptr`` (DEVICE int64 [G + 1], never read on the host) names,
    the outputs the ``POOL_*`` bits of ``modes`` ask for.  Returns ``(out, argmax)``: ``out`` [G, k C] holds the wanted blocks in
    the order mean | max | sum (``hybrid``'s layout), ``argmax`` int32 [G, C] row indices into ``y`` (None without ``POOL_MAX``).
    An empty graph pools to +0.0 / argmax -1; rows outside the graphs are ignored."""
    lib = load_library()
    _require_cuda(y, graph_ptr)
    y = _rowmajor(y).contiguous()
    dev, rows, C = y.device, y.size(0), y.size(1)
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    plan = graph_pool_plan(rows, C, G)
    if plan is None or not modes or modes & ~(POOL_SUM | POOL_MEAN | POOL_MAX):
        raise RuntimeError(f"graph_pool_forward: rows {rows} / width {C} / graphs {G} / modes {modes} outside the kernel's set")
    order = [m for m in (POOL_MEAN, POOL_MAX, POOL_SUM) if modes & m]
    out = torch.empty(G, len(order) * C, dtype=torch.float32, device=dev)
    block = {m: out[:, k * C:(k + 1) * C] for k, m in enumerate(order)}
    argmax = torch.empty(G, C, dtype=torch.int32, device=dev) if modes & POOL_MAX else None
    ws = torch.empty(max(plan["workspace_floats"], 1), dtype=torch.float32, device=dev)
    ptr = lambda m: block[m].data_ptr() if m in block else None  # noqa: E731
    with torch.cuda.device(dev):
        _check(_launch("graph_pool_forward", y,
                       lambda: lib.gnc_graph_pool_forward_f32(y.data_ptr(), rows, C, gp.data_ptr(), G, modes, ptr(POOL_SUM), ptr(POOL_MEAN),
                                                              ptr(POOL_MAX), argmax.data_ptr() if argmax is not None else None,
                                                              out.size(1), ws.data_ptr(), ws.numel(), _stream(y)),
                       float(rows * C)), "gnc_graph_pool_forward_f32")
    return out, argmax


def graph_pool_backward(grad: torch.Tensor, modes: int, argmax: torch.Tensor | None, graph_ptr: torch.Tensor, rows: int):
    """``dy`` [rows, C] of ``graph_pool_forward``: ``grad`` [G, k C] in the forward's block order (mean | max | sum).  Every row is
    written; rows of no graph get exact zeros."""
    lib = load_library()
    _require_cuda(grad, graph_ptr)
    grad = _rowmajor(grad).contiguous()
    dev = grad.device
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    order = [m for m in (POOL_MEAN, POOL_MAX, POOL_SUM) if modes & m]
    if not order or grad.size(0) != G or grad.size(1) % len(order):
        raise ValueError(f"graph_pool_backward: grad {tuple(grad.shape)} does not hold {len(order)} blocks for {G} graphs")
    C = grad.size(1) // len(order)
    if modes & POOL_MAX and (argmax is None or argmax.shape != (G, C) or argmax.dtype != torch.int32 or not argmax.is_contiguous()):
        raise ValueError("graph_pool_backward: argmax must be the forward's int32 [G, C]")
    if graph_pool_plan(rows, C, G) is None:
        raise RuntimeError(f"graph_pool_backward: rows {rows} / width {C} / graphs {G} outside the kernel's set")
    dy = torch.empty(int(rows), C, dtype=torch.float32, device=dev)
    block = {m: grad.data_ptr() + 4 * k * C for k, m in enumerate(order)}
    with torch.cuda.device(dev):
        _check(_launch("graph_pool_backward", grad,
                       lambda: lib.gnc_graph_pool_backward_f32(block.get(POOL_SUM), block.get(POOL_MEAN), block.get(POOL_MAX), grad.size(1),
                                                               argmax.data_ptr() if modes & POOL_MAX else None, gp.data_ptr(), G,
                                                               int(rows), C, dy.data_ptr(), _stream(grad)),
                       float(rows * C)), "gnc_graph_pool_backward_f32")
    return dy


# --------------------------------------------------------------------------- K19: attention read-out
def _attention_scores(scores: torch.Tensor, y: torch.Tensor, who: str) -> torch.Tensor:
    if scores.dtype != torch.float32 or scores.dim() != 1 or scores.size(0) != y.size(0) or scores.device != y.device:
        raise ValueError(f"{who}: scores must be float32 [rows] = [{y.size(0)}] on the device of y, got {scores.dtype} "
                         f"{tuple(scores.shape)} on {scores.device}")
    return scores.contiguous()


def graph_attention_pool_forward(y: torch.Tensor, scores: torch.Tensor, graph_ptr: torch.Tensor):
    """Softmax-weighted pooling (K19): for each graph ``graph_ptr`` (DEVICE int64 [G + 1], never read on the host) names, the
    softmax of its rows' ``scores`` [rows] and the column sums of ``y`` [rows, C] (float32) weighted by it.  Returns ``(out, saved)``:
    ``out`` [G, C]; ``saved`` [G, 2] = (max score, sum of exponentials) per graph, which is all the backward and
    ``graph_attention_weights`` need.  An empty graph pools to +0.0; rows outside the graphs are ignored."""
    lib = load_library()
    _require_cuda(y, graph_ptr)  # (scores on another device: the ValueError below)
    y = _rowmajor(y).contiguous()
    dev, rows, C = y.device, y.size(0), y.size(1)
    scores = _attention_scores(scores, y, "graph_attention_pool_forward")
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    floats = lib.gnc_graph_attention_pool_workspace_floats(rows, C, G)
    if floats < 0:
        raise RuntimeError(f"graph_attention_pool_forward: rows {rows} / width {C} / graphs {G} outside the kernel's set")
    out = torch.empty(G, C, dtype=torch.float32, device=dev)
    saved = torch.empty(G, 2, dtype=torch.float32, device=dev)
    ws = torch.empty(max(floats, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("graph_attention_pool_forward", y,
                       lambda: lib.gnc_graph_attention_pool_forward_f32(y.data_ptr(), scores.data_ptr(), rows, C, gp.data_ptr(), G,
                                                                        out.data_ptr(), C, saved.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                        _stream(y)),
                       float(rows * (C + 1))), "gnc_graph_attention_pool_forward_f32")
    return out, saved


def graph_attention_pool_backward(grad: torch.Tensor, y: torch.Tensor, scores: torch.Tensor, out: torch.Tensor, saved: torch.Tensor,
                                  graph_ptr: torch.Tensor, need_dy: bool = True, need_ds: bool = True):
    """``(dy [rows, C], ds [rows])`` of ``graph_attention_pool_forward`` from ``grad`` [G, C] and the forward's ``out`` / ``saved``;
    an unwanted one is None and costs nothing.  Every row is written; rows of no graph get exact zeros."""
    lib = load_library()
    _require_cuda(grad, y, out, saved, graph_ptr)
    grad, y = _rowmajor(grad), _rowmajor(y).contiguous()
    dev, rows, C = y.device, y.size(0), y.size(1)
    scores = _attention_scores(scores, y, "graph_attention_pool_backward")
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    out = _rowmajor(out)
    if grad.shape != (G, C) or out.shape != (G, C) or saved.shape != (G, 2) or saved.dtype != torch.float32 or not saved.is_contiguous():
        raise ValueError(f"graph_attention_pool_backward: grad {tuple(grad.shape)} / out {tuple(out.shape)} / saved {tuple(saved.shape)} "
                         f"are not the forward's [{G}, {C}] / [{G}, {C}] / [{G}, 2]")
    if lib.gnc_graph_attention_pool_workspace_floats(rows, C, G) < 0:
        raise RuntimeError(f"graph_attention_pool_backward: rows {rows} / width {C} / graphs {G} outside the kernel's set")
    if not (need_dy or need_ds):
        return None, None
    dy = torch.empty(rows, C, dtype=torch.float32, device=dev) if need_dy else None
    ds = torch.empty(rows, dtype=torch.float32, device=dev) if need_ds else None
    with torch.cuda.device(dev):
        _check(_launch("graph_attention_pool_backward", grad,
                       lambda: lib.gnc_graph_attention_pool_backward_f32(grad.data_ptr(), _ld(grad), y.data_ptr(), scores.data_ptr(),
                                                                         out.data_ptr(), _ld(out), saved.data_ptr(), gp.data_ptr(), G,
                                                                         rows, C, dy.data_ptr() if need_dy else None,
                                                                         ds.data_ptr() if need_ds else None, _stream(grad)),
                       float(rows * (C + 1))), "gnc_graph_attention_pool_backward_f32")
    return dy, ds


def graph_attention_weights(scores: torch.Tensor, saved: torch.Tensor, graph_ptr: torch.Tensor) -> torch.Tensor:
    """The softmax weights ``alpha`` [rows] behind ``graph_attention_pool_forward`` (one small launch from its ``saved``): they sum
    to one over each non-empty graph; rows of no graph get +0.0."""
    lib = load_library()
    _require_cuda(scores, saved, graph_ptr)
    if scores.dtype != torch.float32 or scores.dim() != 1:
        raise ValueError(f"graph_attention_weights: scores must be float32 [rows], got {scores.dtype} {tuple(scores.shape)}")
    scores = scores.contiguous()
    dev, rows = scores.device, scores.size(0)
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    if saved.shape != (G, 2) or saved.dtype != torch.float32 or saved.device != dev or not saved.is_contiguous():
        raise ValueError(f"graph_attention_weights: saved must be the forward's float32 [{G}, 2]")
    alpha = torch.empty(rows, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("graph_attention_weights", scores,
                       lambda: lib.gnc_graph_attention_weights_f32(scores.data_ptr(), saved.data_ptr(), gp.data_ptr(), G, rows,
                                                                   alpha.data_ptr(), _stream(scores)),
                       float(rows)), "gnc_graph_attention_weights_f32")
    return alpha


# --------------------------------------------------------------------------- K20: top-K node pooling
def topk_keep_count(ratio: float, n: int) -> int:
    """Rows a graph of ``n`` rows keeps: ``min(n, max(1, math.ceil(ratio * n)))``, 0 for an empty graph (the kernel's rule)."""
    return min(int(n), max(1, math.ceil(float(ratio) * int(n)))) if n > 0 else 0


def _check_ratio(ratio, who: str) -> float:
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"{who}: ratio must be a number in (0, 1], got {ratio!r}")
    return float(ratio)


def topk_pool_select(scores: torch.Tensor, graph_ptr: torch.Tensor, ratio: float, padded: bool = False):
    """Per graph of ``graph_ptr`` (DEVICE int64 [G + 1], never read on the host), the ``k = min(n, max(1, ceil(ratio n)))`` rows
    with the best ``scores`` [rows] (float32): larger first, ``-0.0 == +0.0``, NaN below ``-inf``, ties by lower row.  Returns
    ``(new_id, kept, graph_ptr_out, counts)``, all on the device and allocated at their upper bounds: ``new_id`` int32 [rows] (-1 =
    dropped), ``kept`` int32 [rows] of which the first N' hold the survivors' old ids in ascending order, ``graph_ptr_out`` int64
    [G + 1], ``counts`` int64 [2] whose first entry is N' (the second is ``topk_pool_filter_edges``'s E').  No host
    synchronisation here: the caller reads ``counts`` back ONCE per pooling layer and narrows with views.

    ``padded=True`` (``gnc_topk_pool_select_padded_f32``, the same launches): ``kept[N':]`` holds -1 as well, so every entry of every
    result is defined and nobody has to read ``counts``."""
    lib = load_library()
    ratio = _check_ratio(ratio, "topk_pool_select")
    _require_cuda(scores, graph_ptr)
    if scores.dtype != torch.float32 or scores.dim() != 1:
        raise ValueError(f"topk_pool_select: scores must be float32 [rows], got {scores.dtype} {tuple(scores.shape)}")
    scores = scores.contiguous()
    dev, rows = scores.device, scores.size(0)
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    new_id = torch.empty(rows, dtype=torch.int32, device=dev)
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    gp_out = torch.empty(G + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    name = "gnc_topk_pool_select_padded_f32" if padded else "gnc_topk_pool_select_f32"
    fn = getattr(lib, name)
    with torch.cuda.device(dev):
        _check(_launch("topk_pool_select", scores,
                       lambda: fn(scores.data_ptr(), gp.data_ptr(), G, rows, ratio, new_id.data_ptr(), kept.data_ptr(), gp_out.data_ptr(),
                                  counts.data_ptr(), _stream(scores)),
                       float(rows)), name)
    return new_id, kept, gp_out, counts


def topk_pool_filter_edges(src_sorted: torch.Tensor, dst_sorted: torch.Tensor, rowptr: torch.Tensor, new_id: torch.Tensor,
                           kept: torch.Tensor, counts: torch.Tensor, padded: bool = False):
    """Stream compaction of a destination-sorted edge list (int32 [E] each, ``rowptr`` int32 [rows + 1]) to the edges whose two
    endpoints ``topk_pool_select`` kept, renumbered; the order is kept, so the result is still destination-sorted.  Returns
    ``(src, dst, kept_edges, edge_new_id, rowptr_out)`` at their upper bounds (E, E, E, E, rows + 1): the first E' entries of the
    first three and the first N' + 1 of ``rowptr_out`` are written, ``edge_new_id`` [E] holds -1 for a dropped edge; ``counts[1]``
    receives E'.  No host synchronisation here (see ``topk_pool_select``).

    ``padded=True`` (``gnc_topk_pool_filter_edges_padded``, the same launches, behind the padded select): all E entries of ``src`` /
    ``dst`` / ``kept_edges`` and all rows + 1 of ``rowptr_out`` are written - behind E' the evenly spread self-loops of the slack
    rows ``[N', rows)`` and ``kept_edges = -1``, ``rowptr_out[rows] = E`` - so the results describe a destination-sorted graph of
    ``rows`` nodes and E edges whatever the counts are."""
    lib = load_library()
    _require_cuda(src_sorted, dst_sorted, rowptr, new_id, kept, counts)
    rows, E = new_id.numel(), src_sorted.numel()
    for name, t, n in (("src_sorted", src_sorted, E), ("dst_sorted", dst_sorted, E), ("rowptr", rowptr, rows + 1), ("new_id", new_id, rows),
                       ("kept", kept, rows)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"topk_pool_filter_edges: {name} must be contiguous int32 [{n}], got {t.dtype} {tuple(t.shape)}")
    if counts.dtype != torch.int64 or counts.numel() != 2 or not counts.is_contiguous():
        raise ValueError("topk_pool_filter_edges: counts must be the select's int64 [2]")
    dev = new_id.device
    src, dst, kept_edges, edge_new_id = (torch.empty(E, dtype=torch.int32, device=dev) for _ in range(4))
    rowptr_out = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    need = lib.gnc_topk_pool_edge_workspace_ints(E)
    if need < 0:
        raise RuntimeError(f"topk_pool_filter_edges: {E} edges outside the kernel's set")
    ws = torch.empty(max(need, 1), dtype=torch.int32, device=dev)
    if padded and rows == 0:
        # no row a slack edge could loop on, so the library would launch nothing: the empty layout, written here.  No edge is
        # kept (E' = 0, every id -1) and the one row pointer is 0; an edge list over no rows does not exist, so with E > 0 (only
        # out-of-range endpoints: the source topology's flags are set) ``src`` / ``dst`` are zeros that nobody may index with.
        for t in (src, dst):
            t.zero_()
        for t in (kept_edges, edge_new_id):
            t.fill_(-1)
        rowptr_out.zero_()
        counts[1:].zero_()
        return src, dst, kept_edges, edge_new_id, rowptr_out
    name = "gnc_topk_pool_filter_edges_padded" if padded else "gnc_topk_pool_filter_edges"
    fn = getattr(lib, name)
    with torch.cuda.device(dev):
        _check(_launch("topk_pool_filter_edges", new_id,
                       lambda: fn(src_sorted.data_ptr(), dst_sorted.data_ptr(), rowptr.data_ptr(), E, rows, new_id.data_ptr(),
                                  kept.data_ptr(), counts.data_ptr(), src.data_ptr(), dst.data_ptr(), kept_edges.data_ptr(),
                                  edge_new_id.data_ptr(), rowptr_out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(new_id)),
                       float(E)), name)
    return src, dst, kept_edges, edge_new_id, rowptr_out


def topk_pool_rows_forward(x: torch.Tensor, kept: torch.Tensor, scores: torch.Tensor | None = None,
                           out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[i] = x[kept[i]] * tanh(scores[kept[i]])`` (``scores`` None: no gate, the bits of ``x``): ``x`` [rows, C] float32 with
    unit column stride (a row stride above C is taken as it is), ``kept`` int32 [n_out] - a HOST-known length, i.e. the narrowed
    view of ``topk_pool_select``'s - and ``scores`` float32 [rows]."""
    lib = load_library()
    _require_cuda(x, kept, scores, out)
    x = _rowmajor(x)
    rows, C, n_out = x.size(0), x.size(1), kept.numel()
    if kept.dtype != torch.int32 or kept.dim() != 1 or not kept.is_contiguous() or n_out > rows:
        raise ValueError(f"topk_pool_rows_forward: kept must be contiguous int32 [<= {rows}], got {kept.dtype} {tuple(kept.shape)}")
    if scores is not None:
        scores = _attention_scores(scores, x, "topk_pool_rows_forward")
    if out is None:
        out = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (n_out, C) or (C and out.stride(1) != 1):
        raise ValueError(f"topk_pool_rows_forward: out must be float32 [{n_out}, {C}] with unit column stride")
    if C == 0 or n_out == 0:
        return out
    with torch.cuda.device(x.device):
        _check(_launch("topk_pool_rows_forward", x,
                       lambda: lib.gnc_topk_pool_rows_forward_f32(x.data_ptr(), _ld(x), rows, C, kept.data_ptr(), n_out,
                                                                  scores.data_ptr() if scores is not None else None, out.data_ptr(),
                                                                  _ld(out), _stream(x)),
                       float(n_out * C)), "gnc_topk_pool_rows_forward_f32")
    return out


def topk_pool_rows_backward(grad: torch.Tensor, new_id: torch.Tensor, x: torch.Tensor | None = None, scores: torch.Tensor | None = None,
                            need_dx: bool = True, need_ds: bool = True, dx: torch.Tensor | None = None, ds: torch.Tensor | None = None):
    """``(dx [rows, C], ds [rows])`` of ``topk_pool_rows_forward`` from ``grad`` [n_out, C] and ``new_id`` int32 [rows]: with
    ``j = new_id[r]``, ``dx[r] = tanh(s_r) grad[j]`` and ``ds[r] = (1 - tanh(s_r)^2) sum_c grad[j, c] x[r, c]``; a dropped row gets
    exact +0.0.  Every row is written exactly once (no memset, no atomics).  Without ``scores``: the ungated form, ``dx`` alone.
    An unwanted gradient is None and costs nothing."""
    lib = load_library()
    _require_cuda(grad, new_id, x, scores, dx, ds)
    grad = _rowmajor(grad)
    n_out, C, rows = grad.size(0), grad.size(1), new_id.numel()
    if new_id.dtype != torch.int32 or new_id.dim() != 1 or not new_id.is_contiguous():
        raise ValueError(f"topk_pool_rows_backward: new_id must be contiguous int32 [rows], got {new_id.dtype} {tuple(new_id.shape)}")
    need_ds = need_ds and scores is not None
    if not (need_dx or need_ds):
        return None, None
    if need_ds:
        x = _rowmajor(x)
        if tuple(x.shape) != (rows, C):
            raise ValueError(f"topk_pool_rows_backward: x {tuple(x.shape)} is not the forward's [{rows}, {C}]")
    if scores is not None:
        if scores.dtype != torch.float32 or scores.dim() != 1 or scores.numel() != rows:
            raise ValueError(f"topk_pool_rows_backward: scores must be float32 [{rows}]")
        scores = scores.contiguous()
    dev = grad.device
    if need_dx and dx is None:
        dx = torch.empty(rows, C, dtype=torch.float32, device=dev)
    if need_ds and ds is None:
        ds = torch.empty(rows, dtype=torch.float32, device=dev)
    if need_dx and (dx.dtype != torch.float32 or tuple(dx.shape) != (rows, C) or (C and dx.stride(1) != 1)):
        raise ValueError(f"topk_pool_rows_backward: dx must be float32 [{rows}, {C}] with unit column stride")
    if need_ds and (ds.dtype != torch.float32 or tuple(ds.shape) != (rows,) or not ds.is_contiguous()):
        raise ValueError(f"topk_pool_rows_backward: ds must be contiguous float32 [{rows}]")
    if rows == 0:
        return (dx if need_dx else None), (ds if need_ds else None)
    if C == 0:
        if need_ds:
            ds.zero_()
        return (dx if need_dx else None), (ds if need_ds else None)
    with torch.cuda.device(dev):
        _check(_launch("topk_pool_rows_backward", grad,
                       lambda: lib.gnc_topk_pool_rows_backward_f32(grad.data_ptr(), _ld(grad), n_out, x.data_ptr() if need_ds else None,
                                                                   _ld(x) if need_ds else C,
                                                                   scores.data_ptr() if scores is not None else None,
                                                                   new_id.data_ptr(), rows, C, dx.data_ptr() if need_dx else None,
                                                                   _ld(dx) if need_dx else C, ds.data_ptr() if need_ds else None,
                                                                   _stream(grad)),
                       float(rows * C)), "gnc_topk_pool_rows_backward_f32")
    return (dx if need_dx else None), (ds if need_ds else None)


# --------------------------------------------------------------------------- K16: split-K first Linear of a wide-input MLP
def wide_linear_plan_of(desc: MlpDesc) -> dict | None:
    """The library's decision for running the first Linear of this fused-MLP description on K16 (host only, no GPU needed): None
    when the description stays on the row-tiled kernels, otherwise the split of K in the forward, the row ranges of the
    backward and the workspace sizes in floats."""
    plan = WideLinearPlan()
    if not load_library().gnc_wide_linear_supported(ctypes.byref(desc), ctypes.byref(plan)):
        return None
    return {name: int(getattr(plan, name)) for name, _ in WideLinearPlan._fields_}


def wide_linear_serves(segments, weights, biases, ln, activation: str, residual, rows: int | None) -> bool:
    """Does K16 take the first Linear of this fused-MLP call?  The structure of the call is looked at here (one table in row
    order in front of at least two Linears - everything a description cannot say otherwise), every size by the library's own
    decision."""
    if len(segments) != 1 or segments[0][1] is not None or residual is not None or len(weights) < 2 or activation not in ACTIVATIONS:
        return False
    table, w0 = segments[0][0], weights[0]
    if table.dim() != 2 or table.dtype != torch.float32 or not table.is_cuda:
        return False
    rows = _rows_of(segments, rows)
    lib = load_library()
    if rows != table.size(0) or lib.gnc_wide_linear_workspace_floats(rows, w0.size(1), w0.size(0), 0) < 0:
        return False  # (the size question alone first: it needs no description, and no call of the graph model gets past it)
    table, w0 = _rowmajor(table), _rowmajor(w0.detach())
    desc = make_mlp_desc([(table, None, table.size(1), SEG_MATMUL, 0)], [w0] + [w.detach() for w in weights[1:]], list(biases), ln,
                         activation, 0.0, None, table, rows)
    return lib.gnc_wide_linear_supported(ctypes.byref(desc), None) == 1


def wide_linear_forward(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, activation: str = "ReLU", act_param: float = 0.0,
                        want_z: bool = False):
    """(a0, z0): a0 = act(x w^T + bias) [rows, H] on K16 (gnc_wide_linear_forward_f32: partial products per slice of K, then the
    tail that sums them in ascending order); z0 = the pre-activation when ``want_z`` (the backward of an activation other than
    ReLU reads it), else None.  ``x`` and ``w`` are read where they lie: any row pitch, any alignment."""
    lib = load_library()
    _require_cuda(x, w, bias)
    x, w = _rowmajor(x), _rowmajor(w.detach())
    rows, K, H, dev = x.size(0), x.size(1), w.size(0), x.device
    if w.size(1) != K:
        raise ValueError(f"wide_linear_forward: x has {K} columns, the weight {w.size(1)}")
    n_ws = lib.gnc_wide_linear_workspace_floats(rows, K, H, 0)
    if n_ws < 0:
        raise RuntimeError("wide_linear_forward: shape outside the kernel's set (ask wide_linear_serves first)")
    a0 = torch.empty(rows, H, dtype=torch.float32, device=dev)
    z0 = torch.empty(rows, H, dtype=torch.float32, device=dev) if want_z else None
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    b = bias.detach().contiguous() if bias is not None else None
    with torch.cuda.device(dev):
        _check(_launch(f"wide_linear_forward_in{K}_h{H}", x,
                       lambda: lib.gnc_wide_linear_forward_f32(
                           x.data_ptr(), _ld(x), rows, K, w.data_ptr(), _ld(w), b.data_ptr() if b is not None else None, H,
                           ACTIVATIONS[activation], float(act_param), a0.data_ptr(), H, z0.data_ptr() if want_z else None, H,
                           ws.data_ptr(), ws.numel(), _stream(x)), 2.0 * rows * K * H), "gnc_wide_linear_forward_f32")
    return a0, z0


def wide_linear_backward(grad_a0: torch.Tensor, az: torch.Tensor, x: torch.Tensor, activation: str = "ReLU", act_param: float = 0.0):
    """(dW [H, K], db [H]) of ``wide_linear_forward`` from the gradient of its output: ``az`` is the forward's a0 for ReLU and its
    z0 for every other activation.  The gradient of ``x`` is not formed."""
    lib = load_library()
    _require_cuda(grad_a0, az, x)
    g, az, x = _rowmajor(grad_a0), _rowmajor(az), _rowmajor(x)
    rows, K, H, dev = x.size(0), x.size(1), g.size(1), x.device
    n_ws = lib.gnc_wide_linear_workspace_floats(rows, K, H, 1)
    if n_ws < 0 or g.size(0) != rows or az.shape != g.shape:
        raise RuntimeError("wide_linear_backward: shape outside the kernel's set or operands that do not match")
    dw = torch.empty(H, K, dtype=torch.float32, device=dev)
    db = torch.empty(H, dtype=torch.float32, device=dev)
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev) if n_ws > 0 else None
    with torch.cuda.device(dev):
        _check(_launch(f"wide_linear_backward_in{K}_h{H}", x,
                       lambda: lib.gnc_wide_linear_backward_f32(
                           g.data_ptr(), _ld(g), az.data_ptr(), _ld(az), x.data_ptr(), _ld(x), rows, K, H, ACTIVATIONS[activation],
                           float(act_param), dw.data_ptr(), db.data_ptr(), ws.data_ptr() if ws is not None else None, n_ws,
                           _stream(x)), 2.0 * rows * K * H), "gnc_wide_linear_backward_f32")
    return dw, db


# --------------------------------------------------------------------------- K24: k-nearest-neighbour edges
KNN_MAX_K = 16
KNN_MAX_DIM = 16
KNN_FEW_CANDIDATES = 1  # GNC_KNN_FEW_CANDIDATES: a graph had fewer candidates than k (its unfillable slots hold -1)
KNN_NAN_DISTANCE = 2    # GNC_KNN_NAN_DISTANCE


def knn_graph_constants() -> tuple[int, int]:
    """``(query rows of a workgroup, unroll of the candidate loop)`` of the kNN kernel: the sizes at which it changes path (it
    stages nothing in LDS)."""
    q, t = c_int32(0), c_int32(0)
    load_library().gnc_knn_graph_constants(ctypes.byref(q), ctypes.byref(t))
    return int(q.value), int(t.value)


def _knn_feat(feat: torch.Tensor, k, who: str) -> torch.Tensor:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"{who}: k must be an integer in [1, {KNN_MAX_K}], got {k!r}")
    if feat.dtype != torch.float32:
        raise NotImplementedError(f"{who}: features must be float32, got {feat.dtype}")
    if not 1 <= feat.size(-1) <= KNN_MAX_DIM:
        raise NotImplementedError(f"{who}: {feat.size(-1)} feature columns; the bit-exact kernel serves 1 .. {KNN_MAX_DIM}")
    return feat


def knn_graph(feat: torch.Tensor, graph_ptr: torch.Tensor, k: int, loop: bool = False, return_dist: bool = False):
    """``gnc_knn_graph_f32``: the ``k`` nearest rows of ``feat`` [N, D] (float32, unit column stride, any row stride - never copied
    then) inside each graph of ``graph_ptr`` (DEVICE int64 [G + 1], never read on the host).  Returns ``(edge_index, dist, status)``:
    ``edge_index`` int64 [2, k N] (slot ``v k + j``: sender = the j-th nearest of ``v``, receiver = ``v``; global ids), ``dist``
    float32 [k N] or None, ``status`` int32 [1] on the device (``KNN_FEW_CANDIDATES`` / ``KNN_NAN_DISTANCE`` bits).  One launch, no
    host synchronisation."""
    lib = load_library()
    if feat.dim() != 2:
        raise ValueError(f"knn_graph: feat must be [N, D], got {tuple(feat.shape)}")
    feat = _rowmajor(_knn_feat(feat, k, "knn_graph"))
    _require_cuda(feat, graph_ptr)
    dev, N, D = feat.device, feat.size(0), feat.size(1)
    gp = _pool_graph_ptr(graph_ptr, dev)
    G = gp.numel() - 1
    edge_index = torch.empty(2, k * N, dtype=torch.int64, device=dev)
    dist = torch.empty(k * N, dtype=torch.float32, device=dev) if return_dist else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("knn_graph", feat,
                       lambda: lib.gnc_knn_graph_f32(feat.data_ptr(), _ld(feat), D, gp.data_ptr(), G, N, k, int(bool(loop)),
                                                     edge_index.data_ptr(), k * N, dist.data_ptr() if return_dist else None,
                                                     status.data_ptr(), _stream(feat)),
                       3.0 * D * N * N / max(G, 1)), "gnc_knn_graph_f32")
    return edge_index, dist, status


def knn_graph_padded(feat: torch.Tensor, counts: torch.Tensor, k: int, loop: bool = False, return_dist: bool = False):
    """``gnc_knn_graph_padded_f32`` over the layout of ``rag_build_batched``: ``feat`` [B, node_capacity, D] (float32, contiguous
    rows), the node count of image ``b`` read on the device from ``counts[b, 0]`` (int32 [B] or [B, S]).  Returns ``(edge_index,
    dist, status)``: ``edge_index`` int64 [B, 2, k node_capacity] with ids local to each image and -1 behind ``k n_b``, ``dist``
    float32 [B, k node_capacity] (+inf there) or None, ``status`` as ``knn_graph``'s.  One launch, no host synchronisation."""
    lib = load_library()
    if feat.dim() != 3:
        raise ValueError(f"knn_graph_padded: feat must be [B, node_capacity, D], got {tuple(feat.shape)}")
    feat = _knn_feat(feat, k, "knn_graph_padded").contiguous()
    _require_cuda(feat, counts)
    dev = feat.device
    B, cap, D = feat.shape
    if counts.dtype != torch.int32 or counts.device != dev or counts.dim() not in (1, 2) or counts.size(0) != B:
        raise ValueError(f"knn_graph_padded: counts must be int32 [{B}] or [{B}, S] on the device of feat")
    counts = counts.contiguous()
    stride = counts.size(1) if counts.dim() == 2 else 1
    if cap < 1 or stride < 1:
        raise ValueError("knn_graph_padded: empty capacity")
    edge_index = torch.empty(B, 2, k * cap, dtype=torch.int64, device=dev)
    dist = torch.empty(B, k * cap, dtype=torch.float32, device=dev) if return_dist else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("knn_graph_padded", feat,
                       lambda: lib.gnc_knn_graph_padded_f32(feat.data_ptr(), D, D, counts.data_ptr(), stride, B, cap, k, int(bool(loop)),
                                                            edge_index.data_ptr(), dist.data_ptr() if return_dist else None,
                                                            status.data_ptr(), _stream(feat)),
                       3.0 * D * B * cap * cap), "gnc_knn_graph_padded_f32")
    return edge_index, dist, status


def u8_hwc_to_f32_chw(img: torch.Tensor) -> torch.Tensor:
    """torchvision's ``ToTensor`` for a batch of uint8 images [B, H, W, C] on the device: float32 [B, C, H, W] = value / 255 (a true
    division: bit for bit ``img.permute(0, 3, 1, 2).float().div(255)``), one launch."""
    _require_cuda(img)
    if img.dtype != torch.uint8 or img.dim() != 4:
        raise TypeError(f"u8_hwc_to_f32_chw: expected uint8 [B, H, W, C], got {img.dtype} {tuple(img.shape)}")
    img = img.contiguous()
    B, H, W, C = img.shape
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _check(_launch("u8_hwc_to_f32_chw", img,
                       lambda: load_library().gnc_u8_hwc_to_f32_chw(img.data_ptr(), B, H, W, C, out.data_ptr(), _stream(img))),
               "gnc_u8_hwc_to_f32_chw")
    return out


# --------------------------------------------------------------------------- feed of a captured ragged mini-batch
PAD_BATCH_MAX_GRAPHS = 64  # GNC_PAD_BATCH_MAX_GRAPHS: the offsets and labels travel in the kernel arguments


def ragged_batch_layout(node_capacity: int, edge_capacity: int) -> tuple[int, int]:
    """``(rows, dummies)`` of the buffers a captured ragged-batch step runs on: ``dummies = max(1, ceil(edge_capacity / 8))`` zero
    nodes behind the ``node_capacity`` node slots (the unused edge slots are their self-loops, at most 8 each)."""
    dummies = max(1, (int(edge_capacity) + 7) // 8)
    return int(node_capacity) + dummies, dummies


def pad_graph_batch_supported(num_graphs: int, num_nodes: int, num_edges: int, node_capacity: int, edge_capacity: int,
                              fx: int = 3, fp: int = 2) -> bool:
    return bool(load_library().gnc_pad_graph_batch_supported(int(num_graphs), int(num_nodes), int(num_edges), int(node_capacity),
                                                             int(edge_capacity), int(fx), int(fp)))


def _host_i64(values, count: int, what: str):
    vals = [int(v) for v in (values.tolist() if isinstance(values, torch.Tensor) else values)]
    if len(vals) != count:
        raise ValueError(f"pad_graph_batch: {what} must hold {count} entries, got {len(vals)}")
    return (c_int64 * count)(*vals)


def pad_graph_batch(x: torch.Tensor, pos: torch.Tensor, edge_index: torch.Tensor, graph_ptr, edge_ptr, labels, node_capacity: int,
                    edge_capacity: int, x_buf: torch.Tensor, pos_buf: torch.Tensor, ei_buf: torch.Tensor, graph_ptr_buf: torch.Tensor,
                    labels_buf: torch.Tensor | None, flag: torch.Tensor) -> None:
    """ONE launch (gnc_pad_graph_batch) that writes the input buffers of a captured ragged-batch step from a collated batch on the
    device: ``x`` [N, Fx] / ``pos`` [N, Fp] float32, ``edge_index`` [2, E] int64 with shifted ids; ``graph_ptr`` / ``edge_ptr``
    [G + 1] and ``labels`` [G] (None: not written) are HOST values and travel in the kernel arguments.  Buffers: ``x_buf`` /
    ``pos_buf`` [rows, F] with ``rows`` from ``ragged_batch_layout`` (rows behind ``node_capacity`` stay untouched), ``ei_buf``
    [2, edge_capacity] int64, ``graph_ptr_buf`` int64 [G + 1], ``labels_buf`` int64 [G], ``flag`` int32 [1] (sticky: set when an
    edge leaves its graph's node range, never cleared here).  More than ``PAD_BATCH_MAX_GRAPHS`` graphs or a batch above the
    capacities raises ValueError before any launch."""
    _require_cuda(x, pos, edge_index, x_buf, pos_buf, ei_buf, graph_ptr_buf, labels_buf, flag)
    if x.dtype != torch.float32 or pos.dtype != torch.float32 or edge_index.dtype != torch.int64:
        raise TypeError("pad_graph_batch: float32 x / pos and int64 edge_index expected")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    n, e = int(x.size(0)), int(edge_index.size(1))
    if pos.size(0) != n:
        raise ValueError("pad_graph_batch: x and pos disagree on the node count")
    fx, fp = x[0].numel() if n else x_buf[0].numel(), pos[0].numel() if n else pos_buf[0].numel()
    G = int(graph_ptr_buf.numel()) - 1
    M, C = int(node_capacity), int(edge_capacity)
    if not pad_graph_batch_supported(G, n, e, M, C, fx, fp):
        raise ValueError(f"pad_graph_batch: {G} graphs / {n} nodes / {e} edges do not fit {PAD_BATCH_MAX_GRAPHS} graphs / "
                         f"{M} nodes / {C} edges")
    rows, _ = ragged_batch_layout(M, C)
    for buf, f, what in ((x_buf, fx, "x_buf"), (pos_buf, fp, "pos_buf")):
        if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.size(0) < rows or buf[0].numel() != f:
            raise ValueError(f"pad_graph_batch: {what} must be contiguous float32 [>= {rows}, {f}]")
    if ei_buf.dtype != torch.int64 or not ei_buf.is_contiguous() or tuple(ei_buf.shape) != (2, C):
        raise ValueError(f"pad_graph_batch: ei_buf must be contiguous int64 [2, {C}]")
    if graph_ptr_buf.dtype != torch.int64 or not graph_ptr_buf.is_contiguous() or G < 1:
        raise ValueError("pad_graph_batch: graph_ptr_buf must be contiguous int64 [G + 1]")
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError("pad_graph_batch: flag must be one int32")
    if (labels is None) != (labels_buf is None):
        raise ValueError("pad_graph_batch: labels and labels_buf come together")
    if labels_buf is not None and (labels_buf.dtype != torch.int64 or not labels_buf.is_contiguous() or labels_buf.numel() != G):
        raise ValueError("pad_graph_batch: labels_buf must be contiguous int64 [G]")
    x, pos = x.contiguous(), pos.contiguous()
    if e and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    gp, ep = _host_i64(graph_ptr, G + 1, "graph_ptr"), _host_i64(edge_ptr, G + 1, "edge_ptr")
    lab = _host_i64(labels, G, "labels") if labels is not None else None
    with torch.cuda.device(x_buf.device):
        _check(_launch("pad_graph_batch", x_buf,
                       lambda: load_library().gnc_pad_graph_batch(
                           x.data_ptr(), fx, pos.data_ptr(), fp, edge_index.data_ptr(), max(int(edge_index.stride(0)), e), n, e, G,
                           gp, ep, lab, M, C, x_buf.data_ptr(), pos_buf.data_ptr(), ei_buf.data_ptr(), graph_ptr_buf.data_ptr(),
                           labels_buf.data_ptr() if labels_buf is not None else None, flag.data_ptr(), _stream(x_buf)),
                       4.0 * (x_buf.numel() + pos_buf.numel()) + 8.0 * ei_buf.numel()), "gnc_pad_graph_batch")


def dual_projection(x: torch.Tensor, wa: torch.Tensor, wb: torch.Tensor):
    """(x wa^T, x wb^T) over the same rows.  One launch for the small-batch projection shape (gnc_mlp_dual_projection_f32),
    two single-Linear launches otherwise."""
    lib = load_library()
    _require_cuda(x, wa, wb)
    x, wa, wb = _rowmajor(x), _rowmajor(wa.detach()), _rowmajor(wb.detach())
    rows = x.size(0)
    k, m = x.size(1), wa.size(0)
    small = 1 <= rows <= lib.gnc_mlp_small_batch_max_rows() and k == m == 128
    # a large batch at widths <= 64 (c3): the weights-resident kernel's dual instance - the rows are read once
    large = rows > lib.gnc_mlp_small_batch_max_rows() and k <= 64 and 32 < m <= 64 and m % 4 == 0 and _ld(x) % 4 == 0 \
        and x.data_ptr() % 16 == 0
    if ((small or large) and wa.shape == wb.shape and wa.size(1) == k and _ld(wa) == _ld(wb)
            and os.environ.get("GNC_NO_DUAL_PROJECTION") is None):
        oa = torch.empty(rows, m, dtype=torch.float32, device=x.device)
        ob = torch.empty(rows, m, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = _launch(f"mlp_fused_in{k}_h{m}_out{m}_L1x2", oa,
                         lambda: lib.gnc_mlp_dual_projection_f32(x.data_ptr(), _ld(x), rows, wa.data_ptr(), _ld(wa), wb.data_ptr(), _ld(wb),
                                                                 k, m, oa.data_ptr(), ob.data_ptr(), _ld(oa), _stream(x)),
                         2.0 * rows * 2 * k * m)
        if rc == 0:
            return oa, ob
    return mlp_forward([(x, None)], [wa], [None]), mlp_forward([(x, None)], [wb], [None])


def projection_t2(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, dn: int):
    """a W[:, :dn] + b W[:, dn:2 dn] with W [H, >= 2 dn] as nn.Linear holds it.  One launch on the transposed-read small-batch
    shape (gnc_mlp_projection_t2_f32); otherwise a projection launch over [a | b] with the transposed, stacked weight."""
    lib = load_library()
    _require_cuda(a, b, w)
    a, b, w = _rowmajor(a), _rowmajor(b), _rowmajor(w.detach())
    rows, h = a.size(0), w.size(0)
    if (1 <= rows <= lib.gnc_mlp_small_batch_max_rows() and h == dn == 128 and a.shape == b.shape == (rows, h) and w.size(1) >= 2 * dn
            and os.environ.get("GNC_NO_PROJECTION_T2") is None):
        out = torch.empty(rows, dn, dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            rc = _launch("mlp_fused_in256_h128_out128_L1t", out,
                         lambda: lib.gnc_mlp_projection_t2_f32(a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), rows, w.data_ptr(), _ld(w), h, dn,
                                                               out.data_ptr(), _ld(out), _stream(a)), 2.0 * rows * 2 * h * dn)
        if rc == 0:
            return out
    wt = torch.cat([w[:, :dn], w[:, dn:2 * dn]], dim=0).t().contiguous()  # [dn, 2h]
    return mlp_forward([(a, None), (b, None)], [wt], [None])


def small_batch_kernel_serves(segments, weights, biases, ln=None, activation: str = "ReLU", residual=None, rows=None,
                              modes=None) -> bool:
    """Would the small-batch (column-split) kernel run this ``mlp_forward`` call as its operands lie
    (gnc_mlp_small_batch_supported)?  The reference's one-graph-per-call regime is served by it."""
    lib = load_library()
    segs, w, b, res, rows, _ = _prepare_mlp(segments, weights, biases, residual, rows, modes, vector_rows=False)
    dummy = torch.empty(max(rows, 1), w[-1].size(0), device=segs[0][0].device)
    desc = make_mlp_desc(segs, w, b, ln, activation, 0.0, res, dummy, rows)
    return lib.gnc_mlp_small_batch_supported(ctypes.byref(desc)) == 0


# --------------------------------------------------------------------------- K8 backward
def _backward_desc(lib, segments, weights, biases, ln, activation, residual, rows, modes, saved_act):
    """The forward description of a K8 launch or query: ``(desc, segs, w, b, residual, rows, unpadded)``.  A small batch
    with saved activations is described as its operands lie first (``unpadded``, with them in ``desc.save_act``): its data
    kernel reads them in place, no padded copies of the reference's 3-column inputs / first-layer weights (two pad launches
    each); every other kernel gets rows of 16-B pieces."""
    def describe(vector_rows):
        segs, w, b, res, rows_, _ = _prepare_mlp(segments, weights, biases, residual, rows, modes, vector_rows=vector_rows)
        dummy = torch.empty(1, w[-1].size(0), device=segs[0][0].device)
        # (no residual: the backward never reads it)
        return make_mlp_desc(segs, w, b, ln, activation, 0.0, None, dummy, rows_), segs, w, b, res, rows_

    if saved_act and activation == "ReLU" and len(saved_act) == len(weights) - 1 and _rows_of(segments, rows) <= _small_batch_rows(lib):
        unpadded = describe(False)
        for l, a in enumerate(saved_act):
            unpadded[0].save_act[l] = a.data_ptr()
        if lib.gnc_mlp_backward_small_batch_supported(ctypes.byref(unpadded[0])) == 1:
            return (*unpadded, True)
    return (*describe(True), False)


def _residual_is_last_matmul(segs, residual, out_width: int) -> bool:
    """The residual is the last MATMUL segment handed to the kernel, row-ordered and as wide as the output: a kernel can
    fold its gradient (grad_out) into the dx of that segment."""
    if residual is None:
        return False
    table, index, width = [sg for sg in segs if sg[3] == SEG_MATMUL][-1][:3]
    return index is None and table.data_ptr() == residual.data_ptr() and width == out_width


# --------------------------------------------------------------------------- K8 backward
def mlp_backward_supported(segments, weights, biases, ln, activation, residual, rows, modes=None, saved_act=None) -> bool:
    """Shape query of the HIP backward kernel (ReLU, widths <= 64, 2..7 Linear layers ...).  With ``saved_act`` a small batch
    is asked about as its operands lie (its data kernel needs no padded copies, so the query makes none either)."""
    lib = load_library()
    if activation not in ACTIVATIONS or not (1 <= len(weights) <= GNC_MAX_LINEAR) or len(segments) > GNC_MAX_SEGMENTS:
        return False
    desc, *_, unpadded = _backward_desc(lib, segments, weights, biases, ln, activation, residual, rows, modes, saved_act)
    return unpadded or lib.gnc_mlp_backward_supported(ctypes.byref(desc)) == 0


def mlp_backward(segments, weights, biases, ln, grad_out: torch.Tensor | None, rows: int | None = None, modes=None,
                 need_dx: bool = True, residual: torch.Tensor | None = None, fused: bool = True, grad_gather=None,
                 saved_act=None, defer_ln_sums: bool = False):
    """Data path of the MLP backward (see include/gnc_hip.h, K8).  Returns a dict with
    ``act`` (inputs of Linear 1..L-1), ``dz`` (grads of every pre-activation, dz[-1] = pre-LayerNorm),
    ``dx`` ([rows, in_dim0] in weight-column order, or None) and ``yhat`` (or None).  Shapes of the fused kernel
    (``fused=True`` and gnc_mlp_backward_fused_rows() > 0) return ``dw`` / ``db`` (one per Linear; ``dw[0]`` covers the
    columns of the MATMUL segment) instead of ``act`` / ``dz[1:]``.

    ``grad_gather = (table [N, out_dim], index int32 [rows])``: the gradient of output row r is
    ``(grad_out[r] if grad_out is not None else 0) + table[index[r]]`` - the backward of a scatter-sum that consumed the
    output rows (models/GNN.py:99).  Kernels that honour it (gnc_mlp_backward_grad_gather_honoured) gather inside the
    launch; otherwise the rows are gathered here first (K2).  ``r["grad_out"]`` is the effective row-ordered gradient when
    it had to be materialised, else None.

    ``defer_ln_sums``: leave the per-worker LayerNorm partial sums unsummed in ``r["ln_part"]`` ([P, 2 * out_dim]: d beta |
    d gamma) for the caller to fold into its ``xty_multi`` launch (split path only).

    ``saved_act``: the list ``mlp_forward(save_act=...)`` filled for the same call; kernels that honour it
    (gnc_mlp_backward_saved_act_honoured) read the post-activations instead of recomputing them."""
    lib = load_library()
    bd = MlpBwdDesc()
    bd.fwd, segs, w, b, residual, rows, unpadded = _backward_desc(lib, segments, weights, biases, ln, "ReLU", residual, rows,
                                                                   modes, saved_act)
    dev = segs[0][0].device
    n_lin, out_w = len(w), w[-1].size(0)

    def empty(n, width):
        return torch.empty(n, width, dtype=torch.float32, device=dev)

    # which kernel: the fused data + weight-gradient one (per-wave partials of dW_l / db_l and of the LayerNorm sums instead of
    # the a_l / dz_l / y_hat tensors), or the split path (a data kernel that emits a_l and dz_l for gnc_xty_f32)
    frows = lib.gnc_mlp_backward_fused_rows(ctypes.byref(bd.fwd)) if fused else 0
    fused = frows > 0
    parts = [empty(frows, x.size(0) * x.size(1) + x.size(0)) for x in w] if fused else []
    for l, part in enumerate(parts):
        bd.dw_partial[l] = part.data_ptr()
    # ... reading the forward's saved post-activations, where that kernel has them as inputs
    if saved_act and len(saved_act) == n_lin - 1 and _saved_act_honoured(lib, bd.fwd, [a.data_ptr() for a in saved_act], need_dx, fused):
        bd.act_given = 1
        for l, a in enumerate(saved_act):
            bd.act[l] = a.data_ptr()
            bd.fwd.save_act[l] = a.data_ptr()  # the shape queries that only see the forward description learn of them this way
    # residual given: ask the kernel to fold its gradient (grad_out) into the dx of the segment it came from
    res_fold = _residual_is_last_matmul(segs, residual, out_w)
    bd.dx_add_grad_out = int(need_dx and res_fold and (fused or lib.gnc_mlp_backward_dx_add_honoured(ctypes.byref(bd.fwd)) == 1))
    gt = gi = None
    if grad_gather is not None:
        gt, gi = _vector_rows(_rowmajor(grad_gather[0])), grad_gather[1]
        bd.grad_gather, bd.ld_grad_gather = gt.data_ptr(), _ld(gt)
        bd.grad_gather_index, bd.grad_gather_rows = gi.data_ptr(), gt.size(0)
        # the residual's gradient is the EFFECTIVE output gradient: when the kernel cannot fold it into dx itself (the
        # residual went through a padded copy: width % 4 != 0), the caller adds it and needs the rows as a tensor
        caller_adds_residual = residual is not None and need_dx and not res_fold
        if caller_adds_residual or lib.gnc_mlp_backward_grad_gather_honoured(ctypes.byref(bd)) != 1:  # gather in front of the launch (K2)
            grad_out = gather_rows(gt, gi) if grad_out is None else gather_rows_add(gt, gi, _rowmajor(grad_out))
            bd.grad_gather = bd.grad_gather_index = None
            bd.ld_grad_gather = bd.grad_gather_rows = 0
            gt = gi = None
    # (the small-batch data kernel reads grad_out rows of any width where they lie: no padded copy of the decoder's [rows, 1])
    g = (_rowmajor(grad_out) if unpadded else _vector_rows(_rowmajor(grad_out))) if grad_out is not None else None
    if g is not None:
        bd.grad_out, bd.ld_grad_out = g.data_ptr(), _ld(g)
    g_eff = g if gt is None else None   # the effective output gradient as a tensor (None: part of it is gathered in the kernel)
    launch_ref = g if g is not None else gt
    g_sum = None
    if fused:
        if gt is not None and g is not None and bd.dx_add_grad_out:  # scratch for the summed rows (see gnc_hip.h, grad_sum)
            g_sum = empty(rows, out_w)
            bd.grad_sum, bd.ld_grad_sum = g_sum.data_ptr(), _ld(g_sum)
        act = None  # only dz_0 (gradient of gathered ADD segments) and dx are written
        dz = [empty(rows, w[0].size(0)) if len(segs) > 1 else None] + [None] * (n_lin - 1)
    else:
        act = list(saved_act) if bd.act_given else [empty(rows, w[l].size(0)) for l in range(n_lin - 1)]
        dz = [empty(rows, w[l].size(0)) for l in range(n_lin)]
        for l in range(n_lin - 1):
            bd.act[l] = act[l].data_ptr()
    for l in range(n_lin):
        bd.dz[l] = dz[l].data_ptr() if dz[l] is not None else None
    dx = empty(rows, w[0].size(1)) if need_dx else None
    if dx is not None:
        bd.dx, bd.ld_dx = dx.data_ptr(), _ld(dx)
    yhat = ln_part = None
    if ln is not None:
        prow = frows if fused else lib.gnc_mlp_backward_ln_partial_rows(ctypes.byref(bd.fwd))
        if prow > 0:  # d gamma / d beta sums formed inside the data kernel: no y_hat tensor, no colsum pass
            ln_part = empty(prow, 2 * out_w)
            bd.ln_partial = ln_part.data_ptr()
        else:
            yhat = empty(rows, out_w)
            bd.yhat = yhat.data_ptr()
    flops = 2.0 * rows * ((3 if fused else 2) * sum(x.size(0) * x.size(1) for x in w))
    with torch.cuda.device(dev):
        _check(_launch(f"mlp_backward{'_fused' if fused else ''}_in{w[0].size(1)}_h{w[0].size(0)}_out{out_w}_L{n_lin}", launch_ref,
                       lambda: lib.gnc_mlp_backward_f32(ctypes.byref(bd), _stream(launch_ref)), flops), "gnc_mlp_backward_f32")
    r = {"act": act, "dz": dz, "dx": dx, "yhat": yhat, "ln_sums": None, "residual_folded": bool(bd.dx_add_grad_out),
         "grad_out": g_eff, "saved_act_used": bool(bd.act_given), "_keep": (segs, w, b, g, gt, gi, g_sum, saved_act)}
    if fused:
        tots = [part.sum(dim=0) for part in parts]  # fixed order: reproducible
        r["dw"] = [tot[:x.numel()].view(x.size(0), x.size(1)) for tot, x in zip(tots, w)]
        r["db"] = [tot[x.numel():] for tot, x in zip(tots, w)]
    else:
        r["ln_part"] = ln_part if defer_ln_sums else None
    if ln_part is not None and (fused or not defer_ln_sums):
        tot = ln_part.sum(dim=0)  # fixed order: reproducible
        r["ln_sums"] = (tot[:out_w], tot[out_w:])  # (d beta, d gamma)
    return r


def _xty_spans(n: int, step: int):
    return [(i, min(step, n - i)) for i in range(0, n, step)]


def xty(a: torch.Tensor, b: torch.Tensor):
    """(A^T B [M, K], column sums of A [M]) over the rows; A [rows, M], B [rows, K] fp32.  Blocks of up to
    256 x 256 per launch when both operands are wider than 64 columns (workgroup-shared row tiles), 128 x 128 next to
    a narrow operand; the per-worker partials are summed in a fixed order (bitwise reproducible)."""
    lib = load_library()
    _require_cuda(a, b)
    a, b = _rowmajor(a), _rowmajor(b)
    rows, m, k = a.size(0), a.size(1), b.size(1)
    dev = a.device
    c = torch.empty(m, k, dtype=torch.float32, device=dev)
    colsum = torch.empty(m, dtype=torch.float32, device=dev)
    blocks = []
    for m0, mm in _xty_spans(m, 256 if k > 64 else 128):
        for k0, kk in _xty_spans(k, 256 if mm > 64 else 128):
            if kk <= 64 and mm > 128:  # a narrow remainder of k next to a wide block of m: the per-wave kernel's limit
                blocks += [(m1 + m0, mm1, k0, kk) for m1, mm1 in _xty_spans(mm, 128)]
            else:
                blocks.append((m0, mm, k0, kk))
    with torch.cuda.device(dev):
        for m0, mm, k0, kk in blocks:
            p = lib.gnc_xty_partials_for(rows, mm, kk)
            part = torch.empty(p, mm * kk + mm, dtype=torch.float32, device=dev)
            av, bv = a[:, m0:m0 + mm], b[:, k0:k0 + kk]
            _check(_launch("xty", av, lambda: lib.gnc_xty_f32(av.data_ptr(), _ld(av), bv.data_ptr(), _ld(bv), rows, mm,
                                                              kk, part.data_ptr(), p, _stream(av)),
                           2.0 * rows * mm * kk), "gnc_xty_f32")
            # fixed-order sum of the partials straight into the block's place (one launch, no sum + copies)
            cblk = c[m0:m0 + mm, k0:k0 + kk]
            _check(lib.gnc_reduce_partials_f32(part.data_ptr(), p, mm * kk + mm, mm, kk, cblk.data_ptr(), c.stride(0),
                                               colsum[m0:m0 + mm].data_ptr() if k0 == 0 else None, _stream(av)),
                   "gnc_reduce_partials_f32")
    return c, colsum


def xty_multi(products, row_sums=()):
    """Several weight-gradient products at once.  ``products``: list of ``(a [rows, M], b [rows, K], out)`` with ``out`` an
    [M, K] view to write into (any row stride: a column block of a wider gradient) or None for a fresh tensor; returns the
    list of ``(a^T b, column sums of a)``.  ``row_sums``: list of [P, W] tensors (per-tile partial sums); their row sums
    [W] are returned as a second list.  Small batches (every operand within gnc_xty_small_max_rows rows: the reference's
    one-graph-per-step regime) run as ONE launch per 8 jobs (gnc_xty_small_f32); anything else goes product by product
    through ``xty``."""
    lib = load_library()
    products = [(_rowmajor(a), _rowmajor(b), out) for a, b, out in products]
    row_sums = [_rowmajor(p) for p in row_sums]
    lim = lib.gnc_xty_small_max_rows()
    small = (all(a.size(0) <= lim and a.size(0) >= 1 and a.size(1) <= 4096 and b.size(1) <= 4096 for a, b, _ in products)
             and all(1 <= p.size(0) <= lim for p in row_sums) and (products or row_sums))
    if not small:
        res = []
        for a, b, out in products:
            c, cs = xty(a, b)
            if out is not None:
                out.copy_(c)
                c = out
            res.append((c, cs))
        return res, [p.sum(dim=0) for p in row_sums]
    dev = (products[0][0] if products else row_sums[0]).device
    _require_cuda(*[t for a, b, _ in products for t in (a, b)], *row_sums)
    jobs, res, sums = [], [], []
    for a, b, out in products:
        m, k = a.size(1), b.size(1)
        if a.size(0) != b.size(0):
            raise ValueError("xty_multi: operands of one product must have the same number of rows")
        if out is None:
            out = torch.empty(m, k, dtype=torch.float32, device=dev)
        elif out.shape != (m, k) or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("xty_multi: out must be a float32 [M, K] view with unit column stride")
        cs = torch.empty(m, dtype=torch.float32, device=dev)
        j = XtyJob()
        j.a, j.lda, j.b, j.ldb, j.rows, j.m, j.k = a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), a.size(0), m, k
        j.dw, j.ld_dw, j.db, j.kind = out.data_ptr(), out.stride(0), cs.data_ptr(), 0
        jobs.append(j)
        res.append((out, cs))
    for p in row_sums:
        o = torch.empty(p.size(1), dtype=torch.float32, device=dev)
        j = XtyJob()
        j.a, j.lda, j.rows, j.m, j.dw, j.kind = p.data_ptr(), _ld(p), p.size(0), p.size(1), o.data_ptr(), 1
        jobs.append(j)
        sums.append(o)
    with torch.cuda.device(dev):
        for q in range(0, len(jobs), GNC_XTY_MAX_JOBS):
            chunk = jobs[q:q + GNC_XTY_MAX_JOBS]
            arr = (XtyJob * len(chunk))(*chunk)
            flops = sum(2.0 * j.rows * j.m * j.k for j in chunk if j.kind == 0)
            _check(_launch("xty_small", res[0][0] if res else sums[0],
                           lambda: lib.gnc_xty_small_f32(ctypes.byref(arr), len(chunk), torch.cuda.current_stream(dev).cuda_stream),
                           flops), "gnc_xty_small_f32")
    return res, sums


def colsum_pair(g: torch.Tensor, y: torch.Tensor):
    """(column sums of G, column sums of G*Y): d beta and d gamma of a LayerNorm."""
    lib = load_library()
    g, y = _vector_rows(_rowmajor(g)), _vector_rows(_rowmajor(y))
    rows, width = g.shape
    both = torch.empty(2, width, dtype=torch.float32, device=g.device)  # row 0: colsum(G), row 1: colsum(G * Y)
    with torch.cuda.device(g.device):
        p = lib.gnc_xty_partials(rows)
        for c0 in range(0, width, 64):  # 64-column slabs (a wide LayerNorm is a few launches over column slices)
            w = min(64, width - c0)
            gs, ys = g[:, c0:c0 + w], y[:, c0:c0 + w]
            part = torch.empty(p, 2 * w, dtype=torch.float32, device=g.device)
            _check(lib.gnc_colsum_pair_f32(gs.data_ptr(), _ld(g), ys.data_ptr(), _ld(y), rows, w, part.data_ptr(), p,
                                           _stream(g)), "gnc_colsum_pair_f32")
            _check(lib.gnc_reduce_partials_f32(part.data_ptr(), p, 2 * w, 2, w, both[:, c0:c0 + w].data_ptr(), width, None,
                                               _stream(g)), "gnc_reduce_partials_f32")
    return both[0], both[1]


# --------------------------------------------------------------------------- activations other than ReLU: backward pieces
def _rows_out(out: torch.Tensor | None, like: torch.Tensor, what: str) -> torch.Tensor:
    """The [rows, width] fp32 result tensor of a row-wise kernel: a fresh one, or the caller's (any row stride)."""
    if out is None:
        return torch.empty(like.size(0), like.size(1), dtype=torch.float32, device=like.device)
    if (out.shape != like.shape or out.dtype != torch.float32 or out.device != like.device or (out.size(1) > 1 and out.stride(1) != 1)
            or (out.size(0) > 1 and out.stride(0) < out.size(1))):
        raise ValueError(f"{what}: out must be a float32 [rows, width] tensor with unit column stride on the input's device")
    return out


def activation(z: torch.Tensor, name: str, param: float = 0.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """act(z) elementwise (gnc_activation_f32); ``out`` may be a column slice of a wider tensor."""
    lib = load_library()
    _require_cuda(z)
    z = _rowmajor(z)
    out = _rows_out(out, z, "activation")
    with torch.cuda.device(z.device):
        _check(lib.gnc_activation_f32(z.data_ptr(), _ld(z), z.size(0), z.size(1), ACTIVATIONS[name], param, out.data_ptr(), _ld(out),
                                      _stream(z)), "gnc_activation_f32")
    return out


def activation_backward(z: torch.Tensor, grad_act: torch.Tensor, name: str, param: float = 0.0,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """grad_act * act'(z) (gnc_activation_backward_f32); ``out`` may be a column slice of a wider tensor."""
    lib = load_library()
    _require_cuda(z, grad_act)
    z, grad_act = _rowmajor(z), _rowmajor(grad_act)
    out = _rows_out(out, z, "activation_backward")
    with torch.cuda.device(z.device):
        _check(lib.gnc_activation_backward_f32(z.data_ptr(), _ld(z), grad_act.data_ptr(), _ld(grad_act), z.size(0), z.size(1),
                                               ACTIVATIONS[name], param, out.data_ptr(), _ld(out), _stream(z)),
               "gnc_activation_backward_f32")
    return out


def layer_norm_backward(y: torch.Tensor, gamma: torch.Tensor, grad_out: torch.Tensor, eps: float, out=None):
    """(grad_y, y_hat) of out = LayerNorm(y) * gamma + beta (gnc_layer_norm_backward_f32); ``out`` = (grad_y, y_hat) to write
    into, each possibly a column slice of a wider tensor."""
    lib = load_library()
    _require_cuda(y, gamma, grad_out)
    y, grad_out = _rowmajor(y), _rowmajor(grad_out)
    gy = _rows_out(out[0] if out is not None else None, y, "layer_norm_backward")
    yhat = _rows_out(out[1] if out is not None else None, y, "layer_norm_backward")
    with torch.cuda.device(y.device):
        _check(lib.gnc_layer_norm_backward_f32(y.data_ptr(), _ld(y), gamma.contiguous().data_ptr(), grad_out.data_ptr(), _ld(grad_out),
                                               y.size(0), y.size(1), eps, gy.data_ptr(), _ld(gy), yhat.data_ptr(), _ld(yhat),
                                               _stream(y)), "gnc_layer_norm_backward_f32")
    return gy, yhat


# --------------------------------------------------------------------------- K14 batch normalisation
BN_MAX_WIDTH = 256


def _bn_table(t: torch.Tensor, what: str) -> torch.Tensor:
    _require_cuda(t)
    t = _rowmajor(t)
    if not 1 <= t.size(1) <= BN_MAX_WIDTH:
        raise NotImplementedError(f"{what}: width {t.size(1)} is outside the batch-norm kernels (1..{BN_MAX_WIDTH})")
    return t


def _bn_vec(t: torch.Tensor, width: int) -> torch.Tensor:
    _require_cuda(t)
    if t.dtype != torch.float32 or t.numel() != width:
        raise ValueError(f"expected a float32 vector of {width} values, got {t.dtype} {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()  # only its address is used


def bn_partials(rows: int, width: int) -> int:
    """Partial rows the reducing K14 kernels write for a [rows, width] table (gnc_bn_partials)."""
    return int(load_library().gnc_bn_partials(rows, width))


def bn_stats(z: torch.Tensor, eps: float, momentum: float = 0.0, running_mean: torch.Tensor | None = None,
             running_var: torch.Tensor | None = None):
    """(mean, invstd) [C] each of the columns of ``z`` [rows, C] (biased variance, invstd = 1 / sqrt(var + eps)); the running
    statistics, when given (contiguous float32 [C]), are updated IN PLACE with ``momentum`` (unbiased variance)."""
    lib = load_library()
    z = _bn_table(z, "bn_stats")
    rows, width = z.shape
    if rows < 1:
        raise ValueError("bn_stats: no rows")
    for r in (running_mean, running_var):
        if r is not None and (not r.is_cuda or r.dtype != torch.float32 or r.numel() != width or not r.is_contiguous()):
            raise ValueError("bn_stats: running statistics must be contiguous float32 [C] on the GPU")
    both = torch.empty(2, width, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        p = lib.gnc_bn_partials(rows, width)
        part = torch.empty(p, 3 * width, dtype=torch.float32, device=z.device)
        _check(_launch("bn_stats", z, lambda: lib.gnc_bn_stats_f32(z.data_ptr(), _ld(z), rows, width, part.data_ptr(), p, _stream(z))),
               "gnc_bn_stats_f32")
        _check(lib.gnc_bn_finalize_f32(part.data_ptr(), p, rows, width, eps, momentum, both[0].data_ptr(), both[1].data_ptr(),
                                       running_mean.data_ptr() if running_mean is not None else None,
                                       running_var.data_ptr() if running_var is not None else None, _stream(z)),
               "gnc_bn_finalize_f32")
    return both[0], both[1]


def bn_apply(z: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
             residual: torch.Tensor | None = None, inplace: bool = False) -> torch.Tensor:
    """(z - mean) * invstd * gamma + beta (+ residual); ``inplace`` writes the result over ``z``."""
    lib = load_library()
    zt = _bn_table(z, "bn_apply")
    rows, width = zt.shape
    if residual is not None:
        residual = _bn_table(residual, "bn_apply")
        if residual.shape != zt.shape:
            raise ValueError(f"bn_apply: residual {tuple(residual.shape)} does not match {tuple(zt.shape)}")
    out = zt if (inplace and zt is z) else torch.empty(rows, width, dtype=torch.float32, device=zt.device)
    mean, invstd, gamma, beta = (_bn_vec(v, width) for v in (mean, invstd, gamma, beta))
    with torch.cuda.device(zt.device):
        _check(_launch("bn_apply", zt, lambda: lib.gnc_bn_apply_f32(
            zt.data_ptr(), _ld(zt), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            residual.data_ptr() if residual is not None else None, _ld(residual) if residual is not None else 0, rows, width,
            out.data_ptr(), _ld(out), _stream(zt))), "gnc_bn_apply_f32")
    return out


def bn_small_max_rows() -> int:
    """Row limit of the one-launch kernels (gnc_bn_small_max_rows)."""
    return int(load_library().gnc_bn_small_max_rows())


def bn_forward(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, residual: torch.Tensor | None = None,
               running_mean: torch.Tensor | None = None, running_var: torch.Tensor | None = None, momentum: float = 0.0,
               eps: float = 1e-5, inplace: bool = False):
    """Training-mode batch norm of ``z`` [rows, C] (+ residual): ``(out, mean, invstd)``.  Up to ``bn_small_max_rows()`` rows it is
    one launch (statistics, running statistics and normalisation), above that ``bn_stats`` + ``bn_apply``."""
    lib = load_library()
    zt = _bn_table(z, "bn_forward")
    rows, width = zt.shape
    if rows < 1 or rows > lib.gnc_bn_small_max_rows():
        mean, invstd = bn_stats(zt, eps, momentum, running_mean, running_var)
        return bn_apply(zt, mean, invstd, gamma, beta, residual, inplace=inplace and zt is z), mean, invstd
    if residual is not None:
        residual = _bn_table(residual, "bn_forward")
        if residual.shape != zt.shape:
            raise ValueError(f"bn_forward: residual {tuple(residual.shape)} does not match {tuple(zt.shape)}")
    for r in (running_mean, running_var):
        if r is not None and (not r.is_cuda or r.dtype != torch.float32 or r.numel() != width or not r.is_contiguous()):
            raise ValueError("bn_forward: running statistics must be contiguous float32 [C] on the GPU")
    gamma, beta = _bn_vec(gamma, width), _bn_vec(beta, width)
    out = zt if (inplace and zt is z) else torch.empty(rows, width, dtype=torch.float32, device=zt.device)
    both = torch.empty(2, width, dtype=torch.float32, device=zt.device)
    with torch.cuda.device(zt.device):
        _check(_launch("bn_forward_small", zt, lambda: lib.gnc_bn_forward_small_f32(
            zt.data_ptr(), _ld(zt), gamma.data_ptr(), beta.data_ptr(), residual.data_ptr() if residual is not None else None,
            _ld(residual) if residual is not None else 0, rows, width, eps, momentum, out.data_ptr(), _ld(out), both[0].data_ptr(),
            both[1].data_ptr(), running_mean.data_ptr() if running_mean is not None else None,
            running_var.data_ptr() if running_var is not None else None, _stream(zt))), "gnc_bn_forward_small_f32")
    return out, both[0], both[1]


def bn_backward(grad_out: torch.Tensor, z: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor,
                need_dz: bool = True):
    """(dz, dgamma, dbeta) of out = (z - mean(z)) * invstd(z) * gamma + beta over the rows of ``z``; ``dz`` is None when not asked."""
    lib = load_library()
    z, grad_out = _bn_table(z, "bn_backward"), _bn_table(grad_out, "bn_backward")
    rows, width = z.shape
    if grad_out.shape != z.shape or rows < 1:
        raise ValueError(f"bn_backward: grad_out {tuple(grad_out.shape)} does not match z {tuple(z.shape)}")
    mean, invstd, gamma = (_bn_vec(v, width) for v in (mean, invstd, gamma))
    sums = torch.empty(2, width, dtype=torch.float32, device=z.device)  # row 0: d beta, row 1: d gamma
    dz = torch.empty(rows, width, dtype=torch.float32, device=z.device) if need_dz else None
    if rows <= lib.gnc_bn_small_max_rows():  # one launch: a workgroup per 4 columns sums its rows, then writes its dz columns
        with torch.cuda.device(z.device):
            _check(_launch("bn_backward_small", z, lambda: lib.gnc_bn_backward_small_f32(
                grad_out.data_ptr(), _ld(grad_out), z.data_ptr(), _ld(z), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), rows,
                width, dz.data_ptr() if need_dz else None, _ld(dz) if need_dz else 0, sums[0].data_ptr(), sums[1].data_ptr(),
                _stream(z))), "gnc_bn_backward_small_f32")
        return dz, sums[1], sums[0]
    with torch.cuda.device(z.device):
        p = lib.gnc_bn_partials(rows, width)
        part = torch.empty(p, 2 * width, dtype=torch.float32, device=z.device)
        _check(_launch("bn_backward_sums", z, lambda: lib.gnc_bn_backward_sums_f32(
            grad_out.data_ptr(), _ld(grad_out), z.data_ptr(), _ld(z), mean.data_ptr(), invstd.data_ptr(), rows, width,
            part.data_ptr(), p, _stream(z))), "gnc_bn_backward_sums_f32")
        _check(lib.gnc_reduce_partials_f32(part.data_ptr(), p, 2 * width, 2, width, sums.data_ptr(), width, None, _stream(z)),
               "gnc_reduce_partials_f32")
        if need_dz:
            _check(_launch("bn_backward_dz", z, lambda: lib.gnc_bn_backward_dz_f32(
                grad_out.data_ptr(), _ld(grad_out), z.data_ptr(), _ld(z), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                sums[0].data_ptr(), sums[1].data_ptr(), rows, width, dz.data_ptr(), _ld(dz), _stream(z))), "gnc_bn_backward_dz_f32")
    return dz, sums[1], sums[0]


def bn_fold(weight: torch.Tensor, bias: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
            running_var: torch.Tensor, eps: float):
    """(W', b'): the Linear (weight [out, in], bias) followed by an eval-mode batch norm, as one Linear.  Fresh buffers on every
    call (nothing is cached: the live parameters and running statistics are read each time)."""
    lib = load_library()
    _require_cuda(weight, bias)
    w = _rowmajor(weight.detach())
    m, k = w.shape
    if not 1 <= m <= BN_MAX_WIDTH:
        raise NotImplementedError(f"bn_fold: width {m} is outside the batch-norm kernels (1..{BN_MAX_WIDTH})")
    gamma, beta, running_mean, running_var = (_bn_vec(v, m) for v in (gamma, beta, running_mean, running_var))
    b = _bn_vec(bias, m) if bias is not None else None
    ldo = (k + 3) // 4 * 4  # rows of 16-B pieces for the kernels that read the weights as vectors
    w_out = torch.empty(m, ldo, dtype=torch.float32, device=w.device)[:, :k]
    b_out = torch.empty(m, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib.gnc_bn_fold_f32(w.data_ptr(), _ld(w), b.data_ptr() if b is not None else None, gamma.data_ptr(), beta.data_ptr(),
                                   running_mean.data_ptr(), running_var.data_ptr(), eps, m, k, w_out.data_ptr(), ldo,
                                   b_out.data_ptr(), _stream(w)), "gnc_bn_fold_f32")
    return w_out, b_out


# --------------------------------------------------------------------------- fused Adam
def adam_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor,
              scratch: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float = 0.0) -> None:
    """One Adam update of the flat fp32 buffer ``param`` from ``grad`` (see include/gnc_hip.h); ``step`` is a device
    int64 [1] counter advanced by the call, ``scratch`` a device float32 [2]."""
    lib = load_library()
    _require_cuda(param, grad, exp_avg, exp_avg_sq, step, scratch)
    n = param.numel()
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("adam_step: flat contiguous float32 buffers of one size expected")
    if step.dtype != torch.int64 or scratch.dtype != torch.float32 or scratch.numel() < 2:
        raise ValueError("adam_step: step must be int64 [1], scratch float32 [2]")
    with torch.cuda.device(param.device):
        # lr and the betas go down as the doubles they are: the bias corrections are then torch.optim.Adam's
        _check(_launch("adam_flat", param, lambda: lib.gnc_adam_step_hp64_f32(
            param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n, lr, beta1, beta2, eps, weight_decay,
            step.data_ptr(), scratch.data_ptr(), _stream(param)), 28.0 * n), "gnc_adam_step_f32")


# --------------------------------------------------------------------------- controlled optimizer step (K22)
def opt_ctl(rule: str, lr: float, *, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
            nesterov: bool = False, max_grad_norm: float | None = None, check_nonfinite: bool = False, schedule: str = "constant",
            warmup_steps: int = 0, total_steps: int = 0, min_lr: float = 0.0, gamma: float = 0.1, every: int = 1) -> OptCtl:
    """The ``OptCtl`` of a rule ("adam": Adam + L2, "adamw", "sgd") and a schedule ("constant", "cosine", "step").  Unknown names
    raise ValueError; the ranges are checked by the library on every step."""
    if rule not in OPT_RULES:
        raise ValueError(f"optimizer rule {rule!r}: one of {sorted(OPT_RULES)} expected")
    if schedule not in LR_SCHEDULES:
        raise ValueError(f"lr schedule {schedule!r}: one of {sorted(LR_SCHEDULES)} expected")
    c = OptCtl()
    c.rule, c.schedule, c.nesterov = OPT_RULES[rule], LR_SCHEDULES[schedule], int(bool(nesterov))
    c.clip, c.check_nonfinite = int(max_grad_norm is not None), int(bool(check_nonfinite) or max_grad_norm is not None)
    c.warmup_steps, c.total_steps, c.every = int(warmup_steps), int(total_steps), int(every)
    c.lr, c.min_lr, c.gamma, c.max_grad_norm = float(lr), float(min_lr), float(gamma), float(max_grad_norm or 0.0)
    c.beta1, c.beta2, c.eps, c.weight_decay, c.momentum = float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(momentum)
    return c


def grad_sumsq(grad: torch.Tensor, partials: torch.Tensor) -> None:
    """Sum of ``g * g`` over the flat fp32 ``grad`` into ``partials`` (float64 [GRAD_NORM_BLOCKS]): a fixed grid, no atomics, the
    same bits for the same values at any 16-B aligned address."""
    lib = load_library()
    _require_cuda(grad, partials)
    if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.dim() != 1:
        raise ValueError("grad_sumsq: a flat contiguous float32 buffer expected")
    if partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < GRAD_NORM_BLOCKS:
        raise ValueError(f"grad_sumsq: partials must be float64 [{GRAD_NORM_BLOCKS}]")
    with torch.cuda.device(grad.device):
        _check(_launch("grad_sumsq", grad, lambda: lib.gnc_grad_sumsq_f32(grad.data_ptr(), grad.numel(), partials.data_ptr(),
                                                                          _stream(grad)), 4.0 * grad.numel()), "gnc_grad_sumsq_f32")


def optimizer_ctl_step(param: torch.Tensor, grad: torch.Tensor, state1: torch.Tensor | None, state2: torch.Tensor | None,
                       step: torch.Tensor, scalars: torch.Tensor, skipped: torch.Tensor, partials: torch.Tensor | None,
                       ctl: OptCtl) -> None:
    """One controlled update of the flat fp32 buffer ``param`` from ``grad`` (include/gnc_hip.h, csrc/optimizer_ctl.hip): the
    gradient-norm pass when ``ctl`` clips or checks for non-finite values, the control tick (schedule, clip coefficient, bias
    corrections, skip flag - all on the device) and the element launch of ``ctl``'s rule.  ``state1`` / ``state2``: Adam's moments,
    or SGD's momentum buffer (None without momentum) / None.  ``step`` int64 [1], ``scalars`` float32 [OPT_SCALARS], ``skipped`` int64 [2]
    (count, this step's flag), ``partials`` float64 [GRAD_NORM_BLOCKS] (None when ``ctl`` needs no norm).  ``grad`` is read, never
    written: the clip is applied to the values as they are read."""
    lib = load_library()
    adam = ctl.rule != OPT_RULES["sgd"]
    use_norm = bool(ctl.clip or ctl.check_nonfinite)
    if adam and (state1 is None or state2 is None):
        raise ValueError("optimizer_ctl_step: Adam and AdamW need both moment buffers")
    if not adam and (state2 is not None or (state1 is None) != (ctl.momentum == 0.0)):
        raise ValueError("optimizer_ctl_step: SGD takes the momentum buffer as state1 exactly when momentum != 0, and no state2")
    if use_norm and partials is None:
        raise ValueError("optimizer_ctl_step: clipping and the non-finite check need the partials buffer")
    _require_cuda(param, grad, state1, state2, step, scalars, skipped, partials)
    n = param.numel()
    for t in (param, grad, state1, state2):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise ValueError("optimizer_ctl_step: flat contiguous float32 buffers of one size expected")
    if (step.dtype != torch.int64 or step.numel() < 1 or scalars.dtype != torch.float32 or scalars.numel() < OPT_SCALARS
            or not scalars.is_contiguous() or skipped.dtype != torch.int64 or skipped.numel() < 2 or not skipped.is_contiguous()):
        raise ValueError(f"optimizer_ctl_step: step must be int64 [1], scalars float32 [{OPT_SCALARS}], skipped int64 [2]")
    if partials is not None and (partials.dtype != torch.float64 or partials.numel() < GRAD_NORM_BLOCKS or not partials.is_contiguous()):
        raise ValueError(f"optimizer_ctl_step: partials must be float64 [{GRAD_NORM_BLOCKS}]")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    state_bytes = 8.0 * ((state1 is not None) + (state2 is not None))
    with torch.cuda.device(param.device):
        _check(_launch("optimizer_ctl", param, lambda: lib.gnc_optimizer_ctl_step_f32(
            param.data_ptr(), grad.data_ptr(), ptr(state1), ptr(state2), n, ctypes.byref(ctl), step.data_ptr(), scalars.data_ptr(),
            skipped.data_ptr(), ptr(partials), _stream(param)), (12.0 + state_bytes + 4.0 * use_norm) * n), "gnc_optimizer_ctl_step_f32")


# --------------------------------------------------------------------------- classification loss head (K23)
def class_loss(logits: torch.Tensor, labels: torch.Tensor, *, status: torch.Tensor, kind: str = "ce", class_weight: torch.Tensor | None = None,
               label_smoothing: float = 0.0, pos_weight: float = 1.0, reduction: str = "mean", scale: float = 1.0,
               with_gradient: bool = True, loss_sum: torch.Tensor | None = None, confusion: torch.Tensor | None = None,
               workspace: torch.Tensor | None = None):
    """``(loss float32 [1], dlogits float32 [G, C] | None)`` of ``logits`` [G, C] and ``labels`` int64 [G] (include/gnc_hip.h,
    csrc/class_loss.hip): ``kind`` "ce" (``class_weight`` float32 [C] or None, ``label_smoothing``) or "bce" (C == 1, labels 0 / 1,
    ``pos_weight``), ``reduction`` "mean" / "sum", the loss and its gradient multiplied by ``scale``.  ``with_gradient=False`` scores
    only.  ``loss_sum`` (float64, one element) += the returned loss; ``confusion`` (int64 [K, K], K = C or 2 for "bce") += the counts,
    rows = label, columns = predicted class; ``status`` (int32 [1]) |= 1 when a label lies outside the classes (such a row is left
    out of everything and its gradient row is zeros).  Up to ``CLASS_LOSS_ONE_LAUNCH_ROWS`` rows all of it is ONE kernel launch;
    more rows need ``workspace`` (float64 [CLASS_LOSS_WORKSPACE_DOUBLES]; made here when None)."""
    lib = load_library()
    if kind not in LOSS_KINDS:
        raise ValueError(f"class_loss: kind {kind!r}: one of {sorted(LOSS_KINDS)} expected")
    if reduction not in LOSS_REDUCTIONS:
        raise ValueError(f"class_loss: reduction {reduction!r}: one of {sorted(LOSS_REDUCTIONS)} expected")
    _require_cuda(logits, labels, status, class_weight, loss_sum, confusion, workspace)
    z = _rowmajor(logits.detach())
    G, C = z.shape
    K = 2 if kind == "bce" else C
    if kind == "bce" and C != 1:
        raise ValueError(f"class_loss: kind 'bce' takes ONE logit per sample, got {C}")
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.numel() != G or not labels.is_contiguous():
        raise ValueError(f"class_loss: labels must be contiguous int64 [{G}]")
    if class_weight is not None and (kind == "bce" or class_weight.dtype != torch.float32 or class_weight.shape != (C,)
                                     or not class_weight.is_contiguous()):
        raise ValueError(f"class_loss: class_weight must be contiguous float32 [{C}], with kind 'ce'")
    if status.dtype != torch.int32 or status.numel() < 1:
        raise ValueError("class_loss: status must be int32 [1]")
    if loss_sum is not None and (loss_sum.dtype != torch.float64 or loss_sum.numel() != 1):
        raise ValueError("class_loss: loss_sum must be one float64 element")
    if confusion is not None and (confusion.dtype != torch.int64 or confusion.shape != (K, K) or not confusion.is_contiguous()):
        raise ValueError(f"class_loss: confusion must be contiguous int64 [{K}, {K}]")
    dev = z.device
    if G > CLASS_LOSS_ONE_LAUNCH_ROWS and workspace is None:
        workspace = torch.empty(CLASS_LOSS_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
    if workspace is not None and (workspace.dtype != torch.float64 or workspace.numel() < CLASS_LOSS_WORKSPACE_DOUBLES
                                  or not workspace.is_contiguous()):
        raise ValueError(f"class_loss: workspace must be float64 [{CLASS_LOSS_WORKSPACE_DOUBLES}]")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dz = torch.empty(G, C, dtype=torch.float32, device=dev) if with_gradient else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        _check(_launch("class_loss", z, lambda: lib.gnc_class_loss_f32(
            z.data_ptr(), _ld(z), labels.data_ptr(), ptr(class_weight), G, C, LOSS_KINDS[kind], float(label_smoothing), float(pos_weight),
            LOSS_REDUCTIONS[reduction], float(scale), loss.data_ptr(), ptr(dz), C, ptr(loss_sum), ptr(confusion), status.data_ptr(),
            ptr(workspace), _stream(z)), (8.0 if with_gradient else 4.0) * G * C + 8.0 * G), "gnc_class_loss_f32")
    return loss, dz


def class_loss_launches(num_rows: int, with_gradient: bool = True) -> int:
    """Kernel launches of one ``class_loss`` call (one ``KernelTimers`` entry either way)."""
    return int(load_library().gnc_class_loss_launches(int(num_rows), int(bool(with_gradient))))
