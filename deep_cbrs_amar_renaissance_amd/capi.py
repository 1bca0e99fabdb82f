"""ctypes binding of the C-ABI in ``include/amar_hip.h`` (``libamar_hip.so``).

torch is only the carrier here: tensors provide device memory (``data_ptr()``) and the current
HIP stream; every function below checks shapes on the host, hands raw pointers to the library
and raises on a non-zero return code.  There is NO fallback: if the shared library is missing,
or a tensor is not on a GPU, the call fails loudly.

Binding a new entry point:
  1. add its (restype, argtypes) to SIGNATURES, at its place in the header's order;
  2. check shapes on the host first and raise ValueError naming the wrapper;
  3. marshal with _ptr(t, F32 | I32, name) (typed pointer, None -> NULL), _ptr_entries (per-non-zero arrays), _mat (pointer and
     leading dimension of a 2-D float32 view, (None, 0) for None) and _col (a [B] or [B, 1] column); _ptr(t) for a buffer made here;
  4. launch with _launch('amar_x_f32', ...): it appends the current stream and raises on a non-zero code.  A host-only
     function (a route query) goes through _call('amar_x_route', ..., ctypes.byref(info)): no stream;
  5. a launcher and its route query share one _x_args builder; a route-info structure derives from _RouteInfo.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libamar_hip.so')

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ACT_CODES = {None: ACT_NONE, 'linear': ACT_NONE, 'relu': ACT_RELU, 'sigmoid': ACT_SIGMOID}
AGG_SUM, AGG_MAX, AGG_MIN = 0, 1, 2
AGG_CODES = {'sum': AGG_SUM, 'max': AGG_MAX, 'min': AGG_MIN}
SPMM_BIAS, SPMM_RELU, SPMM_ACCUM, SPMM_ACCUM_DIV, SPMM_SCALE_NEXT, SPMM_SAGE_TAIL, SPMM_LT_NOPAIRS = 1, 2, 4, 8, 16, 32, 64

_P = ctypes.c_void_p
_I32, _I64, _U32, _F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float

# symbol -> (restype, argtypes); kept in the order of include/amar_hip.h
SIGNATURES = {
    'amar_version': (ctypes.c_int, []),
    'amar_error_string': (ctypes.c_char_p, [ctypes.c_int]),
    'amar_last_hip_error': (ctypes.c_int, []),
    'amar_spmm_csr_f32': (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _U32, _P,
                                         _P, _I64, _P, _I64, _F32, _P]),
    'amar_spmm_sj_f32': (ctypes.c_int, [_P, _P, _P, _I32, _P, _I64, _P, _I64, _I32, _I32, _U32, _P,
                                        _P, _I64, _P, _I64, _F32, _P, _I32, _P, _I64, _P]),
    'amar_spmm_xs_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _I32, _P, _I64, _I32, _P, _P, _P, _I64, _I32, _I32, _U32, _P,
                                        _P, _I64, _P, _I64, _F32, _P, _I32, _P, _I64, _P]),
    'amar_gat_lt_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _I64,
                                       _I32, _I32, _I32, _I32, _P]),
    'amar_gat_lt_rows_per_wave': (ctypes.c_int, [_I32]),
    'amar_colmax_f32': (ctypes.c_int, [_P, _I64, _P, _P]),
    'amar_spmm_lt_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _I32, _P, _P, _I64, _I32, _I32, _U32, _P,
                                        _P, _I64, _P, _I64, _F32, _P, _I32, _P, _I64, _P]),
    'amar_propagate_route': (ctypes.c_int, [_I32, _I64, _I64, _I32, _U32, _P]),
    'amar_gat_xs_f32': (ctypes.c_int, [_P, _P, _I32, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P]),
    'amar_gcn_layer_f32': (ctypes.c_int, [_P, _P, _P, _P, _I64, _I32, _P, _P, _I64, _P, _I32, _P, _I64, _I32, _P]),
    'amar_rowwise_xw_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _I32, _P]),
    'amar_rowwise_xw_gather_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _P, _I32, _P, _I64, _P, _I32, _P]),
    'amar_rowwise_xw_route': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _P, _I64, _P, _I64, _I32, _I32, _I32, _P]),
    'amar_sage_layer_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _I32, _P, _I64, _I32, _I32, _P]),
    'amar_sage_tail_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _I32, _P, _P, _I32, _P, _I64, _I64, _P]),
    'amar_sage_tail_route': (ctypes.c_int, [_I32, _I32, _I64, _P]),
    'amar_sage_layer_agg_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _I32, _P, _I64, _I32, _I32, _I32, _P]),
    'amar_sage_aggregate_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _I64, _P, _I64, _I32, _I32, _I32, _P]),
    'amar_sage_aggregate_bwd_f32': (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I32, _P, _P, _I64, _I32, _I32, _P]),
    'amar_gat_layer_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _P, _I64, _I32, _I32, _P]),
    'amar_rowwise_xw_heads_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _I32, _P, _I64, _P, _P, _P, _I32, _P]),
    'amar_gat_heads_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _P]),
    'amar_dense_f32': (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _I64, _I32, _I32, _I32, _P]),
    'amar_dense_route': (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _I64, _I32, _I32, _I32, _P]),
    'amar_dense_split_bytes': (ctypes.c_int64, [_I32, _I32]),
    'amar_dense_split_pack_f32': (ctypes.c_int, [_P, _I32, _I32, _P]),
    'amar_dense_split_f32': (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _I64, _I32, _I32, _I32, _P]),
    'amar_chain_pack_floats': (ctypes.c_int64, [_P, _I32]),
    'amar_chain_pack_f32': (ctypes.c_int, [_P, _P, _P, _I32, _P]),
    'amar_chain_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _I64, _I64, _P]),
    'amar_chain_indexed_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _I64, _P, _I64, _P]),
    'amar_chain_segments_f32': (ctypes.c_int, [_P, _P, _P, _I32, _P, _I32, _P, _P, _P, _I32, _P, _I64, _I64, _P]),
    'amar_chain_rows2_route': (ctypes.c_int, [_P, _P, _P, _P, _P, _I32, _P, _P, _P, _P]),
    'amar_chain_rows2_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _I32, _P, _P, _P, _P]),
    'amar_chain_route': (ctypes.c_int, [_P, _I64, _I32, _P, _I32, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _I64, _P, _I64, _P]),
    'amar_chain_segments_route': (ctypes.c_int, [_P, _P, _P, _I32, _P, _I32, _P, _P, _P, _I32, _P, _I64, _I64, _P]),
    'amar_dual_chain_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _P, _I64, _I64, _P]),
    'amar_dual_chain_indexed_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _P, _I64, _P, _I64, _P]),
    'amar_copy_columns_f32': (ctypes.c_int, [_P, _I64, _P, _I32, _P, _I64, _I64, _I32, _P]),
    'amar_scatter_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _I32, _P]),
    'amar_scatter_closed_f32': (ctypes.c_int, [_P, _P, _P, _I64, _P, _I32, _I32, _P]),
    'amar_reduce_layers_f32': (ctypes.c_int, [_P, _I64, _I32, _I32, _P, _I64, _I64, _I32, _P]),
    'amar_reduce_layers_wsum_f32': (ctypes.c_int, [_P, _I64, _I32, _I32, _P, _P, _I64, _I64, _P]),
    'amar_reduce_layers_wsum_bwd_scratch': (ctypes.c_int64, []),
    'amar_reduce_layers_wsum_bwd_f32': (ctypes.c_int, [_P, _I64, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _P, _I64, _P]),
    'amar_act_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _I64, _I32, _I32, _P]),
    'amar_wgrad_scratch_floats': (ctypes.c_int64, [_I64, _I32, _I32]),
    'amar_wgrad_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I32, _I32, _P, _P, _P, _P]),
    'amar_dense_stack_f32': (ctypes.c_int, [_P, _I64, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I64, _P]),
    'amar_dense_stack_pair_f32': (ctypes.c_int, [_P, _P, _P]),
    'amar_dense_stack_route': (ctypes.c_int, [_P, _I64, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I64, _P]),
    'amar_dense_stack_bwd_groups': (ctypes.c_int64, [_I64]),
    'amar_dense_stack_bwd_workspace_floats': (ctypes.c_int64, [_I64, _I32, _P]),
    'amar_dense_stack_bwd_pair_f32': (ctypes.c_int, [_P, _P, _P]),
    'amar_dense_stack_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I32, _I64, _P]),
    'amar_dense_stack_bwd_route': (ctypes.c_int, [_P, _I64, _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I32, _I64, _P]),
    'amar_dense_bwd_workspace_floats': (ctypes.c_int64, [_I64, _I32, _I32]),
    'amar_dense_bwd_groups': (ctypes.c_int64, [_I64]),
    'amar_dense_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I32, _P, _I64, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _P]),
    'amar_dense_bwd_route': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I32, _P, _I64, _P, _P, _P, _I64, _I64, _I32, _I32, _P]),
    'amar_bce_grad_f32': (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P]),
    'amar_wgrad_route': (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I32, _I32, _P, _P, _P]),
    'amar_scatter_add_rows_route': (ctypes.c_int, [_I64, _I32, _P]),
    'amar_scatter_add_rows_f32': (ctypes.c_int, [_P, _I64, _P, _I32, _P, _I64, _I64, _I32, _P]),
    'amar_add_inplace_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I32, _F32, _P]),
    'amar_row_affine_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I32, _P]),
    'amar_l2norm_fwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I32, _I32, _P]),
    'amar_l2norm_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I32, _I32, _P]),
    'amar_gat_bwd_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                        _I32, _I32, _P]),
    'amar_gat_bwd_directed_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                                 _I32, _I32, _P]),
    'amar_gat_heads_bwd_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                              _I32, _I32, _I32, _P]),
    'amar_attention_mix_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I32, _P]),
    'amar_attention_mix_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _I64, _I32, _P]),
    'amar_add3_act_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I32, _I32, _P]),
    'amar_locality_scale_f32': (ctypes.c_int, [_P, _I64, _P, _P, _I64, _I64, _I32, _P]),
    'amar_locality_scale_bwd_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _I32, _I32, _P]),
    'amar_transpose_f32': (ctypes.c_int, [_P, _I32, _I32, _P, _P]),
    'amar_adam_f32': (ctypes.c_int, [_P, _P, _P, _P, _I64, _F32, _F32, _F32, _F32, _F32, _P]),
    'amar_adam_advance_f32': (ctypes.c_int, [_P, _F32, _F32, _F32, _P]),
    'amar_adam_dev_f32': (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _F32, _F32, _F32, _F32, _P]),
    'amar_optim_state_arrays': (ctypes.c_int, [_I32, _I32, _F32]),
    'amar_optim_advance_f32': (ctypes.c_int, [_P, _I32, _I32, _P, _P]),
    'amar_optim_f32': (ctypes.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P, _I64, _P, _F32, _P]),
    'amar_optim_multi_f32': (ctypes.c_int, [_I32, _I32, _P, _P, _I32, _I64, _P, _F32, _P, _P]),
    'amar_lr_rates_f32': (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P]),
    'amar_adam_advance_lr_f32': (ctypes.c_int, [_P, _P, _P, _F32, _F32, _P]),
    'amar_optim_advance_lr_f32': (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P, _P]),
    'amar_grad_clip_workspace_floats': (ctypes.c_int64, [_I32, _I64]),
    'amar_grad_clip_f32': (ctypes.c_int, [_I32, _F32, _P, _I32, _I64, _P, _P, _F32, _P, _P]),
    'amar_bpr_grad_f32': (ctypes.c_int, [_P, _I64, _P, _P, _I64, _P]),
    'amar_group_loss_grad_f32': (ctypes.c_int, [_I32, _F32, _P, _I64, _P, _P, _I64, _I32, _P]),
    'amar_bpr_sample_i32': (ctypes.c_int, [_P, _P, _P, _P, _I32, ctypes.c_uint64, _P, _I32, _I32, _P, _P, _P, _P]),
    'amar_bpr_sample_triplets_i32': (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, ctypes.c_uint64, _P, _I32, _I32, _P, _P,
                                                    _P, _P]),
    'amar_loss_counters': (ctypes.c_int32, []),
    'amar_loss_grad_f32': (ctypes.c_int, [_I32, _P, _P, _I64, _P, _P, _P, _I64, _P, _P]),
    'amar_loss_grad_weighted_f32': (ctypes.c_int, [_I32, _P, _P, _I64, _P, _P, _P, _P, _P, _I64, _P, _P]),
    'amar_dropout_f32': (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I32, ctypes.c_uint64, _P, _U32, _U32, _F32, _P]),
    'amar_dropout_advance': (ctypes.c_int, [_P, _P]),
    'amar_gat_layer_dropout_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _P, _I64, _I32, _I32,
                                                  ctypes.c_uint64, _P, _U32, _U32, _F32, _P]),
    'amar_gat_bwd_dropout_f32': (ctypes.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                                _I32, _I32, ctypes.c_uint64, _P, _U32, _U32, _F32, _P]),
    'amar_gat_bwd_directed_dropout_f32': (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P,
                                                         _I64, _I32, _I32, ctypes.c_uint64, _P, _U32, _U32, _F32, _P]),
    'amar_csr_transpose_i32': (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_adam_multi_f32': (ctypes.c_int, [_P, _I32, _I64, _P, _F32, _F32, _F32, _F32, _P, _P]),
    'amar_sum_into_f32': (ctypes.c_int, [_P, _I64, _F32, _P, _P]),
    'amar_topk_segmented_f32': (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P]),
    'amar_topk_segmented_after_f32': (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_recommend_slices': (ctypes.c_int32, [_I64, _I32, _P, _I32, _I32]),
    'amar_recommend_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P,
                                          _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_recommend_group_slices': (ctypes.c_int32, [_I64, _I64, _I32, _P, _I32, _I32]),
    'amar_recommend_group_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _P, _I64, _I64, _P, _P,
                                                _I32, _F32, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_recommend_among_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P,
                                                _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_recommend_lists_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P,
                                                _P, _P, _I32, _P, _P, _P]),
    'amar_recommend_after_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P,
                                                _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_nearest_slices': (ctypes.c_int32, [_I64, _I32, _I32, _I32]),
    'amar_nearest_workspace_floats': (ctypes.c_int64, [_I64, _I32, _I32, _I32, _I32]),
    'amar_nearest_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _I32, _P, _I64, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_rank_metrics_f64': (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, _I32, _P, _I32, _P, _P, _P, _P, _P]),
    'amar_rank_of_slices': (ctypes.c_int32, [_I64, _I32, _P, _I32, _I32]),
    'amar_rank_of_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P,
                                        _P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    'amar_rank_of_metrics_f64': (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P]),
    'amar_rank_route': (ctypes.c_int, [_I32, _P, _I32, _P]),
    'amar_rerank_mmr_f32': (ctypes.c_int, [_P, _P, _I64, _I32, _P, _I64, _I32, _I32, _I32, _F32, _I32, _P, _P, _P, _P, _P]),
    'amar_list_diversity_f64': (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _I32, _I32, _P, _I32, _P, _P, _P]),
    'amar_explain_f32': (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, _I32, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _I32, _I32,
                                        _P, _P, _P, _P, _P, _P]),
    'amar_rerank_calibrated_f32': (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _I32, _P, _P, _I32, _I32, _I32, _F32, _F32, _I32,
                                                  _P, _P, _P, _P, _P, _P]),
    'amar_list_calibration_f64': (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, _I32, _P, _P, _I32, _I32, _F32, _P, _I32, _P, _P, _P, _P]),
}

_lib = None


class AmarError(RuntimeError):
    pass


def load():
    """Load libamar_hip.so (once). Raises if it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AmarError(
                "{} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C deep_cbrs_amar_renaissance_amd/csrc`. The HIP path has no fallback.".format(LIB_PATH))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


def _check(code, what):
    if code != 0:
        lib = load()
        msg = lib.amar_error_string(code).decode()
        raise (ValueError if code == -1 else AmarError)(
            "{} failed: {} (code {}, hipError {})".format(what, msg, code, lib.amar_last_hip_error()))


def _ptr(t, dtype=None, name='tensor'):
    if t is None:
        return None
    if not t.is_cuda:
        raise AmarError("{} must live on the GPU (got {}); the HIP path has no CPU fallback".format(name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise ValueError("{} must be {} (got {})".format(name, dtype, t.dtype))
    return t.data_ptr()


_EMPTY_STANDINS = {}


def _ptr_entries(t, dtype, name):
    """Pointer of a per-non-zero array (colidx / vals).  A matrix without any non-zero has empty arrays whose data pointer
    is NULL; the C entry points reject NULL (a NULL with non-zeros behind it would fault the GPU), so an empty array is
    replaced by a one-element stand-in that the kernels never read (every row range is empty)."""
    if t is None or t.numel() > 0:
        return _ptr(t, dtype, name)
    _ptr(t, dtype, name)                                             # same device / dtype checks
    key = (t.device, dtype)
    if key not in _EMPTY_STANDINS:
        _EMPTY_STANDINS[key] = torch.zeros(4, dtype=dtype, device=t.device)
    return _EMPTY_STANDINS[key].data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ld(t, name):
    """Leading dimension of a 2-D row-major view (last dim contiguous)."""
    shape, stride = t.shape, t.stride()                                  # (read once each: this runs for every matrix operand of a launch)
    if len(shape) != 2 or (shape[1] > 1 and stride[1] != 1):
        raise ValueError("{} must be a 2-D tensor whose last dimension is contiguous".format(name))
    return stride[0] if shape[0] > 1 else max(stride[0], shape[1])


# The typed pointers are `_ptr(t, F32, name)` / `_ptr(t, I32, name)`: a wrapper of their own would add a Python call per operand to
# every launch, which an eager step pays a few hundred times.
F32, I32 = torch.float32, torch.int32


def _mat(t, name):
    """(pointer, leading dimension) of a 2-D float32 view; (None, 0) for None."""
    if t is None:
        return None, 0
    return _ptr(t, F32, name), _ld(t, name)


def _col(p, name):
    """(pointer, row stride) of a float32 column given as [B] or as [B, 1]."""
    return _ptr(p, F32, name), _ld(p, name) if p.dim() == 2 else 1


def _call(symbol, *args):
    """One call into the library: raises unless the entry point returns AMAR_OK."""
    code = getattr(load(), symbol)(*args)
    if code:
        _check(code, symbol)


def _launch(symbol, *args):
    """_call with the current stream as the last argument: every entry point that launches takes it there."""
    code = getattr(load(), symbol)(*args, _stream())
    if code:
        _check(code, symbol)


class _RouteInfo(ctypes.Structure):
    """Base of the amar_*_route_info structures.  as_dict(): every field but HIDDEN as int, those of BOOLS as bool, an array
    field as the list of its first n_layers entries, and the `kernel` code as its name where the class has KERNELS."""
    KERNELS, BOOLS, HIDDEN = None, (), ()

    def as_dict(self, n_layers=None):
        d = {}
        for name, _ in self._fields_:
            if name not in self.HIDDEN:
                v, conv = getattr(self, name), bool if name in self.BOOLS else int
                d[name] = [conv(x) for x in v[:n_layers]] if isinstance(v, ctypes.Array) else conv(v)
        if self.KERNELS is not None:
            d['kernel'] = self.KERNELS[d['kernel']]
        return d


def _next_product(what, width_name, n_rows, F, Wnext, Hnext):
    """The epilogue that makes the next layer's dense product, Hnext = Y . Wnext: checked, as (Wnext, Cn, Hnext, ldh)."""
    Cn = 0
    if Wnext is not None:
        if Wnext.shape[0] != F or not Wnext.is_contiguous() or Hnext is None or tuple(Hnext.shape) != (n_rows, Wnext.shape[1]):
            raise ValueError("{}: Wnext [{}, Cn] contiguous and Hnext [n_rows, Cn] expected".format(what, width_name))
        Cn = Wnext.shape[1]
    return (_ptr(Wnext, F32, 'Wnext'), Cn, *_mat(Hnext, 'Hnext'))


def _spmm_epilogue(what, n_rows, F, Y, bias, relu, acc_in, acc_out, acc_div, Wnext, Hnext):
    """The epilogue the SpMM entry points share, checked.  Returns (flags, tail): the BIAS / RELU / ACCUM / ACCUM_DIV bits and the
    arguments after `flags`: bias, acc_in, ld, acc_out, ld, acc_div, Wnext, Cn, Hnext, ld (amar_spmm_csr_f32 ends after acc_div).
    Call it after the wrapper's own checks: it is where marshalling starts."""
    flags = (SPMM_BIAS if bias is not None else 0) | (SPMM_RELU if relu else 0)
    if acc_out is not None:
        flags |= SPMM_ACCUM | (SPMM_ACCUM_DIV if acc_div is not None else 0)
        if acc_in is None or tuple(acc_in.shape) != (n_rows, F) or tuple(acc_out.shape) != (n_rows, F):
            raise ValueError("acc_in/acc_out must be [n_rows, F]")
    if Y is not None and tuple(Y.shape) != (n_rows, F):
        raise ValueError("Y must be [n_rows, F]")
    product = _next_product(what, 'F', n_rows, F, Wnext, Hnext)
    return flags, (_ptr(bias, F32, 'bias'), *_mat(acc_in, 'acc_in'), *_mat(acc_out, 'acc_out'),
                   float(acc_div) if acc_div is not None else 1.0, *product)


def _scaled_table(X, scale):
    """S.X in a fresh table: what a value-free image A = S C S gathers from."""
    Xs = torch.empty((X.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
    row_affine(X, scale, Xs)
    return Xs


def spmm_csr(rowptr, colidx, vals, X, Y=None, bias=None, relu=False, acc_in=None, acc_out=None, acc_div=None):
    """Y = A.X (+bias, ReLU); optionally acc_out = (acc_in + Y) [/ acc_div]. Tensors are views into device memory."""
    n_rows = rowptr.numel() - 1
    F = X.shape[1]
    if colidx.numel() and int(X.shape[0]) < 1:
        raise ValueError("X has no rows")
    if vals is not None and vals.numel() != colidx.numel():
        raise ValueError("vals and colidx differ in length")
    flags, tail = _spmm_epilogue('spmm_csr', n_rows, F, Y, bias, relu, acc_in, acc_out, acc_div, None, None)
    _launch('amar_spmm_csr_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), _ptr_entries(vals, F32, 'vals'),
            *_mat(X, 'X'), *_mat(Y, 'Y'), n_rows, F, flags, *tail[:6])


def spmm_sj(sj, X, Y=None, bias=None, relu=False, acc_in=None, acc_out=None, acc_div=None, Wnext=None, Hnext=None):
    """Y = A.X on the sliced-jagged image `sj` of A (utilities.math.SlicedJagged), with the epilogues of
    spmm_csr / gcn_layer.  Used when the node table does not fit the per-XCD L2."""
    n_rows = sj.shape[0]
    F = X.shape[1]
    if X.shape[0] < sj.shape[1]:
        raise ValueError("X has fewer rows than the matrix has columns")
    flags, tail = _spmm_epilogue('spmm_sj', n_rows, F, Y, bias, relu, acc_in, acc_out, acc_div, Wnext, Hnext)
    _launch('amar_spmm_sj_f32', _ptr(sj.entries, I32, 'entries'), _ptr(sj.counts, torch.int16, 'counts'), _ptr(sj.wave_start, I32, 'wave_start'),
            sj.n_slices, *_mat(X, 'X'), *_mat(Y, 'Y'), n_rows, F, flags, *tail)


def spmm_xs(xs, X, Y=None, bias=None, relu=False, acc_in=None, acc_out=None, acc_div=None, Wnext=None, Hnext=None,
            prescaled=False, scale_next=False, xself=None, rows_needed=None):
    """Y = A.X on the XCD-sliced image `xs` of A (utilities.math.XcdSliced): per-slice partial products with
    XCD <-> L2 affinity, then the combine kernel with the epilogues of spmm_csr / gcn_layer.

    A value-free image (xs.row_scale is set: A = S C S) gathers from S.X: `prescaled=True` says X already is that
    table (the fused GCN chain keeps it so with `scale_next`), otherwise one row_affine pass makes it here.

    `xs` may also be an LDS-tiled image (utilities.lds_tiled.LdsTiled, what DeviceCSR.tiled_image returns where the
    column-ordered form pays): the call is then amar_spmm_lt_f32, same keywords.

    `xself` ([n_rows, F], same leading dimension as X): where the rows' OWN entries of X are read from, instead of
    X[diag_offset:] — a row block of a partition whose own rows of the gathered table may not have landed yet (parallel.py)."""
    if hasattr(xs, 'words'):
        return spmm_lt(xs, X, Y, bias=bias, relu=relu, acc_in=acc_in, acc_out=acc_out, acc_div=acc_div, Wnext=Wnext, Hnext=Hnext,
                       prescaled=prescaled, scale_next=scale_next, xself=xself, rows_needed=rows_needed)
    n_rows = xs.shape[0]
    F = X.shape[1]
    diag_offset = int(getattr(xs, 'diag_offset', 0))
    if X.shape[0] != xs.shape[1] or diag_offset + n_rows > X.shape[0]:
        raise ValueError("X must have one row per column of the matrix")
    row_scale = getattr(xs, 'row_scale', None)
    if row_scale is None and (prescaled or scale_next):
        raise ValueError("spmm_xs: prescaled / scale_next need a value-free image")
    flags, tail = _spmm_epilogue('spmm_xs', n_rows, F, Y, bias, relu, acc_in, acc_out, acc_div, Wnext, Hnext)
    P = xs.partials(F)
    if row_scale is not None and not prescaled:
        col_scale = getattr(xs, 'col_scale', None)
        X = _scaled_table(X, col_scale if col_scale is not None else row_scale)
    if scale_next:
        flags |= SPMM_SCALE_NEXT
    _launch('amar_spmm_xs_f32', _ptr(xs.diag, F32, 'diag'), _ptr(xs.rowptr, I32, 'rowptr'), _ptr(xs.colidx, I32, 'colidx'), _ptr(xs.vals, F32, 'vals'),
            _ptr(row_scale, F32, 'row_scale'), xs.n_slices, *_mat(X, 'X'), X.shape[0],
            _xself_ptr(xself, X, diag_offset, n_rows, prescaled or row_scale is None), _ptr(P, F32, 'partials'),
            *_mat(Y, 'Y'), n_rows, F, flags, *tail)


def _xself_ptr(xself, X, diag_offset, n_rows, usable):
    """The pointer the SpMM kernels read the rows' own entries of X through: `xself` when given, else X[diag_offset:] (None: X)."""
    if xself is None:
        return _ptr(X[diag_offset:], F32, 'X') if diag_offset else None
    if not usable:
        raise ValueError("xself needs the table as the kernel gathers it (prescaled=True on a value-free image)")
    if tuple(xself.shape) != (n_rows, X.shape[1]) or _ld(xself, 'xself') != _ld(X, 'X'):
        raise ValueError("xself must be [n_rows, F] with the leading dimension of X")
    return _ptr(xself, F32, 'xself')


def spmm_lt(lt, X, Y=None, bias=None, relu=False, acc_in=None, acc_out=None, acc_div=None, Wnext=None, Hnext=None,
            prescaled=False, scale_next=False, sage_tail=None, xself=None, rows_needed=None):
    """Y = A.X on the LDS-tiled image `lt` of a value-free A = S C S (utilities.lds_tiled.LdsTiled): one launch, the
    row tile's sums in LDS, gathers in column order.  Keywords as spmm_xs (`prescaled`: X already holds S.X).
    sage_tail = (kernel [2F, F], bias [F]) on GraphSAGE's mean-aggregate image: Y = relu(l2_normalize([X || mean] . kernel + bias))
    in the same launch (AMAR_SPMM_SAGE_TAIL)."""
    n_rows, n_cols = lt.shape
    F = X.shape[1]
    if sage_tail is not None:
        if bias is not None or relu or acc_out is not None or Wnext is not None or not prescaled or Y is None:
            raise ValueError("spmm_lt: sage_tail takes the un-scaled table (prescaled=True), Y, and no other epilogue")
        if Hnext is not None and tuple(Hnext.shape) != (n_rows, F):
            raise ValueError("spmm_lt: with sage_tail, Hnext is a second [n_rows, F] copy of Y")
        kernel, kernel_bias = sage_tail
        if tuple(kernel.shape) != (2 * F, F) or not kernel.is_contiguous() or kernel_bias.numel() != F:
            raise ValueError("spmm_lt: sage_tail = (kernel [2F, F] contiguous, bias [F]) expected")
    if F != lt.F:
        raise ValueError("spmm_lt: the image was built for width {}, X is {} wide".format(lt.F, F))
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    if lt.rw > lds_tiled.geometry(F)[1]:
        raise ValueError("spmm_lt: the image's tiles hold {} rows per wave, the kernel's {}".format(lt.rw, lds_tiled.geometry(F)[1]))
    if X.shape[0] != n_cols or lt.diag_offset + n_rows > X.shape[0]:
        raise ValueError("X must have one row per column of the matrix")
    flags, tail = _spmm_epilogue('spmm_lt', n_rows, F, Y, bias, relu, acc_in, acc_out, acc_div, Wnext, Hnext)
    if sage_tail is not None:
        # (no other epilogue came through the checks above) the tail's kernel and bias travel in the Wnext / Cn and bias places
        flags, tail = SPMM_SAGE_TAIL, (_ptr(kernel_bias, F32, 'bias'), *tail[1:6], _ptr(kernel, F32, 'Wnext'), F, *tail[8:])
    if not prescaled:
        X = _scaled_table(X, lt.col_scale if lt.col_scale is not None else lt.row_scale)
    if scale_next:
        flags |= SPMM_SCALE_NEXT
    if not getattr(lt, 'pairs', True):
        flags |= SPMM_LT_NOPAIRS
    off = lt.diag_offset
    n_tiles = lt.n_tiles
    if rows_needed is not None and rows_needed < n_rows:
        # only the tiles that hold rows [0, rows_needed): the rows of the others are left as they are (the last layer of a
        # user-item-property graph: no tower reads its property rows — models/gnn.py `rows_needed`)
        cache = lt.__dict__.setdefault('_tiles_for_rows', {})
        if rows_needed not in cache:
            cache[rows_needed] = int((lt.tile_row0[:-1] < int(rows_needed)).sum())
        n_tiles = cache[rows_needed]
        if n_tiles == 0:
            return
    _launch('amar_spmm_lt_f32', *_lt_image_args(lt, n_tiles), _ptr(lt.diag, F32, 'diag'), _ptr(lt.row_scale, F32, 'row_scale'),
            *_mat(X, 'X'), X.shape[0], _xself_ptr(xself, X, off, n_rows, prescaled), *_mat(Y, 'Y'), n_rows, F, flags, *tail)


def _lt_image_args(lt, n_tiles):
    """What amar_spmm_lt_f32 and amar_gat_lt_f32 take first: the arrays of an LDS-tiled image and its tile count, window bound and pace."""
    return (_ptr(lt.words, I32, 'words'), _ptr(lt.stream_start, I32, 'stream_start'), _ptr(lt.wsteps, I32, 'wsteps'), _ptr(lt.tile_row0, I32, 'tile_row0'),
            _ptr(lt.n_win, I32, 'n_win'), _ptr(lt.vstart, I32, 'vstart'), _ptr(lt.vcount, I32, 'vcount'), n_tiles, lt.maxwin1, lt.pace_every)


PROPAGATE_KINDS = {'lt': 0, 'gat_lt': 1, 'xs': 2, 'gat_xs': 3}
ADDR_64, ADDR_32, ADDR_32_DENSE = 0, 1, 2
LT_KERNELS = ('pairs', 'nopairs', 'sage_tail', 'unsupported')


class PropagateRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_propagate_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('form', 'kernel', 'col_bits', 'reserved')] + \
               [(name, ctypes.c_int64) for name in ('max_cols', 'span_bytes')]
    KERNELS, HIDDEN = LT_KERNELS, ('reserved',)


def propagate_route(kind, n_cols, ld, width, flags=0, code=False):
    """Which gather-address form (0: 64-bit, 1: 32-bit byte offsets, 2: 32-bit offsets into a dense table) and, for 'lt', which kernel
    ('pairs' | 'nopairs' | 'sage_tail' | 'unsupported') a spmm_lt / gat_lt / spmm_xs / gat_xs call over a table of `n_cols` rows with
    leading dimension `ld` takes (amar_propagate_route: host only, the launchers ask the same function).  kind: 'lt' | 'gat_lt' | 'xs' |
    'gat_xs'; flags: SPMM_SAGE_TAIL / SPMM_LT_NOPAIRS.  A dict with `code` = the launcher's return code for these arguments added when
    code=True (nothing raised), else raises as the launcher's wrapper would."""
    info = PropagateRouteInfo()
    rc = load().amar_propagate_route(PROPAGATE_KINDS[kind], int(n_cols), int(ld), int(width), int(flags), ctypes.byref(info))
    if not code:
        _check(rc, 'amar_propagate_route')
    d = info.as_dict()
    if code:
        d['code'] = int(rc)
    return d


def sage_tail_on_lt_supported(x, f):
    """Whether spmm_lt's fused GraphSAGE tail (sage_tail=...) has a kernel for the table `x` [n_cols, f] as it lies in memory:
    amar_spmm_lt_f32's own decision (widths 8 / 16 / 32 and a table whose span stays below 2^32 bytes), from shapes and strides alone."""
    r = propagate_route('lt', x.shape[0], _ld(x, 'x'), f, SPMM_SAGE_TAIL, code=True)
    return r['code'] == 0 and r['kernel'] == 'sage_tail'


def gcn_layer(rowptr, colidx, vals, H, bias, Y, Wnext=None, Hnext=None):
    n_rows = rowptr.numel() - 1
    C = H.shape[1]
    if tuple(Y.shape) != (n_rows, C) or bias.numel() != C or H.shape[0] < n_rows:
        raise ValueError("gcn_layer: H [>=n_rows, C], bias [C], Y [n_rows, C] expected")
    product = _next_product('gcn_layer', 'C', n_rows, C, Wnext, Hnext)
    _launch('amar_gcn_layer_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), _ptr_entries(vals, F32, 'vals'),
            *_mat(H, 'H'), C, _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'), *product, n_rows)


def rowwise_xw(X, W, H, copy_to=None, a_self=None, a_neigh=None, s_self=None, s_neigh=None, row_scale=None, row_ids=None):
    """H = X . W row by row (+ the X_0 slice copy, GAT's attention scalars, a row scale).  row_ids (int32 [rows of H]): output row p
    reads X[row_ids[p]] and a negative id leaves a zero row (amar_rowwise_xw_gather_f32: the block layout of a node-range partition)."""
    if row_ids is not None:
        n_out, F = int(row_ids.numel()), X.shape[1]
        if copy_to is not None or a_self is not None or s_self is not None:
            raise ValueError("rowwise_xw: the row-gather form computes H only")
        if W.shape[0] != F or not W.is_contiguous() or tuple(H.shape) != (n_out, W.shape[1]) or not row_ids.is_contiguous():
            raise ValueError("rowwise_xw: W [F, C] contiguous, row_ids contiguous and H [len(row_ids), C] expected")
        if row_scale is not None and (row_scale.numel() != n_out or not row_scale.is_contiguous()):
            raise ValueError("rowwise_xw: row_scale must be a contiguous [len(row_ids)] vector")
        _launch('amar_rowwise_xw_gather_f32', *_mat(X, 'X'), F, _ptr(row_ids, I32, 'row_ids'), _ptr(W, F32, 'W'), W.shape[1], *_mat(H, 'H'),
                _ptr(row_scale, F32, 'row_scale'), n_out)
        return
    n_rows, F = X.shape
    if W.shape[0] != F or not W.is_contiguous() or tuple(H.shape) != (n_rows, W.shape[1]):
        raise ValueError("rowwise_xw: W [F, C] contiguous and H [n_rows, C] expected")
    if copy_to is not None and tuple(copy_to.shape) != (n_rows, F):
        raise ValueError("rowwise_xw: copy_to must be [n_rows, F]")
    if row_scale is not None and (row_scale.numel() != n_rows or not row_scale.is_contiguous()):
        raise ValueError("rowwise_xw: row_scale must be a contiguous [n_rows] vector")
    for v, nm in ((s_self, 's_self'), (s_neigh, 's_neigh')):
        if v is not None and (v.numel() != n_rows or not v.is_contiguous()):
            raise ValueError("rowwise_xw: {} must be a contiguous [n_rows] vector".format(nm))
    _launch('amar_rowwise_xw_f32', *_mat(X, 'X'), F, _ptr(W, F32, 'W'), W.shape[1], *_mat(H, 'H'), *_mat(copy_to, 'copy_to'),
            _ptr(a_self, F32, 'a_self'), _ptr(a_neigh, F32, 'a_neigh'), _ptr(s_self, F32, 's_self'), _ptr(s_neigh, F32, 's_neigh'),
            _ptr(row_scale, F32, 'row_scale'), n_rows)


XW_KERNELS = ('generic', 'vec8', 'vec16', 'pieces8')


class XwRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_xw_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'cp', 'rows_per_block', 'blocks')] + [('trips', ctypes.c_int64)]
    KERNELS = XW_KERNELS


def rowwise_xw_route(X, W, H, copy_to=None, attn=False, row_ids=None):
    """Which kernel rowwise_xw() runs for these tensors and how its capped grid walks the rows (amar_rowwise_xw_route: host only,
    nothing is launched; the launcher asks the same function, AMAR_XW_FORM included).  attn: the call computes the attention scalars;
    row_ids: the gather form, H has one row per id.  A dict: kernel 'generic' | 'vec8' | 'vec16' | 'pieces8', cp, rows_per_block,
    blocks, trips.  The product of rowwise_xw_heads() is the call with W viewed as [F, heads*C]."""
    n_rows = int(row_ids.numel()) if row_ids is not None else X.shape[0]
    F = X.shape[1]
    if W.dim() != 2 or W.shape[0] != F or not W.is_contiguous() or tuple(H.shape) != (n_rows, W.shape[1]):
        raise ValueError("rowwise_xw_route: W [F, C] contiguous and H [n_rows, C] expected")
    info = XwRouteInfo()
    _call('amar_rowwise_xw_route', *_mat(X, 'X'), F, _ptr(W, F32, 'W'), W.shape[1], *_mat(H, 'H'), *_mat(copy_to, 'copy_to'),
          1 if attn else 0, 1 if row_ids is not None else 0, n_rows, ctypes.byref(info))
    return info.as_dict()


def sage_layer(rowptr, colidx, X, W, bias, Y, self_loop=True):
    n_rows = rowptr.numel() - 1
    F = X.shape[1]
    if W.shape[0] != 2 * F or not W.is_contiguous() or bias.numel() != W.shape[1] or \
            tuple(Y.shape) != (n_rows, W.shape[1]) or X.shape[0] < n_rows:
        raise ValueError("sage_layer: W [2F, C] contiguous, bias [C], Y [n_rows, C] expected")
    _launch('amar_sage_layer_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), *_mat(X, 'X'), F, _ptr(W, F32, 'W'),
            _ptr(bias, F32, 'bias'), W.shape[1], *_mat(Y, 'Y'), 1 if self_loop else 0, n_rows)


def sage_tail(X, agg, W, bias, Y):
    """Y = relu(l2_normalize([X || agg] . W + bias)): GraphSageConv after its mean aggregate (see amar_sage_tail_f32)."""
    n_rows, F = agg.shape
    if X.shape[1] != F or X.shape[0] < n_rows or W.shape[0] != 2 * F or not W.is_contiguous() or bias.numel() != W.shape[1] or \
            tuple(Y.shape) != (n_rows, W.shape[1]):
        raise ValueError("sage_tail: X [>=n_rows, F], agg [n_rows, F], W [2F, C] contiguous, bias [C], Y [n_rows, C] expected")
    _launch('amar_sage_tail_f32', *_mat(X, 'X'), *_mat(agg, 'agg'), F, _ptr(W, F32, 'W'), _ptr(bias, F32, 'bias'), W.shape[1], *_mat(Y, 'Y'), n_rows)


class SageTailRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_sage_tail_route_info"""
    _fields_ = [('cp', ctypes.c_int32), ('blocks', ctypes.c_int32), ('trips', ctypes.c_int64)]


def sage_tail_route(F, C, n_rows):
    """The instantiation (cp accumulators per thread) and the capped grid of sage_tail() for these sizes (amar_sage_tail_route: host
    only; the launcher takes both from the same function).  A dict: cp, blocks, trips."""
    info = SageTailRouteInfo()
    _call('amar_sage_tail_route', int(F), int(C), int(n_rows), ctypes.byref(info))
    return info.as_dict()


def sage_tail_supported(F, C):
    return F % 4 == 0 and C % 4 == 0 and 4 <= F <= 64 and 4 <= C <= 64


def _agg_code(op, what):
    if op not in AGG_CODES:
        raise ValueError("{}: op must be one of {} (got {!r})".format(what, sorted(AGG_CODES), op))
    return AGG_CODES[op]


def sage_layer_agg(rowptr, colidx, X, W, bias, Y, op, self_loop=True):
    """Y = relu(l2_normalize([X || OP over the row's entries of X] . W + bias)), op in 'sum' | 'max' | 'min' (amar_sage_layer_agg_f32)."""
    n_rows = rowptr.numel() - 1
    F = X.shape[1]
    if W.shape[0] != 2 * F or not W.is_contiguous() or bias.numel() != W.shape[1] or \
            tuple(Y.shape) != (n_rows, W.shape[1]) or X.shape[0] < n_rows:
        raise ValueError("sage_layer_agg: W [2F, C] contiguous, bias [C], Y [n_rows, C] expected")
    _launch('amar_sage_layer_agg_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), *_mat(X, 'X'), F, _ptr(W, F32, 'W'),
            _ptr(bias, F32, 'bias'), W.shape[1], *_mat(Y, 'Y'), 1 if self_loop else 0, _agg_code(op, 'sage_layer_agg'), n_rows)


def sage_agg_layer_supported(F, C):
    return F in (4, 8, 16, 32) and 1 <= C <= 64


def sage_aggregate(rowptr, colidx, X, agg, op, cnt=None, self_loop=True):
    """agg = max | min over the row's entries (+ the row itself) of X; cnt (optional) = how many entries attain it (amar_sage_aggregate_f32)."""
    n_rows = rowptr.numel() - 1
    F = X.shape[1]
    if tuple(agg.shape) != (n_rows, F) or X.shape[0] < n_rows or (cnt is not None and tuple(cnt.shape) != (n_rows, F)):
        raise ValueError("sage_aggregate: X [>=n_rows, F], agg [n_rows, F], cnt [n_rows, F] or None expected")
    _launch('amar_sage_aggregate_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), *_mat(X, 'X'), F, *_mat(agg, 'agg'),
            *_mat(cnt, 'cnt'), 1 if self_loop else 0, _agg_code(op, 'sage_aggregate'), n_rows)


def sage_aggregate_bwd(rowptr, colidx, X, agg, cnt, d_agg, dX, self_loop=True, pack=None):
    """dX[j] += the shares of d_agg that X[j] attained (ties and duplicate edges share equally): the reverse pass of
    sage_aggregate (amar_sage_aggregate_bwd_f32).  rowptr / colidx: the TRANSPOSE of the structure the forward pass walked (row j
    lists the targets whose aggregate X[j] entered; DeviceCSR.transposed() — the same arrays for a symmetric edge multiset).
    pack: [n_rows, 2F] scratch (allocated if None)."""
    n_rows = rowptr.numel() - 1
    F = X.shape[1]
    for t, name in ((agg, 'agg'), (cnt, 'cnt'), (d_agg, 'd_agg'), (dX, 'dX')):
        if tuple(t.shape) != (n_rows, F):
            raise ValueError("sage_aggregate_bwd: {} [n_rows, F] expected".format(name))
    if X.shape[0] < n_rows:
        raise ValueError("sage_aggregate_bwd: X [>=n_rows, F] expected")
    if pack is None:
        pack = torch.empty((n_rows, 2 * F), dtype=torch.float32, device=X.device)
    if tuple(pack.shape) != (n_rows, 2 * F) or not pack.is_contiguous():
        raise ValueError("sage_aggregate_bwd: pack [n_rows, 2F] contiguous expected")
    _launch('amar_sage_aggregate_bwd_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), *_mat(X, 'X'), *_mat(agg, 'agg'),
            *_mat(cnt, 'cnt'), *_mat(d_agg, 'd_agg'), F, _ptr(pack, F32, 'pack'), *_mat(dX, 'dX'), 1 if self_loop else 0, n_rows)


def _gat_layer(what, rowptr, colidx, H, s_self, s_neigh, bias, Y, self_loop, drop):
    """gat_layer (drop None) and gat_layer_dropout: amar_gat_layer_f32 / amar_gat_layer_dropout_f32, which ends with the dropout site."""
    n_rows = rowptr.numel() - 1
    C = H.shape[1]
    if tuple(Y.shape) != (n_rows, C) or bias.numel() != C or s_self.numel() < n_rows or s_neigh.numel() < H.shape[0]:
        raise ValueError("{}: bias [C], Y [n_rows, C], s_self/s_neigh [n] expected".format(what))
    _launch('amar_gat_layer_f32' if drop is None else 'amar_gat_layer_dropout_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'),
            *_mat(H, 'H'), C, _ptr(s_self, F32, 's_self'), _ptr(s_neigh, F32, 's_neigh'), _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'),
            1 if self_loop else 0, n_rows, *(drop._args() if drop is not None else ()))


def gat_layer(rowptr, colidx, H, s_self, s_neigh, bias, Y, self_loop=True):
    _gat_layer('gat_layer', rowptr, colidx, H, s_self, s_neigh, bias, Y, self_loop, None)


GAT_HEADS_MAX_WIDTH = 64                                             # heads * channels the multi-head row kernels hold in one wavefront's lanes


def gat_heads_supported(heads, C):
    """The shapes amar_rowwise_xw_heads_f32 / amar_gat_heads_f32 / amar_gat_heads_bwd_f32 are built for."""
    return heads >= 1 and C >= 4 and C % 4 == 0 and heads * C <= GAT_HEADS_MAX_WIDTH


def rowwise_xw_heads(X, W, Hd, a_self, a_neigh, S):
    """Hd [n, heads*C] = X . W with W [F, heads, C], and S [n, 2*heads]: per row the heads' self scalars, then their neighbour scalars
    (a_self / a_neigh [C, heads, 1] in Keras's order)."""
    n_rows, F = X.shape
    if W.dim() != 3 or W.shape[0] != F or not W.is_contiguous():
        raise ValueError("rowwise_xw_heads: W [F, heads, C] contiguous expected")
    heads, C = int(W.shape[1]), int(W.shape[2])
    if tuple(Hd.shape) != (n_rows, heads * C) or tuple(S.shape) != (n_rows, 2 * heads) or not S.is_contiguous() or \
            any(v.numel() != C * heads or not v.is_contiguous() for v in (a_self, a_neigh)):
        raise ValueError("rowwise_xw_heads: Hd [n, heads*C], S [n, 2*heads] contiguous, a_self / a_neigh [C, heads, 1] contiguous expected")
    _launch('amar_rowwise_xw_heads_f32', *_mat(X, 'X'), F, _ptr(W, F32, 'W'), heads, C, *_mat(Hd, 'Hd'), _ptr(a_self, F32, 'a_self'),
            _ptr(a_neigh, F32, 'a_neigh'), _ptr(S, F32, 'S'), n_rows)


def _gat_heads_shapes(what, rowptr, Hd, heads, S, bias, Y, concat):
    n, HC = rowptr.numel() - 1, int(Hd.shape[1])
    if heads < 1 or HC % heads:
        raise ValueError("{}: Hd must be [n, heads*C]".format(what))
    width = HC if concat else HC // heads
    if Hd.shape[0] < n or tuple(S.shape) != (Hd.shape[0], 2 * heads) or not S.is_contiguous() or bias.numel() != width or tuple(Y.shape) != (n, width):
        raise ValueError("{}: S [n, 2*heads] contiguous, bias and Y of width {} expected".format(what, width))
    return n, HC // heads


def gat_heads(rowptr, colidx, Hd, heads, S, bias, Y, concat=True, self_loop=True, out_tape=None):
    """One multi-head GAT layer on rowwise_xw_heads' Hd / S (amar_gat_heads_f32).  concat: Y [n, heads*C], else the heads' mean,
    Y [n, C].  out_tape [n, heads*C] contiguous: the heads' outputs before the bias, which gat_heads_bwd needs under concat=False."""
    n, C = _gat_heads_shapes('gat_heads', rowptr, Hd, heads, S, bias, Y, concat)
    if out_tape is not None and (tuple(out_tape.shape) != (n, heads * C) or not out_tape.is_contiguous()):
        raise ValueError("gat_heads: out_tape must be a contiguous [n, heads*C] buffer")
    _launch('amar_gat_heads_f32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), *_mat(Hd, 'Hd'), heads, C, _ptr(S, F32, 'S'),
            _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'), _ptr(out_tape, F32, 'out_tape'), 1 if concat else 0, 1 if self_loop else 0, n)


def gat_heads_bwd(rowptr, colidx, Hd, heads, S, Y, dY, bias, a_self, a_neigh, concat=True, self_loop=True, out_tape=None, transposed=None):
    """Reverse of gat_heads (amar_gat_heads_bwd_f32).  Returns (dout [n, width of Y], dS [n, 2*heads], dHd [n, heads*C]); dS holds the
    gradients of the self scalars, then of the neighbour scalars, as S does.  transposed = (t_rowptr, t_colidx) of a directed
    structure (None: the edge multiset is symmetric and the one structure serves both walks)."""
    n, C = _gat_heads_shapes('gat_heads_bwd', rowptr, Hd, heads, S, bias, Y, concat)
    if Hd.shape[0] != n or tuple(dY.shape) != tuple(Y.shape) or a_self.numel() != C * heads or a_neigh.numel() != C * heads or \
            not a_self.is_contiguous() or not a_neigh.is_contiguous():
        raise ValueError("gat_heads_bwd: Hd [n, heads*C], dY like Y, a_self / a_neigh [C, heads, 1] contiguous expected")
    if not concat and (out_tape is None or tuple(out_tape.shape) != (n, heads * C) or not out_tape.is_contiguous()):
        raise ValueError("gat_heads_bwd: concat=False needs the forward's out_tape [n, heads*C]")
    dev = Hd.device
    dout = torch.empty(tuple(Y.shape), dtype=torch.float32, device=dev)
    scratch = torch.empty(3 * heads * n, dtype=torch.float32, device=dev)
    dS = torch.empty((n, 2 * heads), dtype=torch.float32, device=dev)
    dHd = torch.empty((n, heads * C), dtype=torch.float32, device=dev)
    structure = (_ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'))
    _launch('amar_gat_heads_bwd_f32', *structure, *(_transposed_ptrs(transposed, n, colidx) or structure), *_mat(Hd, 'Hd'), heads, C,
            _ptr(S, F32, 'S'), *_mat(Y, 'Y'), *_mat(dY, 'dY'), _ptr(bias, F32, 'bias'), _ptr(a_self, F32, 'a_self'), _ptr(a_neigh, F32, 'a_neigh'),
            _ptr(out_tape, F32, 'out_tape'), _ptr(dout), _ptr(scratch), _ptr(dS), _ptr(dHd), heads * C, 1 if concat else 0,
            1 if self_loop else 0, n)
    return dout, dS, dHd


def gat_xs(xs, H, s_self, s_neigh, bias, Y, self_loop=True):
    """gat_layer on the XCD-sliced image `xs` of the edge-list adjacency (utilities.math.XcdSliced; values unused).
    `xs` may be a row block (multi-GPU partition): H / s_self / s_neigh then cover all of its columns."""
    n, n_cols = xs.shape
    row_offset = int(getattr(xs, 'diag_offset', 0))
    C = H.shape[1]
    if tuple(Y.shape) != (n, C) or H.shape[0] != n_cols or bias.numel() != C or s_self.numel() != n_cols or s_neigh.numel() != n_cols:
        raise ValueError("gat_xs: H [n_cols, C], Y [n_rows, C], bias [C], s_self / s_neigh [n_cols] expected")
    scratch = xs.__dict__.setdefault('_gat_scratch', {})
    if C not in scratch:
        scratch[C] = (torch.empty((n_cols, 2 * C), dtype=torch.float32, device=H.device),
                      torch.empty((xs.n_slices, n, 2 * C), dtype=torch.float32, device=H.device))
    packed, partials = scratch[C]
    _launch('amar_gat_xs_f32', _ptr(xs.rowptr, I32, 'rowptr'), _ptr(xs.colidx, I32, 'colidx'), xs.n_slices, *_mat(H, 'H'), C,
            _ptr(s_self, F32, 's_self'), _ptr(s_neigh, F32, 's_neigh'), _ptr(bias, F32, 'bias'), _ptr(packed), _ptr(partials), *_mat(Y, 'Y'),
            1 if self_loop else 0, n, n_cols, row_offset)


def colmax(x, out):
    """out[0] = max(x) (a 1-element float32 device tensor), in-stream."""
    if not x.is_contiguous() or out.numel() < 1:
        raise ValueError("colmax: contiguous x and a 1-element out expected")
    _launch('amar_colmax_f32', _ptr(x, F32, 'x'), x.numel(), _ptr(out, F32, 'out'))


def gat_lt(lt, csr, H, s_self, s_neigh, bias, Y, self_loop=True):
    """gat_layer on the LDS-tiled image `lt` (utilities.lds_tiled.LdsTiled built with the GAT geometry, DeviceCSR.tiled_gat_image)
    of the edge-list adjacency `csr` (a DeviceCSR, or a row block carrying diag_offset): one launch + the bound's reduction."""
    n, n_cols = lt.shape
    row_offset = int(getattr(lt, 'diag_offset', 0))
    C = H.shape[1]
    if C != lt.F or tuple(Y.shape) != (n, C) or H.shape[0] != n_cols or bias.numel() != C or s_self.numel() != n_cols or s_neigh.numel() != n_cols:
        raise ValueError("gat_lt: H [n_cols, C], Y [n_rows, C], bias [C], s_self / s_neigh [n_cols] and an image built for C expected")
    if tuple(csr.shape) != (n, n_cols):
        raise ValueError("gat_lt: the CSR and the image must describe the same block")
    bmax = lt.__dict__.setdefault('_gat_bound', torch.empty(1, dtype=torch.float32, device=H.device))
    colmax(s_neigh, bmax)
    _launch('amar_gat_lt_f32', *_lt_image_args(lt, lt.n_tiles), int(lt.rw), _ptr(lt.diag, F32, 'diag'), _ptr(csr.rowptr, I32, 'rowptr'),
            _ptr_entries(csr.colidx, I32, 'colidx'), *_mat(H, 'H'), C, _ptr(s_self, F32, 's_self'), _ptr(s_neigh, F32, 's_neigh'), _ptr(bmax, F32, 'bmax'),
            _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'), 1 if self_loop else 0, n, n_cols, row_offset)


DENSE_WT = 0x100


def _dense_args(X, W, bias, Y, act, ids, w_transposed, check_bias):
    """The argument list of amar_dense_f32 / amar_dense_route without the last one.  check_bias: the launcher's check of the bias,
    which the route query does not make."""
    K, N = (W.shape[1], W.shape[0]) if w_transposed else W.shape
    M = ids.numel() if ids is not None else X.shape[0]
    if X.shape[1] != K or not W.is_contiguous() or tuple(Y.shape) != (M, N):
        raise ValueError("dense: X [*, K], W [K, N] contiguous, Y [M, N] expected")
    if check_bias and bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("dense: bias must be a contiguous [N] vector")
    return [*_mat(X, 'X'), _ptr(ids, I32, 'ids'), _ptr(W, F32, 'W'), _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'), M, K, N,
            ACT_CODES[act] | (DENSE_WT if w_transposed else 0)]


def dense(X, W, bias, Y, act='relu', ids=None, w_transposed=False):
    """Y = act(X[ids] . W + bias). Y may be a column slice of a wider buffer (concatenation).
    w_transposed: W holds the transpose ([N, K]), i.e. Y = X . W^T — the reverse pass' dX = dZ . W^T without a transpose launch."""
    _launch('amar_dense_f32', *_dense_args(X, W, bias, Y, act, ids, w_transposed, check_bias=True))


class DenseRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_dense_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'vec_x', 'vec_w', 'w_trans', 'grid_x', 'grid_y', 'n_col_blocks', 'launches')]
    KERNELS = {0: 'small', 1: 'tile128', 2: 'full', 3: 'guarded', -1: None}
    BOOLS = ('vec_x', 'vec_w', 'w_trans')


def dense_route(X, W, Y, act='relu', ids=None, w_transposed=False, bias=None):
    """Which kernel dense() takes for these tensors (amar_dense_route: host only, nothing is launched; the launcher asks the same
    function).  A dict: kernel 'small' | 'tile128' | 'full' | 'guarded', vec_x, vec_w, w_trans, grid_x, grid_y, n_col_blocks, launches."""
    info = DenseRouteInfo()
    _call('amar_dense_route', *_dense_args(X, W, bias, Y, act, ids, w_transposed, check_bias=False), ctypes.byref(info))
    return info.as_dict()


def dense_split_supported(K, N):
    """amar_dense_split_f32 takes this layer (the wide layers of the content towers); AMAR_DENSE_SPLIT=0 keeps the f32 instruction."""
    return K % 32 == 0 and N % 128 == 0 and K >= 32 and os.environ.get('AMAR_DENSE_SPLIT', '1') != '0'


def dense_split_pack(W):
    """Kernel [K, N] (host numpy float32) -> the pre-split image of amar_dense_split_pack_f32 as a uint8 numpy array."""
    import numpy as np
    W = np.ascontiguousarray(W, dtype=np.float32)
    K, N = W.shape
    nbytes = int(load().amar_dense_split_bytes(K, N))
    if nbytes < 0:
        _check(nbytes, 'amar_dense_split_bytes')
    out = np.empty(nbytes, dtype=np.uint8)
    _call('amar_dense_split_pack_f32', W.ctypes.data, K, N, out.ctypes.data)
    return out


def dense_split(X, Wq, K, N, bias, Y, act='relu', ids=None):
    """Y = act(X[ids] . W + bias) with W pre-split (dense_split_pack, on the device as uint8): amar_dense_split_f32."""
    M = ids.numel() if ids is not None else X.shape[0]
    if X.shape[1] != K or tuple(Y.shape) != (M, N) or Wq.numel() != K * N * 6 or Wq.dtype != torch.uint8 or not Wq.is_contiguous():
        raise ValueError("dense_split: X [*, K], Wq of K N 6 bytes, Y [M, N] expected")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("dense_split: bias must be a contiguous [N] vector")
    _launch('amar_dense_split_f32', *_mat(X, 'X'), _ptr(ids, I32, 'ids'), _ptr(Wq, torch.uint8, 'Wq'), _ptr(bias, F32, 'bias'), *_mat(Y, 'Y'),
            M, K, N, ACT_CODES[act])


CHAIN_MAX_WIDTH, CHAIN_MAX_LAYERS, CHAIN_MAX_BLOB_BYTES = 128, 8, 150 * 1024


def chain_supported(dims, in_a, in_b=0, sum_inputs=False):
    """True when amar_chain_f32 can run a dense stack with these widths (else use dense() per layer): the width, layer-count and
    alignment limits of include/amar_hip.h, and a packed blob (amar_chain_pack_floats) of at most 150 KB — three 128 x 128 layers
    are too many."""
    width_in = in_a if sum_inputs else in_a + in_b
    if not (1 <= len(dims) - 1 <= CHAIN_MAX_LAYERS and min(dims) >= 1 and max(dims) <= CHAIN_MAX_WIDTH and in_a % 4 == 0 and in_a >= 4
            and in_b % 4 == 0 and dims[0] == width_in and (not sum_inputs or in_a == in_b)
            and (dims[-1] % 4 == 0 or (dims[-1] == 1 and len(dims) > 2))):
        return False
    floats = load().amar_chain_pack_floats((ctypes.c_int32 * len(dims))(*dims), len(dims) - 1)
    return 0 < 4 * floats <= CHAIN_MAX_BLOB_BYTES


def chain_pack(kernels, biases):
    """Host-side packing of a Dense stack into MFMA fragment order; returns a device float32 blob + dims."""
    import numpy as np
    ks = [np.ascontiguousarray(k, dtype=np.float32) for k in kernels]
    bs = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
    dims = [ks[0].shape[0]] + [k.shape[1] for k in ks]
    for k, b, kin, n in zip(ks, bs, dims[:-1], dims[1:]):
        if k.shape != (kin, n) or b.shape != (n,):
            raise ValueError("chain_pack: inconsistent layer shapes")
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    total = load().amar_chain_pack_floats(dims_c, len(ks))
    if total < 0:
        _check(int(total), 'amar_chain_pack_floats')
    out = np.empty(total, dtype=np.float32)
    kp = (ctypes.c_void_p * len(ks))(*[k.ctypes.data for k in ks])
    bp = (ctypes.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    _call('amar_chain_pack_f32', kp, bp, dims_c, len(ks), out.ctypes.data)
    return out, dims


class ConcatTable:
    """The column-wise concatenation of several [rows, w_j] device tables with the same row numbering, NOT materialised: what
    ReductionLayer('concatenation') hands to the towers when every layer's output stays where its producer (or the all-gather of a
    node-range partition) left it.  `chain` reads it in place (amar_chain_segments_f32) where the stack has a compile-time tower
    shape and assembles it once otherwise (`materialize`)."""

    def __init__(self, tables):
        tables = list(tables)
        if not tables:
            raise ValueError("ConcatTable: at least one table expected")
        rows = int(tables[0].shape[0])
        if any(t.dim() != 2 or int(t.shape[0]) != rows or t.dtype != torch.float32 for t in tables):
            raise ValueError("ConcatTable: float32 [rows, w] tables with equal row counts expected")
        # the segment-reading kernel moves float4s: tables whose widths are not multiples of 4 are assembled once instead (`chain`)
        self.in_place = all(int(t.shape[1]) % 4 == 0 for t in tables)
        self.segments = tables
        self.shape = (rows, sum(int(t.shape[1]) for t in tables))
        self.device, self.dtype = tables[0].device, torch.float32

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("ConcatTable supports contiguous row slices only")
        return ConcatTable([t[key] for t in self.segments])

    def materialize(self):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        off = 0
        for t in self.segments:
            copy_columns(t, out[:, off:off + t.shape[1]])
            off += t.shape[1]
        return out


def _chain_segments_args(table, wpack, dims, acts, out, ids=None, base=0):
    P = out.shape[0]
    segs = table.segments
    if ids is not None and ids.numel() != P:
        raise ValueError("chain: ids must have one id per output row")
    if ids is None and table.shape[0] < P:
        raise ValueError("chain: input blocks have fewer rows than the output")
    n = len(segs)
    ptrs = (ctypes.c_void_p * n)(*[_ptr(t, F32, 'segment') for t in segs])
    lds = (ctypes.c_int64 * n)(*[_ld(t, 'segment') for t in segs])
    ws = (ctypes.c_int32 * n)(*[int(t.shape[1]) for t in segs])
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    acts_c = (ctypes.c_int32 * len(acts))(*[ACT_CODES[a] for a in acts])
    return [ptrs, lds, ws, n, _ptr(ids, I32, 'ids'), int(base), _ptr(wpack, F32, 'wpack'), dims_c, acts_c, len(acts), *_mat(out, 'out'), P]


def chain_segments(table, wpack, dims, acts, out, ids=None, base=0):
    """`chain` on a ConcatTable read in place; returns False when the stack's shape has no segment-reading kernel."""
    code = load().amar_chain_segments_f32(*_chain_segments_args(table, wpack, dims, acts, out, ids=ids, base=base), _stream())
    if code == -2:                                                   # AMAR_EUNSUPPORTED: no compile-time tower shape for this stack
        return False
    _check(code, 'amar_chain_segments_f32')
    return True


def _chain_args(A, wpack, dims, acts, out, ids_a=None, base_a=0, B=None, ids_b=None, base_b=0, sum_inputs=False, in_act=None, out_index=None):
    P = out.shape[0]
    Da, Db = A.shape[1], (B.shape[1] if B is not None else 0)
    for ids, nm in ((ids_a, 'ids_a'), (ids_b, 'ids_b')):
        if ids is not None and ids.numel() != P:
            raise ValueError("chain: {} must have one id per output row".format(nm))
    if ids_a is None and A.shape[0] < P or (B is not None and ids_b is None and B.shape[0] < P):
        raise ValueError("chain: input blocks have fewer rows than the output")
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    acts_c = (ctypes.c_int32 * len(acts))(*[ACT_CODES[a] for a in acts])
    if out_index is not None and out_index.numel() != P:
        raise ValueError("chain: out_index must have one entry per output row")
    return [*_mat(A, 'A'), Da, _ptr(ids_a, I32, 'ids_a'), int(base_a), *_mat(B, 'B'), Db, _ptr(ids_b, I32, 'ids_b'), int(base_b),
            1 if sum_inputs else 0, ACT_CODES[in_act], _ptr(wpack, F32, 'wpack'), dims_c, acts_c, len(acts),
            *_mat(out, 'out'), _ptr(out_index, I32, 'out_index'), P]


def chain(A, wpack, dims, acts, out, ids_a=None, base_a=0, B=None, ids_b=None, base_b=0, sum_inputs=False, in_act=None, out_index=None):
    """out = DenseStack([A[ids_a - base_a] || B[ids_b - base_b]]), or DenseStack(in_act(A[..] + B[..])) with
    sum_inputs; see amar_chain_f32 in include/amar_hip.h.  out_index (int32 [P]): row p goes to out[out_index[p]]
    (amar_chain_indexed_f32: a pair list kept in XCD-affine order, scores back in the caller's order).
    A may be a ConcatTable (per-layer tables read in place: amar_chain_segments_f32)."""
    if isinstance(A, ConcatTable):
        if A.in_place and B is None and not sum_inputs and out_index is None and chain_segments(A, wpack, dims, acts, out, ids=ids_a, base=base_a):
            return
        A = A.materialize()
    together = chain_together.active
    if together is not None and ids_a is None and B is None and not sum_inputs and out_index is None:
        together.calls.append((A, wpack, list(dims), list(acts), out))      # a one-table call on the rows themselves: launched at the block's end
        return
    _chain_launch(A, wpack, dims, acts, out, ids_a=ids_a, base_a=base_a, B=B, ids_b=ids_b, base_b=base_b, sum_inputs=sum_inputs,
                  in_act=in_act, out_index=out_index)


def _chain_launch(A, wpack, dims, acts, out, **kw):
    args = _chain_args(A, wpack, dims, acts, out, **kw)
    _check(load().amar_chain_indexed_f32(*args, _stream()), 'amar_chain_indexed_f32' if kw.get('out_index') is not None else 'amar_chain_f32')


class chain_together:
    """`with chain_together():` — the one-table `chain` calls made inside the block (rows themselves: no ids, no second table, no output
    index) are held back and launched when the block ends: two of them in ONE launch (`chain2`) where the launcher's route takes them
    (and AMAR_TOWERS_LAUNCH is not 'two'), else each on its own, in the order of the calls.  The outputs are defined after the block;
    every other `chain` call launches at once.  The same bits either way.
    Why the holding back sits inside `chain` and the caller does not call `chain2` itself: `chain` is the one place that decides
    what a table is (a ConcatTable read in place, or assembled first) and the one call the launch-recording tests and tools wrap —
    a caller keeps making one `chain` call per stack, whichever way they are launched."""
    active = None

    def __enter__(self):
        self.calls, self.outer = [], chain_together.active
        chain_together.active = self
        return self

    def __exit__(self, exc_type, exc, tb):
        chain_together.active = self.outer
        if exc_type is not None:
            return False
        calls = self.calls
        if len(calls) == 2:
            # (chain2 asks the launcher's route itself and launches nothing where it declines)
            if os.environ.get('AMAR_TOWERS_LAUNCH', '') != 'two' and len(calls[0][3]) == len(calls[1][3]) and chain2(calls[0], calls[1]):
                return False
        for A, wpack, dims, acts, out in calls:
            _chain_launch(A, wpack, dims, acts, out)
        return False


CHAIN_KERNEL_GENERIC, CHAIN_KERNEL_PIPE, CHAIN_KERNEL_ROWS = 0, 1, 2


class ChainRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_chain_route_info (`kernel` stays a CHAIN_KERNEL_* code)"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'maxt', 'full', 'am', 'split', 'scatter', 'shape', 'lastlin', 'seg', 'has_dot',
                                                    'layers', 'threads')] + [('blocks', ctypes.c_int64), ('lds_bytes', ctypes.c_int64)]
    BOOLS = ('full', 'split', 'scatter', 'lastlin', 'seg', 'has_dot')


def chain_shape(*tiles):
    """The `shape` of ChainRouteInfo for a tower whose widths dims[0..n] have these tile counts (n = len(tiles) - 1 layers)."""
    code = len(tiles) - 1
    for j, t in enumerate(tiles):
        code |= t << (3 * (j + 1))
    return code


def chain_route(A, wpack, dims, acts, out, ids_a=None, base_a=0, B=None, ids_b=None, base_b=0, sum_inputs=False, in_act=None, out_index=None):
    """What `chain` does with these operands (amar_chain_route / amar_chain_segments_route: host only, nothing is launched; the
    launchers start from the same function).  A dict of the fields of amar_chain_route_info.  A ConcatTable is asked about in
    place: a shape without a segment-reading kernel raises AmarError (`chain` then assembles the table and runs that)."""
    info = ChainRouteInfo()
    if isinstance(A, ConcatTable):
        if not (A.in_place and B is None and not sum_inputs and out_index is None):
            raise ValueError("chain_route: this ConcatTable call is assembled first; ask about the assembled table")
        args = _chain_segments_args(A, wpack, dims, acts, out, ids=ids_a, base=base_a)
        _call('amar_chain_segments_route', *args, ctypes.byref(info))
        return info.as_dict()
    args = _chain_args(A, wpack, dims, acts, out, ids_a=ids_a, base_a=base_a, B=B, ids_b=ids_b, base_b=base_b, sum_inputs=sum_inputs,
                       in_act=in_act, out_index=out_index)
    _call('amar_chain_route', *args, ctypes.byref(info))
    return info.as_dict()


class ChainRows2RouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_chain_rows2_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('one_launch', 'shape', 'lastlin', 'threads')] + [('blocks', ctypes.c_int64 * 2),
                                                                                                 ('lds_bytes', ctypes.c_int64)]
    BOOLS = ('one_launch', 'lastlin')

    def as_dict(self):
        d = super().as_dict()
        d['blocks'] = tuple(d['blocks'])                                # the two problems' block counts as a pair
        return d


def _chain2_raw(ptrs_a, ldas, ptrs_w, dims, acts, ptrs_out, ldos, rows):
    """The argument list of amar_chain_rows2_f32 / _route from plain numbers: two entries each (addresses as ints)."""
    if len(acts[0]) != len(acts[1]) or any(len(d) != len(a) + 1 for d, a in zip(dims, acts)):
        raise ValueError("chain2: both stacks need the same number of layers, dims one entry longer than acts")
    keep = [(ctypes.c_int32 * len(d))(*d) for d in dims] + [(ctypes.c_int32 * len(a))(*[ACT_CODES[x] for x in a]) for a in acts]
    vp = lambda vals: (ctypes.c_void_p * 2)(*vals)                                                # noqa: E731
    i64 = lambda vals: (ctypes.c_int64 * 2)(*[int(v) for v in vals])                               # noqa: E731
    args = [vp(ptrs_a), i64(ldas), vp(ptrs_w), vp([ctypes.addressof(keep[0]), ctypes.addressof(keep[1])]),
            vp([ctypes.addressof(keep[2]), ctypes.addressof(keep[3])]), len(acts[0]), vp(ptrs_out), i64(ldos), i64(rows)]
    return args, keep


def _chain2_args(first, second):
    """first / second: (A, wpack, dims, acts, out) as `chain` takes them, rows themselves."""
    for A, _, _, _, out in (first, second):
        if A.shape[0] < out.shape[0]:
            raise ValueError("chain2: input blocks have fewer rows than the output")
    both = (first, second)
    return _chain2_raw([_ptr(p[0], F32, 'A') for p in both], [_ld(p[0], 'A') for p in both],
                       [_ptr(p[1], F32, 'wpack') for p in both], [p[2] for p in both], [p[3] for p in both],
                       [_ptr(p[4], F32, 'out') for p in both], [_ld(p[4], 'out') for p in both], [p[4].shape[0] for p in both])


def chain2(first, second):
    """Two `chain` calls on one table each — first / second = (A, wpack, dims, acts, out), rows themselves — in ONE launch
    (amar_chain_rows2_f32: the workgroups of one grid dealt to the two problems by their rows; the same bits as two `chain` calls).
    Returns False, with nothing launched, where chain2_route says one_launch is off: make two `chain` calls."""
    args, keep = _chain2_args(first, second)
    code = load().amar_chain_rows2_f32(*args, _stream())
    if code == -2:                                                   # AMAR_EUNSUPPORTED: not one compile-time tower kernel for both
        return False
    _check(code, 'amar_chain_rows2_f32')
    return True


def chain2_route(first, second):
    """What `chain2` does with these operands (amar_chain_rows2_route: host only, nothing is launched): a dict of the fields of
    amar_chain_rows2_route_info.  one_launch False: make two `chain` calls."""
    info = ChainRows2RouteInfo()
    args, keep = _chain2_args(first, second)
    _call('amar_chain_rows2_route', *args, ctypes.byref(info))
    return info.as_dict()


_MADE_UP = 0x7F0000100000      # a 16-byte aligned address: the route functions look at alignment and NULL only


def towers_route(u_dims, u_acts, u_rows, i_dims, i_acts, i_rows, u_ids=False, i_ids=False, info=False):
    """How BasicRS.towers launches its two stacks: 'one' (chain2: both towers in one grid) or 'two' (a `chain` call each).  Host only:
    needs no GPU (the same route function as the launcher's, asked with dense tables at made-up addresses).  'one' needs both stacks
    on the same compile-time tower kernel (ChainRouteInfo: kernel ROWS, equal shape / lastlin), rows on both sides and no id lists;
    AMAR_TOWERS_LAUNCH=two keeps the two launches.  info=True: (route, the dict of amar_chain_rows2_route_info or None)."""
    route, d = 'two', None
    if (os.environ.get('AMAR_TOWERS_LAUNCH', '') != 'two' and not u_ids and not i_ids and len(u_acts) == len(i_acts)
            and len(u_dims) == len(u_acts) + 1 and len(i_dims) == len(i_acts) + 1):
        dims, acts = (list(u_dims), list(i_dims)), (list(u_acts), list(i_acts))
        pad4 = lambda w: (int(w) + 3) // 4 * 4                                                     # noqa: E731
        args, keep = _chain2_raw([_MADE_UP, _MADE_UP + (1 << 40)], [pad4(d_[0]) for d_ in dims], [_MADE_UP + (2 << 40), _MADE_UP + (3 << 40)],
                                 dims, acts, [_MADE_UP + (4 << 40), _MADE_UP + (5 << 40)], [pad4(d_[-1]) for d_ in dims], [u_rows, i_rows])
        r = ChainRows2RouteInfo()
        if load().amar_chain_rows2_route(*args, ctypes.byref(r)) == 0:
            d = r.as_dict()
            route = 'one' if d['one_launch'] else 'two'
    return (route, d) if info else route


def dual_chain_supported(D, n_branch_dims_equal, trunk_dims):
    return (D % 16 == 0 and D <= 64 and n_branch_dims_equal and len(trunk_dims) >= 3 and trunk_dims[0] == 2 * D
            and trunk_dims[-1] == 1 and len(set(trunk_dims[1:-1])) == 1 and trunk_dims[1] <= 64 and trunk_dims[1] % 4 == 0)


def dual_chain(tables_a, tables_b, ids_a, ids_b, bases_a, bases_b, D, in_act, branch_acts, trunk_dims, trunk_acts, wpack, out,
               out_index=None):
    """Fused two-branch head: see amar_dual_chain_f32. tables_* / ids_* / bases_* are 2-element sequences; out_index (int32 [P]):
    pair p goes to out[out_index[p]] (amar_dual_chain_indexed_f32)."""
    P = out.shape[0]
    arr = lambda vals, ctype: (ctype * 2)(*vals)
    A = arr([_ptr(t, F32, 'A') for t in tables_a], ctypes.c_void_p)
    B = arr([_ptr(t, F32, 'B') for t in tables_b], ctypes.c_void_p)
    IA = arr([_ptr(t, I32, 'ida') for t in ids_a], ctypes.c_void_p)
    IB = arr([_ptr(t, I32, 'idb') for t in ids_b], ctypes.c_void_p)
    for ids in list(ids_a) + list(ids_b):
        if ids is not None and ids.numel() != P:
            raise ValueError("dual_chain: one id per output row expected")
    lda = arr([_ld(t, 'A') for t in tables_a], ctypes.c_int64)
    ldb = arr([_ld(t, 'B') for t in tables_b], ctypes.c_int64)
    ba, bb = arr([int(b) for b in bases_a], ctypes.c_int32), arr([int(b) for b in bases_b], ctypes.c_int32)
    bacts = (ctypes.c_int32 * max(1, len(branch_acts)))(*[ACT_CODES[a] for a in branch_acts])
    tdims = (ctypes.c_int32 * len(trunk_dims))(*trunk_dims)
    tacts = (ctypes.c_int32 * len(trunk_acts))(*[ACT_CODES[a] for a in trunk_acts])
    if out_index is not None and out_index.numel() != P:
        raise ValueError("dual_chain: out_index must have one entry per output row")
    # (one entry point serves both: without an index the error names the call the caller made, amar_dual_chain_f32 — hence no _launch)
    _check(load().amar_dual_chain_indexed_f32(A, lda, IA, ba, B, ldb, IB, bb, D, ACT_CODES[in_act], len(branch_acts), bacts, tdims, tacts,
                                              len(trunk_acts), _ptr(wpack, F32, 'wpack'), *_mat(out, 'out'), _ptr(out_index, I32, 'out_index'),
                                              P, _stream()),
           'amar_dual_chain_f32' if out_index is None else 'amar_dual_chain_indexed_f32')


SCATTER_CLOSED_MAX_WINDOW = 65536      # include/amar_hip.h: AMAR_SCATTER_CLOSED_MAX_WINDOW


def scatter_route(n, ldd, max_window, closed):
    """Which form `scatter` takes: 'lds' (amar_scatter_closed_f32: every window finished on chip, whole-line stores) or 'global'
    (amar_scatter_f32: one store per score).  Host only.  'lds' needs the caller's promise (`closed`: every window's indices are a
    bijection onto the window's own range), a dense destination (ldd == 1), something to move, and no window longer than
    SCATTER_CLOSED_MAX_WINDOW (`max_window`: the longest window, known on the host); AMAR_PAIR_SCATTER=global keeps the global form."""
    if os.environ.get('AMAR_PAIR_SCATTER', '') == 'global':
        return 'global'
    if not closed or int(ldd) != 1 or int(n) <= 0 or max_window is None or not 1 <= int(max_window) <= SCATTER_CLOSED_MAX_WINDOW:
        return 'global'
    return 'lds'


def scatter(src, index, dst, window_off=None, n_windows=1, closed=False, max_window=None):
    """dst[index[t]] = src[t] (rows of a [n, 1] / [n] float32 destination), window by window: see amar_scatter_f32.  closed=True with
    max_window (the longest window): the caller's promise of amar_scatter_closed_f32, taken where scatter_route says 'lds'."""
    n = int(index.numel())
    if src.numel() < n or (window_off is not None and window_off.numel() != n_windows + 1):
        raise ValueError("scatter: one source value per index and n_windows + 1 window offsets expected")
    if n == 0:
        return
    ldd = _ld(dst, 'dst') if dst.dim() == 2 else 1
    if window_off is not None and scatter_route(n, ldd, max_window, closed) == 'lds':
        _launch('amar_scatter_closed_f32', _ptr(src, F32, 'src'), _ptr(index, I32, 'index'), _ptr(dst, F32, 'dst'), n, _ptr(window_off, I32, 'window_off'),
                int(n_windows), int(max_window))
        return
    _launch('amar_scatter_f32', _ptr(src, F32, 'src'), _ptr(index, I32, 'index'), _ptr(dst, F32, 'dst'), ldd, n, _ptr(window_off, I32, 'window_off'),
            int(n_windows))


def copy_columns(src, dst, ids=None, base=0):
    """dst[r, :] = src[ids[r] - base, :] (or src[r, :] without ids); dst may be a column slice."""
    n = ids.numel() if ids is not None else src.shape[0]
    if src.shape[1] != dst.shape[1] or dst.shape[0] != n:
        raise ValueError("copy_columns: shapes differ")
    _launch('amar_copy_columns_f32', *_mat(src, 'src'), _ptr(ids, I32, 'ids'), int(base), *_mat(dst, 'dst'), n, src.shape[1])


def reduce_layers(cat, n_layers, width, out, mean=False):
    if cat.shape[1] != n_layers * width or tuple(out.shape) != (cat.shape[0], width):
        raise ValueError("reduce_layers: cat [n, n_layers*width], out [n, width] expected")
    _launch('amar_reduce_layers_f32', *_mat(cat, 'cat'), n_layers, width, *_mat(out, 'out'), cat.shape[0], 1 if mean else 0)


def reduce_layers_wsum(cat, n_layers, width, w, out):
    """out = sum_l (w_l * w_l) * cat[:, block l]  (ReductionLayer('w-sum'), reduction.py:36-55); w: device vector of n_layers floats."""
    if cat.shape[1] != n_layers * width or tuple(out.shape) != (cat.shape[0], width) or w.numel() != n_layers or not w.is_contiguous():
        raise ValueError("reduce_layers_wsum: cat [n, n_layers*width], w [n_layers], out [n, width] expected")
    _launch('amar_reduce_layers_wsum_f32', *_mat(cat, 'cat'), n_layers, width, _ptr(w, F32, 'w'), *_mat(out, 'out'), cat.shape[0])


def reduce_layers_wsum_bwd(cat, n_layers, width, w, d_out, d_cat, dw):
    """Reverse of reduce_layers_wsum: d_cat[:, block l] = w_l^2 d_out, dw[l] = 2 w_l sum(d_out . cat[:, block l]) (deterministic)."""
    n = cat.shape[0]
    if (cat.shape[1] != n_layers * width or tuple(d_cat.shape) != tuple(cat.shape) or tuple(d_out.shape) != (n, width)
            or w.numel() != n_layers or dw.numel() != n_layers or not w.is_contiguous() or not dw.is_contiguous()):
        raise ValueError("reduce_layers_wsum_bwd: cat / d_cat [n, n_layers*width], d_out [n, width], w / dw [n_layers] expected")
    scratch = torch.empty(int(load().amar_reduce_layers_wsum_bwd_scratch()), dtype=torch.float32, device=cat.device)
    _launch('amar_reduce_layers_wsum_bwd_f32', *_mat(cat, 'cat'), n_layers, width, _ptr(w, F32, 'w'), *_mat(d_out, 'd_out'),
            *_mat(d_cat, 'd_cat'), _ptr(dw, F32, 'dw'), _ptr(scratch, F32, 'scratch'), n)


def adam_advance(state, learning_rate, beta_1, beta_2):
    if state.numel() != 2 or not state.is_contiguous():
        raise ValueError("adam_advance: state must be 2 contiguous floats (t, lr_t)")
    _launch('amar_adam_advance_f32', _ptr(state, F32, 'state'), float(learning_rate), float(beta_1), float(beta_2))


def adam_dev(w, g, m, v, state, beta_1, beta_2, epsilon, l2=0.0):
    if not (w.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()) or \
            not (w.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adam_dev: contiguous tensors of equal size expected")
    _launch('amar_adam_dev_f32', _ptr(w, F32, 'w'), _ptr(g, F32, 'g'), _ptr(m, F32, 'm'), _ptr(v, F32, 'v'), w.numel(), _ptr(state, F32, 'state'), float(beta_1),
            float(beta_2), float(epsilon), float(l2))


class DeferredGradient:
    """A weight / bias gradient still in partial sums: `partials` [groups, n] (a view of a dense_bwd workspace), to be added in group
    order by its consumer (adam_slot_table -> amar_adam_multi_f32's g_groups).  `materialize()` adds them on the spot."""

    def __init__(self, partials, groups, shape):
        self.partials, self.groups, self.shape = partials, int(groups), tuple(shape)

    def materialize(self):
        """The sum in GROUP ORDER, starting from 0 — the order of the library's own reduction, so the bits are those of a call without
        `defer` (a library-chosen order, as torch.sum's, need not be)."""
        parts = self.partials.view(self.groups, -1)
        total = torch.zeros_like(parts[0])
        for g in range(self.groups):
            total += parts[g]
        return total.view(self.shape)


def flat_gradient(g):
    """A gradient as adam_slot_table takes it: a DeferredGradient as it is, a tensor flat and contiguous."""
    return g if isinstance(g, DeferredGradient) else g.contiguous().view(-1)


class AdamSlot(ctypes.Structure):
    """include/amar_hip.h: amar_adam_slot"""
    _fields_ = [('w', ctypes.c_void_p), ('g', ctypes.c_void_p), ('m', ctypes.c_void_p), ('v', ctypes.c_void_p),
                ('n', ctypes.c_int64), ('first_block', ctypes.c_int64), ('l2', ctypes.c_float), ('g_groups', ctypes.c_int32)]


def _slot_table(struct, entries, name, expected, checked=True):
    """The slot table of a multi-tensor launch over `struct` (amar_adam_slot, amar_optim_slot, amar_clip_slot: w, g, the struct's state
    pointers, n, first_block, l2, g_groups).  entries: [(w, g, state arrays, l2)], g a tensor or a DeferredGradient; every parameter takes
    (n + 1023) // 1024 blocks.  name / expected word the errors; checked: pointers through `_ptr` (on the device, float32).
    Returns (host uint8 tensor holding the table, total blocks)."""
    table = (struct * len(entries))()
    n_arrays = len(struct._fields_) - 6
    ptr = (lambda t, what: _ptr(t, F32, what)) if checked else (lambda t, what: t.data_ptr())
    block = 0
    for k, (w, g, arrays, l2) in enumerate(entries):
        groups = 0
        if isinstance(g, DeferredGradient):                          # partial gradients [groups][n] left by dense_bwd(defer=True)
            g, groups = g.partials, g.groups
            if g.numel() != groups * w.numel():
                raise ValueError("{}: deferred gradient of the wrong size".format(name))
        elif g.numel() != w.numel():
            raise ValueError("{}: gradient of the wrong size".format(name))
        arrays = list(arrays)
        if len(arrays) > n_arrays or not all(t.is_contiguous() for t in [w, g] + arrays) or not all(a.numel() == w.numel() for a in arrays):
            raise ValueError("{}: {}".format(name, expected))
        states = [ptr(a, 'state array') for a in arrays] + [None] * (n_arrays - len(arrays))
        table[k] = struct(ptr(w, 'w'), ptr(g, 'g'), *states, w.numel(), block, float(l2), int(groups))
        block += (w.numel() + 1023) // 1024
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).clone(), block


def adam_slot_table(entries):
    """entries: [(w, g, m, v, l2)] contiguous fp32 tensors -> (host uint8 tensor holding the slot table, total blocks)."""
    return _slot_table(AdamSlot, [(w, g, (m, v), l2) for w, g, m, v, l2 in entries], 'adam_slot_table',
                       'contiguous tensors of equal size expected', checked=False)


def adam_multi(table_dev, n_slots, total_blocks, state, beta_1, beta_2, epsilon, reg_scale=0.0, loss_acc=None):
    _launch('amar_adam_multi_f32', ctypes.c_void_p(table_dev.data_ptr()), n_slots, total_blocks, _ptr(state, F32, 'state'),
            float(beta_1), float(beta_2), float(epsilon), float(reg_scale), _ptr(loss_acc, F32, 'loss_acc'))


# ---- the optimizers as rules (include/amar_hip.h: AMAR_OPT_*) --------------------------------------------------------------------------
OPT_SGD, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADAMAX, OPT_NADAM, OPT_AMSGRAD, OPT_ADAM = 1, 2, 3, 4, 5, 6, 7
OPT_NESTEROV, OPT_CENTERED = 0x100, 0x200
OPTIM_STATE_FLOATS = 8


class OptimHyper(ctypes.Structure):
    """include/amar_hip.h: amar_optim_hyper (a host struct; a rule ignores the members it does not use)"""
    _fields_ = [(name, ctypes.c_float) for name in ('learning_rate', 'momentum', 'rho', 'beta_1', 'beta_2', 'epsilon')]


def optim_hyper(learning_rate=0.001, momentum=0.0, rho=0.9, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    return OptimHyper(float(learning_rate), float(momentum), float(rho), float(beta_1), float(beta_2), float(epsilon))


class OptimSlot(ctypes.Structure):
    """include/amar_hip.h: amar_optim_slot"""
    _fields_ = [('w', ctypes.c_void_p), ('g', ctypes.c_void_p), ('s0', ctypes.c_void_p), ('s1', ctypes.c_void_p), ('s2', ctypes.c_void_p),
                ('n', ctypes.c_int64), ('first_block', ctypes.c_int64), ('l2', ctypes.c_float), ('g_groups', ctypes.c_int32)]


def optim_state_arrays(rule, flags=0, momentum=0.0):
    """How many state arrays (0 .. 3) a parameter needs under this rule."""
    count = load().amar_optim_state_arrays(int(rule), int(flags), float(momentum))
    _check(count if count < 0 else 0, 'amar_optim_state_arrays')
    return count


def optim_advance(state, rule, flags, hyper):
    if state.numel() != OPTIM_STATE_FLOATS or not state.is_contiguous():
        raise ValueError("optim_advance: state must be {} contiguous floats".format(OPTIM_STATE_FLOATS))
    _launch('amar_optim_advance_f32', _ptr(state, F32, 'state'), int(rule), int(flags), ctypes.byref(hyper))


def optim(rule, flags, hyper, w, g, arrays, state, l2=0.0):
    """One tensor under `rule`: arrays = its state arrays in the header's order (the first optim_state_arrays are used)."""
    arrays = list(arrays) + [None] * (3 - len(arrays))
    if not all(t.is_contiguous() and t.numel() == w.numel() for t in [w, g] + [a for a in arrays if a is not None]):
        raise ValueError("optim: contiguous tensors of equal size expected")
    if state.numel() != OPTIM_STATE_FLOATS:
        raise ValueError("optim: state must be {} floats".format(OPTIM_STATE_FLOATS))
    _launch('amar_optim_f32', int(rule), int(flags), ctypes.byref(hyper), _ptr(w, F32, 'w'), _ptr(g, F32, 'g'), _ptr(arrays[0], F32, 's0'),
            _ptr(arrays[1], F32, 's1'), _ptr(arrays[2], F32, 's2'), w.numel(), _ptr(state, F32, 'state'), float(l2))


def optim_slot_table(entries):
    """entries: [(w, g, [state arrays], l2)] contiguous fp32 tensors (g: a tensor or a DeferredGradient) -> (host uint8 tensor holding the
    slot table, total blocks): adam_slot_table for amar_optim_multi_f32."""
    return _slot_table(OptimSlot, entries, 'optim_slot_table', 'at most three state arrays, contiguous tensors of equal size expected')


def optim_multi(rule, flags, hyper, table_dev, n_slots, total_blocks, state, reg_scale=0.0, loss_acc=None):
    if state.numel() != OPTIM_STATE_FLOATS:
        raise ValueError("optim_multi: state must be {} floats".format(OPTIM_STATE_FLOATS))
    _launch('amar_optim_multi_f32', int(rule), int(flags), ctypes.byref(hyper), ctypes.c_void_p(table_dev.data_ptr()), n_slots,
            total_blocks, _ptr(state, F32, 'state'), float(reg_scale), _ptr(loss_acc, F32, 'loss_acc'))


# ---- learning-rate schedules (include/amar_hip.h: AMAR_LR_*) ---------------------------------------------------------------------------
LR_CONSTANT, LR_EXPONENTIAL, LR_INVERSE_TIME, LR_POLYNOMIAL, LR_COSINE, LR_PIECEWISE = 0, 1, 2, 3, 4, 5
LR_STAIRCASE, LR_CYCLE = 0x1, 0x2
LR_MAX_BOUNDARIES, LR_STATE_FLOATS, LR_MAX_STEP = 16, 2, 1 << 24
LR_KINDS = {'constant': LR_CONSTANT, 'exponential': LR_EXPONENTIAL, 'inverse_time': LR_INVERSE_TIME, 'polynomial': LR_POLYNOMIAL,
            'cosine': LR_COSINE, 'piecewise': LR_PIECEWISE}


class LrSchedule(ctypes.Structure):
    """include/amar_hip.h: amar_lr_schedule (a host struct; a kind ignores the members it does not use)"""
    _fields_ = [('kind', ctypes.c_int32), ('flags', ctypes.c_int32)] + \
               [(name, ctypes.c_float) for name in ('initial_learning_rate', 'decay_steps', 'decay_rate', 'end_learning_rate', 'power', 'alpha')] + \
               [('n_boundaries', ctypes.c_int32), ('boundaries', ctypes.c_float * LR_MAX_BOUNDARIES),
                ('values', ctypes.c_float * (LR_MAX_BOUNDARIES + 1))]


def lr_schedule(schedule=None):
    """The amar_lr_schedule of a host schedule: None -> AMAR_LR_CONSTANT (the rate is lr_state[0]); else an object of
    utilities/schedules.py, or anything whose `device_args()` returns {'kind': a name of LR_KINDS, 'staircase' / 'cycle': bool, the
    struct's float members by name, 'boundaries', 'values'} — what is left out stays zero."""
    if schedule is None:
        return LrSchedule(LR_CONSTANT, 0)
    args = dict(schedule.device_args())
    kind = args.pop('kind')
    if kind not in LR_KINDS:
        raise ValueError("lr_schedule: no schedule kind '{}': one of {}".format(kind, ', '.join(sorted(LR_KINDS))))
    flags = (LR_STAIRCASE if args.pop('staircase', False) else 0) | (LR_CYCLE if args.pop('cycle', False) else 0)
    boundaries, values = list(args.pop('boundaries', ())), list(args.pop('values', ()))
    if len(boundaries) > LR_MAX_BOUNDARIES:
        raise ValueError("lr_schedule: at most {} boundaries (got {})".format(LR_MAX_BOUNDARIES, len(boundaries)))
    if LR_KINDS[kind] == LR_PIECEWISE and len(values) != len(boundaries) + 1:
        raise ValueError("lr_schedule: a piecewise schedule needs one value more than boundaries")
    out = LrSchedule(LR_KINDS[kind], flags)
    for name, value in args.items():
        if name not in ('initial_learning_rate', 'decay_steps', 'decay_rate', 'end_learning_rate', 'power', 'alpha'):
            raise ValueError("lr_schedule: amar_lr_schedule has no member '{}'".format(name))
        setattr(out, name, float(value))
    out.n_boundaries = len(boundaries)
    for k, b in enumerate(boundaries):
        out.boundaries[k] = float(b)
    for k, v in enumerate(values):
        out.values[k] = float(v)
    return out


def _lr_state(lr_state, what):
    if lr_state.numel() != LR_STATE_FLOATS or not lr_state.is_contiguous():
        raise ValueError("{}: lr_state must be {} contiguous floats (base rate, rate of the last step)".format(what, LR_STATE_FLOATS))
    return _ptr(lr_state, F32, 'lr_state')


def lr_rates(sched, lr_state, first_step, n, out=None):
    """The rates of the steps first_step .. first_step + n - 1 (zero-based) under `sched` (an LrSchedule), into out[:n] (float32, on the
    device; allocated when not given).  Returns out."""
    first_step, n = int(first_step), int(n)
    if first_step < 0 or n < 0 or first_step + n > LR_MAX_STEP:
        raise ValueError("lr_rates: steps {} .. {} are outside 0 .. 2^24".format(first_step, first_step + n))
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=lr_state.device)
    if out.numel() < n or not out.is_contiguous():
        raise ValueError("lr_rates: out must hold {} contiguous floats".format(n))
    _launch('amar_lr_rates_f32', ctypes.byref(sched), _lr_state(lr_state, 'lr_rates'), first_step, n, _ptr(out, F32, 'out'))
    return out


def adam_advance_lr(state, sched, lr_state, beta_1, beta_2):
    if state.numel() != 2 or not state.is_contiguous():
        raise ValueError("adam_advance_lr: state must be 2 contiguous floats (t, lr_t)")
    _launch('amar_adam_advance_lr_f32', _ptr(state, F32, 'state'), ctypes.byref(sched), _lr_state(lr_state, 'adam_advance_lr'),
            float(beta_1), float(beta_2))


def optim_advance_lr(state, rule, flags, hyper, sched, lr_state):
    if state.numel() != OPTIM_STATE_FLOATS or not state.is_contiguous():
        raise ValueError("optim_advance_lr: state must be {} contiguous floats".format(OPTIM_STATE_FLOATS))
    _launch('amar_optim_advance_lr_f32', _ptr(state, F32, 'state'), int(rule), int(flags), ctypes.byref(hyper), ctypes.byref(sched),
            _lr_state(lr_state, 'optim_advance_lr'))


# ---- gradient clipping (include/amar_hip.h: AMAR_CLIP_*) -------------------------------------------------------------------------------
CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = 1, 2, 3


class ClipSlot(ctypes.Structure):
    """include/amar_hip.h: amar_clip_slot"""
    _fields_ = [('w', ctypes.c_void_p), ('g', ctypes.c_void_p), ('n', ctypes.c_int64), ('first_block', ctypes.c_int64),
                ('l2', ctypes.c_float), ('g_groups', ctypes.c_int32)]


def clip_slot_table(entries):
    """entries: [(w, g, l2)] contiguous fp32 tensors (g: a tensor or a DeferredGradient) -> (host uint8 tensor holding the slot table,
    total blocks): the block partition of adam_slot_table / optim_slot_table over the same parameters."""
    return _slot_table(ClipSlot, [(w, g, (), l2) for w, g, l2 in entries], 'clip_slot_table', 'contiguous tensors expected')


def finished_gradient(g, n):
    """Where amar_grad_clip_f32 leaves a slot's finished gradient: group 0 of a DeferredGradient's partials, else the tensor itself."""
    return g.partials.view(-1)[:n] if isinstance(g, DeferredGradient) else g


def grad_clip_workspace_floats(n_slots, total_blocks):
    count = load().amar_grad_clip_workspace_floats(int(n_slots), int(total_blocks))
    _check(count if count < 0 else 0, 'amar_grad_clip_workspace_floats')
    return count


def grad_clip(mode, clip, table_dev, n_slots, total_blocks, workspace=None, norms=None, reg_scale=0.0, loss_acc=None):
    """Finish, measure and clip the gradients of a slot table in place (group 0 of every slot); see include/amar_hip.h."""
    if workspace is not None and workspace.numel() < max(int(total_blocks), 0) + max(int(n_slots), 0):
        raise ValueError("grad_clip: workspace of grad_clip_workspace_floats(n_slots, total_blocks) floats expected")
    if norms is not None and mode in (CLIP_NORM, CLIP_GLOBAL_NORM) and norms.numel() < (n_slots if mode == CLIP_NORM else 1):
        raise ValueError("grad_clip: norms must hold one float per slot (CLIP_NORM) or one float (CLIP_GLOBAL_NORM)")
    _launch('amar_grad_clip_f32', int(mode), float(clip), None if table_dev is None else ctypes.c_void_p(table_dev.data_ptr()),
            int(n_slots), int(total_blocks), _ptr(workspace, F32, 'workspace'), _ptr(norms, F32, 'norms'), float(reg_scale),
            _ptr(loss_acc, F32, 'loss_acc'))


def sum_into(x, acc, scale=1.0):
    _launch('amar_sum_into_f32', _ptr(x, F32, 'x'), x.numel(), float(scale), _ptr(acc, F32, 'acc'))


def topk_segmented(seg_ptr, item_ids, scores, k):
    n_users = seg_ptr.numel() - 1
    out_items = torch.empty((n_users, k), dtype=torch.int32, device=scores.device)
    out_scores = torch.empty((n_users, k), dtype=torch.float32, device=scores.device)
    _launch('amar_topk_segmented_f32', _ptr(seg_ptr, I32, 'seg_ptr'), _ptr(item_ids, I32, 'item_ids'), _ptr(scores, F32, 'scores'), n_users, k,
            _ptr(out_items), _ptr(out_scores))
    return out_items, out_scores


def _check_cursor(what, after_items, after_scores, rows):
    """The cursor of a paging call: one (item, score) per row, both given (ValueError, prefixed by `what`)."""
    if after_items is None or after_scores is None:
        raise ValueError("{}: after_items and after_scores are both required".format(what))
    if after_items.numel() != rows or after_scores.numel() != rows:
        raise ValueError("{}: after_items and after_scores must hold one entry per listed row ({} and {} for {})".format(
            what, after_items.numel(), after_scores.numel(), rows))


def topk_segmented_after(seg_ptr, item_ids, scores, k, after_items, after_scores):
    """amar_topk_segmented_after_f32: `topk_segmented` from a cursor.  User u's list holds the k best pairs strictly after the
    position (after_scores[u], after_items[u]) (int32 / float32 device arrays of n_users entries) in the order score descending, item
    id ascending; (+inf, -1) is the start, (-inf, -1) admits nothing.  The scores are only read: one call per page of one scored chunk."""
    n_users = seg_ptr.numel() - 1
    _check_cursor('topk_segmented_after', after_items, after_scores, n_users)
    out_items = torch.empty((n_users, k), dtype=torch.int32, device=scores.device)
    out_scores = torch.empty((n_users, k), dtype=torch.float32, device=scores.device)
    _launch('amar_topk_segmented_after_f32', _ptr(seg_ptr, I32, 'seg_ptr'), _ptr(item_ids, I32, 'item_ids'), _ptr(scores, F32, 'scores'),
            n_users, k, _ptr(after_scores, F32, 'after_scores'), _ptr(after_items, I32, 'after_items'), _ptr(out_items), _ptr(out_scores))
    return out_items, out_scores


def _sliced_topk(slices_fn, slices_args, n_slices, m, k, dev, split_head=True):
    """What the fused rankers allocate alike: the slices the library will launch for the request `n_slices` (its `slices_fn` over
    `slices_args`, then the request; a negative answer raises), the [m, k] outputs and the int32 workspace of the per-slice lists
    (None with one slice).  split_head (the rankers of the split head, not `nearest`): a request <= 0 is read from
    AMAR_RECOMMEND_SLICES, and the float32 workspace of the per-slice scores is the fifth value (else None)."""
    if split_head and n_slices <= 0:
        n_slices = int(os.environ.get('AMAR_RECOMMEND_SLICES', '0'))
    slices = getattr(load(), slices_fn)(*slices_args, int(n_slices))
    if slices < 0:
        _check(int(slices), slices_fn)
    out_rows = torch.empty((m, k), dtype=torch.int32, device=dev)
    out_scores = torch.empty((m, k), dtype=torch.float32, device=dev)
    ws_rows = torch.empty((m * slices * k,), dtype=torch.int32, device=dev) if slices > 1 else None
    ws_scores = torch.empty((m * slices * k,), dtype=torch.float32, device=dev) if split_head and slices > 1 else None
    return slices, out_rows, out_scores, ws_rows, ws_scores


RANK_KINDS = {'recommend': 0, 'group': 1, 'rank_of': 2, 'among': 4, 'lists': 5}    # include/amar_hip.h: AMAR_RANK_RECOMMEND / _GROUP / _RANK_OF / _AMONG / _LISTS


class RankRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_rank_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('maxt', 'pt', 'tile_items', 'tile_stride', 'wpack_floats', 'fits', 'large_lds',
                                                    'reserved')] + [('lds_bytes', ctypes.c_int64)]
    BOOLS, HIDDEN = ('fits', 'large_lds'), ('reserved',)


def rank_route(kind, dims, code=False):
    """What `recommend` ('recommend'), `recommend_group` ('group'), `rank_of` ('rank_of'), `recommend_among` ('among') or
    `recommend_lists` ('lists': no item tile in its sum, so it takes heads the others refuse) does with a rest stack of the widths
    `dims` (c1, ..., 1): the launch geometry (maxt, pt, tile_items, tile_stride), wpack_floats, the dynamic LDS of a launch
    (lds_bytes), `fits` (lds_bytes <= 160 KB: False = the entry point refuses the head with AMAR_EUNSUPPORTED) and `large_lds`
    (> 64 KB).  amar_rank_route: host only, the launchers ask the same function.  A dict; with code=True the return code is added as
    `code` and nothing is raised, else dims the launchers refuse raise as their wrappers would."""
    info = RankRouteInfo()
    dims = [int(d) for d in dims]
    rc = load().amar_rank_route(RANK_KINDS[kind], (ctypes.c_int32 * max(len(dims), 1))(*dims), len(dims) - 1, ctypes.byref(info))
    if not code:
        _check(rc, 'amar_rank_route')
    d = info.as_dict()
    if code:
        d['code'] = int(rc)
    return d


def rank_fits(kind, dims):
    """Whether the fused ranker `kind` takes a rest stack of these widths: its argument checks pass and its LDS sum fits
    (`rank_route`).  False sends the caller to its pair route; nothing is raised."""
    r = rank_route(kind, dims, code=True)
    return r['code'] == 0 and r['fits']


def _rank_head(what, Tu, Ti, wpack, dims, acts, in_act):
    """The head of a fused ranker's call, as `recommend`, `recommend_among`, `recommend_group` and `rank_of` marshal it: the width
    check (ValueError, prefixed by `what`) and the `dims` / `acts` arrays.  Returns (n_users, n_items, dims_c, head): `head()` gives
    the twelve leading arguments of the entry point, Tu .. in_act; the tensors are looked at (device, dtype, layout) when it is
    called, in the argument list of the launch, so a wrapper's own host checks keep their place in front of them."""
    n_users, c1, n_items = int(Tu.shape[0]), int(Tu.shape[1]), int(Ti.shape[0])
    if int(Ti.shape[1]) != c1:
        raise ValueError("{}: Tu and Ti must have the same width".format(what))
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    acts_c = (ctypes.c_int32 * len(acts))(*[ACT_CODES[a] for a in acts])

    def head():
        return (*_mat(Tu, 'Tu'), n_users, *_mat(Ti, 'Ti'), n_items, c1, _ptr(wpack, F32, 'wpack'), dims_c, acts_c, len(acts), ACT_CODES[in_act])
    return n_users, n_items, dims_c, head


def _check_exclusion(what, excl_ptr, excl_items, rows, entries='n_users + 1 entries'):
    """The two checks of a ranker's exclusion CSR over `rows` rows (ValueError, prefixed by `what`)."""
    if (excl_ptr is None) != (excl_items is None):
        raise ValueError("{}: excl_ptr and excl_items go together".format(what))
    if excl_ptr is not None and excl_ptr.numel() != rows + 1:
        raise ValueError("{}: excl_ptr must have {}".format(what, entries))


def recommend(Tu, Ti, wpack, dims, acts, in_act, k, users=None, excl_ptr=None, excl_items=None, n_slices=0):
    """Fused full-catalogue top-k of the split head (amar_recommend_f32): for every user row of `users` (all rows of Tu when None)
    the k best items of Ti that are not in its exclusion CSR.  Returns (items int32 [m, k] (-1 padded), scores float32 [m, k]).
    n_slices <= 0: the library's automatic item slicing (AMAR_RECOMMEND_SLICES overrides it)."""
    n_users, n_items, dims_c, head = _rank_head('recommend', Tu, Ti, wpack, dims, acts, in_act)
    m = int(users.numel()) if users is not None else n_users
    slices, out_items, out_scores, ws_i, ws_s = _sliced_topk('amar_recommend_slices', (m, n_items, dims_c, len(acts)), n_slices, m, k, Tu.device)
    _check_exclusion('recommend', excl_ptr, excl_items, n_users)
    _launch('amar_recommend_f32', *head(), _ptr(users, I32, 'users'), m, _ptr(excl_ptr, I32, 'excl_ptr'),
            _ptr_entries(excl_items, I32, 'excl_items'), int(k), int(slices) if slices > 1 else 1, _ptr(ws_i), _ptr(ws_s),
            _ptr(out_items) if m else None, _ptr(out_scores) if m else None)
    return out_items, out_scores


def check_candidate_rows(cand, n_items, what='recommend_among'):
    """Host int32 item rows of a candidate list as amar_recommend_among_f32 wants them: integers, strictly ascending (so distinct),
    each in [0, n_items).  The kernel cannot check its list, so nothing that fails here is uploaded: ValueError."""
    import numpy as np
    a = cand.detach().cpu().numpy() if isinstance(cand, torch.Tensor) else np.asarray(cand)
    if a.ndim != 1 or (a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer))):
        raise ValueError("{}: cand must be a 1-D sequence of integer item rows".format(what))
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n_items):
        raise ValueError("{}: cand must lie in [0, {}) (got {}..{})".format(what, n_items, int(a.min()), int(a.max())))
    if a.size > 1 and (np.diff(a) <= 0).any():
        raise ValueError("{}: cand must be strictly ascending (sorted, no duplicates)".format(what))
    return np.ascontiguousarray(a, dtype=np.int32)


def recommend_among(Tu, Ti, wpack, dims, acts, in_act, k, cand, users=None, excl_ptr=None, excl_items=None, n_slices=0):
    """Fused top-k among a candidate slice of the items (amar_recommend_among_f32): for every user row of `users` (all rows of Tu
    when None) the k best of the item rows `cand` that are not in its exclusion CSR.  `cand` is a HOST sequence of item rows; it is
    checked here (`check_candidate_rows`: ascending, distinct, in range — ValueError) before it is uploaded, because the kernel
    cannot check it.  Returns (items int32 [m, k] item rows (-1 padded), scores float32 [m, k] (-inf padded)): what `recommend`
    returns with the complement of `cand` merged into every exclusion row, bit for bit.  n_slices <= 0: the library's automatic
    slicing of the candidate positions (AMAR_RECOMMEND_SLICES overrides it)."""
    n_users, n_items, dims_c, head = _rank_head('recommend_among', Tu, Ti, wpack, dims, acts, in_act)
    rows = check_candidate_rows(cand, n_items)
    n_cand = int(rows.size)
    _check_exclusion('recommend_among', excl_ptr, excl_items, n_users)
    m = int(users.numel()) if users is not None else n_users
    slices, out_items, out_scores, ws_i, ws_s = _sliced_topk('amar_recommend_slices', (m, n_cand, dims_c, len(acts)), n_slices, m, k, Tu.device)
    cand_dev = torch.from_numpy(rows).to(Tu.device) if n_cand else None
    _launch('amar_recommend_among_f32', *head(), _ptr(users, I32, 'users'), m, _ptr(excl_ptr, I32, 'excl_ptr'),
            _ptr_entries(excl_items, I32, 'excl_items'), _ptr(cand_dev, I32, 'cand'), n_cand,
            int(k), int(slices) if slices > 1 else 1, _ptr(ws_i), _ptr(ws_s),
            _ptr(out_items) if m else None, _ptr(out_scores) if m else None)
    return out_items, out_scores


def check_candidate_lists(cand_ptr, cand_items, m, n_items, what='recommend_lists'):
    """A HOST CSR of candidate lists as amar_recommend_lists_f32 wants it: cand_ptr m + 1 non-decreasing integers from 0 to
    len(cand_items) < 2^31, cand_items integer item rows in [0, n_items), strictly ascending inside every list.  The kernel cannot
    check its lists, so nothing that fails here is uploaded: ValueError.  Returns (ptr int32, items int32)."""
    import numpy as np
    ptr, rows = np.asarray(cand_ptr), np.asarray(cand_items)
    for a, name in ((ptr, 'cand_ptr'), (rows, 'cand_items')):
        if a.ndim != 1 or (a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer))):
            raise ValueError("{}: {} must be a 1-D sequence of integers".format(what, name))
    ptr, rows = ptr.astype(np.int64), rows.astype(np.int64)
    if ptr.size != m + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != rows.size:
        raise ValueError("{}: cand_ptr must hold {} non-decreasing offsets from 0 to len(cand_items)".format(what, m + 1))
    if rows.size >= 1 << 31:
        raise ValueError("{}: the candidate lists must hold fewer than 2^31 entries together".format(what))
    if rows.size and (rows.min() < 0 or rows.max() >= n_items):
        raise ValueError("{}: cand_items must lie in [0, {}) (got {}..{})".format(what, n_items, int(rows.min()), int(rows.max())))
    if rows.size > 1:
        falls = np.diff(rows) <= 0                                           # allowed only where a new list starts
        falls[ptr[1:-1][(ptr[1:-1] > 0) & (ptr[1:-1] < rows.size)] - 1] = False
        if falls.any():
            raise ValueError("{}: cand_items must be strictly ascending inside every list (sorted, no duplicates)".format(what))
    return np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(rows, dtype=np.int32)


def recommend_lists(Tu, Ti, wpack, dims, acts, in_act, k, cand_ptr, cand_items, users=None, excl_ptr=None, excl_items=None):
    """Fused top-k over per-user candidate lists (amar_recommend_lists_f32): for listed row j (user users[j]; row j of Tu when
    `users` is None) the k best of the item rows cand_items[cand_ptr[j] : cand_ptr[j + 1]] that are not in the user's exclusion CSR.
    The CSR is either a pair of HOST sequences, checked here (`check_candidate_lists`: ascending inside every list, distinct, in
    range — ValueError) before it is uploaded, or a pair of int32 DEVICE tensors, which the caller answers for: the kernel cannot
    check its lists.  Returns (items int32 [m, k] item rows (-1 padded), scores float32 [m, k] (-inf padded)): what `recommend`
    returns with the complement of every row's list merged into its exclusion row, bit for bit.  One launch, no workspace."""
    n_users, n_items, dims_c, head = _rank_head('recommend_lists', Tu, Ti, wpack, dims, acts, in_act)
    m = int(users.numel()) if users is not None else n_users
    on_device = isinstance(cand_ptr, torch.Tensor) and cand_ptr.is_cuda
    if on_device != (isinstance(cand_items, torch.Tensor) and cand_items.is_cuda):
        raise ValueError("recommend_lists: cand_ptr and cand_items must both be host sequences or both device tensors")
    if on_device:
        if cand_ptr.dim() != 1 or cand_ptr.numel() != m + 1 or cand_items.dim() != 1 or cand_items.numel() >= 1 << 31:
            raise ValueError("recommend_lists: cand_ptr must have {} entries, cand_items fewer than 2^31".format(m + 1))
    else:
        ptr, rows = check_candidate_lists(cand_ptr.cpu().numpy() if isinstance(cand_ptr, torch.Tensor) else cand_ptr,
                                          cand_items.cpu().numpy() if isinstance(cand_items, torch.Tensor) else cand_items, m, n_items)
        cand_ptr, cand_items = torch.from_numpy(ptr).to(Tu.device), torch.from_numpy(rows).to(Tu.device)
    _check_exclusion('recommend_lists', excl_ptr, excl_items, n_users)
    out_items = torch.empty((m, k), dtype=torch.int32, device=Tu.device)
    out_scores = torch.empty((m, k), dtype=torch.float32, device=Tu.device)
    _launch('amar_recommend_lists_f32', *head(), _ptr(users, I32, 'users'), m, _ptr(excl_ptr, I32, 'excl_ptr'),
            _ptr_entries(excl_items, I32, 'excl_items'), _ptr(cand_ptr, I32, 'cand_ptr'), _ptr_entries(cand_items, I32, 'cand_items'),
            int(k), _ptr(out_items) if m else None, _ptr(out_scores) if m else None)
    return out_items, out_scores


def recommend_after(Tu, Ti, wpack, dims, acts, in_act, k, after_items, after_scores, users=None, excl_ptr=None, excl_items=None, n_slices=0):
    """Fused top-k after a position of every listed user's ranking (amar_recommend_after_f32): `recommend` with a cursor per listed
    row.  after_items int32 [m] / after_scores float32 [m] on the device, indexed by the listed row (not by the user row): row j's
    list holds the k best unexcluded items strictly after (after_scores[j], after_items[j]) in the order score descending, item row
    ascending.  (+inf, -1) is the start (`recommend`'s output, bit for bit); (-inf, -1), the padding of an exhausted list, admits
    nothing; the item is only a position (it may be excluded or no row at all).  Returns (items int32 [m, k] (-1 padded), scores
    float32 [m, k] (-inf padded)); the typical next cursor is (items[:, -1], scores[:, -1]).  n_slices as in `recommend`."""
    n_users, n_items, dims_c, head = _rank_head('recommend_after', Tu, Ti, wpack, dims, acts, in_act)
    m = int(users.numel()) if users is not None else n_users
    _check_cursor('recommend_after', after_items, after_scores, m)
    slices, out_items, out_scores, ws_i, ws_s = _sliced_topk('amar_recommend_slices', (m, n_items, dims_c, len(acts)), n_slices, m, k, Tu.device)
    _check_exclusion('recommend_after', excl_ptr, excl_items, n_users)
    _launch('amar_recommend_after_f32', *head(), _ptr(users, I32, 'users'), m, _ptr(excl_ptr, I32, 'excl_ptr'),
            _ptr_entries(excl_items, I32, 'excl_items'), _ptr_entries(after_scores, F32, 'after_scores'),
            _ptr_entries(after_items, I32, 'after_items'), int(k), int(slices) if slices > 1 else 1, _ptr(ws_i), _ptr(ws_s),
            _ptr(out_items) if m else None, _ptr(out_scores) if m else None)
    return out_items, out_scores


GROUP_STRATEGIES = {'mean': 0, 'min': 1, 'max': 2}                    # include/amar_hip.h: AMAR_GROUP_MEAN / _MIN / _MAX


def recommend_group(Tu, Ti, wpack, dims, acts, in_act, k, grp_ptr, grp_users, strategy='mean', min_score=None, excl_ptr=None, excl_items=None,
                    n_slices=0):
    """Fused group top-k of the split head (amar_recommend_group_f32): group j has the members grp_users[grp_ptr[j]:grp_ptr[j + 1]]
    (int32 rows of Tu, ascending and distinct inside a group); every item's member scores are combined by `strategy` ('mean', 'min' =
    least misery, 'max' = most pleasure), an item is dropped when any member scores it below `min_score` (None: no veto), and the k
    best items that are not in segment j of the exclusion CSR (excl_ptr [g + 1], a CSR over GROUPS) are kept.  Returns (items int32
    [g, k] (-1 padded), scores float32 [g, k] (-inf padded)).  n_slices <= 0: the library's automatic item slicing
    (AMAR_RECOMMEND_SLICES overrides it)."""
    if strategy not in GROUP_STRATEGIES:
        raise ValueError("recommend_group: strategy must be one of {} (got {!r})".format(sorted(GROUP_STRATEGIES), strategy))
    n_users, n_items, dims_c, head = _rank_head('recommend_group', Tu, Ti, wpack, dims, acts, in_act)
    g, n_members = int(grp_ptr.numel()) - 1, int(grp_users.numel())
    if g < 0:
        raise ValueError("recommend_group: grp_ptr must have one entry per group plus one")
    _check_exclusion('recommend_group', excl_ptr, excl_items, g, 'one entry per group plus one')
    slices, out_items, out_scores, ws_i, ws_s = _sliced_topk('amar_recommend_group_slices', (g, n_members, n_items, dims_c, len(acts)), n_slices,
                                                             g, k, Tu.device)
    _launch('amar_recommend_group_f32', *head(), _ptr(grp_ptr, I32, 'grp_ptr'), _ptr_entries(grp_users, I32, 'grp_users'), g, n_members,
            _ptr(excl_ptr, I32, 'excl_ptr'), _ptr_entries(excl_items, I32, 'excl_items'), GROUP_STRATEGIES[strategy],
            float('-inf') if min_score is None else float(min_score), int(k), int(slices) if slices > 1 else 1, _ptr(ws_i), _ptr(ws_s),
            _ptr(out_items) if g else None, _ptr(out_scores) if g else None)
    return out_items, out_scores


NEAREST_METRICS = {'dot': 0, 'cosine': 1}                              # include/amar_hip.h: AMAR_NEAREST_DOT / _COSINE
NEAREST_MAX_D, NEAREST_MAX_K = 512, 64


def nearest_supported(d, k):
    """Whether amar_nearest_f32 takes vectors of width d and lists of length k."""
    return d % 4 == 0 and 4 <= d <= NEAREST_MAX_D and 1 <= k <= NEAREST_MAX_K


def nearest(Q, T, k, metric='cosine', query_rows=None, excl_ptr=None, excl_rows=None, n_slices=0):
    """Fused dot / cosine top-k (amar_nearest_f32): for every listed query (row query_rows[j] of Q, all rows of Q when None) the k
    best rows of T that are not in segment j of the exclusion CSR (excl_ptr [m + 1], excl_rows sorted per segment).  Returns
    (rows int32 [m, k] (-1 padded), scores float32 [m, k] (-inf padded)).  n_slices <= 0: the library's automatic table slicing."""
    if metric not in NEAREST_METRICS:
        raise ValueError("nearest: metric must be one of {} (got {!r})".format(sorted(NEAREST_METRICS), metric))
    n_q, d = int(Q.shape[0]), int(Q.shape[1])
    n_rows = int(T.shape[0])
    if int(T.shape[1]) != d:
        raise ValueError("nearest: Q and T must have the same width")
    m = int(query_rows.numel()) if query_rows is not None else n_q
    if (excl_ptr is None) != (excl_rows is None):
        raise ValueError("nearest: excl_ptr and excl_rows go together")
    if excl_ptr is not None and excl_ptr.numel() != m + 1:
        raise ValueError("nearest: excl_ptr must have one entry per listed query plus one")
    lib = load()
    metric_code = NEAREST_METRICS[metric]
    slices, out_rows, out_scores, ws_r, _ = _sliced_topk('amar_nearest_slices', (m, n_rows, d), n_slices, m, k, Q.device, split_head=False)
    floats = lib.amar_nearest_workspace_floats(m, n_rows, int(k), metric_code, int(slices))
    if floats < 0:
        _check(int(floats), 'amar_nearest_workspace_floats')
    ws_s = torch.empty((floats,), dtype=torch.float32, device=Q.device) if floats else None
    _launch('amar_nearest_f32', *_mat(Q, 'Q'), n_q, *_mat(T, 'T'), n_rows, d, metric_code, _ptr(query_rows, I32, 'query_rows'), m,
            _ptr(excl_ptr, I32, 'excl_ptr'), _ptr_entries(excl_rows, I32, 'excl_rows'), int(k), int(slices), _ptr(ws_r), _ptr(ws_s),
            _ptr(out_rows) if m else None, _ptr(out_scores) if m else None)
    return out_rows, out_scores


RANK_METRICS_MAX_KS, RANK_METRICS_MAX_BLOCKS = 8, 1024                 # include/amar_hip.h: AMAR_RANK_METRICS_MAX_KS / _MAX_BLOCKS
RANK_METRICS_CELLS = 4 * RANK_METRICS_MAX_KS + 2


def rank_metrics_args(K, ks):
    """The host arguments of amar_rank_metrics_f64, checked: (ks as a list of ints, cum_disc float64 [K + 1] with cum_disc[0] = 0 and
    cum_disc[j] = sum_{r <= j} 1 / log2(r + 1)).  ValueError for K outside [1, 64], no or more than 8 cutoffs, a cutoff outside [1, K]."""
    import numpy as np
    K = int(K)
    ks = [int(k) for k in ks]
    if not 1 <= K <= 64:
        raise ValueError("rank_metrics: the lists must hold between 1 and 64 ranks (got {})".format(K))
    if not 1 <= len(ks) <= RANK_METRICS_MAX_KS:
        raise ValueError("rank_metrics: between 1 and {} cutoffs (got {})".format(RANK_METRICS_MAX_KS, len(ks)))
    if any(k < 1 or k > K for k in ks):
        raise ValueError("every k must lie in [1, {}] (the length of the lists)".format(K))
    cum = np.zeros(K + 1, dtype=np.float64)
    np.cumsum(1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0), out=cum[1:])
    return ks, cum


def rank_metrics(lists, rel_ptr, rel_items, ks, users=None):
    """Full-ranking metrics of device lists (amar_rank_metrics_f64): lists int32 [m, K] item rows best first (-1 padded), the relevant
    items as a CSR over users (rel_ptr int32 [n_users + 1], rel_items int32 sorted and de-duplicated per user), row j belonging to
    users[j] (int32 [m]; None: user j, m == n_users).  Returns (means float64 [nk, 4]: precision, recall, ndcg, hit per cutoff — the
    sums over the evaluated users divided by their number, the sums themselves when nobody was evaluated —, evaluated, skipped)."""
    import numpy as np
    if lists.dim() != 2 or not lists.is_contiguous():
        raise ValueError("rank_metrics: lists must be a contiguous [m, K] tensor")
    m, K = int(lists.shape[0]), int(lists.shape[1])
    ks, cum = rank_metrics_args(K, ks)
    n_users = int(rel_ptr.numel()) - 1
    if n_users < 0:
        raise ValueError("rank_metrics: rel_ptr must have n_users + 1 entries")
    if users is not None and int(users.numel()) != m:
        raise ValueError("rank_metrics: users must name one user per list")
    if users is None and m != n_users:
        raise ValueError("rank_metrics: without users the lists must cover every user ({} lists, {} users)".format(m, n_users))
    dev = rel_ptr.device
    ws = torch.empty(RANK_METRICS_MAX_BLOCKS * RANK_METRICS_CELLS, dtype=torch.float64, device=dev)
    sums = torch.empty((len(ks), 4), dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ks_c = (ctypes.c_int32 * len(ks))(*ks)
    _launch('amar_rank_metrics_f64', _ptr(lists, I32, 'lists') if m else None, m, K, _ptr(users, I32, 'users'), _ptr(rel_ptr, I32, 'rel_ptr'),
            _ptr_entries(rel_items, I32, 'rel_items'), n_users, ks_c, len(ks), cum.ctypes.data_as(ctypes.c_void_p),
            _ptr(ws), _ptr(sums), _ptr(counts))
    evaluated, skipped = (int(c) for c in counts.cpu().numpy())
    sums = sums.cpu().numpy()
    return (sums / evaluated if evaluated else sums), evaluated, skipped


RANK_OF_MAX_TARGETS = 64                                               # include/amar_hip.h: AMAR_RANK_OF_MAX_TARGETS


def rank_of_entries(users, tgt_ptr, max_targets=RANK_OF_MAX_TARGETS):
    """Entries of at most `max_targets` targets from rows of any length: (users int32 [m'], tgt_ptr int32 [m' + 1]) on the host.  A
    row of n targets becomes ceil(n / max_targets) consecutive entries of the same user (an empty row: none), so the flat order of
    the targets, and with it of the outputs, is the caller's."""
    import numpy as np
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    ptr = np.asarray(tgt_ptr, dtype=np.int64).reshape(-1)
    if len(ptr) != len(users) + 1 or (len(ptr) and ptr[0] != 0) or (np.diff(ptr) < 0).any():
        raise ValueError("rank_of: tgt_ptr must be a CSR pointer over the listed users ({} users, {} entries)".format(len(users), len(ptr)))
    n = np.diff(ptr)
    pieces = (n + max_targets - 1) // max_targets
    owner = np.repeat(np.arange(len(users)), pieces)
    first = np.cumsum(pieces) - pieces
    start = ptr[:-1][owner] + (np.arange(len(owner)) - first[owner]) * max_targets
    out_ptr = np.append(start, ptr[-1] if len(ptr) else 0)
    return users[owner].astype(np.int32), out_ptr.astype(np.int32)


def rank_of(Tu, Ti, wpack, dims, acts, in_act, users, tgt_ptr, tgt_items, excl_ptr=None, excl_items=None, n_slices=0, split=True):
    """Exact full-catalogue positions by counting (amar_rank_of_f32).  `users` (rows of Tu, host integers [m]; the same user may be
    listed more than once) and `tgt_ptr` [m + 1] / `tgt_items` (host integers: the item rows asked about per listed user, ascending
    and distinct inside a row) name the pairs; the exclusion CSR over the rows of Tu is on the device, as for `recommend`.  Rows
    longer than RANK_OF_MAX_TARGETS are cut into several entries of the same user (`rank_of_entries`; split=False hands them to the
    library as they are, which refuses them).  Returns the device tensors (scores float32, greater int32, eq_before int32,
    eq_after int32), one value per target in the order of `tgt_items`: 1 + greater + eq_before is the item's position in the user's
    full ranking (score descending, item row ascending) among the items outside the user's exclusion row.
    n_slices <= 0: the library's automatic item slicing."""
    import numpy as np
    n_users, n_items, _, head = _rank_head('rank_of', Tu, Ti, wpack, dims, acts, in_act)
    _check_exclusion('rank_of', excl_ptr, excl_items, n_users)
    items = np.ascontiguousarray(np.asarray(tgt_items).reshape(-1), dtype=np.int32)
    if split:
        users_h, ptr_h = rank_of_entries(users, tgt_ptr)
    else:
        users_h, ptr_h = np.asarray(users, dtype=np.int32).reshape(-1), np.asarray(tgt_ptr, dtype=np.int32).reshape(-1)
        if len(ptr_h) != len(users_h) + 1:
            raise ValueError("rank_of: tgt_ptr must have one entry per listed user plus one")
    m, n_targets = len(users_h), len(items)
    if (int(ptr_h[-1]) if len(ptr_h) else 0) != n_targets:
        raise ValueError("rank_of: tgt_ptr must end at the number of targets ({} != {})".format(int(ptr_h[-1]) if len(ptr_h) else 0, n_targets))
    if m and (users_h.min() < 0 or users_h.max() >= n_users):
        raise ValueError("rank_of: users must be rows of Tu")
    if n_targets and (items.min() < 0 or items.max() >= n_items):
        raise ValueError("rank_of: targets must be rows of Ti")
    dev = Tu.device
    _ptr(Tu, F32, 'Tu')                                                # (a host tensor is refused before anything is allocated beside it)
    scores = torch.empty(n_targets, dtype=torch.float32, device=dev)
    greater, before, after = (torch.empty(n_targets, dtype=torch.int32, device=dev) for _ in range(3))
    users_d, ptr_d, items_d = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (users_h, ptr_h, items))
    longest = int(np.diff(ptr_h.astype(np.int64)).max()) if m else 0
    _launch('amar_rank_of_f32', *head(), _ptr_entries(users_d, I32, 'users'), m, _ptr(excl_ptr, I32, 'excl_ptr'), _ptr_entries(excl_items, I32, 'excl_items'),
            _ptr(ptr_d, I32, 'tgt_ptr'), _ptr_entries(items_d, I32, 'tgt_items'), n_targets, longest, int(n_slices) if n_slices > 0 else 0,
            _ptr_entries(scores, F32, 'scores'), _ptr_entries(greater, I32, 'greater'), _ptr_entries(before, I32, 'eq_before'),
            _ptr_entries(after, I32, 'eq_after'))
    return scores, greater, before, after


def rank_of_metrics(scores, greater, eq_before, eq_after, rel_ptr, n_cand):
    """AUC, reciprocal rank and average precision per evaluated user from `rank_of`'s flat outputs (amar_rank_of_metrics_f64):
    rel_ptr int32 [n_eval + 1] cuts the flat order into the users' held-out items, n_cand int32 [n_eval] = the items outside each
    user's exclusion row.  Returns the device tensors (out float64 [n_eval, 3]: auc, rr, ap; valid int32 [n_eval]: 0 for a user
    without a target or without a candidate that is not one)."""
    n_eval, n_targets = int(rel_ptr.numel()) - 1, int(scores.numel())
    if n_eval < 0 or int(n_cand.numel()) != n_eval:
        raise ValueError("rank_of_metrics: rel_ptr must have one entry per evaluated user plus one, n_cand one per user")
    if any(int(t.numel()) != n_targets for t in (greater, eq_before, eq_after)):
        raise ValueError("rank_of_metrics: scores, greater, eq_before and eq_after must have one value per target")
    dev = rel_ptr.device
    out = torch.empty((n_eval, 3), dtype=torch.float64, device=dev)
    valid = torch.empty(n_eval, dtype=torch.int32, device=dev)
    _launch('amar_rank_of_metrics_f64', _ptr_entries(scores, F32, 'scores'), _ptr_entries(greater, I32, 'greater'),
            _ptr_entries(eq_before, I32, 'eq_before'), _ptr_entries(eq_after, I32, 'eq_after'), n_targets, _ptr(rel_ptr, I32, 'rel_ptr'),
            _ptr_entries(n_cand, I32, 'n_cand'), n_eval, _ptr_entries(out, torch.float64, 'out'), _ptr_entries(valid, I32, 'valid'))
    return out, valid


DIVERSIFY_MAX_P = 64                                                   # include/amar_hip.h: AMAR_DIVERSIFY_MAX_P


def _lists_matrix(t, name):
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError("{} must be a contiguous [m, P] tensor".format(name))
    return int(t.shape[0]), int(t.shape[1])


def rerank_mmr(pool_items, pool_scores, T, k, trade_off=0.7, metric='cosine', want_mmr=False, want_ild=False):
    """Greedy MMR re-ranking of device pools (amar_rerank_mmr_f32): pool_items int32 [m, P] rows of T (valid prefix, -1 padded),
    pool_scores float32 [m, P], T float32 [n_rows, d].  Returns (items int32 [m, k], scores float32 [m, k]) in selection order,
    followed by the MMR values float32 [m, k] (want_mmr) and the lists' ILD float64 [m] (want_ild).  One launch, no workspace."""
    if metric not in NEAREST_METRICS:
        raise ValueError("rerank_mmr: metric must be one of {} (got {!r})".format(sorted(NEAREST_METRICS), metric))
    m, P = _lists_matrix(pool_items, 'pool_items')
    if _lists_matrix(pool_scores, 'pool_scores') != (m, P):
        raise ValueError("rerank_mmr: pool_items and pool_scores must have the same shape")
    dev = T.device
    k = int(k)
    out_items = torch.empty((m, max(k, 0)), dtype=torch.int32, device=dev)
    out_scores = torch.empty((m, max(k, 0)), dtype=torch.float32, device=dev)
    out_mmr = torch.empty((m, max(k, 0)), dtype=torch.float32, device=dev) if want_mmr else None
    out_ild = torch.empty((m,), dtype=torch.float64, device=dev) if want_ild else None
    _launch('amar_rerank_mmr_f32', _ptr(pool_items, I32, 'pool_items') if m else None, _ptr(pool_scores, F32, 'pool_scores') if m else None,
            m, P, *_mat(T, 'T'), int(T.shape[0]), int(T.shape[1]), NEAREST_METRICS[metric], float(trade_off),
            k, _ptr(out_items) if m else None, _ptr(out_scores) if m else None, _ptr(out_mmr) if m else None,
            _ptr(out_ild) if m else None)
    return (out_items, out_scores) + ((out_mmr,) if want_mmr else ()) + ((out_ild,) if want_ild else ())


def list_diversity(lists, T, ks, metric='cosine'):
    """Intra-list diversity of device lists (amar_list_diversity_f64): lists int32 [m, K] rows of T (-1 padded), cutoffs ks.  Returns
    (ild float64 [m, nk]: the mean of 1 - sim over the pairs of valid items in the first ks[q] ranks, 0 below two items;
    count int32 [m, nk]: those items), both on the device."""
    if metric not in NEAREST_METRICS:
        raise ValueError("list_diversity: metric must be one of {} (got {!r})".format(sorted(NEAREST_METRICS), metric))
    m, K = _lists_matrix(lists, 'lists')
    ks = [int(k) for k in ks]
    dev = T.device
    out_ild = torch.empty((m, len(ks)), dtype=torch.float64, device=dev)
    out_count = torch.empty((m, len(ks)), dtype=torch.int32, device=dev)
    ks_c = (ctypes.c_int32 * max(1, len(ks)))(*ks)
    _launch('amar_list_diversity_f64', _ptr(lists, I32, 'lists') if m else None, m, K, *_mat(T, 'T'), int(T.shape[0]), int(T.shape[1]),
            NEAREST_METRICS[metric], ks_c, len(ks), _ptr(out_ild) if m else None, _ptr(out_count) if m else None)
    return out_ild, out_count


EXPLAIN_MAX_K, EXPLAIN_MAX_E, EXPLAIN_MAX_PROP_ROW = 64, 16, 2048      # include/amar_hip.h: AMAR_EXPLAIN_MAX_*


def explain(lists, liked_ptr, liked_items, T, n_evidence=3, n_properties=0, metric='cosine', users=None, prop_ptr=None, prop_ids=None,
            prop_weight=None, max_prop_row=0):
    """Evidence items and shared properties of device lists (amar_explain_f32): lists int32 [m, K] rows of T (-1 padded), row j
    belonging to users[j] (int32 [m]; None: user j), the liked items as a CSR over users, the item-property links as an optional CSR
    over items with float32 weights (max_prop_row: its longest row).  Returns (evidence int32 [m, K, E], evidence_sim float32 [m, K, E],
    props int32 [m, K, Q], prop_score float32 [m, K, Q], prop_support int32 [m, K, Q]) on the device.  One launch, no workspace."""
    if metric not in NEAREST_METRICS:
        raise ValueError("explain: metric must be one of {} (got {!r})".format(sorted(NEAREST_METRICS), metric))
    m, K = _lists_matrix(lists, 'lists')
    if users is not None and int(users.numel()) != m:
        raise ValueError("explain: users must name one user per list")
    n_users = int(liked_ptr.numel()) - 1
    n_items = int(T.shape[0])
    if prop_ptr is not None and int(prop_ptr.numel()) != n_items + 1:
        raise ValueError("explain: prop_ptr must have one entry per row of T plus one")
    E, Q = int(n_evidence), int(n_properties)
    dev = T.device
    out_ev = torch.empty((m, K, max(E, 0)), dtype=torch.int32, device=dev)
    out_sim = torch.empty((m, K, max(E, 0)), dtype=torch.float32, device=dev)
    out_p = torch.empty((m, K, max(Q, 0)), dtype=torch.int32, device=dev)
    out_ps = torch.empty((m, K, max(Q, 0)), dtype=torch.float32, device=dev)
    out_pc = torch.empty((m, K, max(Q, 0)), dtype=torch.int32, device=dev)
    filled = m > 0 and Q > 0
    _launch('amar_explain_f32', _ptr(lists, I32, 'lists') if m else None, m, K, _ptr(users, I32, 'users'), _ptr(liked_ptr, I32, 'liked_ptr'),
            _ptr_entries(liked_items, I32, 'liked_items'), n_users, *_mat(T, 'T'), n_items, int(T.shape[1]), NEAREST_METRICS[metric],
            _ptr(prop_ptr, I32, 'prop_ptr'), _ptr_entries(prop_ids, I32, 'prop_ids'), _ptr_entries(prop_weight, F32, 'prop_weight'),
            int(prop_weight.numel()) if prop_weight is not None else 0, int(max_prop_row), E, Q,
            _ptr(out_ev) if m else None, _ptr(out_sim) if m else None, _ptr(out_p) if filled else None, _ptr(out_ps) if filled else None,
            _ptr(out_pc) if filled else None)
    return out_ev, out_sim, out_p, out_ps, out_pc


CALIBRATE_MAX_P, CALIBRATE_MAX_G, CALIBRATE_POOL_BUDGET = 64, 1024, 4096   # include/amar_hip.h: AMAR_CALIBRATE_*


def _calibrate_sizes(what, m, users, liked_ptr, cat_ptr):
    if users is not None and int(users.numel()) != m:
        raise ValueError("{}: users must name one user per list".format(what))
    return int(liked_ptr.numel()) - 1, int(cat_ptr.numel()) - 1


def rerank_calibrated(pool_items, pool_scores, liked_ptr, liked_items, cat_ptr, cat_ids, n_categories, k, trade_off=0.5, smoothing=0.01,
                      users=None, max_cat_row=0, want_value=False, want_kl=False, want_target=False):
    """Greedy calibrated re-ranking of device pools (amar_rerank_calibrated_f32): pool_items int32 [m, P] item rows (-1 padded),
    pool_scores float32 [m, P], row j belonging to users[j] (int32 [m]; None: user j), the liked items as a CSR over users, the
    categories as a CSR over items with values in 0..n_categories-1 (max_cat_row: its longest row).  Returns (items int32 [m, k],
    scores float32 [m, k]) in selection order, followed by the step values float32 [m, k] (want_value), the miscalibration after
    each step float32 [m, k] (want_kl) and the users' targets float32 [m, G] (want_target).  One launch, no workspace."""
    m, P = _lists_matrix(pool_items, 'pool_items')
    if _lists_matrix(pool_scores, 'pool_scores') != (m, P):
        raise ValueError("rerank_calibrated: pool_items and pool_scores must have the same shape")
    n_users, n_items = _calibrate_sizes('rerank_calibrated', m, users, liked_ptr, cat_ptr)
    dev = pool_items.device
    k, G = int(k), int(n_categories)
    out_items = torch.empty((m, max(k, 0)), dtype=torch.int32, device=dev)
    out_scores = torch.empty((m, max(k, 0)), dtype=torch.float32, device=dev)
    out_value = torch.empty((m, max(k, 0)), dtype=torch.float32, device=dev) if want_value else None
    out_kl = torch.empty((m, max(k, 0)), dtype=torch.float32, device=dev) if want_kl else None
    out_target = torch.empty((m, max(G, 0)), dtype=torch.float32, device=dev) if want_target else None
    _launch('amar_rerank_calibrated_f32', _ptr(pool_items, I32, 'pool_items') if m else None, _ptr(pool_scores, F32, 'pool_scores') if m else None,
            m, P, _ptr(users, I32, 'users'), _ptr(liked_ptr, I32, 'liked_ptr'), _ptr_entries(liked_items, I32, 'liked_items'), n_users,
            _ptr(cat_ptr, I32, 'cat_ptr'), _ptr_entries(cat_ids, I32, 'cat_ids'), n_items, G, int(max_cat_row), float(trade_off),
            float(smoothing), k, _ptr(out_items) if m else None, _ptr(out_scores) if m else None, _ptr(out_value) if m else None,
            _ptr(out_kl) if m else None, _ptr(out_target) if m else None)
    return (out_items, out_scores) + tuple(t for t in (out_value, out_kl, out_target) if t is not None)


def list_calibration(lists, liked_ptr, liked_items, cat_ptr, cat_ids, n_categories, ks, smoothing=0.01, users=None):
    """Miscalibration of device lists (amar_list_calibration_f64): lists int32 [m, K] item rows (-1 padded) of users[j] (None: user
    j), CSRs as in rerank_calibrated, cutoffs ks.  Returns (kl float64 [m, nk]: C(p, the first ks[q] ranks), 0 for a user without a
    target; count int32 [m, nk]: the items with a category in those ranks; support int32 [m]: the user's liked items with a
    category), all on the device."""
    m, K = _lists_matrix(lists, 'lists')
    n_users, n_items = _calibrate_sizes('list_calibration', m, users, liked_ptr, cat_ptr)
    ks = [int(k) for k in ks]
    dev = lists.device
    out_kl = torch.empty((m, len(ks)), dtype=torch.float64, device=dev)
    out_count = torch.empty((m, len(ks)), dtype=torch.int32, device=dev)
    out_support = torch.empty((m,), dtype=torch.int32, device=dev)
    ks_c = (ctypes.c_int32 * max(1, len(ks)))(*ks)
    _launch('amar_list_calibration_f64', _ptr(lists, I32, 'lists') if m else None, m, K, _ptr(users, I32, 'users'),
            _ptr(liked_ptr, I32, 'liked_ptr'), _ptr_entries(liked_items, I32, 'liked_items'), n_users, _ptr(cat_ptr, I32, 'cat_ptr'),
            _ptr_entries(cat_ids, I32, 'cat_ids'), n_items, int(n_categories), float(smoothing), ks_c, len(ks),
            _ptr(out_kl) if m else None, _ptr(out_count) if m else None, _ptr(out_support) if m else None)
    return out_kl, out_count, out_support


# ---- training step ----------------------------------------------------------------------------------------------
def act_bwd(dY, Y, dZ, act):
    """dZ = dY * act'(Y) with Y the layer output (dZ may alias dY)."""
    if tuple(dY.shape) != tuple(Y.shape) or tuple(dZ.shape) != tuple(Y.shape):
        raise ValueError("act_bwd: shapes differ")
    _launch('amar_act_bwd_f32', *_mat(dY, 'dY'), *_mat(Y, 'Y'), *_mat(dZ, 'dZ'), Y.shape[0], Y.shape[1], ACT_CODES[act])


def _wgrad_args(X, dZ, dW, db, checked):
    """The arguments amar_wgrad_f32 and amar_wgrad_route share (all but the last two / one), and (M, K, N).  checked: the launcher's
    shape checks, which the route query does not make."""
    M, N = dZ.shape
    K = X.shape[1] if X is not None else 0
    if checked and dW is not None and (X is None or X.shape[0] != M or tuple(dW.shape) != (K, N) or not dW.is_contiguous()):
        raise ValueError("wgrad: X [M, K], dZ [M, N], dW [K, N] contiguous expected")
    if checked and db is not None and (db.numel() != N or not db.is_contiguous()):
        raise ValueError("wgrad: db must be a contiguous [N] vector")
    # X travels only where dW is asked for (not _mat: a dW without an X stays an error in the route query too)
    x_ptr, ldx = (_ptr(X, F32, 'X'), _ld(X, 'X')) if dW is not None else (None, 0)
    return [x_ptr, ldx, *_mat(dZ, 'dZ'), M, K, N, _ptr(dW, F32, 'dW'), _ptr(db, F32, 'db')], (M, K, N)


def wgrad(X, dZ, dW=None, db=None):
    """dW = X^T . dZ and / or db = column sums of dZ (deterministic two-stage reduction)."""
    args, (M, K, N) = _wgrad_args(X, dZ, dW, db, checked=True)
    n_scratch = load().amar_wgrad_scratch_floats(M, K if dW is not None else 0, N)
    scratch = torch.empty(max(int(n_scratch), 1), dtype=torch.float32, device=dZ.device)
    _launch('amar_wgrad_f32', *args, _ptr(scratch))


class WgradRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_wgrad_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'wg_rows', 'grid_k', 'grid_n')] + \
               [('chunks', ctypes.c_int64), ('scratch_floats', ctypes.c_int64)]
    KERNELS = {0: 'partial', 1: 'mfma'}


def wgrad_route(X, dZ, dW=None, db=None):
    """Which kernel wgrad takes for these operands (amar_wgrad_route: host only, nothing is launched; the launcher asks the same
    function).  A dict: kernel 'mfma' | 'partial', wg_rows, chunks, grid_k, grid_n, scratch_floats."""
    info = WgradRouteInfo()
    _call('amar_wgrad_route', *_wgrad_args(X, dZ, dW, db, checked=False)[0], ctypes.byref(info))
    return info.as_dict()


def dense_stack_supported(dims):
    """amar_dense_stack_f32 takes a stack of these widths (at most 4 layers, every width <= 128)."""
    return 2 <= len(dims) <= 5 and all(1 <= int(d) <= 128 for d in dims)


def _dense_stack_args(X, weights, biases, acts, outs, ids=None, xcopy=None):
    """The argument list of amar_dense_stack_f32 (without the stream) for one stack, checked."""
    n = len(weights)
    M = int(ids.numel()) if ids is not None else int(X.shape[0])
    dims = [int(weights[0].shape[0])] + [int(w.shape[1]) for w in weights]
    if X.shape[1] != dims[0] or len(biases) != n or len(acts) != n or len(outs) != n:
        raise ValueError("dense_stack: X [*, K_0] and one kernel / bias / activation / output per layer expected")
    for l, (w, b, y) in enumerate(zip(weights, biases, outs)):
        if tuple(w.shape) != (dims[l], dims[l + 1]) or not w.is_contiguous() or tuple(y.shape) != (M, dims[l + 1]):
            raise ValueError("dense_stack: layer {}: W [K, N] contiguous and Y [M, N] expected".format(l))
        if b is not None and (b.numel() != dims[l + 1] or not b.is_contiguous()):
            raise ValueError("dense_stack: layer {}: bias must be a contiguous [N] vector".format(l))
    if xcopy is not None and tuple(xcopy.shape) != (M, dims[0]):
        raise ValueError("dense_stack: xcopy must be [M, K_0]")
    arr_p = ctypes.c_void_p * n
    wp = arr_p(*[_ptr(w, F32, 'W') for w in weights])
    bp = arr_p(*[_ptr(b, F32, 'bias') for b in biases])
    yp = arr_p(*[_ptr(y, F32, 'Y') for y in outs])
    ld = (ctypes.c_int64 * n)(*[_ld(y, 'Y') for y in outs])
    dm = (ctypes.c_int32 * (n + 1))(*dims)
    ac = (ctypes.c_int32 * n)(*[ACT_CODES[a] for a in acts])
    return [*_mat(X, 'X'), _ptr(ids, I32, 'ids'), *_mat(xcopy, 'xcopy'), n, wp, bp, dm, ac, yp, ld, M]


def dense_stack(X, weights, biases, acts, outs, ids=None, xcopy=None):
    """A Dense stack forward in one launch with every layer's output kept (amar_dense_stack_f32): y_0 = X[ids], outs[l] = act_l(y_l . W_l + b_l).
    outs[l] may be column slices of wider buffers; xcopy ([M, K_0]): also receives the gathered input rows."""
    _launch('amar_dense_stack_f32', *_dense_stack_args(X, weights, biases, acts, outs, ids=ids, xcopy=xcopy))


class DenseStackDesc(ctypes.Structure):
    """include/amar_hip.h: amar_dense_stack_desc"""
    _fields_ = [('X', ctypes.c_void_p), ('ldx', ctypes.c_int64), ('ids', ctypes.c_void_p), ('Xcopy', ctypes.c_void_p), ('ldxc', ctypes.c_int64),
                ('n_layers', ctypes.c_int32), ('W', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('dims', ctypes.c_void_p), ('acts', ctypes.c_void_p),
                ('Y', ctypes.c_void_p), ('ldy', ctypes.c_void_p), ('M', ctypes.c_int64)]


class DenseStackBwdDesc(ctypes.Structure):
    """include/amar_hip.h: amar_dense_stack_bwd_desc"""
    _fields_ = [('dYtop', ctypes.c_void_p), ('lddy', ctypes.c_int64), ('Ytop', ctypes.c_void_p), ('ldytop', ctypes.c_int64), ('n_layers', ctypes.c_int32),
                ('X', ctypes.c_void_p), ('ldx', ctypes.c_void_p), ('W', ctypes.c_void_p), ('dims', ctypes.c_void_p), ('acts', ctypes.c_void_p),
                ('dX0', ctypes.c_void_p), ('lddx0', ctypes.c_int64), ('dW', ctypes.c_void_p), ('db', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
                ('flags', ctypes.c_int32), ('M', ctypes.c_int64)]


def _as_pointer(v):
    """ctypes arrays (host arrays of device pointers / values) and c_void_p values as plain addresses for a Structure field."""
    if isinstance(v, ctypes.Array):
        return ctypes.cast(v, ctypes.c_void_p).value
    return v.value if isinstance(v, ctypes.c_void_p) else v


def dense_stack_pair(first, second):
    """Two independent Dense stacks forward in ONE launch (amar_dense_stack_pair_f32).  first / second: dicts of dense_stack's arguments
    (X, weights, biases, acts, outs, ids, xcopy).  Same results as two dense_stack calls."""
    a0, a1 = _dense_stack_args(**first), _dense_stack_args(**second)
    d0, d1 = DenseStackDesc(*[_as_pointer(v) for v in a0]), DenseStackDesc(*[_as_pointer(v) for v in a1])
    _launch('amar_dense_stack_pair_f32', ctypes.byref(d0), ctypes.byref(d1))


def dense_stack_bwd_supported(dims, M):
    """amar_dense_stack_bwd_f32 takes this stack (at most 4 layers no wider than 128, batch-sized operands: M <= 4 096 rows)."""
    return dense_stack_supported(dims) and 1 <= int(M) <= 4096 and os.environ.get('AMAR_DENSE_STACK_BWD', '1') != '0'


def dense_stack_bwd_workspace(M, dims, device):
    n = len(dims) - 1
    dm = (ctypes.c_int32 * (n + 1))(*[int(d) for d in dims])
    floats = int(load().amar_dense_stack_bwd_workspace_floats(int(M), n, dm))
    return torch.empty(max(floats, 4), dtype=torch.float32, device=device)


def _dense_stack_bwd_args(dYtop, Ytop, inputs, weights, acts, workspace, dWs, dbs, dX0=None, defer=False):
    """The argument list of amar_dense_stack_bwd_f32 (without the stream) for one stack, checked, and its (n, M, dims)."""
    n = len(weights)
    M = int(dYtop.shape[0])
    dims = [int(weights[0].shape[0])] + [int(w.shape[1]) for w in weights]
    if len(inputs) != n or len(acts) != n or len(dWs) != n or len(dbs) != n or dYtop.shape[1] != dims[-1]:
        raise ValueError("dense_stack_bwd: one input / kernel / activation / dW / db per layer and dYtop [M, N_last] expected")
    for l in range(n):
        if tuple(inputs[l].shape) != (M, dims[l]) or tuple(weights[l].shape) != (dims[l], dims[l + 1]) or not weights[l].is_contiguous() or \
                tuple(dWs[l].shape) != (dims[l], dims[l + 1]) or not dWs[l].is_contiguous() or dbs[l].numel() != dims[l + 1]:
            raise ValueError("dense_stack_bwd: layer {}: shapes".format(l))
    if dX0 is not None and tuple(dX0.shape) != (M, dims[0]):
        raise ValueError("dense_stack_bwd: dX0 must be [M, K_0]")
    arr_p = ctypes.c_void_p * n
    xp = arr_p(*[_ptr(x, F32, 'X') for x in inputs])
    lx = (ctypes.c_int64 * n)(*[_ld(x, 'X') for x in inputs])
    wp = arr_p(*[_ptr(w, F32, 'W') for w in weights])
    dwp = arr_p(*[_ptr(w, F32, 'dW') for w in dWs])
    dbp = arr_p(*[_ptr(b, F32, 'db') for b in dbs])
    dm = (ctypes.c_int32 * (n + 1))(*dims)
    ac = (ctypes.c_int32 * n)(*[ACT_CODES[a] for a in acts])
    if workspace.numel() < load().amar_dense_stack_bwd_workspace_floats(M, n, dm):
        raise ValueError("dense_stack_bwd: workspace too small (capi.dense_stack_bwd_workspace)")
    args = [*_mat(dYtop, 'dYtop'), *_mat(Ytop, 'Ytop'), n, xp, lx, wp, dm, ac, *_mat(dX0, 'dX0'), dwp, dbp,
            _ptr(workspace, F32, 'workspace'), DENSE_BWD_DEFER if defer else 0, M]
    return args, (n, M, dims)


def _deferred_stack_gradients(workspace, n, M, dims):
    g = int(load().amar_dense_stack_bwd_groups(int(M)))
    out, off = [], 4
    for l in range(n):
        kn, nn = dims[l] * dims[l + 1], dims[l + 1]
        out.append((DeferredGradient(workspace[off:off + g * kn], g, (dims[l], dims[l + 1])),
                    DeferredGradient(workspace[off + g * kn:off + g * (kn + nn)], g, (nn,))))
        off += g * (kn + nn)
    return out


def dense_stack_bwd(dYtop, Ytop, inputs, weights, acts, workspace, dWs, dbs, dX0=None, defer=False):
    """The reverse pass of a Dense stack in one launch (amar_dense_stack_bwd_f32).  inputs[l] = layer l's input, Ytop = the last layer's
    output (None: dYtop already is the last pre-activation's gradient).  defer=True: dWs / dbs are not written; returns one
    (DeferredGradient dW, DeferredGradient db) per layer."""
    args, (n, M, dims) = _dense_stack_bwd_args(dYtop, Ytop, inputs, weights, acts, workspace, dWs, dbs, dX0=dX0, defer=defer)
    _launch('amar_dense_stack_bwd_f32', *args)
    return _deferred_stack_gradients(workspace, n, M, dims) if defer else None


def dense_stack_bwd_pair(first, second):
    """The reverse passes of two independent Dense stacks in ONE launch (amar_dense_stack_bwd_pair_f32).  first / second: dicts of
    dense_stack_bwd's arguments.  Returns the two results dense_stack_bwd would have returned."""
    (a0, m0), (a1, m1) = _dense_stack_bwd_args(**first), _dense_stack_bwd_args(**second)
    d0, d1 = DenseStackBwdDesc(*[_as_pointer(v) for v in a0]), DenseStackBwdDesc(*[_as_pointer(v) for v in a1])
    _launch('amar_dense_stack_bwd_pair_f32', ctypes.byref(d0), ctypes.byref(d1))
    return (_deferred_stack_gradients(first['workspace'], *m0) if first.get('defer') else None,
            _deferred_stack_gradients(second['workspace'], *m1) if second.get('defer') else None)


class DenseStackRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_dense_stack_route_info (as_dict(n_layers): vec_w one per layer)"""
    _fields_ = [('rows', ctypes.c_int32), ('vec_x', ctypes.c_int32), ('vec_w', ctypes.c_int32 * 4), ('groups', ctypes.c_int64),
                ('lds_bytes', ctypes.c_int64)]
    BOOLS = ('vec_x', 'vec_w')


class DenseStackBwdRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_dense_stack_bwd_route_info (as_dict(n_layers): vec_x and vec_w one per layer)"""
    _fields_ = [('rows', ctypes.c_int32), ('vec_top', ctypes.c_int32), ('vec_x', ctypes.c_int32 * 4), ('vec_w', ctypes.c_int32 * 4),
                ('groups', ctypes.c_int64), ('lds_bytes', ctypes.c_int64)]
    BOOLS = ('vec_top', 'vec_x', 'vec_w')


def dense_stack_route(X, weights, biases, acts, outs, ids=None, xcopy=None):
    """What dense_stack does with these operands (amar_dense_stack_route: host only, nothing is launched; the launcher asks the same
    functions).  A dict: rows (16 | 64), groups, lds_bytes, vec_x, vec_w (one per layer)."""
    args = _dense_stack_args(X, weights, biases, acts, outs, ids=ids, xcopy=xcopy)
    info = DenseStackRouteInfo()
    _call('amar_dense_stack_route', *args, ctypes.byref(info))
    return info.as_dict(len(weights))


def dense_stack_bwd_route(dYtop, Ytop, inputs, weights, acts, workspace, dWs, dbs, dX0=None, defer=False):
    """What dense_stack_bwd does with these operands (amar_dense_stack_bwd_route: host only).  A dict: rows (16 | 64), groups,
    lds_bytes, vec_top, vec_x and vec_w (one per layer)."""
    args, _ = _dense_stack_bwd_args(dYtop, Ytop, inputs, weights, acts, workspace, dWs, dbs, dX0=dX0, defer=defer)
    info = DenseStackBwdRouteInfo()
    _call('amar_dense_stack_bwd_route', *args, ctypes.byref(info))
    return info.as_dict(len(weights))


def dense_bwd_supported(K, N):
    """amar_dense_bwd_f32 can take this layer (act', dX, dW, db: two launches instead of four)."""
    return 1 <= K <= 128 and 1 <= N <= 128


def dense_bwd_enabled():
    """Whether the training tapes use amar_dense_bwd_f32 (AMAR_DENSE_BWD=0: the separate kernels).  Measured at ml1m(s=1), BasicGCN
    16 x 2, batch 1 024 (tools/profile_train.sh): 703 ms of kernel time per 1 482 batches against 768."""
    return os.environ.get('AMAR_DENSE_BWD', '1') != '0'


def dense_stack_enabled():
    """Whether the training tapes run a Dense stack's forward as ONE launch (amar_dense_stack_f32; AMAR_DENSE_STACK=0: layer by layer)."""
    return os.environ.get('AMAR_DENSE_STACK', '1') != '0'


def dense_bwd_workspace(M, K, N, device):
    """A workspace for dense_bwd calls of this shape (allocate once, reuse every batch: it holds the workgroups' partial gradients)."""
    n = int(load().amar_dense_bwd_workspace_floats(int(M), int(K), int(N)))
    return torch.zeros(max(n, 4), dtype=torch.float32, device=device)


DENSE_BWD_DEFER = 0x100


DENSE_BWD_ACCUM_DX = 0x200


def _dense_bwd_args(X, Y, dY, W, act, workspace, dX, dW, db, defer, dZ, accumulate_dx, K, checked):
    """The arguments amar_dense_bwd_f32 and amar_dense_bwd_route share (up to dZ's leading dimension; the launcher's workspace
    follows, then M, K, N in both), and (M, K, N).  checked: the launcher's checks, which the route query does not make."""
    M, N = dY.shape
    K = W.shape[0] if W is not None else (X.shape[1] if X is not None else int(K or 1))    # (K only sizes the workspace when neither is given)
    if checked:
        if dX is not None and (W is None or tuple(W.shape) != (K, N) or not W.is_contiguous() or tuple(dX.shape) != (M, K)):
            raise ValueError("dense_bwd: W [K, N] contiguous and dX [M, K] expected")
        if dW is not None and (X is None or tuple(X.shape) != (M, K) or tuple(dW.shape) != (K, N) or not dW.is_contiguous()):
            raise ValueError("dense_bwd: X [M, K] and dW [K, N] contiguous expected")
        if db is not None and (db.numel() != N or not db.is_contiguous()):
            raise ValueError("dense_bwd: db must be a contiguous [N] vector")
        if Y is not None and tuple(Y.shape) != (M, N):
            raise ValueError("dense_bwd: Y [M, N] expected")
        if dZ is not None and tuple(dZ.shape) != (M, N):
            raise ValueError("dense_bwd: dZ [M, N] expected")
        if workspace is None or workspace.numel() < load().amar_dense_bwd_workspace_floats(M, K, N):
            raise ValueError("dense_bwd: workspace too small (capi.dense_bwd_workspace)")
    return [*_mat(X, 'X'), *_mat(Y, 'Y'), *_mat(dY, 'dY'), _ptr(W, F32, 'W'),
            ACT_CODES[act] | (DENSE_BWD_DEFER if defer else 0) | (DENSE_BWD_ACCUM_DX if accumulate_dx else 0),
            *_mat(dX, 'dX'), _ptr(dW, F32, 'dW'), _ptr(db, F32, 'db'), *_mat(dZ, 'dZ')], (M, K, N)


def dense_bwd(X, Y, dY, W, act, workspace, dX=None, dW=None, db=None, defer=False, dZ=None, accumulate_dx=False, K=None):
    """The reverse pass of one Dense layer in two launches instead of four (amar_dense_bwd_f32): dZ = dY * act'(Y); dX = dZ . W^T; dW = X^T . dZ;
    db = column sums of dZ.  Y is the layer's OUTPUT (None with act None: dY already is dZ); any of dX / dW / db may be None."""
    args, (M, K, N) = _dense_bwd_args(X, Y, dY, W, act, workspace, dX, dW, db, defer, dZ, accumulate_dx, K, checked=True)
    _launch('amar_dense_bwd_f32', *args, _ptr(workspace, F32, 'workspace'), M, K, N)
    if defer:
        # defer=True: dW / db are NOT written; the partial sums stay in the workspace — returned as DeferredGradients (dW's, db's)
        g = int(load().amar_dense_bwd_groups(M))
        nw = g * K * N if dW is not None else 0
        return (DeferredGradient(workspace[4:4 + nw], g, (K, N)) if dW is not None else None,
                DeferredGradient(workspace[4 + nw:4 + nw + g * N], g, (N,)) if db is not None else None)
    return None


class DenseBwdRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_dense_bwd_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'mt', 'kp', 'np', 'vec', 'x_scalar', 'subtiles', 'fold', 'fold_launch')] + \
               [('launched_groups', ctypes.c_int64), ('out_groups', ctypes.c_int64)]
    KERNELS, BOOLS = {0: 'tile', 1: 'rows'}, ('vec', 'x_scalar', 'fold_launch')


def dense_bwd_route(X, Y, dY, W, act, workspace=None, dX=None, dW=None, db=None, defer=False, dZ=None, accumulate_dx=False, K=None):
    """Which kernel dense_bwd takes for these operands (amar_dense_bwd_route: host only, nothing is launched; the launcher asks the same
    function).  A dict: kernel 'tile' | 'rows', mt (tile), kp / np (rows), vec, x_scalar, subtiles, launched_groups, fold, fold_launch,
    out_groups."""
    args, (M, K, N) = _dense_bwd_args(X, Y, dY, W, act, workspace, dX, dW, db, defer, dZ, accumulate_dx, K, checked=False)
    info = DenseBwdRouteInfo()
    _call('amar_dense_bwd_route', *args, M, K, N, ctypes.byref(info))
    return info.as_dict()


def bce_grad(p, y, dz, loss_terms):
    B = y.numel()
    _launch('amar_bce_grad_f32', *_col(p, 'p'), _ptr(y, F32, 'y'), _ptr(dz, F32, 'dz'), _ptr(loss_terms, F32, 'loss_terms'), B)


def bpr_grad(p, dz, loss_terms):
    """BPR loss terms and d(loss)/d(logit) for the probability column p ([B] or [B, 1]); dz [B, 1] / loss_terms [B] contiguous."""
    B = p.shape[0]
    if dz.numel() != B or loss_terms.numel() != B or not dz.is_contiguous() or not loss_terms.is_contiguous():
        raise ValueError("bpr_grad: p [B] or [B, 1], dz and loss_terms of B contiguous floats expected")
    _launch('amar_bpr_grad_f32', *_col(p, 'p'), _ptr(dz, F32, 'dz'), _ptr(loss_terms, F32, 'loss_terms'), B)


# include/amar_hip.h: AMAR_GROUP_*
GROUP_SOFTMAX, GROUP_HARDEST, GROUP_MARGIN = range(3)


def group_loss_grad(kind, hyper, p, dz, loss_terms, n_negatives=1):
    """Listwise loss terms and d(loss)/d(logit) on the triplet layout (amar_group_loss_grad_f32): kind one of GROUP_*, hyper the
    temperature (GROUP_SOFTMAX) or the margin (GROUP_MARGIN), p the probability column ([B] or [B, 1]) whose h = B // 2 triples
    split into groups of n_negatives; dz [B, 1] / loss_terms [B] contiguous."""
    B = p.shape[0]
    if dz.numel() != B or loss_terms.numel() != B or not dz.is_contiguous() or not loss_terms.is_contiguous():
        raise ValueError("group_loss_grad: p [B] or [B, 1], dz and loss_terms of B contiguous floats expected")
    K = int(n_negatives)
    if K < 1 or (B // 2) % K:
        raise ValueError("group_loss_grad: {} triples do not split into groups of n_negatives = {}".format(B // 2, n_negatives))
    _launch('amar_group_loss_grad_f32', int(kind), float(hyper), *_col(p, 'p'), _ptr(dz, F32, 'dz'), _ptr(loss_terms, F32, 'loss_terms'), B, K)


# include/amar_hip.h: AMAR_LOSS_*
LOSS_BCE, LOSS_MSE, LOSS_MAE, LOSS_HINGE, LOSS_SQUARED_HINGE, LOSS_HUBER, LOSS_LOG_COSH, LOSS_POISSON, LOSS_FOCAL = range(9)
LOSS_HYPER_FLOATS = 4
AUC_BUCKETS = 199
LOSS_COUNTERS = 4 + 2 * AUC_BUCKETS


def loss_counters():
    """Size of the metric counter block of `loss_grad` (int64 cells), as the library states it."""
    return int(load().amar_loss_counters())


def loss_grad(loss, hyper, p, y, dz, loss_terms, counters=None, sample_weight=None, class_weight=None):
    """Per-pair terms and d(mean loss)/d(logit) of Keras loss `loss` (a LOSS_* code; hyper: LOSS_HYPER_FLOATS floats or None) for the
    probability column p ([B] or [B, 1]) and labels y [B]; dz [B, 1] / loss_terms [B] contiguous.  counters: None, or the int64 block
    of LOSS_COUNTERS cells on the device that this batch is added to (tp, fp, tn, fn, then the 2 x 199 AUC histogram).
    sample_weight ([B] floats) / class_weight (two floats: class 0, class 1), device tensors: with either one the call is
    amar_loss_grad_weighted_f32 and both outputs carry the pair's weight as their last float32 multiplication; with neither it is
    amar_loss_grad_f32, the launch it always was."""
    B = p.shape[0]
    if p.dim() not in (1, 2) or (p.dim() == 2 and p.shape[1] != 1) or (p.dim() == 1 and B > 1 and p.stride(0) != 1):
        raise ValueError("loss_grad: p must be [B] contiguous or a [B, 1] column")
    if y.numel() != B or dz.numel() != B or loss_terms.numel() != B or not y.is_contiguous() or not dz.is_contiguous() \
            or not loss_terms.is_contiguous():
        raise ValueError("loss_grad: y, dz and loss_terms of B contiguous floats expected")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != LOSS_COUNTERS or not counters.is_contiguous()):
        raise ValueError("loss_grad: counters must be {} contiguous int64 cells".format(LOSS_COUNTERS))
    hp = None
    if hyper is not None:
        if len(hyper) != LOSS_HYPER_FLOATS:
            raise ValueError("loss_grad: hyper must hold {} floats".format(LOSS_HYPER_FLOATS))
        hp = (ctypes.c_float * LOSS_HYPER_FLOATS)(*[float(v) for v in hyper])
    if sample_weight is not None or class_weight is not None:
        if sample_weight is not None and (sample_weight.numel() != B or not sample_weight.is_contiguous()):
            raise ValueError("loss_grad: sample_weight of B contiguous floats expected")
        if class_weight is not None and (class_weight.numel() != 2 or not class_weight.is_contiguous()):
            raise ValueError("loss_grad: class_weight must be two contiguous floats (class 0, class 1)")
        _launch('amar_loss_grad_weighted_f32', int(loss), hp, *_col(p, 'p'), _ptr(y, F32, 'y'), _ptr(sample_weight, F32, 'sample_weight'),
                _ptr(class_weight, F32, 'class_weight'), _ptr(dz, F32, 'dz'), _ptr(loss_terms, F32, 'loss_terms'), B,
                _ptr(counters, torch.int64, 'counters'))
        return
    _launch('amar_loss_grad_f32', int(loss), hp, *_col(p, 'p'), _ptr(y, F32, 'y'), _ptr(dz, F32, 'dz'), _ptr(loss_terms, F32, 'loss_terms'), B,
            _ptr(counters, torch.int64, 'counters'))


def bpr_sample(pos_ptr, pos_ids, neg_ptr, neg_ids, n_users, seed, step, u, items, y=None, advance=True):
    """One BPR batch of h = items.numel() // 2 draws into u [2h], items [2h] (int32) and y [2h] (float32, optional); step: one
    int64 on the device (the counter of the draws, advanced by one when `advance`).  The CSRs are int32 device tensors whose user
    rows are all non-empty (checked by the caller where they are uploaded)."""
    h = items.numel() // 2
    if u.numel() != 2 * h or items.numel() != 2 * h or (y is not None and y.numel() != 2 * h) or step.numel() != 1 \
            or step.dtype != torch.int64 or pos_ptr.numel() != n_users + 1 or neg_ptr.numel() != n_users + 1:
        raise ValueError("bpr_sample: u, items (and y) of 2h elements, an int64 step and CSR row pointers [n_users + 1] expected")
    _launch('amar_bpr_sample_i32', _ptr(pos_ptr, I32, 'pos_ptr'), _ptr(pos_ids, I32, 'pos_ids'), _ptr(neg_ptr, I32, 'neg_ptr'), _ptr(neg_ids, I32, 'neg_ids'),
            int(n_users), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(step), int(bool(advance)), h, _ptr(u, I32, 'u'), _ptr(items, I32, 'items'),
            _ptr(y, F32, 'y'))


def bpr_sample_triplets(pos_ptr, pos_ids, excl_ptr, excl_ids, n_users, n_items, item_base, seed, step, u, items, y=None,
                        n_negatives=1, mode=0, advance=True):
    """One batch of h = items.numel() // 2 BPR triples into u [2h], items [2h] (int32) and y [2h] (float32, optional):
    u[t] = u[h + t] = the triple's user, items[t] its positive, items[h + t] its negative — uniform over the items outside the user's
    exclusion row.  `n_negatives` triples share one (user, positive) draw; mode 0 draws users uniformly, 1 interactions.  step: one
    int64 on the device, advanced by one when `advance`.  The CSRs are int32 device tensors, exclusion rows strictly ascending inside
    [item_base, item_base + n_items) and shorter than n_items, positive rows non-empty (checked by the caller where they are
    uploaded)."""
    h = items.numel() // 2
    if u.numel() != 2 * h or items.numel() != 2 * h or (y is not None and y.numel() != 2 * h) or step.numel() != 1 \
            or step.dtype != torch.int64 or pos_ptr.numel() != n_users + 1 or excl_ptr.numel() != n_users + 1:
        raise ValueError("bpr_sample_triplets: u, items (and y) of 2h elements, an int64 step and CSR row pointers [n_users + 1] expected")
    _launch('amar_bpr_sample_triplets_i32', _ptr(pos_ptr, I32, 'pos_ptr'), _ptr(pos_ids, I32, 'pos_ids'), _ptr(excl_ptr, I32, 'excl_ptr'),
            _ptr_entries(excl_ids, I32, 'excl_ids'), int(n_users), int(n_items), int(item_base), int(n_negatives), int(mode),
            int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(step), int(bool(advance)), h, _ptr(u, I32, 'u'), _ptr(items, I32, 'items'), _ptr(y, F32, 'y'))


class Dropout:
    """The arguments of one dropout site as the library takes them: the 64-bit key, the step counter (one int64 on the device,
    read by the kernels, advanced by `dropout_advance`), the site (1..255) and the rate as (threshold, scale): a 32-bit word
    keeps its value iff word >= threshold = min(2^32 - 1, floor(rate * 2^32 + 0.5)), kept values are multiplied by
    scale = float32(1 / (1 - rate)).  data/datasets.py:dropout_node_mask / dropout_edge_mask restate the bits."""

    __slots__ = ('seed', 'step', 'site', 'rate', 'threshold', 'scale')

    def __init__(self, seed, step, site, rate):
        rate = check_dropout_rate(rate, 'rate')
        if step.numel() != 1 or step.dtype != torch.int64:
            raise ValueError("Dropout: step must be one int64 on the device")
        if not 1 <= int(site) <= 255:
            raise ValueError("Dropout: site must lie in 1..255")
        self.seed, self.step, self.site, self.rate = int(seed) & 0xFFFFFFFFFFFFFFFF, step, int(site), rate
        self.threshold, self.scale = dropout_threshold(rate), dropout_scale(rate)

    def at(self, site):
        return Dropout(self.seed, self.step, site, self.rate)

    def _args(self):
        return (self.seed, _ptr(self.step, torch.int64, 'step'), self.site, self.threshold, self.scale)


def check_dropout_rate(rate, name='dropout'):
    """None, 0 and 0.0 -> 0.0 (no dropout); a rate outside [0, 1) raises ValueError."""
    if rate is None:
        return 0.0
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= float(rate) < 1.0:
        raise ValueError("{} must be a number in [0, 1) or None (got {!r})".format(name, rate))
    return float(rate)


def dropout_threshold(rate):
    return min(0xFFFFFFFF, int(float(rate) * 4294967296.0 + 0.5))


def dropout_scale(rate):
    return ctypes.c_float(1.0 / (1.0 - float(rate))).value         # the float32 nearest to 1 / (1 - rate)


def dropout(X, drop, out=None):
    """out = X * keep * scale on a 2-D slice (out None: in place); the same call on a gradient slice is the reverse pass."""
    Y = X if out is None else out
    if X.dim() != 2 or tuple(Y.shape) != tuple(X.shape):
        raise ValueError("dropout: X and out [n, C] expected")
    n, C = X.shape
    _launch('amar_dropout_f32', *_mat(X, 'X'), *_mat(Y, 'out'), n, C, *drop._args())
    return Y


def dropout_advance(step):
    """step += 1 on the device: once per training step, after the last kernel that reads it."""
    if step.numel() != 1 or step.dtype != torch.int64:
        raise ValueError("dropout_advance: one int64 on the device expected")
    _launch('amar_dropout_advance', _ptr(step, torch.int64, 'step'))


def gat_layer_dropout(rowptr, colidx, H, s_self, s_neigh, bias, Y, drop, self_loop=True):
    """gat_layer with the attention coefficients dropped after the softmax (training); sorted columns.  Entries (i, j, o) and
    (j, i, o) share one bit (a symmetric multiset's two images of an edge; on a directed graph, a reciprocal pair)."""
    _gat_layer('gat_layer_dropout', rowptr, colidx, H, s_self, s_neigh, bias, Y, self_loop, drop)


def gat_bwd_dropout(rowptr, colidx, H, s_self, s_neigh, Y, dY, bias, a_self, a_neigh, drop, self_loop=True, transposed=None):
    """Reverse of gat_layer_dropout with the regenerated bits. Returns (dout [n, C], ds [n], dt [n], dH [n, C]).
    transposed = (t_rowptr, t_colidx), the stable transpose of the structure, for an edge multiset that is not symmetric
    (amar_gat_bwd_directed_dropout_f32); None: the structure is its own transpose."""
    return _gat_bwd('gat_bwd_dropout', rowptr, colidx, H, s_self, s_neigh, Y, dY, bias, a_self, a_neigh, self_loop, transposed, drop)


class ScatterAddRowsRouteInfo(_RouteInfo):
    """include/amar_hip.h: amar_scatter_add_rows_route_info"""
    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'blocks', 'lds_bytes', 'positions_per_wave')]
    KERNELS = {0: 'owner', 1: 'atomic'}


def scatter_add_rows_route(M, W):
    """Which kernel scatter_add_rows takes for M ids of W columns (amar_scatter_add_rows_route: host only).  A dict: kernel 'owner' |
    'atomic', blocks, lds_bytes, positions_per_wave."""
    info = ScatterAddRowsRouteInfo()
    _call('amar_scatter_add_rows_route', int(M), int(W), ctypes.byref(info))
    return info.as_dict()


def scatter_add_rows(src, ids, dst, base=0):
    if src.shape[0] != ids.numel() or src.shape[1] != dst.shape[1]:
        raise ValueError("scatter_add_rows: src [M, W], ids [M], dst [*, W] expected")
    _launch('amar_scatter_add_rows_f32', *_mat(src, 'src'), _ptr(ids, I32, 'ids'), int(base), *_mat(dst, 'dst'), src.shape[0], src.shape[1])


def add_inplace(dst, src, scale=1.0):
    if tuple(dst.shape) != tuple(src.shape):
        raise ValueError("add_inplace: shapes differ")
    _launch('amar_add_inplace_f32', *_mat(dst, 'dst'), *_mat(src, 'src'), dst.shape[0], dst.shape[1], float(scale))


def row_affine(a, scale, out, b=None):
    """out = (a + b) * scale[row] on strided [M, W] blocks (b optional)."""
    M, W = a.shape
    if tuple(out.shape) != (M, W) or scale.numel() != M or (b is not None and tuple(b.shape) != (M, W)):
        raise ValueError("row_affine: a, b, out [M, W] and scale [M] expected")
    _launch('amar_row_affine_f32', *_mat(a, 'a'), *_mat(b, 'b'), _ptr(scale, F32, 'scale'), *_mat(out, 'out'), M, W)


def l2norm_fwd(z, nrm, inv, y, act='relu'):
    """nrm = l2_normalize(z) per row, inv = the row scale, y = act(nrm)  (GraphSageConv's tail)."""
    M, C = z.shape
    if tuple(nrm.shape) != (M, C) or tuple(y.shape) != (M, C) or inv.numel() != M:
        raise ValueError("l2norm_fwd: z, nrm, y [M, C] and inv [M] expected")
    _launch('amar_l2norm_fwd_f32', *_mat(z, 'z'), *_mat(nrm, 'nrm'), _ptr(inv, F32, 'inv'), *_mat(y, 'y'), M, C, ACT_CODES[act])


def l2norm_bwd(dy, nrm, inv, dz, act='relu'):
    M, C = dy.shape
    if tuple(nrm.shape) != (M, C) or tuple(dz.shape) != (M, C) or inv.numel() != M:
        raise ValueError("l2norm_bwd: dy, nrm, dz [M, C] and inv [M] expected")
    _launch('amar_l2norm_bwd_f32', *_mat(dy, 'dy'), *_mat(nrm, 'nrm'), _ptr(inv, F32, 'inv'), *_mat(dz, 'dz'), M, C, ACT_CODES[act])


def _transposed_ptrs(transposed, n, colidx):
    """The two extra pointers of the `directed` GAT reverse entry points (nothing for the symmetric ones)."""
    if transposed is None:
        return ()
    t_rowptr, t_colidx = transposed
    if t_rowptr.numel() != n + 1 or t_colidx.numel() != colidx.numel():
        raise ValueError("gat_bwd: transposed = (t_rowptr [n + 1], t_colidx [nnz]) of the same square structure expected")
    return _ptr(t_rowptr, I32, 't_rowptr'), _ptr_entries(t_colidx, I32, 't_colidx')


# (directed structure, dropout) -> the reverse entry point: the directed ones take the transpose after the structure, the
# dropout ones the dropout site before the stream
_GAT_BWD_SYMBOLS = {(False, False): 'amar_gat_bwd_f32', (True, False): 'amar_gat_bwd_directed_f32',
                    (False, True): 'amar_gat_bwd_dropout_f32', (True, True): 'amar_gat_bwd_directed_dropout_f32'}


def _gat_bwd(what, rowptr, colidx, H, s_self, s_neigh, Y, dY, bias, a_self, a_neigh, self_loop, transposed, drop):
    """gat_bwd (drop None) and gat_bwd_dropout."""
    n = rowptr.numel() - 1
    C = H.shape[1]
    if tuple(Y.shape) != (n, C) or tuple(dY.shape) != (n, C) or H.shape[0] != n or bias.numel() != C or \
            a_self.numel() != C or a_neigh.numel() != C:
        raise ValueError("{}: H, Y, dY [n, C]; bias, a_self, a_neigh [C] expected".format(what))
    dev = H.device
    dout = torch.empty((n, C), dtype=torch.float32, device=dev)
    scratch = torch.empty(3 * n, dtype=torch.float32, device=dev)
    ds, dt = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    dH = torch.empty((n, C), dtype=torch.float32, device=dev)
    _launch(_GAT_BWD_SYMBOLS[transposed is not None, drop is not None], _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'),
            *_transposed_ptrs(transposed, n, colidx), *_mat(H, 'H'), C, _ptr(s_self, F32, 's_self'), _ptr(s_neigh, F32, 's_neigh'), *_mat(Y, 'Y'),
            *_mat(dY, 'dY'), _ptr(bias, F32, 'bias'), _ptr(a_self, F32, 'a_self'), _ptr(a_neigh, F32, 'a_neigh'), _ptr(dout), _ptr(scratch), _ptr(ds),
            _ptr(dt), _ptr(dH), C, 1 if self_loop else 0, n, *(drop._args() if drop is not None else ()))
    return dout, ds, dt, dH


def gat_bwd(rowptr, colidx, H, s_self, s_neigh, Y, dY, bias, a_self, a_neigh, self_loop=True, transposed=None):
    """Reverse of gat_layer. Returns (dout [n, C], ds [n], dt [n], dH [n, C]).  transposed = (t_rowptr, t_colidx): as
    gat_bwd_dropout (amar_gat_bwd_directed_f32)."""
    return _gat_bwd('gat_bwd', rowptr, colidx, H, s_self, s_neigh, Y, dY, bias, a_self, a_neigh, self_loop, transposed, None)


def csr_transpose(rowptr, colidx, n_cols):
    """The stable transpose of an int32 CSR structure [n_rows, n_cols] (amar_csr_transpose_i32): returns (t_rowptr [n_cols + 1],
    t_colidx [nnz], perm [nnz]) with perm[q] = the input position of the entry at output position q — inside an output row the
    entries keep the order of their input positions, so values and multiplicities follow as vals[perm].  Same bits on every run.
    Checks the structure first (two host reads; this runs once per graph, never inside a captured graph)."""
    n_rows, n_cols, nnz = int(rowptr.numel()) - 1, int(n_cols), int(colidx.numel())
    if n_rows < 0 or n_cols < 0:
        raise ValueError("csr_transpose: rowptr [n_rows + 1] and n_cols >= 0 expected")
    dev = rowptr.device
    _ptr(rowptr, I32, 'rowptr'), _ptr(colidx, I32, 'colidx')                     # on the device, int32: before the host reads below
    if int(rowptr[0]) != 0 or int(rowptr[-1]) != nnz:
        raise ValueError("csr_transpose: rowptr must run from 0 to nnz")
    if nnz and (n_rows < 1 or bool((rowptr[1:] < rowptr[:-1]).any()) or int(colidx.min()) < 0 or int(colidx.max()) >= n_cols):
        raise ValueError("csr_transpose: rowptr must not decrease and every column must lie in [0, n_cols)")
    t_rowptr = torch.empty(n_cols + 1, dtype=torch.int32, device=dev)
    t_colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
    perm = torch.empty(nnz, dtype=torch.int32, device=dev)
    cursor = torch.empty(max(n_cols, 1), dtype=torch.int32, device=dev)
    _launch('amar_csr_transpose_i32', _ptr(rowptr, I32, 'rowptr'), _ptr_entries(colidx, I32, 'colidx'), n_rows, n_cols, nnz, _ptr(t_rowptr, I32, 't_rowptr'),
            _ptr_entries(t_colidx, I32, 't_colidx'), _ptr_entries(perm, I32, 'perm'), _ptr(cursor, I32, 'cursor'))
    return t_rowptr, t_colidx, perm


def attention_mix(a, b, ta, tb, out):
    """out = wa * a + (1 - wa) * b with wa = sigmoid(tanh(ta) - tanh(tb)) per feature (FusionLayer 'attention')."""
    M, D = a.shape
    if any(tuple(t.shape) != (M, D) for t in (b, ta, tb, out)):
        raise ValueError("attention_mix: five [M, D] blocks expected")
    _launch('amar_attention_mix_f32', *_mat(a, 'a'), *_mat(b, 'b'), *_mat(ta, 'ta'), *_mat(tb, 'tb'), *_mat(out, 'out'), M, D)


def attention_mix_bwd(dout, a, b, ta, tb):
    """Returns (dA, dB, dTA, dTB), contiguous [M, D]."""
    M, D = a.shape
    if any(tuple(t.shape) != (M, D) for t in (dout, b, ta, tb)):
        raise ValueError("attention_mix_bwd: five [M, D] blocks expected")
    outs = [torch.empty((M, D), dtype=torch.float32, device=a.device) for _ in range(4)]
    _launch('amar_attention_mix_bwd_f32', *_mat(dout, 'dout'), *_mat(a, 'a'), *_mat(b, 'b'), *_mat(ta, 'ta'), *_mat(tb, 'tb'),
            _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), M, D)
    return outs


def add3_act(a, b, c, out, act='relu'):
    M, W = a.shape
    if any(tuple(t.shape) != (M, W) for t in (b, c, out)):
        raise ValueError("add3_act: four [M, W] blocks expected")
    _launch('amar_add3_act_f32', *_mat(a, 'a'), *_mat(b, 'b'), *_mat(c, 'c'), *_mat(out, 'out'), M, W, ACT_CODES[act])


def locality_scale(x, w, out):
    """out = x * sigmoid(w[row])  (DGCFConv's LocalityAdaptive)."""
    M, W = x.shape
    if tuple(out.shape) != (M, W) or w.numel() != M or not w.is_contiguous():
        raise ValueError("locality_scale: x, out [M, W] and contiguous w [M] expected")
    _launch('amar_locality_scale_f32', *_mat(x, 'x'), _ptr(w, F32, 'w'), *_mat(out, 'out'), M, W)


def locality_scale_bwd(dout, x, w, dx, dw, accumulate=False):
    M, W = x.shape
    if tuple(dout.shape) != (M, W) or tuple(dx.shape) != (M, W) or w.numel() != M or dw.numel() != M:
        raise ValueError("locality_scale_bwd: dout, x, dx [M, W]; w, dw [M] expected")
    _launch('amar_locality_scale_bwd_f32', *_mat(dout, 'dout'), *_mat(x, 'x'), _ptr(w, F32, 'w'), *_mat(dx, 'dx'), _ptr(dw, F32, 'dw'), M, W,
            1 if accumulate else 0)


def transpose(src):
    K, N = src.shape
    if not src.is_contiguous():
        raise ValueError("transpose: contiguous [K, N] expected")
    dst = torch.empty((N, K), dtype=torch.float32, device=src.device)
    _launch('amar_transpose_f32', _ptr(src, F32, 'src'), K, N, _ptr(dst))
    return dst


def adam(w, g, m, v, lr_t, beta_1, beta_2, epsilon, l2=0.0):
    if not (w.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()) or \
            not (w.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adam: contiguous tensors of equal size expected")
    _launch('amar_adam_f32', _ptr(w, F32, 'w'), _ptr(g, F32, 'g'), _ptr(m, F32, 'm'), _ptr(v, F32, 'v'), w.numel(), float(lr_t), float(beta_1), float(beta_2),
            float(epsilon), float(l2))
