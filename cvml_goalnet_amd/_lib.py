"""ctypes binding of libgoalnet_hip.so (C ABI: include/goalnet_hip.h).

The product path has no CPU or eager-PyTorch fallback: if the shared library is missing or a call
fails, an exception is raised (task rule ③: "the product path must fail loudly when the HIP extension
is missing").
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOALNET_LIB_PATH") or os.path.join(_HERE, "libgoalnet_hip.so")   # override: A/B builds of the kernels
ABI_VERSION = 7
STAT_PARTS = 1024
ADAM_RANGES_MAX = 32      # GOALNET_ADAM_RANGES_MAX

P = c_void_p  # device pointers and the stream travel as void*


class RowCopy(ctypes.Structure):
    """goalnet_rowcopy (include/goalnet_hip.h)"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("row_bytes", c_int64), ("nrows", c_int), ("gather", c_int), ("cursor", c_void_p),
                ("cursor_bias", c_int64)]


class RowCopyIndexed(ctypes.Structure):
    """goalnet_rowcopy_indexed (include/goalnet_epoch.h)"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("row_bytes", c_int64), ("nrows", c_int), ("gather", c_int), ("cursor", c_void_p),
                ("cursor_bias", c_int64), ("indexed", c_int), ("table_rows", c_int64)]


class RowMix(ctypes.Structure):
    """goalnet_rowmix (include/goalnet_mix.h)"""
    _fields_ = [("table", c_void_p), ("dst", c_void_p), ("row_elems", c_int64), ("nrows", c_int), ("cursor", c_void_p), ("cursor_bias", c_int64),
                ("table_rows", c_int64)]


class AdamRange(ctypes.Structure):
    """goalnet_adam_range (include/goalnet_hip.h)"""
    _fields_ = [("begin", c_int64), ("count", c_int64), ("skipped", c_int64)]


class OptimRange(ctypes.Structure):
    """goalnet_optim_range (include/goalnet_optim.h)"""
    _fields_ = [("begin", c_int64), ("count", c_int64), ("skipped", c_int64), ("decay", c_int32), ("pad", c_int32)]


class OptimOpts(ctypes.Structure):
    """goalnet_optim_opts (include/goalnet_optim.h)"""
    _fields_ = [("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
                ("max_norm", c_double), ("min_lr", c_double), ("gamma", c_double), ("warmup", c_int64), ("total", c_int64),
                ("period", c_int64), ("decoupled", c_int32), ("schedule", c_int32)]


class GroupHyper(ctypes.Structure):
    """goalnet_group_hyper (include/goalnet_groups.h)"""
    _fields_ = [("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
                ("amsgrad", c_int32), ("pad", c_int32)]


class GroupRange(ctypes.Structure):
    """goalnet_group_range (include/goalnet_groups.h)"""
    _fields_ = [("begin", c_int64), ("count", c_int64), ("skipped", c_int64), ("decay", c_int32), ("group", c_int32)]


class EmaOpts(ctypes.Structure):
    """goalnet_ema_opts (include/goalnet_ema.h)"""
    _fields_ = [("decay", c_double), ("every", c_int64), ("start_step", c_int64), ("warmup", c_int32), ("pad", c_int32)]


# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_hip.h
PROTOTYPES = {
    "goalnet_abi_version": (c_int, []),
    "goalnet_last_error": (c_char_p, []),
    "goalnet_fill_uniform": (c_int, [P, c_int64, c_uint64, c_uint32, c_float, c_float, P]),
    "goalnet_dropout_mask": (c_int, [P, c_int64, c_uint64, c_uint32, c_float, P]),
    "goalnet_transpose_inner": (c_int, [P, P, c_int64, c_int64, c_int64, P]),
    "goalnet_conv3x3_weight_flip": (c_int, [P, P, c_int, c_int, P]),
    "goalnet_conv3x3_weight_flip2": (c_int, [P, P, c_int, c_int, P, P, c_int, c_int, P]),
    "goalnet_conv1_fwd": (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    "goalnet_conv1_wgrad_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "goalnet_conv1_wgrad": (c_int, [P, P, P, P, P, c_size_t, c_int, c_int, c_int, P]),
    "goalnet_conv1_dgrad": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_stat_parts": (c_int, [c_int64]),
    "goalnet_pool_bnstats_fwd": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_pool_bnstats_fwd_p16": (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_bn_finalize": (c_int, [P, c_int, P, P, P, P, c_float, c_float, c_int64, c_int, P, P, P, P, P]),
    "goalnet_pool_bn_eval_fwd": (c_int, [P, c_int, P, c_int, P, P, P, P, P, c_float, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_bn_bwd_finalize_eval": (c_int, [P, c_int, P, P, c_int, P, P, P, P]),
    "goalnet_bn_bwd_reduce": (c_int, [P, P, P, P, P, c_int, c_int64, c_int, P]),
    "goalnet_bn_bwd_reduce_t": (c_int, [P, c_int, P, c_int, P, P, P, c_int, c_int64, c_int, c_int, P]),
    "goalnet_bn_bwd_finalize": (c_int, [P, c_int, P, P, P, c_int64, c_int, P, P, P, P]),
    "goalnet_bnpool_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_bnpool_bwd_bf16p": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_bnpool_bwd_bf16p_t": (c_int, [P, c_int, P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_bn_small_ws_bytes": (c_size_t, [c_int]),
    "goalnet_pool_bn_fwd_small": (c_int, [P, P, P, P, P, P, P, c_float, c_float, P, P, P, P, P, c_size_t, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_bn_bwd_reduce_small": (c_int, [P, P, P, P, P, P, P, P, P, c_size_t, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_bn_bwd_reduce_small_eval": (c_int, [P, P, P, P, P, P, P, P, P, c_size_t, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_bnpool_bwd_small": (c_int, [P, P, P, P, P, P, P, c_size_t, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_partials_sum": (c_int, [P, c_int, c_int64, c_int, P, P]),
    "goalnet_partials_sum2": (c_int, [P, c_int, c_int, P, P, c_int, c_int, P, P]),
    "goalnet_partials_sum_f64": (c_int, [P, c_int, c_int64, c_int, P, P]),
    "goalnet_conv3x3_fwd_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_fwd": (c_int, [P, P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P, c_int, P]),
    "goalnet_conv3x3_fwd_kernel_name": (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_fwd_bf16p_kernel_name": (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_wgrad_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_wgrad_codes_bytes": (c_size_t, [c_int, c_int, c_int]),
    "goalnet_conv3x3_wgrad_codes": (c_int, [P, c_int, c_int, c_int, P]),
    "goalnet_conv3x3_wgrad": (c_int, [P, P, P, P, P, P, c_size_t, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_cast_bf16": (c_int, [P, P, c_int64, c_int, P]),
    "goalnet_cast_f32": (c_int, [P, P, c_int64, c_int, P]),
    "goalnet_bn_apply_bf16": (c_int, [P, P, P, P, c_int64, c_int, c_int, P]),
    "goalnet_bn_apply_bf16_p16": (c_int, [P, P, P, P, c_int64, c_int, c_int, P]),
    "goalnet_conv3x3_fwd_bf16": (c_int, [P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_linear_fwd_bf16_ws_bytes": (c_size_t, [c_int, c_int64, c_int]),
    "goalnet_linear_fwd_bf16": (c_int, [P, c_int64, P, P, c_int, P, c_int64, P, c_int64, P, c_int64, c_int, c_int64, c_int, P, c_size_t, c_int, P]),
    "goalnet_bf16_padded_layout": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "goalnet_to_bf16_padded": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_to_bf16_padded_p16": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_conv3x3_fwd_bf16p_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_fwd_bf16p": (c_int, [P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, c_int, P]),
    "goalnet_conv3x3_wgrad_bf16_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_wgrad_bf16": (c_int, [P, P, P, P, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_absmax": (c_int, [P, c_int64, P, P, c_int, c_int64, c_int64, P, P]),
    "goalnet_split_scales": (c_int, [P, P, P, P]),
    "goalnet_split_padded": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "goalnet_split_rows": (c_int, [c_int, P, c_int64, P, P, c_int, P, P, c_int64, c_int64, P]),
    "goalnet_conv3x3_fwd_split": (c_int, [c_int, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "goalnet_conv3x3_wgrad_split_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_wgrad_split": (c_int, [c_int, P, P, P, P, c_size_t, c_int, c_int, c_int, c_int, c_int, P, P]),
    "goalnet_linear_split_ok": (c_int, [c_int, c_int, c_int64, c_int]),
    "goalnet_linear_fwd_split_ws_bytes": (c_size_t, [c_int, c_int, c_int64, c_int]),
    "goalnet_linear_fwd_split": (c_int, [c_int, P, P, P, c_int, P, c_int64, P, c_int64, P, c_int64, c_int, c_int64, c_int, P, c_size_t, P, P]),
    "goalnet_linear_bwd_dx_split": (c_int, [c_int, P, P, P, c_int64, c_int, c_int64, c_int, P, P]),
    "goalnet_linear_bwd_dw_split": (c_int, [c_int, P, P, P, c_int, c_int64, c_int, P, P]),
    "goalnet_linear_bwd_dx_bf16": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, c_int, c_int64, c_int, c_int, P]),
    "goalnet_linear_bwd_dx_bf16_o16_ok": (c_int, [c_int, c_int64, c_int]),
    "goalnet_linear_bwd_dx_bf16_o16": (c_int, [P, c_int64, P, P, c_int64, c_int, c_int64, c_int, c_int, P]),
    "goalnet_conv3x3_fwd_bf16p_o16_ok": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv3x3_fwd_bf16p_o16": (c_int, [P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_linear_bwd_dw_bf16": (c_int, [P, c_int64, P, c_int64, P, c_int, c_int64, c_int, c_int, P]),
    "goalnet_linear_fwd_ws_bytes": (c_size_t, [c_int, c_int64, c_int]),
    "goalnet_linear_fwd": (c_int, [P, c_int64, P, P, c_int, P, P, c_int, P, c_int64, P, c_int64, P, c_int64,
                                   c_int, c_int64, c_int, P, c_size_t, P]),
    "goalnet_linear_bwd_dx": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, c_int, c_int64, c_int, P]),
    "goalnet_linear_bwd_dw": (c_int, [P, c_int64, P, c_int64, P, P, c_int, P, P, c_int, c_int64, c_int, P]),
    "goalnet_linear_bwd_dw_adam": (c_int, [P, c_int64, P, c_int64, P, P, c_int, P, P, P, P, c_int, c_int64, c_int,
                                           c_double, c_double, c_double, c_double, P, c_int64, c_float, P]),
    "goalnet_colsum": (c_int, [P, c_int64, c_int, c_int, P, P]),
    "goalnet_mul": (c_int, [P, c_int64, P, c_int64, P, c_int64, c_int, c_int, P]),
    "goalnet_conv1d_fwd": (c_int, [P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_conv1d_bwd_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "goalnet_conv1d_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "goalnet_conv1d_bwd_small_ok": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "goalnet_conv1d_bwd_small": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_relu_bwd": (c_int, [P, P, P, c_int64, P]),
    "goalnet_mlp_blocks": (c_int, []),
    "goalnet_mlp_fwd": (c_int, [P, c_int64, c_int, P, P, P, P, P, P, P, P, P, P, P, c_int, P, P]),
    "goalnet_mlp_bwd_ws_bytes": (c_size_t, [c_int]),
    "goalnet_mlp_bwd": (c_int, [P, P, P, c_int64, P, c_int64, P, P, P, P, c_int64, P, c_int, c_int, c_int, P, c_size_t, P, P]),
    "goalnet_head_fwd": (c_int, [P, c_int64, P, P, P, P, c_int, c_int, P]),
    "goalnet_head_bwd": (c_int, [P, P, P, c_int64, P, P, c_int64, P, c_int64, P, P, c_int, c_int, P]),
    "goalnet_mse_bcast": (c_int, [P, P, c_int, P, P, P]),
    "goalnet_cubic_resample": (c_int, [P, P, P, c_int64, c_int, c_int, P]),
    "goalnet_logmel_slots": (c_int, [P, P, P, c_int, c_int, P, P, P, P, P, P, P, P]),
    "goalnet_mfcc_from_logmel": (c_int, [P, P, c_int, c_int, P, P, P, P, c_int, c_int, c_double, P]),
    "goalnet_cls_head_fwd": (c_int, [P, c_int64, P, P, P, P, c_int, c_int, c_int, P]),
    "goalnet_cross_entropy": (c_int, [P, P, P, P, c_int, c_int, P]),
    "goalnet_cls_head_bwd": (c_int, [P, P, P, c_int64, P, P, c_int64, P, c_int64, P, P, c_int, c_int, c_int, P]),
    "goalnet_argmax_plus1": (c_int, [P, P, c_int, c_int, P]),
    "goalnet_adam_step": (c_int, [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, c_int, c_float, P]),
    "goalnet_counter_add": (c_int, [P, c_int64, P]),
    "goalnet_dropout_masks_dev": (c_int, [P, c_int, ctypes.POINTER(c_int), c_int, c_uint64, c_uint32, c_uint32, P, c_float, c_int64, P]),
    "goalnet_adam_step_dev": (c_int, [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, P, c_int64, c_float, P]),
    "goalnet_adam_step_dev_blocks": (c_int, [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, P, c_int64, c_float, c_int, P]),
    "goalnet_adam_step_dev_shadow": (c_int, [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, P, c_int64, c_float, P, c_int64,
                                             c_int64, c_int, P]),
    "goalnet_adam_step_dev_guarded": (c_int, [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, P, c_int64, c_float, P, c_int64,
                                              c_int64, c_int, P, P]),
    "goalnet_adam_step_dev_ranges": (c_int, [P, P, P, P, ctypes.POINTER(AdamRange), c_int, c_double, c_double, c_double, c_double, P, c_float,
                                             P, c_int64, c_int64, c_int, P, P]),
    "goalnet_scale": (c_int, [P, c_int64, c_float, P]),
    "goalnet_grad_finite_check": (c_int, [P, c_int64, P, c_int64, P, P, P]),
    "goalnet_counters_add4": (c_int, [P, c_int64, c_int64, c_int64, c_int64, P]),
    "goalnet_counters_add4_guarded": (c_int, [P, c_int64, c_int64, c_int64, c_int64, P, P]),
    "goalnet_rows_scatter_tick": (c_int, [ctypes.POINTER(RowCopy), c_int, P, c_int64, c_int64, c_int64, c_int64, P, P]),
    "goalnet_rows_copy_batch": (c_int, [ctypes.POINTER(RowCopy), c_int, P]),
    "goalnet_frames_preprocess": (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, P, P]),
    "goalnet_frames_preprocess_strided": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P, P]),
    "goalnet_gather_clips_ws_bytes": (c_size_t, [c_int]),
    "goalnet_gather_clips": (c_int, [P, c_int, c_int64, P, P, c_int, P, c_int64, P, P, P, P, c_size_t, P]),
    "goalnet_kts_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "goalnet_kts": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_int, c_int, P, P, P, P, P, P, P, c_size_t, P]),
    "goalnet_rank_corr": (c_int, [P, c_int64, c_int, P, c_int64, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P]),
    "goalnet_knapsack_ws_bytes": (c_size_t, [c_int, c_int]),
    "goalnet_knapsack": (c_int, [P, P, c_int, c_int, P, P, c_size_t, P]),
    "goalnet_fscore": (c_int, [P, P, c_int, c_int, P, P, P]),
    "goalnet_postprocess_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "goalnet_postprocess": (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, c_int, P, c_int, P, P, P, P, P, P, P, c_size_t, P]),
    "goalnet_postprocess_batch_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "goalnet_postprocess_batch": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, P, c_int, P, P, P, P, P, P, P, c_size_t, P]),
    "goalnet_postprocess_batch_kernel_name": (c_char_p, [c_int, c_int]),
    "goalnet_mean_annotations": (c_int, [P, c_int, c_int, c_int, P, P, P]),
    "goalnet_rows_gather": (c_int, [P, P, c_int64, c_int, P, P]),
    "goalnet_rows_scatter": (c_int, [P, P, c_int64, c_int, P, P]),
}

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_loss.h, the second public header: additions
# that leave include/goalnet_hip.h, PROTOTYPES and ABI_VERSION as they are
LOSS_PROTOTYPES = {
    "goalnet_frame_loss_ws_bytes": (c_size_t, [c_int, c_int]),
    "goalnet_frame_loss": (c_int, [c_int, c_double, P, P, P, c_int, P, P, P, c_size_t, P]),
    "goalnet_mlp_fwd_loss": (c_int, [P, c_int64, c_int, P, P, P, P, P, P, P, P, P, P, P, c_int, c_double, P, c_int, P, P]),
}
# GOALNET_LOSS_* (include/goalnet_loss.h)
LOSS_KINDS = {"mse_bcast": 0, "mse": 1, "l1": 2, "smooth_l1": 3, "rank": 4}
FRAME_LOSS_MAX_N = 65536


# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_epoch.h, the third public header (shuffled,
# augmented passes over a resident video): additions again, the first two tables stay as they are
EPOCH_PROTOTYPES = {
    "goalnet_epoch_plan": (c_int, [P, c_int, c_uint64, c_uint32, c_int, c_float, c_int, c_float, c_float, P]),
    "goalnet_frames_gather_aug": (c_int, [P, c_int64, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int64, c_int, P]),
    "goalnet_rows_copy_indexed": (c_int, [ctypes.POINTER(RowCopyIndexed), c_int, P, c_int, P]),
}
EPOCH_MAX_N = 65536       # GOALNET_EPOCH_MAX_N
PLAN_WORDS = 8            # GOALNET_PLAN_WORDS
MAX_SHIFT = 32767         # GOALNET_MAX_SHIFT
ROWCOPY_MAX = 4           # GOALNET_ROWCOPY_MAX

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_optim.h, the fourth public header (weight decay,
# gradient-norm clipping and learning-rate schedules on the fused step): additions, the tables above stay as they are
OPTIM_PROTOTYPES = {
    "goalnet_grad_sumsq_ws_bytes": (c_size_t, [ctypes.POINTER(OptimRange), c_int]),
    "goalnet_grad_sumsq": (c_int, [P, ctypes.POINTER(OptimRange), c_int, P, P, c_size_t, P]),
    "goalnet_optim_step_dev_ranges": (c_int, [P, P, P, P, ctypes.POINTER(OptimRange), c_int, ctypes.POINTER(OptimOpts), P, c_float, P,
                                              P, c_int64, c_int64, c_int, P, P]),
    "goalnet_optim_lr": (c_int, [ctypes.POINTER(OptimOpts), P, P, P]),
}
SCHEDULES = {"constant": 0, "cosine": 1, "step": 2}       # GOALNET_SCHED_* (include/goalnet_optim.h)

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_ema.h, the fifth public header (the weight
# average behind the fused step and the exchange of two arenas): additions, the tables above stay as they are
EMA_PROTOTYPES = {
    "goalnet_ema_update_dev_ranges": (c_int, [P, P, ctypes.POINTER(AdamRange), c_int, ctypes.POINTER(EmaOpts), P, c_int64, P, P]),
    "goalnet_swap_ranges": (c_int, [P, P, ctypes.POINTER(AdamRange), c_int, P]),
}

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_accum.h, the sixth public header (gradient
# accumulation over the sub-batches of a window): additions, the tables above stay as they are
ACCUM_PROTOTYPES = {
    "goalnet_grad_accum_dev_ranges": (c_int, [P, P, ctypes.POINTER(AdamRange), c_int, c_float, c_int, P]),
}

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_groups.h, the seventh public header (parameter
# groups and AMSGrad on the fused step): additions, the tables above stay as they are
GROUPS_PROTOTYPES = {
    "goalnet_group_step_dev_ranges": (c_int, [P, P, P, P, P, ctypes.POINTER(GroupRange), c_int, ctypes.POINTER(GroupHyper), c_int,
                                              ctypes.POINTER(OptimOpts), P, c_float, P, P, c_int64, c_int64, c_int, P, P]),
    "goalnet_group_lr": (c_int, [ctypes.POINTER(OptimOpts), ctypes.POINTER(GroupHyper), c_int, P, P, P]),
}
GROUPS_MAX = 8            # GOALNET_GROUPS_MAX

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_mix.h, the eighth public header (audio
# augmentation and mixup on a shuffled / augmented pass): additions, the tables above stay as they are
MIX_PROTOTYPES = {
    "goalnet_epoch_plan2": (c_int, [P, P, c_int, c_uint64, c_uint32, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, P]),
    "goalnet_audio_gather_aug": (c_int, [P, c_int64, P, P, P, c_int, c_int, c_int, c_int, P, c_int64, c_int, c_float, P]),
    "goalnet_frames_gather_mix": (c_int, [P, c_int64, P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int64, c_int, P]),
    "goalnet_rows_mix_indexed": (c_int, [ctypes.POINTER(RowMix), c_int, P, P, c_int, P]),
}
PLAN2_WORDS = 12          # GOALNET_PLAN2_WORDS
PLAN2_MAX_INDEX = 1 << 26  # GOALNET_PLAN2_MAX_INDEX
AUDIO_GAIN, AUDIO_NOISE, AUDIO_MIX = 1, 2, 4      # GOALNET_AUDIO_*

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_wave.h, the ninth public header (the audio
# front end: downmix and polyphase resampling to the feature rate): additions, the tables above stay as they are
WAVE_PROTOTYPES = {
    "goalnet_wave_plan": (c_int, [c_int, c_int, c_int64, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                  ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "goalnet_wave_resample": (c_int, [P, c_int, c_int64, c_int, P, c_int, c_int, c_int, c_int, P, c_int64, P]),
}
WAVE_F32, WAVE_S16 = 0, 1         # GOALNET_WAVE_F32 / _S16
WAVE_MAX_RATIO = 16               # GOALNET_WAVE_MAX_RATIO
WAVE_MAX_CHANNELS = 8             # GOALNET_WAVE_MAX_CHANNELS
WAVE_MAX_RATE = 1 << 24           # GOALNET_WAVE_MAX_RATE

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_nv12.h, the tenth public header (NV12 frames
# in: conversion, strided pre-processing and clip gather): additions, the tables above stay as they are. `coeffs`
# is a HOST int32[8] table (checked before any launch), so it travels as a ctypes pointer, not as a device address
NV12_PROTOTYPES = {
    "goalnet_nv12_to_bgr": (c_int, [P, c_int, c_int, c_int, c_int64, c_int64, c_int64, ctypes.POINTER(c_int32), P, P]),
    "goalnet_nv12_preprocess_strided": (c_int, [P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, ctypes.POINTER(c_int32), P, c_int,
                                                c_int, P, P]),
    "goalnet_nv12_gather_clips_bgr_ws_bytes": (c_size_t, [c_int]),
    "goalnet_nv12_gather_clips_bgr": (c_int, [P, c_int, c_int, c_int, c_int64, c_int64, c_int64, ctypes.POINTER(c_int32), P, P, c_int, P,
                                              c_int64, P, P, P, P, c_size_t, P]),
}
NV12_MIN_SHIFT, NV12_MAX_SHIFT = 8, 24        # GOALNET_NV12_MIN_SHIFT / _MAX_SHIFT

# name -> (restype, [argtypes])   — one row per entry point declared in include/goalnet_storyboard.h, the eleventh public header (the
# static summary: keyframes, thumbnails and a contact sheet): additions, the tables above stay as they are. The NV12
# colour table is HOST memory, as in NV12_PROTOTYPES
STORYBOARD_PROTOTYPES = {
    "goalnet_storyboard_keyframes": (c_int, [P, c_int, c_int, c_int, P, P, c_int, c_int, P, P, P, c_int, P, P]),
    "goalnet_storyboard_render": (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "goalnet_storyboard_render_nv12": (c_int, [P, c_int, c_int, c_int, c_int64, c_int64, c_int64, ctypes.POINTER(c_int32), P, c_int, c_int,
                                               c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]),
}
STORYBOARD_MAX_CLIPS = 4096       # GOALNET_STORYBOARD_MAX_CLIPS
STORYBOARD_MAX_DIM = 16384        # GOALNET_STORYBOARD_MAX_DIM

_lib = None


class GoalnetError(RuntimeError):
    pass


def load():
    """Load libgoalnet_hip.so (built by __graft_entry__.build()). Raises if absent — no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GoalnetError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no CPU / eager fallback for the AVM hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (*PROTOTYPES.items(), *LOSS_PROTOTYPES.items(), *EPOCH_PROTOTYPES.items(), *OPTIM_PROTOTYPES.items(),
                              *EMA_PROTOTYPES.items(), *ACCUM_PROTOTYPES.items(), *GROUPS_PROTOTYPES.items(), *MIX_PROTOTYPES.items(),
                              *WAVE_PROTOTYPES.items(), *NV12_PROTOTYPES.items(), *STORYBOARD_PROTOTYPES.items()):
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.goalnet_abi_version()
    if v != ABI_VERSION:
        raise GoalnetError(f"libgoalnet_hip.so ABI {v} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().goalnet_last_error()
        raise GoalnetError(f"{what}: rc={rc}: {msg.decode() if msg else ''}")
