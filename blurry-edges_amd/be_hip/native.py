"""ctypes binding of libblurry_edges_hip.so (the C ABI declared in include/blurry_edges_hip.h).

This module is the only place the Python host side touches native code.  There is NO fallback: if the
shared library is missing or a tensor is not a contiguous fp32 CUDA(HIP) tensor, the call raises.
PyTorch is used for device memory and the current stream only.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BE_LIB_DIR: another build of the SAME C ABI (e.g. lib/wino3 from `make -C csrc wino3`, the 5x5-tile Winograd A/B library); the torch
# extension links against the default library, so an alternative directory runs on the ctypes binding
_ALT_DIR = os.environ.get("BE_LIB_DIR")
LIB_PATH = os.path.join(_ALT_DIR or os.path.join(os.path.dirname(_HERE), "lib"), "libblurry_edges_hip.so")

BE_R = 21
NPIX = 441
NTENSORS = 86


class PackJob(C.Structure):
    """be_pack_job (include/blurry_edges_hip.h): one be_conv_pack_f32 / be_conv_pack_dgrad_f32 call of a job table."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
                ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p), ("packed_w", C.c_void_p), ("packed_bias", C.c_void_p),
                ("bn_eps", C.c_float), ("cout", C.c_int), ("cin", C.c_int), ("ksize", C.c_int), ("layout_chw_hw", C.c_int),
                ("dgrad", C.c_int)]


class AdamEntry(C.Structure):
    """be_adam_entry: one workgroup's slice of a parameter for be_clip_adamw_f32."""
    _fields_ = [("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("goff", C.c_int64), ("n", C.c_int)]


class DepthConsts(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("s", "numerator", "den_const", "k", "k2", "intercept", "sin_w", "cos_w", "sin_m", "cos_m")]


class RenderOpts(C.Structure):
    _fields_ = [("lambda_ridge", C.c_float), ("w", C.c_float), ("delta_sq", C.c_float),
                ("wrap_angles", C.c_int), ("lin", C.c_float * BE_R)]


class PatchView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("s_aperture", C.c_int64), ("s_chan", C.c_int64), ("s_row", C.c_int64),
                ("s_col", C.c_int64), ("s_pi", C.c_int64), ("s_pj", C.c_int64), ("wp", C.c_int)]


RECORD_FLOATS = 32


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n", "h", "w", "cin", "cout", "ksize", "act")]


class TrainUnitFwd(C.Structure):
    """be_train_unit_fwd: one unit of be_train_unit_pair_fwd_f32 (the arguments of be_train_unit_fwd_f32 as a struct)."""
    _fields_ = [("desc", ConvDesc)] + [(n, C.c_void_p) for n in
                ("x", "packed_w", "packed_bias", "gamma", "beta", "res", "run_mean", "run_var", "y", "mean", "invstd", "s_in", "out")] + \
               [("act", C.c_int)]


class TrainUnitBwd(C.Structure):
    """be_train_unit_bwd: one unit of be_train_unit_pair_bwd_f32."""
    _fields_ = [("desc", ConvDesc)] + [(n, C.c_void_p) for n in
                ("x", "dout", "s_in", "y", "mean", "invstd", "gamma", "dgrad_packed_w", "dgrad_packed_bias", "dx_add")] + \
               [("layout_chw_hw", C.c_int)] + [(n, C.c_void_p) for n in ("ds", "dy", "dgamma", "dbeta", "dw", "db", "dx")]


_P = C.c_void_p
_SIGNATURES = {
    "be_version": (C.c_int, []),
    "be_last_error": (C.c_char_p, []),
    "be_params2etas_f32": (C.c_int, [_P, _P, C.c_int64, _P]),
    "be_etas2depth_f32": (C.c_int, [C.POINTER(DepthConsts), _P, _P, _P, _P, C.c_int64, _P]),
    "be_depth2sigma_f32": (C.c_int, [C.POINTER(DepthConsts), _P, C.c_float, _P, C.c_int64, _P]),
    "be_local_depth_f32": (C.c_int, [C.POINTER(DepthConsts), _P, _P, C.c_int64, _P]),
    "be_render_colors_f32": (C.c_int, [C.POINTER(RenderOpts), _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "be_local_stage_packed_floats": (C.c_size_t, []),
    "be_local_stage_pack_f32": (C.c_int, [C.POINTER(_P), C.c_float, _P, _P]),
    "be_local_stage_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "be_local_stage_forward_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_size_t, _P, _P]),
    "be_local_stage_forward_view_f32": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_size_t, _P, _P]),
    "be_render_colors_view_f32": (C.c_int, [C.POINTER(RenderOpts), _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P,
                                            C.c_int64, _P]),
    "be_view_to_nhwc4_f32": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P]),
    "be_conv_packed_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_conv_pack_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "be_conv_pack_jobs_f32": (C.c_int, [_P, C.c_int, _P]),
    "be_conv_nhwc_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.c_int, _P]),
    "be_conv_nhwc_splitk_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "be_conv_nhwc_batched_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, _P]),
    "be_wino_tile_rows": (C.c_int, []),
    "be_wino_packed_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "be_wino_pack_f32": (C.c_int, [_P] * 6 + [C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "be_wino_workspace_floats": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "be_wino_conv3x3_6x6_f32": (C.c_int, [_P] * 5 + [C.c_int64, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "be_gemm_rows_bf6_packed_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "be_gemm_rows_bf6_pack_f32": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "be_gemm_rows_bf6_f32": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P]),
    "be_conv3x3_pm_bf6_packed_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_conv3x3_pm_bf6_pack_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "be_conv3x3_pm_bf6_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "be_wino_pair_workspace_floats": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "be_wino_conv3x3_pair_6x6_f32": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P,
                                               C.c_size_t, _P]),
    "be_wino_conv3x3_pair_chain_6x6_f32": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int64, C.c_int, C.c_int, C.c_int,
                                                     _P, C.c_size_t, _P, C.c_int, C.c_int]),
    "be_maxpool_wino_in_11x11_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "be_wino_ds_positions": (C.c_int, []),
    "be_wino_ds_packed_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "be_wino_ds_pack_f32": (C.c_int, [_P] * 6 + [C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "be_wino_pair_ds_workspace_floats": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "be_wino_conv3x3_pair_ds_6x6_f32": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int64, C.c_int, C.c_int, C.c_int,
                                                  _P, C.c_size_t, _P, C.c_int, C.c_int]),
    "be_wino_gemms_ext_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "be_conv_fused2_packed_floats": (C.c_size_t, [C.c_int] * 4),
    "be_conv_pack_fused2_f32": (C.c_int, [_P] * 12 + [C.c_float] + [C.c_int] * 4 + [_P, _P, _P]),
    "be_conv_nhwc_fused2_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "be_maxpool_nhwc_f32": (C.c_int, [_P, _P] + [C.c_int] * 7 + [_P]),
    "be_eval_depth_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 4 + [C.c_float] * 3 + [_P, _P]),
    "be_maxpool_nhwc_ld_f32": (C.c_int, [_P, C.c_int, _P] + [C.c_int] * 7 + [_P]),
    "be_nchw_to_nhwc_pad_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int64, C.c_int, _P]),
    "be_upconv2x2_scatter_f32": (C.c_int, [_P, _P, C.c_int64] + [C.c_int] * 9 + [_P]),
    "be_datagen_raster_words": (C.c_size_t, [C.c_int] * 4),
    "be_datagen_raster_u32": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P, _P]),
    "be_datagen_scene_f64": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 4 + [C.c_double] + [_P] * 5),
    "be_datagen_blur_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "be_datagen_blur_composite_f64": (C.c_int, [_P] * 5 + [C.c_int] * 5 + [_P, _P, C.c_size_t, _P]),
    "be_datagen_finish_f64": (C.c_int, [_P] * 4 + [C.c_int] * 3 + [_P, C.c_size_t, _P]),
    "be_datagen_noise_f64": (C.c_int, [_P, _P, C.c_double, C.c_uint32, C.c_int64, C.c_int64, _P, _P, _P]),
    "be_datagen_candidates_f64": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "be_datagen_crop_f64": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64] + [C.c_int] * 4 + [_P, _P]),
    "be_datagen_test_psf_doubles": (C.c_size_t, [C.c_int] * 3),
    "be_datagen_test_render_f64": (C.c_int, [_P] * 8 + [C.c_size_t] + [C.c_int] * 6 + [_P, _P, _P]),
    "be_attention_train_workspace_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_attention_train_fwd_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, _P]),
    "be_attention_bwd_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_attention_bwd_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, _P]),
    "be_attention_dropout_mask_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, _P]),
    "be_attention_train_keep_offset_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_attention_keep_bits_u16": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, _P]),
    "be_dropout_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, C.c_uint32, C.c_uint32, _P]),
    "be_add_layernorm_train_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_uint32,
                                             C.c_uint32, _P]),
    "be_layernorm_bwd_partial_floats": (C.c_size_t, [C.c_int64, C.c_int]),
    "be_layernorm_bwd_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_uint32,
                                       C.c_uint32, _P]),
    "be_nchw3_to_nhwc4_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "be_nchw3_to_nhwc4p_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "be_view_to_nhwc4p_f32": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int, _P]),
    "be_conv7x7_nhwc4p_f32": (C.c_int, [C.POINTER(ConvDesc), _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "be_conv7x7_pool_nhwc4p_f32": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P]),
    "be_conv7x7_pool_bf6_nhwc4p_f32": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P]),
    "be_render_full_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts), C.c_float, C.c_int, _P,
                                     C.POINTER(PatchView), _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "be_fold_records_f32": (C.c_int, [C.POINTER(RenderOpts), _P] + [C.c_int] * 6 + [_P] * 6 + [_P]),
    "be_fold_records_batch_f32": (C.c_int, [C.POINTER(RenderOpts), _P] + [C.c_int] * 7 + [_P] * 6 + [_P]),
    "be_render_full_grid_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts), C.c_float, C.c_int, _P, _P, C.c_int, C.c_int,
                                          _P, _P, C.c_int, C.c_int, _P, _P]),
    "be_fold_records_grid_f32": (C.c_int, [C.POINTER(RenderOpts), _P] + [C.c_int] * 4 + [_P, _P, C.c_int] + [_P] * 6 + [_P]),
    "be_refocus_stack_chunk": (C.c_int, []),
    "be_fold_refocus_stack_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts), _P] + [C.c_int] * 5 + [_P, _P, _P, C.c_int, _P, _P]),
    "be_fold_records_at_f32": (C.c_int, [C.POINTER(RenderOpts), _P] + [C.c_int] * 5 + [_P, _P] + [C.c_int] * 6 + [_P] * 6 + [_P]),
    "be_fold_refocus_stack_at_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts), _P] + [C.c_int] * 5 + [_P, _P] + [C.c_int] * 5
                                     + [_P, C.c_int, _P, _P]),
    "be_fold_records_points_f32": (C.c_int, [C.POINTER(RenderOpts), _P] + [C.c_int] * 5 + [_P, _P, _P, C.c_int64, C.c_int] + [_P] * 6 + [_P]),
    "be_fold_refocus_stack_points_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts), _P] + [C.c_int] * 5
                                         + [_P, _P, _P, C.c_int64, _P, C.c_int, _P, _P]),
    "be_unproject_f32": (C.c_int, [_P] + [C.c_int] * 5 + [C.POINTER(C.c_float)] * 2 + [_P, _P]),
    "be_reproject_f32": (C.c_int, [_P] + [C.c_int] * 5 + [C.POINTER(C.c_float)] * 3 + [C.c_float, C.c_int, C.c_int, _P, C.c_int] + [_P] * 4 + [_P]),
    "be_fuse_scratch_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "be_fuse_views_f32": (C.c_int, [C.c_int, _P, _P, _P, C.c_int] + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_float)] * 3
                          + [C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int] + [_P] * 7 + [_P]),
    "be_tsdf_integrate_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 6 + [C.POINTER(C.c_float)] * 2 + [C.c_float, C.POINTER(C.c_int)]
                              + [C.POINTER(C.c_float)] * 2 + [C.c_float, _P, _P, _P, _P]),
    "be_tsdf_mean_f32": (C.c_int, [C.POINTER(C.c_int), C.c_int] + [_P] * 6 + [_P]),
    "be_tsdf_raycast_f32": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_float)] * 4
                            + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int] + [_P] * 3 + [_P]),
    "be_exclusive_scan_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "be_exclusive_scan_u8_i32": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "be_tsdf_mesh_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "be_tsdf_mesh_count_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_float] + [_P] * 6 + [C.c_size_t, _P]),
    "be_tsdf_mesh_emit_f32": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_float)] * 2 + [C.c_float] + [_P] * 4
                              + [C.c_int64, C.c_int64] + [_P] * 7 + [_P]),
    "be_mesh_raster_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "be_mesh_raster_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, _P, _P] + [C.POINTER(C.c_float)] * 2
                           + [C.c_float, C.c_int, C.c_int, C.c_int] + [_P] * 7 + [_P, C.c_size_t, _P]),
    "be_mesh_components_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "be_mesh_components_i32": (C.c_int, [_P, C.c_int64, C.c_int64] + [_P] * 5 + [C.c_size_t, _P]),
    "be_mesh_components_stats": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, _P, _P]),
    "be_mesh_components_decide": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_float, C.c_int, _P, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "be_mesh_select_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "be_mesh_select_count": (C.c_int, [_P, C.c_int64, C.c_int64] + [_P] * 5 + [C.c_size_t, _P]),
    "be_mesh_select_emit": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int] + [_P] * 7 + [C.c_int64, C.c_int64] + [_P] * 10 + [_P]),
    "be_mesh_cluster_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "be_mesh_cluster_f32": (C.c_int, [_P, _P, C.c_int64] + [C.POINTER(C.c_float)] * 2 + [_P] * 5 + [C.c_size_t, _P]),
    "be_mesh_simplify_sum_rows": (C.c_int, [C.c_int, C.c_int]),
    "be_mesh_simplify_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "be_mesh_simplify_count": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P] + [C.POINTER(C.c_float)] * 2
                               + [_P, C.c_int] + [_P] * 5 + [C.c_size_t, _P]),
    "be_mesh_simplify_emit": (C.c_int, [_P, _P, C.c_int64, C.c_int64] + [C.POINTER(C.c_float)] * 2 + [_P] * 4 + [C.c_int, C.c_int, _P, _P,
                                                                                                              C.c_int64, C.c_int64] + [_P] * 7 + [_P]),
    "be_mesh_smooth_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "be_mesh_adjacency_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "be_mesh_smooth_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int] + [_P] * 5 + [C.c_size_t, _P]),
    "be_mesh_normals_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "be_depth_normals_f32": (C.c_int, [_P] + [C.c_int] * 5 + [C.POINTER(C.c_float), C.c_int, C.c_float, _P, _P]),
    "be_icp_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "be_icp_linearize_f32": (C.c_int, [_P, _P] + [C.c_int] * 5 + [C.POINTER(C.c_float), _P, _P, _P, C.c_int, C.c_int]
                             + [C.POINTER(C.c_float)] * 2 + [C.c_float] * 3 + [_P] * 3 + [_P]),
    "be_fill_nearest_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int] + [_P] * 4 + [_P]),
    "be_fill_diffuse_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "be_fill_diffuse_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int] + [_P] * 5 + [_P]),
    "be_unfold_patches_f32": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "be_local_features_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "be_global_denorm_f32": (C.c_int, [_P, _P, C.c_int64, _P]),
    "be_local_loss_f32": (C.c_int, [C.POINTER(RenderOpts), _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P,
                                    C.c_int64, _P]),
    "be_train_scratch_bytes": (C.c_size_t, []),
    "be_bn_train_fwd_f32": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                      C.c_int, _P, C.c_size_t, _P]),
    "be_bn_train_bwd_f32": (C.c_int, [_P] * 10 + [C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "be_col_sum_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "be_maxpool_nhwc_bwd_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [_P]),
    "be_conv_wgrad_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [_P, C.c_size_t, _P]),
    "be_conv_dgrad_packed_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_conv_pack_dgrad_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "be_linear_small_bwd_f32": (C.c_int, [_P] * 6 + [C.c_int] * 3 + [_P]),
    "be_adam_chunk": (C.c_int, []),
    "be_clip_adamw_f32": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int, C.c_float, C.c_float] + [C.c_double] * 5 + [_P, _P, C.c_int, _P]),
    "be_local_loss_finish_f32": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, _P, _P]),
    "be_train_unit_fwd_f32": (C.c_int, [_P] * 7 + [C.c_float, C.c_float] + [_P] * 7 + [C.c_int, _P, C.c_size_t, _P]),
    "be_train_unit_bwd_f32": (C.c_int, [_P] * 11 + [C.c_int] + [_P] * 8 + [C.c_size_t, _P]),
    "be_train_unit_pair_fwd_f32": (C.c_int, [C.POINTER(TrainUnitFwd), C.POINTER(TrainUnitFwd), C.c_float, C.c_float, _P, C.c_size_t, _P]),
    "be_train_unit_pair_bwd_f32": (C.c_int, [C.POINTER(TrainUnitBwd), C.POINTER(TrainUnitBwd), _P, C.c_size_t, _P]),
    "be_train_sk_plan_debug": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                         C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "be_conv_plan_debug": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_double)]),
    "be_local_stage_layout_debug": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_int]),
    "be_local_stage_route_debug": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "be_linear_param_grads_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "be_linear_small_fwd_f32": (C.c_int, [_P] * 4 + [C.c_int] * 3 + [_P]),
    "be_maxpool_nhwc_fwd_idx_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [_P]),
    "be_maxpool_nhwc_bwd_idx_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [_P]),
    "be_params2dists_f32": (C.c_int, [C.POINTER(RenderOpts), _P, _P, C.c_int64, _P]),
    "be_dists2indicators_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "be_inverse3x3_f32": (C.c_int, [_P, _P, C.c_int64, _P]),
    "be_image_derivative_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "be_fold_patches_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [C.c_int64] * 6 + [C.c_int, _P]),
    "be_params2dists_bwd_f32": (C.c_int, [C.POINTER(RenderOpts), _P, _P, _P, C.c_int64, _P]),
    "be_dists2indicators_bwd_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _P]),
    "be_inverse3x3_bwd_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "be_image_derivative_bwd_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "be_params2etas_bwd_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "be_normalized_gaussian_f32": (C.c_int, [_P, _P, C.c_float, C.c_int64, _P]),
    "be_normalized_gaussian_bwd_f32": (C.c_int, [_P, _P, _P, C.c_float, C.c_int64, _P]),
    "be_etas2depth_bwd_f32": (C.c_int, [C.POINTER(DepthConsts), _P, _P, _P, _P, _P, C.c_int64, _P]),
    "be_depth2sigma_bwd_f32": (C.c_int, [C.POINTER(DepthConsts), _P, C.c_float, _P, _P, C.c_int64, _P]),
    "be_fold_patches_bwd_f32": (C.c_int, [_P, _P] + [C.c_int] * 7 + [C.c_int64] * 6 + [C.c_int, _P]),
    "be_wrap_angles_inplace_f32": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "be_attention_workspace_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "be_attention_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "be_add_layernorm_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "be_add_pe_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "be_global_loss_f32": (C.c_int, [C.POINTER(RenderOpts), C.POINTER(DepthConsts)] + [_P] * 9 + [C.POINTER(C.c_float)]
                           + [_P] * 3 + [C.c_int] * 6 + [_P]),
    "be_profile_enable": (C.c_int, [C.c_int]),
    "be_profile_reset": (C.c_int, []),
    "be_profile_read": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int]),
}
EXPORTED = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load the shared library once; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C blurry-edges_amd/csrc`). There is no CPU fallback for the HIP path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError here = header / library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


TORCH_OPS_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libbe_torch_ops.so")
_ops = None


def ops():
    """torch.ops.be - the C entry points of the LocalStage hot path registered as PyTorch operators (csrc/be_torch_ops.cpp, built
    by build() next to the C-ABI library) - or None when BE_TORCH_OPS=0 asks for the ctypes binding alone.  Both bindings call the
    same C symbols; a missing extension file is an error (build() makes both), not a reason to fall back silently."""
    global _ops
    if _ops is None:
        if os.environ.get("BE_TORCH_OPS", "1") == "0" or _ALT_DIR:
            _ops = False
        else:
            lib()                                      # the C-ABI library first: the extension links against it
            if not os.path.exists(TORCH_OPS_PATH):
                raise RuntimeError(f"{TORCH_OPS_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   f"(or set BE_TORCH_OPS=0 to use the ctypes binding alone)")
            torch.ops.load_library(TORCH_OPS_PATH)
            _ops = torch.ops.be
    return _ops or None


_struct_cache = {}


def struct_tensor(obj) -> torch.Tensor:
    """A host struct of the C ABI (be_render_opts, be_depth_consts) as the CPU uint8 tensor the torch operators take."""
    raw = bytes(obj)
    t = _struct_cache.get(raw)
    if t is None:
        if len(_struct_cache) > 64:
            _struct_cache.clear()
        t = _struct_cache[raw] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    return t


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError(f"{what or 'libblurry_edges_hip'} failed ({rc}): {lib().be_last_error().decode()}")


def dptr(t: torch.Tensor | None, name: str = "tensor", dtypes=(torch.float32, torch.int32)):
    """Device pointer of a contiguous HIP tensor of one of `dtypes` (fp32 unless told otherwise; None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the GPU; the HIP path has no CPU fallback "
                           f"(got {type(t).__name__} on {getattr(t, 'device', '?')})")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{name}: expected {' / '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---------------------------------------------------------------------------------------------- wrappers

def params2etas(p: torch.Tensor) -> torch.Tensor:
    p = p.contiguous()
    o = ops()
    if o is not None:
        return o.params2etas(p)
    out = torch.empty_like(p)
    check(lib().be_params2etas_f32(dptr(p, "params"), dptr(out), p.numel(), stream_ptr(p.device)), "be_params2etas_f32")
    return out


def params2etas_bwd(p: torch.Tensor, geta: torch.Tensor) -> torch.Tensor:
    p, geta = p.contiguous(), geta.contiguous()
    o = ops()
    if o is not None:
        return o.params2etas_bwd(p, geta)
    gp = torch.empty_like(p)
    check(lib().be_params2etas_bwd_f32(dptr(p, "params"), dptr(geta, "geta"), dptr(gp), p.numel(), stream_ptr(p.device)),
          "be_params2etas_bwd_f32")
    return gp


def etas2depth(consts: DepthConsts, eta1: torch.Tensor, eta2: torch.Tensor, want_branch=False):
    eta1, eta2 = torch.broadcast_tensors(eta1, eta2)
    eta1, eta2 = eta1.contiguous(), eta2.contiguous()
    o = ops() if not want_branch else None
    if o is not None:
        return o.etas2depth(struct_tensor(consts), eta1, eta2)
    z = torch.empty_like(eta1)
    br = torch.empty(eta1.shape, dtype=torch.int32, device=eta1.device) if want_branch else None
    check(lib().be_etas2depth_f32(C.byref(consts), dptr(eta1, "eta1"), dptr(eta2, "eta2"), dptr(z), dptr(br),
                                  eta1.numel(), stream_ptr(eta1.device)), "be_etas2depth_f32")
    return (z, br) if want_branch else z


def etas2depth_bwd(consts: DepthConsts, eta1, eta2, gz):
    """eta1, eta2, gz: contiguous, one shape -> (geta1, geta2)."""
    o = ops()
    if o is not None:
        return o.etas2depth_bwd(struct_tensor(consts), eta1, eta2, gz)
    g1, g2 = torch.empty_like(eta1), torch.empty_like(eta1)
    check(lib().be_etas2depth_bwd_f32(C.byref(consts), dptr(eta1, "eta1"), dptr(eta2, "eta2"), dptr(gz, "gdepth"), dptr(g1), dptr(g2),
                                      eta1.numel(), stream_ptr(eta1.device)), "be_etas2depth_bwd_f32")
    return g1, g2


def depth2sigma(consts: DepthConsts, depth: torch.Tensor, rho_prime: float) -> torch.Tensor:
    depth = depth.contiguous()
    o = ops()
    if o is not None:
        return o.depth2sigma(struct_tensor(consts), depth, float(rho_prime))
    out = torch.empty_like(depth)
    check(lib().be_depth2sigma_f32(C.byref(consts), dptr(depth, "depth"), float(rho_prime), dptr(out), depth.numel(),
                                   stream_ptr(depth.device)), "be_depth2sigma_f32")
    return out


def depth2sigma_bwd(consts: DepthConsts, depth, rho_prime, geta):
    o = ops()
    if o is not None:
        return o.depth2sigma_bwd(struct_tensor(consts), depth, float(rho_prime), geta)
    g = torch.empty_like(depth)
    check(lib().be_depth2sigma_bwd_f32(C.byref(consts), dptr(depth, "depth"), float(rho_prime), dptr(geta, "geta"), dptr(g),
                                       depth.numel(), stream_ptr(depth.device)), "be_depth2sigma_bwd_f32")
    return g


# ---- the fine-grained PostProcess methods and their adjoints (flat one-row-per-patch layouts, contiguous float32 on the GPU) ----

def params2dists(opts: RenderOpts, params8):
    """params8 [N,8] -> dists [N,2,21,21]."""
    o = ops()
    if o is not None:
        return o.params2dists(struct_tensor(opts), params8)
    n = params8.shape[0]
    out = torch.empty(n, 2, BE_R, BE_R, dtype=torch.float32, device=params8.device)
    check(lib().be_params2dists_f32(C.byref(opts), dptr(params8, "params"), dptr(out), n, stream_ptr(params8.device)), "be_params2dists_f32")
    return out


def params2dists_bwd(opts: RenderOpts, params8, gdists):
    o = ops()
    if o is not None:
        return o.params2dists_bwd(struct_tensor(opts), params8, gdists)
    g = torch.empty_like(params8)
    check(lib().be_params2dists_bwd_f32(C.byref(opts), dptr(params8, "params"), dptr(gdists, "gdists"), dptr(g), params8.shape[0],
                                        stream_ptr(params8.device)), "be_params2dists_bwd_f32")
    return g


def dists2indicators(dists, etas):
    """dists [N,2,21,21], etas [N,2] -> wedges [N,3,21,21]."""
    o = ops()
    if o is not None:
        return o.dists2indicators(dists, etas)
    n = dists.shape[0]
    out = torch.empty(n, 3, BE_R, BE_R, dtype=torch.float32, device=dists.device)
    check(lib().be_dists2indicators_f32(dptr(dists, "dists"), dptr(etas, "etas"), dptr(out), n, stream_ptr(dists.device)),
          "be_dists2indicators_f32")
    return out


def dists2indicators_bwd(dists, etas, gwedges):
    o = ops()
    if o is not None:
        return o.dists2indicators_bwd(dists, etas, gwedges)
    gd, ge = torch.empty_like(dists), torch.empty_like(etas)
    check(lib().be_dists2indicators_bwd_f32(dptr(dists, "dists"), dptr(etas, "etas"), dptr(gwedges, "gwedges"), dptr(gd), dptr(ge),
                                            dists.shape[0], stream_ptr(dists.device)), "be_dists2indicators_bwd_f32")
    return gd, ge


def inverse3x3(a):
    o = ops()
    if o is not None:
        return o.inverse3x3(a)
    out = torch.empty_like(a)
    check(lib().be_inverse3x3_f32(dptr(a, "A"), dptr(out), a.numel() // 9, stream_ptr(a.device)), "be_inverse3x3_f32")
    return out


def inverse3x3_bwd(inv, gout):
    o = ops()
    if o is not None:
        return o.inverse3x3_bwd(inv, gout)
    ga = torch.empty_like(inv)
    check(lib().be_inverse3x3_bwd_f32(dptr(inv, "inv"), dptr(gout, "gout"), dptr(ga), inv.numel() // 9, stream_ptr(inv.device)),
          "be_inverse3x3_bwd_f32")
    return ga


def image_derivative(img):
    """img [N,C,H,W] -> Sobel magnitude [N,C,H-2,W-2]."""
    o = ops()
    if o is not None:
        return o.image_derivative(img)
    n, c, h, w = img.shape
    out = torch.empty(n, c, h - 2, w - 2, dtype=torch.float32, device=img.device)
    check(lib().be_image_derivative_f32(dptr(img, "img"), dptr(out), n * c, h, w, stream_ptr(img.device)), "be_image_derivative_f32")
    return out


def image_derivative_bwd(img, gout):
    o = ops()
    if o is not None:
        return o.image_derivative_bwd(img, gout)
    n, c, h, w = img.shape
    g = torch.empty_like(img)
    check(lib().be_image_derivative_bwd_f32(dptr(img, "img"), dptr(gout, "gout"), dptr(g), n * c, h, w, stream_ptr(img.device)),
          "be_image_derivative_bwd_f32")
    return g


def normalized_gaussian(x, delta_sq: float):
    o = ops()
    if o is not None:
        return o.normalized_gaussian(x, float(delta_sq))
    y = torch.empty_like(x)
    check(lib().be_normalized_gaussian_f32(dptr(x, "x"), dptr(y), float(delta_sq), x.numel(), stream_ptr(x.device)),
          "be_normalized_gaussian_f32")
    return y


def normalized_gaussian_bwd(x, gy, delta_sq: float):
    o = ops()
    if o is not None:
        return o.normalized_gaussian_bwd(x, gy, float(delta_sq))
    gx = torch.empty_like(x)
    check(lib().be_normalized_gaussian_bwd_f32(dptr(x, "x"), dptr(gy, "gy"), dptr(gx), float(delta_sq), x.numel(), stream_ptr(x.device)),
          "be_normalized_gaussian_bwd_f32")
    return gx


def fold_patches(src, B, C, hp, wp, H, W, stride, mode):
    """nn.Fold of a contiguous [B,C,21,21,Hp,Wp] tensor -> [B,C,H,W]; mode 0 sum, 1 mean over the overlap, 2 number of covering
    patches whose entry is > 0 (src may be int32 then)."""
    o = ops()
    if o is not None:
        return o.fold_patches(src, B, C, hp, wp, H, W, stride, mode)
    p = hp * wp
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=src.device)
    is_int = src.dtype == torch.int32
    check(lib().be_fold_patches_f32(None if is_int else dptr(src, "patches"), dptr(src, "mask") if is_int else None, dptr(out), B, C, hp, wp,
                                    H, W, stride, C * NPIX * p, NPIX * p, BE_R * p, p, wp, 1, mode, stream_ptr(src.device)),
          "be_fold_patches_f32")
    return out


def fold_patches_bwd(gout, hp, wp, stride, mode):
    """gout [B,C,H,W] -> the cotangent of fold_patches' source, [B,C,21,21,Hp,Wp]."""
    o = ops()
    if o is not None:
        return o.fold_patches_bwd(gout, hp, wp, stride, mode)
    B, Cc, H, W = gout.shape
    p = hp * wp
    g = torch.empty(B, Cc, BE_R, BE_R, hp, wp, dtype=torch.float32, device=gout.device)
    check(lib().be_fold_patches_bwd_f32(dptr(gout, "gout"), dptr(g), B, Cc, hp, wp, H, W, stride, Cc * NPIX * p, NPIX * p, BE_R * p, p, wp, 1,
                                        mode, stream_ptr(gout.device)), "be_fold_patches_bwd_f32")
    return g


def wrap_angles_(est, col0=4, col1=8):
    """est[:, col0:col1] <- remainder(., 2 pi) in place (est [N,ld] contiguous)."""
    o = ops()
    if o is not None:
        o.wrap_angles_(est, col0, col1)
        return est
    check(lib().be_wrap_angles_inplace_f32(dptr(est, "est"), est.shape[0], est.shape[1], col0, col1, stream_ptr(est.device)),
          "be_wrap_angles_inplace_f32")
    return est


def local_depth(consts: DepthConsts, params10: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """params10 [2P,10] image-major -> depth [P,2]."""
    if params10.dim() != 2 or params10.shape[1] != 10 or params10.shape[0] % 2:
        raise RuntimeError(f"local_depth: params10 must be [2P,10], got {tuple(params10.shape)}")
    p = params10.shape[0] // 2
    o = ops()
    if o is not None:
        return o.local_depth(struct_tensor(consts), params10.contiguous(), out)
    if out is None:
        out = torch.empty(p, 2, dtype=torch.float32, device=params10.device)
    check(lib().be_local_depth_f32(C.byref(consts), dptr(params10, "params10"), dptr(out), p,
                                   stream_ptr(params10.device)), "be_local_depth_f32")
    return out


def render_colors(opts: RenderOpts, params10: torch.Tensor, patches: torch.Tensor, *, colors=None, want=()):
    """params10 [N,10], patches [N,3,21,21] -> colors [N,3,3] and the optional outputs named in `want`
    (any of 'recon','boundary','dists','wedges','gram','aty').  Returns (colors, dict)."""
    n = params10.shape[0]
    if tuple(params10.shape) != (n, 10) or tuple(patches.shape) != (n, 3, BE_R, BE_R):
        raise RuntimeError(f"render_colors: bad shapes {tuple(params10.shape)} / {tuple(patches.shape)}")
    dev = params10.device
    o = ops() if not want else None
    if o is not None:                                   # colours only: the registered operator
        return o.render_colors(struct_tensor(opts), params10.contiguous(), patches.contiguous(), colors), {}
    if colors is None:
        colors = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    shapes = dict(recon=(n, 3, BE_R, BE_R), boundary=(n, BE_R, BE_R), dists=(n, 2, BE_R, BE_R),
                  wedges=(n, 3, BE_R, BE_R), gram=(n, 3, 3), aty=(n, 3, 3))
    extra = {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in want}
    g = lambda k: dptr(extra.get(k))
    check(lib().be_render_colors_f32(C.byref(opts), dptr(params10, "params10"), dptr(patches, "patches"), dptr(colors),
                                     g("recon"), g("boundary"), g("dists"), g("wedges"), g("gram"), g("aty"), n,
                                     stream_ptr(dev)), "be_render_colors_f32")
    return colors, extra


def render_colors_view(opts: RenderOpts, params10: torch.Tensor, view, patches_per_image: int, *, want=()):
    """render_colors with the pixels gathered through a PatchView: params10 [A*P,10] aperture-major (the order of
    img_patches.flatten(0,1), blurry_edges_test.py:120-123) -> (colors [A*P,3,3], extras)."""
    n = params10.shape[0]
    if tuple(params10.shape) != (n, 10) or n % patches_per_image:
        raise RuntimeError(f"render_colors_view: bad shapes {tuple(params10.shape)} / P={patches_per_image}")
    dev = params10.device
    colors = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    shapes = dict(recon=(n, 3, BE_R, BE_R), boundary=(n, BE_R, BE_R), dists=(n, 2, BE_R, BE_R),
                  wedges=(n, 3, BE_R, BE_R), gram=(n, 3, 3), aty=(n, 3, 3))
    extra = {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in want}
    g = lambda k: dptr(extra.get(k))
    check(lib().be_render_colors_view_f32(C.byref(opts), dptr(params10, "params10"), C.byref(view), patches_per_image,
                                          dptr(colors), g("recon"), g("boundary"), g("dists"), g("wedges"), g("gram"),
                                          g("aty"), n, stream_ptr(dev)), "be_render_colors_view_f32")
    return colors, extra


def conv_pack(weight, bias, bn=None, eps=1e-5, chw_hw=0):
    """weight [Cout,Cin,k,k] (or [Cout,Cin] for a Linear), optional bn=(gamma,beta,mean,var) -> (pw, pb)."""
    cout, cin = weight.shape[0], weight.shape[1]
    ks = weight.shape[2] if weight.dim() == 4 else 1
    nfl = lib().be_conv_packed_floats(cout, cin, ks)
    if nfl == 0:
        raise RuntimeError(f"conv_pack: unsupported conv shape cout={cout} cin={cin} k={ks}")
    dev = weight.device
    pw = torch.empty(nfl, dtype=torch.float32, device=dev)
    pb = torch.empty((cout + 31) // 32 * 32, dtype=torch.float32, device=dev)
    g = bn if bn is not None else (None, None, None, None)
    check(lib().be_conv_pack_f32(dptr(weight.contiguous(), "weight"), dptr(bias), dptr(g[0]), dptr(g[1]), dptr(g[2]),
                                 dptr(g[3]), eps, cout, cin, ks, chw_hw, dptr(pw), dptr(pb), stream_ptr(dev)),
          "be_conv_pack_f32")
    return pw, pb


def _residual_ptr(residual, rows, cout, ld):
    """The kernels read the residual with y's row stride (residual[m * ld + c], every route): a dense [.., ld] tensor of `rows`
    rows, or its [.., :cout] view.  Anything else - a contiguous [N,H,W,cout] residual beside a wider out - would be read at the
    wrong stride and past its end, so it is refused here, on shapes alone, before any pointer is taken or kernel launched."""
    if residual is None:
        return None
    if not isinstance(residual, torch.Tensor) or residual.dim() < 2:
        raise RuntimeError("conv_nhwc: residual: expected a tensor of at least two dimensions")
    c = residual.shape[-1]
    want, run = [], ld                                     # the strides of a dense [.., ld] tensor under this shape
    for size in reversed(residual.shape[:-1]):
        want.append(run)
        run *= size
    dense = residual.stride(-1) == 1 and all(s == w_ or size == 1 for s, w_, size in
                                             zip(reversed(residual.stride()[:-1]), want, reversed(residual.shape[:-1])))
    if c not in (cout, ld) or not dense or residual.numel() != rows * c:
        raise RuntimeError(f"conv_nhwc: the residual is read with y's row stride ({ld} floats, {rows} rows of {cout} channels): got "
                           f"shape {tuple(residual.shape)} with strides {tuple(residual.stride())}")
    return dptr(residual if c == ld else residual.as_strided((rows, ld), (ld, 1)), "residual")


def conv_nhwc(x, pw, pb, cout, ksize, act, residual=None, out=None, scratch=None):
    """x [N,H,W,Cin] NHWC -> [N,H,W,cout]; out = a [N,H,W,ld] tensor whose first cout channels receive the result (the other
    columns are left as they are); residual = a tensor with out's row stride: [N,H,W,ld], or its [..., :cout] view - with no out,
    [N,H,W,cout]; scratch = a float32 buffer the library may use to split the K loop of small launches (training)."""
    n, h, w, cin = x.shape
    y = torch.empty(n, h, w, cout, dtype=torch.float32, device=x.device) if out is None else out
    res = _residual_ptr(residual, n * h * w, cout, y.shape[-1])
    d = ConvDesc(n, h, w, cin, cout, ksize, int(act))
    if scratch is not None:
        check(lib().be_conv_nhwc_splitk_f32(C.byref(d), dptr(x, "x"), dptr(pw), dptr(pb), res, dptr(y), y.shape[-1],
                                            dptr(scratch), scratch.numel() * 4, stream_ptr(x.device)), "be_conv_nhwc_splitk_f32")
        return y
    check(lib().be_conv_nhwc_f32(C.byref(d), dptr(x, "x"), dptr(pw), dptr(pb), res, dptr(y), y.shape[-1],
                                 stream_ptr(x.device)), "be_conv_nhwc_f32")
    return y


def maxpool_nhwc(x, k, stride, pad, channels=None):
    """x [N,H,W,ld]; pools its first `channels` channels (default: all)."""
    n, h, w, ld = x.shape
    c = ld if channels is None else channels
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.empty(n, oh, ow, c, dtype=torch.float32, device=x.device)
    check(lib().be_maxpool_nhwc_ld_f32(dptr(x, "x"), ld, dptr(y), n, h, w, c, k, stride, pad, stream_ptr(x.device)),
          "be_maxpool_nhwc_f32")
    return y


def eval_depth(pred, gt, mask_src, crop=0, tau_n=1.25, z_min=0.75, z_max=1.18):
    """pred, gt, mask_src [B,H,W] float32 on the GPU -> float64 tensor [5] (delta1-3, RMSE cm, AbsRel cm) on the GPU."""
    b, h, w = pred.shape
    out = torch.empty(5, dtype=torch.float64, device=pred.device)
    check(lib().be_eval_depth_f32(dptr(pred, "pred"), dptr(gt, "gt"), dptr(mask_src, "mask"), b, h, w, int(crop), float(tau_n),
                                  float(z_min), float(z_max), C.c_void_p(out.data_ptr()), stream_ptr(pred.device)),
          "be_eval_depth_f32")
    return out


def nchw_to_nhwc_pad(x, cpad):
    """x [N,C,H,W] -> [N,H,W,cpad] with zero channels C..cpad-1."""
    n, c, h, w = x.shape
    y = torch.empty(n, h, w, cpad, dtype=torch.float32, device=x.device)
    check(lib().be_nchw_to_nhwc_pad_f32(dptr(x, "x"), dptr(y), n, c, h * w, cpad, stream_ptr(x.device)), "be_nchw_to_nhwc_pad_f32")
    return y


def upconv2x2_scatter(t, out, cout, ch_off):
    """t [N,h,w,4*cout] -> channels [ch_off, ch_off+cout) of out [N,oh,ow,ld], centred as F.pad(diff//2) does."""
    n, h, w, _ = t.shape
    _, oh, ow, ld = out.shape
    check(lib().be_upconv2x2_scatter_f32(dptr(t, "t"), dptr(out, "out"), n, h, w, cout, oh, ow, (oh - 2 * h) // 2,
                                         (ow - 2 * w) // 2, ld, ch_off, stream_ptr(t.device)), "be_upconv2x2_scatter_f32")
    return out


def nchw3_to_nhwc4(x):
    n, c, h, w = x.shape
    if c != 3:
        raise RuntimeError("nchw3_to_nhwc4: expected 3 channels")
    y = torch.empty(n, h, w, 4, dtype=torch.float32, device=x.device)
    check(lib().be_nchw3_to_nhwc4_f32(dptr(x, "x"), dptr(y), n, h * w, stream_ptr(x.device)), "be_nchw3_to_nhwc4_f32")
    return y


def patches_to_nhwc4(x):
    """x: logical [N,3,h,w] patches -> the NHWC4 staging [N,h,w,4] conv1 reads.  A contiguous NCHW tensor takes
    be_nchw3_to_nhwc4_f32; a PERMUTED VIEW of a channels-last tensor - what `img.permute(0,3,1,2)` makes of the dataset's
    [N,h,w,3] batches (local_training.py:103) - is read in place through a patch view (be_view_to_nhwc4_f32): no NCHW copy first."""
    n, c, h, w = x.shape
    if c == 3 and (h, w) == (BE_R, BE_R) and x.dtype == torch.float32 and n > 0 and x.stride() == (h * w * 3, 1, w * 3, 3):
        dptr(x.permute(0, 2, 3, 1), "x")                     # contiguous [N,h,w,3] on the GPU, else this raises
        view = PatchView(x.data_ptr(), 0, 1, w * 3, 3, 0, h * w * 3, n)
        y = torch.empty(n, h, w, 4, dtype=torch.float32, device=x.device)
        check(lib().be_view_to_nhwc4_f32(C.byref(view), n, 0, dptr(y), n, stream_ptr(x.device)), "be_view_to_nhwc4_f32")
        return y
    return nchw3_to_nhwc4(x.to(torch.float32).contiguous())


def nchw3_to_nhwc4p(x, wrow=28):
    """[N,3,h,w] -> [N,h,wrow,4]: image column c at padded column c + 3, zeros elsewhere (staging of conv1 for large batches)."""
    n, c, h, w = x.shape
    if c != 3:
        raise RuntimeError("nchw3_to_nhwc4p: expected 3 channels")
    y = torch.empty(n, h, wrow, 4, dtype=torch.float32, device=x.device)
    check(lib().be_nchw3_to_nhwc4p_f32(dptr(x, "x"), dptr(y), n, h, w, wrow, stream_ptr(x.device)), "be_nchw3_to_nhwc4p_f32")
    return y


def conv7x7_nhwc4p(xp, w_img, pw, pb, cout, act):
    """conv1 on the padded staging xp [N,h,wrow,4] (image width w_img) -> [N,h,w_img,cout]."""
    n, h, wrow, c4 = xp.shape
    y = torch.empty(n, h, w_img, cout, dtype=torch.float32, device=xp.device)
    d = ConvDesc(n, h, w_img, 4, cout, 7, int(act))
    check(lib().be_conv7x7_nhwc4p_f32(C.byref(d), dptr(xp, "x"), wrow, dptr(pw), dptr(pb), dptr(y), cout, stream_ptr(xp.device)),
          "be_conv7x7_nhwc4p_f32")
    return y


def conv7x7_pool_nhwc4p(xp, pw, pb):
    """conv1 + Smish + MaxPool2d(3, 2, 1) in one launch on the padded staging xp [N,21,28,4] -> [N,11,11,64]."""
    n, h, wrow, c4 = xp.shape
    if (h, wrow, c4) != (21, 28, 4):
        raise RuntimeError(f"conv7x7_pool_nhwc4p: expected [N,21,28,4], got {tuple(xp.shape)}")
    y = torch.empty(n, 11, 11, 64, dtype=torch.float32, device=xp.device)
    check(lib().be_conv7x7_pool_nhwc4p_f32(dptr(xp, "x"), n, dptr(pw), dptr(pb), dptr(y), stream_ptr(xp.device)),
          "be_conv7x7_pool_nhwc4p_f32")
    return y


def conv7x7_pool_bf6_nhwc4p(xp, pw, pb):
    """conv7x7_pool_nhwc4p in split-bf16 arithmetic (k_conv1_pool_bf6): same operands, [N,21,28,4] -> [N,11,11,64]."""
    n, h, wrow, c4 = xp.shape
    if (h, wrow, c4) != (21, 28, 4):
        raise RuntimeError(f"conv7x7_pool_bf6_nhwc4p: expected [N,21,28,4], got {tuple(xp.shape)}")
    y = torch.empty(n, 11, 11, 64, dtype=torch.float32, device=xp.device)
    check(lib().be_conv7x7_pool_bf6_nhwc4p_f32(dptr(xp, "x"), n, dptr(pw), dptr(pb), dptr(y), stream_ptr(xp.device)),
          "be_conv7x7_pool_bf6_nhwc4p_f32")
    return y


def local_stage_pack(tensors, eps=1e-5):
    """tensors: the 86 fp32 state-dict tensors on the GPU, in the order documented in the header."""
    if len(tensors) != NTENSORS:
        raise RuntimeError(f"local_stage_pack: expected {NTENSORS} tensors, got {len(tensors)}")
    o = ops()
    if o is not None:
        return o.local_stage_pack(list(tensors), float(eps))
    keep = [t.contiguous() for t in tensors]
    arr = (_P * NTENSORS)(*[dptr(t, f"tensor[{i}]") for i, t in enumerate(keep)])
    dev = keep[0].device
    packed = torch.empty(lib().be_local_stage_packed_floats(), dtype=torch.float32, device=dev)
    check(lib().be_local_stage_pack_f32(arr, eps, dptr(packed), stream_ptr(dev)), "be_local_stage_pack_f32")
    return packed


class LocalStageOpts(C.Structure):
    """be_local_stage_opts: per-call options of the LocalStage forward (no process-wide state in the library)."""
    _fields_ = [("winograd", C.c_int), ("chunk", C.c_int)]


def local_stage_forward(packed, x, out=None, workspace=None, winograd=True, chunk=0):
    n = x.shape[0]
    if tuple(x.shape[1:]) != (3, BE_R, BE_R):
        raise RuntimeError(f"LocalStage input must be [N,3,21,21], got {tuple(x.shape)}")
    dev = x.device
    o = ops()
    if o is not None:
        return o.local_stage_forward(packed, x, out, workspace, bool(winograd), int(chunk))
    if out is None:
        out = torch.empty(n, 10, dtype=torch.float32, device=dev)
    need = lib().be_local_stage_workspace_bytes(n, int(chunk))
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    opts = LocalStageOpts(int(bool(winograd)), int(chunk))
    check(lib().be_local_stage_forward_f32(dptr(packed, "packed"), dptr(x, "x"), dptr(out), n, dptr(workspace),
                                           workspace.numel() * 4, C.byref(opts), stream_ptr(dev)), "be_local_stage_forward_f32")
    return out, workspace


def wino_pack(weight, bias, bn=None, eps=1e-5):
    """weight [Cout,Cin,3,3] (+ bias, + eval BatchNorm) -> (U [25*cout_pad*cin], bias [cout_pad]) for wino_conv3x3."""
    cout, cin = weight.shape[0], weight.shape[1]
    nfl = lib().be_wino_packed_floats(cout, cin)
    if nfl == 0 or tuple(weight.shape[2:]) != (3, 3):
        raise RuntimeError(f"wino_pack: unsupported conv shape {tuple(weight.shape)}")
    dev = weight.device
    pw = torch.empty(nfl, dtype=torch.float32, device=dev)
    pb = torch.empty((cout + 31) // 32 * 32, dtype=torch.float32, device=dev)
    g = bn if bn is not None else (None, None, None, None)
    check(lib().be_wino_pack_f32(dptr(weight.contiguous(), "weight"), dptr(bias), dptr(g[0]), dptr(g[1]), dptr(g[2]), dptr(g[3]), eps,
                                 cout, cin, dptr(pw), dptr(pb), stream_ptr(dev)), "be_wino_pack_f32")
    return pw, pb


def gemm_rows_bf6_pack(pw, cout, cin):
    """pw: a packed fp32 matrix [cout_pad32][cin] (conv_pack of a 1x1 convolution / linear) -> its hi / mid / lo bf16 planes (as float32 storage)."""
    nfl = lib().be_gemm_rows_bf6_packed_floats(cout, cin)
    if nfl == 0:
        raise RuntimeError(f"gemm_rows_bf6_pack: unsupported shape cout={cout} cin={cin}")
    planes = torch.empty(nfl, dtype=torch.float32, device=pw.device)
    check(lib().be_gemm_rows_bf6_pack_f32(dptr(pw, "pw"), cout, cin, dptr(planes), stream_ptr(pw.device)), "be_gemm_rows_bf6_pack_f32")
    return planes


def gemm_rows_bf6(x, planes, n, bias=None, residual=None, act=0, out=None):
    """x [M,K] -> act(x w^T + bias (+ residual)) [M,n] in split-bf16 arithmetic; out = an [M,ld] tensor whose first n columns receive it."""
    m, k = x.shape
    y = torch.empty(m, n, dtype=torch.float32, device=x.device) if out is None else out
    check(lib().be_gemm_rows_bf6_f32(dptr(x, "x"), m, k, dptr(planes), n, dptr(bias), dptr(residual), int(act), dptr(y), y.shape[-1],
                                     stream_ptr(x.device)), "be_gemm_rows_bf6_f32")
    return y


def conv3x3_pm_bf6_pack(pw, cout, cin, cin2=0):
    """pw: the packed fp32 matrix [96][9 cin + cin2] of a 3x3 convolution (conv_pack) or of a 3x3 + 1x1 pair (conv_pack_fused2)
    -> its hi / mid / lo bf16 planes (as float32 storage) for conv3x3_pm_bf6."""
    nfl = lib().be_conv3x3_pm_bf6_packed_floats(cout, cin, cin2)
    if nfl == 0:
        raise RuntimeError(f"conv3x3_pm_bf6_pack: unsupported shape cout={cout} cin={cin} cin2={cin2}")
    planes = torch.empty(nfl, dtype=torch.float32, device=pw.device)
    check(lib().be_conv3x3_pm_bf6_pack_f32(dptr(pw, "pw"), cout, cin, cin2, dptr(planes), stream_ptr(pw.device)),
          "be_conv3x3_pm_bf6_pack_f32")
    return planes


def conv3x3_pm_bf6(x, planes, pb, cout, act=0, x2=None, out=None):
    """x [N,H,W,Cin] NHWC -> act(conv3x3(x) (+ conv1x1(x2)) + bias) [N,H,W,cout] in split-bf16 arithmetic; out = an [N,H,W,ld]
    tensor whose first cout channels receive it."""
    n, h, w, cin = x.shape
    y = torch.empty(n, h, w, cout, dtype=torch.float32, device=x.device) if out is None else out
    d = ConvDesc(n, h, w, cin, cout, 3, int(act))
    check(lib().be_conv3x3_pm_bf6_f32(C.byref(d), dptr(x, "x"), dptr(x2), 0 if x2 is None else x2.shape[-1], dptr(planes), dptr(pb),
                                      dptr(y), y.shape[-1], stream_ptr(x.device)), "be_conv3x3_pm_bf6_f32")
    return y


def wino_conv3x3(x, pw, pb, cout, act=0, residual=None, workspace=None):
    """x [N,6,6,Cin] NHWC -> [N,6,6,cout] by Winograd F(3x3,3x3)."""
    n, h, w, cin = x.shape
    if (h, w) != (6, 6):
        raise RuntimeError(f"wino_conv3x3: 6x6 maps only, got {h}x{w}")
    need = lib().be_wino_workspace_floats(n, cin, cout)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)
    y = torch.empty(n, 6, 6, cout, dtype=torch.float32, device=x.device)
    check(lib().be_wino_conv3x3_6x6_f32(dptr(x, "x"), dptr(pw), dptr(pb), dptr(residual), dptr(y), n, cin, cout, int(act),
                                        dptr(workspace), workspace.numel(), stream_ptr(x.device)), "be_wino_conv3x3_6x6_f32")
    return y, workspace


def wino_conv3x3_pair(x, pw1, pb1, cmid, pw2, pb2, cout, act1=1, act2=1, residual=None, workspace=None):
    """conv3x3 -> act1 -> conv3x3 (+ residual) -> act2 on 6x6 maps, intermediate map never written."""
    n_, h, w, cin = x.shape
    need = lib().be_wino_pair_workspace_floats(n_, cin, cmid, cout)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)
    y = torch.empty(n_, 6, 6, cout, dtype=torch.float32, device=x.device)
    check(lib().be_wino_conv3x3_pair_6x6_f32(dptr(x, "x"), dptr(pw1), dptr(pb1), int(act1), dptr(pw2), dptr(pb2), dptr(residual),
                                             int(act2), dptr(y), n_, cin, cmid, cout, dptr(workspace), workspace.numel(),
                                             stream_ptr(x.device)), "be_wino_conv3x3_pair_6x6_f32")
    return y, workspace


def wino_conv3x3_pair_chain(x, pw1, pb1, cmid, pw2, pb2, cout, workspace, act1=1, act2=1, residual=None, x_in_v=False, next_cmid=0):
    """wino_conv3x3_pair as a link of a chain of blocks that share `workspace` (at least be_wino_pair_workspace_floats of every link).
    x_in_v: the start of the workspace already holds x's input transform (left by the link in front or by maxpool_wino_in);
    next_cmid > 0: y's input transform for a following block whose conv1 has next_cmid outputs is left there.  Same bits as unchained."""
    n_, h, w, cin = x.shape
    y = torch.empty(n_, 6, 6, cout, dtype=torch.float32, device=x.device)
    check(lib().be_wino_conv3x3_pair_chain_6x6_f32(dptr(x, "x"), dptr(pw1), dptr(pb1), int(act1), dptr(pw2), dptr(pb2), dptr(residual),
                                                   int(act2), dptr(y), n_, cin, cmid, cout, dptr(workspace), workspace.numel(),
                                                   stream_ptr(x.device), int(bool(x_in_v)), int(next_cmid)),
          "be_wino_conv3x3_pair_chain_6x6_f32")
    return y


def wino_ds_pack(weight, bias=None, bn=None, eps=1e-5, with_bias=True):
    """A block's 1x1 downsample weight [Cout,Cin] (or [Cout,Cin,1,1]; + bias, + eval BatchNorm) in the form conv2's Winograd GEMMs take
    as their second K segment -> (packed_ds: U_ds [positions', cout_pad, cin] fp32, then its bf16 planes; folded bias [cout_pad])."""
    cout, cin = weight.shape[0], weight.shape[1]
    nfl = lib().be_wino_ds_packed_floats(cout, cin)
    if nfl == 0 or weight.numel() != cout * cin:
        raise RuntimeError(f"wino_ds_pack: unsupported shape {tuple(weight.shape)}")
    dev = weight.device
    pd = torch.empty(nfl, dtype=torch.float32, device=dev)
    pb = torch.zeros((cout + 31) // 32 * 32, dtype=torch.float32, device=dev) if with_bias else None
    g = bn if bn is not None else (None, None, None, None)
    check(lib().be_wino_ds_pack_f32(dptr(weight.contiguous(), "weight"), dptr(bias), dptr(g[0]), dptr(g[1]), dptr(g[2]), dptr(g[3]), eps,
                                    cout, cin, dptr(pd), dptr(pb), stream_ptr(dev)), "be_wino_ds_pack_f32")
    return pd, pb


def wino_conv3x3_pair_ds(x, pw1, pb1, cmid, pw2, pb2, pds, cout, act1=1, act2=1, workspace=None, x_in_v=False, next_cmid=0, cin=None,
                         n=None, store_y=True):
    """wino_conv3x3_pair_chain with the block's 1x1 downsample (pds: wino_ds_pack; its bias already in pb2) inside conv2's GEMMs instead
    of a residual tensor.  x may be None with x_in_v (pass cin and n), and store_y=False with next_cmid leaves y unwritten (None).
    -> (y, workspace)"""
    if x is not None:
        n, _, _, cin = x.shape
    dev = pw1.device
    need = lib().be_wino_pair_ds_workspace_floats(n, cin, cmid, cout)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=dev)
    y = torch.empty(n, 6, 6, cout, dtype=torch.float32, device=dev) if store_y else None
    check(lib().be_wino_conv3x3_pair_ds_6x6_f32(dptr(x), dptr(pw1), dptr(pb1), int(act1), dptr(pw2), dptr(pb2), dptr(pds), int(act2),
                                                dptr(y), n, cin, cmid, cout, dptr(workspace), workspace.numel(), stream_ptr(dev),
                                                int(bool(x_in_v)), int(next_cmid)), "be_wino_conv3x3_pair_ds_6x6_f32")
    return y, workspace


def wino_gemms_ext(v, pw, n, cin, cout, vx=None, pds=None, cin_ext=0, tile_major=False):
    """The transform-domain GEMMs of one Winograd layer alone: v [positions, tiles, cin] (tile_major: [tiles, positions, cin]) ->
    M likewise with cout channels; with vx / pds (wino_ds_pack) the second K segment over vx at pds's positions."""
    npos = 5 * (lib().be_wino_tile_rows() + 2)
    tiles = 12 // lib().be_wino_tile_rows() * n
    m = torch.empty((tiles, npos, cout) if tile_major else (npos, tiles, cout), dtype=torch.float32, device=v.device)
    check(lib().be_wino_gemms_ext_f32(dptr(v, "v"), dptr(pw), dptr(m), n, cin, cout, dptr(vx), dptr(pds), int(cin_ext), int(bool(tile_major)),
                                      stream_ptr(v.device)), "be_wino_gemms_ext_f32")
    return m


def maxpool_wino_in(x, next_cmid, workspace):
    """x [N,11,11,C] NHWC -> its 3/2/1 max-pool [N,6,6,C] (maxpool_nhwc's bits); the pooled map's Winograd input transform for a block
    whose conv1 has next_cmid outputs is left at the start of `workspace` (head of a wino_conv3x3_pair_chain)."""
    n_, h, w, c = x.shape
    if (h, w) != (11, 11):
        raise RuntimeError(f"maxpool_wino_in: 11x11 maps only, got {h}x{w}")
    y = torch.empty(n_, 6, 6, c, dtype=torch.float32, device=x.device)
    check(lib().be_maxpool_wino_in_11x11_f32(dptr(x, "x"), dptr(y), n_, c, int(next_cmid), dptr(workspace), workspace.numel(),
                                             stream_ptr(x.device)), "be_maxpool_wino_in_11x11_f32")
    return y


def local_stage_forward_view(packed, view, patches_per_image: int, n: int, device, out=None, workspace=None, winograd=True,
                             chunk=0):
    """LocalStage eval forward over the n = A*P patches of a PatchView (no unfolded copy) -> [n,10]."""
    if out is None:
        out = torch.empty(n, 10, dtype=torch.float32, device=device)
    need = lib().be_local_stage_workspace_bytes(n, int(chunk))
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    opts = LocalStageOpts(int(bool(winograd)), int(chunk))
    check(lib().be_local_stage_forward_view_f32(dptr(packed, "packed"), C.byref(view), patches_per_image, dptr(out), n,
                                                dptr(workspace), workspace.numel() * 4, C.byref(opts), stream_ptr(device)),
          "be_local_stage_forward_view_f32")
    return out, workspace


LOCAL_STAGE_FORMS = ("f32", "fused2", "wino", "ds_f32", "rows_bf6", "l0_bf6", "wino_ds", "zero")
LOCAL_STAGE_ROUTE_FIELDS = ("staging", "conv1", "conv1_pools", "l0_bf6", "chain", "blocks6", "store_maps", "fc1_bf6")


def local_stage_layout():
    """The packed LocalStage buffer's regions in buffer order (be_local_stage_layout_debug; no GPU): dicts of layer (-1: none), form
    (LOCAL_STAGE_FORMS), w_off / w_floats / b_off / b_floats, and reads = the index of the region its pack call reads, or None."""
    a, o = (C.c_int * 96)(), (C.c_int64 * 128)()
    n = lib().be_local_stage_layout_debug(a, o, 32)
    if n < 0:
        check(n, "be_local_stage_layout_debug")
    return [dict(layer=a[3 * k], form=LOCAL_STAGE_FORMS[a[3 * k + 1]], w_off=o[4 * k], w_floats=o[4 * k + 1], b_off=o[4 * k + 2],
                 b_floats=o[4 * k + 3], reads=a[3 * k + 2] if a[3 * k + 2] >= 0 else None) for k in range(n)]


def local_stage_route(winograd, nb):
    """The kernels a sub-batch of nb patches takes (be_local_stage_route_debug; no GPU) -> {LOCAL_STAGE_ROUTE_FIELDS: int}."""
    out = (C.c_int * 8)()
    n = lib().be_local_stage_route_debug(int(bool(winograd)), int(nb), out)
    if n < 0:
        check(n, "be_local_stage_route_debug")
    return dict(zip(LOCAL_STAGE_ROUTE_FIELDS, list(out)[:n]))


KERNEL_NAMES = {0: "k_conv_igemm<2,2,2,2,TAPS> (128x128)", 1: "k_conv_igemm<4,1,1,3,TAPS> (128x96)",
                2: "k_conv_igemm<4,1,1,2,TAPS> (128x64)", 3: "k_conv_igemm<4,1,1,1,TAPS> (128x32)",
                4: "k_conv_igemm<4,1,1,2,ROW8> (conv1)", 5: "k_conv_igemm small-M tiles (64x64 / 128x32)",
                6: "k_wino_gemm_ps<0, 0> (128x128 tiles, the Winograd transform-domain GEMMs of a layer - one per position: 40 for the 8x5 tiles - per launch, in split-bf16 arithmetic: six v_mfma_f32_32x32x16_bf16 per product, FLOPs counted as fp32 products; in LocalStage conv2's launches carry the block's 1x1 downsample as a second K segment at 18 of the 40 positions, k_wino_gemm_ps<0, 0, 1>, unless BE_WINO_DS_GEMM=1; BE_WINO_F32=1: the fp32 k_wino_gemm_ws / k_wino_gemm / batched k_conv_igemm)",
                7: "row GEMMs: k_wino_gemm_ps<EPI> on pre-split weights (split-bf16 arithmetic, FLOPs counted as fp32 products: fc.1, and LocalStage's 1x1 downsamples under BE_WINO_DS_GEMM=1; BE_ROWS_F32=1 / BE_WINO_F32=1: fp32) and the fp32 k_wino_gemm<1> / k_wino_gemm_ws<.., 1> (1x1 convolutions / linears of large batches)",
                8: "k_wino_in / k_wino_out_in / k_wino_out / k_wino_out_pool2 / k_wino_out_res_in / k_pool_wino_in (Winograd transforms; the chained LocalStage runs k_pool_wino_in - the 3/2/1 max-pool with layer1's input transform - three k_wino_out_in, two k_wino_out_res_in and k_wino_out_pool2; BE_WINO_NO_CHAIN=1: k_maxpool_nhwc and a k_wino_in and k_wino_out per block)",
                9: "k_maxpool_nhwc",
                10: "k_render_colors (pass A)", 11: "conv1 input staging",
                12: "k_unit_gemms / k_unit_gemms_sk (training units: weight-gradient GEMMs + data-gradient convolutions of one or two units in one launch; a residual block's two forward convolutions)",
                13: "k_conv1_pool_bf6 (conv1 7x7 + Smish + max-pool 3/2/1 in one image-major kernel, in split-bf16 arithmetic with the image pre-split in LDS, FLOPs counted as fp32 products; BE_C1_F32=1 / BE_WINO_F32=1: the fp32 k_conv1_pool)"}
HBM_KERNEL_IDS = (8, 9, 10, 11)


def profile_enable(max_launches: int):
    check(lib().be_profile_enable(int(max_launches)), "be_profile_enable")


def profile_reset():
    lib().be_profile_reset()


def profile_read(cap: int):
    """-> list of (kernel_id, flops, bytes, ms, flops_executed) in launch order (waits for the events)."""
    ids = (C.c_int * cap)(); fl = (C.c_double * cap)(); by = (C.c_double * cap)(); ms = (C.c_float * cap)()
    fx = (C.c_double * cap)()
    n = lib().be_profile_read(ids, fl, by, fx, ms, cap)
    if n < 0:
        check(n, "be_profile_read")
    return [(ids[i], fl[i], by[i], ms[i], fx[i]) for i in range(n)]


# ---------------------------------------------------------------------------------------------- pass B / tiling

def view_image_pair(img: torch.Tensor, stride: int = 2, window=None) -> PatchView:
    """img [2,3,H,W] -> gather-on-read view of its (H-21)/stride+1 x (W-21)/stride+1 patch grid; window =
    (top, left, height, width) restricts it to one block of a big image (blurry_edges_test_big.py:142-150) in place."""
    if img.dim() != 4 or img.shape[0] != 2 or img.shape[1] != 3:
        raise RuntimeError(f"view_image_pair: expected [2,3,H,W], got {tuple(img.shape)}")
    dptr(img, "img")
    _, _, h, w = img.shape
    top, left, bh, bw = window if window is not None else (0, 0, h, w)
    if top < 0 or left < 0 or top + bh > h or left + bw > w or bh < BE_R or bw < BE_R:
        raise RuntimeError(f"view_image_pair: window {window} outside the {h}x{w} image")
    return PatchView(img.data_ptr() + 4 * (top * w + left), 3 * h * w, h * w, w, 1, stride * w, stride,
                     (bw - BE_R) // stride + 1)


def view_flat_patches(pat: torch.Tensor, wp: int) -> PatchView:
    """pat [2,P,3,21,21] (what unfold_patches returns for an image pair)."""
    if pat.dim() != 5 or pat.shape[0] != 2 or tuple(pat.shape[2:]) != (3, BE_R, BE_R):
        raise RuntimeError(f"view_flat_patches: expected [2,P,3,21,21], got {tuple(pat.shape)}")
    dptr(pat, "patches")
    p = pat.shape[1]
    return PatchView(pat.data_ptr(), 3 * NPIX * p, NPIX, BE_R, 1, 3 * NPIX * wp, 3 * NPIX, wp)


def view_unfolded(t: torch.Tensor) -> PatchView:
    """t [2,3,21,21,Hp,Wp]: the layout nn.Unfold(...).view(...) has in blurry_edges_test.py:120."""
    if t.dim() != 6 or t.shape[0] != 2 or tuple(t.shape[1:4]) != (3, BE_R, BE_R):
        raise RuntimeError(f"view_unfolded: expected [2,3,21,21,Hp,Wp], got {tuple(t.shape)}")
    dptr(t, "img_patches")
    hp, wp = t.shape[4], t.shape[5]
    p = hp * wp
    return PatchView(t.data_ptr(), 3 * NPIX * p, NPIX * p, BE_R * p, p, wp, 1, wp)


RENDER_EXTRAS = ("patches", "shpd", "refoc", "boundary", "depth_map", "depth_mask")


def render_full(opts, consts, rho_prime, densify_w, params12, view: PatchView, want=(), pixels=None):
    """params12 [P,12] -> records [P,32] (+ optional per-patch tensors named in `want`:
    'patches','shpd','refoc','boundary','depth_map','depth_mask').  pixels: the tensor `view` points into (the torch operator
    wants to see it; without it the ctypes binding is used)."""
    n = params12.shape[0]
    if tuple(params12.shape) != (n, 12):
        raise RuntimeError(f"render_full: params12 must be [P,12], got {tuple(params12.shape)}")
    dev = params12.device
    o = ops() if pixels is not None else None
    if o is not None:
        mask = sum(1 << i for i, k in enumerate(RENDER_EXTRAS) if k in want)
        r = o.render_full(struct_tensor(opts), struct_tensor(consts), float(rho_prime), bool(densify_w), params12.contiguous(),
                          torch.frombuffer(bytearray(bytes(view)), dtype=torch.uint8), pixels, mask)
        return r[0], dict(zip([k for k in RENDER_EXTRAS if k in want], r[1:]))
    rec = torch.empty(n, RECORD_FLOATS, dtype=torch.float32, device=dev)
    shapes = dict(patches=(n, 2, 3, BE_R, BE_R), shpd=(n, 3, BE_R, BE_R), refoc=(n, 3, BE_R, BE_R),
                  boundary=(n, BE_R, BE_R), depth_map=(n, BE_R, BE_R), depth_mask=(n, BE_R, BE_R))
    extra = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "depth_mask" else torch.float32, device=dev) for k in want}
    g = lambda k: dptr(extra.get(k))
    check(lib().be_render_full_f32(C.byref(opts), C.byref(consts), float(rho_prime), int(bool(densify_w)),
                                   dptr(params12, "params12"), C.byref(view), dptr(rec), g("patches"), g("shpd"),
                                   g("refoc"), g("boundary"), g("depth_map"), g("depth_mask"), n, stream_ptr(dev)),
          "be_render_full_f32")
    return rec, extra


FOLD_MAPS = ("image", "shpd", "refoc", "bndry", "depth", "conf")


def _map_shapes(tail, batch=(), image=(2, 3)):
    """The shape of each folded map over the samples `tail` ((H, W), (Ho, Wo), the points' leading shape, (N,)), after `batch`."""
    tail, batch = tuple(tail), tuple(batch)
    return dict(image=batch + image + tail, shpd=batch + (3,) + tail, refoc=batch + (3,) + tail, bndry=batch + tail, depth=batch + tail,
                conf=batch + tail)


def _fold_maps(want, shapes, dev, by_op, by_lib):
    """The maps named in `want`, as {name: tensor} in FOLD_MAPS order, through either binding: by_op(mask) calls the torch operator
    (bit i of mask = FOLD_MAPS[i]) and returns the requested maps in that order; without the operator library the maps are
    allocated here with `shapes` and by_lib(*pointers) calls the C entry with the six map pointers, null where not wanted.
    A name in `want` that is not in FOLD_MAPS is ignored, under either binding."""
    names = [k for k in FOLD_MAPS if k in want]
    if ops() is not None:
        return dict(zip(names, by_op(sum(1 << FOLD_MAPS.index(k) for k in names))))
    out = {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in names}
    by_lib(*(dptr(out.get(k)) for k in FOLD_MAPS))
    return out


def fold_records(opts, records, hp, wp, H, W, stride=2, densify_w=False, want=FOLD_MAPS):
    if tuple(records.shape) != (hp * wp, RECORD_FLOATS):
        raise RuntimeError(f"fold_records: records must be [{hp * wp},{RECORD_FLOATS}], got {tuple(records.shape)}")
    dev = records.device
    return _fold_maps(
        want, _map_shapes((H, W)), dev,
        lambda mask: ops().fold_records(struct_tensor(opts), records.contiguous(), hp, wp, H, W, stride, bool(densify_w), mask),
        lambda *maps: check(lib().be_fold_records_f32(C.byref(opts), dptr(records, "records"), hp, wp, H, W, stride, int(bool(densify_w)),
                                                      *maps, stream_ptr(dev)), "be_fold_records_f32"))


def fold_records_batch(opts, records, hp, wp, H, W, stride=2, densify_w=False, want=FOLD_MAPS):
    """records [B, hp*wp, 32] -> the maps of fold_records with a leading batch dimension, one launch."""
    if records.dim() != 3 or tuple(records.shape[1:]) != (hp * wp, RECORD_FLOATS):
        raise RuntimeError(f"fold_records_batch: records must be [B,{hp * wp},{RECORD_FLOATS}], got {tuple(records.shape)}")
    dev, B = records.device, records.shape[0]
    return _fold_maps(
        want, _map_shapes((H, W), batch=(B,)), dev,
        lambda mask: ops().fold_records(struct_tensor(opts), records.contiguous(), hp, wp, H, W, stride, bool(densify_w), mask),
        lambda *maps: check(lib().be_fold_records_batch_f32(C.byref(opts), dptr(records, "records"), B, hp, wp, H, W, stride,
                                                            int(bool(densify_w)), *maps, stream_ptr(dev)), "be_fold_records_batch_f32"))


def origin_table(lines, size: int, device, name: str = "origins", cover: bool = False) -> torch.Tensor:
    """One axis of a patch grid given by origins -> the device int32 table the *_grid entry points take.  `lines`: a sequence of
    ints or an integer tensor; checked HERE, on the host, because the kernels trust it: strictly increasing, inside
    [0, size - 21]; cover=True (the fold, which divides by the number of covering patches) also wants every pixel of [0, size)
    under a patch: first origin 0, last size - 21, no gap above 21."""
    vals = [int(v) for v in (lines.tolist() if isinstance(lines, torch.Tensor) else lines)]
    if not vals:
        raise ValueError(f"{name}: empty origin table")
    if any(b <= a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"{name}: patch origins must be strictly increasing")
    if vals[0] < 0 or vals[-1] + BE_R > size:
        raise ValueError(f"{name}: origins {vals[0]}..{vals[-1]} leave [0, {size} - {BE_R}]")
    if cover and (vals[0] != 0 or vals[-1] != size - BE_R or any(b - a > BE_R for a, b in zip(vals, vals[1:]))):
        raise ValueError(f"{name}: the patches do not cover every pixel of [0, {size}) (first origin 0, last {size - BE_R}, gaps <= {BE_R})")
    if isinstance(lines, torch.Tensor) and lines.is_cuda and lines.dtype == torch.int32 and lines.is_contiguous():
        return lines
    return torch.tensor(vals, dtype=torch.int32, device=device)


def render_full_grid(opts, consts, rho_prime, densify_w, params12, img, ys, xs):
    """params12 [HP*WP,12] + img [2,3,H,W] -> records [HP*WP,32] with patch (i, j) at pixel (ys[i], xs[j]): render_full over a
    grid given by origin tables (tiling.patch_grid), one launch.  ys / xs: int sequences or device int32 tensors."""
    if img.dim() != 4 or img.shape[0] != 2 or img.shape[1] != 3:
        raise RuntimeError(f"render_full_grid: expected img [2,3,H,W], got {tuple(img.shape)}")
    dptr(img, "img", (torch.float32,))
    dev, (_, _, H, W) = img.device, img.shape
    ys, xs = origin_table(ys, H, dev, "render_full_grid(ys)"), origin_table(xs, W, dev, "render_full_grid(xs)")
    HP, WP = ys.numel(), xs.numel()
    if tuple(params12.shape) != (HP * WP, 12):
        raise RuntimeError(f"render_full_grid: params12 must be [{HP * WP},12], got {tuple(params12.shape)}")
    o = ops()
    if o is not None:
        return o.render_full_grid(struct_tensor(opts), struct_tensor(consts), float(rho_prime), bool(densify_w), params12.contiguous(),
                                  img, ys, xs)
    rec = torch.empty(HP * WP, RECORD_FLOATS, dtype=torch.float32, device=dev)
    check(lib().be_render_full_grid_f32(C.byref(opts), C.byref(consts), float(rho_prime), int(bool(densify_w)),
                                        dptr(params12, "params12", (torch.float32,)), dptr(img), H, W, dptr(ys), dptr(xs), HP, WP,
                                        dptr(rec), stream_ptr(dev)), "be_render_full_grid_f32")
    return rec


def fold_records_grid(opts, records, H, W, ys, xs, densify_w=False, want=FOLD_MAPS):
    """records [HP*WP,32] of a grid given by origin tables -> the maps of fold_records on an H x W image; each pixel is divided
    by the number of patches that cover it.  The tables must cover every pixel (checked here)."""
    dev = records.device
    ys, xs = origin_table(ys, H, dev, "fold_records_grid(ys)", cover=True), origin_table(xs, W, dev, "fold_records_grid(xs)", cover=True)
    HP, WP = ys.numel(), xs.numel()
    if tuple(records.shape) != (HP * WP, RECORD_FLOATS):
        raise RuntimeError(f"fold_records_grid: records must be [{HP * WP},{RECORD_FLOATS}], got {tuple(records.shape)}")
    return _fold_maps(
        want, _map_shapes((H, W)), dev,
        lambda mask: ops().fold_records_grid(struct_tensor(opts), records.contiguous(), ys, xs, H, W, bool(densify_w), mask),
        lambda *maps: check(lib().be_fold_records_grid_f32(C.byref(opts), dptr(records, "records", (torch.float32,)), HP, WP, H, W, dptr(ys),
                                                           dptr(xs), int(bool(densify_w)), *maps, stream_ptr(dev)), "be_fold_records_grid_f32"))


REFOCUS_STACK_KC = 8          # BE_REFOCUS_STACK_KC of the header: the planes one workgroup of a stack fold accumulates


def rho_prime_list(rho_primes, name: str = "rho_primes"):
    """A sequence of floats or a tensor of optical powers -> a list of python floats, checked on the host (before any native
    code is touched): one dimension, non-empty, finite."""
    if isinstance(rho_primes, torch.Tensor):
        if rho_primes.dim() != 1:
            raise ValueError(f"{name}: expected a 1-d tensor of optical powers, got shape {tuple(rho_primes.shape)}")
        vals = rho_primes.detach().double().cpu().tolist()
    else:
        vals = [float(v) for v in rho_primes]
    if not vals:
        raise ValueError(f"{name}: empty - a focal stack needs at least one optical power")
    if not all(v == v and abs(v) != float("inf") for v in vals):
        raise ValueError(f"{name}: optical powers must be finite, got {vals}")
    return vals


def _rho_tensor(rho_primes, vals, dev):
    """The float32 [K] tensor on `dev` the stack entries read: rho_primes itself when it already is one, else built from
    vals = rho_prime_list(rho_primes)."""
    if isinstance(rho_primes, torch.Tensor) and rho_primes.device == dev and rho_primes.dtype == torch.float32 and rho_primes.is_contiguous():
        return rho_primes
    return torch.tensor(vals, dtype=torch.float32, device=dev)


def _record_grid(who, records, H, W, hp, wp, ys, xs):
    """The host side the wrappers over an optional-table grid share, before the library is touched: ys / xs both or neither, the
    tables (origin_table, cover=True), the record shape, records on the GPU.  -> (records, ys, xs, hp, wp)."""
    if (ys is None) != (xs is None):
        raise ValueError(f"{who}: ys and xs must both be given (origin tables) or both be None (uniform grid)")
    if not isinstance(records, torch.Tensor) or records.dim() != 2:
        raise RuntimeError(f"{who}: records must be a [P,{RECORD_FLOATS}] tensor")
    dev = records.device
    if ys is not None:
        ys, xs = origin_table(ys, H, dev, f"{who}(ys)", cover=True), origin_table(xs, W, dev, f"{who}(xs)", cover=True)
        if (hp is not None and hp != ys.numel()) or (wp is not None and wp != xs.numel()):
            raise RuntimeError(f"{who}: hp / wp ({hp}, {wp}) do not match the tables ({ys.numel()}, {xs.numel()})")
        hp, wp = ys.numel(), xs.numel()
    elif hp is None or wp is None:
        raise RuntimeError(f"{who}: the uniform grid needs hp and wp")
    if tuple(records.shape) != (hp * wp, RECORD_FLOATS):
        raise RuntimeError(f"{who}: records must be [{hp * wp},{RECORD_FLOATS}], got {tuple(records.shape)}")
    records = records.contiguous()
    dptr(records, "records", (torch.float32,))
    return records, ys, xs, hp, wp


def fold_refocus_stack(opts, consts, records, rho_primes, H, W, hp=None, wp=None, stride=2, ys=None, xs=None):
    """records [hp*wp,32] (render_full / render_full_grid at ANY rho_prime) + K optical powers -> [K,3,H,W]: plane k is the
    `refoc` map of render_full*(rho_prime=rho_primes[k]) + fold_records*, bit for bit, from one launch that shares the record
    fetch and the wedge distances between the planes.  ys / xs (both): origin tables as fold_records_grid takes them (hp / wp
    then come from the tables); neither: the uniform grid hp x wp of `stride`.  rho_primes: floats or a float32 tensor."""
    vals = rho_prime_list(rho_primes, "fold_refocus_stack(rho_primes)")
    records, ys, xs, hp, wp = _record_grid("fold_refocus_stack", records, H, W, hp, wp, ys, xs)
    dev = records.device
    rho = _rho_tensor(rho_primes, vals, dev)
    o = ops()
    if o is not None:
        return o.fold_refocus_stack(struct_tensor(opts), struct_tensor(consts), records, rho, ys, xs, hp, wp, H, W, stride)
    out = torch.empty(len(vals), 3, H, W, dtype=torch.float32, device=dev)
    check(lib().be_fold_refocus_stack_f32(C.byref(opts), C.byref(consts), dptr(records, "records", (torch.float32,)), hp, wp, H, W,
                                          stride, dptr(ys), dptr(xs), dptr(rho), len(vals), dptr(out), stream_ptr(dev)),
          "be_fold_refocus_stack_f32")
    return out


def _at_grid(who, records, H, W, scale, window, hp, wp, ys, xs):
    """The lattice (tiling.lattice), then _record_grid.  -> (lattice, records, ys, xs, hp, wp)."""
    from . import tiling
    lat = tiling.lattice(H, W, scale, window)
    return (lat,) + _record_grid(who, records, H, W, hp, wp, ys, xs)


def fold_records_at(opts, records, H, W, scale=1, window=None, hp=None, wp=None, stride=2, ys=None, xs=None, densify_w=False,
                    want=FOLD_MAPS):
    """records [hp*wp,32] -> the maps of fold_records / fold_records_grid sampled on a lattice `scale` times finer than the pixels,
    over window = (top, left, h, w) of the H x W image (None: all of it): each map [..,Ho,Wo], Ho = (h-1)*scale + 1.  Sample
    (iy, ix) sits at pixel position (top + iy / scale, left + ix / scale); out[..., ::scale, ::scale] equals the integer-pixel fold
    over the window bit for bit.  ys / xs (both): origin tables (hp / wp then come from them); neither: the uniform grid."""
    lat, records, ys, xs, hp, wp = _at_grid("fold_records_at", records, H, W, scale, window, hp, wp, ys, xs)
    dev, (top, left, h, w) = records.device, lat["window"]
    return _fold_maps(
        want, _map_shapes((lat["Ho"], lat["Wo"])), dev,
        lambda mask: ops().fold_records_at(struct_tensor(opts), records, ys, xs, hp, wp, H, W, stride, scale, top, left, h, w,
                                           bool(densify_w), mask),
        lambda *maps: check(lib().be_fold_records_at_f32(C.byref(opts), dptr(records, "records", (torch.float32,)), hp, wp, H, W, stride,
                                                         dptr(ys), dptr(xs), scale, top, left, h, w, int(bool(densify_w)), *maps,
                                                         stream_ptr(dev)), "be_fold_records_at_f32"))


def fold_refocus_stack_at(opts, consts, records, rho_primes, H, W, scale=1, window=None, hp=None, wp=None, stride=2, ys=None, xs=None):
    """fold_refocus_stack on the lattice of fold_records_at: [K,3,Ho,Wo]; plane k at [::scale, ::scale] equals fold_refocus_stack's
    plane over the window bit for bit."""
    vals = rho_prime_list(rho_primes, "fold_refocus_stack_at(rho_primes)")
    lat, records, ys, xs, hp, wp = _at_grid("fold_refocus_stack_at", records, H, W, scale, window, hp, wp, ys, xs)
    dev, (top, left, h, w) = records.device, lat["window"]
    rho = _rho_tensor(rho_primes, vals, dev)
    o = ops()
    if o is not None:
        return o.fold_refocus_stack_at(struct_tensor(opts), struct_tensor(consts), records, rho, ys, xs, hp, wp, H, W, stride, scale, top,
                                       left, h, w)
    out = torch.empty(len(vals), 3, lat["Ho"], lat["Wo"], dtype=torch.float32, device=dev)
    check(lib().be_fold_refocus_stack_at_f32(C.byref(opts), C.byref(consts), dptr(records, "records", (torch.float32,)), hp, wp, H, W,
                                             stride, dptr(ys), dptr(xs), scale, top, left, h, w, dptr(rho), len(vals), dptr(out),
                                             stream_ptr(dev)), "be_fold_refocus_stack_at_f32")
    return out


def _point_list(who, points):
    """points [...,2] float32 (y, x) -> (the contiguous [N,2] view the kernels read, the leading shape).  Checked before the library."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be a float32 tensor [...,2] of (y, x) positions, got "
                         f"{getattr(points, 'dtype', type(points).__name__)}")
    if points.dim() < 1 or points.shape[-1] != 2 or points.numel() == 0:
        raise ValueError(f"{who}: points must be [...,2] with at least one point, got {tuple(points.shape)}")
    return points.reshape(-1, 2).contiguous(), tuple(points.shape[:-1])


def fold_records_points(opts, records, H, W, points, hp=None, wp=None, stride=2, ys=None, xs=None, densify_w=False, want=FOLD_MAPS):
    """records [hp*wp,32] -> the maps of fold_records / fold_records_grid evaluated at points [...,2]: float32 (y, x) positions on the
    records' device, in input-pixel coordinates (pixel centres at the integers, the domain 0 <= y <= H-1, 0 <= x <= W-1 closed).
    Each map keeps the points' leading shape: image [2,3,*lead], shpd / refoc [3,*lead], bndry / depth / conf [*lead].  A point on a
    pixel centre equals the integer-pixel fold bit for bit; a point outside the domain (NaN included) gives 0 in every map.
    ys / xs (both): origin tables (hp / wp then come from them); neither: the uniform grid."""
    pts, lead = _point_list("fold_records_points", points)
    records, ys, xs, hp, wp = _record_grid("fold_records_points", records, H, W, hp, wp, ys, xs)
    dev, N = records.device, pts.shape[0]
    dptr(pts, "points", (torch.float32,))
    out = _fold_maps(                                                   # the kernels write channel-major over the points: [6,N], [3,N], [N]
        want, _map_shapes((N,), image=(6,)), dev,
        lambda mask: ops().fold_records_points(struct_tensor(opts), records, ys, xs, hp, wp, H, W, stride, pts, bool(densify_w), mask),
        lambda *maps: check(lib().be_fold_records_points_f32(C.byref(opts), dptr(records, "records", (torch.float32,)), hp, wp, H, W, stride,
                                                             dptr(ys), dptr(xs), dptr(pts), N, int(bool(densify_w)), *maps,
                                                             stream_ptr(dev)), "be_fold_records_points_f32"))
    shapes = _map_shapes(lead)
    return {k: v.view(shapes[k]) for k, v in out.items()}


def fold_refocus_stack_points(opts, consts, records, rho_primes, H, W, points, hp=None, wp=None, stride=2, ys=None, xs=None):
    """fold_refocus_stack at the points of fold_records_points: [K,3,*lead]; plane k at a pixel centre equals fold_refocus_stack's
    pixel bit for bit."""
    vals = rho_prime_list(rho_primes, "fold_refocus_stack_points(rho_primes)")
    pts, lead = _point_list("fold_refocus_stack_points", points)
    records, ys, xs, hp, wp = _record_grid("fold_refocus_stack_points", records, H, W, hp, wp, ys, xs)
    dev, N = records.device, pts.shape[0]
    dptr(pts, "points", (torch.float32,))
    rho = _rho_tensor(rho_primes, vals, dev)
    o = ops()
    if o is not None:
        out = o.fold_refocus_stack_points(struct_tensor(opts), struct_tensor(consts), records, rho, ys, xs, hp, wp, H, W, stride, pts)
    else:
        out = torch.empty(len(vals), 3, N, dtype=torch.float32, device=dev)
        check(lib().be_fold_refocus_stack_points_f32(C.byref(opts), C.byref(consts), dptr(records, "records", (torch.float32,)), hp, wp, H, W,
                                                     stride, dptr(ys), dptr(xs), dptr(pts), N, dptr(rho), len(vals), dptr(out),
                                                     stream_ptr(dev)), "be_fold_refocus_stack_points_f32")
    return out.view((len(vals), 3) + lead)


# ---- the geometry entries (unproject .. fill_diffuse): one statement per kind of argument.  A new entry starts from these; the numbers
# that need no torch (check_size, check_number) sit in camera.py beside as_pinhole / as_pose.  The tensor checks take CPU tensors too,
# except _depth_map's on_gpu: tests/test_geometry_args_cpu.py runs every one of them without a GPU.
TARGET_MAX_SIDE, TARGET_MAX_PIXELS = 1 << 24, 0x7fffffff                # a target image: float32 holds its coordinates, int32 its pixel indices


def _got(t):
    return f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}"


def _target_size(who, size):
    """size -> (Ho, Wo) of the image a splatting or ray-casting entry writes (raster.check_params states the rasteriser's own bound)."""
    from . import camera
    return camera.check_size(who, size, TARGET_MAX_SIDE, "size must be (Ho, Wo), integers >= 1 with Ho * Wo < 2^31", TARGET_MAX_PIXELS)


def _near(who, near):
    """near -> float, or "{who}: near must be a finite number >= 0"."""
    from . import camera
    return camera.check_number(who, "near", near)


def _depth_map(who, depth, statement, dims="[Hs,Ws]", on_gpu=True):
    """A depth map: a float32 tensor [H,W] with at least one sample, on the GPU -> depth.  `statement` names the host statement."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"{who}: depth must be a float32 tensor {dims}, got {_got(depth)}")
    if on_gpu and not depth.is_cuda:
        raise ValueError(f"{who}: depth is not on the GPU; nothing here computes on the CPU ({statement} is the host statement)")
    return depth


def _map_like(who, name, t, depth, dtypes=(torch.float32,), kind="a float32"):
    """An optional map on the samples of depth (weight, edge): one of `dtypes`, depth's shape, on depth's device -> float32 and
    contiguous (a bool mask becomes 1 / 0); None stays None."""
    if t is None:
        return None
    H, W = depth.shape
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != (H, W):
        raise ValueError(f"{who}: {name} must be {kind} tensor [{H},{W}], got {_got(t)}")
    if t.device != depth.device:
        raise ValueError(f"{who}: {name} is on {t.device}, depth on {depth.device}")
    return t.to(torch.float32).contiguous()


def _channels(who, name, t, depth, C=None, required=False):
    """Channels that ride on the samples of depth (feat; normal_d: C=3, required): float32 [C,Hs,Ws] or [C,Hs*Ws] on depth's device
    -> [C,Hs*Ws] contiguous; None stays None unless required."""
    if t is None and not required:
        return None
    Hs, Ws = depth.shape
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (2, 3) or (C is not None and t.shape[0] != C)
            or tuple(t.shape[1:]) not in ((Hs, Ws), (Hs * Ws,))):
        raise ValueError(f"{who}: {name} must be a float32 tensor [{C or 'C'},{Hs},{Ws}] or [{C or 'C'},{Hs * Ws}], got {_got(t)}")
    if t.device != depth.device:
        raise ValueError(f"{who}: {name} is on {t.device}, depth on {depth.device}")
    return t.reshape(t.shape[0], Hs * Ws).contiguous()


def view_list(who, views, of):
    """views -> list(views), or "{who}: views must be a list of {of}" for what cannot be iterated."""
    try:
        return list(views)
    except TypeError:
        raise ValueError(f"{who}: views must be a list of {of}, got {type(views).__name__}") from None


def _new(dev):
    """The allocator of the ctypes arms: new(*shape, dtype=float32) -> an uninitialised tensor on dev."""
    return lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)


def _view(who, v, keys, cam_key, dev=None, whose=None):
    """One view dict (fuse_views / tsdf_integrate: FUSE_VIEW_KEYS, "cam_src"; icp_linearize / register_depth: ICP_VIEW_KEYS, "cam"),
    validated -> (depth [Hs,Ws], weight [Hs,Ws] or None, feat [C,Hs*Ws] or None, camera float32 [4], pose float32 [12], scale, top,
    left), every tensor contiguous on one device - `dev`, which belongs to `whose`, when given."""
    if not isinstance(v, dict) or "depth" not in v or cam_key not in v:
        raise ValueError(f"{who}: a view is a dict with the keys {keys} (depth and {cam_key} at least)")
    unknown = [k for k in v if k not in keys]
    if unknown:
        raise ValueError(f"{who}: unknown keys {unknown}; a view holds {keys}")
    scale = v.get("scale", 1)
    depth, (cs,), p12, top, left = _reproject_args(who, v["depth"], [(cam_key, v[cam_key])], v.get("pose"), scale, v.get("window_origin", (0, 0)))
    if dev is not None and depth.device != dev:
        raise ValueError(f"{who}: depth is on {depth.device}, {whose} on {dev}")
    return depth, _map_like(who, "weight", v.get("weight"), depth), _channels(who, "feat", v.get("feat"), depth), cs, p12, scale, top, left


def _reproject_args(who, depth, cams, pose, scale, window_origin):
    """The host side unproject and reproject share, before the library is touched: depth [Hs,Ws] float32 on the GPU, the cameras
    (camera.Pinhole, (fy, fx, cy, cx) or a 3x3 K) and the pose (camera.as_pose) as float32 numpy, scale in 1..16, the window
    origin.  -> (depth, [camera float32 [4]], pose float32 [12], top, left)."""
    from . import camera, tiling
    _depth_map(who, depth, "camera.splat_f32")
    if depth.numel() > 0x7fffffff:
        raise ValueError(f"{who}: {depth.numel()} source samples; at most 2^31 - 1 (the index map is int32)")
    if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= tiling.MAX_SCALE:
        raise ValueError(f"{who}: scale must be an integer in [1, {tiling.MAX_SCALE}], got {scale!r}")
    try:
        top, left = window_origin
        ok = all(not isinstance(v, bool) and int(v) == v and 0 <= v <= 1 << 24 for v in (top, left))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: window_origin must be (top, left), integers >= 0, got {window_origin!r}")
    cams = [camera.as_pinhole(c, f"{who}({n})").f32() for n, c in cams]
    return depth.contiguous(), cams, camera.as_pose(pose, f"{who}(pose)"), int(top), int(left)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def unproject(depth, cam_src, pose=None, scale=1, window_origin=(0, 0)):
    """depth [Hs,Ws] (metres along the optical axis; sample (iy, ix) at (top + iy / scale, left + ix / scale) in source pixels)
    -> xyz [3,Hs,Ws]: the samples as points (X, Y, Z) in the frame `pose` maps the source camera's to (None: the camera's own);
    0 in all three where the depth is not a finite number > 0.  camera.unproject_f32 is the host statement, bit for bit."""
    depth, (cs,), p12, top, left = _reproject_args("unproject", depth, [("cam_src", cam_src)], pose, scale, window_origin)
    Hs, Ws = depth.shape
    o = ops()
    if o is not None:
        return o.unproject(depth, torch.from_numpy(cs), torch.from_numpy(p12), scale, top, left)
    xyz = torch.empty(3, Hs, Ws, dtype=torch.float32, device=depth.device)
    check(lib().be_unproject_f32(dptr(depth, "depth", (torch.float32,)), Hs, Ws, scale, top, left, _fptr(cs), _fptr(p12), dptr(xyz),
                                 stream_ptr(depth.device)), "be_unproject_f32")
    return xyz


def reproject(depth, cam_src, cam_dst, pose, size, feat=None, near=1e-3, scale=1, window_origin=(0, 0)):
    """Forward warp of depth [Hs,Ws] (the samples of unproject) from cam_src to cam_dst, size = (Ho, Wo): every sample with a
    finite depth > 0 whose depth in the target frame exceeds `near` and whose projection rounds to a pixel of the target is
    splatted there; the nearest wins, on equal depth the lowest source index.  -> dict(depth [Ho,Wo] in the target frame,
    index [Ho,Wo] int32 = the winner's iy * Ws + ix, valid = index >= 0 (on the device, no sync), feat [C,Ho,Wo] gathered from
    feat [C,Hs,Ws] or [C,Hs*Ws] - None when feat is None); +0 / -1 / False / +0 where nothing landed.  The result does not depend
    on the order of execution; camera.splat_f32 is the host statement, bit for bit."""
    depth, (cs, cd), p12, top, left = _reproject_args("reproject", depth, [("cam_src", cam_src), ("cam_dst", cam_dst)], pose, scale,
                                                      window_origin)
    Ho, Wo = _target_size("reproject", size)
    near = _near("reproject", near)
    Hs, Ws = depth.shape
    dev = depth.device
    feat = _channels("reproject", "feat", feat, depth)
    o = ops()
    if o is not None:
        d, index, f = o.reproject(depth, torch.from_numpy(cs), torch.from_numpy(cd), torch.from_numpy(p12), near, Ho, Wo, feat, scale,
                                  top, left)
        f = f if feat is not None else None
    else:
        new = _new(dev)
        zbuf, d, index = new(Ho * Wo, dtype=torch.int64), new(Ho, Wo), new(Ho, Wo, dtype=torch.int32)
        C_ = 0 if feat is None else feat.shape[0]
        f = None if feat is None else new(C_, Ho, Wo)
        check(lib().be_reproject_f32(dptr(depth, "depth", (torch.float32,)), Hs, Ws, scale, top, left, _fptr(cs), _fptr(cd), _fptr(p12),
                                     near, Ho, Wo, dptr(feat if C_ else None), C_, dptr(zbuf, "zbuf", (torch.int64,)), dptr(d),
                                     dptr(index), dptr(f if C_ else None), stream_ptr(dev)), "be_reproject_f32")
    return dict(depth=d, index=index, valid=index >= 0, feat=f)


FUSE_VIEW_KEYS = ("depth", "weight", "feat", "cam_src", "pose", "scale", "window_origin")


def fuse_views(views, cam_dst, size, tau=0.05, min_views=1, recentre=True, peel=0, near=1e-3):
    """The depth of several views merged in one camera.  views: a list of 1..32 dicts with the keys depth [Hs,Ws] (float32 on the
    GPU, the samples of reproject), weight [Hs,Ws] or None (1 everywhere), feat [C,Hs,Ws] / [C,Hs*Ws] or None (the same C in
    every view), cam_src, pose (this view's frame -> the target's; None: the identity), scale and window_origin (as reproject;
    1 and (0, 0) when absent).  Every sample is projected into cam_dst, size = (Ho, Wo), as reproject projects it.  Per target
    pixel the samples with a weight > 0 that lie within tau (metres) behind the nearest one are averaged with their weights;
    recentre repeats the average over the window of half-width tau about that first mean, which removes the bias of measuring
    from a noisy front.  A pixel is kept when samples of at least min_views distinct views agree; otherwise its front cluster is
    peeled off and the next of `peel` further rounds looks behind it - a sample no second view confirms does not hide the
    surface behind it.  -> dict(depth [Ho,Wo], valid = layer >= 0 (on the device, no sync), weight [Ho,Wo] = the sum of the
    members' weights, views, count, layer [Ho,Wo] int32 = the distinct views and the samples that agreed and the round that kept
    the pixel, feat [C,Ho,Wo] = the weighted mean of the members' channels, None without feat); +0 / False / 0 / 0 / 0 / -1 / +0
    where no pixel was kept - holes are left open (fill_nearest / fill_diffuse with (out["depth"], out["weight"]) close them).
    The sums are integers in fixed point (weights in 2^-16, clamped to 16; depth offsets in 2^-20 m; channels in 2^-16, clamped to
    +-2048) under integer atomics: the result depends neither on the order of execution nor on the order of the views, and is
    exact while fewer than 2^16 samples agree on one pixel.  Nothing synchronises with the host.  fusion.fuse is the host
    statement, bit for bit; with tau=0, recentre=False, peel=0 and one view depth and valid are reproject's."""
    from . import camera, fusion
    views = view_list("fuse_views", views, f"dicts with the keys {FUSE_VIEW_KEYS}")
    tau, min_views, recentre, peel = fusion.check_params("fuse_views", len(views), tau, min_views, recentre, peel)
    Ho, Wo = _target_size("fuse_views", size)
    near = _near("fuse_views", near)
    cd = camera.as_pinhole(cam_dst, "fuse_views(cam_dst)").f32()
    checked, dev = [], None
    for i, v in enumerate(views):
        checked.append(_view(f"fuse_views(views[{i}])", v, FUSE_VIEW_KEYS, "cam_src", dev, "the first view's"))
        dev = checked[0][0].device
    depths, weights, feats, cams, poses, scales, tops, lefts = map(list, zip(*checked))
    Cs = sorted({0 if f is None else f.shape[0] for f in feats})
    if len(Cs) != 1:
        raise ValueError(f"fuse_views: every view must carry the same number of feat channels (or none), got {Cs}")
    C_ = Cs[0]
    if C_ > FUSE_MAX_CHANNELS:
        raise ValueError(f"fuse_views: feat holds {C_} channels; at most {FUSE_MAX_CHANNELS}")
    import numpy as np
    V = len(views)
    cam_all, pose_all = np.ascontiguousarray(np.stack(cams), np.float32), np.ascontiguousarray(np.stack(poses), np.float32)
    o = ops()
    if o is not None:
        empty = torch.empty(0, dtype=torch.float32, device=dev)
        d, wsum, nviews, count, layer, f = o.fuse_views(depths, [empty if w is None else w for w in weights], feats if C_ else [],
                                                        torch.from_numpy(cam_all), torch.from_numpy(pose_all), torch.from_numpy(cd), near, Ho, Wo,
                                                        scales, tops, lefts, tau, min_views, recentre, peel)
    else:
        new = _new(dev)
        scratch = new(lib().be_fuse_scratch_bytes(Ho, Wo, C_) // 8 + 1, dtype=torch.int64)
        d, wsum, f = new(Ho, Wo), new(Ho, Wo), new(C_, Ho, Wo)
        nviews, count, layer = (new(Ho, Wo, dtype=torch.int32) for _ in range(3))
        ptrs = lambda ts: (C.c_void_p * V)(*[None if t is None else t.data_ptr() for t in ts])
        ints = lambda xs: (C.c_int * V)(*xs)
        check(lib().be_fuse_views_f32(V, ptrs(depths), ptrs(weights), ptrs(feats) if C_ else None, C_, ints([t.shape[0] for t in depths]),
                                      ints([t.shape[1] for t in depths]), ints(scales), ints(tops), ints(lefts), _fptr(cam_all),
                                      _fptr(pose_all), _fptr(cd), near, Ho, Wo, tau, min_views, int(recentre), peel,
                                      dptr(scratch, "scratch", (torch.int64,)), dptr(d), dptr(wsum), dptr(nviews), dptr(count), dptr(layer),
                                      dptr(f if C_ else None), stream_ptr(dev)), "be_fuse_views_f32")
    return dict(depth=d, valid=layer >= 0, weight=wsum, views=nviews, count=count, layer=layer, feat=f if C_ else None)


def tsdf_volume(dims, origin, voxel, trunc, C=0, device="cuda"):
    """An empty truncated signed distance volume on the GPU -> volume.Volume: dims = (Nz, Ny, Nx) voxels (each in 1..1024, product
    < 2^31), origin = (X0, Y0, Z0) the centre of voxel (0, 0, 0), voxel = (sX, sY, sZ) the spacing per axis (the pipeline's own
    camera sees 3 cm across at 1 m with centimetres of depth noise: cubes are useless to it), trunc the truncation distance, all
    in metres; C channels ride along.  Its sums sw int32 [Nz,Ny,Nx], swd int64 [Nz,Ny,Nx] and swf int64 [C,Nz,Ny,Nx] start at zero."""
    from . import volume
    dims, origin, voxel, trunc, C_ = volume.check_params("tsdf_volume", dims, origin, voxel, trunc, C)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("tsdf_volume: the volume lives on the GPU; nothing here computes on the CPU (volume.Volume is the host statement)")
    return volume.Volume(dims, origin, voxel, trunc, C_, torch.zeros(dims, dtype=torch.int32, device=dev),
                         torch.zeros(dims, dtype=torch.int64, device=dev), torch.zeros((C_,) + dims, dtype=torch.int64, device=dev))


def _tsdf_state(who, vol):
    """The volume's description as the host arrays the entries take, its sums checked -> (dims int32 [3], origin, voxel float32 [3])."""
    from . import volume
    import numpy as np
    if not isinstance(vol, volume.Volume):
        raise ValueError(f"{who}: volume must be a volume.Volume (native.tsdf_volume makes one), got {type(vol).__name__}")
    dims, origin, voxel, trunc, C_ = volume.check_params(who, vol.dims, vol.origin, vol.voxel, vol.trunc, vol.C)
    for name, t, dt, shape in (("sw", vol.sw, torch.int32, dims), ("swd", vol.swd, torch.int64, dims), ("swf", vol.swf, torch.int64, (C_,) + dims)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: volume.{name} must be a contiguous {dt} tensor {shape} on the GPU (volume.integrate is the host "
                             f"statement), got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        if t.device != vol.sw.device:
            raise ValueError(f"{who}: volume.{name} is on {t.device}, volume.sw on {vol.sw.device}")
    return np.array(dims, np.int32), np.array(origin, np.float32), np.array(voxel, np.float32)


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def tsdf_integrate(volume, views, near=1e-3):
    """views: fuse_views' view dicts (depth, weight, feat, cam_src, pose = the view's frame -> the volume's, scale,
    window_origin), each integrated into `volume` (native.tsdf_volume) in place, one launch per view -> volume.  A voxel takes the
    sample its centre projects to (the nearest of the view's lattice) when that sample's depth is a finite number > 0, its weight
    > 0 and the voxel lies no further than trunc behind it; it adds the weight, the weighted signed distance clamped to trunc and
    the weighted channels to its integer sums (weights in 2^-8, clamped to 16; distances in trunc * 2^-15; channels in 2^-16,
    clamped to +-2048).  Every view must carry the volume's C channels.  Each voxel is owned by one thread: no atomics, and the
    sums depend neither on the order of the views nor on how they are grouped into calls; exact below 2^19 views.  Nothing
    synchronises with the host.  volume.integrate is the host statement, bit for bit."""
    dims, origin, voxel = _tsdf_state("tsdf_integrate", volume)
    views = view_list("tsdf_integrate", views, f"dicts with the keys {FUSE_VIEW_KEYS}")
    near = _near("tsdf_integrate", near)
    dev = volume.sw.device
    checked = []
    for i, v in enumerate(views):
        who = f"tsdf_integrate(views[{i}])"
        item = _view(who, v, FUSE_VIEW_KEYS, "cam_src", dev, "the volume")
        if (0 if item[2] is None else item[2].shape[0]) != volume.C:
            raise ValueError(f"{who}: feat holds {0 if item[2] is None else item[2].shape[0]} channels, the volume {volume.C}")
        checked.append(item)
    o = ops()
    for depth, w, f, cs, p12, scale, top, left in checked:
        Hs, Ws = depth.shape
        if o is not None:
            o.tsdf_integrate(depth, w, f, torch.from_numpy(cs), torch.from_numpy(p12), near, scale, top, left, torch.from_numpy(origin),
                             torch.from_numpy(voxel), volume.trunc, volume.sw, volume.swd, volume.swf)
        else:
            check(lib().be_tsdf_integrate_f32(dptr(depth, "depth", (torch.float32,)), dptr(w), dptr(f), volume.C, Hs, Ws, scale, top, left,
                                              _fptr(cs), _fptr(p12), near, _iptr(dims), _fptr(origin), _fptr(voxel), volume.trunc,
                                              dptr(volume.sw, "sw", (torch.int32,)), dptr(volume.swd, "swd", (torch.int64,)),
                                              dptr(volume.swf if volume.C else None, "swf", (torch.int64,)), stream_ptr(dev)),
                  "be_tsdf_integrate_f32")
    return volume


def tsdf_mean(volume):
    """The means of a volume's sums -> (D [Nz,Ny,Nx] = the signed distance in units of trunc, in [-1, 1], W [Nz,Ny,Nx] = the sum
    of the weights, Fm [C,Nz,Ny,Nx] = the weighted mean channels); D and Fm +0 where the voxel holds nothing (W == 0).
    volume.mean is the host statement, bit for bit."""
    dims, _, _ = _tsdf_state("tsdf_mean", volume)
    o = ops()
    if o is not None:
        return tuple(o.tsdf_mean(volume.sw, volume.swd, volume.swf))
    dev = volume.sw.device
    D = torch.empty(volume.dims, dtype=torch.float32, device=dev)
    W = torch.empty(volume.dims, dtype=torch.float32, device=dev)
    Fm = torch.empty((volume.C,) + volume.dims, dtype=torch.float32, device=dev)
    check(lib().be_tsdf_mean_f32(_iptr(dims), volume.C, dptr(volume.sw, "sw", (torch.int32,)), dptr(volume.swd, "swd", (torch.int64,)),
                                 dptr(volume.swf if volume.C else None, "swf", (torch.int64,)), dptr(D), dptr(W),
                                 dptr(Fm if volume.C else None), stream_ptr(dev)), "be_tsdf_mean_f32")
    return D, W, Fm


def tsdf_raycast(volume, cam_dst, pose, size, z_range, step=None, normals=False, normals_kw=None):
    """The volume as the camera cam_dst sees it from `pose` (camera.pose: the camera's frame -> the volume's; None: the identity),
    size = (Ho, Wo): every pixel's ray is sampled at z = z_near + i * step (z_range = (z_near, z_far) in metres along the optical
    axis, 0 < z_near; step None: trunc / 4; at most 4096 samples), the signed distance is interpolated trilinearly where all 8
    voxels about the sample hold data, and the first crossing from in front (> 0) to behind (<= 0) between two consecutive valid
    samples is the surface, placed by linear interpolation.  -> dict(depth [Ho,Wo] = Z in the camera's frame, valid (depth > 0;
    on the device, no sync), weight [Ho,Wo] = the interpolated sum of weights, feat [C,Ho,Wo] or None); +0 / False where no ray
    hit.  normals=True: also normal [3,Ho,Wo] and normal_valid, depth_normals(depth, cam_dst, **normals_kw).  Runs tsdf_mean,
    then the ray cast; nothing synchronises with the host.  volume.raycast is the host statement, bit for bit."""
    from . import camera, volume as volume_
    dims, origin, voxel = _tsdf_state("tsdf_raycast", volume)
    Ho, Wo = _target_size("tsdf_raycast", size)
    z_near, _, step, n = volume_.check_raycast("tsdf_raycast", z_range, step, volume.trunc)
    cd = camera.as_pinhole(cam_dst, "tsdf_raycast(cam_dst)").f32()
    p12 = camera.as_pose(pose, "tsdf_raycast(pose)")
    D, W, Fm = tsdf_mean(volume)
    dev = D.device
    o = ops()
    if o is not None:
        d, w, f = o.tsdf_raycast(D, W, Fm, torch.from_numpy(origin), torch.from_numpy(voxel), torch.from_numpy(cd), torch.from_numpy(p12),
                                 Ho, Wo, z_near, step, n)
    else:
        new = _new(dev)
        d, w, f = new(Ho, Wo), new(Ho, Wo), new(volume.C, Ho, Wo)
        check(lib().be_tsdf_raycast_f32(dptr(D), dptr(W), dptr(Fm if volume.C else None), volume.C, _iptr(dims), _fptr(origin), _fptr(voxel),
                                        _fptr(cd), _fptr(p12), Ho, Wo, z_near, step, n, dptr(d), dptr(w), dptr(f if volume.C else None),
                                        stream_ptr(dev)), "be_tsdf_raycast_f32")
    out = dict(depth=d, valid=d > 0, weight=w, feat=f if volume.C else None)
    if normals:
        nrm = depth_normals(d, cam_dst, **dict(normals_kw or {}))
        out.update(normal=nrm["normal"], normal_valid=nrm["valid"])
    return out


def exclusive_scan(counts):
    """counts: a uint8 tensor [n] on the GPU (n >= 0) -> (offsets int32 [n], offsets[i] = counts[0] + .. + counts[i - 1], total int64
    [1] on the device = the sum of all counts).  Three launches - sums per workgroup of 1024 counts, a scan of those sums in 64
    bits by one workgroup, 256 at a time, and the apply pass - with wave shuffles inside; integer sums, so the result is the same
    on every run.  No workgroup waits for another.  Nothing synchronises with the host."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.uint8 or counts.dim() != 1:
        raise ValueError(f"exclusive_scan: counts must be a uint8 tensor [n], got {getattr(counts, 'dtype', type(counts).__name__)} "
                         f"{tuple(getattr(counts, 'shape', ()))}")
    if not counts.is_cuda:
        raise ValueError("exclusive_scan: counts must be on the GPU; nothing here computes on the CPU (numpy.cumsum is the host statement)")
    counts = counts.contiguous()
    o = ops()
    if o is not None:
        return tuple(o.exclusive_scan(counts))
    n, dev = counts.numel(), counts.device
    offsets = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = lib().be_exclusive_scan_workspace_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    check(lib().be_exclusive_scan_u8_i32(dptr(counts, "counts", (torch.uint8,)) if n else None, n, dptr(offsets) if n else None,
                                         dptr(total, "total", (torch.int64,)), dptr(ws, "workspace", (torch.int64,)), nbytes, stream_ptr(dev)),
          "be_exclusive_scan_u8_i32")
    return offsets, total


def mesh_field(D, W, Fm=None, origin=(0.0, 0.0, 0.0), voxel=(1.0, 1.0, 1.0), min_weight=0.0, normals=True):
    """A triangle mesh out of a signed distance field: D, W [Nz,Ny,Nx] and Fm [C,Nz,Ny,Nx] or None (float32 on the GPU, as tsdf_mean
    returns them), origin = (X0, Y0, Z0) the centre of voxel (0, 0, 0) and voxel = (sX, sY, sZ) in metres.  Marching tetrahedra on
    the Kuhn split of every cell whose 8 voxels have W > min_weight; the surface is D = 0 and its triangles are wound so that
    their normals point towards D > 0.  -> dict(vertices [V,3] (X, Y, Z in the field's frame), faces [T,3] int32, weight [V],
    feat [C,V] or None, normal [V,3] = the normalised gradient of D and normal_valid [V] bool (None with normals=False), edge [V]
    int64 = 7 * (owner voxel's linear index) + (edge type): the vertex's identity).  Vertices are shared between triangles and lie
    in the order of edge; V == 0 and T == 0 is a legal result.  A count phase, one read-back of the two totals - the one
    synchronisation with the host, the cost of a result of variable length - and an emit phase; no atomics, the same bits on
    every run.  mesh.extract is the host statement, bit for bit."""
    from . import mesh
    import numpy as np
    for name, t in (("D", D), ("W", W)) + ((("Fm", Fm),) if Fm is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"mesh_field: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    dims, origin, voxel, min_weight, C_ = mesh.check_field("mesh_field", D, W, Fm, origin, voxel, min_weight)
    if not D.is_cuda:
        raise ValueError("mesh_field: the field lives on the GPU; nothing here computes on the CPU (mesh.extract is the host statement)")
    dev = D.device
    for name, t in (("W", W), ("Fm", Fm)):
        if t is not None and t.device != dev:
            raise ValueError(f"mesh_field: {name} is on {t.device}, D on {dev}")
    D, W = D.contiguous(), W.contiguous()
    Fm = torch.empty((0,) + dims, dtype=torch.float32, device=dev) if Fm is None else Fm.contiguous()
    normals = bool(normals)
    origin, voxel = np.array(origin, np.float32), np.array(voxel, np.float32)
    o = ops()
    if o is not None:
        vertices, faces, weight, feat, normal, normal_valid, edge, totals = o.tsdf_mesh(D, W, Fm, torch.from_numpy(origin), torch.from_numpy(voxel),
                                                                                        min_weight, normals)
        mesh.check_totals(int(totals[0]), int(totals[1]))
    else:
        n = D.numel()
        idims = np.array(dims, np.int32)
        nt, mask = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        voff, toff = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        nbytes = lib().be_tsdf_mesh_workspace_bytes(n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        u8, i64 = (torch.uint8,), (torch.int64,)
        check(lib().be_tsdf_mesh_count_f32(dptr(D), dptr(W), _iptr(idims), min_weight, dptr(nt, "nt", u8), dptr(mask, "mask", u8), dptr(voff),
                                           dptr(toff), dptr(totals, "totals", i64), dptr(ws, "workspace", i64), nbytes, stream_ptr(dev)),
              "be_tsdf_mesh_count_f32")
        V, T = mesh.check_totals(*totals.tolist())                      # the read-back: synchronises with the stream
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(T, 3, dtype=torch.int32, device=dev)
        weight = torch.empty(V, dtype=torch.float32, device=dev)
        feat = torch.empty(C_, V, dtype=torch.float32, device=dev)
        edge = torch.empty(V, dtype=torch.int64, device=dev)
        normal = torch.empty(V if normals else 0, 3, dtype=torch.float32, device=dev)
        normal_valid = torch.empty(V if normals else 0, dtype=torch.bool, device=dev)
        if V or T:
            check(lib().be_tsdf_mesh_emit_f32(dptr(D), dptr(W), dptr(Fm if C_ else None), C_, _iptr(idims), _fptr(origin), _fptr(voxel), min_weight,
                                              dptr(nt, "nt", u8), dptr(mask, "mask", u8), dptr(voff), dptr(toff), V, T, dptr(vertices),
                                              dptr(faces), dptr(weight), dptr(feat if C_ else None), dptr(normal if normals else None),
                                              dptr(normal_valid if normals else None, "normal_valid", (torch.bool,)), dptr(edge, "edge", i64),
                                              stream_ptr(dev)), "be_tsdf_mesh_emit_f32")
    return dict(vertices=vertices, faces=faces, weight=weight, feat=feat if C_ else None, normal=normal if normals else None,
                normal_valid=normal_valid if normals else None, edge=edge)


def tsdf_mesh(volume, min_weight=0.0, normals=True):
    """The surface a volume (native.tsdf_volume / tsdf_integrate) holds, as one triangle mesh in the volume's frame: tsdf_mean, then
    mesh_field on the means - a cell takes part when all 8 of its voxels hold a sum of weights > min_weight (0: the ray cast's
    rule), and the volume's C channels ride along as feat [C,V].  mesh.extract_volume is the host statement, bit for bit."""
    _, origin, voxel = _tsdf_state("tsdf_mesh", volume)
    D, W, Fm = tsdf_mean(volume)
    return mesh_field(D, W, Fm if volume.C else None, tuple(origin.tolist()), tuple(voxel.tolist()), min_weight, normals)


def raster_mesh(mesh, cam_dst, pose, size, near=1e-3, cull="none", want=("feat", "normal", "weight", "bary")):
    """A triangle mesh as the camera cam_dst sees it from `pose` (camera.pose: the camera's frame -> the mesh's, as tsdf_raycast
    takes it; None: the identity), size = (Ho, Wo) with 1 <= Ho, Wo <= 16384.  mesh: a dict as mesh_field / tsdf_mesh return it,
    on the GPU: vertices [V,3] float32, faces [T,3] int32, and optionally (absent or None) weight [V], feat [C,V], normal [V,3]
    with normal_valid [V] bool.  A z-buffered rasteriser: vertices are projected and snapped to 1/256 pixel, coverage is exact on
    those integers with the top-left rule (two triangles that share an edge cover each pixel centre on it once), depth is
    interpolated perspective-correctly and the nearest fragment wins, the lowest face index on a tie.  A triangle with a vertex at
    Z <= near in the camera's frame, or further than 2^14 pixels from the image origin, is dropped whole: nothing is clipped.  A
    triangle faces the camera when its winding normal (mesh.py: towards free space) points at it; cull = "back" drops the others,
    "front" those, "none" neither.  -> dict(depth [Ho,Wo] = Z in the camera's frame, face [Ho,Wo] int32 = the triangle seen (-1:
    none), valid (face >= 0; on the device, no sync), and, of `want`, what the mesh holds: weight [Ho,Wo], feat [C,Ho,Wo], normal
    [3,Ho,Wo] in the camera's frame with normal_valid, bary [3,Ho,Wo] = the perspective-correct barycentric coordinates in the
    face's vertex order; None otherwise); +0 / -1 / False where nothing landed.  A face whose index lies outside [0, V) is dropped
    (the statement refuses it; finding it here would cost a read-back).  Three kernels and a memset; order-independent atomics,
    the same bits on every run; nothing synchronises with the host.  raster.render is the host statement, bit for bit."""
    from . import camera, raster, volume as volume_
    V, T, C_ = raster.check_mesh("raster_mesh", mesh)
    Ho, Wo, near, cull, want = raster.check_params("raster_mesh", size, near, cull, want)
    kinds = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32, normal_valid=torch.bool)
    dev = getattr(mesh["vertices"], "device", None)
    m = {}
    for name, dt in kinds.items():
        t = mesh.get(name)
        if t is None:
            m[name] = None
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"raster_mesh: {name} must be a {str(dt).replace('torch.', '')} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if not t.is_cuda:
            raise ValueError("raster_mesh: the mesh lives on the GPU; nothing here computes on the CPU (raster.render is the host statement)")
        if t.device != dev:
            raise ValueError(f"raster_mesh: {name} is on {t.device}, vertices on {dev}")
        m[name] = t.contiguous()
    cd = camera.as_pinhole(cam_dst, "raster_mesh(cam_dst)").f32()
    camera.as_pose(pose, "raster_mesh(pose)")
    q12 = volume_.inverse_pose(pose)
    weight = m["weight"] if "weight" in want else None
    feat = m["feat"] if "feat" in want else None
    normal = m["normal"] if "normal" in want else None
    nvalid = m["normal_valid"] if normal is not None else None
    bary = "bary" in want
    o = ops()
    if o is not None:
        d, face, w, f, nrm, nv, b = o.mesh_raster(m["vertices"], m["faces"], weight, feat, normal, nvalid, torch.from_numpy(cd),
                                                  torch.from_numpy(q12), near, cull, Ho, Wo, bary)
    else:
        new = _new(dev)
        d, face = new(Ho, Wo), new(Ho, Wo, dtype=torch.int32)
        w = new(Ho, Wo) if weight is not None else None
        f = new(C_, Ho, Wo) if feat is not None else None
        nrm, nv = (new(3, Ho, Wo), new(Ho, Wo, dtype=torch.bool)) if normal is not None else (None, None)
        b = new(3, Ho, Wo) if bary else None
        nbytes = lib().be_mesh_raster_workspace_bytes(V, Ho, Wo)
        ws = new((nbytes + 15) // 16, 2, dtype=torch.int64)
        u8 = (torch.bool,)
        check(lib().be_mesh_raster_f32(dptr(m["vertices"]), V, dptr(m["faces"]), T, dptr(weight), dptr(feat if C_ else None), C_, dptr(normal),
                                       dptr(nvalid, "normal_valid", u8), _fptr(cd), _fptr(q12), near, cull, Ho, Wo, dptr(d), dptr(face), dptr(w),
                                       dptr(f if C_ else None), dptr(nrm), dptr(nv, "normal_valid", u8), dptr(b),
                                       dptr(ws, "workspace", (torch.int64,)), nbytes, stream_ptr(dev)), "be_mesh_raster_f32")
    keep = lambda t, has: t if has else None
    return dict(depth=d, face=face, valid=face >= 0, weight=keep(w, weight is not None), feat=keep(f, feat is not None),
                normal=keep(nrm, normal is not None), normal_valid=keep(nv, normal is not None), bary=keep(b, bary))


MESH_KINDS = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32,
                  normal_valid=torch.bool, edge=torch.int64)
_I64, _BOOL = (torch.int64,), (torch.bool,)


def _mesh_on_gpu(who, mesh):
    """A mesh dict for the cleaning entries: components.check_mesh, every member a tensor of its MESH_KINDS dtype on one GPU ->
    (V, T, C, the members contiguous - None for what the mesh does not hold -, the device)."""
    from . import components
    V, T, C_ = components.check_mesh(who, mesh)
    dev = getattr(mesh["vertices"], "device", None)
    m = {}
    for name, dt in MESH_KINDS.items():
        t = mesh.get(name)
        if t is None:
            m[name] = None
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"{who}: {name} must be a {str(dt).replace('torch.', '')} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if not t.is_cuda:
            raise ValueError(f"{who}: the mesh lives on the GPU; nothing here computes on the CPU (be_hip.components is the host statement)")
        if t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, vertices on {dev}")
        m[name] = t.contiguous()
    return V, T, C_, m, dev


def _components_label(m, V, T, dev):
    """-> (label [V], component [V], face_component [T] int32, total [1] int64 on the device = K); no synchronisation."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_components(m["faces"], V))
    new = _new(dev)
    label, component, fc = new(V, dtype=torch.int32), new(V, dtype=torch.int32), new(T, dtype=torch.int32)
    total = new(1, dtype=torch.int64)
    nbytes = lib().be_mesh_components_workspace_bytes(V)
    ws = new((nbytes + 7) // 8, dtype=torch.int64)
    check(lib().be_mesh_components_i32(dptr(m["faces"]), V, T, dptr(label), dptr(component), dptr(fc), dptr(total, "total", _I64),
                                       dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)), "be_mesh_components_i32")
    return label, component, fc, total


def _components_stats(m, V, T, component, Kcap, dev):
    """-> (triangles, vertices int32 [Kcap], area_q int64 [Kcap]) per dense id; 0 from K on."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_components_stats(m["vertices"], m["faces"], component, Kcap))
    new = _new(dev)
    tri, nv, aq = new(Kcap, dtype=torch.int32), new(Kcap, dtype=torch.int32), new(Kcap, dtype=torch.int64)
    check(lib().be_mesh_components_stats(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(component), Kcap, dptr(tri), dptr(nv),
                                         dptr(aq, "area_q", _I64), stream_ptr(dev)), "be_mesh_components_stats")
    return tri, nv, aq


def _components_decide(tri, aq, total, mt, ma, largest, component, dev):
    """-> (keep [Kcap] bool, False from K on, vertex_keep [V] bool = keep[component] or None); K is read on the device."""
    o = ops()
    if o is not None:
        keep, vk = o.mesh_components_decide(tri, aq, total, mt, ma, largest, component)
        return keep, (vk if component is not None else None)
    Kcap, V = tri.numel(), 0 if component is None else component.numel()
    keep = torch.zeros(Kcap, dtype=torch.bool, device=dev)
    vk = None if component is None else torch.empty(V, dtype=torch.bool, device=dev)
    ws = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib().be_mesh_components_decide(dptr(tri), dptr(aq, "area_q", _I64), dptr(total, "total", _I64), Kcap, mt, ma, int(largest),
                                          dptr(keep, "keep", _BOOL), dptr(component), V, dptr(vk, "vertex_keep", _BOOL),
                                          dptr(ws, "workspace", _I64), 8, stream_ptr(dev)), "be_mesh_components_decide")
    return keep, vk


def _select_count(m, V, T, vertex_keep, dev):
    """-> (voff [V], foff [T] int32, totals [2] int64 on the device = (V', T')); no synchronisation."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_select_count(m["faces"], vertex_keep))
    new = _new(dev)
    voff, foff, totals = new(V, dtype=torch.int32), new(T, dtype=torch.int32), new(2, dtype=torch.int64)
    nbytes = lib().be_mesh_select_workspace_bytes(V, T)
    ws = new((nbytes + 7) // 8, dtype=torch.int64)
    check(lib().be_mesh_select_count(dptr(m["faces"]), V, T, dptr(vertex_keep, "vertex_keep", _BOOL), dptr(voff), dptr(foff),
                                     dptr(totals, "totals", _I64), dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)), "be_mesh_select_count")
    return voff, foff, totals


def _select_emit(m, V, T, C_, component, vertex_keep, voff, foff, V2, T2, dev):
    """The emit phase -> the compacted mesh (components.select's keys, and component [V2] when one was given)."""
    has = lambda k: m[k] is not None
    o = ops()
    if o is not None:
        v, f, w, ft, n, nv, e, c, vi, fi = o.mesh_select(m["vertices"], m["faces"], m["weight"], m["feat"], m["normal"], m["normal_valid"], m["edge"],
                                                         component, vertex_keep, voff, foff, V2, T2)
    else:
        new = _new(dev)
        v, f = new(V2, 3), new(T2, 3, dtype=torch.int32)
        w = new(V2) if has("weight") else None
        ft = new(C_, V2) if has("feat") else None
        n = new(V2, 3) if has("normal") else None
        nv = new(V2, dtype=torch.bool) if has("normal_valid") else None
        e = new(V2, dtype=torch.int64) if has("edge") else None
        c = new(V2, dtype=torch.int32) if component is not None else None
        vi, fi = new(V2, dtype=torch.int32), new(T2, dtype=torch.int32)
        check(lib().be_mesh_select_emit(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(m["weight"]), dptr(m["feat"] if C_ else None), C_,
                                        dptr(m["normal"]), dptr(m["normal_valid"], "normal_valid", _BOOL), dptr(m["edge"], "edge", _I64),
                                        dptr(component), dptr(vertex_keep, "vertex_keep", _BOOL), dptr(voff), dptr(foff), V2, T2, dptr(v), dptr(f),
                                        dptr(w), dptr(ft if C_ else None), dptr(n), dptr(nv, "normal_valid", _BOOL), dptr(e, "edge", _I64), dptr(c),
                                        dptr(vi), dptr(fi), stream_ptr(dev)), "be_mesh_select_emit")
    keep = lambda t, k: t if has(k) else None
    out = dict(vertices=v, faces=f, weight=keep(w, "weight"), feat=keep(ft, "feat"), normal=keep(n, "normal"),
               normal_valid=keep(nv, "normal_valid"), edge=keep(e, "edge"), vertex_index=vi, face_index=fi)
    if component is not None:
        out["component"] = c
    return out


def _components_dict(tri, nv, aq, K):
    from . import components
    aq = aq[:K]
    return dict(triangles=tri[:K], vertices=nv[:K], area_q=aq, area=aq.to(torch.float64) * 2.0 ** -components.AREA_BITS)


def mesh_components(mesh):
    """The connected components of a mesh on the GPU (a dict as mesh_field / tsdf_mesh return it: vertices [V,3] float32, faces
    [T,3] int32): two vertices are connected when a chain of faces joins them, one shared vertex being enough.  -> dict(label [V]
    int32 = the least vertex index of the vertex's component, component [V] int32 = its dense id 0..K-1 in increasing order of
    label, face_component [T] int32 (-1: a face with an index outside [0, V), which is ignored - the statement refuses it; finding
    it here would cost a read-back), K (a python int: the one read-back), and per component triangles, vertices int32 [K], area_q
    int64 [K] (2^-40 m^2, summed as integers), area float64 [K] in m^2).  A lock-free union-find (atomicMin links from the larger
    root to the smaller, so a root is its component's least index), the scan for the dense ids, integer atomics for the sizes:
    the same bits on every run.  components.label / stats are the host statement, bit for bit."""
    V, T, _, m, dev = _mesh_on_gpu("mesh_components", mesh)
    label, component, fc, total = _components_label(m, V, T, dev)
    K = int(total.item())                                                # the read-back: synchronises with the stream
    tri, nv, aq = _components_stats(m, V, T, component, K, dev)
    return dict(label=label, component=component, face_component=fc, K=K, **_components_dict(tri, nv, aq, K))


def _vertex_keep(who, vertex_keep, V, dev):
    if not isinstance(vertex_keep, torch.Tensor) or vertex_keep.dtype != torch.bool or tuple(vertex_keep.shape) != (V,):
        raise ValueError(f"{who}: vertex_keep must be a bool tensor [{V}], got {_got(vertex_keep)}")
    if vertex_keep.device != dev:
        raise ValueError(f"{who}: vertex_keep is on {vertex_keep.device}, vertices on {dev}")
    return vertex_keep.contiguous()


def mesh_select(mesh, vertex_keep):
    """The mesh compacted to the vertices vertex_keep [V] bool names: they stay in their order, the faces whose three indices are
    all in range and kept stay in theirs, re-indexed, and every per-vertex array the mesh holds (weight, feat [C,V], normal,
    normal_valid, edge) is gathered; None stays None.  vertex_index [V'] / face_index [T'] int32 give the old positions; V' == 0 and
    T' == 0 are legal.  Two scans, one read-back of (V', T'), one gather.  components.select is the host statement, bit for bit."""
    V, T, C_, m, dev = _mesh_on_gpu("mesh_select", mesh)
    vertex_keep = _vertex_keep("mesh_select", vertex_keep, V, dev)
    voff, foff, totals = _select_count(m, V, T, vertex_keep, dev)
    V2, T2 = totals.tolist()                                            # the read-back: synchronises with the stream
    return _select_emit(m, V, T, C_, None, vertex_keep, voff, foff, V2, T2, dev)


def mesh_clean(mesh, min_triangles=None, min_area=None, largest=False):
    """The mesh without its small components: a component stays when it holds at least min_triangles triangles and min_area square
    metres (None: not asked); largest=True keeps, of those, only the one with the most triangles (the lowest id on a tie).  ->
    mesh_select's result for the vertices of the components that stay, with component [V'] int32 = their OLD dense ids and
    components = dict(triangles, vertices, area_q, area, keep [K] bool) over all K components.  ONE read-back: the per-component
    arrays are sized by V (K <= V) and the decision reads K on the device, so (K, V', T') come back together, after the count
    phase of the selection.  components.clean is the host statement, bit for bit."""
    from . import components
    V, T, C_, m, dev = _mesh_on_gpu("mesh_clean", mesh)
    mt, ma, largest = components.check_decision("mesh_clean", min_triangles, min_area, largest)
    _, component, _, total = _components_label(m, V, T, dev)
    tri, nv, aq = _components_stats(m, V, T, component, V, dev)
    keep, vertex_keep = _components_decide(tri, aq, total, mt, ma, largest, component, dev)
    voff, foff, totals = _select_count(m, V, T, vertex_keep, dev)
    K, V2, T2 = torch.cat([total, totals]).tolist()                     # the read-back: synchronises with the stream
    out = _select_emit(m, V, T, C_, component, vertex_keep, voff, foff, V2, T2, dev)
    out["components"] = dict(_components_dict(tri, nv, aq, K), keep=keep[:K])
    return out


def mesh_decide(stats, K, min_triangles=None, min_area=None, largest=False):
    """keep [K] bool of mesh_components' result (its triangles and area_q) under components.decide's rule, on the GPU."""
    from . import components
    mt, ma, largest = components.check_decision("mesh_decide", min_triangles, min_area, largest)
    tri, aq = stats["triangles"], stats["area_q"]
    if not (isinstance(tri, torch.Tensor) and isinstance(aq, torch.Tensor) and tri.is_cuda and aq.is_cuda and tri.dtype == torch.int32
            and aq.dtype == torch.int64 and tri.shape == aq.shape == (K,)):
        raise ValueError(f"mesh_decide: triangles int32 [{K}] and area_q int64 [{K}] on the GPU, as mesh_components returned them")
    total = torch.full((1,), K, dtype=torch.int64, device=tri.device)
    return _components_decide(tri.contiguous(), aq.contiguous(), total, mt, ma, largest, None, tri.device)[0]


def _simplify_grid(who, cell, origin):
    """simplify.grid's checks -> (cell, origin) as float32 numpy arrays [3], what both bindings hand to the C entry points."""
    from . import simplify
    c, _, o = simplify.grid(cell, origin, who)
    return c, o


def _cluster(m, V, cell, origin, dev):
    """-> (label [V], cluster [V], members [V] int32 (0 from V' on), totals [2] int64 on the device = (V', overflow)); no sync."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_cluster(m["vertices"], m["weight"], torch.from_numpy(cell), torch.from_numpy(origin)))
    new = _new(dev)
    label, cluster, members = (new(V, dtype=torch.int32) for _ in range(3))
    totals = new(2, dtype=torch.int64)
    nbytes = lib().be_mesh_cluster_workspace_bytes(V)
    ws = new((nbytes + 7) // 8, dtype=torch.int64)
    check(lib().be_mesh_cluster_f32(dptr(m["vertices"]), dptr(m["weight"]), V, _fptr(cell), _fptr(origin), dptr(label), dptr(cluster), dptr(members),
                                    dptr(totals, "totals", _I64), dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)), "be_mesh_cluster_f32")
    return label, cluster, members, totals


def _table_overflow(who, overflow):
    if overflow:
        raise RuntimeError(f"{who}: a hash table was exhausted before every key found a slot (its probe loops are bounded and do not spin); "
                           "the result is not to be used")


def mesh_cluster(mesh, cell, origin=(0, 0, 0)):
    """The vertex clusters of a mesh on the GPU (a dict as mesh_field / tsdf_mesh / mesh_clean return it) under the grid of cells of
    `cell` metres - one number or three (cX, cY, cZ) - with a corner of cell (0, 0, 0) at `origin`: the labelling alone of
    mesh_simplify.  -> dict(label [V] int32 = the least index among the usable vertices of the vertex's cell, cluster [V] int32 =
    the cell's dense id 0..V'-1 in increasing order of label, members [V'] int32, V (a python int: V', the one read-back)); -1 for
    an unusable vertex (a position that is not finite or lies 2^20 cells or more from the origin, a weight whose quantised
    value is 0).  A hash table of vertex indices (atomicCAS on an empty slot, atomicMin on an equal cell; every probe loop is
    bounded), the scan for the dense ids: the same bits on every run.  simplify.cluster is the host statement, bit for bit."""
    V, _, _, m, dev = _mesh_on_gpu("mesh_cluster", mesh)
    cell, origin = _simplify_grid("mesh_cluster", cell, origin)
    label, cluster, members, totals = _cluster(m, V, cell, origin, dev)
    V2, overflow = totals.tolist()                                      # the read-back: synchronises with the stream
    _table_overflow("mesh_cluster", overflow)
    return dict(label=label, cluster=cluster, members=members[:V2], V=V2)


def mesh_simplify(mesh, cell, origin=(0, 0, 0), flaps=False):
    """The mesh made coarser by vertex clustering: every vertex falls into a cell of the grid mesh_cluster describes, every occupied
    cell becomes ONE vertex at the weighted mean of its members (weights quantised as fuse_views quantises them, positions as 2^-24
    of a cell, every sum an integer), and every face is re-indexed; a face with two corners in one cell, or with an unusable
    corner, is dropped, of the faces that name the same three cells in the same winding the least index stays, and with
    flaps=False three cells named in BOTH windings lose all their faces (back-to-back flaps of zero volume; flaps=True keeps the
    least face of each winding).  -> the mesh with components.select's keys but vertex_index (vertices [V',3], faces [T',3] int32 in
    their old order and corner order, weight [V'] = the mean weight, feat [C,V'], normal [V',3] = the normalised mean over the
    members with a valid normal, normal_valid [V'], each None where the mesh holds none; edge = None: an edge id does not survive),
    and cluster [V] int32 (the new id of every old vertex, -1: unusable), members [V'] int32, face_index [T'] int32 (the old
    positions).  V' == 0 and T' == 0 are legal.  Two hash tables (bounded probe loops, no thread waits for another), integer
    atomics, a count phase, ONE read-back of (V', T') and an emit phase: the same bits on every run.  simplify.simplify is the
    host statement, bit for bit; a face index outside [0, V), which it refuses, is ignored here (finding it would cost a read-back)."""
    V, T, C_, m, dev = _mesh_on_gpu("mesh_simplify", mesh)
    cell, origin = _simplify_grid("mesh_simplify", cell, origin)
    flaps = bool(flaps)
    has = lambda k: m[k] is not None
    normals = has("normal")
    label, cluster, members, totals_v = _cluster(m, V, cell, origin, dev)
    o = ops()
    new = _new(dev)
    if o is not None:
        tc, to = torch.from_numpy(cell), torch.from_numpy(origin)
        sums, fflag, foff, totals_f = o.mesh_simplify_count(m["vertices"], m["faces"], m["weight"], m["feat"], m["normal"], m["normal_valid"], tc, to,
                                                            cluster, flaps)
    else:
        rows = lib().be_mesh_simplify_sum_rows(C_, int(normals))
        sums, fflag, foff = new(rows, V, dtype=torch.int64), new(T, dtype=torch.uint8), new(T, dtype=torch.int32)
        totals_f = new(2, dtype=torch.int64)
        nbytes = lib().be_mesh_simplify_workspace_bytes(T)
        ws = new((nbytes + 7) // 8, dtype=torch.int64)
        check(lib().be_mesh_simplify_count(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(m["weight"]), dptr(m["feat"] if C_ else None), C_,
                                           dptr(m["normal"]), dptr(m["normal_valid"], "normal_valid", _BOOL), _fptr(cell), _fptr(origin), dptr(cluster),
                                           int(flaps), dptr(sums, "sums", _I64), dptr(fflag, "fflag", (torch.uint8,)), dptr(foff),
                                           dptr(totals_f, "totals", _I64), dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)),
              "be_mesh_simplify_count")
    V2, over_v, T2, over_f = torch.cat([totals_v, totals_f]).tolist()   # the read-back: synchronises with the stream
    _table_overflow("mesh_simplify", over_v or over_f)
    if o is not None:
        v, f, w, ft, n, nv, fi = o.mesh_simplify(m["vertices"], m["faces"], tc, to, label, cluster, members, sums, C_, normals, has("weight"), fflag,
                                                 foff, V2, T2)
    else:
        v, f, fi = new(V2, 3), new(T2, 3, dtype=torch.int32), new(T2, dtype=torch.int32)
        w = new(V2) if has("weight") else None
        ft = new(C_, V2)
        n, nv = (new(V2, 3), new(V2, dtype=torch.bool)) if normals else (None, None)
        check(lib().be_mesh_simplify_emit(dptr(m["vertices"]), dptr(m["faces"]), V, T, _fptr(cell), _fptr(origin), dptr(label), dptr(cluster),
                                          dptr(members), dptr(sums, "sums", _I64), C_, int(normals), dptr(fflag, "fflag", (torch.uint8,)), dptr(foff),
                                          V2, T2, dptr(v), dptr(f), dptr(w), dptr(ft if C_ else None), dptr(n), dptr(nv, "normal_valid", _BOOL),
                                          dptr(fi), stream_ptr(dev)), "be_mesh_simplify_emit")
    return dict(vertices=v, faces=f, weight=w if has("weight") else None, feat=ft if has("feat") else None, normal=n if normals else None,
                normal_valid=nv if normals else None, edge=None, cluster=cluster, members=members[:V2], face_index=fi)


def _smooth_workspace(V, T, dev):
    nbytes = lib().be_mesh_smooth_workspace_bytes(V, T)
    return _new(dev)((nbytes + 7) // 8, dtype=torch.int64), nbytes


def _adjacency(m, V, T, dev):
    """-> (valence [V] int32, boundary [V] bool); no synchronisation."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_adjacency(m["vertices"], m["faces"]))
    new = _new(dev)
    valence, boundary = new(V, dtype=torch.int32), new(V, dtype=torch.bool)
    ws, nbytes = _smooth_workspace(V, T, dev)
    check(lib().be_mesh_adjacency_f32(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(valence), dptr(boundary, "boundary", _BOOL),
                                      dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)), "be_mesh_adjacency_f32")
    return valence, boundary


def _normals(vertices, faces, V, T, dev):
    """-> (normal [V,3], normal_valid [V] bool); no synchronisation."""
    o = ops()
    if o is not None:
        return tuple(o.mesh_normals(vertices, faces))
    new = _new(dev)
    normal, valid = new(V, 3), new(V, dtype=torch.bool)
    ws, nbytes = _smooth_workspace(V, T, dev)
    check(lib().be_mesh_normals_f32(dptr(vertices), dptr(faces), V, T, dptr(normal), dptr(valid, "normal_valid", _BOOL), dptr(ws, "workspace", _I64),
                                    nbytes, stream_ptr(dev)), "be_mesh_normals_f32")
    return normal, valid


def mesh_adjacency(mesh):
    """What mesh_smooth knows of a mesh on the GPU (a dict as mesh_field / tsdf_mesh / mesh_clean / mesh_simplify return it) before
    it moves a vertex -> dict(valence [V] int32 = the usable faces at the vertex, boundary [V] bool = the vertex touches an edge
    that exactly one usable face holds).  A vertex is usable when its coordinates are finite and below 2^16 m in size, a face when
    its indices are in range, pairwise distinct and name usable vertices; a face given twice counts twice.  An edge table of
    64-bit keys that cannot overflow; no read-back.  smooth.adjacency is the host statement, bit for bit; a face index outside
    [0, V), which it refuses, is ignored here."""
    V, T, _, m, dev = _mesh_on_gpu("mesh_adjacency", mesh)
    valence, boundary = _adjacency(m, V, T, dev)
    return dict(valence=valence, boundary=boundary)


def mesh_normals(mesh):
    """Area-weighted vertex normals of a mesh on the GPU from its faces alone -> dict(normal [V,3], normal_valid [V] bool): per
    usable face cross(b - a, c - a) in float32, quantised to 2^-40 m^2, summed per vertex in int64, normalised in float32; +0 and
    False where the sum has no direction.  The winding normal points to free space, as extract_mesh winds its faces.
    smooth.vertex_normals is the host statement, bit for bit; no read-back."""
    V, T, _, m, dev = _mesh_on_gpu("mesh_normals", mesh)
    normal, valid = _normals(m["vertices"], m["faces"], V, T, dev)
    return dict(normal=normal, normal_valid=valid)


def mesh_smooth(mesh, iters=10, lam=0.5, mu=-0.53, boundary="fixed", normals="keep"):
    """The mesh denoised at its own resolution by Taubin's lambda | mu smoothing: per iteration every movable vertex steps towards the
    mean of its neighbours by lam, then away from the new mean by mu (mu = 0: a plain Laplacian, which shrinks).  boundary="fixed"
    holds the vertices mesh_adjacency calls boundary, "free" moves them too.  Positions are integers of 2^-30 m and a neighbour sum
    is an integer sum, so the result has the same bits on every run.  -> the mesh's keys (faces, weight, feat the tensors given;
    edge = None: a moved vertex has left its lattice edge; normals="keep" passes normal / normal_valid through, "recompute"
    replaces them by mesh_normals of the result, "drop" gives None) and valence [V] int32, boundary [V] bool, displacement [V] =
    how far each vertex moved.  No vertex or face is lost; iters=0 returns the positions bit for bit.  One launch per step, no
    atomics in it, no read-back.  smooth.smooth is the host statement, bit for bit; a face index outside [0, V), which it refuses,
    is ignored here."""
    from . import smooth
    V, T, _, m, dev = _mesh_on_gpu("mesh_smooth", mesh)
    iters, lam, mu, free, normals = smooth.check_args("mesh_smooth", iters, lam, mu, boundary, normals)
    o = ops()
    if o is not None:
        v, disp, valence, bnd = o.mesh_smooth(m["vertices"], m["faces"], iters, lam, mu, free)
    else:
        new = _new(dev)
        v, disp, valence, bnd = new(V, 3), new(V), new(V, dtype=torch.int32), new(V, dtype=torch.bool)
        ws, nbytes = _smooth_workspace(V, T, dev)
        check(lib().be_mesh_smooth_f32(dptr(m["vertices"]), dptr(m["faces"]), V, T, iters, lam, mu, int(free), dptr(v), dptr(disp), dptr(valence),
                                       dptr(bnd, "boundary", _BOOL), dptr(ws, "workspace", _I64), nbytes, stream_ptr(dev)), "be_mesh_smooth_f32")
    out = dict(vertices=v, faces=m["faces"], weight=m["weight"], feat=m["feat"], normal=None, normal_valid=None, edge=None, valence=valence,
               boundary=bnd, displacement=disp)
    if normals == "keep":
        out.update(normal=m["normal"], normal_valid=m["normal_valid"])
    elif normals == "recompute":
        out["normal"], out["normal_valid"] = _normals(v, m["faces"], V, T, dev)
    return out


def depth_normals(depth, cam, step=3, max_jump=0.05, scale=1, window_origin=(0, 0)):
    """Surface normals of a depth map: depth [H,W] (float32 on the GPU, the samples of unproject on the lattice (scale,
    window_origin) of `cam`) -> dict(normal [3,H,W] = the unit normal (X, Y, Z) of the surface through each sample, facing the
    camera (n . P <= 0), valid [H,W] = normal non-zero (on the device, no sync)).  The normal is the cross product of the
    differences of the unprojected samples `step` apart along x and along y - central where both neighbours are inside the image,
    hold a finite depth > 0 and lie within max_jump * step metres of the sample's depth, one-sided where one does - so that no
    normal spans an occlusion step; (+0, +0, +0) where a direction has no such neighbour.  step > 1 trades resolution for noise.
    registration.normals_f32 is the host statement, bit for bit."""
    from . import registration
    step, max_jump = registration.check_normals_params("depth_normals", step, max_jump)
    depth, (cs,), _, top, left = _reproject_args("depth_normals", depth, [("cam", cam)], None, scale, window_origin)
    H, W = depth.shape
    o = ops()
    if o is not None:
        normal = o.depth_normals(depth, torch.from_numpy(cs), step, max_jump, scale, top, left)
    else:
        normal = torch.empty(3, H, W, dtype=torch.float32, device=depth.device)
        check(lib().be_depth_normals_f32(dptr(depth, "depth", (torch.float32,)), H, W, scale, top, left, _fptr(cs), step, max_jump,
                                         dptr(normal), stream_ptr(depth.device)), "be_depth_normals_f32")
    return dict(normal=normal, valid=(normal != 0).any(0))


ICP_VIEW_KEYS = ("depth", "weight", "cam", "scale", "window_origin")


def icp_linearize(src, dst, normal_d, pose, near=1e-3, max_dist=0.1, huber=0.0, rows=False):
    """The linearised point-to-plane step of a depth registration at `pose` (source frame -> target frame; None: the identity).
    src, dst: dicts with the keys depth [H,W] (float32 on the GPU), weight [H,W] or None (1 everywhere), cam, scale and
    window_origin (as reproject; the target's samples are the pixels of its camera: scale 1, origin (0, 0)); normal_d [3,Hd,Wd]:
    the target's normals (depth_normals).  Every source sample is projected as reproject projects it; one that lands on a target
    pixel with a finite depth > 0 and a non-zero normal, within max_dist (metres) of that pixel's point and with a weight product
    in (0, inf), contributes its residual r = n . (P - Q) and its row J = (P x n, n), with its weight scaled by huber / |r| where
    huber > 0 and |r| > huber.  -> dict(sums = float64 [32] on the device: the 21 sums w J[a] J[b] (a <= b), the 6 sums
    w J[a] r, sum w r r, sum w, the number of samples, 0, 0; rows = float32 [8,Hs*Ws] (J, r, w per sample, 0 where it took no
    part) when rows is true, else None).  The sums are double, added in an order that depends on the number of samples alone: no
    floating-point atomics, the same bits on every run, stream and device.  Nothing synchronises with the host.
    registration.linearize is the host statement, bit for bit."""
    from . import camera, registration
    near, max_dist, huber = registration.check_linearize_params("icp_linearize", near, max_dist, huber)
    ds, ws, _, cs, _, scale, top, left = _view("icp_linearize(src)", src, ICP_VIEW_KEYS, "cam")
    dev = ds.device
    dd, wd, _, cd, _, dscale, dtop, dleft = _view("icp_linearize(dst)", dst, ICP_VIEW_KEYS, "cam", dev, "the source's")
    if dscale != 1 or (dtop, dleft) != (0, 0):
        raise ValueError("icp_linearize(dst): the target's samples are the pixels of its camera: scale must be 1 and window_origin (0, 0)")
    Hs, Ws = ds.shape
    Hd, Wd = dd.shape
    normal_d = _channels("icp_linearize", "normal_d", normal_d, dd, C=3, required=True).view(3, Hd, Wd)
    p12 = camera.as_pose(pose, "icp_linearize(pose)")
    rows = bool(rows)
    o = ops()
    if o is not None:
        sums, r = o.icp_linearize(ds, ws, torch.from_numpy(cs), scale, top, left, dd, normal_d, wd, torch.from_numpy(cd),
                                  torch.from_numpy(p12), near, max_dist, huber, rows)
        r = r if rows else None
    else:
        scratch = torch.empty(lib().be_icp_scratch_bytes(Hs, Ws) // 8, dtype=torch.float64, device=dev)
        sums = torch.empty(32, dtype=torch.float64, device=dev)
        r = torch.empty(8, Hs * Ws, dtype=torch.float32, device=dev) if rows else None
        f64 = (torch.float64,)
        check(lib().be_icp_linearize_f32(dptr(ds, "depth", (torch.float32,)), dptr(ws), Hs, Ws, scale, top, left, _fptr(cs),
                                         dptr(dd, "depth", (torch.float32,)), dptr(normal_d), dptr(wd), Hd, Wd, _fptr(cd), _fptr(p12), near,
                                         max_dist, huber, dptr(scratch, "scratch", f64), dptr(sums, "sums", f64), dptr(r), stream_ptr(dev)),
              "be_icp_linearize_f32")
    return dict(sums=sums, rows=r)


def register_depth(src, dst, pose0=None, **kw):
    """The pose of the source view in the target view's frame by point-to-plane ICP on their depth maps.  src, dst: the view
    dicts of icp_linearize; pose0: the start (None: the identity); kw: the keywords of registration.register - iters=20,
    damping=1e-6, max_dist=0.1, huber=0.0, step=3, max_jump=0.05, near=1e-3, tol=1e-9.  -> the dict of registration.register:
    pose (12 float32 numbers: X' = R X + t from the source frame to the target's - what fuse takes), poses, rms, count, A, cond,
    cov, converged, iters.  The loop, the 6 x 6 solve and the composition are registration.register itself, in float64 on the
    host, with depth_normals (once) and icp_linearize (once per iteration) in place of the numpy statements: each iteration
    copies 32 doubles to the host, one synchronisation per iteration.  The sums equal the statement's bit for bit, so the
    iterates equal registration.register's bit for bit."""
    from . import registration
    unknown = [k for k in kw if k not in ("iters", "damping", "max_dist", "huber", "step", "max_jump", "near", "tol")]
    if unknown:
        raise ValueError(f"register_depth: unknown keywords {unknown}")
    _view("register_depth(src)", src, ICP_VIEW_KEYS, "cam")
    _view("register_depth(dst)", dst, ICP_VIEW_KEYS, "cam", src["depth"].device, "the source's")

    def normals(depth, cam, step, max_jump):
        return depth_normals(depth, cam, step=step, max_jump=max_jump)["normal"]

    def linearize(s, d, pose12, near, max_dist, huber):
        view = {k: v for k, v in d.items() if k != "normal"}
        return icp_linearize(s, view, d["normal"], pose12, near=near, max_dist=max_dist, huber=huber)["sums"].cpu().numpy()

    return registration.register(src, dst, pose0, linearize=linearize, normals=normals, who="register_depth", **kw)


FUSE_MAX_CHANNELS = 64
FILL_MAX_SIDE, FILL_MAX_SMOOTH = 16384, 8


def _fill_args(who, statement, depth, weight, edge, smooth, sigma_z):
    """What fill_nearest and fill_diffuse take alike, checked in the order both state it: depth [H,W] on the GPU with H, W <=
    FILL_MAX_SIDE, weight (float32, or a bool mask) and edge (fill_diffuse's; None otherwise) [H,W] or None, smooth in 0..8, sigma_z
    -> (depth, weight, edge - contiguous float32 -, smooth, sigma_z as a float)."""
    from . import camera
    H, W = _depth_map(who, depth, statement, "[H,W]").shape
    if H > FILL_MAX_SIDE or W > FILL_MAX_SIDE:
        raise ValueError(f"{who}: H and W must be at most {FILL_MAX_SIDE} (squared distances are int32), got {H} x {W}")
    weight = _map_like(who, "weight", weight, depth, (torch.float32, torch.bool), "a float32 (or bool: a mask)")
    edge = _map_like(who, "edge", edge, depth)
    if isinstance(smooth, bool) or not isinstance(smooth, int) or not 0 <= smooth <= FILL_MAX_SMOOTH:
        raise ValueError(f"{who}: smooth must be an integer in [0, {FILL_MAX_SMOOTH}], got {smooth!r}")
    return depth.contiguous(), weight, edge, smooth, camera.check_number(who, "sigma_z", sigma_z, lo_open=True)


def fill_nearest(depth, weight=None, smooth=2, sigma_z=0.02, fuse=True):
    """Dense depth from sparse samples: depth [H,W] float32 on the GPU, weight [H,W] (None: 1 everywhere).  A pixel is a seed iff
    its weight is > 0 and its depth a finite number > 0; every other pixel takes the depth of the seed jump flooding assigns it -
    the nearest seed on almost every pixel, a near-nearest one on the rest (fill.nearest_seed; ties to the lower index).
    smooth = r in 0..8: 0 copies the seed's depth, r > 0 takes the robust mean of the seeds within r of it, weighted
    w / (1 + ((z - z_seed) / sigma_z)^2).  -> dict(depth [H,W]: the input at seeds, the filled depth at holes; index [H,W] int32:
    the seed's linear index y * W + x; dist2 [H,W] int32: the squared distance to it); 0 / -1 / -1 everywhere when there is no
    seed.  fuse: run the last passes (steps <= 8) as one launch over LDS tiles - the same integers either way.  The result is a
    function of the inputs alone; fill.fill_nearest_f32 is the host statement, bit for bit.  General: with depth=out["depth"],
    weight=out["valid"] (a bool mask counts as weights 1 / 0) it closes the holes of a reproject result."""
    depth, weight, _, smooth, sigma_z = _fill_args("fill_nearest", "fill.fill_nearest_f32", depth, weight, None, smooth, sigma_z)
    H, W = depth.shape
    fuse = bool(fuse)
    o = ops()
    if o is not None:
        d, index, dist2 = o.fill_nearest(depth, weight, smooth, sigma_z, fuse)
    else:
        dev = depth.device
        new = _new(dev)
        scratch = new(3 if smooth > 0 else 2, H, W, dtype=torch.int32)
        d, index, dist2 = new(H, W), new(H, W, dtype=torch.int32), new(H, W, dtype=torch.int32)
        check(lib().be_fill_nearest_f32(dptr(depth, "depth", (torch.float32,)), dptr(weight), H, W, smooth, sigma_z, int(fuse),
                                        dptr(scratch, "scratch", (torch.int32,)), dptr(d), dptr(index, "index", (torch.int32,)),
                                        dptr(dist2, "dist2", (torch.int32,)), stream_ptr(dev)), "be_fill_nearest_f32")
    return dict(depth=d, index=index, dist2=dist2)


FILL_MAX_ITERS = 4096


def fill_diffuse(depth, weight=None, edge=None, smooth=2, sigma_z=0.02, leak=1e-3, iters=None, fuse=True):
    """Dense depth from sparse samples by edge-aware diffusion: depth [H,W] float32 on the GPU, weight [H,W] (None: 1 everywhere),
    edge [H,W] float32 (None: 0 everywhere).  The seeds are fill_nearest's; a seed's boundary value is what fill_nearest copies from
    it (its depth at smooth = 0, the robust mean of the seeds within r of it at smooth = r > 0).  Every hole takes the harmonic
    interpolant of the boundary values under the conductances c_pq = max(leak, 1 - max(e_p, e_q)), e = edge clamped to [0, 1] (NaN
    counts as 0), between 4-neighbours, with no term across the image border: a surface between two samples comes out as the plane
    through them where fill_nearest puts a step, and an edge of 1 keeps two regions from mixing (leak > 0 keeps the system
    connected).  -> dict(depth [H,W]: the input at seeds, the interpolant at holes; index, dist2 [H,W] int32: fill_nearest's, bit
    for bit; residual [1] float32 on the GPU: max over the holes of |avg - u| after the last sweep); 0 / -1 / -1 / 0 when there is
    no seed.  iters None: the default schedule (4 x the longer side sweeps on every pyramid level), an int in 1..4096: that many
    sweeps per level.  fuse False runs one sweep per launch (the baseline tools/bench_diffuse.py times).  The schedule depends on
    (H, W, iters) alone; nothing synchronises with the host; repeated calls give the same bits.  diffuse.fill_diffuse is the host
    statement (close, not bit-equal: the kernels contract to FMA), diffuse.solve_exact the float64 direct solve."""
    from . import camera
    depth, weight, edge, smooth, sigma_z = _fill_args("fill_diffuse", "diffuse.fill_diffuse", depth, weight, edge, smooth, sigma_z)
    H, W = depth.shape
    leak = camera.check_number("fill_diffuse", "leak", leak, lo_open=True, hi=1, hi_closed=True)
    if iters is not None and (isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= FILL_MAX_ITERS):
        raise ValueError(f"fill_diffuse: iters must be None or an integer in [1, {FILL_MAX_ITERS}], got {iters!r}")
    iters = 0 if iters is None else iters
    fuse = bool(fuse)
    o = ops()
    if o is not None:
        d, index, dist2, residual = o.fill_diffuse(depth, weight, edge, smooth, sigma_z, leak, iters, fuse)
    else:
        dev = depth.device
        new = _new(dev)
        scratch = new(lib().be_fill_diffuse_scratch_bytes(H, W) // 4, dtype=torch.int32)
        d, index, dist2, residual = new(H, W), new(H, W, dtype=torch.int32), new(H, W, dtype=torch.int32), new(1)
        check(lib().be_fill_diffuse_f32(dptr(depth, "depth", (torch.float32,)), dptr(weight), dptr(edge), H, W, smooth, sigma_z, leak, iters,
                                        int(fuse), dptr(scratch, "scratch", (torch.int32,)), dptr(d), dptr(index, "index", (torch.int32,)),
                                        dptr(dist2, "dist2", (torch.int32,)), dptr(residual), stream_ptr(dev)), "be_fill_diffuse_f32")
    return dict(depth=d, index=index, dist2=dist2, residual=residual)


def unfold_patches(img: torch.Tensor, stride: int = 2) -> torch.Tensor:
    """img [B,C,H,W] -> [B, Hp*Wp, C, 21, 21]."""
    b, c, h, w = img.shape
    hp, wp = (h - BE_R) // stride + 1, (w - BE_R) // stride + 1
    out = torch.empty(b, hp * wp, c, BE_R, BE_R, dtype=torch.float32, device=img.device)
    check(lib().be_unfold_patches_f32(dptr(img, "img"), dptr(out), b, c, h, w, stride, stream_ptr(img.device)),
          "be_unfold_patches_f32")
    return out


def local_features(params10: torch.Tensor, colors: torch.Tensor) -> torch.Tensor:
    """params10 [2,P,10] (or [2P,10]) + colors [2,P,3,3] (or [2P,3,3]) -> pm [P,38]."""
    p = params10.numel() // 20
    pm = torch.empty(p, 38, dtype=torch.float32, device=params10.device)
    check(lib().be_local_features_f32(dptr(params10, "params10"), dptr(colors, "colors"), dptr(pm), p,
                                      stream_ptr(params10.device)), "be_local_features_f32")
    return pm


def global_denorm(y: torch.Tensor) -> torch.Tensor:
    """y [P,12] -> est [P,12]."""
    y = y.contiguous()
    est = torch.empty_like(y)
    check(lib().be_global_denorm_f32(dptr(y, "y"), dptr(est), y.numel() // 12, stream_ptr(y.device)), "be_global_denorm_f32")
    return est


def local_loss(opts, est, img_fit, gt, bdist, deri, beta_bndry, beta_smooth, want_grad=True, want=()):
    """-> (partial [B,3], grad_est [B,10] or None, extras {'patches','boundary'})."""
    b = est.shape[0]
    if tuple(est.shape) != (b, 10) or tuple(img_fit.shape) != (b, BE_R, BE_R, 3) or tuple(gt.shape) != (b, BE_R, BE_R, 3) \
            or tuple(bdist.shape) != (b, BE_R, BE_R) or tuple(deri.shape) != (b, 19, 19, 3):
        raise RuntimeError("local_loss: bad shapes (est [B,10], img/gt [B,21,21,3], bdist [B,21,21], deri [B,19,19,3])")
    dev = est.device
    o = ops() if not want else None
    if o is not None:
        partial, grad = o.local_loss(struct_tensor(opts), est, img_fit, gt, bdist, deri, float(beta_bndry), float(beta_smooth), bool(want_grad))
        return partial, (grad if want_grad else None), {}
    partial = torch.empty(b, 3, dtype=torch.float32, device=dev)
    grad = torch.empty(b, 10, dtype=torch.float32, device=dev) if want_grad else None
    shapes = dict(patches=(b, 3, BE_R, BE_R), boundary=(b, BE_R, BE_R))
    extra = {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in want}
    check(lib().be_local_loss_f32(C.byref(opts), dptr(est, "est"), dptr(img_fit, "img_fit"), dptr(gt, "gt"),
                                  dptr(bdist, "bdist"), dptr(deri, "deri"), float(beta_bndry), float(beta_smooth),
                                  dptr(partial), dptr(grad), dptr(extra.get("patches")), dptr(extra.get("boundary")), b,
                                  stream_ptr(dev)), "be_local_loss_f32")
    return partial, grad, extra


# ---------------------------------------------------------------------------------------------- GlobalStage pieces

def local_loss_finish(partial, beta_bndry, beta_smooth):
    """partial [B,3] of local_loss -> the scalar loss (0-dim tensor): S0/(441 B) + beta_b S1/(441 B) + beta_s S2/(361 B)."""
    o = ops()
    if o is not None:
        return o.local_loss_finish(partial, float(beta_bndry), float(beta_smooth))[0]
    out = torch.empty(1, dtype=torch.float32, device=partial.device)
    check(lib().be_local_loss_finish_f32(dptr(partial, "partial"), partial.shape[0], float(beta_bndry), float(beta_smooth), dptr(out),
                                         stream_ptr(partial.device)), "be_local_loss_finish_f32")
    return out[0]


def linear(x2d, pw, pb, cout, act=0, residual=None):
    """x2d [T, Cin] (Cin % 32 == 0) -> [T, cout] on the implicit-GEMM kernel (a Linear is a 1x1 conv on a 1x1 image)."""
    t, cin = x2d.shape
    y = conv_nhwc(x2d.view(t, 1, 1, cin), pw, pb, cout, 1, act, residual=residual)
    return y.view(t, cout)


def attention(qkv, B, L, H, workspace=None, l_valid=None):
    """qkv [B*L, 3*H*16] -> [B*L, H*16].  l_valid: real tokens per sequence when L is padded to a multiple of 128."""
    dev = qkv.device
    o = ops()
    if o is not None:
        return o.attention(qkv, B, L, L if l_valid is None else int(l_valid), H, workspace)
    need = lib().be_attention_workspace_floats(B, L, H)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.float32, device=dev)
    out = torch.empty(B * L, H * 16, dtype=torch.float32, device=dev)
    check(lib().be_attention_f32(dptr(qkv, "qkv"), dptr(out), dptr(workspace), B, L, L if l_valid is None else int(l_valid), H,
                                 stream_ptr(dev)), "be_attention_f32")
    return out, workspace


def add_layernorm(x, res, gamma, beta, eps=1e-5, out=None):
    rows, d = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().be_add_layernorm_f32(dptr(x, "x"), dptr(res), dptr(gamma), dptr(beta), dptr(out), rows, d, eps,
                                     stream_ptr(x.device)), "be_add_layernorm_f32")
    return out


def add_pe_(x, pe, batches):
    check(lib().be_add_pe_f32(dptr(x, "x"), dptr(pe, "pe"), batches, x.numel() // batches, stream_ptr(x.device)), "be_add_pe_f32")
    return x


# ---------------------------------------------------------------------------------------------- global-stage training

def view_image_pair_nhwc(img: torch.Tensor, stride: int = 2) -> PatchView:
    """img [2,H,W,3] channels-last (the dataset layout of data/dataset.py:52) -> gather-on-read patch view."""
    if img.dim() != 4 or img.shape[0] != 2 or img.shape[3] != 3:
        raise RuntimeError(f"view_image_pair_nhwc: expected [2,H,W,3], got {tuple(img.shape)}")
    dptr(img, "img")
    _, h, w, _ = img.shape
    return PatchView(img.data_ptr(), h * w * 3, 1, w * 3, 3, stride * w * 3, stride * 3, (w - BE_R) // stride + 1)


def global_loss(opts, consts, est, img_fit, img_gt, G, Gd, Gb, bdist, deri, bdepth, gamma6, hp, wp, stride=2):
    """-> (partial [B*P,8], grad [B*P,12], grad_depth [B*P,4])."""
    B, P = est.shape[0], est.shape[1]
    H, W = img_gt.shape[2], img_gt.shape[3]
    dev = est.device
    o = ops()
    if o is not None:
        return o.global_loss(struct_tensor(opts), struct_tensor(consts), est, img_fit, img_gt, G, Gd, Gb, bdist, deri, bdepth,
                             [float(v) for v in gamma6], hp, wp, stride)
    partial = torch.empty(B * P, 8, dtype=torch.float32, device=dev)
    grad = torch.empty(B * P, 12, dtype=torch.float32, device=dev)
    gdep = torch.empty(B * P, 4, dtype=torch.float32, device=dev)
    g6 = (C.c_float * 6)(*[float(v) for v in gamma6])
    check(lib().be_global_loss_f32(C.byref(opts), C.byref(consts), dptr(est, "est"), dptr(img_fit, "img_fit"),
                                   dptr(img_gt, "img_gt"), dptr(G, "G"), dptr(Gd, "Gderi"), dptr(Gb, "Gbndry"),
                                   dptr(bdist, "bdist"), dptr(deri, "deri"), dptr(bdepth, "bdepth"), g6, dptr(partial),
                                   dptr(grad), dptr(gdep), B, hp, wp, H, W, stride, stream_ptr(dev)), "be_global_loss_f32")
    return partial, grad, gdep


def conv_pack_fused2(w, b, bn, w2, b2, bn2, eps=1e-5):
    """conv kxk (w,b,bn) + 1x1 branch (w2,b2,bn2) packed for conv_nhwc_fused2 -> (pw, pb)."""
    cout, cin = w.shape[0], w.shape[1]
    ks = w.shape[2]
    cin2 = w2.shape[1]
    nfl = lib().be_conv_fused2_packed_floats(cout, cin, ks, cin2)
    if nfl == 0:
        raise RuntimeError("conv_pack_fused2: unsupported shapes")
    dev = w.device
    pw = torch.empty(nfl, dtype=torch.float32, device=dev)
    pb = torch.empty((cout + 31) // 32 * 32, dtype=torch.float32, device=dev)
    g, g2 = (bn or (None,) * 4), (bn2 or (None,) * 4)
    check(lib().be_conv_pack_fused2_f32(dptr(w.contiguous()), dptr(b), dptr(g[0]), dptr(g[1]), dptr(g[2]), dptr(g[3]),
                                        dptr(w2.contiguous()), dptr(b2), dptr(g2[0]), dptr(g2[1]), dptr(g2[2]), dptr(g2[3]),
                                        eps, cout, cin, ks, cin2, dptr(pw), dptr(pb), stream_ptr(dev)),
          "be_conv_pack_fused2_f32")
    return pw, pb


def conv_nhwc_fused2(x, x2, pw, pb, cout, ksize, act, out=None):
    """y = act(conv_kxk(x) + conv_1x1(x2) + bias): x [N,H,W,Cin], x2 [N,H,W,Cin2]; out = a [N,H,W,ld] tensor whose first cout
    channels receive the result, as in conv_nhwc."""
    n, h, w, cin = x.shape
    y = torch.empty(n, h, w, cout, dtype=torch.float32, device=x.device) if out is None else out
    d = ConvDesc(n, h, w, cin, cout, ksize, int(act))
    check(lib().be_conv_nhwc_fused2_f32(C.byref(d), dptr(x, "x"), dptr(x2, "x2"), x2.shape[-1], dptr(pw), dptr(pb), dptr(y),
                                        y.shape[-1], stream_ptr(x.device)), "be_conv_nhwc_fused2_f32")
    return y


def graph_node_counts(graph) -> dict:
    """Node census of a captured torch.cuda.CUDAGraph built with keep_graph=True: {'nodes': all, 'kernels': kernel nodes,
    'memcpy': .., 'memset': ..} read with hipGraphGetNodes / hipGraphNodeGetType (measurement plumbing: the launch count of a
    replayed training step is not visible from the host otherwise)."""
    hip = C.CDLL("libamdhip64.so")
    raw = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (C.c_void_p * max(1, n.value))()
    if hip.hipGraphGetNodes(raw, nodes, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    kinds = {}
    for i in range(n.value):
        t = C.c_int(-1)
        hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t))
        kinds[t.value] = kinds.get(t.value, 0) + 1
    return dict(nodes=n.value, kernels=kinds.get(0, 0), memcpy=kinds.get(1, 0), memset=kinds.get(2, 0))
