"""ctypes binding of libhumanliff_hip.so (the C ABI declared in include/humanliff_hip.h).

There is no fallback: if the HIP library is missing or a call fails, this raises.
"""
import contextlib
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HL_LIB_PATH") or os.path.join(_HERE, "libhumanliff_hip.so")   # (HL_LIB_PATH: developer A / B of build variants)

HL_RENDER_MLP_FP16 = 16
HL_RENDER_MLP_BF16X3 = 32
HL_RENDER_MLP_FP16X2 = 64
HL_RENDER_FOUR_LAUNCH = 128
HL_CONV_FP32 = 0
HL_CONV_BF16X3 = 1
HL_CONV_FP32_F23 = 3
HL_CONV_FP32_DIRECT = 2
HL_CONV_BF16 = 4
HL_CONV_FP16 = 5
HL_CONV_FP32_MFMA = 6
HL_RENDER_WHITE_BKGD = 1
HL_RENDER_NORMALIZE_DEPTH = 2
HL_RENDER_REEVALUATE = 4
HL_RENDER_CLAMP_DEPTH = 8
HL_COMPOSITE_SERIAL_RAW = 1
HL_COMPOSITE_WAVE_FWD = 2
HL_COMPOSITE_SERIAL_EXACT = 3
HL_COMPOSITE_WAVE_BWD = 4
HL_COMPOSITE_SERIAL_BWD = 5
HL_RASTER_CAM_ROW = 30
HL_RASTER_WHITE_BKGD = 1
HL_RASTER_HEADLIGHT = 2
HL_RASTER_CULL_BACK = 4
HL_RASTER_CULL_FRONT = 8
HL_SIMPLIFY_BOUNDS_WORDS = 6 + 6 * 1024
HL_SIMPLIFY_ACC_WORDS = 20
HL_DISTANCE_WIDE_CELLS = 4096
HL_DISTANCE_MAX_WIDE = 65536
HL_DISTANCE_REDUCE_FIELDS = 16
HL_DISTANCE_REDUCE_WORDS = 16 + 16 * 1024


class HipLibraryMissing(RuntimeError):
    pass


class HipCallError(RuntimeError):
    pass


class RenderMlpParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "pts0_w", "pts0_b", "pts1_w", "pts1_b", "pts2_w", "pts2_b", "feat_w", "feat_b",
        "alpha_w", "alpha_b", "views_w", "views_b", "rgb_w", "rgb_b")]


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("model_channels", C.c_int), ("out_channels", C.c_int),
                ("num_res_blocks", C.c_int), ("n_levels", C.c_int), ("channel_mult", C.c_int * 8),
                ("n_attention_ds", C.c_int), ("attention_ds", C.c_int * 8), ("num_heads", C.c_int),
                ("num_heads_upsample", C.c_int), ("num_classes", C.c_int), ("controlnet", C.c_int), ("adagn", C.c_int), ("cross_attn", C.c_int), ("aware3d", C.c_int),
                ("no_scale_shift", C.c_int)]


class LpipsParams(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 13), ("conv_b", C.c_void_p * 13), ("lin", C.c_void_p * 5), ("shift", C.c_float * 3), ("scale", C.c_float * 3)]


HL_FID_LAYERS = 94
HL_FID_DIMS = 2048
HL_FID_STATE_BYTES = HL_FID_DIMS * HL_FID_DIMS * 8 + HL_FID_DIMS * 8


class FidParams(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * HL_FID_LAYERS), ("conv_b", C.c_void_p * HL_FID_LAYERS)]


_lib = None

_p, _i, _i64, _u, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_size_t

# name -> (restype, argtypes); must list every symbol include/humanliff_hip.h declares
SIGNATURES = {
    "hl_version": (_i, []),
    "hl_last_error": (C.c_char_p, []),
    "hl_render_mlp_packed_bytes": (_sz, []),
    "hl_render_mlp_pack": (_i, [C.POINTER(RenderMlpParams), _p, _p]),
    "hl_planes_packed_bytes": (_sz, [_i, _i]),
    "hl_planes_pack": (_i, [_p, _i, _i, _p, _p]),
    "hl_render_workspace_bytes": (_sz, [_i64, _i, _i]),
    "hl_render_workspace_new_depths_offset": (_sz, [_i64, _i, _i]),
    "hl_render_importance_plan": (_i, [_i64]),
    "hl_render_rays": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _p, _p]),
    "hl_render_rays_u_event": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _p, _p]),
    "hl_render_coarse": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i64, _i, _p, _p]),
    "hl_render_importance": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _p, _p]),
    "hl_deform_points": (_i, [_p, _p, _p, _p, _p, _p, _i, _i64, _p, _p, _p, _p]),
    "hl_deform_rays": (_i, [_p, _p, _p, _p, _p, _i, _i64, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "hl_render_eval_points": (_i, [_p, _p, _i, _i, _p, _p, _p, _i64, _i, _p, _p]),
    "hl_render_canonical_workspace_bytes": (_sz, [_i64, _i, _i]),
    "hl_render_rays_canonical": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p]),
    "hl_camera_rays": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "hl_camera_rays_train": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "hl_render_eval": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _p, _p]),
    "hl_render_eval_products": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _u, _p, _p]),
    "hl_render_importance_new": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _p, _p]),
    "hl_render_composite": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _p]),
    "hl_render_composite_noise": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _p]),
    "hl_render_composite_plan": (_i, [_i64, _i, _i, _i]),
    "hl_render_composite_backward_plan": (_i, [_i, _i]),
    "hl_render_mlp_bwd_packed_bytes": (_sz, []),
    "hl_render_mlp_pack_bwd": (_i, [C.POINTER(RenderMlpParams), _p, _p]),
    "hl_render_train_rows": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hl_render_eval_acts": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _p, _p, _i64, _i64, _p]),
    "hl_render_composite_backward_scratch_bytes": (_sz, [_i64, _i, _i]),
    "hl_render_composite_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u, _p, _p, _p, _i64, _p, _p]),
    "hl_render_eval_points_acts": (_i, [_p, _p, _i, _i, _p, _p, _p, _i64, _i, _p, _p, _i64, _i64, _p]),
    "hl_render_plane_grads_points_scratch_bytes": (_sz, [_i64, _i, _i]),
    "hl_render_plane_grads_points": (_i, [_i, _i, _p, _p, _p, _i64, _i, _i, _p, _i64, _p, _p, _p]),
    "hl_render_weight_grads": (_i, [_p, _i64, _p, _i64, _i64, C.POINTER(RenderMlpParams), _p, _p]),
    "hl_render_weight_grads_scratch_bytes": (_sz, [_i64]),
    "hl_render_plane_grads_scratch_bytes": (_sz, [_i64]),
    "hl_render_mlp_backward": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _p, _p, _i64, _i64, _p, _i64, _i64, _p]),
    "hl_render_plane_grads": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _i, _p, _i64, _p, _p, _p]),
    "hl_render_fine": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _u, _p, _p, _p, _p]),
    "hl_unet_packed_bytes": (_sz, [C.POINTER(UNetCfg)]),
    "hl_unet_create": (_i, [C.POINTER(UNetCfg), _i, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                            _p, _p, C.POINTER(C.c_void_p)]),
    "hl_unet_destroy": (None, [_p]),
    "hl_unet_workspace_bytes": (_sz, [_p, _i, _i, _i]),
    "hl_unet_forward": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "hl_unet_set_overlap": (_i, [_p, _i]),
    "hl_unet_set_conv_mode": (_i, [_p, _i]),
    "hl_unet_profile": (_i, [_p, _i]),
    "hl_unet_profile_read": (_i, [_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "hl_unet_profile_read_ex": (_i, [_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "hl_unet_dispatch_census": (_i, [_p, C.POINTER(C.c_int64)]),
    "hl_unet_dispatch_census_ex": (_i, [_p, _p, _i]),
    "hl_unet_profile_dominant": (_i, [_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "hl_diffusion_step": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p, _p]),
    "hl_diffusion_q_sample": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _p]),
    "hl_diffusion_reverse_step": (_i, [_i, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "hl_diffusion_vb_scratch_bytes": (_sz, [_i64, _i]),
    "hl_diffusion_vb_terms": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _i64, _p, _p, _i64, _i, _i, _p, _p, _p, _i64, _i64, _p, _sz, _p]),
    "hl_diffusion_prior_bpd": (_i, [_p, _p, _i64, _i, _i, _p, _p, _sz, _p]),
    "hl_conv2d_scratch_bytes": (_sz, [_i] * 10),
    "hl_conv2d_plan": (_i, [_i] * 10 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hl_conv2d_plan_ex": (_i, [_i] * 12 + [C.POINTER(C.c_int)]),
    "hl_conv2d_gn_scratch_bytes": (_sz, [_i] * 10),
    "hl_conv2d_bwd_data_scratch_bytes": (_sz, [_i] * 11),
    "hl_conv2d_nhwc": (_i, [_p, _i, _i, _i, _i, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _sz, _p]),
    "hl_conv2d_nhwc_mode": (_i, [_i, _p, _i, _i, _i, _i, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _sz, _p]),
    "hl_conv2d_nhwc_gn": (_i, [_i, _p, _i, _i, _i, _i, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p, C.POINTER(C.c_int), _p, _sz, _p]),
    "hl_conv2d_bwd_data_plan": (_i, [_i] * 11 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hl_conv2d_nhwc_bwd_data": (_i, [_i, _p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _p, _i, _p, _sz, _p]),
    "hl_conv2d_wgrad_scratch_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "hl_conv2d_wgrad_nhwc_ws": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _sz, _p]),
    "hl_conv2d_wgrad_nhwc_ws_mode": (_i, [_i, _p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _sz, _p]),
    "hl_gn_apply_nhwc": (_i, [_p, _i64, _i, _i, _i, _p, _p, _i, _p, _p]),
    "hl_gn_backward_scratch_bytes": (_sz, [_i, _i, _i]),
    "hl_gn_backward_reduce": (_i, [_p, _i64, _p, _i, _i, _i, _p, _p, _i, _p, _p, _sz, _p]),
    "hl_gn_backward_apply": (_i, [_p, _i64, _p, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p]),
    "hl_groupnorm_scratch_bytes": (_sz, [_i]),
    "hl_groupnorm_train_backward_scratch_bytes": (_sz, [_i, _i, _i]),
    "hl_groupnorm_train_forward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_groupnorm_train_backward": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_upsample2_backward_nhwc": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "hl_zero_stuff2_nhwc": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "hl_triplane_agg_backward_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "hl_triplane_agg_forward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "hl_triplane_agg_backward": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _sz, _p]),
    "hl_layernorm_train_forward": (_i, [_p, _i64, _i, _p, _p, C.c_float, _p, _p, _p]),
    "hl_layernorm_backward_scratch_bytes": (_sz, [_i64, _i]),
    "hl_layernorm_train_backward": (_i, [_p, _p, _p, _i64, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_geglu_forward": (_i, [_p, _i64, _i, _p, _p]),
    "hl_geglu_backward": (_i, [_p, _p, _i64, _i, _p, _p]),
    "hl_groupnorm_train_forward_eps": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _i, C.c_float, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_groupnorm_coef": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_attention_nhwc": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "hl_attention_nhwc_mode": (_i, [_i, _p, _i, _i, _i, _i, _p, _p]),
    "hl_attention_backward_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "hl_attention_nhwc_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _sz, _p]),
    "hl_timestep_embedding": (_i, [_p, _p, _i, _i, _p, _p]),
    "hl_mt19937_uniform": (_i, [_p, _i, _p, C.c_int64, _p, _p]),
    "hl_debug_set_h16_min_blocks": (_i, [C.c_long]),
    "hl_debug_set_single_op_scale_source": (_i, [_i]),
    "hl_debug_set_attention_tiling": (_i, [_i, _i]),
    "hl_debug_set_mt19937_piece": (_i, [C.c_int64]),
    "hl_smooth_workspace_bytes": (_sz, [_i, _i, _i]),
    "hl_smooth_prepare": (_i, [_p, _i, _i, _i, _i, C.c_double, _p, _p, _p, _sz, _p]),
    "hl_smooth_band": (_i, [_p, _i, _i, _i, C.c_double, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_smooth_sweep_scratch_bytes": (_sz, [_i64]),
    "hl_smooth_sweeps": (_i, [_p, _p, _p, _i64, _i, _p, _p, _p, _sz, _p]),
    "hl_smooth_scatter": (_i, [_p, _p, _i64, _p, _p]),
    "hl_mc_workspace_bytes": (_sz, [_i, _i, _i]),
    "hl_mc_count": (_i, [_p, _i, _i, _i, C.c_double, _p, _p, _sz, _p]),
    "hl_mc_emit": (_i, [_p, _i, _i, _i, C.c_double, _p, _p, _p, _sz, _p]),
    "hl_mc_max_triangles": (_i, []),
    "hl_mc_case_table": (_i, [_p, _p]),
    "hl_mc_vertex_normals": (_i, [_p, _i, _i, _i, C.c_double, _p, _i64, _p, _p, _p, _sz, _p]),
    "hl_cc_workspace_bytes": (_sz, [_i, _i, _i]),
    "hl_cc_label": (_i, [_p, _i, _i, _i, C.c_double, _p, _p, _p, _sz, _p]),
    "hl_cc_sizes": (_i, [_p, _i64, _i64, _p, _p]),
    "hl_cc_filter": (_i, [_p, _p, _p, _i64, _i64, C.c_double, _p, _p]),
    "hl_mesh_pack_points": (_i, [_p, _p, _i64, _p, _p, _p]),
    "hl_mesh_unpack_colors": (_i, [_p, _i64, _p, _p, _p]),
    "hl_adamw_chunks": (_i64, [C.POINTER(C.c_int64), _i]),
    "hl_adamw_table_bytes": (_sz, [_i, _i64]),
    "hl_adamw_table_pack": (_i, [_i, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), _i, _p, _sz]),
    "hl_adamw_scratch_bytes": (_sz, [_i64]),
    "hl_adamw_step": (_i, [_p, _i, _i64, _i, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                           C.c_float, C.c_float, _p, _sz, _p]),
    "hl_adamw_sum_partials": (_i, [_p, _i64, _p, _p]),
    "hl_fit_reg_scratch_bytes": (_sz, [_i64, _i, _i]),
    "hl_fit_reg": (_i, [_p, _p, _i64, _i, _i, C.c_float, C.c_float, C.c_float, _p, _p, _sz, _p]),
    "hl_fit_adam_planes": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_float, _i, _p]),
    "hl_image_metrics_workspace_bytes": (_sz, [_i, _i, _i]),
    "hl_image_metrics": (_i, [_p, _p, _p, _i, _i, _i, C.c_double, _u, _p, _p, _p, _p, _sz, _p]),
    "hl_lpips_workspace_bytes": (_sz, [_i, _i, _i]),
    "hl_lpips_tap_shape": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hl_lpips_features": (_i, [C.POINTER(LpipsParams), _p, _p, _i, _i, _i, _p, _sz, _p]),
    "hl_lpips": (_i, [C.POINTER(LpipsParams), _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "hl_camera_table_row": (_i, [_p, _p, _p, _p, _p]),
    "hl_ray_views_prepare": (_i, [_p, _p, _i64, _i, _i, _p, _p, _p]),
    "hl_ray_batch": (_i, [_p, _i, _p, _i, _p, _p, _p, _i64, _i, _i, _i, C.c_double, _p, C.c_uint64, C.c_uint64, _i, _p, _p, _p, _p, _p, _p,
                          _p, _p, _p, _p]),
    "hl_body_packed_bytes": (_sz, [_i, _i, _i]),
    "hl_body_pack": (_i, [_p, _p, _i, _p, _p, _p, _i, _i, _i, _p, _p]),
    "hl_body_chunk_frames": (_i, []),
    "hl_body_pose_workspace_bytes": (_sz, [_i, _i]),
    "hl_body_pose": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_area_max_taps": (_i, [_i, _i]),
    "hl_area_taps": (_i, [_i, _i, _i, _p, _p, _p]),
    "hl_nearest_taps": (_i, [_i, _i, _p]),
    "hl_view_ingest_table_words": (_sz, [_i, _i]),
    "hl_view_ingest_table": (_i, [_i, _i, _p]),
    "hl_view_ingest": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "hl_view_ingest_layers": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "hl_pose_body_margins": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, C.c_float, C.c_float, _p]),
    "hl_smplx_packed_bytes": (_sz, [_i, _i, _i, _i]),
    "hl_smplx_pack": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p, _i, _i, _p, _p]),
    "hl_smplx_chunk_frames": (_i, []),
    "hl_smplx_pose_workspace_bytes": (_sz, [_i, _i]),
    "hl_smplx_pose": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, C.c_float, C.c_float, _p]),
    "hl_mesh_bind": (_i, [_p, _p, _i64, _p, _p, _i, _p, _p, _i, _p, _p, _p, _p, _p]),
    "hl_mesh_repose_scratch_bytes": (_sz, [_i64, _i]),
    "hl_mesh_repose": (_i, [_p, _p, _p, _p, _i64, _i, _p, _i, _i, _p, _i, _p, _p, _p, _p, C.c_float, C.c_float, _p, _sz, _p]),
    "hl_mesh_raster_small_box": (_i, []),
    "hl_mesh_raster_scratch_bytes": (_sz, [_i64, _i64, _i, _i, _i]),
    "hl_mesh_raster": (_i, [_p, _i, _i64, _p, _i64, _p, _i, _p, _p, _i, _i, _i, _i, C.c_double, _u, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_mesh_simplify_bounds": (_i, [_p, _i64, _p, _p, _p]),
    "hl_mesh_simplify_scratch_bytes": (_sz, [_i64] * 5),
    "hl_mesh_simplify_count": (_i, [_p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _p, _p, _sz, _p]),
    "hl_mesh_simplify_emit": (_i, [_p, _p, _p, _i64, _p, _i64, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "hl_mesh_distance_scratch_bytes": (_sz, [_i64] * 4),
    "hl_mesh_distance_areas": (_i, [_p, _i64, _p, _i64, _p, C.c_double, _p, _p, _p, _sz, _p]),
    "hl_mesh_distance_count": (_i, [_p, _i64, _p, _i64, _p, C.c_double, _i64, _i64, _i64, _p, _p, _p, _sz, _p]),
    "hl_mesh_distance_fill": (_i, [_i64, _p, C.c_double, _i64, _i64, _i64, _p, _i64, _p, _sz, _p]),
    "hl_mesh_distance_query": (_i, [_p, _p, _i64, _i64, _p, C.c_double, _i64, _i64, _i64, _p, _i64, _i64, C.c_double, _p, _p, _p, _p, _p, _p, _p, _p, _sz,
                                    _p]),
    "hl_mesh_distance_sample": (_i, [_p, _i64, _p, _i64, _p, _p, _i64, _i64, C.c_uint64, _p, _p, _p, _p, _p]),
    "hl_mesh_distance_reduce": (_i, [_p, _p, _p, _i64, _p, _i, _p, _p]),
    "hl_fid_layer": (_i, [_i, C.c_char_p, _i, C.POINTER(C.c_int)]),
    "hl_fid_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "hl_fid_block_shape": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hl_fid_features": (_i, [C.POINTER(FidParams), _p, _i, _i, _i, _i, _i, _p, _p, _sz, _p]),
    "hl_fid_moments_update": (_i, [_p, _p, _i, _p]),
    "hl_fid_moments_finalize": (_i, [_p, _i64, _p, _p, _p]),
    "hl_feat_workspace_bytes": (_sz, [_i, _i64, _i64, _i64, _i64, _i]),
    "hl_feat_split": (_i, [_i64, _i64, _i]),
    "hl_feat_pairwise": (_i, [_p, _i64, _p, _i64, _i64, _i, _p, _p, _sz, _p]),
    "hl_feat_kid": (_i, [_p, _i64, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _p, _sz, _p]),
    "hl_feat_knn_radii": (_i, [_p, _i64, _i64, _i, _i, _p, _p, _sz, _p]),
    "hl_feat_manifold": (_i, [_p, _i64, _p, _i64, _i64, _p, _p, _i, _p, _p, _p, _p, _sz, _p]),
}


def lib():
    """Load (once) and return the ctypes handle. Raises HipLibraryMissing if it was never built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -m humanliff_amd.build` "
                "(there is no CPU or PyTorch fallback for the hot paths)")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().hl_last_error()
        raise HipCallError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


_PTR_DTYPES = (torch.float32, torch.int64)


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor, or None.  The pointers of the C ABI are `float*` or `int64_t*`
    (include/humanliff_hip.h) unless a call site names another `dtype` (the uint8 box mask of hl_camera_rays, the int32 vertex
    ids of hl_deform_points); anything else would be reinterpreted bytewise by the kernels, so it is refused here."""
    if t is None:
        return None
    assert t.is_cuda, "humanliff_amd kernels need device tensors (no CPU path)"
    assert t.is_contiguous()
    if (t.dtype != dtype) if dtype is not None else (t.dtype not in _PTR_DTYPES):
        raise TypeError(f"humanliff_amd kernel argument must be {dtype or 'float32 / int64'}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on `device` (default: the current device).  Through the raw-stream query (what torch's own
    generated launch code uses: ~0.3 us) rather than torch.cuda.current_stream(), whose Stream object costs ~9 us a call - 5 ms of the
    ~70 ms of Python a UNet training step spends enqueueing its ~1 300 launches."""
    if device is None:
        idx = torch.cuda.current_device()
    else:
        idx = torch.device(device).index if not isinstance(device, int) else device
        if idx is None:
            idx = torch.cuda.current_device()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


_SAME_DEVICE = contextlib.nullcontext()


def on(device):
    """Context that makes `device` the current HIP device for the launches inside it: the library launches on the caller's stream,
    and a stream can only be used from its own device.  Nothing to do - and no torch.cuda.device object to build, ~10 us a use - when it
    is the current device already, the case of every launch of a one-process-per-GPU job."""
    idx = device if isinstance(device, int) else torch.device(device).index
    if idx is None or idx == torch.cuda.current_device():
        return _SAME_DEVICE
    return torch.cuda.device(idx)
