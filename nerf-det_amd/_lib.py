"""ctypes binding of libnerfdet_hip.so (the C ABI declared in include/nerfdet_hip.h).

There is deliberately NO fallback: if the shared library is missing the import of any compute
entry point raises -- a silent PyTorch path would void every parity and performance claim.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnerfdet_hip.so")

NDET_LAYOUT_CN = 0
NDET_LAYOUT_NC = 1

_P = c_void_p
_F3 = ctypes.POINTER(c_float)


class NdetConvArgs(ctypes.Structure):    # ndet_conv_split's block: include/nerfdet_hip.h::NdetConvArgs (C's `in` is `in_`), size = sizeof(NdetConvArgs)
    _fields_ = ([("size", ctypes.c_int32), ("in_", _P), ("w_planes", _P), ("out", _P)] + [(f, c_int) for f in ("D", "H", "W", "Cin", "Cout")]
                + [(f, c_int * 3) for f in ("kernel", "stride", "pad")] + [("transposed", c_int), ("scale", _P), ("shift", _P), ("residual", _P)]
                + [(f, c_int) for f in ("residual_up2", "relu", "splits", "tile", "arith")] + [("in_amax", _P), ("w_inv_scale", c_float)]
                + [(f, _P) for f in ("w_amax", "out_amax", "workspace", "guard")] + [("guard_l1", c_float), ("guard_tol", c_float), ("keep_partials", c_int)]
                + [(f, _P) for f in ("map_w", "map_b", "map_out")])


class NdetDepthGate(ctypes.Structure):   # the depth gate of the *_gated entry points: include/nerfdet_hip.h::NdetDepthGate, size = sizeof(NdetDepthGate)
    _fields_ = [(f, ctypes.c_int32) for f in ("size", "dtype", "n_views", "h", "w", "H", "W")] + [
        ("depth_f", _P), ("f_view_pitch", c_int64), ("f_row_pitch", c_int64),
        ("depth_r", _P), ("r_view_pitch", c_int64), ("r_row_pitch", c_int64), ("band", ctypes.c_double)]


class NdetSceneAccum(ctypes.Structure):  # a streaming scene's state: include/nerfdet_hip.h::NdetSceneAccum, size = sizeof(NdetSceneAccum)
    _fields_ = [(f, ctypes.c_int32) for f in ("size", "N", "C", "cm", "n_views")] + [
        ("k1_sum", _P), ("k1_pitch", c_int64), ("k1_count", _P), ("k2_sum", _P), ("k2_pitch", c_int64), ("k2_count", _P)]


class NdetBankView(ctypes.Structure):    # one source view of a view bank (a DEVICE table of these): include/nerfdet_hip.h::NdetBankView, 64 bytes
    _fields_ = [("feat", _P), ("rgb4", _P), ("ke", c_float * 12)]


NDET_GROUP_MAX = 64
NDET_OUTSIDE = {"keep": 0, "cull": 1}   # ndet_cull_*'s `outside`: include/nerfdet_hip.h::NDET_OUTSIDE_KEEP / NDET_OUTSIDE_CULL


class NdetSceneSlot(ctypes.Structure):   # one scene of a scene group (a DEVICE table of these): include/nerfdet_hip.h::NdetSceneSlot, 64 bytes
    _fields_ = [(f, _P) for f in ("k1_sum", "k1_count", "k2_sum", "k2_count", "points")] + [("reserved", c_int64 * 3)]


class NdetSceneGroup(ctypes.Structure):  # what a group's scenes share: include/nerfdet_hip.h::NdetSceneGroup, size = sizeof(NdetSceneGroup)
    _fields_ = [(f, ctypes.c_int32) for f in ("size", "n_slots", "N", "C", "cm", "reserved")] + [
        ("k1_pitch", c_int64), ("k2_pitch", c_int64), ("table", _P)]


class NdetGroupSel(ctypes.Structure):    # the scenes one grouped call serves: include/nerfdet_hip.h::NdetGroupSel, size = sizeof(NdetGroupSel)
    _fields_ = [("size", ctypes.c_int32), ("n", ctypes.c_int32), ("slot", ctypes.c_int32 * NDET_GROUP_MAX),
                ("n_views", ctypes.c_int32 * NDET_GROUP_MAX)]


NDET_RING_MAX = 64
NDET_GROUP_POOL_MAX = NDET_GROUP_MAX * (NDET_RING_MAX + 1)   # states a windowed group's pool table may hold


class NdetGroupRingSel(ctypes.Structure):  # the scenes one grouped ring finish serves: include/nerfdet_hip.h::NdetGroupRingSel, 520 bytes
    _fields_ = [("size", ctypes.c_int32), ("n", ctypes.c_int32), ("n_segs", ctypes.c_int32 * NDET_GROUP_MAX),
                ("n_views", ctypes.c_int32 * NDET_GROUP_MAX)]


class NdetBankGroupSel(ctypes.Structure):  # the view banks one grouped sampler call serves: include/nerfdet_hip.h::NdetBankGroupSel, 1032 bytes
    _fields_ = [("size", ctypes.c_int32), ("n", ctypes.c_int32), ("views", _P * NDET_GROUP_MAX), ("n_views", ctypes.c_int32 * NDET_GROUP_MAX),
                ("n_points", ctypes.c_int32 * NDET_GROUP_MAX)]


_G = ctypes.POINTER(NdetDepthGate)
_GR = ctypes.POINTER(NdetGroupRingSel)
_S = ctypes.POINTER(NdetSceneAccum)
_SG = ctypes.POINTER(NdetSceneGroup)
_GS = ctypes.POINTER(NdetGroupSel)

# name -> argtypes; kept in one table so tests can check the .so exports exactly this surface
SIGNATURES = {
    "ndet_version": ([], c_int),
    "ndet_last_error": ([], c_char_p),
    "ndet_get_points": ([_P, c_int, c_int, c_int, _F3, _F3, _P], c_int),
    "ndet_nchw_to_nhwc": ([_P, _P, c_int, c_int, c_int, _P], c_int),
    "ndet_hbm_copy": ([_P, _P, c_int64, _P], c_int),
    "ndet_backproject": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, _P, c_int, _P, _P, _P, _P], c_int),
    "ndet_backproject_aggregate": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, c_int, _P, _P, _P, c_int, _P, _P], c_int),
    "ndet_density_features": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64,
                               c_int64, _P, c_int, _P, _P, _P, _P], c_int),
    "ndet_density_features_packed": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64,
                                      c_int64, _P, c_int, _P, _P, _P, _P], c_int),
    "ndet_depth_resize": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, c_int, c_int, _P, c_int, c_int, _P], c_int),
    "ndet_backproject_gated": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, _P, c_int, _P, _P, _P, _G, _P], c_int),
    "ndet_backproject_aggregate_gated": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, c_int, _P, _P, _P, c_int, _P, _G, _P], c_int),
    "ndet_density_features_gated": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64,
                                     c_int64, _P, c_int, _P, _P, _P, _G, _P], c_int),
    "ndet_density_features_packed_gated": ([_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64,
                                            c_int64, _P, c_int, _P, _P, _P, _G, _P], c_int),
    "ndet_backproject_aggregate_bwd_gated": ([_P, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, c_int, _P, _P, _G, _P], c_int),
    "ndet_density_features_bwd_gated": ([_P, _P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, _P, _P, _P, _G, _P], c_int),
    "ndet_scene_accumulate": ([_S, _P, c_int, c_int, c_int, c_int64, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64, c_int64,
                               _P, _P, _P, _G, _P], c_int),
    "ndet_scene_density_finish": ([_S, _P, _P, _P], c_int),
    "ndet_scene_volume_finish": ([_S, _P, _P, _P, _P], c_int),
    "ndet_scene_density_finish_ring": ([_S, c_int, _P, _P, _P], c_int),
    "ndet_scene_volume_finish_ring": ([_S, c_int, _P, _P, _P, _P], c_int),
    "ndet_scene_group_check": ([_SG, _GS, c_int], c_int),
    "ndet_scene_accumulate_group": ([_SG, _GS, c_int, _P, c_int, c_int, c_int64, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int, c_int64, c_int64,
                                     c_int64, _P, _P, _G, _P], c_int),
    "ndet_scene_density_finish_group": ([_SG, _GS, _P, _P, _P], c_int),
    "ndet_scene_volume_finish_group": ([_SG, _GS, _P, _P, _P, _P], c_int),
    "ndet_scene_group_ring_check": ([_SG, _GR, _P], c_int),
    "ndet_scene_density_finish_group_ring": ([_SG, _GR, _P, _P, _P, _P, _P], c_int),
    "ndet_scene_volume_finish_group_ring": ([_SG, _GR, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_alpha_gate": ([_P, _P, _P, _P, c_int, c_int, c_int, _P], c_int),
    "ndet_sigma_to_alpha": ([_P, _P, c_int, _P], c_int),
    "ndet_posenc_concat": ([_P, _P, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_sigma_head": ([_P, c_int, _P, c_int, c_int, _P, _P, c_int, _P, _P, _P], c_int),
    "ndet_nms_workspace_bytes": ([c_int], c_int64),
    "ndet_aligned_3d_nms": ([_P, _P, _P, c_int, c_float, _P, _P, _P, _P], c_int),
    "ndet_head_decode": ([_P, c_int, _P, _P, c_int, c_int, c_int, _F3, _F3, _P, _P, _P, _P], c_int),
    "ndet_head_decode_levels": ([c_int, _P, _P, _P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_sample_along_rays": ([_P, _P, c_int, c_int, c_float, c_float, _P, _P, _P, _P], c_int),
    "ndet_ray_view_stats": ([_P, c_int, _P, c_int, c_float, c_float, _P, c_int, c_int, c_int64, c_int64, c_int64,
                             _P, c_int, c_int, c_int, c_int64, c_int64, _P, _P, _P, _P], c_int),
    "ndet_pack_rgb_nhwc4": ([_P, c_int, c_int, c_int, c_int64, c_int64, c_int64, _P, _P], c_int),
    "ndet_ray_view_stats_packed": ([_P, c_int, _P, c_int, c_float, c_float, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int64, c_int64,
                                    _P, _P, _P, _P], c_int),
    "ndet_ray_view_stats_bank": ([_P, c_int, _P, c_int, c_float, c_float, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_ray_view_stats_bank_group": ([_P, ctypes.POINTER(NdetBankGroupSel), c_float, c_float, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_occupancy_bits": ([_P, _P, c_int, c_int, c_int, c_float, c_int, _P, _P], c_int),
    "ndet_cull_blocks": ([c_int64], c_int64),
    "ndet_cull_count": ([_P, c_int64, _P, ctypes.POINTER(c_int), _F3, _F3, c_int, _P, _P], c_int),
    "ndet_cull_write": ([_P, c_int64, _P, ctypes.POINTER(c_int), _F3, _F3, c_int, _P, _P, _P, _P], c_int),
    "ndet_ray_view_count_bank": ([_P, c_int64, _P, c_int, c_float, c_float, _P, _P, _P], c_int),
    "ndet_ray_advance": ([_P, _P, c_int, c_int, c_int, c_int, _P], c_int),
    "ndet_front_blocks": ([c_int64, c_int], c_int64),
    "ndet_front_count": ([_P, c_int, c_int, c_int, c_int, _P, c_float, _P, ctypes.POINTER(c_int), _F3, _F3, c_int, _P, _P], c_int),
    "ndet_front_write": ([_P, c_int, c_int, c_int, c_int, _P, c_float, _P, ctypes.POINTER(c_int), _F3, _F3, c_int, _P, _P, _P, _P], c_int),
    "ndet_carve_accumulate": ([_P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int64, c_int64, c_int, c_int, ctypes.c_double, _P, _P], c_int),
    "ndet_carve_bits": ([ctypes.POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P], c_int),
    "ndet_cloud_accumulate": ([_P, c_int, c_int64, c_int64, _P, c_int64, c_int64, c_int64, _P, _P, _P, c_int, c_int, c_int, _F3, _F3, c_int, c_int,
                               c_int, c_float, c_int, _P, _P], c_int),
    "ndet_cloud_blocks": ([c_int64], c_int64),
    "ndet_cloud_count": ([ctypes.POINTER(_P), c_int, c_int, c_int, c_int, _F3, _F3, c_int, _P, _P], c_int),
    "ndet_cloud_write": ([ctypes.POINTER(_P), c_int, c_int, c_int, c_int, _F3, _F3, c_int, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_label_points": ([_P, c_int64, _P, c_int, _P, _P], c_int),
    "ndet_ray_view_stats_packed_bwd": ([_P, _P, c_int, _P, c_int, c_float, c_float, _P, c_int, c_int, c_int, c_int64, c_int64, _P, _P], c_int),
    "ndet_project_sample": ([_P, c_int, _P, c_int, c_float, c_float, _P, c_int, c_int, c_int64, c_int64, c_int64,
                             _P, c_int, c_int, c_int, c_int64, c_int64, _P, _P, _P], c_int),
    "ndet_composite": ([_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_sample_pdf": ([_P, _P, c_int, c_int, _P, c_int, c_int, _P, _P], c_int),
    "ndet_importance_merge": ([_P, _P, _P, _P, c_int, c_int, _P, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_backproject_aggregate_bwd": ([_P, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, c_int, _P, _P, _P], c_int),
    "ndet_density_features_bwd": ([_P, _P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, c_int, _P, _P, _P, _P], c_int),
    "ndet_ray_view_stats_bwd": ([_P, _P, c_int, _P, c_int, c_float, c_float, _P, c_int, c_int, c_int, c_int64, c_int64, _P, _P], c_int),
    "ndet_composite_bwd": ([_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P], c_int),
    "ndet_split_weights_bf16x3": ([_P, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_split_weights_f16x2": ([_P, c_int, c_int, c_int, c_float, _P, _P], c_int),
    "ndet_conv_split": ([ctypes.POINTER(NdetConvArgs), _P], c_int),
    "ndet_conv_split_batch": ([ctypes.POINTER(NdetConvArgs), c_int, _P], c_int),
    "ndet_conv_halo_patch": ([c_int] * 4 + [ctypes.POINTER(c_int)] * 3, c_int),
    "ndet_conv_halo_taps": ([c_int] * 4 + [ctypes.POINTER(c_int)] * 2, c_int),
    "ndet_conv_tile_info": ([c_int] + [ctypes.POINTER(c_int)] * 3, c_int),
    "ndet_conv_chain": ([_P, _P] + [c_int] * 5 + [_P] * 6 + [c_int, _P, _P, _P, c_int, _P, c_int, _P, c_float, c_float, _P, c_float, c_float, c_float, _P, _P], c_int),
    "ndet_bottleneck_f16x2": ([_P, c_int, c_int, c_int, c_int, c_int, _P, c_float, _P, _P, _P, c_float, _P, _P, _P, c_float, _P, _P, _P, c_float, _P, _P, _P, _P, _P,
                               _P, c_float, _P, _P], c_int),
    "ndet_amax_f32": ([_P, ctypes.c_int64, _P, _P], c_int),
    "ndet_amax_slot_floats": ([], c_int),
    "ndet_point_mlp_alpha": ([_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_measurement_knob": ([c_char_p, c_int64], c_int),
    "ndet_split_weights_bf16x3_torch": ([_P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_level_valid": ([_P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_select_candidates": ([c_int, _P, _P, _P, _P, c_float, _P, _P, _P, _P, _P], c_int),
    "ndet_select_candidates_topk": ([c_int, _P, _P, _P, _P, c_float, c_int, _P, _P, _P, _P, _P], c_int),
    "ndet_gather_detections": ([_P, c_int, _P, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_nms_pack_detections": ([_P, _P, _P, _P, c_int, c_int, c_int, c_float, _P, _P, _P, _P, c_int, _P, _P], c_int),
    "ndet_normalize_views": ([_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P], c_int),
    "ndet_target_rays": ([_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_resize_normalize_views": ([_P, _P] + [c_int] * 7 + [_P] * 6, c_int),
    "ndet_resize_normalize_views_nv12": ([_P, _P] + [c_int] * 10 + [_P] * 6, c_int),
    "ndet_nv12_to_bgr": ([_P, _P] + [c_int] * 6 + [_P, _P], c_int),
    "ndet_bgr_to_nv12": ([_P] + [c_int] * 3 + [_P, _P], c_int),
    "ndet_depth_frames": ([_P, _P] + [c_int] * 6 + [_P, _P], c_int),
    "ndet_positive_indices": ([_P, c_int64, _P, _P, _P, _P], c_int),
    "ndet_positive_indices_workspace_bytes": ([c_int64], c_int64),
    "ndet_camera_rays": ([_P, _P, _P] + [c_int] * 6 + [_P, _P, _P], c_int),
    "ndet_pack_frames": ([_P, _P, _P, c_int64, _P, _P, _P], c_int),
    "ndet_frame_errors": ([_P, _P, _P, _P, c_int, c_int64, _P, _P], c_int),
    "ndet_frame_ssim": ([_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_project_boxes": ([_P, _P, _P] + [c_int] * 7 + [c_float, _P, _P, _P, _P, _P], c_int),
    "ndet_draw_boxes": ([_P, _P, _P, _P] + [c_int] * 5 + [_P, _P], c_int),
    "ndet_project_boxes_w": ([_P, _P, _P] + [c_int] * 7 + [c_float, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_draw_overlay": ([_P] * 6 + [c_float, c_int] + [_P] * 4 + [c_int] * 6 + [_P, _P], c_int),
    "ndet_label_frames": ([_P] * 5 + [c_int] * 7 + [_P, _P], c_int),
    "ndet_stem_pack_weights": ([_P, _P, _P], c_int),
    "ndet_stem_conv_bn_relu_maxpool": ([_P, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, _P, c_float, _P, _P, _P, _P, _P], c_int),
    "ndet_stem_pack_weights_f16x2": ([_P, c_float, _P, _P], c_int),
    "ndet_wgrad_dy_planes": ([_P, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_wgrad_dy_planes_f16x2": ([_P, c_int, c_int, c_int, _P, _P, _P], c_int),
    "ndet_bn_workspace_floats": ([c_int64, c_int], c_int64),
    "ndet_bn_train_forward": ([_P, c_int64, c_int, _P, _P, _P, _P, c_float, c_float, _P, c_int, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_bn_train_backward": ([_P, _P, _P, c_int64, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P], c_int),
    "ndet_wgrad_to_torch": ([_P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_split_weights_train": ([_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_relu_affine_bwd": ([_P, _P, _P, c_int64, c_int, c_int, _P, _P, _P], c_int),
    "ndet_relu_affine_bwd_amax": ([_P, _P, _P, c_int64, c_int, c_int, _P, _P, _P, _P], c_int),
    "ndet_wgrad_split": ([_P] + [c_int] * 4 + [_P, _P, _P, _P] + [c_int] * 4 + [_P, _P, _P, _P, c_int, _P], c_int),
    "ndet_wgrad_rows": ([_P] + [c_int] * 4 + [_P, _P, _P] + [c_int] * 3 + [_P, _P], c_int),
    "ndet_bn_relu_maxpool_nhwc": ([_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_conv3d_workspace_bytes": ([c_int] * 8, c_int64),
    "ndet_conv_ndhwc": ([_P, _P, _P, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                         ctypes.POINTER(c_int), _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P], c_int),
    "ndet_conv3d_ndhwc": ([_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, c_int,
                           _P, _P], c_int),
}

_lib = None


class NdetError(RuntimeError):
    pass


def load():
    """Load the library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C nerf-det_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def check(code: int, what: str):
    """0 -> ok.  NDET_E_INVALID maps to AssertionError (the reference asserts on bad arguments),
    NDET_E_UNSUPPORTED to ValueError, anything else to NdetError."""
    if code == 0:
        return
    msg = load().ndet_last_error().decode("utf-8", "replace")
    if code == -1:
        raise AssertionError(f"{what}: {msg}")
    if code == -2:
        raise ValueError(f"{what}: {msg}")
    raise NdetError(f"{what}: error {code}: {msg}")


def float3(vals):
    return (c_float * 3)(*[float(v) for v in vals])


def _ptr(t):
    """A tensor's device address as the C ABI takes it; None -> the null pointer."""
    return c_void_p(0 if t is None else t.data_ptr())


def i3(a, b, c):
    return (c_int * 3)(a, b, c)


def _stream(t):
    """The current HIP stream of the tensor's device, as the C ABI takes it."""
    return c_void_p(raw_stream(t.device))


def raw_stream(device) -> int:
    """The current HIP stream of ``device`` as the raw handle the C ABI takes -- what ``torch.cuda.current_stream(device).cuda_stream`` returns,
    without building the Stream object on the way (measured: 4.6 us a call, ~360 calls per training step)."""
    import torch
    idx = device.index if isinstance(device, torch.device) else (torch.device(device).index if isinstance(device, str) else device)
    if idx is None:
        idx = torch.cuda.current_device()
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return raw(idx) if raw is not None else torch.cuda.current_stream(idx).cuda_stream      # (private getter: the public path if a build lacks it)
