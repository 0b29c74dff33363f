"""ctypes binding of ``libmacvo_hip.so`` (C ABI declared in ``include/macvo_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C mac-vo_amd/csrc``.  There is no
CPU fallback: if the library is missing or a symbol is absent, loading raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmacvo_hip.so")

MV_OK = 0
MV_F32, MV_F16, MV_BF16, MV_BF16X3, MV_BF16X2, MV_PACK_BF16X3, MV_PACK_F16X2 = 0, 1, 2, 3, 4, 5, 6
MV_VOL_ENC16 = 16
MV_LAYOUT_CHW, MV_LAYOUT_HWC = 0, 1
MV_KP_NODEPTH, MV_KP_FULL, MV_KP_MAPPING = 0, 1, 2
MV_KP_RANDOM, MV_KP_GRID, MV_KP_EXPLICIT = 3, 4, 5
MV_KP_TABLE_MAX = 4096
MV_GRAPH_ICP, MV_GRAPH_REPROJ, MV_GRAPH_DISP = 0, 1, 2
MV_COV_MATCH, MV_COV_GMM, MV_COV_NONE = 0, 1, 2
MV_COVMOD_DIAG, MV_COVMOD_NORMALIZE = 1, 2
MV_MOTION_STATIC, MV_MOTION_TARTAN = 0, 1
MV_SOLVE_WORLD, MV_SOLVE_LOCAL = 0, 1
MV_NOCOV_DEPTH, MV_NOCOV_MATCH = 1, 2
MV_UPDATE_COV, MV_UPDATE_FLOW = 0, 1
ABI_VERSION = 8
MV_MAX_LANES = 64        # include/macvo_hip.h
# row columns of mv_eval_flow_lanes / mv_eval_depth_lanes (enum order of the header)
EVAL_FLOW_COLS = ("masked_epe", "epe", "px1", "px3", "px5", "masked_nll", "q25_nll", "q50_nll", "q75_nll", "t25", "t50", "t75",
                  "n_mask", "n_mask_finite", "n_finite", "n_q25", "n_q50", "n_q75", "n_mask_nll")
EVAL_DEPTH_COLS = ("masked_err", "err_25", "err_50", "err_75", "masked_nll", "q25_nll", "q50_nll", "q75_nll", "t25", "t50", "t75",
                   "n_mask", "n_mask_finite", "n_finite", "n_q25", "n_q50", "n_q75", "n_mask_nll")
EVAL_GRID = 100          # GridRecorder((0, 25, .25), ...) / ((0, 50, .5), ...): 100 x 100 bins
EVAL_MAX_PIXELS = 1 << 22
# mv_eval_traj_lanes: dtypes, alignment modes, per-lane status and the row columns (enum order of the header)
MV_TRAJ_F32, MV_TRAJ_F64 = 0, 1
MV_TRAJ_ALIGN_UMEYAMA, MV_TRAJ_ALIGN_ORIGIN, MV_TRAJ_ALIGN_NONE = 0, 1, 2
MV_TRAJ_OK, MV_TRAJ_TOO_SHORT, MV_TRAJ_DEGENERATE, MV_TRAJ_NONFINITE = 0, 1, 2, 3
MV_TRAJ_UNSORTED = 4                             # mv_traj_associate_lanes only
MV_TRAJ_TIME_F64, MV_TRAJ_TIME_I64 = 0, 1        # mv_traj_associate_lanes: the dtype of both clocks
TRAJ_ALIGN = {"umeyama": MV_TRAJ_ALIGN_UMEYAMA, "origin": MV_TRAJ_ALIGN_ORIGIN, "none": MV_TRAJ_ALIGN_NONE}
TRAJ_STATUS = ("OK", "TOO_SHORT", "DEGENERATE", "NONFINITE")
TRAJ_ASSOC_STATUS = TRAJ_STATUS + ("UNSORTED",)  # mv_traj_associate_lanes' status by value (DEGENERATE never occurs there)
EVAL_TRAJ_COLS = ("ate_mean", "ate_std", "ate_rmse", "rte_mean", "rte_std", "rte_rmse", "roe_mean", "roe_std", "roe_rmse", "rpe_mean", "rpe_std",
                  "rpe_rmse", "r00", "r01", "r02", "r10", "r11", "r12", "r20", "r21", "r22", "tx", "ty", "tz", "scale", "d1", "d2", "d3", "n_poses",
                  "n_pairs", "status")
EVAL_TRAJ_MAX_POSES = 1 << 20
# mv_preprocess_plan / mv_preprocess_lanes: transform kinds, interpolation modes, plane-group kinds, the uint8 / bool element type
MV_PP_SCALE, MV_PP_CENTER_CROP, MV_PP_SMART_RESIZE, MV_PP_CAST = 0, 1, 2, 3
MV_PP_NEAREST, MV_PP_BILINEAR = 0, 1
MV_PP_IMAGE, MV_PP_FLOW, MV_PP_MASK, MV_PP_DEPTH = 0, 1, 2, 3
MV_PP_U8 = 7
MV_PP_MAX_GROUPS = 8
PP_INTERP = {"nearest": MV_PP_NEAREST, "bilinear": MV_PP_BILINEAR}
# mv_rectify_maps / mv_remap_lanes: cameras or groups per launch, source layouts
MV_RM_MAX_GROUPS = 4
MV_RM_PLANAR, MV_RM_HWC = 0, 1


class mvKpSelectParams(C.Structure):
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32), ("mode", C.c_int32), ("kernel_size", C.c_int32),
        ("mask_width", C.c_int32), ("max_depth", C.c_float), ("max_depth_cov", C.c_float),
        ("max_match_cov", C.c_float),
    ]


class mvKpGradParams(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("mask_width", C.c_int32), ("nms_size", C.c_int32), ("grad_std", C.c_float)]


class mvMatchCovParams(C.Structure):
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32), ("kernel_size", C.c_int32), ("use_patch_var", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("min_flow_cov_sq", C.c_float), ("min_depth_cov", C.c_float),
    ]


class mvLMParams(C.Structure):
    _fields_ = [
        ("huber_delta", C.c_double), ("radius", C.c_double),
        ("tr_high", C.c_double), ("tr_low", C.c_double), ("tr_up", C.c_double), ("tr_down", C.c_double),
        ("tr_factor", C.c_double), ("tr_min", C.c_double), ("tr_max", C.c_double),
        ("diag_min", C.c_double), ("diag_max", C.c_double), ("decreasing", C.c_double),
        ("pinv_rcond", C.c_double),
        ("reject", C.c_int32), ("max_steps", C.c_int32), ("patience", C.c_int32), ("stop_on_reject", C.c_int32),
    ]


class mvFramePipeConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "H", "W", "C", "pairs", "iters", "radius", "feat_dtype", "layout", "volume_split", "selector_mode",
        "kp_kernel_size", "kp_mask_width", "num_point", "edgewidth", "min_num_point", "graph_type", "filters",
        "cov_kernel_size", "mapping", "map_num_point", "map_mask_width", "async_backend")] + [(n, C.c_float) for n in (
        "fx", "fy", "cx", "cy", "baseline", "bl_fx", "bl_fx_sq", "match_cov_default", "max_match_cov", "max_depth_cov",
        "max_depth", "min_flow_cov_sq", "min_depth_cov", "filter_min_depth", "map_max_depth", "map_max_depth_cov")] + [("lm", mvLMParams)] + [
        (n, C.c_int32) for n in ("cov_model", "cov_modifiers", "motion_model", "frontend_nocov")] + [("cov_match_cov_default", C.c_float)]


class mvMapStores(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "K", "baseline", "pose", "T_BS", "need_interp", "time_ns", "pos_Tw", "cov_Tw", "color",
        "pixel1_uv", "pixel2_uv", "pixel1_d", "pixel2_d", "pixel1_disp", "pixel2_disp", "pixel1_disp_cov", "pixel2_disp_cov",
        "obs1_covTc", "obs2_covTc", "pixel1_uv_cov", "pixel2_uv_cov", "pixel1_d_cov", "pixel2_d_cov",
        "frame2match_ranges", "frame2match_num", "frame2map_ranges", "frame2map_num", "match2frame1", "match2frame2",
        "match2point", "point2match_edges", "point2match_deg", "counts")] + [("max_pt_obs", C.c_int32), ("max_frame_range", C.c_int32)] + \
        [("cap_frames", C.c_int64), ("cap_match", C.c_int64), ("cap_points", C.c_int64)] + \
        [("mp_pos_Tw", C.c_void_p), ("mp_cov_Tw", C.c_void_p), ("mp_color", C.c_void_p), ("cap_map_points", C.c_int64)]


class mvMapFrame(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("table_stride", C.c_int32), ("prev_frame", C.c_int32), ("min_num_point", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("valid", "kp0", "kp1", "vals", "sigma0", "sigma1", "cov0", "cov1", "pos_Tw", "cov0_world",
                                   "color", "K", "T_BS", "prior_pose")] + \
        [("baseline", C.c_float), ("time_ns", C.c_int64), ("out_frame_idx", C.c_void_p)]


class mvMapFrameLanes(C.Structure):
    _fields_ = [("lanes", C.c_int32), ("cap", C.c_int32), ("prev_frame", C.c_int32), ("min_num_point", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("n_rows", "time_ns", "valid", "kp0", "kp1", "vals", "sigma0", "sigma1", "cov0", "cov1", "pos_Tw", "cov0_world",
                                   "color", "K", "T_BS", "prior_pose")] + [("baseline", C.c_float)]


class mvPreprocessPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "src_h", "src_w", "win_h", "win_w", "win_y0", "win_x0", "win_vy0", "win_vy1", "win_vx0", "win_vx1", "rs_h", "rs_w",
        "out_h", "out_w", "out_y0", "out_x0", "out_vy0", "out_vy1", "out_vx0", "out_vx1", "scaled", "interp", "mid_dtype", "out_dtype")] + \
        [("round_scale_u", C.c_float), ("round_scale_v", C.c_float), ("K", C.c_float * 9)]


class mvPreprocessGroup(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_lane_stride", C.c_int64), ("dst_lane_stride", C.c_int64)] + \
        [(n, C.c_int32) for n in ("planes", "kind", "src_dtype", "dst_dtype")]


class mvRectifyCam(C.Structure):
    _fields_ = [("iR", C.c_double * 9), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 8)]


class mvRectifyPlan(C.Structure):
    _fields_ = [("R1", C.c_double * 9), ("R2", C.c_double * 9), ("P1", C.c_double * 12), ("P2", C.c_double * 12), ("cam", mvRectifyCam * 2),
                ("fc", C.c_double), ("baseline", C.c_double), ("K", C.c_float * 9), ("width", C.c_int32), ("height", C.c_int32), ("idx", C.c_int32)]


class mvRemapGroup(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("map_x", C.c_void_p), ("map_y", C.c_void_p)] + \
        [(n, C.c_int64) for n in ("src_lane_stride", "dst_lane_stride", "map_lane_stride")] + \
        [(n, C.c_int32) for n in ("channels", "layout", "reverse_channels", "src_dtype", "dst_dtype", "reserved")]


class mvFrameInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("fmap1", "fmap2", "coords", "flow", "logcov", "flow8", "cov8", "up_mask",
                                          "cov_mask")]


# mv_frame_pipe_buffer ids (enum order of the header)
FB_NAMES = ("VOLUME", "TOKENS", "DISPARITY", "DISPARITY_COV", "DEPTH", "DEPTH_COV", "MATCH_FLOW", "MATCH_COV", "CAND",
            "COUNT", "STATS", "KP0", "KP0F", "KP1", "INBOUND", "VALS", "SIGMA0", "SIGMA1", "POS_TC", "POS_TW", "ROT", "COV0",
            "COV0W", "COV1", "VALID", "NVALID", "POSE64", "INFO", "POSE", "MAP_UV", "MAP_D", "MAP_SDD", "MAP_TC", "MAP_TW", "MAP_COV",
            "MAP_COLOR", "PERM", "LIVE", "MOTION_IN", "PRIOR")
FB = {n: i for i, n in enumerate(FB_NAMES)}

_P = C.c_void_p
_PD = C.POINTER(C.c_double)
# the four window lookups: vol, coords, out, B, H1, W1, H2, W2, radius, stream
_LOOKUP = [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]
# the six posed solves: (nprob, offsets, n_live, cap, graph_type) or (nprob, offsets, n_live_dev, n_live_stride, cap, graph_type), then the poses and tables
# (14 pointers, one more per extra pose), then filter_flags ... stream
_POSED_HOST = [C.c_int, _P, _P, C.c_int, C.c_int]
_POSED_DEV = [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int]
_POSED_TAIL = [C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, C.c_int, C.POINTER(mvLMParams)] + [_P] * 5
# name -> (restype, argtypes): every symbol include/macvo_hip.h declares
SIGNATURES = {
    "mv_abi_version": (C.c_int, []),
    "mv_error_string": (C.c_char_p, [C.c_int]),
    "mv_corr_volume": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_split_bf16x3": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "mv_corr_volume_last_kernel": (C.c_char_p, []),
    "mv_volume_pack_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mv_volume_pack": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_corr_volume_packed_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mv_corr_volume_packed": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_corr_volume_packed_shared": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_corr_lookup": (C.c_int, _LOOKUP),
    "mv_corr_lookup_tiled": (C.c_int, _LOOKUP),
    "mv_corr_lookup_vol16": (C.c_int, _LOOKUP),
    "mv_corr_lookup_tiled_vol16": (C.c_int, _LOOKUP),
    "mv_fmap_tile_rows16": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_tiled_slice_cells": (C.c_int, [C.c_int, C.c_int]),
    "mv_corr_volume_out16_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mv_corr_volume_out16": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_volume_pack_tiled": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_frontend_epilogue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                       _P, _P, _P, _P, _P, _P, _P, _P]),
    "mv_convex_upsample": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "mv_convex_upsample_m": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "mv_input_pad": (None, [C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "mv_convex_upsample_crop": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [C.c_float, C.c_int, _P]),
    "mv_convex_upsample_crop_m": (C.c_int, [_P, _P, C.c_int, _P] + [C.c_int] * 7 + [C.c_float, C.c_int, _P]),
    "mv_kp_select_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mv_kp_select": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(mvKpSelectParams), _P, C.c_size_t,
                               _P, _P, _P, _P]),
    "mv_kp_select_finish_capacity": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mv_kp_gather": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "mv_kp_track": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                              C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "mv_match_cov": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(mvMatchCovParams), C.c_int, _P, _P, _P, _P]),
    "mv_match_cov_pair": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(mvMatchCovParams), C.c_int, _P]),
    "mv_obs_cov": (C.c_int, [C.c_int, C.c_int32, _P, _P, _P, _P, _P, _P, C.POINTER(mvMatchCovParams), C.c_int, _P, _P, _P, _P]),
    "mv_obs_cov_pair_lanes": (C.c_int, [C.c_int, C.c_int32] + [_P] * 12 + [C.POINTER(mvMatchCovParams), C.c_int, _P, C.c_int, _P]),
    "mv_obs_cov_pair_nomatch_lanes": (C.c_int, [C.c_int, C.c_int32] + [_P] * 11 + [C.c_float, _P, C.POINTER(mvMatchCovParams), C.c_int, _P, C.c_int, _P]),
    "mv_motion_input_lanes": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_longlong, _P, C.c_longlong] + [C.c_float] * 5 + [_P, _P]),
    "mv_pose_exp_compose": (C.c_int, [C.c_int, _P, _P, C.c_longlong, _P, _P, _P]),
    "mv_pgo_solve_posed_motion": (C.c_int, _POSED_HOST + [_P] * 15 + _POSED_TAIL),
    "mv_pgo_solve_posed_motion_dev": (C.c_int, _POSED_DEV + [_P] * 15 + _POSED_TAIL),
    "mv_frame_pipe_wait_motion_input": (C.c_int, [_P, _P]),
    "mv_frame_pipe_set_motion": (C.c_int, [_P, _P, _P]),
    "mv_lm_default_params": (None, [C.POINTER(mvLMParams)]),
    "mv_pgo_solve": (C.c_int, [C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int,
                               C.POINTER(mvLMParams), _P, _P, _P, _P]),
    "mv_pgo_solve_posed": (C.c_int, _POSED_HOST + [_P] * 14 + _POSED_TAIL),
    "mv_pgo_solve_posed_dev": (C.c_int, _POSED_DEV + [_P] * 14 + _POSED_TAIL),
    "mv_pgo_solve_local": (C.c_int, [C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int,
                                     C.POINTER(mvLMParams), _P, _P, _P, _P]),
    "mv_pgo_solve_posed_local": (C.c_int, _POSED_HOST + [_P] * 16 + _POSED_TAIL),
    "mv_pgo_solve_posed_local_dev": (C.c_int, _POSED_DEV + [_P] * 16 + _POSED_TAIL),
    "mv_backend_front_draw_lanes": (C.c_int, [_P, C.c_size_t, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int] + [_P] * 10 +
                                    [C.c_int, C.c_float, C.POINTER(mvMatchCovParams)] + [_P] * 13),
    "mv_backend_front_lanes": (C.c_int, [_P, C.c_size_t, _P, _P, C.c_int, _P, C.c_int] + [_P] * 10 + [C.c_int, C.c_float, C.POINTER(mvMatchCovParams)] +
                               [_P] * 11),
    "mv_backproject": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P, C.c_int,
                                 _P, _P, _P, _P]),
    "mv_obs_filter": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    "mv_map_points": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P,
                                C.c_float, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mv_local_corr81": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_map_append": (C.c_int, [C.POINTER(mvMapFrame), C.POINTER(mvMapStores), _P]),
    "mv_body_poses": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mv_motion_interpolate": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    # lane-batched variants (lanes independent frames per launch)
    "mv_frontend_epilogue_lanes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                             _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "mv_pose_apply_lanes": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "mv_frontend_epilogue_select_lanes": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                    C.POINTER(mvKpSelectParams), _P, C.c_size_t, _P, _P, _P, C.c_int, _P]),
    "mv_kp_select_lanes": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(mvKpSelectParams), _P, C.c_size_t,
                                     _P, _P, _P, C.c_int, _P]),
    "mv_kp_gather_lanes": (C.c_int, [_P, C.c_size_t, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "mv_kp_track_lanes": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                    C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "mv_backproject_lanes": (C.c_int, [_P, _P, C.c_int, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_float, _P,
                                       C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "mv_match_cov_pair_lanes": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(mvMatchCovParams), C.c_int, _P,
                                          C.c_int, _P]),
    "mv_obs_filter_lanes": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, C.c_int, _P, _P, _P]),
    "mv_patch_embed_packed_bytes": (C.c_size_t, []),
    "mv_patch_embed_pack": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "mv_cost_patch_embed_supported": (C.c_int, [C.c_int, C.c_int]),
    "mv_cost_patch_embed": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_cost_patch_embed_t": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_frame_pipe_arena_bytes": (C.c_size_t, [C.POINTER(mvFramePipeConfig)]),
    "mv_frame_pipe_max_pending": (C.c_int, []),
    "mv_frame_pipe_default_depth": (C.c_int, [C.c_int, C.c_int]),
    "mv_frame_pipe_create": (C.c_int, [C.POINTER(mvFramePipeConfig), _P, C.c_size_t, C.POINTER(_P)]),
    "mv_frame_pipe_destroy": (None, [_P]),
    "mv_frame_pipe_set_pose": (C.c_int, [_P, _P]),
    "mv_frame_pipe_enqueue": (C.c_int, [_P, C.POINTER(mvFrameInputs), _P, C.c_int]),
    "mv_frame_pipe_enqueue_volume": (C.c_int, [_P, C.POINTER(mvFrameInputs), _P]),
    "mv_frame_pipe_wait_candidates": (C.c_int, [_P, _P]),
    "mv_frame_pipe_finish": (C.c_int, [_P, _P, _P, _P]),
    "mv_map_append_points": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "mv_map_append_skipped": (C.c_int, [C.POINTER(mvMapStores), _P, _P, _P, C.c_float, C.c_int64, _P]),
    "mv_frame_pipe_set_solve_frame": (C.c_int, [_P, C.c_int]),
    "mv_frame_pipe_skip": (C.c_int, [_P]),
    "mv_frame_pipe_map_skip": (C.c_int, [_P, C.POINTER(mvMapStores), C.c_int, _P, _P, C.c_float, C.c_int64]),
    "mv_kp_front_lanes": (C.c_int, [_P, C.c_size_t, _P, _P, C.c_int, _P, C.c_int] + [_P] * 10 + [C.c_int, C.c_int, C.c_int] +
                          [C.c_float] * 5 + [_P] * 8 + [_P]),
    "mv_frame_pipe_wait_tracked": (C.c_int, [_P, _P, _P]),
    "mv_frame_pipe_map_points": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mv_frame_pipe_seed_lanes": (C.c_int, [_P, _P]),
    "mv_frame_pipe_finish_seeded": (C.c_int, [_P, _P, _P, _P]),
    "mv_frame_pipe_map_append": (C.c_int, [_P, C.POINTER(mvMapStores), C.c_int, C.c_int, _P, _P, C.c_float, C.c_int64, _P]),
    "mv_frame_pipe_release": (C.c_int, [_P, _P]),
    "mv_frame_pipe_sync": (C.c_int, [_P, _P, C.c_int]),
    "mv_frame_pipe_time_volume": (C.c_int, [_P, C.c_int]),
    "mv_frame_pipe_volume_times": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "mv_frame_pipe_volume_starts": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "mv_frame_pipe_time_detail": (C.c_int, [_P, C.c_int]),
    "mv_randperm_heads": (C.c_int, [C.c_uint64, _P, C.c_int, C.c_int, _P]),
    "mv_frame_pipe_device_draw": (C.c_int, [_P]),
    "mv_frame_pipe_volume_tiled": (C.c_int, [_P]),
    "mv_frame_pipe_host_threads": (C.c_int, [_P]),
    "mv_frame_pipe_finish_device": (C.c_int, [_P, _P]),
    "mv_frame_pipe_finished_counts": (C.c_int, [_P, C.c_int, _P, _P]),
    "mv_frame_pipe_wait_finished": (C.c_int, [_P, C.c_int]),
    "mv_randperm_state_words": (C.c_int, []),
    "mv_randperm_max_head": (C.c_int, []),
    "mv_mt19937_seed": (C.c_int, [C.c_uint64, _P]),
    "mv_randperm_head_lanes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    "mv_randperm_heads_emulated": (C.c_int, [C.c_uint64, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mv_kp_random_max_point": (C.c_int, []),
    "mv_kp_random_lanes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mv_kp_random_emulated": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_kp_random_then_randperm_emulated": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P]),
    "mv_kp_random_heads": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mv_kp_grid_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mv_kp_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    # the image-gradient selectors: (image, params, workspace, workspace_bytes, out_cand, out_count, out_stats, lanes, stream) and the device finish
    # (state, cand, cand_lane_stride, count_dev, count_stride, lanes, k, cap, W, out_uv, out_n_sel, stream)
    "mv_kp_gradient_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mv_kp_gradient_lanes": (C.c_int, [_P, C.POINTER(mvKpGradParams), _P, C.c_size_t, _P, _P, _P, C.c_int, _P]),
    "mv_kp_finish_device_lanes": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "mv_frame_pipe_table_rows": (C.c_int, [_P]),
    "mv_frame_pipe_finish_keypoints": (C.c_int, [_P, _P, _P, _P]),
    "mv_frame_pipe_finish_keypoints_dev": (C.c_int, [_P, _P, _P, _P, _P]),
    "mv_frame_pipe_timeline": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "mv_frame_pipe_timeline_backend": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "mv_frame_pipe_buffer": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    # one map per lane of a batched pipe (stores: a DEVICE array mvMapStores[lanes]; time_ns: a host int64 array [lanes])
    "mv_map_append_lanes": (C.c_int, [C.POINTER(mvMapFrameLanes), _P, _P]),
    "mv_map_append_skipped_lanes": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_float, _P, _P]),
    "mv_map_set_pose_lanes": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "mv_frame_pipe_map_append_lanes": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_float, _P]),
    "mv_frame_pipe_map_skip_lanes": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_float, _P]),
    # frontend evaluation (EvalFlow.py / EvalDepth.py): rows[lanes][rows_per_lane][COLS] on the device, one row per lane and call
    "mv_eval_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mv_eval_flow_lanes": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_float, C.c_int,
                                     _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "mv_eval_depth_lanes": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_float, _P, C.c_int, C.c_int, _P, _P, _P,
                                      _P, C.c_size_t, _P]),
    # trajectory evaluation (MetricsSeq.py / EvalSeq.py): est / ref / T are HOST arrays [lanes] (device pointers, counts); rows fp64 [lanes][len(EVAL_TRAJ_COLS)]
    "mv_eval_traj_lanes": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_int64, _P]),
    # trajectory association (Trajectory.from_sandbox's align_origin / rebase / align_time): src, src_time, T, query_time, Q, origin_ref, out_poses,
    # out_extrapolated are HOST arrays [lanes]; status int32 [lanes] on the device
    "mv_traj_associate_lanes": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _P, _P, _P, _P]),
    # PoseInterpolate (MapProcessor.py:28-49): one table, or every lane's map through the device descriptor array (T: host int32 [lanes])
    "mv_pose_interpolate": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mv_pose_interpolate_lanes": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P]),
    # frame preprocessing (DataLoader/Transform.py): the host-only plan (plan, prev or NULL, src_h, src_w, K host [9] or NULL, kind, a0, a1, mode) and the launch
    "mv_preprocess_plan": (C.c_int, [C.POINTER(mvPreprocessPlan), C.POINTER(mvPreprocessPlan), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_double,
                                     C.c_double, C.c_int]),
    "mv_preprocess_lanes": (C.c_int, [C.POINTER(mvPreprocessPlan), C.POINTER(mvPreprocessGroup), C.c_int, C.c_int, _P]),
    # stereo rectification (DataLoader/Dataset/EuRoC.py:143-174, 231-236; VBR.py:60-64, 155-180): the host-only plan (plan, K1, D1, n_d1, K2, D2, n_d2, nx, ny,
    # R, T: host doubles), the map builder (cams host [n_cams], n_cams, out_h, out_w, map_x, map_y, stream) and the per-frame remap (groups host [n_groups],
    # n_groups, lanes, src_h, src_w, out_h, out_w, stream)
    "mv_stereo_rectify_plan": (C.c_int, [C.POINTER(mvRectifyPlan), _PD, _PD, C.c_int, _PD, _PD, C.c_int, C.c_int, C.c_int, _PD, _PD]),
    "mv_rectify_maps": (C.c_int, [C.POINTER(mvRectifyCam), C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "mv_remap_lanes": (C.c_int, [C.POINTER(mvRemapGroup), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # the PoseNet of TartanMotionNet: tensor table, host packer, forward (packed, x, lanes, out, workspace, stage_out [6] or NULL, stream)
    "mv_posenet_tensor_count": (C.c_int, []),
    "mv_posenet_tensor_info": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mv_posenet_packed_bytes": (C.c_size_t, []),
    "mv_posenet_workspace_bytes": (C.c_size_t, [C.c_int]),
    "mv_posenet_pack": (C.c_int, [C.POINTER(_P), _P]),
    "mv_posenet_forward_lanes": (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(_P), _P]),
    # the decoder's update blocks (kind MV_UPDATE_COV / MV_UPDATE_FLOW, operand MV_F16 / MV_BF16): tensor table, device packer (kind, operand, tensors, packed,
    # stream), forward (kind, operand, packed, net, inp, B, H, W, channels_last, net_out, delta, mask, workspace, stream)
    "mv_update_block_tensor_count": (C.c_int, [C.c_int]),
    "mv_update_block_tensor_info": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mv_update_block_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mv_update_block_pack": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P), _P, _P]),
    "mv_update_block_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mv_update_block_forward": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    # the decoder's motion encoder (operand MV_F16 / MV_BF16): tensor table, device packer (operand, tensors, packed, stream), forward (operand, packed, flow,
    # corr, B, H, W, channels_last, out, workspace, stream)
    "mv_motion_encoder_tensor_count": (C.c_int, []),
    "mv_motion_encoder_tensor_info": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mv_motion_encoder_packed_bytes": (C.c_size_t, [C.c_int]),
    "mv_motion_encoder_pack": (C.c_int, [C.c_int, C.POINTER(_P), _P, _P]),
    "mv_motion_encoder_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mv_motion_encoder_forward": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
}

_lib = None
_lock = threading.Lock()


class MacvoHipError(RuntimeError):
    pass


def load(path: str | None = None) -> C.CDLL:
    """Load (once) and type the shared library.  Raises if it is missing — there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # libmacvo_hip.so needs libamdhip64.so.7: import torch first so that the HIP runtime PyTorch already
        # loaded is the one the dynamic linker binds (one runtime per process -> shared streams/allocations).
        import torch  # noqa: F401

        p = path or os.environ.get("MACVO_HIP_LIB") or LIB_PATH   # MACVO_HIP_LIB: A/B a differently built library
        if not os.path.exists(p):
            raise MacvoHipError(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C mac-vo_amd/csrc` (no CPU fallback exists for the HIP hot path)"
            )
        try:
            lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            # no HIP runtime resolvable yet (e.g. CPU-only process): point the loader at ROCm's copy
            for cand in ("/opt/rocm/lib/libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
                if os.path.exists(cand):
                    C.CDLL(cand, mode=C.RTLD_GLOBAL)
                    break
            lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.mv_abi_version() != ABI_VERSION:
            raise MacvoHipError(f"ABI mismatch: library {lib.mv_abi_version()} != binding {ABI_VERSION}")
        _lib = lib
    return _lib


def check(code: int, what: str) -> None:
    if code != MV_OK:
        msg = load().mv_error_string(code).decode()
        raise MacvoHipError(f"{what} failed: {msg} ({code})")
