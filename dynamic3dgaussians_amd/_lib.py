"""Loader and ctypes mirrors of libgsplat_hip.so (C ABI: include/gsplat_hip.h).

The library is the only way the package reaches the GPU: there is no CPU or
PyTorch fallback.  If it is missing or cannot be loaded, every entry point
raises immediately with the reason.  The losses, the optimizer, densification
and the motion warp are called through the prototypes below; the rasterizer's
forward and backward go through the C++ binding instead (_C.py,
csrc/gs_torch_binding.cpp), and their prototypes and struct mirrors here serve
the tests and tools that drive the C ABI directly.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch

from . import build as _build

_lock = threading.Lock()
_lib = None

c_void_p = ctypes.c_void_p
ABI_VERSION = 13  # include/gsplat_hip.h GS_ABI_VERSION
GS_FLAG_ACCUMULATE = 1  # include/gsplat_hip.h
GS_FLAG_ACTIVATE = 2  # include/gsplat_hip.h: raw opacity / scale / rotation parameters
GS_FLAG_SCRATCH_ZEROED = 4  # include/gsplat_hip.h: the backward's scratch was zeroed by the forward
c_int32, c_int64, c_float, c_size_t = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t

GS_COMPAT = {"reference": 0, "fixed": 1}
SUPPORTED_F = (0, 4, 8, 16, 32, 36, 64)


class GsGaussians(ctypes.Structure):
    _fields_ = [("P", c_int32), ("D", c_int32), ("M", c_int32), ("F", c_int32),
                ("means3D", c_void_p), ("shs", c_void_p), ("colors_precomp", c_void_p),
                ("semantic_feature", c_void_p), ("opacities", c_void_p), ("scales", c_void_p),
                ("rotations", c_void_p), ("cov3D_precomp", c_void_p),
                ("scale_modifier", c_float), ("flags", ctypes.c_uint32),
                ("grad_mask", c_void_p), ("densify_accum", c_void_p), ("densify_denom", c_void_p),
                ("max_radius", c_void_p), ("feature_ready", c_void_p), ("walk_order", c_void_p),
                ("zero_fill", c_void_p), ("zero_fill_bytes", c_int64)]


class GsCamera(ctypes.Structure):
    _fields_ = [("viewmatrix", c_void_p), ("projmatrix", c_void_p), ("campos", c_void_p),
                ("background", c_void_p), ("c_x", c_float), ("c_y", c_float),
                ("tan_fovx", c_float), ("tan_fovy", c_float),
                ("image_width", c_int32), ("image_height", c_int32),
                ("tile_x0", c_int32), ("tile_y0", c_int32), ("tile_x1", c_int32), ("tile_y1", c_int32)]


class GsNeighborGraph(ctypes.Structure):
    """include/gs_neighbor.h gs_neighbor_graph."""
    _fields_ = [("N", c_int64), ("K", c_int32), ("_pad", c_int32), ("nbr", c_void_p),
                ("weight", c_void_p), ("dist", c_void_p), ("prev_offset", c_void_p),
                ("prev_inv_rot", c_void_p), ("rev_ptr", c_void_p), ("rev_pos", c_void_p)]


class GsPhotoLoss(ctypes.Structure):
    """include/gs_loss.h gs_photo_loss."""
    _fields_ = [("B", c_int32), ("Ch", c_int32), ("H", c_int32), ("W", c_int32), ("image", c_void_p),
                ("target", c_void_p), ("mask", c_void_p), ("gain", c_void_p), ("offset", c_void_p),
                ("mask_batch_stride", c_int64), ("l1_weight", c_float), ("ssim_weight", c_float),
                ("losses", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


class GsDepthLoss(ctypes.Structure):
    """include/gs_depth_loss.h gs_depth_loss."""
    _fields_ = [("B", c_int32), ("H", c_int32), ("W", c_int32), ("depth", c_void_p), ("target", c_void_p),
                ("mask", c_void_p), ("mask_batch_stride", c_int64), ("near", c_float), ("far", c_float),
                ("skip_degenerate", c_int32), ("losses", c_void_p), ("stats", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", ctypes.c_uint64)]


class GsRobustLoss(ctypes.Structure):
    """include/gs_robust_loss.h gs_robust_loss."""
    _fields_ = [("B", c_int32), ("R", c_int32), ("N", c_int32), ("layout", c_int32), ("pred", c_void_p),
                ("gt", c_void_p), ("mask", c_void_p), ("mask_batch_stride", c_int64), ("quantile", ctypes.c_double),
                ("select", c_int32), ("over_masked", c_int32), ("normalize", c_int32), ("norm_width", c_int32),
                ("skip_degenerate", c_int32), ("_pad", c_int32), ("losses", c_void_p), ("stats", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


class GsResample(ctypes.Structure):
    """include/gs_resample.h gs_resample."""
    _fields_ = [("B", c_int32), ("Ch", c_int32), ("H", c_int32), ("W", c_int32), ("h", c_int32), ("w", c_int32),
                ("align_corners", c_int32), ("x", c_void_p), ("y", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", ctypes.c_uint64)]


class GsFeatureDecoder(ctypes.Structure):
    """include/gs_feature_decoder.h gs_feature_decoder."""
    _fields_ = [("B", c_int32), ("F_in", c_int32), ("C_out", c_int32), ("h", c_int32), ("w", c_int32),
                ("mask_per_camera", c_int32), ("x", c_void_p), ("weight", c_void_p), ("bias", c_void_p),
                ("target", c_void_p), ("mask", c_void_p), ("up", c_void_p), ("d_y", c_void_p), ("y", c_void_p),
                ("loss", c_void_p), ("d_x", c_void_p), ("d_weight", c_void_p), ("d_bias", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


# include/gs_feature_decoder.h: the tile shape, the grid rule's block count, the limits and the passes
FD_TILE_ROWS, FD_TILE_PIXELS, FD_GRID, FD_GRID_FORWARD = 32, 128, 512, 1024
FD_MAX_F_IN, FD_MAX_C_OUT, FD_MAX_WEIGHTS = 64, 512, 16384
FD_PASS_DECODE, FD_PASS_LOSS, FD_PASS_LOSS_BACKWARD, FD_PASS_BACKWARD = 0, 1, 2, 3


class GsFeaturePca(ctypes.Structure):
    """include/gs_feature_pca.h gs_feature_pca."""
    _fields_ = [("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32), ("k", c_int32),
                ("mask_per_image", c_int32), ("normalize", c_int32), ("sample_stride", c_int32), ("ddof", c_int32),
                ("compute_shift", c_int32), ("out_uint8", c_int32), ("clamp", c_int32),
                ("x", c_void_p), ("mask", c_void_p), ("shift", c_void_p), ("state", c_void_p), ("mean", c_void_p),
                ("cov", c_void_p), ("evals", c_void_p), ("evecs", c_void_p), ("components", c_void_p),
                ("components_f32", c_void_p), ("mean_f32", c_void_p), ("status", c_void_p),
                ("proj_components", c_void_p), ("proj_mean", c_void_p), ("t", c_void_p), ("tmin", c_void_p),
                ("tmax", c_void_p), ("sub", c_void_p), ("u", c_void_p), ("lo", c_void_p), ("hi", c_void_p),
                ("out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


# include/gs_feature_pca.h: the limits, the sweep cap, the tile and slab sizes and the passes
FPCA_MAX_C, FPCA_MAX_K, FPCA_MAX_SWEEPS = 128, 8, 24
FPCA_TILE_PIXELS, FPCA_CHUNK, FPCA_SLAB_GROUP, FPCA_LDS_MAX_C = 128, 4096, 64, 64
(FPCA_PASS_UPDATE, FPCA_PASS_COVARIANCE, FPCA_PASS_FIT, FPCA_PASS_PROJECT, FPCA_PASS_OFFSET,
 FPCA_PASS_COLOUR) = range(6)


class GsFeatureKnn(ctypes.Structure):
    """include/gs_feature_knn.h gs_feature_knn_args."""
    _fields_ = [("N", c_int32), ("M", c_int32), ("E", c_int32), ("k", c_int32), ("splits", c_int32), ("_pad", c_int32),
                ("feats", c_void_p), ("queries", c_void_p), ("sim", c_void_p), ("index", c_void_p), ("stats", c_void_p),
                ("cand_sim", c_void_p), ("cand_index", c_void_p), ("cand_count", c_void_p), ("cand_theta", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


# include/gs_feature_knn.h: the limits, the scan's slack and its tile shape
FKNN_MAX_E, FKNN_MAX_K, FKNN_MAX_ROWS, FKNN_MAX_SPLITS = 128, 32, 1 << 26, 32
FKNN_SLACK, FKNN_ROW_BLOCK, FKNN_TILE = 16, 128, 32


class GsSpectral(ctypes.Structure):
    """include/gs_spectral.h gs_spectral_args."""
    _fields_ = [("n", c_int32), ("num_vectors", c_int32), ("nnz", c_int64), ("degree", c_int32),
                ("max_outer", c_int32), ("row_normalize", c_int32), ("_pad", c_int32), ("seed", ctypes.c_uint64),
                ("tol", ctypes.c_double), ("row_ptr", c_void_p), ("col", c_void_p), ("val", c_void_p),
                ("eigenvalues", c_void_p), ("vectors", c_void_p), ("embedding", c_void_p), ("residuals", c_void_p),
                ("status", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


# include/gs_spectral.h: the limits and the guard columns of the block
SPECTRAL_MAX_K, SPECTRAL_MAX_N, SPECTRAL_MAX_DEGREE, SPECTRAL_MAX_OUTER = 64, 1 << 26, 64, 1000
SPECTRAL_GUARD, SPECTRAL_MAX_B = 8, 72


class GsSceneLoss(ctypes.Structure):
    """include/gs_scene_loss.h gs_scene_loss."""
    _fields_ = [("P", c_int64), ("n_fg", c_int64), ("n_bg", c_int64), ("slot", c_void_p), ("means", c_void_p),
                ("rotations", c_void_p), ("colors", c_void_p), ("init_bg_pts", c_void_p), ("init_bg_rot", c_void_p),
                ("prev_col", c_void_p), ("raw_rotations", c_int32), ("_pad", c_int32), ("losses", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


class GsImageMetrics(ctypes.Structure):
    """include/gs_metrics.h struct gs_image_metrics."""
    _fields_ = [("B", c_int32), ("Ch", c_int32), ("H", c_int32), ("W", c_int32), ("pred", c_void_p),
                ("target", c_void_p), ("mask", c_void_p), ("mask_batch_stride", c_int64), ("want_ssim", c_int32),
                ("_pad", c_int32), ("out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


GS_SAMPLE_POINTS, GS_SAMPLE_DISPLACEMENT = 0, 1  # include/gs_depth_geometry.h


class GsPointDepth(ctypes.Structure):
    """include/gs_depth_geometry.h struct gs_point_depth."""
    _fields_ = [("P", c_int64), ("B", c_int32), ("H", c_int32), ("W", c_int32), ("_pad", c_int32),
                ("points", c_void_p), ("points_batch_stride", c_int64), ("w2c", c_void_p), ("K", c_void_p),
                ("depth", c_void_p)]


class GsDepthAbsRel(ctypes.Structure):
    """include/gs_depth_geometry.h struct gs_depth_abs_rel."""
    _fields_ = [("B", c_int32), ("H", c_int32), ("W", c_int32), ("_pad", c_int32), ("est", c_void_p),
                ("gt", c_void_p), ("exclude", c_void_p), ("exclude_batch_stride", c_int64), ("out", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


class GsDepthUnproject(ctypes.Structure):
    """include/gs_depth_geometry.h struct gs_depth_unproject."""
    _fields_ = [("B", c_int32), ("H", c_int32), ("W", c_int32), ("_pad", c_int32), ("depth", c_void_p),
                ("xy", c_void_p), ("Kinv", c_void_p), ("c2w", c_void_p), ("xyz", c_void_p)]


class GsDepthFlow(ctypes.Structure):
    """include/gs_depth_geometry.h struct gs_depth_flow."""
    _fields_ = [("B", c_int32), ("H", c_int32), ("W", c_int32), ("_pad", c_int32), ("depth1", c_void_p),
                ("Kinv1", c_void_p), ("T", c_void_p), ("K2", c_void_p), ("flow", c_void_p), ("valid", c_void_p)]


class GsSampleBilinear(ctypes.Structure):
    """include/gs_depth_geometry.h struct gs_sample_bilinear."""
    _fields_ = [("B", c_int32), ("Ch", c_int32), ("H", c_int32), ("W", c_int32), ("mode", c_int32),
                ("add_displacement", c_int32), ("N", c_int64), ("h", c_int32), ("w", c_int32), ("src", c_void_p),
                ("coords", c_void_p), ("out", c_void_p)]


class GsKmeansAssign(ctypes.Structure):
    """include/gs_motion_init.h struct gs_kmeans_assign."""
    _fields_ = [("N", c_int64), ("D", c_int32), ("K", c_int32), ("x", c_void_p), ("centers", c_void_p),
                ("valid", c_void_p), ("prev_labels", c_void_p), ("labels", c_void_p), ("moved", c_void_p)]


class GsKmeansUpdate(ctypes.Structure):
    """include/gs_motion_init.h struct gs_kmeans_update."""
    _fields_ = [("N", c_int64), ("D", c_int32), ("K", c_int32), ("x", c_void_p), ("labels", c_void_p),
                ("centers", c_void_p), ("counts", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", ctypes.c_uint64)]


class GsCoefsFromCenters(ctypes.Structure):
    """include/gs_motion_init.h struct gs_coefs_from_centers."""
    _fields_ = [("N", c_int64), ("K", c_int32), ("_pad", c_int32), ("means", c_void_p), ("centers", c_void_p),
                ("coefs", c_void_p)]


class GsProcrustes(ctypes.Structure):
    """include/gs_motion_init.h struct gs_procrustes."""
    _fields_ = [("N", c_int64), ("T", c_int32), ("K", c_int32), ("cano_t", c_int32), ("rot_dim", c_int32),
                ("min_weight_sum", ctypes.c_double), ("tracks", c_void_p), ("order", c_void_p), ("offsets", c_void_p),
                ("weights", c_void_p), ("confidences", c_void_p), ("rots", c_void_p), ("transls", c_void_p),
                ("err_after", c_void_p), ("err_before", c_void_p), ("skipped", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", ctypes.c_uint64)]


GS_DENSIFY_MAX_TENSORS = 16  # include/gs_densify.h
GS_DENSIFY_N_SPLIT = 2
GS_DENSIFY_ROLES = {"plain": 0, "means": 1, "log_scales": 2, "rotations": 3, "logit_opacities": 4}
GS_DENSIFY_CLONE, GS_DENSIFY_SPLIT, GS_DENSIFY_PRUNE, GS_DENSIFY_PRUNE_SPLIT = 1, 2, 4, 8  # the flag byte


class GsDensifyPlanArgs(ctypes.Structure):
    """include/gs_densify.h gs_densify_plan_args."""
    _fields_ = [("P", c_int64), ("grad_accum", c_void_p), ("denom", c_void_p), ("log_scales", c_void_p),
                ("logit_opacities", c_void_p), ("grad_thresh", c_float), ("clone_max_scale", c_float),
                ("prune_min_opacity", c_float), ("prune_max_scale", c_float), ("n_split", c_int32),
                ("_pad", c_int32), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_uint64)]


class GsDensifyTensor(ctypes.Structure):
    """include/gs_densify.h gs_densify_tensor."""
    _fields_ = [("src", c_void_p), ("src_exp_avg", c_void_p), ("src_exp_avg_sq", c_void_p), ("dst", c_void_p),
                ("dst_exp_avg", c_void_p), ("dst_exp_avg_sq", c_void_p), ("width", c_int32), ("role", c_int32)]


class GsDensifyApplyArgs(ctypes.Structure):
    """include/gs_densify.h gs_densify_apply_args."""
    _fields_ = [("P", c_int64), ("counts", c_int64 * 4), ("workspace", c_void_p),
                ("workspace_bytes", ctypes.c_uint64), ("n_split", c_int32), ("n_tensors", c_int32),
                ("noise", c_void_p), ("stats", c_void_p * 3), ("reset_opacity", c_int32),
                ("opacity_reset", c_float), ("t", GsDensifyTensor * GS_DENSIFY_MAX_TENSORS)]


GS_MOTION_MAX_K, GS_MOTION_MAX_B = 64, 32  # include/gs_motion.h


class GsMotionDesc(ctypes.Structure):
    """include/gs_motion.h gs_motion_desc."""
    _fields_ = [("G", c_int64), ("K", c_int32), ("T", c_int32), ("B", c_int32), ("coef_mode", c_int32),
                ("rots", c_void_p), ("transls", c_void_p), ("coefs", c_void_p), ("means", c_void_p),
                ("ts", c_int32 * GS_MOTION_MAX_B)]


GS_ADAM_MAX_TENSORS = 16  # include/gs_optim.h


class GsAdamTensor(ctypes.Structure):
    """include/gs_optim.h gs_adam_tensor."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("numel", c_int64), ("step_size", c_float), ("bc2_sqrt", c_float)]


class GsAdamArgs(ctypes.Structure):
    """include/gs_optim.h gs_adam_args (GS_ADAM_MAX_TENSORS = 16)."""
    _fields_ = [("n_tensors", c_int32), ("_pad", c_int32), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("t", GsAdamTensor * GS_ADAM_MAX_TENSORS)]


class GsDensifyStats(ctypes.Structure):
    """include/gs_optim.h gs_densify_stats."""
    _fields_ = [("P", c_int64), ("radii", c_void_p), ("means2D_grad", c_void_p), ("max_radius", c_void_p),
                ("grad_accum", c_void_p), ("denom", c_void_p)]


class GsBatchHint(ctypes.Structure):
    """include/gsplat_hip.h gs_batch_hint (ABI 11): the previous plan's sort
    extents, written back by gs_forward_batch."""
    _fields_ = [("valid", c_int32), ("p1", c_int32), ("q1", c_int32), ("p2", c_int32),
                ("max_len", c_int64), ("total", c_int64)]


GS_WINDOW_MAX_FRAMES = 64  # include/gs_window.h
GS_CAMERA_GRAD_MAX_CAMS = 64  # include/gs_camera_grad.h
GS_TRACK_MAX_K, GS_TRACK_MAX_CAMS = 4, 64  # include/gs_track.h


class GsWindow(ctypes.Structure):
    """include/gs_window.h gs_window: a temporal window of B frames of means3D
    (P x B x 3) and each camera's frame (host array, non-decreasing)."""
    _fields_ = [("B", c_int32), ("cam_frame", ctypes.POINTER(c_int32))]


P_G = ctypes.POINTER(GsGaussians)
P_W = ctypes.POINTER(GsWindow)
P_NG = ctypes.POINTER(GsNeighborGraph)
P_C = ctypes.POINTER(GsCamera)

# name -> (restype, argtypes); must match include/gsplat_hip.h
PROTOTYPES = {
    "gs_version": (ctypes.c_int, []),
    "gs_last_error": (ctypes.c_char_p, []),
    "gs_geom_buffer_bytes": (c_size_t, [c_int64]),
    "gs_binning_buffer_bytes": (c_size_t, [c_int64]),
    "gs_image_buffer_bytes": (c_size_t, [c_int32, c_int32]),
    "gs_backward_scratch_bytes": (c_size_t, [c_int64, c_int32]),
    "gs_forward_plan": (ctypes.c_int, [P_G, P_C, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                       c_void_p]),
    "gs_forward_render": (ctypes.c_int, [P_G, P_C, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                         c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "gs_backward": (ctypes.c_int, [P_G, P_C, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                   c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_batch_geom_buffer_bytes": (c_size_t, [c_int64, c_int32]),
    "gs_batch_image_buffer_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "gs_batch_binning_buffer_bytes": (c_size_t, [c_int32, ctypes.POINTER(c_int64)]),
    "gs_batch_backward_scratch_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "gs_forward_plan_batch": (ctypes.c_int, [P_G, P_C, c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64),
                                             ctypes.POINTER(c_int64), c_void_p]),
    "gs_forward_render_batch": (ctypes.c_int, [P_G, P_C, c_int32, ctypes.c_int, ctypes.c_int, c_void_p,
                                               c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_forward_batch": (ctypes.c_int, [P_G, P_C, c_int32, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                        c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(GsBatchHint), c_void_p,
                                        ctypes.POINTER(c_int64), ctypes.POINTER(c_int64), ctypes.POINTER(c_int32),
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_backward_batch": (ctypes.c_int, [P_G, P_C, c_int32, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p,
                                         c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # include/gs_window.h: the batch calls with a window before the stream
    "gs_check_window": (ctypes.c_int, [P_W, c_int32]),
    "gs_forward_plan_batch_window": (ctypes.c_int, [P_G, P_C, c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64),
                                                    ctypes.POINTER(c_int64), P_W, c_void_p]),
    "gs_forward_batch_window": (ctypes.c_int, [P_G, P_C, c_int32, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                               c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(GsBatchHint),
                                               c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                               ctypes.POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_void_p, P_W,
                                               c_void_p]),
    "gs_backward_batch_window": (ctypes.c_int, [P_G, P_C, c_int32, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p,
                                                c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, P_W, c_void_p]),
    # include/gs_camera_grad.h
    "gs_camera_grad_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "gs_check_camera_grad": (ctypes.c_int, [c_int64, c_int32, ctypes.c_int, c_void_p, ctypes.c_uint64, c_void_p,
                                            c_void_p, c_void_p]),
    "gs_camera_grad_batch": (ctypes.c_int, [P_G, P_C, c_int32, P_W, c_void_p, ctypes.c_int, c_void_p, c_void_p,
                                            c_void_p, ctypes.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    # include/gs_track.h
    "gs_check_contributors": (ctypes.c_int, [c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "gs_contributors_batch": (ctypes.c_int, [P_C, c_int32, c_int64, ctypes.c_int, c_void_p, c_void_p, c_void_p,
                                             ctypes.POINTER(c_int64), c_int32, c_void_p, c_void_p, c_void_p]),
    "gs_check_track_project": (ctypes.c_int, [c_int64, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "gs_track_project": (ctypes.c_int, [P_C, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "gs_mark_visible": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_debug_export": (ctypes.c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_sort_scratch_bytes": (c_size_t, [c_int64]),
    "gs_sort_pairs": (ctypes.c_int, [c_int64, c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "gs_check_plan_header": (ctypes.c_int, [c_void_p, c_int64]),
    "gs_check_ranges": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int64]),
    "gs_check_point_list": (ctypes.c_int, [c_void_p, c_int64, c_int64]),
    "gs_check_walk_order": (ctypes.c_int, [c_void_p, c_int64]),
    "gs_spatial_order_scratch_bytes": (c_size_t, [c_int64]),
    "gs_spatial_order": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_test_wave_reduce": (ctypes.c_int, [ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "gs_timing_enable": (ctypes.c_int, [ctypes.c_int]),
    # include/gs_knn.h
    "gs_knn_workspace_bytes": (c_size_t, [c_int64]),
    "gs_knn": (ctypes.c_int, [c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # include/gs_optim.h
    "gs_adam_step": (ctypes.c_int, [ctypes.POINTER(GsAdamArgs), ctypes.POINTER(GsDensifyStats), c_void_p]),
    # include/gs_neighbor.h
    "gs_neighbor_workspace_bytes": (c_size_t, [c_int64, c_int32, ctypes.c_int]),
    "gs_neighbor_loss_forward": (ctypes.c_int, [P_NG, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_neighbor_loss_backward": (ctypes.c_int, [P_NG, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_void_p]),
    "gs_neighbor_reverse_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "gs_neighbor_reverse": (ctypes.c_int, [c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    # include/gs_loss.h
    "gs_photo_loss_struct_bytes": (c_size_t, []),
    "gs_photo_loss_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "gs_photo_loss_validate": (ctypes.c_int, [ctypes.POINTER(GsPhotoLoss), ctypes.c_int, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "gs_photo_loss_forward": (ctypes.c_int, [ctypes.POINTER(GsPhotoLoss), c_void_p]),
    "gs_photo_loss_backward": (ctypes.c_int, [ctypes.POINTER(GsPhotoLoss), c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    # include/gs_depth_loss.h
    "gs_depth_loss_struct_bytes": (c_size_t, []),
    "gs_depth_loss_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "gs_depth_loss_validate": (ctypes.c_int, [ctypes.POINTER(GsDepthLoss), ctypes.c_int, c_void_p, c_void_p]),
    "gs_depth_loss_forward": (ctypes.c_int, [ctypes.POINTER(GsDepthLoss), c_void_p]),
    "gs_depth_loss_backward": (ctypes.c_int, [ctypes.POINTER(GsDepthLoss), c_void_p, c_void_p, c_void_p]),
    # include/gs_robust_loss.h
    "gs_robust_loss_struct_bytes": (c_size_t, []),
    "gs_robust_loss_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "gs_robust_loss_validate": (ctypes.c_int, [ctypes.POINTER(GsRobustLoss), ctypes.c_int, c_void_p, c_void_p]),
    "gs_robust_loss_forward": (ctypes.c_int, [ctypes.POINTER(GsRobustLoss), c_void_p]),
    "gs_robust_loss_backward": (ctypes.c_int, [ctypes.POINTER(GsRobustLoss), c_void_p, c_void_p, c_void_p]),
    # include/gs_resample.h
    "gs_resample_struct_bytes": (c_size_t, []),
    "gs_resample_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "gs_resample_validate": (ctypes.c_int, [ctypes.POINTER(GsResample), ctypes.c_int, c_void_p, c_void_p]),
    "gs_resample_axis": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "gs_resample_forward": (ctypes.c_int, [ctypes.POINTER(GsResample), c_void_p]),
    "gs_resample_backward": (ctypes.c_int, [ctypes.POINTER(GsResample), c_void_p, c_void_p, c_void_p]),
    # include/gs_feature_decoder.h
    "gs_feature_decoder_struct_bytes": (c_size_t, []),
    "gs_feature_decoder_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gs_feature_decoder_grid_x": (c_int32, [c_int32, c_int32, c_int32]),
    "gs_feature_decoder_n_t": (c_int32, [c_int32]),
    "gs_feature_decoder_n_acc": (c_int64, [c_int32, c_int32, c_int32]),
    "gs_feature_decoder_validate": (ctypes.c_int, [ctypes.POINTER(GsFeatureDecoder), c_int32]),
    "gs_feature_decoder_forward": (ctypes.c_int, [ctypes.POINTER(GsFeatureDecoder), c_void_p]),
    "gs_feature_decoder_loss_forward": (ctypes.c_int, [ctypes.POINTER(GsFeatureDecoder), c_void_p]),
    "gs_feature_decoder_loss_backward": (ctypes.c_int, [ctypes.POINTER(GsFeatureDecoder), c_void_p]),
    "gs_feature_decoder_backward": (ctypes.c_int, [ctypes.POINTER(GsFeatureDecoder), c_void_p]),
    # include/gs_feature_pca.h
    "gs_feature_pca_struct_bytes": (c_size_t, []),
    "gs_feature_pca_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gs_feature_pca_n_acc": (c_int64, [c_int32, c_int32, c_int32]),
    "gs_feature_pca_max_sweeps": (c_int32, []),
    "gs_feature_pca_validate": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_int32]),
    "gs_feature_pca_eig_host": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int32),
                                               ctypes.POINTER(c_int64)]),
    "gs_feature_pca_update": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    "gs_feature_pca_covariance": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    "gs_feature_pca_fit": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    "gs_feature_pca_project": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    "gs_feature_pca_offset": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    "gs_feature_pca_colour": (ctypes.c_int, [ctypes.POINTER(GsFeaturePca), c_void_p]),
    # include/gs_feature_knn.h
    "gs_feature_knn_struct_bytes": (c_size_t, []),
    "gs_feature_knn_splits": (c_int32, [c_int32, c_int32, c_int32, c_int32]),
    "gs_feature_knn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "gs_feature_knn_bound": (ctypes.c_double, [c_int32]),
    "gs_feature_knn_e_pad": (c_int32, [c_int32]),
    "gs_feature_knn_validate": (ctypes.c_int, [ctypes.POINTER(GsFeatureKnn)]),
    "gs_feature_knn": (ctypes.c_int, [ctypes.POINTER(GsFeatureKnn), c_void_p]),
    # include/gs_spectral.h
    "gs_spectral_struct_bytes": (c_size_t, []),
    "gs_spectral_block_width": (c_int32, [c_int32, c_int32]),
    "gs_spectral_workspace_bytes": (c_size_t, [c_int32, c_int64, c_int32]),
    "gs_spectral_validate": (ctypes.c_int, [ctypes.POINTER(GsSpectral)]),
    "gs_spectral_svqb_host": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p]),
    "gs_spectral_ritz_host": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p]),
    "gs_spectral_embedding": (ctypes.c_int, [ctypes.POINTER(GsSpectral), c_void_p]),
    # include/gs_scene_loss.h
    "gs_scene_loss_struct_bytes": (c_size_t, []),
    "gs_scene_loss_workspace_bytes": (c_size_t, [c_int64]),
    "gs_scene_loss_validate": (ctypes.c_int, [ctypes.POINTER(GsSceneLoss), ctypes.c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "gs_scene_loss_forward": (ctypes.c_int, [ctypes.POINTER(GsSceneLoss), c_void_p]),
    "gs_scene_loss_backward": (ctypes.c_int, [ctypes.POINTER(GsSceneLoss), c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "gs_fg_gather_forward": (ctypes.c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "gs_fg_gather_backward": (ctypes.c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    # include/gs_metrics.h
    "gs_image_metrics_struct_bytes": (c_size_t, []),
    "gs_image_metrics_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "gs_image_metrics_validate": (ctypes.c_int, [ctypes.POINTER(GsImageMetrics)]),
    "gs_image_metrics": (ctypes.c_int, [ctypes.POINTER(GsImageMetrics), c_void_p]),
    "gs_mask_iou_validate": (ctypes.c_int, [c_int32, c_int64, c_void_p, c_void_p, c_float, c_void_p]),
    "gs_mask_iou": (ctypes.c_int, [c_int32, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    # include/gs_depth_geometry.h
    "gs_point_depth_struct_bytes": (c_size_t, []),
    "gs_depth_abs_rel_struct_bytes": (c_size_t, []),
    "gs_depth_unproject_struct_bytes": (c_size_t, []),
    "gs_depth_flow_struct_bytes": (c_size_t, []),
    "gs_sample_bilinear_struct_bytes": (c_size_t, []),
    "gs_depth_abs_rel_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "gs_point_depth_validate": (ctypes.c_int, [ctypes.POINTER(GsPointDepth)]),
    "gs_depth_abs_rel_validate": (ctypes.c_int, [ctypes.POINTER(GsDepthAbsRel)]),
    "gs_depth_unproject_validate": (ctypes.c_int, [ctypes.POINTER(GsDepthUnproject)]),
    "gs_depth_flow_validate": (ctypes.c_int, [ctypes.POINTER(GsDepthFlow)]),
    "gs_sample_bilinear_validate": (ctypes.c_int, [ctypes.POINTER(GsSampleBilinear)]),
    "gs_point_depth": (ctypes.c_int, [ctypes.POINTER(GsPointDepth), c_void_p]),
    "gs_depth_abs_rel": (ctypes.c_int, [ctypes.POINTER(GsDepthAbsRel), c_void_p]),
    "gs_depth_unproject": (ctypes.c_int, [ctypes.POINTER(GsDepthUnproject), c_void_p]),
    "gs_depth_flow": (ctypes.c_int, [ctypes.POINTER(GsDepthFlow), c_void_p]),
    "gs_sample_bilinear": (ctypes.c_int, [ctypes.POINTER(GsSampleBilinear), c_void_p]),
    # include/gs_motion_init.h
    "gs_kmeans_assign_struct_bytes": (c_size_t, []),
    "gs_kmeans_update_struct_bytes": (c_size_t, []),
    "gs_coefs_from_centers_struct_bytes": (c_size_t, []),
    "gs_procrustes_struct_bytes": (c_size_t, []),
    "gs_kmeans_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "gs_procrustes_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "gs_kmeans_assign_validate": (ctypes.c_int, [ctypes.POINTER(GsKmeansAssign)]),
    "gs_kmeans_update_validate": (ctypes.c_int, [ctypes.POINTER(GsKmeansUpdate)]),
    "gs_coefs_from_centers_validate": (ctypes.c_int, [ctypes.POINTER(GsCoefsFromCenters)]),
    "gs_procrustes_validate": (ctypes.c_int, [ctypes.POINTER(GsProcrustes)]),
    "gs_kmeans_assign": (ctypes.c_int, [ctypes.POINTER(GsKmeansAssign), c_void_p]),
    "gs_kmeans_update": (ctypes.c_int, [ctypes.POINTER(GsKmeansUpdate), c_void_p]),
    "gs_coefs_from_centers": (ctypes.c_int, [ctypes.POINTER(GsCoefsFromCenters), c_void_p]),
    "gs_procrustes": (ctypes.c_int, [ctypes.POINTER(GsProcrustes), c_void_p]),
    # include/gs_densify.h
    "gs_densify_plan_struct_bytes": (c_size_t, []),
    "gs_densify_tensor_struct_bytes": (c_size_t, []),
    "gs_densify_apply_struct_bytes": (c_size_t, []),
    "gs_densify_workspace_bytes": (c_size_t, [c_int64]),
    "gs_densify_counts_offset": (c_size_t, [c_int64]),
    "gs_densify_flags_offset": (c_size_t, [c_int64]),
    "gs_densify_ranks_offset": (c_size_t, [c_int64]),
    "gs_densify_scan_block": (c_int64, []),
    "gs_densify_scan_tile": (c_int64, []),
    "gs_densify_new_count": (c_int64, [ctypes.POINTER(c_int64), c_int32]),
    "gs_densify_plan_validate": (ctypes.c_int, [ctypes.POINTER(GsDensifyPlanArgs)]),
    "gs_densify_apply_validate": (ctypes.c_int, [ctypes.POINTER(GsDensifyApplyArgs)]),
    "gs_densify_plan": (ctypes.c_int, [ctypes.POINTER(GsDensifyPlanArgs), c_void_p]),
    "gs_densify_apply": (ctypes.c_int, [ctypes.POINTER(GsDensifyApplyArgs), c_void_p]),
    # include/gs_motion.h
    "gs_motion_struct_bytes": (c_size_t, []),
    "gs_motion_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32, ctypes.c_int]),
    "gs_motion_backward_block": (c_int32, [c_int32, c_int32]),
    "gs_motion_forward_validate": (ctypes.c_int, [ctypes.POINTER(GsMotionDesc), c_void_p, c_void_p, c_void_p]),
    "gs_motion_backward_validate": (ctypes.c_int, [ctypes.POINTER(GsMotionDesc), c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_motion_forward": (ctypes.c_int, [ctypes.POINTER(GsMotionDesc), c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_motion_backward": (ctypes.c_int, [ctypes.POINTER(GsMotionDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "gs_timing_select": (ctypes.c_int, [ctypes.c_uint32]),
    "gs_timing_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int64),
                                      ctypes.c_int]),
}

STAGES = ["preprocess", "scan", "duplicate", "sort", "ranges", "render_fwd", "render_bwd",
          "preprocess_bwd"]


def timing_enable(on: bool = True, stages=None):
    """Enable/disable live stage timing; `stages` (names) restricts it."""
    L = load()
    mask = 0xFFFFFFFF if stages is None else sum(1 << STAGES.index(s) for s in stages)
    L.gs_timing_select(mask)
    L.gs_timing_enable(1 if on else 0)


def timing_read() -> dict:
    """{stage: (total_ms, launches)} since the last timing_enable()."""
    n = len(STAGES)
    ms = (ctypes.c_double * n)()
    cnt = (c_int64 * n)()
    check(load().gs_timing_read(ms, cnt, n), "timing read")
    return {s: (ms[i], cnt[i]) for i, s in enumerate(STAGES)}


class GsplatError(RuntimeError):
    pass


def lib_path() -> str:
    return _build.LIB


def load(auto_build: bool = True):
    """Load libgsplat_hip.so (building it first if stale and hipcc is present)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.LIB
        if auto_build:
            try:
                if _build.is_stale():
                    _build.build()
            except RuntimeError:
                if not os.path.exists(path):
                    raise
        if not os.path.exists(path):
            raise GsplatError(
                f"libgsplat_hip.so not found at {path}; build it with "
                "`python -m dynamic3dgaussians_amd.build` (requires ROCm hipcc). "
                "There is no CPU fallback.")
        L = ctypes.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.gs_version() != ABI_VERSION:
            raise GsplatError(f"ABI version mismatch: library reports {L.gs_version()}")
        _lib = L
        return L


def stream(device) -> int:
    """The gs_stream_t of a call: the device's current torch stream."""
    return torch.cuda.current_stream(device).cuda_stream


def check(code: int, what: str):
    if code != 0:
        msg = load().gs_last_error().decode(errors="replace")
        raise GsplatError(f"{what} failed (status {code}): {msg}")
