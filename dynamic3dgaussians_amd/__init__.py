"""dynamic3dgaussians_amd -- MI355X-native (gfx950, HIP) differentiable 3D-Gaussian
rasterizer, a drop-in for Dynamic3DGaussians' `diff_gaussian_rasterization`.

Layout:
  csrc/           hand-written HIP kernels + the C ABI (include/gsplat_hip.h)
  build.py        hipcc build of lib/libgsplat_hip.so and of the rasterizer's C++ binding (in-tree)
  _lib.py         loads the library: ctypes mirrors of the C ABI (fails loudly; no CPU fallback)
  _C.py           positional mirror of the reference pybind module `_C`, over csrc/gs_torch_binding.cpp
  rasterizer.py   autograd boundary (GaussianRasterizer & friends)
  camera.py       helpers.setup_camera restatement + synthetic camera rig + PoseRefiner (trainable poses for the
                  rasterizer's differentiable camera tensors, include/gs_camera_grad.h)
  scene.py        synthetic scenes for tests and the benchmark
  distributed.py  camera-sharded data parallelism with one RCCL all-reduce
  image_loss.py   the reference's L1 + SSIM photometric loss, fused (include/gs_loss.h)
  depth_loss.py   the reference's masked depth-correlation (Pearson) loss, fused (include/gs_depth_loss.h)
  robust_loss.py  the reference's quantile-trimmed squared losses and a batched exact quantile: radix select,
                  no sort (include/gs_robust_loss.h)
  resample.py     the reference's bilinear F.interpolate to a prior's size, deterministic (include/gs_resample.h)
  feature_loss.py the reference's feature-distillation loss: resample to the prior, then L1 (+ SSIM)
  feature_decoder.py the reference's "speedup" 1x1 decoder fused with the L1 loss on the matrix cores
                  (include/gs_feature_decoder.h)
  feature_pca.py  the reference's PCA colouring of feature maps: moments on the matrix cores, an on-device
                  eigensolve, project / range / colour (include/gs_feature_pca.h)
  feature_knn.py  exact cosine top-k neighbours in feature space: candidates on the matrix cores, an fp64 rerank
                  with a certificate, an exhaustive fp64 search for the rest (include/gs_feature_knn.h)
  spectral.py     spectral embedding and clustering of the feature kNN graph: Chebyshev-filtered subspace
                  iteration, fp64, nothing read back (include/gs_spectral.h)
  densify.py      the reference's clone / split / prune with the Adam state (include/gs_densify.h)
  scene_loss.py   the reference's floor / bg / soft_col_cons terms and its foreground split, no host syncs
                  (include/gs_scene_loss.h)
  metrics.py      the reference's quality reports: masked PSNR, masked SSIM, mask IoU (include/gs_metrics.h),
                  pose errors, PCK, the mMDE depth error
  depth_geometry.py  geometry on depth maps: point z-buffer and abs-rel score, unprojection, depth-induced flow,
                  bilinear border sampling, flow warping and chaining, track lifting (include/gs_depth_geometry.h)
  tracking.py     point tracking: top-K contributor maps, track projection, visibility (include/gs_track.h)
  motion.py       the reference's motion-basis warp: SE(3) basis blend, fused (include/gs_motion.h)
  motion_init.py  the motion bases' initialisation: k-means, per-cluster medians, coefficients, one weighted
                  Procrustes solve per (basis, frame) (include/gs_motion_init.h)
"""
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, GradientSink,  # noqa: F401
                         _RasterizeGaussians, rasterize_gaussians)
from ._C import set_default_compat, get_default_compat  # noqa: F401
from .image_loss import photometric_image_loss, photometric_loss, photometric_loss_torch  # noqa: F401
from .depth_loss import depth_correlation_loss, depth_correlation_loss_torch  # noqa: F401
from .robust_loss import (masked_trimmed_mse_loss, masked_trimmed_mse_loss_torch, plane_quantile,  # noqa: F401
                          plane_quantile_torch, trimmed_mse_loss, trimmed_mse_loss_torch)
from .resample import bilinear_resize, bilinear_resize_torch  # noqa: F401
from .feature_loss import decoded_distillation_loss, distillation_image_loss, feature_distillation_loss  # noqa: F401
from .feature_decoder import (FeatureDecoder, decode_features, decode_features_torch, decoded_l1_loss,  # noqa: F401
                              decoded_l1_loss_torch)
from .feature_pca import (FeaturePCA, FeaturePCATorch, feature_map, feature_map_pca, feature_map_torch,  # noqa: F401
                          fit_sequence, fit_sequence_torch, pca_colour, pca_colour_torch, pca_covariance_torch,
                          pca_eig_torch, pca_moments_torch, pca_project, pca_project_torch, pca_range_torch)
from .feature_knn import (cosine_topk, feature_knn, feature_knn_candidates, feature_knn_torch,  # noqa: F401
                          knn_affinity)
# `densify` here is the function; its module (schedule, plan, classify_torch, ...) is
# importlib.import_module('dynamic3dgaussians_amd.densify')
from .densify import densify, densify_torch  # noqa: F401
from .scene_loss import (foreground_split, gather_foreground, reference_extra_loss, regularizer_losses,  # noqa: F401
                         regularizer_losses_torch)
from .metrics import (PCK, ImageMetrics, MaskedPSNR, MaskedSSIM, MaskIoU, MeanDepthError, MeanIoU,  # noqa: F401
                      evaluate_cameras, evaluate_sequence, image_metrics, image_metrics_torch, iou, mask_iou,
                      mask_iou_torch, pose_errors, psnr_clamped, psnr_masked, psnr_plain)
from .depth_geometry import (accumulate_flows, accumulate_flows_torch, depth_abs_rel, depth_abs_rel_torch,  # noqa: F401
                             depth_flow, depth_flow_torch, lift_tracks, lift_tracks_torch, point_depth_maps,
                             point_depth_maps_torch, resize_flow, resize_flow_torch, sample_bilinear,
                             sample_bilinear_torch, unproject_depth, unproject_depth_torch, warp_flow,
                             warp_flow_torch)
from .tracking import (Tracks, contributor_maps, project_tracks, project_tracks_torch, select_gaussians,  # noqa: F401
                       track_points, visible_in_maps)
from .camera import PoseRefiner  # noqa: F401
from .motion import (MotionBases, cont_6d_to_rmat, motion_positions, motion_positions_torch,  # noqa: F401
                     motion_transforms)
from .motion_init import (KMeansResult, MotionInit, ProcrustesInit, cluster_medians, cluster_medians_torch,  # noqa: F401
                          coefs_from_centers, coefs_from_centers_torch, init_motion_bases_from_tracks,
                          init_motion_coefs_from_features, kmeans, kmeans_assign, kmeans_assign_torch, kmeans_torch,
                          kmeans_update, kmeans_update_torch, solve_procrustes_bases,
                          solve_procrustes_bases_torch, velocity_directions)
from .spectral import (SpectralClustering, SpectralEmbedding, graph_check, knn_graph, spectral_clustering,  # noqa: F401
                       spectral_clustering_graph, spectral_embedding, spectral_embedding_dense,
                       spectral_embedding_torch)

__version__ = "0.1.0"
