// gs_feature_pca_layout.h -- sizes, grid rules and workspace layouts of the
// feature-map PCA (include/gs_feature_pca.h), written once for the kernels
// (gs_feature_pca.hip) and the host-only validator (gs_feature_pca_host.cpp).
// Plain C++ on the host, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/gs_feature_pca.h"

namespace gs {

constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = 4;
constexpr int FP_PIX = GS_FPCA_TILE_PIXELS;        // pixels per step of the moments kernels
constexpr int FP_LD = FP_PIX + 4;                  // LDS row stride in floats (16-byte aligned rows)
constexpr int FP_CHUNK = GS_FPCA_CHUNK;            // pixels per block = per slab
constexpr int FP_STEPS = FP_CHUNK / FP_PIX;
constexpr int FP_GROUP = GS_FPCA_SLAB_GROUP;
constexpr int FP_PROJ_PIX = 256;                   // pixels per block of project / offset / colour
constexpr int FP_EIG_THREADS = 512;
constexpr int FP_EIG_LDS_ORDER = GS_FPCA_LDS_MAX_C;

inline bool fp_sizes_ok(int64_t B, int64_t C, int64_t H, int64_t W) {
  return B >= 1 && B <= 65535 && C >= 1 && C <= GS_FPCA_MAX_C && H >= 1 && W >= 1 && H * W < 2147483647LL - FP_CHUNK;
}
inline bool fp_k_ok(int64_t C, int64_t k) { return k >= 1 && k <= GS_FPCA_MAX_K && k <= C; }
inline int fp_channel_tiles(int C) { return (C + 31) / 32; }
inline int64_t fp_chunks(int64_t H, int64_t W) { return (H * W + FP_CHUNK - 1) / FP_CHUNK; }
inline int64_t fp_proj_blocks(int64_t H, int64_t W) { return (H * W + FP_PROJ_PIX - 1) / FP_PROJ_PIX; }
constexpr int fp_even(int C) { return C + (C & 1); }  // constexpr: also callable in the kernels
inline size_t fp_pad16(size_t n) { return (n + 15) / 16 * 16; }

// update: the slabs [slabs][C*C + C + 1] floats, their group sums [groups][..]
// doubles, and the same pair for the shift pass ([slabs][C + 1] doubles).
struct FeaturePcaUpdateLayout {
  size_t off_slabs, off_groups, off_mean, off_mean_groups, total;  // bytes
  int64_t chunks, slabs, groups, slab_elems;
  FeaturePcaUpdateLayout(int64_t B, int C, int64_t H, int64_t W) {
    chunks = fp_chunks(H, W);
    slabs = chunks * B;
    groups = (slabs + FP_GROUP - 1) / FP_GROUP;
    slab_elems = (int64_t)C * C + C + 1;
    size_t o = 0;
    off_slabs = o;
    o += fp_pad16((size_t)slabs * slab_elems * sizeof(float));
    off_groups = o;
    o += fp_pad16((size_t)groups * slab_elems * sizeof(double));
    off_mean = o;
    o += fp_pad16((size_t)slabs * (C + 1) * sizeof(double));
    off_mean_groups = o;
    o += fp_pad16((size_t)groups * (C + 1) * sizeof(double));
    total = o;
  }
};

// fit: A and V [ne, ne + 1] doubles (an odd leading dimension) above the LDS order, nothing below.
constexpr int fp_eig_ld(int C) { return fp_even(C) + 1; }
inline size_t fp_fit_workspace(int C) {
  const size_t ne = (size_t)fp_even(C);
  return C > FP_EIG_LDS_ORDER ? 2 * ne * fp_eig_ld(C) * sizeof(double) : 0;
}
// project: the blocks' minima and maxima [B][blocks][k][2] floats.
inline size_t fp_project_workspace(int64_t B, int64_t H, int64_t W, int k) {
  return fp_pad16((size_t)B * fp_proj_blocks(H, W) * k * 2 * sizeof(float));
}

}  // namespace gs
