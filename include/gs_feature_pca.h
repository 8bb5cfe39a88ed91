/* gs_feature_pca.h -- C ABI of the feature-map PCA colouring, exported by the
 * same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces what the reference does with a rendered semantic_feature map when
 * somebody wants to look at it (utils/image_utils.py:27-58 feature_map;
 * sanity_feature.py:570-591, sanity_visuals.py:80-108, sanity_get_pca_feat*.py;
 * sanity_visuals_along_temporal*.py:56-129): a PCA over the channels, every
 * pixel projected onto the top three components, rescaled to [0, 1] and saved
 * as RGB -- without the device-to-host copy and the [n, C] transpose.
 *
 *   x      [B, C, H, W]   planar contiguous fp32, p over the H * W pixels
 *   mask   [H, W] or [B, H, W] bytes, optional (NULL: every pixel); a pixel
 *          takes part iff its byte is non-zero
 *
 * Arithmetic (fl32 = one fp32 rounding; built with -ffp-contract=off so every
 * product and sum below rounds as written):
 *
 *   xh[c]    = normalize ? x[c] / max(sqrt(sum_c x[c]^2), 1e-12) : x[c]   (fp32, the
 *              squares added in channel order; F.normalize(dim=1))
 *   fit set  = pixels with mask != 0 and flat index p % sample_stride == 0
 *
 * update (moments).  x' = fl32(xh - shift) on the fit set, 0 elsewhere.
 *   state[0]          n  += |fit set|
 *   state[1 + c]      S  += sum x'[c]
 *   state[1 + C + ..] M  += sum x' x'^T           (row-major [C, C], stored symmetric)
 * all fp64.  With compute_shift the call first sets shift[c] = fl32(sum xh[c] / n)
 * over its own fit set (fp64 partials per block, summed in block order; 0 for
 * an empty set).  The Gram matrix runs on the matrix cores and is
 * fp32-equivalent: x' is split into three bf16 pieces, six piece products per
 * 32x32x16 step accumulated in fp32 (gs_split_mfma.h).  A block takes one run
 * of at most GS_FPCA_CHUNK consecutive pixels of one image, GS_FPCA_TILE_PIXELS
 * per step, and writes one slab of C*C + C + 1 floats (the upper triangle of M,
 * S, n); so one fp32 accumulator sees at most gs_feature_pca_n_acc(B, H, W) =
 * min(GS_FPCA_CHUNK, H*W rounded up to the tile) pixels.  The slabs are summed
 * in fp64 in slab order (groups of GS_FPCA_SLAB_GROUP, then the groups) and
 * added to the state.  Only tiles with row tile <= column tile are computed
 * (a diagonal tile uses the same registers for both operands); M[i][j] and
 * M[j][i] are both read from the slab's upper entry.  No atomics: reruns are
 * bit-identical.
 *
 * covariance.  d = S / n, mean = shift + d, cov = (M - (n d) d^T) / (n - ddof),
 *   fp64; all zeros (mean = shift) when n <= ddof.
 *
 * fit.  One workgroup diagonalises cov with the cyclic Jacobi of
 *   csrc/gs_sym_eig.h (fp64, round-robin ordering, at most GS_FPCA_MAX_SWEEPS
 *   sweeps, leaves when off(A) <= 2^-52 ||A||_F).  Eigenpairs sorted by
 *   descending eigenvalue (ties: lower index first); each eigenvector's sign
 *   makes its entry of largest magnitude positive (lowest index on a tie;
 *   sklearn's svd_flip(u_based_decision=False)).
 *   status: 0 ok, 1 n <= ddof, 2 the sweep cap was reached, 3 the covariance is
 *   not finite (a NaN or infinite pixel took part, or its squares overflow
 *   fp64); with a non-zero status components / components_f32 are zeros, never
 *   NaN (with 1 and 3 evals and evecs are zeros too).
 *
 * project.  t[b,j,p] = sum_c fl32(xh[c] - mean[c]) * V[j,c], fp32, channel order,
 *   0 where the mask is 0.  tmin / tmax [B, k]: min / max of t over the pixels
 *   with mask != 0 (every pixel, whatever sample_stride), 0 / 0 for none; from
 *   per-block partials reduced in a fixed order (minima and maxima: any order gives
 *   the same bits).
 *
 * offset.  u = fl32(t - sub[b,j])  (the quantile range's non-negative planes).
 *
 * colour.  v = (t - lo[b,j]) / (hi[b,j] - lo[b,j]) in fp64 from the fp32 t, 0 where
 *   hi == lo and where the mask is 0; clamp: v = min(max(v, 0), 1).
 *   out_uint8: out [B, H, W, 3] bytes trunc(255 min(max(v, 0), 1)); else out
 *   [B, 3, H, W] floats fl32(v).  k must be 3.
 *
 * Limits: 1 <= C <= GS_FPCA_MAX_C, 1 <= k <= min(C, GS_FPCA_MAX_K), 1 <= B <=
 * 65535, H * W < 2^31 - GS_FPCA_CHUNK.  Plane offsets are 64-bit.
 * Byte models per pixel: update 4 C read (+ 1 mask), twice with compute_shift;
 * project 4 C read + 4 k written; colour 4 k read + 3 written.
 *
 * All calls are asynchronous on `stream`, read nothing back, and return 0 or
 * an error code with gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_FEATURE_PCA_H
#define GS_FEATURE_PCA_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_FPCA_MAX_C 128
#define GS_FPCA_MAX_K 8
#define GS_FPCA_MAX_SWEEPS 24
#define GS_FPCA_TILE_PIXELS 128
#define GS_FPCA_CHUNK 4096
#define GS_FPCA_SLAB_GROUP 64
#define GS_FPCA_LDS_MAX_C 64 /* the eigensolve's matrices are in LDS up to here, in the workspace above */

/* `pass` of gs_feature_pca_workspace_bytes / gs_feature_pca_validate. */
#define GS_FPCA_PASS_UPDATE 0
#define GS_FPCA_PASS_COVARIANCE 1
#define GS_FPCA_PASS_FIT 2
#define GS_FPCA_PASS_PROJECT 3
#define GS_FPCA_PASS_OFFSET 4
#define GS_FPCA_PASS_COLOUR 5

typedef struct gs_feature_pca {
  int32_t B, C, H, W;
  int32_t k;                   /* components (fit, project, offset, colour) */
  int32_t mask_per_image;      /* 0: mask is [H, W]; else [B, H, W] */
  int32_t normalize;           /* update, project */
  int32_t sample_stride;       /* update, >= 1 */
  int32_t ddof;                /* covariance, fit, >= 0 */
  int32_t compute_shift;       /* update: set shift from this call's fit set first */
  int32_t out_uint8, clamp;    /* colour */
  const float *x;              /* [B, C, H, W] (update, project) */
  const uint8_t *mask;         /* see mask_per_image, or NULL (update, project, colour) */
  float *shift;                /* [C] (update: read, written with compute_shift; covariance, fit: read) */
  double *state;               /* [1 + C + C*C] n, S, M (update: added to; covariance, fit: read) */
  double *mean;                /* [C] (covariance, fit) */
  double *cov;                 /* [C, C] (covariance) */
  double *evals;               /* [C] descending (fit) */
  double *evecs;               /* [C, C], row j the j-th eigenvector (fit) */
  double *components;          /* [k, C] = the first k rows of evecs (fit) */
  float *components_f32;       /* [k, C] its fp32 rounding (fit) */
  float *mean_f32;             /* [C] (fit) */
  int32_t *status;             /* [1] (fit) */
  const float *proj_components; /* [k, C] (project) */
  const float *proj_mean;      /* [C] (project) */
  float *t;                    /* [B, k, H, W] (project: written; offset, colour: read) */
  float *tmin, *tmax;          /* [B, k] (project) */
  const float *sub;            /* [B, k] (offset) */
  float *u;                    /* [B, k, H, W] (offset) */
  const double *lo, *hi;       /* [B, 3] (colour) */
  void *out;                   /* colour: [B, H, W, 3] bytes or [B, 3, H, W] floats */
  void *workspace;             /* gs_feature_pca_workspace_bytes bytes, 16-byte aligned */
  uint64_t workspace_bytes;
} gs_feature_pca;

/* sizeof(gs_feature_pca) as the library was compiled (for binding mirrors). */
size_t gs_feature_pca_struct_bytes(void);

/* Workspace of one pass (0 for sizes out of range, and for the passes that use none). */
size_t gs_feature_pca_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t pass);

/* The pixels behind one fp32 accumulator of a slab; the compiled sweep cap.  0 for sizes out of range. */
int64_t gs_feature_pca_n_acc(int32_t B, int32_t H, int32_t W);
int32_t gs_feature_pca_max_sweeps(void);

/* The argument check every entry point runs first (host code, no device access). */
int gs_feature_pca_validate(const gs_feature_pca *args, int32_t pass);

/* The host build of csrc/gs_sym_eig.h on the symmetric A [C, C] (row-major, C <= GS_FPCA_MAX_C):
 * evals [C] and evecs [C, C] sorted and signed as fit's, the sweeps it took and the rotations it
 * applied.  Returns fit's status (0, 2 or 3), or an error code. */
int gs_feature_pca_eig_host(int32_t C, const double *A, double *evals, double *evecs, int32_t *sweeps,
                            int64_t *rotations);

int gs_feature_pca_update(const gs_feature_pca *args, gs_stream_t stream);
int gs_feature_pca_covariance(const gs_feature_pca *args, gs_stream_t stream);
int gs_feature_pca_fit(const gs_feature_pca *args, gs_stream_t stream);
int gs_feature_pca_project(const gs_feature_pca *args, gs_stream_t stream);
int gs_feature_pca_offset(const gs_feature_pca *args, gs_stream_t stream);
int gs_feature_pca_colour(const gs_feature_pca *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_FEATURE_PCA_H */
