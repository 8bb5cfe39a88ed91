/* gs_motion_init.h -- C ABI of the motion-basis initialisation: Lloyd's
 * k-means (assign, update), the basis coefficients from cluster centres and
 * the weighted Procrustes solve per (basis, frame).  Exported by the same
 * libgsplat_hip.so as gsplat_hip.h.  Forward only.
 *
 * Replaces the host code (scikit-learn and Python loops over clusters and
 * frames) of the reference's init_motion_params_with_procrustes
 * (dyn_som.py:25-135), its k-means on velocity directions
 * (motion_utils.py:219-244) and feature_bases (motion_utils.py:57-162).
 * Parity unpinned: dyn_som.py is a fragment that cannot be imported; the
 * semantics are the ones DESIGN.md 9.16 fixes, stated in PyTorch by the
 * _torch twins of dynamic3dgaussians_amd/motion_init.py.
 *
 * Conventions.  Device data is contiguous; points, centres, tracks and weights
 * are fp32, labels, counts and ids are int64.  Every struct shares its name
 * with its entry point.  Every call is asynchronous on `stream`, reads nothing
 * back, allocates nothing, uses no floating-point atomic (two calls give the
 * same bits) and returns 0 or an error code with gs_last_error() set.  Each
 * call runs its _validate function (host code, no device access) first.
 *
 * gs_kmeans_assign: labels[i] = argmin_k sum_d (x[i][d] - centers[k][d])^2,
 * the difference form, added over d in index order in fp32 without
 * contraction; ties go to the lowest k.  With `valid` (one byte per point) a
 * point whose byte is 0 gets label -1.  With `prev_labels` and `moved` the
 * number of points whose label differs from prev_labels is added to *moved
 * (one 64-bit integer atomic per workgroup; the caller zeroes it).  The
 * centres pass through LDS in chunks of 32 dimensions, a thread owns a point
 * and keeps one accumulator per centre.  Bytes: 4 N D read, 8 N written;
 * flops: 3 N K D (K rounded up to 8, 16, 32 or 64 in the kernel).
 *
 * gs_kmeans_update: centers[k] = the mean of the points with label k, the sum
 * taken in fp64 in a fixed order and rounded to fp32 once; counts[k] their
 * number.  A cluster without a member keeps its centre bit for bit and
 * reports 0 (scikit-learn relocates it; documented difference).  Labels
 * outside [0, K) are ignored.  Two stages: a workgroup (one wave, a lane per
 * dimension of a 64-dimension chunk) walks its contiguous slice of points in
 * order into its own fp64 LDS column per cluster and writes the partial sums
 * [block][K][D] and counts [block][K]; a second kernel adds the blocks in
 * index order.  Bytes: 4 N D + 8 N read, 8 blocks K D written and read again.
 *
 * gs_coefs_from_centers: coefs[i][k] = 10 exp(-|means[i] - centers[k]|), a
 * thread per point.
 *
 * gs_procrustes: for basis n and frame t, over the points listed for n
 * (order[offsets[n] .. offsets[n + 1]), ids into tracks; a stable sort of the
 * ids by label gives a fixed order), with
 *
 *   w_i = W[i][cano_t] W[i][t] (conf[i][cano_t] + conf[i][t]) / 2
 *
 * (W = weights or 1, conf = confidences or 1), 19 fp64 moments are added in a
 * fixed order from the fp32 inputs: sum w, sum w s, sum w g, sum w s g^T,
 * sum w |s|^2, sum w |g|^2 and sum w |s - g|^2, with s = tracks[i][cano_t]
 * and g = tracks[i][t].  One thread per basis then walks the frames in the
 * order cano_t - 1, ..., 0, cano_t, ..., T - 1; prev_t starts at cano_t and
 * is afterwards the frame visited before; everything starts at the identity.
 * If sum w < min_weight_sum the frame copies prev_t's rotation and
 * translation, skipped = 1 and both errors are -1.  Otherwise the proper
 * rotation R and translation t minimising sum w |R s + t - g|^2 come from
 * Horn's symmetric 4 x 4 matrix of the centred cross-covariance: its largest
 * eigenvector, by cyclic Jacobi sweeps in fp64, is the quaternion (w, x, y,
 * z), so det R = +1 always.  t = cg - R cs maps the weighted source centroid
 * onto the target's.  err_after = sqrt(sum w |R s + t - g|^2 / sum w), added
 * directly in a second pass over the points with the fp64 (R, t) (its
 * expansion in the moments cancels where the residual is near zero),
 * err_before = sqrt(sum w |s - g|^2 / sum w).  rot_dim 4 writes the
 * quaternion with the sign that is nearer to prev_t's; rot_dim 6 writes
 * (R[:, 0], R[:, 1]).  A rank-deficient cluster gives some finite proper
 * rotation. */
#ifndef GS_MOTION_INIT_H
#define GS_MOTION_INIT_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_KMEANS_MAX_K 64 /* GS_MOTION_MAX_K of gs_motion.h */

struct gs_kmeans_assign {
  int64_t N;                  /* points (>= 0) */
  int32_t D, K;               /* dimensions (>= 1), centres (1 .. 64) */
  const float *x;             /* [N, D]; may be NULL when N == 0 */
  const float *centers;       /* [K, D] */
  const uint8_t *valid;       /* optional [N]: 0 gives label -1 */
  const int64_t *prev_labels; /* optional [N] */
  int64_t *labels;            /* [N] */
  int64_t *moved;             /* optional (with prev_labels): += labels that differ */
};

struct gs_kmeans_update {
  int64_t N;                /* points (>= 0) */
  int32_t D, K;             /* dimensions (>= 1), centres (1 .. 64) */
  const float *x;           /* [N, D]; may be NULL when N == 0 */
  const int64_t *labels;    /* [N]; outside [0, K) is ignored */
  float *centers;           /* [K, D] in and out: an empty cluster's row is not written */
  int64_t *counts;          /* [K] */
  void *workspace;          /* gs_kmeans_workspace_bytes(N, K, D) bytes */
  uint64_t workspace_bytes; /* size of the buffer behind `workspace` */
};

struct gs_coefs_from_centers {
  int64_t N;            /* points (>= 0) */
  int32_t K;            /* centres (>= 1) */
  int32_t _pad;
  const float *means;   /* [N, 3]; may be NULL when N == 0 */
  const float *centers; /* [K, 3] */
  float *coefs;         /* [N, K] */
};

struct gs_procrustes {
  int64_t N;                /* tracks (>= 0) */
  int32_t T, K;             /* frames (>= 1), bases (1 .. 64) */
  int32_t cano_t;           /* the canonical frame, in [0, T) */
  int32_t rot_dim;          /* 4: quaternion (w, x, y, z); 6: (R[:, 0], R[:, 1]) */
  double min_weight_sum;    /* a frame with sum w below this copies the previous one */
  const float *tracks;      /* [N, T, 3]; may be NULL when N == 0 */
  const int64_t *order;     /* [N] ids sorted by basis; entries outside [0, N) are skipped */
  const int64_t *offsets;   /* [K + 1] ranges of `order` per basis, clamped to [0, N] */
  const float *weights;     /* optional [N, T] */
  const float *confidences; /* optional [N, T] */
  float *rots;              /* [K, T, rot_dim] */
  float *transls;           /* [K, T, 3] */
  float *err_after;         /* [K, T] */
  float *err_before;        /* [K, T] */
  uint8_t *skipped;         /* [K, T] */
  void *workspace;          /* gs_procrustes_workspace_bytes(K, T) bytes */
  uint64_t workspace_bytes; /* size of the buffer behind `workspace` */
};

/* sizeof each struct as the library was compiled (for binding mirrors). */
size_t gs_kmeans_assign_struct_bytes(void);
size_t gs_kmeans_update_struct_bytes(void);
size_t gs_coefs_from_centers_struct_bytes(void);
size_t gs_procrustes_struct_bytes(void);

/* Workspace of one gs_kmeans_update call: the fp64 partial sums and the
 * counts of every block of points.  0 outside the limits. */
size_t gs_kmeans_workspace_bytes(int64_t N, int32_t K, int32_t D);
/* Workspace of one gs_procrustes call: 19 fp64 moments and the fp64 (R, t) per (basis, frame). */
size_t gs_procrustes_workspace_bytes(int32_t K, int32_t T);

/* The argument checks the entry points run first (host code, no device access). */
int gs_kmeans_assign_validate(const struct gs_kmeans_assign *args);
int gs_kmeans_update_validate(const struct gs_kmeans_update *args);
int gs_coefs_from_centers_validate(const struct gs_coefs_from_centers *args);
int gs_procrustes_validate(const struct gs_procrustes *args);

int gs_kmeans_assign(const struct gs_kmeans_assign *args, gs_stream_t stream);
int gs_kmeans_update(const struct gs_kmeans_update *args, gs_stream_t stream);
int gs_coefs_from_centers(const struct gs_coefs_from_centers *args, gs_stream_t stream);
int gs_procrustes(const struct gs_procrustes *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_MOTION_INIT_H */
