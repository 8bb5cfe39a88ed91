/* gs_motion.h -- C ABI of the motion-basis warp (a per-Gaussian blend of K
 * shared SE(3) trajectories), exported by the same libgsplat_hip.so as
 * gsplat_hip.h.
 *
 * Replaces the PyTorch chain of the reference's motion-basis scene
 * (dyn_train.py:410-431, MotionBases.compute_transforms external.py:47-58,
 * cont_6d_to_rmat motion_utils.py:10-22) by one launch forward and three
 * backward.  For Gaussian g and the b-th requested frame t = ts[b]:
 *
 *   c        = coefs[g, :]                       (coef_mode 0)
 *            = softmax(coefs[g, :])              (coef_mode 1, max-subtracted)
 *   r6       = sum_k c[k] rots[k, t, :]          t3 = sum_k c[k] transls[k, t, :]
 *   x        = r6[0:3] / max(|r6[0:3]|, 1e-12)
 *   u        = r6[3:6] - (r6[3:6] . x) x         y = u / max(|u|, 1e-12)
 *   z        = x cross y
 *   transforms[g, b] = [x y z t3]                (3 x 4, x y z are COLUMNS)
 *   positions[g, b]  = [x y z] means[g] + t3
 *
 * The backward writes (never accumulates) d_means, d_coefs (in mode 1 the
 * gradient of the logits) and the basis tables' gradients d_rots [K, T, 6] and
 * d_transls [K, T, 3]: rows of frames not in ts are zero, a frame that appears
 * more than once in ts receives the sum of its occurrences in ascending b.
 * The sum over the Gaussians is taken per workgroup into partial slabs in the
 * workspace and over the slabs in a second pass, both in a fixed order with
 * fp32 adds and no atomics: the same inputs give the same bits.  At a
 * degenerate blend (a zero vector, parallel halves) the forward is defined by
 * the clamps above; the backward there is not specified.
 *
 * Everything is fp32, contiguous device memory, 4-byte aligned (the
 * transforms move as 16-byte vectors where their pointer allows, as scalars
 * otherwise).  ts is HOST memory inside the descriptor and travels to the
 * kernels by value: no device read, no synchronisation.  All calls are
 * asynchronous on `stream`; they return 0 or an error code with
 * gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_MOTION_H
#define GS_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_MOTION_MAX_K 64 /* bases per call */
#define GS_MOTION_MAX_B 32 /* frames per call */

#define GS_MOTION_COEFS_GIVEN 0  /* coefs are used as they are */
#define GS_MOTION_COEFS_LOGITS 1 /* coefs are logits: row softmax over K inside the kernels */

typedef struct gs_motion_desc {
  int64_t G;                   /* Gaussians (>= 0) */
  int32_t K;                   /* bases, 1 .. GS_MOTION_MAX_K */
  int32_t T;                   /* frames of the tables (> 0) */
  int32_t B;                   /* frames of this call, 1 .. GS_MOTION_MAX_B */
  int32_t coef_mode;           /* GS_MOTION_COEFS_* */
  const float *rots;           /* [K, T, 6] */
  const float *transls;        /* [K, T, 3] */
  const float *coefs;          /* [G, K] */
  const float *means;          /* [G, 3], or NULL when only transforms are wanted */
  int32_t ts[GS_MOTION_MAX_B]; /* the first B: frame indices, 0 <= ts[b] < T (host memory) */
} gs_motion_desc;

/* sizeof(gs_motion_desc) as the library was compiled (for binding mirrors). */
size_t gs_motion_struct_bytes(void);

/* Workspace of one call.  The forward needs none (0); the backward keeps the
 * per-workgroup partial slabs [workgroups, B, K, 9] and their sum there.
 * 0 outside the envelope and for G <= 0. */
size_t gs_motion_workspace_bytes(int64_t G, int32_t K, int32_t B, int backward);
/* Gaussians per workgroup of the backward at this K and B (for tests of the
 * cross-workgroup sum). */
int32_t gs_motion_backward_block(int32_t K, int32_t B);

/* The argument checks the two entry points run first (host code, no device
 * access). */
int gs_motion_forward_validate(const gs_motion_desc *desc, const float *positions, const float *transforms,
                               const void *workspace);
int gs_motion_backward_validate(const gs_motion_desc *desc, const float *d_positions, const float *d_transforms,
                                const float *d_means, const float *d_coefs, const float *d_rots,
                                const float *d_transls, const void *workspace);

/* positions [G, B, 3] and / or transforms [G, B, 3, 4]; at least one is
 * non-NULL, positions needs desc->means.  G = 0 makes no launch. */
int gs_motion_forward(const gs_motion_desc *desc, float *positions, float *transforms, void *workspace,
                      gs_stream_t stream);

/* The gradients for the upstream d_positions [G, B, 3] and / or d_transforms
 * [G, B, 3, 4] (at least one non-NULL; d_positions needs desc->means).
 * d_means [G, 3] may be NULL; d_coefs [G, K], d_rots [K, T, 6] and d_transls
 * [K, T, 3] are required.  `workspace` holds
 * gs_motion_workspace_bytes(G, K, B, 1) bytes, 16-byte aligned.  G = 0 only
 * zeroes d_rots and d_transls. */
int gs_motion_backward(const gs_motion_desc *desc, const float *d_positions, const float *d_transforms,
                       float *d_means, float *d_coefs, float *d_rots, float *d_transls, void *workspace,
                       gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_MOTION_H */
