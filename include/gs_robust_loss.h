/* gs_robust_loss.h -- C ABI of the quantile-trimmed (outlier-robust) squared
 * losses and of the batched exact quantile under them, exported by the same
 * libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the reference's helpers.py:16-38 (masked_mse_loss) and
 * ideaII.py:378-384 (trimmed_mse_loss): a per-element squared residual, the
 * torch.quantile of it, the mean of the residuals below that threshold.  For
 * B planes of N elements at once, with no sort and nothing read back.
 *
 * Residual e_i of plane b (fp32, R terms summed in index order, divided once):
 *   GS_ROBUST_CHANNELS  pred, gt [B, R, N]:  e_i = (sum_c (pred[b,c,i] - gt[b,c,i])^2) / R
 *   GS_ROBUST_ROWS      pred, gt [B, N, R]:  e_i = (sum_j (pred[b,i,j] - gt[b,i,j])^2) / R
 *   GS_ROBUST_VALUES    pred     [B, N]:     e_i = pred[b,i] (values >= 0 or NaN; R = 1, gt unused)
 *
 * Threshold of a plane, over the n participating elements (all N, or with
 * over_masked != 0 the ones whose mask byte is non-zero) and the quantile q:
 *   r = q (n - 1) in fp64, lo = floor(r), hi = min(lo + 1, n - 1), w = r - lo,
 *   thr = (double)v_lo + w ((double)v_hi - (double)v_lo)
 * with v_lo, v_hi the exact lo-th and hi-th order statistics, found by a radix
 * select (11 + 10 + 10 bits) on the bit patterns of the non-negative floats.
 * thr is NaN when a participating element is NaN (or negative) or n = 0.
 * Element i is kept iff it participates and (double)e_i < thr.  With
 * select = 0 no threshold is computed, every participating element is kept
 * and stats[b, 0] is +inf.
 *
 * Loss of a plane, m_i the mask byte != 0 (1 without a mask):
 *   S = sum kept_i m_i e_i,  cnt = sum kept_i,  cm = sum kept_i m_i
 *   normalize = 0:  D = cnt                       losses[b] = S / D
 *   normalize != 0: D = norm_width * cm + 1e-8    losses[b] = S / D
 * cnt = 0 with normalize = 0 is 0/0 = NaN, or 0 under skip_degenerate != 0.
 * stats [B, 4] (fp64) = {thr, cnt, cm, number of participating NaN elements}.
 * GS_ROBUST_VALUES computes the thresholds only (losses may be NULL; columns
 * 1 and 2 of stats are 0).
 *
 * Gradient (gs_robust_loss_backward, not for GS_ROBUST_VALUES), to pred only:
 *   d pred = dL_dloss[b] kept_i m_i 2 (pred - gt) / R / D
 * with e_i recomputed by the forward's own expression, so the kept set is the
 * forward's bit for bit.  Reads stats as the forward wrote it; workspace and
 * losses may be NULL there.
 *
 * Sums are per-workgroup fp64 partials added in a fixed order; the histograms
 * use integer atomics only: two calls on the same inputs give the same bits.
 * All calls are asynchronous on `stream`, read nothing back and never
 * synchronise; return 0 or an error code with gs_last_error() set (as
 * gsplat_hip.h).  Everything is contiguous device memory. */
#ifndef GS_ROBUST_LOSS_H
#define GS_ROBUST_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GS_ROBUST_CHANNELS = 0, GS_ROBUST_ROWS = 1, GS_ROBUST_VALUES = 2 };

typedef struct gs_robust_loss {
  int32_t B, R, N;            /* planes, length of the reduced axis, elements per plane (B * N < 2^31) */
  int32_t layout;             /* GS_ROBUST_CHANNELS, GS_ROBUST_ROWS or GS_ROBUST_VALUES */
  const float *pred;          /* see above */
  const float *gt;            /* pred's layout; unused for GS_ROBUST_VALUES */
  const uint8_t *mask;        /* optional [N] or [B, N], non-zero = the element takes part */
  int64_t mask_batch_stride;  /* bytes between the masks of two planes: 0 or N */
  double quantile;            /* q in [0, 1] */
  int32_t select;             /* 0: keep every participating element, no threshold */
  int32_t over_masked;        /* != 0: the quantile is over the masked elements only */
  int32_t normalize;          /* != 0: D = norm_width * sum kept m + 1e-8 */
  int32_t norm_width;         /* the reference's ndim (the width of the image) */
  int32_t skip_degenerate;    /* != 0: an empty kept set gives 0, not NaN */
  int32_t _pad;
  float *losses;              /* [B], written by the forward */
  double *stats;              /* [B, 4], written by the forward, read by the backward */
  void *workspace;            /* gs_robust_loss_workspace_bytes(B, N, layout) bytes (forward only) */
  uint64_t workspace_bytes;   /* size of the buffer behind `workspace` */
} gs_robust_loss;

/* sizeof(gs_robust_loss) as the library was compiled (for binding mirrors). */
size_t gs_robust_loss_struct_bytes(void);

/* Workspace of one forward: per-plane selection state and histograms, the
 * per-workgroup partial sums and (not for GS_ROBUST_VALUES) the fp32 residual
 * plane [B, N].  0 for non-positive shapes or an unknown layout. */
size_t gs_robust_loss_workspace_bytes(int32_t B, int32_t N, int32_t layout);

/* The argument check both entry points run first (host code, no device
 * access).  backward = 0 ignores the two gradient pointers; backward != 0
 * ignores losses and the workspace. */
int gs_robust_loss_validate(const gs_robust_loss *args, int backward, const float *dL_dloss,
                            const float *dL_dpred);

/* losses[b] and stats[b, 0:4] for every plane. */
int gs_robust_loss_forward(const gs_robust_loss *args, gs_stream_t stream);

/* dL_dpred in pred's layout (every element written once, never accumulated)
 * for the upstream gradients dL_dloss [B] (device memory). */
int gs_robust_loss_backward(const gs_robust_loss *args, const float *dL_dloss, float *dL_dpred,
                            gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_ROBUST_LOSS_H */
