/* gs_depth_loss.h -- C ABI of the fused masked depth-correlation loss,
 * exported by the same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the PyTorch chain of the reference's depth term (dyn_train.py:
 * 256-265: boolean indexing, clamp, reciprocal, standardisation, Pearson) for
 * a whole batch of B camera planes [B, H, W] at once.  Per camera b, over the
 * pixels M where the mask is non-zero (every pixel without a mask), n = |M|:
 *
 *   p_i = 1 / clamp(depth_i, near, far)          g_i = target_i
 *   Sxx = sum (p_i - mean p)^2,  Syy = sum (g_i - mean g)^2,
 *   Sxy = sum (p_i - mean p)(g_i - mean g)
 *   r   = Sxy / sqrt(Sxx * Syy)                  losses[b] = 1 - clamp(r, -1, 1)
 *
 * stats [B, 8] = {n, mean p, mean g, Sxx, Syy, Sxy, r (unclamped), valid}.
 * A camera is degenerate (valid = 0) when n < 2, Sxx = 0, Syy = 0 or a moment
 * is not finite.  With skip_degenerate = 0 its loss is NaN and its gradient
 * NaN at the masked pixels where the clamp is open (the reference's 0/0);
 * with skip_degenerate != 0 its loss is 0 and its gradient plane all zeros.
 * The other cameras of the batch are unaffected either way.
 *
 * depth and target are fp32; the mask is one BYTE per pixel ([H, W]:
 * mask_batch_stride 0, or [B, H, W]: mask_batch_stride H*W; NULL: no mask).
 * Everything is contiguous device memory.
 *
 * The moments are centred sums merged pairwise in a fixed order (per thread,
 * wave, workgroup, then one record per workgroup in the workspace, merged by
 * one workgroup per camera): no raw power sums and no floating-point atomics,
 * so two calls on the same inputs give the same bits.
 *
 * The forward needs the workspace (gs_depth_loss_workspace_bytes).  The
 * backward reads only `stats` (as the forward wrote it) and the inputs:
 * workspace and losses may be NULL there.
 *
 * All calls are asynchronous on `stream`, read nothing back and never
 * synchronise; return 0 or an error code with gs_last_error() set (as
 * gsplat_hip.h). */
#ifndef GS_DEPTH_LOSS_H
#define GS_DEPTH_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_depth_loss {
  int32_t B, H, W;            /* cameras, rows, columns (all > 0) */
  const float *depth;         /* [B, H, W] the rendered depth */
  const float *target;        /* [B, H, W] the prior, in inverse-depth units */
  const uint8_t *mask;        /* optional [H, W] or [B, H, W], non-zero = the pixel takes part */
  int64_t mask_batch_stride;  /* bytes between the masks of two cameras: 0 or H*W */
  float near, far;            /* clamp bounds, 0 < near < far (dyn_train.py:20: 1e-7, 50) */
  int32_t skip_degenerate;    /* 0: NaN as the reference; else loss 0 and a zero gradient */
  float *losses;              /* [B], written by the forward */
  float *stats;               /* [B, 8], written by the forward, read by the backward */
  void *workspace;            /* gs_depth_loss_workspace_bytes(B, H, W) bytes (forward only) */
  uint64_t workspace_bytes;   /* size of the buffer behind `workspace` */
} gs_depth_loss;

/* sizeof(gs_depth_loss) as the library was compiled (for binding mirrors). */
size_t gs_depth_loss_struct_bytes(void);

/* Workspace of one forward: one 6-float record {n, mean p, mean g, Sxx, Syy,
 * Sxy} per workgroup.  0 for non-positive shapes. */
size_t gs_depth_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);

/* The argument check both entry points run first (host code, no device
 * access).  backward = 0 ignores the two gradient pointers; backward != 0
 * ignores losses and the workspace. */
int gs_depth_loss_validate(const gs_depth_loss *args, int backward, const float *dL_dloss,
                           const float *dL_ddepth);

/* losses[b] and stats[b, 0:8] for every camera of the batch. */
int gs_depth_loss_forward(const gs_depth_loss *args, gs_stream_t stream);

/* dL_ddepth [B, H, W] (every element written, never accumulated) for the
 * upstream gradients dL_dloss [B] (device memory).  target and mask get no
 * gradient. */
int gs_depth_loss_backward(const gs_depth_loss *args, const float *dL_dloss, float *dL_ddepth,
                           gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_DEPTH_LOSS_H */
