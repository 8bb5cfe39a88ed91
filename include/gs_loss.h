/* gs_loss.h -- C ABI of the fused photometric loss (L1 + SSIM), exported by
 * the same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the PyTorch chain of the reference's per-camera image loss
 * (train.py:161-183; helpers.py:110-111 l1_loss_v1; external.py:90-133
 * calc_ssim) for a whole batch [B, Ch, H, W] at once:
 *
 *   x      = (gain[b,c] * image + offset[b,c]) * mask       y = target * mask
 *   L1_b   = mean over Ch*H*W of |x - y|
 *   SSIM_b = mean over Ch*H*W of the SSIM map of (x, y): 11x11 Gaussian
 *            window, sigma 1.5, zero padding of 5, c1 = 0.01^2, c2 = 0.03^2
 *   losses[b] = l1_weight * L1_b + ssim_weight * (1 - SSIM_b)
 *
 * gain / offset [B, Ch] and mask ([H, W]: mask_batch_stride 0, or [B, H, W]:
 * mask_batch_stride H*W) are optional (1, 0, 1 when NULL).  Everything is
 * fp32, contiguous device memory.
 *
 * The forward keeps the three derivative maps of the SSIM term in the
 * workspace; the backward convolves them with the same window.  The same
 * workspace (gs_photo_loss_workspace_bytes) must therefore reach both calls
 * unchanged in between.  All sums (the two loss sums, the gain and offset
 * gradients) are per-workgroup partials added in a fixed order: two calls on
 * the same inputs give the same bits.  No floating-point atomics.
 *
 * All calls are asynchronous on `stream`, read nothing back and never
 * synchronise; return 0 or an error code with gs_last_error() set (as
 * gsplat_hip.h). */
#ifndef GS_LOSS_H
#define GS_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_photo_loss {
  int32_t B, Ch, H, W;          /* batch, channels, rows, columns (all > 0) */
  const float *image;           /* [B, Ch, H, W] the render */
  const float *target;          /* [B, Ch, H, W] */
  const float *mask;            /* optional [H, W] or [B, H, W] */
  const float *gain;            /* optional [B, Ch] */
  const float *offset;          /* optional [B, Ch] */
  int64_t mask_batch_stride;    /* floats between the masks of two images: 0 or H*W */
  float l1_weight, ssim_weight; /* train.py:183: 0.8, 0.2 */
  float *losses;                /* [B], written by the forward */
  void *workspace;              /* gs_photo_loss_workspace_bytes(B, Ch, H, W) bytes */
  uint64_t workspace_bytes;     /* size of the buffer behind `workspace` */
} gs_photo_loss;

/* sizeof(gs_photo_loss) as the library was compiled (for binding mirrors). */
size_t gs_photo_loss_struct_bytes(void);

/* Workspace of one forward + backward pair: three fp32 planes of the image's
 * size and the per-workgroup partial sums.  0 for non-positive shapes. */
size_t gs_photo_loss_workspace_bytes(int32_t B, int32_t Ch, int32_t H, int32_t W);

/* The argument check both entry points run first (host code, no device
 * access).  backward = 0 ignores the four gradient pointers. */
int gs_photo_loss_validate(const gs_photo_loss *args, int backward, const float *dL_dloss,
                           const float *dL_dimage, const float *dL_dgain, const float *dL_doffset);

/* losses[b] for every image of the batch. */
int gs_photo_loss_forward(const gs_photo_loss *args, gs_stream_t stream);

/* dL_dimage [B, Ch, H, W], and dL_dgain / dL_doffset [B, Ch] when non-NULL
 * (written, not accumulated), for the upstream gradients dL_dloss [B]
 * (device memory).  target and mask get no gradient. */
int gs_photo_loss_backward(const gs_photo_loss *args, const float *dL_dloss, float *dL_dimage,
                           float *dL_dgain, float *dL_doffset, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_LOSS_H */
