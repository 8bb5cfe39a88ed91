/* gs_metrics.h -- C ABI of the evaluation metrics (masked PSNR sums, masked
 * SSIM, mask IoU), exported by the same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the PyTorch chains of the reference's quality reports for a whole
 * batch [B, Ch, H, W] at once: calc_psnr (external.py:85-87), compute_psnr /
 * mPSNR (metrics.py:14-43, 82-129), mSSIM (metrics.py:334-424) and mask_iou /
 * MaskIoU (metrics.py:222-250, 523-551).  Forward only.
 *
 * The struct and the entry point share the name gs_image_metrics (the struct
 * is always written `struct gs_image_metrics`).  The call writes, per image
 * b with m = mask (1 when NULL):
 *
 *   out[b][0]  sse       sum over Ch, H, W of ((pred - target) * m)^2
 *   out[b][1]  sae       sum over Ch, H, W of |(pred - target) * m|
 *   out[b][2]  mask_sum  sum over H, W of m
 *   out[b][3]  ssim      mean of the masked-SSIM map, or 0 when want_ssim == 0
 *
 * Masked SSIM (metrics.py:349-420 for channels-first data): the window is
 * w[k] = exp(-((k - 5) / 1.5)^2 / 2), k = 0..10, normalised to sum 1.  The
 * masked blur of a plane z runs along the rows and then down the columns,
 * each pass "valid" (no padding):  u = sum_k w[k] z m,  n = sum_k m over the
 * same 11 taps,  result = u * 11 / n where n != 0, else 0; the pass's output
 * mask (1 where n != 0) is the next pass's mask.  The rescale is by the tap
 * count over the unmasked count, not by the unmasked weight: the reference's
 * choice, kept.  With mu0, mu1 the blurs of pred and target:
 *
 *   s00 = max(blur(pred^2) - mu0^2, 0)      s11 likewise
 *   s   = blur(pred target) - mu0 mu1       s01 = sign(s) min(sqrt(s00 s11), |s|)
 *   map = (2 mu0 mu1 + c1)(2 s01 + c2) / ((mu0^2 + mu1^2 + c1)(s00 + s11 + c2))
 *
 * with c1 = 0.01^2, c2 = 0.03^2, over the (H - 10) x (W - 10) positions of
 * every channel; a position whose window holds no unmasked pixel has map = 1
 * exactly and is part of the mean.
 *
 * mask is [H, W] (mask_batch_stride 0) or [B, H, W] (mask_batch_stride H*W).
 * Everything is fp32, contiguous device memory.  Sums are per-workgroup
 * partials in the workspace, added in a fixed order in fp64: two calls on the
 * same inputs give the same bits.  No floating-point atomics.
 *
 * HBM bytes of one call, from shapes: (2 Ch + 1) floats read per pixel per
 * image (pred, target and the mask once), 16 bytes written per workgroup.
 * Halo re-reads are expected to hit in cache and are not counted.
 *
 * gs_mask_iou counts, per image of n pixels, those where both
 * (pred > threshold) and (target > threshold) hold and those where either
 * holds: exact integers (integer adds only).  threshold 0.9 is mask_iou,
 * threshold 0 is MaskIoU for {0, 1} masks.
 *
 * All calls are asynchronous on `stream`, read nothing back and never
 * synchronise; return 0 or an error code with gs_last_error() set (as
 * gsplat_hip.h). */
#ifndef GS_METRICS_H
#define GS_METRICS_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

struct gs_image_metrics {
  int32_t B, Ch, H, W;        /* batch, channels, rows, columns (all > 0) */
  const float *pred;          /* [B, Ch, H, W] */
  const float *target;        /* [B, Ch, H, W] */
  const float *mask;          /* optional [H, W] or [B, H, W] */
  int64_t mask_batch_stride;  /* floats between the masks of two images: 0 or H*W */
  int32_t want_ssim;          /* 0: out[b][3] = 0 and any H, W; else H, W >= 11 */
  int32_t _pad;
  float *out;                 /* [B, 4]: sse, sae, mask_sum, ssim */
  void *workspace;            /* gs_image_metrics_workspace_bytes(B, Ch, H, W) bytes */
  uint64_t workspace_bytes;   /* size of the buffer behind `workspace` */
};

/* sizeof(struct gs_image_metrics) as the library was compiled (for binding mirrors). */
size_t gs_image_metrics_struct_bytes(void);

/* Workspace of one call: four partial sums per workgroup.  0 for
 * non-positive shapes. */
size_t gs_image_metrics_workspace_bytes(int32_t B, int32_t Ch, int32_t H, int32_t W);

/* The argument check gs_image_metrics runs first (host code, no device access). */
int gs_image_metrics_validate(const struct gs_image_metrics *args);

/* out[b][0..3] for every image of the batch. */
int gs_image_metrics(const struct gs_image_metrics *args, gs_stream_t stream);

/* The argument check gs_mask_iou runs first (host code, no device access). */
int gs_mask_iou_validate(int32_t B, int64_t n, const float *pred, const float *target, float threshold,
                         const int64_t *out);

/* out[b] = {intersection, union} of (pred > threshold), (target > threshold)
 * over the n pixels of image b; pred, target [B, n]. */
int gs_mask_iou(int32_t B, int64_t n, const float *pred, const float *target, float threshold, int64_t *out,
                gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_METRICS_H */
