// gs_metrics_host.cpp -- host-only part of the evaluation metrics' C ABI
// (include/gs_metrics.h): the workspace size and the argument validators that
// gs_image_metrics / gs_mask_iou (gs_metrics.hip) run before they enqueue
// anything.  Plain C++ with no HIP dependency, so the same file is linked into
// libgsplat_hip.so and into the CPU sanitizer program
// tools/metrics_host_sanitize.c (tests/test_metrics.py).
#include <math.h>
#include <stdint.h>

#include "../../include/gs_metrics.h"
#include "gs_host_util.h"
#include "gs_metrics_layout.h"

using namespace gs;

extern "C" {

size_t gs_image_metrics_struct_bytes(void) { return sizeof(struct gs_image_metrics); }

size_t gs_image_metrics_workspace_bytes(int32_t B, int32_t Ch, int32_t H, int32_t W) {
  if (B <= 0 || Ch <= 0 || H <= 0 || W <= 0) return 0;
  return ImageMetricsLayout(B, Ch, H, W).total;
}

int gs_image_metrics_validate(const struct gs_image_metrics* a) {
  if (!a) return gs_set_error(-1, "image metrics: null argument block");
  if (a->B <= 0 || a->Ch <= 0 || a->H <= 0 || a->W <= 0)
    return gs_set_error(-1, "image metrics: B, Ch, H, W must be > 0 (got %d, %d, %d, %d)", a->B, a->Ch, a->H, a->W);
  const ImageMetricsLayout L(a->B, a->Ch, a->H, a->W);
  if (L.blocks > 0x7FFFFFFF || L.planes * L.plane_elems > ((int64_t)1 << 40))
    return gs_set_error(-1, "image metrics: batch of %d x %d x %d x %d is too large", a->B, a->Ch, a->H, a->W);
  if (!a->pred || !a->target) return gs_set_error(-1, "image metrics: pred and target are required");
  if (!a->out) return gs_set_error(-1, "image metrics: out is required");
  if (!aligned4(a->pred) || !aligned4(a->target) || !aligned4(a->mask) || !aligned4(a->out))
    return gs_set_error(-1, "image metrics: pred, target, mask and out must be 4-byte aligned");
  if (a->mask && a->mask_batch_stride != 0 && a->mask_batch_stride != L.plane_elems)
    return gs_set_error(-1, "image metrics: mask_batch_stride must be 0 or H*W = %lld (got %lld)",
                        (long long)L.plane_elems, (long long)a->mask_batch_stride);
  if (a->want_ssim && (a->H < MT_TAPS || a->W < MT_TAPS))
    return gs_set_error(-1, "image metrics: the masked SSIM needs H, W >= %d (got %d x %d): no window fits", MT_TAPS,
                        a->H, a->W);
  return check_workspace("image metrics", a->workspace, a->workspace_bytes, L.total);
}

int gs_mask_iou_validate(int32_t B, int64_t n, const float* pred, const float* target, float threshold,
                         const int64_t* out) {
  if (B <= 0 || n <= 0)
    return gs_set_error(-1, "mask IoU: B and n must be > 0 (got %d, %lld)", B, (long long)n);
  if ((n + MT_IOU_CHUNK - 1) / MT_IOU_CHUNK > 0x7FFFFFFF || B > 65535)
    return gs_set_error(-1, "mask IoU: batch of %d x %lld is too large", B, (long long)n);
  if (!pred || !target) return gs_set_error(-1, "mask IoU: pred and target are required");
  if (!out) return gs_set_error(-1, "mask IoU: out is required");
  if (!aligned4(pred) || !aligned4(target)) return gs_set_error(-1, "mask IoU: pred and target must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(out) & 7u) != 0) return gs_set_error(-1, "mask IoU: out must be 8-byte aligned");
  if (isnan(threshold)) return gs_set_error(-1, "mask IoU: threshold must not be NaN");
  return 0;
}

}  // extern "C"
