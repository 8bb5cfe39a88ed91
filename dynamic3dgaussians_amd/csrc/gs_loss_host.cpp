// gs_loss_host.cpp -- host-only part of the photometric loss's C ABI
// (include/gs_loss.h): the workspace size and the argument validator that
// gs_photo_loss_forward / gs_photo_loss_backward (gs_loss.hip) run before
// they enqueue anything.  Plain C++ with no HIP dependency, so the same file
// is linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/loss_host_sanitize.c (tests/test_image_loss.py).
#include <math.h>
#include <stdint.h>

#include "../../include/gs_loss.h"
#include "gs_host_util.h"
#include "gs_loss_layout.h"

using namespace gs;

extern "C" {

size_t gs_photo_loss_struct_bytes(void) { return sizeof(gs_photo_loss); }

size_t gs_photo_loss_workspace_bytes(int32_t B, int32_t Ch, int32_t H, int32_t W) {
  if (B <= 0 || Ch <= 0 || H <= 0 || W <= 0) return 0;
  return PhotoLossLayout(B, Ch, H, W).total;
}

int gs_photo_loss_validate(const gs_photo_loss* a, int backward, const float* dL_dloss, const float* dL_dimage,
                           const float* dL_dgain, const float* dL_doffset) {
  if (!a) return gs_set_error(-1, "photometric loss: null argument block");
  if (a->B <= 0 || a->Ch <= 0 || a->H <= 0 || a->W <= 0)
    return gs_set_error(-1, "photometric loss: B, Ch, H, W must be > 0 (got %d, %d, %d, %d)", a->B, a->Ch, a->H,
                        a->W);
  const PhotoLossLayout L(a->B, a->Ch, a->H, a->W);
  if (L.blocks > 0x7FFFFFFF || L.planes * L.plane_elems > ((int64_t)1 << 40))
    return gs_set_error(-1, "photometric loss: batch of %d x %d x %d x %d is too large", a->B, a->Ch, a->H, a->W);
  if (!a->image || !a->target) return gs_set_error(-1, "photometric loss: image and target are required");
  if (!a->losses) return gs_set_error(-1, "photometric loss: losses is required");
  if (!aligned4(a->image) || !aligned4(a->target))
    return gs_set_error(-1, "photometric loss: image and target must be 4-byte aligned");
  if (!aligned4(a->mask) || !aligned4(a->gain) || !aligned4(a->offset) || !aligned4(a->losses))
    return gs_set_error(-1, "photometric loss: mask, gain, offset and losses must be 4-byte aligned");
  if (a->mask && a->mask_batch_stride != 0 && a->mask_batch_stride != L.plane_elems)
    return gs_set_error(-1, "photometric loss: mask_batch_stride must be 0 or H*W = %lld (got %lld)",
                        (long long)L.plane_elems, (long long)a->mask_batch_stride);
  if (!isfinite(a->l1_weight) || !isfinite(a->ssim_weight))
    return gs_set_error(-1, "photometric loss: l1_weight and ssim_weight must be finite");
  if (int e = check_workspace("photometric loss", a->workspace, a->workspace_bytes, L.total)) return e;
  if (backward) {
    if (!dL_dloss) return gs_set_error(-1, "photometric loss backward: dL_dloss is required");
    if (!dL_dimage) return gs_set_error(-1, "photometric loss backward: dL_dimage is required");
    if (!aligned4(dL_dimage) || !aligned4(dL_dloss) || !aligned4(dL_dgain) || !aligned4(dL_doffset))
      return gs_set_error(-1, "photometric loss backward: gradient pointers must be 4-byte aligned");
  }
  return 0;
}

}  // extern "C"
