// gs_depth_loss_host.cpp -- host-only part of the depth-correlation loss's C
// ABI (include/gs_depth_loss.h): the workspace size and the argument
// validator that gs_depth_loss_forward / gs_depth_loss_backward
// (gs_depth_loss.hip) run before they enqueue anything.  Plain C++ with no HIP
// dependency, so the same file is linked into libgsplat_hip.so and into the
// CPU sanitizer program tools/depth_loss_host_sanitize.c
// (tests/test_depth_loss.py).
#include <math.h>
#include <stdint.h>

#include "../../include/gs_depth_loss.h"
#include "gs_depth_loss_layout.h"
#include "gs_host_util.h"

using namespace gs;

extern "C" {

size_t gs_depth_loss_struct_bytes(void) { return sizeof(gs_depth_loss); }

size_t gs_depth_loss_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return DepthLossLayout(B, H, W).total;
}

int gs_depth_loss_validate(const gs_depth_loss* a, int backward, const float* dL_dloss, const float* dL_ddepth) {
  if (!a) return gs_set_error(-1, "depth loss: null argument block");
  if (a->B <= 0 || a->H <= 0 || a->W <= 0)
    return gs_set_error(-1, "depth loss: B, H, W must be > 0 (got %d, %d, %d)", a->B, a->H, a->W);
  const DepthLossLayout L(a->B, a->H, a->W);
  if (a->B > 65535 || L.plane_elems > ((int64_t)1 << 40))
    return gs_set_error(-1, "depth loss: batch of %d x %d x %d is too large", a->B, a->H, a->W);
  if (!a->depth || !a->target) return gs_set_error(-1, "depth loss: depth and target are required");
  if (!a->stats) return gs_set_error(-1, "depth loss: stats is required");
  if (!aligned4(a->depth) || !aligned4(a->target))
    return gs_set_error(-1, "depth loss: depth and target must be 4-byte aligned");
  if (!aligned4(a->stats)) return gs_set_error(-1, "depth loss: stats must be 4-byte aligned");
  if (a->mask && a->mask_batch_stride != 0 && a->mask_batch_stride != L.plane_elems)
    return gs_set_error(-1, "depth loss: mask_batch_stride must be 0 or H*W = %lld (got %lld)",
                        (long long)L.plane_elems, (long long)a->mask_batch_stride);
  if (!isfinite(a->near) || !isfinite(a->far)) return gs_set_error(-1, "depth loss: near and far must be finite");
  if (!(a->near > 0.f)) return gs_set_error(-1, "depth loss: near must be > 0 (got %g)", (double)a->near);
  if (!(a->near < a->far))
    return gs_set_error(-1, "depth loss: near must be < far (got %g, %g)", (double)a->near, (double)a->far);
  if (backward) {
    if (!dL_dloss) return gs_set_error(-1, "depth loss backward: dL_dloss is required");
    if (!dL_ddepth) return gs_set_error(-1, "depth loss backward: dL_ddepth is required");
    if (!aligned4(dL_dloss) || !aligned4(dL_ddepth))
      return gs_set_error(-1, "depth loss backward: gradient pointers must be 4-byte aligned");
  } else {
    if (!a->losses) return gs_set_error(-1, "depth loss: losses is required");
    if (!aligned4(a->losses)) return gs_set_error(-1, "depth loss: losses must be 4-byte aligned");
    if (int e = check_workspace("depth loss", a->workspace, a->workspace_bytes, L.total)) return e;
  }
  return 0;
}

}  // extern "C"
