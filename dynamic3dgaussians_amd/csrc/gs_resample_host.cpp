// gs_resample_host.cpp -- host-only part of the bilinear resample's C ABI
// (include/gs_resample.h): the workspace size, the argument validator that
// gs_resample_forward / gs_resample_backward (gs_resample.hip) run before
// they enqueue anything, and the axis function as host code.  Plain C++ with
// no HIP dependency, so the same file is linked into libgsplat_hip.so and into
// the CPU sanitizer program tools/resample_host_sanitize.c
// (tests/test_resample.py).
#include <stdint.h>

#include "../../include/gs_resample.h"
#include "gs_host_util.h"
#include "gs_resample_layout.h"

using namespace gs;

namespace {
bool size_ok(int32_t v) { return v >= 1 && v <= RS_MAX_SIZE; }
}  // namespace

extern "C" {

size_t gs_resample_struct_bytes(void) { return sizeof(gs_resample); }

size_t gs_resample_workspace_bytes(int32_t H, int32_t W) {
  if (!size_ok(H) || !size_ok(W)) return 0;
  return ResampleLayout(H, W).total;
}

int gs_resample_validate(const gs_resample* a, int backward, const float* d_y, const float* d_x) {
  if (!a) return gs_set_error(-1, "resample: null argument block");
  if (a->B <= 0 || a->Ch <= 0) return gs_set_error(-1, "resample: B, Ch must be > 0 (got %d, %d)", a->B, a->Ch);
  if (!size_ok(a->H) || !size_ok(a->W))
    return gs_set_error(-1, "resample: H, W must be in [1, %d] (got %d, %d)", RS_MAX_SIZE, a->H, a->W);
  if (!size_ok(a->h) || !size_ok(a->w))
    return gs_set_error(-1, "resample: h, w must be in [1, %d] (got %d, %d)", RS_MAX_SIZE, a->h, a->w);
  if (backward) {
    if (!d_y) return gs_set_error(-1, "resample backward: d_y is required");
    if (!d_x) return gs_set_error(-1, "resample backward: d_x is required");
    if (!aligned4(d_y) || !aligned4(d_x))
      return gs_set_error(-1, "resample backward: gradient pointers must be 4-byte aligned");
    if (int e = check_workspace("resample backward", a->workspace, a->workspace_bytes, ResampleLayout(a->H, a->W).total))
      return e;
  } else {
    if (!a->x) return gs_set_error(-1, "resample: x is required");
    if (!a->y) return gs_set_error(-1, "resample: y is required");
    if (!aligned4(a->x) || !aligned4(a->y)) return gs_set_error(-1, "resample: x and y must be 4-byte aligned");
  }
  return 0;
}

int gs_resample_axis(int32_t I, int32_t O, int32_t align_corners, int32_t* i0, float* l1, int32_t* first) {
  if (!size_ok(I) || !size_ok(O))
    return gs_set_error(-1, "resample axis: I, O must be in [1, %d] (got %d, %d)", RS_MAX_SIZE, I, O);
  const float scale = resample_scale(I, O, align_corners);
  for (int o = 0; o < O; ++o) {
    const AxisTap t = resample_tap(scale, I, o, align_corners);
    if (i0) i0[o] = t.i0;
    if (l1) l1[o] = t.l1;
    if (first) resample_first_of(scale, I, O, o, align_corners, first);
  }
  return 0;
}

}  // extern "C"
