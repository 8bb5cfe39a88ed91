// gs_camera_grad_host.cpp -- host-only part of the camera gradients' C ABI
// (include/gs_camera_grad.h): the workspace size and the argument validator
// that gs_camera_grad_batch (gs_api.hip) runs before it enqueues anything.
// Plain C++ with no HIP dependency, so the same file is linked into
// libgsplat_hip.so and into the CPU sanitizer program
// tools/camera_grad_host_sanitize.c.
#include <stdint.h>

#include "../../include/gs_camera_grad.h"
#include "gs_camera_grad_layout.h"
#include "gs_host_util.h"

using namespace gs;

static_assert(GS_CAMERA_GRAD_MAX_CAMS == CG_MAX_CAMS, "gs_camera_grad.h and gs_camera_grad_layout.h");

extern "C" {

size_t gs_camera_grad_workspace_bytes(int64_t P, int32_t C) { return camera_grad_bytes(P, C); }

int gs_check_camera_grad(int64_t P, int32_t C, int compat, const void* workspace, uint64_t workspace_bytes,
                         const float* dL_dview, const float* dL_dproj, const float* dL_dcampos) {
  if (P < 0 || P > 0x7FFFFFFF) return gs_set_error(-1, "camera grad: P must be in [0, 2^31) (got %lld)", (long long)P);
  if (C < 1 || C > CG_MAX_CAMS)
    return gs_set_error(-1, "camera grad: camera batch size %d outside 1..%d", C, CG_MAX_CAMS);
  if (compat != 1)  // COMPAT_FIXED (gs_common.h)
    return gs_set_error(-1, "camera grad: compat %d is refused: only compat = fixed (1) has a forward whose exact "
                            "derivative the backward's terms are (reference mode swaps the camera scalars, Q2)",
                        compat);
  if (!dL_dview || !dL_dproj || !dL_dcampos)
    return gs_set_error(-1, "camera grad: dL_dview, dL_dproj and dL_dcampos are required");
  if (!aligned4(dL_dview) || !aligned4(dL_dproj) || !aligned4(dL_dcampos))
    return gs_set_error(-1, "camera grad: the outputs must be 4-byte aligned");
  return check_workspace("camera grad", workspace, workspace_bytes, camera_grad_bytes(P, C));
}

}  // extern "C"
