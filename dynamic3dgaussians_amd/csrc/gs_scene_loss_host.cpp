// gs_scene_loss_host.cpp -- host-only part of the scene regularisers' C ABI
// (include/gs_scene_loss.h): the workspace size and the argument validators
// that gs_scene_loss_forward / gs_scene_loss_backward and gs_fg_gather_forward
// / gs_fg_gather_backward (gs_scene_loss.hip) run before they enqueue
// anything.  Plain C++ with no HIP dependency, so the same file is linked into
// libgsplat_hip.so and into the CPU sanitizer program
// tools/scene_loss_host_sanitize.c (tests/test_scene_loss.py).
#include <stdint.h>

#include "../../include/gs_scene_loss.h"
#include "gs_host_util.h"
#include "gs_scene_loss_layout.h"

using namespace gs;

namespace gs {

int fg_gather_check(const char* who, int backward, int64_t P, int64_t n_fg, const void* slot, const void* means,
                    const void* rotations, const void* fg_pts, const void* fg_rot) {
  if (P <= 0 || P > SL_MAX_ROWS) return gs_set_error(-1, "%s: P must be in [1, 2^31 - 1] (got %lld)", who, (long long)P);
  if (n_fg < 0 || n_fg > P)
    return gs_set_error(-1, "%s: n_fg must be in [0, P = %lld] (got %lld)", who, (long long)P, (long long)n_fg);
  if (!slot) return gs_set_error(-1, "%s: slot is required", who);
  if (!backward) {  // the backward takes a null table as "no gradient" / "not wanted"
    if (!means || !rotations) return gs_set_error(-1, "%s: the two [P] tables are required", who);
    if (n_fg > 0 && (!fg_pts || !fg_rot)) return gs_set_error(-1, "%s: the two [n_fg] tables are required", who);
  }
  if (!aligned4(slot) || !aligned4(means) || !aligned4(rotations) || !aligned4(fg_pts) || !aligned4(fg_rot))
    return gs_set_error(-1, "%s: every pointer must be 4-byte aligned", who);
  return 0;
}

}  // namespace gs

extern "C" {

size_t gs_scene_loss_struct_bytes(void) { return sizeof(gs_scene_loss); }

size_t gs_scene_loss_workspace_bytes(int64_t P) {
  if (P <= 0) return 0;
  return SceneLossLayout(P).total;
}

int gs_scene_loss_validate(const gs_scene_loss* a, int backward, const float* dL_dlosses, const float* dL_dmeans,
                           const float* dL_drotations, const float* dL_dcolors) {
  if (!a) return gs_set_error(-1, "scene loss: null argument block");
  if (a->P <= 0 || a->P > SL_MAX_ROWS)
    return gs_set_error(-1, "scene loss: P must be in [1, 2^31 - 1] (got %lld)", (long long)a->P);
  if (a->n_fg < 0 || a->n_bg < 0)
    return gs_set_error(-1, "scene loss: n_fg and n_bg must be >= 0 (got %lld, %lld)", (long long)a->n_fg,
                        (long long)a->n_bg);
  if (a->n_fg + a->n_bg != a->P)
    return gs_set_error(-1, "scene loss: n_fg + n_bg must equal P (got %lld + %lld, P = %lld)", (long long)a->n_fg,
                        (long long)a->n_bg, (long long)a->P);
  if (!a->slot) return gs_set_error(-1, "scene loss: slot is required");
  if (!a->means || !a->rotations || !a->colors)
    return gs_set_error(-1, "scene loss: means, rotations and colors are required");
  if (!a->prev_col) return gs_set_error(-1, "scene loss: prev_col is required");
  if (a->n_bg > 0 && (!a->init_bg_pts || !a->init_bg_rot))
    return gs_set_error(-1, "scene loss: init_bg_pts and init_bg_rot are required when n_bg > 0");
  if (!aligned4(a->slot) || !aligned4(a->means) || !aligned4(a->rotations) || !aligned4(a->colors) ||
      !aligned4(a->prev_col) || !aligned4(a->init_bg_pts) || !aligned4(a->init_bg_rot))
    return gs_set_error(-1, "scene loss: every table must be 4-byte aligned");
  if (backward) {
    if (!dL_dlosses) return gs_set_error(-1, "scene loss backward: dL_dlosses is required");
    if (!dL_dmeans || !dL_drotations || !dL_dcolors)
      return gs_set_error(-1, "scene loss backward: dL_dmeans, dL_drotations and dL_dcolors are required");
    if (!aligned4(dL_dlosses) || !aligned4(dL_dmeans) || !aligned4(dL_drotations) || !aligned4(dL_dcolors))
      return gs_set_error(-1, "scene loss backward: gradient pointers must be 4-byte aligned");
  } else {
    if (!a->losses) return gs_set_error(-1, "scene loss: losses is required");
    if (!aligned4(a->losses)) return gs_set_error(-1, "scene loss: losses must be 4-byte aligned");
    if (int e = check_workspace("scene loss", a->workspace, a->workspace_bytes, SceneLossLayout(a->P).total)) return e;
  }
  return 0;
}

}  // extern "C"
