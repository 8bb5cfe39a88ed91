// gs_motion_host.cpp -- host-only part of the motion-basis warp's C ABI
// (include/gs_motion.h): the size queries and the two argument validators that
// gs_motion_forward / gs_motion_backward (gs_motion.hip) run before they
// enqueue anything.  Plain C++ with no HIP dependency, so the same file is
// linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/motion_host_sanitize.c (tests/test_motion.py).
#include <stdint.h>

#include "../../include/gs_motion.h"
#include "gs_host_util.h"
#include "gs_motion_layout.h"

using namespace gs;

static_assert(GS_MOTION_MAX_K == MT_MAX_K && GS_MOTION_MAX_B == MT_MAX_B, "gs_motion.h and gs_motion_layout.h");

namespace {
// the descriptor alone: envelope, tables, frame indices
int check_desc(const char* who, const gs_motion_desc* d) {
  if (!d) return gs_set_error(-1, "%s: null descriptor", who);
  if (d->G < 0 || d->G > MT_MAX_G)
    return gs_set_error(-1, "%s: G must be in [0, %lld] (got %lld)", who, (long long)MT_MAX_G, (long long)d->G);
  if (d->K < 1 || d->K > MT_MAX_K)
    return gs_set_error(-1, "%s: K must be in [1, %d] (got %d)", who, MT_MAX_K, d->K);
  if (d->B < 1 || d->B > MT_MAX_B)
    return gs_set_error(-1, "%s: B must be in [1, %d] frames per call (got %d)", who, MT_MAX_B, d->B);
  if (d->T < 1) return gs_set_error(-1, "%s: T must be > 0 (got %d)", who, d->T);
  if (d->coef_mode != GS_MOTION_COEFS_GIVEN && d->coef_mode != GS_MOTION_COEFS_LOGITS)
    return gs_set_error(-1, "%s: unknown coef_mode %d", who, d->coef_mode);
  for (int b = 0; b < d->B; ++b)
    if (d->ts[b] < 0 || d->ts[b] >= d->T)
      return gs_set_error(-1, "%s: ts[%d] = %d is outside [0, %d)", who, b, d->ts[b], d->T);
  if (!d->rots || !d->transls) return gs_set_error(-1, "%s: rots and transls are required", who);
  if (d->G > 0 && !d->coefs) return gs_set_error(-1, "%s: coefs is required", who);
  if (!aligned4(d->rots) || !aligned4(d->transls) || !aligned4(d->coefs) || !aligned4(d->means))
    return gs_set_error(-1, "%s: rots, transls, coefs and means must be 4-byte aligned", who);
  return 0;
}
}  // namespace

extern "C" {

size_t gs_motion_struct_bytes(void) { return sizeof(gs_motion_desc); }

size_t gs_motion_workspace_bytes(int64_t G, int32_t K, int32_t B, int backward) {
  if (!backward || G <= 0 || G > MT_MAX_G || K < 1 || K > MT_MAX_K || B < 1 || B > MT_MAX_B) return 0;
  return MotionLayout(G, K, B).total;
}

int32_t gs_motion_backward_block(int32_t K, int32_t B) {
  if (K < 1 || K > MT_MAX_K || B < 1 || B > MT_MAX_B) return 0;
  return mt_backward_threads(K, B);
}

int gs_motion_forward_validate(const gs_motion_desc* d, const float* positions, const float* transforms,
                               const void* workspace) {
  (void)workspace;  // the forward needs none
  const char* who = "motion forward";
  if (int e = check_desc(who, d)) return e;
  if (!positions && !transforms) return gs_set_error(-1, "%s: positions or transforms is required", who);
  if (positions && d->G > 0 && !d->means) return gs_set_error(-1, "%s: positions needs means", who);
  if (!aligned4(positions) || !aligned4(transforms))
    return gs_set_error(-1, "%s: positions and transforms must be 4-byte aligned", who);
  return 0;
}

int gs_motion_backward_validate(const gs_motion_desc* d, const float* d_positions, const float* d_transforms,
                                const float* d_means, const float* d_coefs, const float* d_rots,
                                const float* d_transls, const void* workspace) {
  const char* who = "motion backward";
  if (int e = check_desc(who, d)) return e;
  if (!d_rots || !d_transls) return gs_set_error(-1, "%s: d_rots and d_transls are required", who);
  if (!aligned4(d_positions) || !aligned4(d_transforms) || !aligned4(d_means) || !aligned4(d_coefs) ||
      !aligned4(d_rots) || !aligned4(d_transls))
    return gs_set_error(-1, "%s: gradient pointers must be 4-byte aligned", who);
  if (d->G == 0) return 0;
  if (!d_positions && !d_transforms) return gs_set_error(-1, "%s: d_positions or d_transforms is required", who);
  if (d_positions && !d->means) return gs_set_error(-1, "%s: d_positions needs means", who);
  if (d_means && !d->means) return gs_set_error(-1, "%s: d_means needs means", who);
  if (!d_coefs) return gs_set_error(-1, "%s: d_coefs is required", who);
  // the ABI carries no byte count: required and aligned only
  const size_t need = MotionLayout(d->G, d->K, d->B).total;
  return check_workspace(who, workspace, need, need);
}

}  // extern "C"
