// gs_robust_loss_host.cpp -- host-only part of the quantile-trimmed losses' C
// ABI (include/gs_robust_loss.h): the workspace size and the argument
// validator that gs_robust_loss_forward / gs_robust_loss_backward
// (gs_robust_loss.hip) run before they enqueue anything.  Plain C++ with no
// HIP dependency, so the same file is linked into libgsplat_hip.so and into
// the CPU sanitizer program tools/robust_loss_host_sanitize.c
// (tests/test_robust_loss.py).
#include <math.h>
#include <stdint.h>

#include "../../include/gs_robust_loss.h"
#include "gs_host_util.h"
#include "gs_robust_loss_layout.h"

using namespace gs;

namespace {
bool known_layout(int32_t l) { return l == GS_ROBUST_CHANNELS || l == GS_ROBUST_ROWS || l == GS_ROBUST_VALUES; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
}  // namespace

extern "C" {

size_t gs_robust_loss_struct_bytes(void) { return sizeof(gs_robust_loss); }

size_t gs_robust_loss_workspace_bytes(int32_t B, int32_t N, int32_t layout) {
  if (B <= 0 || N <= 0 || !known_layout(layout)) return 0;
  return RobustLossLayout(B, N, layout != GS_ROBUST_VALUES).total;
}

int gs_robust_loss_validate(const gs_robust_loss* a, int backward, const float* dL_dloss, const float* dL_dpred) {
  if (!a) return gs_set_error(-1, "robust loss: null argument block");
  if (!known_layout(a->layout)) return gs_set_error(-1, "robust loss: unknown layout %d", a->layout);
  if (a->B <= 0 || a->R <= 0 || a->N <= 0)
    return gs_set_error(-1, "robust loss: B, R, N must be > 0 (got %d, %d, %d)", a->B, a->R, a->N);
  if ((int64_t)a->B * a->N > INT32_MAX)
    return gs_set_error(-1, "robust loss: B * N = %lld does not fit int32", (long long)a->B * a->N);
  if (a->B > 65535) return gs_set_error(-1, "robust loss: batch of %d planes is too large", a->B);
  const bool values = a->layout == GS_ROBUST_VALUES;
  if (values && a->R != 1) return gs_set_error(-1, "robust loss: R must be 1 for GS_ROBUST_VALUES (got %d)", a->R);
  if (values && backward) return gs_set_error(-1, "robust loss: GS_ROBUST_VALUES has no backward");
  if (!a->pred) return gs_set_error(-1, "robust loss: pred is required");
  if (!values && !a->gt) return gs_set_error(-1, "robust loss: gt is required");
  if (!a->stats) return gs_set_error(-1, "robust loss: stats is required");
  if (!aligned4(a->pred) || !aligned4(a->gt)) return gs_set_error(-1, "robust loss: pred and gt must be 4-byte aligned");
  if (!aligned8(a->stats)) return gs_set_error(-1, "robust loss: stats must be 8-byte aligned");
  if (a->mask && a->mask_batch_stride != 0 && a->mask_batch_stride != a->N)
    return gs_set_error(-1, "robust loss: mask_batch_stride must be 0 or N = %d (got %lld)", a->N,
                        (long long)a->mask_batch_stride);
  if (a->over_masked && !a->mask) return gs_set_error(-1, "robust loss: over_masked needs a mask");
  if (!isfinite(a->quantile) || a->quantile < 0.0 || a->quantile > 1.0)
    return gs_set_error(-1, "robust loss: quantile must be in [0, 1] (got %g)", a->quantile);
  if (values && !a->select) return gs_set_error(-1, "robust loss: GS_ROBUST_VALUES needs select != 0");
  if (a->normalize && a->norm_width <= 0)
    return gs_set_error(-1, "robust loss: norm_width must be > 0 with normalize (got %d)", a->norm_width);
  if (backward) {
    if (!dL_dloss) return gs_set_error(-1, "robust loss backward: dL_dloss is required");
    if (!dL_dpred) return gs_set_error(-1, "robust loss backward: dL_dpred is required");
    if (!aligned4(dL_dloss) || !aligned4(dL_dpred))
      return gs_set_error(-1, "robust loss backward: gradient pointers must be 4-byte aligned");
  } else {
    if (!values && !a->losses) return gs_set_error(-1, "robust loss: losses is required");
    if (!aligned4(a->losses)) return gs_set_error(-1, "robust loss: losses must be 4-byte aligned");
    const RobustLossLayout L(a->B, a->N, !values);
    if (int e = check_workspace("robust loss", a->workspace, a->workspace_bytes, L.total)) return e;
  }
  return 0;
}

}  // extern "C"
