// gs_motion_init_host.cpp -- host-only part of the motion-basis
// initialisation's C ABI (include/gs_motion_init.h): struct sizes, workspace
// sizes and the argument validators that the entry points
// (gs_motion_init.hip) run before they enqueue anything.  Plain C++ with no
// HIP dependency, so the same file is linked into libgsplat_hip.so and into
// the CPU sanitizer program tools/motion_init_host_sanitize.c
// (tests/test_motion_init.py).
#include <stdint.h>

#include "../../include/gs_motion_init.h"
#include "gs_host_util.h"
#include "gs_motion_init_layout.h"

using namespace gs;

namespace {

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// N, D, K of a k-means call.
int check_kmeans_shape(const char* who, int64_t N, int32_t D, int32_t K) {
  if (N < 0 || N > MI_MAX_N) return gs_set_error(-1, "%s: N must be in [0, 2^36] (got %lld)", who, (long long)N);
  if (D < 1 || D > MI_MAX_D) return gs_set_error(-1, "%s: D must be in [1, %d] (got %d)", who, MI_MAX_D, D);
  if (K < 1 || K > MI_MAX_K) return gs_set_error(-1, "%s: K must be in [1, %d] (got %d)", who, MI_MAX_K, K);
  return 0;
}

}  // namespace

extern "C" {

size_t gs_kmeans_assign_struct_bytes(void) { return sizeof(struct gs_kmeans_assign); }
size_t gs_kmeans_update_struct_bytes(void) { return sizeof(struct gs_kmeans_update); }
size_t gs_coefs_from_centers_struct_bytes(void) { return sizeof(struct gs_coefs_from_centers); }
size_t gs_procrustes_struct_bytes(void) { return sizeof(struct gs_procrustes); }

size_t gs_kmeans_workspace_bytes(int64_t N, int32_t K, int32_t D) {
  if (N < 0 || N > MI_MAX_N || K < 1 || K > MI_MAX_K || D < 1 || D > MI_MAX_D) return 0;
  return KMeansLayout(N, K, D).total;
}

size_t gs_procrustes_workspace_bytes(int32_t K, int32_t T) {
  if (K < 1 || K > MI_MAX_K || T < 1 || T > MI_MAX_T) return 0;
  return ProcrustesLayout(K, T).total;
}

int gs_kmeans_assign_validate(const struct gs_kmeans_assign* a) {
  if (!a) return gs_set_error(-1, "kmeans assign: null argument block");
  if (int e = check_kmeans_shape("kmeans assign", a->N, a->D, a->K)) return e;
  if (a->N > 0 && !a->x) return gs_set_error(-1, "kmeans assign: x is required when N > 0");
  if (!a->centers) return gs_set_error(-1, "kmeans assign: centers are required");
  if (a->N > 0 && !a->labels) return gs_set_error(-1, "kmeans assign: labels are required when N > 0");
  if ((a->moved != nullptr) != (a->prev_labels != nullptr))
    return gs_set_error(-1, "kmeans assign: prev_labels and moved go together");
  if (!aligned4(a->x) || !aligned4(a->centers))
    return gs_set_error(-1, "kmeans assign: x and centers must be 4-byte aligned");
  if (!aligned8(a->labels) || !aligned8(a->prev_labels) || !aligned8(a->moved))
    return gs_set_error(-1, "kmeans assign: labels, prev_labels and moved must be 8-byte aligned");
  return 0;
}

int gs_kmeans_update_validate(const struct gs_kmeans_update* a) {
  if (!a) return gs_set_error(-1, "kmeans update: null argument block");
  if (int e = check_kmeans_shape("kmeans update", a->N, a->D, a->K)) return e;
  if (a->N > 0 && (!a->x || !a->labels)) return gs_set_error(-1, "kmeans update: x and labels are required when N > 0");
  if (!a->centers) return gs_set_error(-1, "kmeans update: centers are required");
  if (!a->counts) return gs_set_error(-1, "kmeans update: counts are required");
  if (!aligned4(a->x) || !aligned4(a->centers))
    return gs_set_error(-1, "kmeans update: x and centers must be 4-byte aligned");
  if (!aligned8(a->labels) || !aligned8(a->counts))
    return gs_set_error(-1, "kmeans update: labels and counts must be 8-byte aligned");
  return check_workspace("kmeans update", a->workspace, a->workspace_bytes, KMeansLayout(a->N, a->K, a->D).total);
}

int gs_coefs_from_centers_validate(const struct gs_coefs_from_centers* a) {
  if (!a) return gs_set_error(-1, "coefs from centers: null argument block");
  if (a->N < 0 || a->N > MI_MAX_N)
    return gs_set_error(-1, "coefs from centers: N must be in [0, 2^36] (got %lld)", (long long)a->N);
  if (a->K < 1 || a->K > (1 << 20))
    return gs_set_error(-1, "coefs from centers: K must be in [1, 2^20] (got %d)", a->K);
  if (a->N > 0 && (!a->means || !a->coefs))
    return gs_set_error(-1, "coefs from centers: means and coefs are required when N > 0");
  if (!a->centers) return gs_set_error(-1, "coefs from centers: centers are required");
  if (!aligned4(a->means) || !aligned4(a->centers) || !aligned4(a->coefs))
    return gs_set_error(-1, "coefs from centers: means, centers and coefs must be 4-byte aligned");
  return 0;
}

int gs_procrustes_validate(const struct gs_procrustes* a) {
  if (!a) return gs_set_error(-1, "procrustes: null argument block");
  if (a->N < 0 || a->N > MI_MAX_N)
    return gs_set_error(-1, "procrustes: N must be in [0, 2^36] (got %lld)", (long long)a->N);
  if (a->T < 1 || a->T > MI_MAX_T) return gs_set_error(-1, "procrustes: T must be in [1, %d] (got %d)", MI_MAX_T, a->T);
  if (a->K < 1 || a->K > MI_MAX_K) return gs_set_error(-1, "procrustes: K must be in [1, %d] (got %d)", MI_MAX_K, a->K);
  if (a->cano_t < 0 || a->cano_t >= a->T)
    return gs_set_error(-1, "procrustes: cano_t = %d is outside [0, %d)", a->cano_t, a->T);
  if (a->rot_dim != 4 && a->rot_dim != 6)
    return gs_set_error(-1, "procrustes: rot_dim must be 4 or 6 (got %d)", a->rot_dim);
  if (!(a->min_weight_sum == a->min_weight_sum))
    return gs_set_error(-1, "procrustes: min_weight_sum must not be NaN");
  if (a->N > 0 && (!a->tracks || !a->order))
    return gs_set_error(-1, "procrustes: tracks and order are required when N > 0");
  if (!a->offsets) return gs_set_error(-1, "procrustes: offsets are required");
  if (!a->rots || !a->transls) return gs_set_error(-1, "procrustes: rots and transls are required");
  if (!a->err_after || !a->err_before || !a->skipped)
    return gs_set_error(-1, "procrustes: err_after, err_before and skipped are required");
  if (!aligned4(a->tracks) || !aligned4(a->weights) || !aligned4(a->confidences) || !aligned4(a->rots) ||
      !aligned4(a->transls) || !aligned4(a->err_after) || !aligned4(a->err_before))
    return gs_set_error(-1, "procrustes: the fp32 tensors must be 4-byte aligned");
  if (!aligned8(a->order) || !aligned8(a->offsets))
    return gs_set_error(-1, "procrustes: order and offsets must be 8-byte aligned");
  return check_workspace("procrustes", a->workspace, a->workspace_bytes, ProcrustesLayout(a->K, a->T).total);
}

}  // extern "C"
