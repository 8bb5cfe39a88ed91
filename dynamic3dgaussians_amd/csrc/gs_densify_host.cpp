// gs_densify_host.cpp -- host-only part of densification's C ABI
// (include/gs_densify.h): the size queries and the two argument validators
// that gs_densify_plan / gs_densify_apply (gs_densify.hip) run before they
// enqueue anything.  Plain C++ with no HIP dependency, so the same file is
// linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/densify_host_sanitize.c (tests/test_densify.py).
#include <math.h>
#include <stdint.h>

#include "../../include/gs_densify.h"
#include "gs_densify_layout.h"
#include "gs_host_util.h"

using namespace gs;

namespace {
const char* const ROLE_NAME[] = {"plain", "means", "log_scales", "rotations", "logit_opacities"};
const int ROLE_WIDTH[] = {0, 3, 3, 4, 1};
}  // namespace

extern "C" {

size_t gs_densify_plan_struct_bytes(void) { return sizeof(gs_densify_plan_args); }
size_t gs_densify_tensor_struct_bytes(void) { return sizeof(gs_densify_tensor); }
size_t gs_densify_apply_struct_bytes(void) { return sizeof(gs_densify_apply_args); }

size_t gs_densify_workspace_bytes(int64_t P) { return (P <= 0 || P > DN_MAX_P) ? 0 : DensifyLayout(P).total; }
size_t gs_densify_counts_offset(int64_t P) { return DensifyLayout(P).counts; }
size_t gs_densify_flags_offset(int64_t P) { return DensifyLayout(P).flags; }
size_t gs_densify_ranks_offset(int64_t P) { return DensifyLayout(P).ranks; }
int64_t gs_densify_scan_block(void) { return DN_BLOCK; }
int64_t gs_densify_scan_tile(void) { return DN_TILE; }

int64_t gs_densify_new_count(const int64_t counts[4], int32_t n_split) {
  if (!counts) return 0;
  return counts[GS_DENSIFY_KEPT_ORIGINALS] + counts[GS_DENSIFY_KEPT_CLONES] +
         (int64_t)n_split * counts[GS_DENSIFY_KEPT_SPLITS];
}

int gs_densify_plan_validate(const gs_densify_plan_args* a) {
  if (!a) return gs_set_error(-1, "densify plan: null argument block");
  if (a->P < 0 || a->P > DN_MAX_P)
    return gs_set_error(-1, "densify plan: P must be in [0, %lld] (got %lld)", (long long)DN_MAX_P, (long long)a->P);
  if (a->n_split != GS_DENSIFY_N_SPLIT)
    return gs_set_error(-1, "densify plan: n_split must be %d (got %d)", GS_DENSIFY_N_SPLIT, a->n_split);
  if (!isfinite(a->grad_thresh) || !isfinite(a->clone_max_scale) || !isfinite(a->prune_min_opacity) ||
      !isfinite(a->prune_max_scale))
    return gs_set_error(-1, "densify plan: the thresholds must be finite");
  if (a->P == 0) return 0;
  if (!a->grad_accum || !a->denom || !a->log_scales || !a->logit_opacities)
    return gs_set_error(-1, "densify plan: grad_accum, denom, log_scales and logit_opacities are required");
  if (!aligned4(a->grad_accum) || !aligned4(a->denom) || !aligned4(a->log_scales) || !aligned4(a->logit_opacities))
    return gs_set_error(-1, "densify plan: the inputs must be 4-byte aligned");
  return check_workspace("densify plan", a->workspace, a->workspace_bytes, DensifyLayout(a->P).total);
}

int gs_densify_apply_validate(const gs_densify_apply_args* a) {
  if (!a) return gs_set_error(-1, "densify apply: null argument block");
  if (a->P < 0 || a->P > DN_MAX_P)
    return gs_set_error(-1, "densify apply: P must be in [0, %lld] (got %lld)", (long long)DN_MAX_P, (long long)a->P);
  if (a->n_split != GS_DENSIFY_N_SPLIT)
    return gs_set_error(-1, "densify apply: n_split must be %d (got %d)", GS_DENSIFY_N_SPLIT, a->n_split);
  if (a->n_tensors < 0 || a->n_tensors > GS_DENSIFY_MAX_TENSORS)
    return gs_set_error(-1, "densify apply: n_tensors must be in [0, %d] (got %d)", GS_DENSIFY_MAX_TENSORS,
                        a->n_tensors);
  const int64_t ko = a->counts[GS_DENSIFY_KEPT_ORIGINALS], kc = a->counts[GS_DENSIFY_KEPT_CLONES];
  const int64_t as = a->counts[GS_DENSIFY_ALL_SPLITS], ks = a->counts[GS_DENSIFY_KEPT_SPLITS];
  if (ko < 0 || kc < 0 || as < 0 || ks < 0 || ks > as || ko + as > a->P || kc + as > a->P)
    return gs_set_error(-1, "densify apply: counts (%lld, %lld, %lld, %lld) do not fit P = %lld", (long long)ko,
                        (long long)kc, (long long)as, (long long)ks, (long long)a->P);
  if (a->reset_opacity && !isfinite(a->opacity_reset))
    return gs_set_error(-1, "densify apply: opacity_reset must be finite");
  int seen[5] = {0, 0, 0, 0, 0};
  for (int t = 0; t < a->n_tensors; ++t) {
    const gs_densify_tensor& x = a->t[t];
    if (x.width <= 0 || x.width > DN_MAX_WIDTH)
      return gs_set_error(-1, "densify apply: tensor %d: width must be in [1, %d] (got %d)", t, DN_MAX_WIDTH, x.width);
    if (x.role < GS_DENSIFY_ROLE_PLAIN || x.role > GS_DENSIFY_ROLE_LOGIT_OPACITIES)
      return gs_set_error(-1, "densify apply: tensor %d: unknown role %d", t, x.role);
    if (x.role != GS_DENSIFY_ROLE_PLAIN) {
      if (seen[x.role]++) return gs_set_error(-1, "densify apply: role %s is used twice", ROLE_NAME[x.role]);
      if (x.width != ROLE_WIDTH[x.role])
        return gs_set_error(-1, "densify apply: tensor %d: role %s has width %d (got %d)", t, ROLE_NAME[x.role],
                            ROLE_WIDTH[x.role], x.width);
    }
    if (a->P > 0 && !x.src) return gs_set_error(-1, "densify apply: tensor %d: src is required", t);
    if (gs_densify_new_count(a->counts, a->n_split) > 0 && !x.dst)
      return gs_set_error(-1, "densify apply: tensor %d: dst is required", t);
    if (!aligned4(x.src) || !aligned4(x.src_exp_avg) || !aligned4(x.src_exp_avg_sq) || !aligned4(x.dst) ||
        !aligned4(x.dst_exp_avg) || !aligned4(x.dst_exp_avg_sq))
      return gs_set_error(-1, "densify apply: tensor %d: pointers must be 4-byte aligned", t);
    if ((x.dst_exp_avg == nullptr) != (x.dst_exp_avg_sq == nullptr) ||
        (x.src_exp_avg == nullptr) != (x.src_exp_avg_sq == nullptr))
      return gs_set_error(-1, "densify apply: tensor %d: exp_avg and exp_avg_sq come together", t);
  }
  for (int r = GS_DENSIFY_ROLE_MEANS; r <= GS_DENSIFY_ROLE_LOGIT_OPACITIES; ++r)
    if (!seen[r]) return gs_set_error(-1, "densify apply: role %s is missing", ROLE_NAME[r]);
  if (ks > 0 && !a->noise)
    return gs_set_error(-1, "densify apply: noise is required (%lld rows)", (long long)(a->n_split * as));
  if (!aligned4(a->noise) || !aligned4(a->stats[0]) || !aligned4(a->stats[1]) || !aligned4(a->stats[2]))
    return gs_set_error(-1, "densify apply: noise and stats must be 4-byte aligned");
  return check_workspace("densify apply", a->workspace, a->workspace_bytes, DensifyLayout(a->P).total);
}

}  // extern "C"
