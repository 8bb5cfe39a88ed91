// gs_feature_decoder_host.cpp -- host-only part of the feature decoder's C ABI
// (include/gs_feature_decoder.h): the struct size, the workspace sizes, the
// documented constants and the argument validator that every entry point of
// gs_feature_decoder.hip runs before it enqueues anything.  Plain C++ with no
// HIP dependency, so the same file is linked into libgsplat_hip.so and into
// the CPU sanitizer program tools/feature_decoder_host_sanitize.c
// (tests/test_feature_decoder.py).
#include <stdint.h>

#include "../../include/gs_feature_decoder.h"
#include "gs_feature_decoder_layout.h"
#include "gs_host_util.h"

using namespace gs;

namespace {
const char* const PASS_NAME[4] = {"feature decoder forward", "feature decoder loss forward",
                                  "feature decoder loss backward", "feature decoder backward"};
}  // namespace

extern "C" {

size_t gs_feature_decoder_struct_bytes(void) { return sizeof(gs_feature_decoder); }

size_t gs_feature_decoder_workspace_bytes(int32_t B, int32_t F_in, int32_t C_out, int32_t h, int32_t w, int32_t pass) {
  if (!fd_sizes_ok(B, F_in, C_out, h, w) || pass < 0 || pass > 3) return 0;
  return FeatureDecoderLayout(B, F_in, C_out, h, w, pass).total;
}

int32_t gs_feature_decoder_grid_x(int32_t B, int32_t h, int32_t w) {
  if (!fd_sizes_ok(B, 1, 1, h, w)) return 0;
  return (int32_t)fd_grid_x(B, h, w, GS_FD_PASS_BACKWARD);
}

int32_t gs_feature_decoder_n_t(int32_t C_out) {
  if (C_out < 1 || C_out > GS_FD_MAX_C_OUT) return 0;
  return 16 * fd_row_tiles(C_out);
}

int64_t gs_feature_decoder_n_acc(int32_t B, int32_t h, int32_t w) {
  if (!fd_sizes_ok(B, 1, 1, h, w)) return 0;
  const int64_t gx = fd_grid_x(B, h, w, GS_FD_PASS_BACKWARD);
  return (fd_tiles(h, w) + gx - 1) / gx * FD_PIX;
}

int gs_feature_decoder_validate(const gs_feature_decoder* a, int32_t pass) {
  if (!a) return gs_set_error(-1, "feature decoder: null argument block");
  if (pass < 0 || pass > 3) return gs_set_error(-1, "feature decoder: unknown pass %d", pass);
  const char* who = PASS_NAME[pass];
  if (a->B < 1 || a->B > 65535) return gs_set_error(-1, "%s: B must be in [1, 65535] (got %d)", who, a->B);
  if (a->F_in < 1 || a->F_in > GS_FD_MAX_F_IN)
    return gs_set_error(-1, "%s: F_in must be in [1, %d] (got %d); decode_features_torch / decoded_l1_loss_torch "
                        "take any size", who, GS_FD_MAX_F_IN, a->F_in);
  if (a->C_out < 1 || a->C_out > GS_FD_MAX_C_OUT)
    return gs_set_error(-1, "%s: C_out must be in [1, %d] (got %d); decode_features_torch / decoded_l1_loss_torch "
                        "take any size", who, GS_FD_MAX_C_OUT, a->C_out);
  if ((int64_t)a->F_in * a->C_out > GS_FD_MAX_WEIGHTS)
    return gs_set_error(-1, "%s: F_in * C_out must be <= %d (got %d * %d); decode_features_torch / "
                        "decoded_l1_loss_torch take any size", who, GS_FD_MAX_WEIGHTS, a->F_in, a->C_out);
  if (a->h < 1 || a->w < 1 || !fd_sizes_ok(a->B, a->F_in, a->C_out, a->h, a->w))
    return gs_set_error(-1, "%s: h, w must be >= 1 with h * w < 2^31 - %d (got %d, %d); decode_features_torch / "
                        "decoded_l1_loss_torch take any size", who, FD_PIX, a->h, a->w);
  const bool loss = pass == GS_FD_PASS_LOSS || pass == GS_FD_PASS_LOSS_BACKWARD;
  const bool bwd = pass == GS_FD_PASS_LOSS_BACKWARD || pass == GS_FD_PASS_BACKWARD;
  if (!a->weight) return gs_set_error(-1, "%s: weight is required", who);
  if (pass != GS_FD_PASS_BACKWARD && !a->x) return gs_set_error(-1, "%s: x is required", who);
  if (pass == GS_FD_PASS_BACKWARD && !a->x) return gs_set_error(-1, "%s: x is required (for d_weight)", who);
  if (loss && !a->target) return gs_set_error(-1, "%s: target is required", who);
  if (pass == GS_FD_PASS_DECODE && !a->y) return gs_set_error(-1, "%s: y is required", who);
  if (pass == GS_FD_PASS_LOSS && !a->loss) return gs_set_error(-1, "%s: loss is required", who);
  if (pass == GS_FD_PASS_LOSS_BACKWARD && !a->up) return gs_set_error(-1, "%s: up is required", who);
  if (pass == GS_FD_PASS_BACKWARD && !a->d_y) return gs_set_error(-1, "%s: d_y is required", who);
  if (bwd && !a->d_x) return gs_set_error(-1, "%s: d_x is required", who);
  if (bwd && !a->d_weight) return gs_set_error(-1, "%s: d_weight is required", who);
  const void* const ptrs[] = {a->x, a->weight, a->bias, a->target, a->mask, a->up, a->d_y,
                              a->y, a->loss, a->d_x, a->d_weight, a->d_bias};
  for (const void* p : ptrs)
    if (!aligned4(p)) return gs_set_error(-1, "%s: every pointer must be 4-byte aligned", who);
  return check_workspace(who, a->workspace, a->workspace_bytes,
                         FeatureDecoderLayout(a->B, a->F_in, a->C_out, a->h, a->w, pass).total);
}

}  // extern "C"
