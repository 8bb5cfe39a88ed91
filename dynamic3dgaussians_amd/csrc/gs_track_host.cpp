// gs_track_host.cpp -- host-only part of the tracking C ABI
// (include/gs_track.h): the argument validators that gs_contributors_batch
// and gs_track_project (gs_api.hip) run before they enqueue anything.  Plain
// C++ with no HIP dependency, so the same file is linked into
// libgsplat_hip.so and into the CPU sanitizer program
// tools/track_host_sanitize.c.
#include <stdint.h>

#include <initializer_list>

#include "../../include/gs_track.h"
#include "gs_host_util.h"

using namespace gs;

namespace {

// a * b * c * d for non-negative factors, or -1 past 2^62
int64_t product(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t lim = (int64_t)1 << 62;
  int64_t n = 1;
  for (int64_t f : {a, b, c, d}) {
    if (f == 0) return 0;
    if (n > lim / f) return -1;
    n *= f;
  }
  return n;
}

}  // namespace

extern "C" {

int gs_check_contributors(int64_t P, int32_t C, int32_t W, int32_t H, int32_t K, const int32_t* top_id,
                          const float* top_w) {
  if (P < 0 || P > 0x7FFFFFFF) return gs_set_error(-1, "contributors: P must be in [0, 2^31) (got %lld)", (long long)P);
  if (C < 1 || C > GS_TRACK_MAX_CAMS)
    return gs_set_error(-1, "contributors: camera batch size %d outside 1..%d", C, GS_TRACK_MAX_CAMS);
  if (K < 1 || K > GS_TRACK_MAX_K) return gs_set_error(-1, "contributors: K = %d outside 1..%d", K, GS_TRACK_MAX_K);
  if (W < 0 || H < 0) return gs_set_error(-1, "contributors: image size must not be negative (got %dx%d)", W, H);
  const int64_t n = product(C, K, H, W);
  if (n < 0) return gs_set_error(-1, "contributors: %d x %d x %d x %d elements exceed 2^62", C, K, H, W);
  if (n == 0) return 0;
  if (!top_id || !top_w) return gs_set_error(-1, "contributors: top_id and top_w are required");
  if (!aligned4(top_id) || !aligned4(top_w)) return gs_set_error(-1, "contributors: the outputs must be 4-byte aligned");
  return 0;
}

int gs_check_track_project(int64_t P, int32_t T, int32_t C, int64_t N, const int32_t* ids, const float* uv,
                           const float* depth, const uint8_t* inside) {
  if (P < 0 || P > 0x7FFFFFFF) return gs_set_error(-1, "track project: P must be in [0, 2^31) (got %lld)", (long long)P);
  if (C < 1 || C > GS_TRACK_MAX_CAMS)
    return gs_set_error(-1, "track project: camera batch size %d outside 1..%d", C, GS_TRACK_MAX_CAMS);
  if (T < 0) return gs_set_error(-1, "track project: T must not be negative (got %d)", T);
  if (N < 0) return gs_set_error(-1, "track project: N must not be negative (got %lld)", (long long)N);
  const int64_t n = product(T, C, N, 1);
  if (n < 0) return gs_set_error(-1, "track project: %d x %d x %lld elements exceed 2^62", T, C, (long long)N);
  if (n == 0) return 0;
  if (!ids) return gs_set_error(-1, "track project: ids are required");
  if (!aligned4(ids)) return gs_set_error(-1, "track project: ids must be 4-byte aligned");
  if (!uv || !depth || !inside) return gs_set_error(-1, "track project: uv, depth and inside are required");
  if ((reinterpret_cast<uintptr_t>(uv) & 7u) != 0) return gs_set_error(-1, "track project: uv must be 8-byte aligned");
  if (!aligned4(depth)) return gs_set_error(-1, "track project: depth must be 4-byte aligned");
  return 0;
}

}  // extern "C"
