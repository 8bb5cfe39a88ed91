// gs_robust_loss_layout.h -- workgroup decomposition and workspace layout of
// the quantile-trimmed losses (gs_robust_loss.hip), shared with their
// host-only validator (gs_robust_loss_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int RL_THREADS = 256;
constexpr int RL_UNROLL = 4;                         // elements per thread and chunk, RL_THREADS apart
constexpr int RL_CHUNK = RL_THREADS * RL_UNROLL;     // elements per workgroup and chunk
// Workgroups per plane, every streaming pass: one per chunk up to 128; past
// that a workgroup walks the plane's chunks with stride `groups`, so the
// histogram merge (one integer atomic per non-empty bin and workgroup) and the
// partial sums (one record per workgroup) stay small against the streaming.
constexpr int RL_MAX_GROUPS = 128;
// The radix select's digits, most significant first: 11 + 10 + 10 bits of the
// 31 value bits of a non-negative float.
constexpr int RL_BITS1 = 11, RL_BITS2 = 10, RL_BITS3 = 10;
constexpr int RL_BINS1 = 1 << RL_BITS1, RL_BINS2 = 1 << RL_BITS2, RL_BINS3 = 1 << RL_BITS3;
constexpr int RL_STATE_WORDS = 16;                   // uint32 words of selection state per plane
constexpr int RL_PART = 4;                           // doubles per workgroup record: S, cnt, cm, unused
constexpr int RL_STATS = 4;                          // doubles per plane in `stats`

struct RobustLossLayout {
  int64_t chunks, groups;                            // per plane
  // byte offsets: the state and the three histograms come first and are
  // zeroed as one range of `zero_bytes`
  size_t state, hist1, hist2, hist3, zero_bytes, partials, plane, total;
  RobustLossLayout(int64_t B, int64_t N, bool with_plane) {
    chunks = (N + RL_CHUNK - 1) / RL_CHUNK;
    groups = chunks < RL_MAX_GROUPS ? chunks : RL_MAX_GROUPS;
    const size_t b = (size_t)B, u = sizeof(uint32_t);
    state = 0;
    hist1 = state + b * RL_STATE_WORDS * u;
    hist2 = hist1 + b * RL_BINS1 * u;
    hist3 = hist2 + b * 2 * RL_BINS2 * u;
    zero_bytes = hist3 + b * 2 * RL_BINS3 * u;
    partials = zero_bytes;                           // a multiple of 64 bytes
    plane = partials + b * (size_t)groups * RL_PART * sizeof(double);
    total = plane + (with_plane ? b * (size_t)N * sizeof(float) : 0);
    total = (total + 15) / 16 * 16;
  }
};

}  // namespace gs
