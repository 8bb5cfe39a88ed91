// gs_densify_layout.h -- scan geometry and workspace layout of densification
// (gs_densify.hip), shared with its host-only validator (gs_densify_host.cpp).
// Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int DN_THREADS = 256;
constexpr int DN_ITEMS = 4;                       // Gaussians per thread of a scan workgroup
constexpr int DN_BLOCK = DN_THREADS * DN_ITEMS;   // Gaussians per scan workgroup
constexpr int DN_TILE = DN_THREADS * DN_ITEMS;    // block sums per pass of the block-sum scan
constexpr int64_t DN_MAX_P = (int64_t)1 << 30;    // ranks are int32 and a split doubles
constexpr int DN_MAX_WIDTH = 1 << 16;

struct DensifyLayout {
  int64_t P, blocks;
  size_t counts, flags, ranks, sums, total;  // byte offsets
  explicit DensifyLayout(int64_t P_) {
    P = P_ < 0 ? 0 : P_;
    blocks = (P + DN_BLOCK - 1) / DN_BLOCK;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    counts = o; o = up(o + 4 * sizeof(int64_t));               // the four totals
    flags = o;  o = up(o + (size_t)P);                         // one byte per Gaussian
    ranks = o;  o = up(o + 4 * sizeof(int32_t) * (size_t)P);   // four exclusive ranks per Gaussian
    sums = o;   o = up(o + 4 * sizeof(int32_t) * (size_t)blocks);  // four sums per scan workgroup
    total = P > 0 ? o : 0;
  }
};

}  // namespace gs
