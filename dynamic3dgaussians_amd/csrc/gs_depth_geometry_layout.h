// gs_depth_geometry_layout.h -- launch geometry, size limits and the abs-rel
// workspace layout of the depth-map geometry kernels (gs_depth_geometry.hip),
// shared with their host-only validators (gs_depth_geometry_host.cpp).  Plain
// C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int DG_THREADS = 256;
constexpr int64_t DG_CHUNK = 4096;          // pixels of one image per abs-rel workgroup
constexpr int32_t DG_MAX_B = 65535;         // the batch is the grid's y extent
constexpr int32_t DG_MAX_SIDE = 32768;      // H, W: exact as floats, H * W * 3 below 2^32
constexpr int64_t DG_MAX_N = (int64_t)1 << 36;  // points / sample positions: N / DG_THREADS fits a grid's x extent

inline int64_t dg_blocks(int64_t n) { return (n + DG_THREADS - 1) / DG_THREADS; }

struct DepthAbsRelLayout {
  int64_t plane_elems, chunks;
  size_t partial, total;  // byte offsets
  DepthAbsRelLayout(int64_t B, int64_t H, int64_t W) {
    plane_elems = H * W;
    chunks = (plane_elems + DG_CHUNK - 1) / DG_CHUNK;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    partial = o; o = up(o + sizeof(double) * 2 * (size_t)(B * chunks));  // {sum, count} per workgroup
    total = o;
  }
};

}  // namespace gs
