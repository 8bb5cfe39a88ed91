// gs_loss_layout.h -- tile geometry and workspace layout of the photometric
// loss (gs_loss.hip), shared with its host-only validator (gs_loss_host.cpp).
// Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int PL_TILE = 32;                  // output tile, pixels per side
constexpr int PL_HALO = 5;                   // 11-tap window: 5 pixels each way
constexpr int PL_TAPS = 2 * PL_HALO + 1;
constexpr int PL_IN = PL_TILE + 2 * PL_HALO; // staged tile, pixels per side
constexpr int PL_THREADS = 256;

struct PhotoLossLayout {
  int64_t tiles_x, tiles_y, tiles, planes, blocks, plane_elems;
  size_t pqr, fwd_partial, bwd_partial, total;  // byte offsets
  PhotoLossLayout(int64_t B, int64_t Ch, int64_t H, int64_t W) {
    tiles_x = (W + PL_TILE - 1) / PL_TILE;
    tiles_y = (H + PL_TILE - 1) / PL_TILE;
    tiles = tiles_x * tiles_y;
    planes = B * Ch;
    blocks = planes * tiles;
    plane_elems = H * W;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    pqr = o;         o = up(o + sizeof(float) * 3 * (size_t)planes * (size_t)plane_elems);
    fwd_partial = o; o = up(o + sizeof(float) * 2 * (size_t)blocks);  // {sum |x - y|, sum ssim map} per workgroup
    bwd_partial = o; o = up(o + sizeof(float) * 2 * (size_t)blocks);  // {d gain, d offset} per workgroup
    total = o;
  }
};

}  // namespace gs
