// gs_metrics_layout.h -- tile geometry and workspace layout of the evaluation
// metrics (gs_metrics.hip), shared with their host-only validators
// (gs_metrics_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int MT_TILE = 32;                   // tile, pixels per side (inputs owned and outputs)
constexpr int MT_TAPS = 11;                   // the window
constexpr int MT_IN = MT_TILE + MT_TAPS - 1;  // staged tile, pixels per side ("valid" window: halo to the right / below)
constexpr int MT_THREADS = 256;
constexpr int MT_SUMS = 4;                    // sse, sae, mask_sum, ssim
constexpr int MT_IOU_THREADS = 256;
constexpr int64_t MT_IOU_CHUNK = 16 * 1024;   // pixels of one image per mask-IoU workgroup

struct ImageMetricsLayout {
  int64_t tiles_x, tiles_y, tiles, planes, blocks, plane_elems;
  size_t partial, total;  // byte offsets
  ImageMetricsLayout(int64_t B, int64_t Ch, int64_t H, int64_t W) {
    // the tiling covers H x W, not the (H - 10) x (W - 10) outputs: every input pixel belongs
    // to exactly one workgroup for the three plain sums
    tiles_x = (W + MT_TILE - 1) / MT_TILE;
    tiles_y = (H + MT_TILE - 1) / MT_TILE;
    tiles = tiles_x * tiles_y;
    planes = B * Ch;
    blocks = planes * tiles;
    plane_elems = H * W;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    partial = o; o = up(o + sizeof(float) * MT_SUMS * (size_t)blocks);  // MT_SUMS per workgroup
    total = o;
  }
};

}  // namespace gs
