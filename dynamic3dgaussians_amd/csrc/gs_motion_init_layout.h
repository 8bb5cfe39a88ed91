// gs_motion_init_layout.h -- launch geometry, size limits and the workspace
// layouts of the motion-basis initialisation kernels (gs_motion_init.hip),
// shared with their host-only validators (gs_motion_init_host.cpp).  Plain
// C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int MI_THREADS = 256;             // assign, coefficients, the update's second stage
constexpr int MI_MAX_K = 64;                // centres / bases: one register accumulator each in the assign kernel
constexpr int MI_ASSIGN_DC = 32;            // dimensions of the centres staged through LDS at a time
constexpr int MI_UPDATE_DC = 64;            // dimensions per update workgroup: one wave, a lane each
constexpr int64_t MI_UPDATE_SLICE = 512;    // points per update workgroup, at least
constexpr int64_t MI_UPDATE_MAX_BLOCKS = 1024;  // and at most this many workgroups along the points
constexpr int64_t MI_MAX_N = (int64_t)1 << 36;  // N / MI_THREADS fits a grid's x extent
constexpr int32_t MI_MAX_D = 1 << 20;       // D / MI_UPDATE_DC fits a grid's y extent; N * D below 2^62
constexpr int32_t MI_MAX_T = 1 << 18;       // frames: T / MI_FRAMES fits a grid's y extent
constexpr int MI_FRAMES = 8;                // frames per moments workgroup
constexpr int MI_POINT_LANES = MI_THREADS / MI_FRAMES;  // point lanes per frame of a moments workgroup
constexpr int MI_MOMENTS = 19;              // fp64 sums per (basis, frame)

inline int64_t mi_blocks(int64_t n) { return (n + MI_THREADS - 1) / MI_THREADS; }

// The update's partial sums: a function of the shapes alone, so two calls add in the same order.
struct KMeansLayout {
  int64_t slice, blocks;
  size_t partial, pcount, total;  // byte offsets
  KMeansLayout(int64_t N, int64_t K, int64_t D) {
    slice = (N + MI_UPDATE_MAX_BLOCKS - 1) / MI_UPDATE_MAX_BLOCKS;
    if (slice < MI_UPDATE_SLICE) slice = MI_UPDATE_SLICE;
    blocks = (N + slice - 1) / slice;
    if (blocks < 1) blocks = 1;  // N = 0: one block of zeros, every cluster empty
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    partial = o; o = up(o + sizeof(double) * (size_t)(blocks * K * D));
    pcount = o; o = up(o + sizeof(int64_t) * (size_t)(blocks * K));
    total = o;
  }
};

constexpr int MI_POSE = 12;                 // fp64 R (row-major) and t per (basis, frame), for the residual pass

struct ProcrustesLayout {
  size_t moments, poses, total;  // byte offsets
  ProcrustesLayout(int64_t K, int64_t T) {
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    moments = o; o = up(o + sizeof(double) * MI_MOMENTS * (size_t)(K * T));
    poses = o; o = up(o + sizeof(double) * MI_POSE * (size_t)(K * T));
    total = o;
  }
};

}  // namespace gs
