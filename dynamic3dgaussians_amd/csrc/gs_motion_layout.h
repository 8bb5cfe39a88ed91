// gs_motion_layout.h -- launch geometry, LDS budget and workspace layout of
// the motion-basis warp (gs_motion.hip), shared with its host-only validator
// (gs_motion_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int MT_MAX_K = 64, MT_MAX_B = 32;
constexpr int MT_THREADS = 256;           // Gaussians per workgroup (one thread each)
constexpr int MT_PAD = 4;                 // floats between two LDS columns' ends: rows stay 16-byte aligned
constexpr int MT_ROW = 9;                 // (rots | transls) floats per basis and frame
constexpr size_t MT_LDS_LIMIT = 160 * 1024;  // gfx950: LDS per CU, all of which one workgroup may use
constexpr int64_t MT_MAX_G = (int64_t)1 << 38;
constexpr int MT_SUM_LANES = 64, MT_SUM_SEGMENTS = 16;  // the slab sum: outputs x slab segments per workgroup

// LDS floats of one workgroup of `threads` Gaussians: the coefficient columns
// [K][threads + PAD], the staged bases [K][B][9], and in the backward the
// d_coefs columns and the per-frame (d_r6, dt) columns [9][threads + PAD].
inline size_t mt_lds_bytes(int K, int B, int threads, bool backward) {
  const size_t col = (size_t)threads + MT_PAD;
  size_t fl = (size_t)K * col + (size_t)K * B * MT_ROW;
  if (backward) fl += (size_t)K * col + (size_t)MT_ROW * col;
  return fl * sizeof(float);
}

// The backward halves its workgroup where 256 columns would not fit the LDS
// (K = 64 at B = 32: 145 KB with 128).
inline int mt_backward_threads(int K, int B) {
  return mt_lds_bytes(K, B, MT_THREADS, true) <= MT_LDS_LIMIT ? MT_THREADS : MT_THREADS / 2;
}

struct MotionLayout {
  int64_t blocks;             // workgroups of the backward = partial slabs
  size_t slab_floats;         // B * K * 9
  size_t slabs, sum, total;   // byte offsets
#ifdef GS_MOTION_STORE_SUM
  size_t pairs;               // [G, B, 9]: the timing-only store-and-sum alternative (gs_motion.hip)
#endif
  MotionLayout(int64_t G, int K, int B) {
    const int threads = mt_backward_threads(K, B);
    blocks = G > 0 ? (G + threads - 1) / threads : 0;
    slab_floats = (size_t)B * K * MT_ROW;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    slabs = o; o = up(o + (size_t)blocks * slab_floats * sizeof(float));
    sum = o;   o = up(o + slab_floats * sizeof(float));
#ifdef GS_MOTION_STORE_SUM
    pairs = o; o = up(o + (size_t)(G > 0 ? G : 0) * B * MT_ROW * sizeof(float));
#endif
    total = G > 0 ? o : 0;
  }
};

}  // namespace gs
