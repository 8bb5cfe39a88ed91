// gs_resample_layout.h -- the axis function of the bilinear resample
// (include/gs_resample.h), written once for the forward kernel, the backward
// kernel, the table kernel (gs_resample.hip) and the host-only export and
// validator (gs_resample_host.cpp): forward and backward agree on every floor
// decision by construction.  Also the thread decomposition and the backward's
// workspace layout.  Plain C++ on the host, no HIP dependency there.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_RS_HD __host__ __device__
#else
#define GS_RS_HD
#endif

namespace gs {

constexpr int RS_THREADS = 256;
constexpr int RS_VEC = 4;          // consecutive x per thread: one 16-byte store
constexpr int RS_MAX_SIZE = 32768; // per axis; o + 0.5f is exact up to 2^23
constexpr int RS_MAX_PLANE_GROUPS = 65535;  // the limit of gridDim.y
#ifndef GS_RS_TARGET_GROUPS
#define GS_RS_TARGET_GROUPS 2048  // 8 workgroups of 4 waves per CU
#endif
constexpr int RS_TARGET_GROUPS = GS_RS_TARGET_GROUPS;  // workgroups per backward launch aimed at
#ifndef GS_RS_PLANE_BATCH
#define GS_RS_PLANE_BATCH 4  // build.py's "rs_pb1" variant: 1
#endif
constexpr int RS_PB = GS_RS_PLANE_BATCH;  // planes a backward thread takes per step

// Source step per output index.  Computed on the host only (the kernels get
// the value as an argument), so host and device cannot differ in the division.
inline float resample_scale(int I, int O, int align_corners) {
  if (align_corners) return O > 1 ? (float)(I - 1) / (float)(O - 1) : 0.f;
  return (float)I / (float)O;
}

struct AxisTap {
  int i0, i1;     // lower and upper tap, both in [0, I)
  float l0, l1;   // their weights, l0 = 1 - l1
};

// Source coordinate of output index o.  Both forms are ONE rounding written
// as an explicit fmaf, so no compiler flag can contract them with what
// follows and host and device give the same bits:
//   align_corners     : round(scale * o)
//   half-pixel centres: max(0, round(scale * (o + 0.5) - 0.5)), the fused form
//                       torch's CPU kernel computes
GS_RS_HD inline float resample_src(float scale, int o, int align_corners) {
  if (align_corners) return fmaf(scale, (float)o, 0.f);
  return fmaxf(0.f, fmaf(scale, (float)o + 0.5f, -0.5f));
}

GS_RS_HD inline AxisTap resample_tap(float scale, int I, int o, int align_corners) {
  const float src = resample_src(scale, o, align_corners);
  AxisTap t;
  const int f = (int)src;
  t.i0 = f < I - 1 ? f : I - 1;
  t.i1 = t.i0 + 1 < I - 1 ? t.i0 + 1 : I - 1;
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// first[i], i in [0, I]: the smallest o with i0(o) >= i (O where there is
// none).  i0 is non-decreasing in o, so the outputs whose lower tap is i are
// [first[i], first[i + 1]).  Output o owns the entries (i0(o - 1), i0(o)],
// output 0 the entries [0, i0(0)] and the last output also (i0(O - 1), I]:
// every entry is written exactly once, by the table kernel with one thread
// per o and by the host export in a loop over o.
GS_RS_HD inline void resample_first_of(float scale, int I, int O, int o, int align_corners, int32_t* first) {
  const int hi = resample_tap(scale, I, o, align_corners).i0;
  const int lo = o > 0 ? resample_tap(scale, I, o - 1, align_corners).i0 + 1 : 0;
  for (int i = lo; i <= hi; ++i) first[i] = o;
  if (o == O - 1)
    for (int i = hi + 1; i <= I; ++i) first[i] = O;
}

// The backward's workspace: first_y [H + 1] then first_x [W + 1], int32.
struct ResampleLayout {
  size_t off_first_y, off_first_x, total;  // bytes
  ResampleLayout(int64_t H, int64_t W) {
    off_first_y = 0;
    off_first_x = ((size_t)(H + 1) * sizeof(int32_t) + 15) / 16 * 16;
    total = off_first_x + ((size_t)(W + 1) * sizeof(int32_t) + 15) / 16 * 16;
  }
};

// Threads of a plane of R rows by C columns: one per RS_VEC consecutive x of a row.
inline int64_t resample_quads(int64_t C) { return (C + RS_VEC - 1) / RS_VEC; }
inline int64_t resample_groups(int64_t R, int64_t C) { return (R * resample_quads(C) + RS_THREADS - 1) / RS_THREADS; }
// gridDim.y of the forward: a workgroup per plane and chunk (measured faster
// than walking planes there); past the grid's limit a thread
// walks the planes with that stride.
inline int64_t resample_fwd_plane_groups(int64_t planes) {
  return planes < RS_MAX_PLANE_GROUPS ? planes : RS_MAX_PLANE_GROUPS;
}
// gridDim.y of the backward: a thread takes RS_PB planes per step (one set of
// taps and weights, RS_PB independent loads per term) and walks further steps
// with stride gridDim.y * RS_PB; about RS_TARGET_GROUPS workgroups per launch.
inline int64_t resample_bwd_plane_groups(int64_t planes, int64_t groups) {
  int64_t g = RS_TARGET_GROUPS / groups;
  const int64_t steps = (planes + RS_PB - 1) / RS_PB;
  if (g > RS_MAX_PLANE_GROUPS) g = RS_MAX_PLANE_GROUPS;
  if (g > steps) g = steps;
  return g < 1 ? 1 : g;
}

}  // namespace gs
