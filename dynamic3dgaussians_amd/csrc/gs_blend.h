// gs_blend.h -- device helpers shared by the kernels that walk the tile lists
// strip by strip: the blend kernels (gs_render.hip) and the contributor kernel
// (gs_track.hip).  The workgroup -> (camera, strip) dispatch, the record
// gather, the strip cull and the exponent arithmetic live here once, so that
// every kernel that repeats the forward's walk computes the forward's power
// and alpha bit for bit.  Nothing in here has a contractable multiply-add
// outside an explicit fmaf, so the results do not depend on a file's
// -ffp-contract setting.
#pragma once

#include "gs_common.h"

namespace gs {

constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr int CHUNK = 64;

__device__ inline bool wave_any(bool p) { return __ballot(p) != 0ull; }

// Workgroup -> (camera, slot) of a batch launch: groups of 8 cameras one
// after the other, camera-minor inside a group -- block b of a group is
// camera g0 + b % 8, tile slot b / 8.  Workgroups are dealt to the 8 XCDs
// round-robin (b % 8), so while a group runs each XCD renders ONE camera:
// the 4 strip workgroups of a backward tile (slots 4t .. 4t+3, blocks 8 apart)
// and the neighbouring tiles of the camera share that XCD's L2, and every
// camera's longest tiles still start first.  Measured at the 27-camera batch
// (profiles/r03n_*): render_bwd HBM reads 6.3 vs 20.1 GB per launch against
// all 27 cameras interleaved (each tile's strips then sat on 4 different XCDs
// and fetched the tile's records 4 times), 5.26-5.39 vs 5.30-5.45 ms.
// Camera-major order (all of camera 0's workgroups, then camera 1's, ...)
// measured 5.55 vs 5.23 ms: every strip in flight adds into
// the same camera's accumulation records and the contended float atomics
// cost more than the locality gains.  A final group of C % 8 cameras is
// interleaved the same way without the one-camera-per-XCD property.
constexpr int CAM_GROUP = 8;  // cameras interleaved at a time (8 = one per XCD)
__device__ inline void cam_slot(int bid, int C, int per_cam, int& cam, int& slot) {
  // groups of CAM_GROUP cameras one after the other, camera-minor inside
  const int G = CAM_GROUP < C ? CAM_GROUP : C;
  const int grp = bid / (G * per_cam), r = bid - grp * G * per_cam;
  const int g0 = grp * G, gn = C - g0 < G ? C - g0 : G;  // the last group may be smaller
  cam = g0 + r % gn;
  slot = r / gn;
}
// Workgroup -> (camera, strip item) of the wave-per-workgroup blend
// kernels.  A (camera, tile) unit is 4 strip workgroups, and those 4 sit on
// one XCD (one L2 fill of the tile's records and feature rows): units are
// dealt 8 at a time, one per XCD -- the k-th group of 8 units is blocks
// 32k .. 32k+31, block 32k + 8s + x holding strip s of unit 8k + (x + r) mod 8
// on XCD x (r = k at C < 8, else 0: see below).  Units are ordered by
// cam_slot (groups of 8 cameras, camera-minor, longest tiles first).  At
// C < 8 (an 8-rank split: 3-4 cameras per rank) the groups are rotated by k:
// without it XCD x rendered only camera x mod C, and the XCDs holding the
// heavier cameras finished last (per-XCD work at 4 cameras 698-809 us of
// the 850 us backward, tools/batch_steps.py --stamps; 4-camera backward
// 0.785-0.798 vs 0.825-0.832 ms rotated, profiles/r04j/).  At C >= 8 each XCD
// renders one camera of a group at a time, unrotated: the rotation measured
// the same there but read 3.6 GB more per 27-camera step (render_fwd 4.25
// vs 2.56 GB, render_bwd 7.13 vs 5.19; profiles/r04q/).  The last U % 8
// units keep plain order.
__device__ inline void strip_of_block(int bid, int C, int num_tiles, int& cam, int& item) {
  const int U = C * num_tiles, full = U & ~7;
  int u, s;
  if (bid < 4 * full) {
    const int x = bid & 7, q = bid >> 3, k = q >> 2;
    s = q & 3;
    u = k * 8 + ((x + (C < CAM_GROUP ? k : 0)) & 7);
  } else {
    const int r = bid - 4 * full;
    u = full + (r >> 2);
    s = r & 3;
  }
  int tslot;
  cam_slot(u, C, num_tiles, cam, tslot);
  item = tslot * 4 + s;
}
template <class A>
__device__ inline int num_tiles_of(const A& a) { return a.num_tiles; }

// Dispatch record of slot `i`: {tile, range.x, range.y, 0}.  The plan's
// order puts the longest tile lists first (tile_order_kernel), so the
// long-running workgroups start early and short ones fill the end of the
// launch instead of a few long ones trailing; the record carries the tile's
// list range too, so a workgroup starts with one 16-B load instead of two
// dependent ones.
__device__ inline uint4 tile_rec(const uint4* __restrict__ order, int i) { return order[i]; }

// Gather the fields of list entry i's record the blend kernels use.  The index is clamped
// to the last entry of the (non-empty) range, so the loads are unconditional:
// lanes past the end re-read a valid record and are masked out by the caller.
// (A conditional update of a register struct made the compiler keep it in
// scratch memory.)
struct RecRegs {
  float4 q0, q1;
  float2 q2;  // b, depth
  float tq;   // cull threshold
  uint32_t gid;
};
__device__ inline uint32_t load_gid(const uint32_t* __restrict__ point_list, uint32_t i, uint32_t last_valid) {
  return point_list[i < last_valid ? i : last_valid];
}
__device__ inline RecRegs load_rec_gid(const float* __restrict__ rec, uint32_t gid) {
  RecRegs r;
  r.gid = gid;
  const float4* p = reinterpret_cast<const float4*>(rec + (size_t)gid * REC);
  r.q0 = p[0];  // x, y, conic a, conic b
  r.q1 = p[1];  // conic c, opacity, r, g
  r.q2 = reinterpret_cast<const float2*>(p)[4];  // b, depth (R_EX, R_EY, R_RAD unused)
  r.tq = reinterpret_cast<const float*>(p)[R_TQ];
  return r;
}
__device__ inline RecRegs load_rec(const uint32_t* __restrict__ point_list, const float* __restrict__ rec,
                                   uint32_t i, uint32_t last_valid) {
  return load_rec_gid(rec, load_gid(point_list, i, last_valid));
}

// Gaussian exponent at pixel offset (dx, dy) from the conic scaled once per
// record: h = (-a/2, -b, -c/2).  power = -1/2 (a dx^2 + c dy^2) - b dx dy
// (CR/forward.cu:353-355) in a fixed fma order shared by the forward and the
// backward kernel, so both make bit-identical alpha decisions.
// The exponent is carried in base 2: the half conic is scaled by log2(e) once
// per record, so alpha = opacity * 2^power' costs one v_exp_f32 and no
// multiply per pixel.
constexpr float HC_SCALE = 1.4426950408889634f;
__device__ inline float gauss_exp(float p) { return __builtin_amdgcn_exp2f(p); }
__device__ inline float4 half_conic(const float4& q0, const float4& q1) {
  return make_float4((-0.5f * HC_SCALE) * q0.z, -HC_SCALE * q0.w, (-0.5f * HC_SCALE) * q1.x, 0.0f);
}
__device__ inline float gauss_power(float dx, float dy, const float4& h) {
  return fmaf(h.x * dx, dx, fmaf(h.z * dy, dy, (h.y * dx) * dy));
}

// Can the Gaussian reach alpha >= 1/255 at any pixel centre of the strip
// [sx0, sx1] x [sy0, sy1]?  rect_culled (gs_common.h) on the record's mean,
// conic and threshold tq: exact up to tq's margin, so it culls the Gaussians
// whose bounding box touches the strip but whose ellipse does not.
__device__ inline bool strip_culled(const RecRegs& q, float sx0, float sx1, float sy0, float sy1) {
  return rect_culled(q.q0.x, q.q0.y, q.q0.z, q.q0.w, q.q1.x, q.tq, sx0, sx1, sy0, sy1);
}

}  // namespace gs
