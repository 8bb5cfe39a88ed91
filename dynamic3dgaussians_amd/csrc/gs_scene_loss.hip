// gs_scene_loss.hip -- the scene regularisers of the reference's per-step
// loss (train.py:275-282: floor, bg, soft_col_cons) and the foreground gather
// that feeds its neighbour block (train.py:256-257), forward and backward
// (C ABI: include/gs_scene_loss.h).
//
// The reference splits the tables with boolean indexing; here the split is the
// int32 table slot [P] (rank r >= 0 among the foreground rows, -1 - r among the
// background rows), so a thread reads its own row, knows which set it is in
// and which anchor row belongs to it, and nothing is compacted, counted or read
// back.  A slot outside [0, n_fg) / [0, n_bg) is never dereferenced: such a row
// contributes nothing and gets a zero gradient.
//
// scene_loss_fwd_kernel   grid-stride over the rows, 256 threads; four fp32
//                         partials per thread {floor, bg means, bg rotations,
//                         colour}, wave_sum, the four waves in order, one record
//                         per workgroup in the workspace
// scene_loss_finish_kernel one workgroup: wave w sums quantity w of the records
//                         in double (lane l takes l, l + 64, ... in order, then
//                         wave_sum), divides by n_fg, n_bg, n_bg, P
// scene_loss_bwd_kernel   one thread per row, every gradient element written once
// fg_gather_fwd / _bwd    one thread per row, a copy each way
//
// Rotation rows (16 bytes) move as one float4 where the host found the base
// pointer 16-byte aligned, as four floats otherwise (a parameter that is a view
// into a flat optimizer buffer is only 4-byte aligned).  Compiled without fma
// contraction: act_normalize follows the preprocess kernels' order.
// No atomics anywhere: the results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gs_scene_loss.h"
#include "gs_activate.h"
#include "gs_common.h"
#include "gs_host_util.h"
#include "gs_launch.h"
#include "gs_scene_loss_layout.h"

using namespace gs;

namespace {

constexpr int SL_WAVES = SL_THREADS / WAVE;
static_assert(SL_THREADS % WAVE == 0 && SL_WAVES == SL_REC, "the finisher gives each of its four waves one quantity");

struct SceneArgs {
  int64_t P, n_fg, n_bg;
  const int32_t* slot;
  const float* means;
  const float* rot;
  const float* col;
  const float* a_pts;
  const float* a_rot;
  const float* prev_col;
  int raw;
  int vec_rot, vec_anchor;  // 16-byte loads of rot / a_rot rows (host-checked alignment)
};

__device__ inline float4 ld4(const float* base, int64_t row, int vec) {
  if (vec) return reinterpret_cast<const float4*>(base)[row];
  const float* p = base + 4 * row;
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ inline void st4(float* base, int64_t row, int vec, float4 v) {
  if (vec) {
    reinterpret_cast<float4*>(base)[row] = v;
  } else {
    float* p = base + 4 * row;
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}
// torch's sign: 0 at 0 (and at NaN)
__device__ inline float sgn(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// The background row's rank, or -1 when the slot is foreground or out of range.
__device__ inline int64_t bg_rank(int32_t s, int64_t n_bg) {
  const int64_t r = -1 - (int64_t)s;
  return (s < 0 && r < n_bg) ? r : -1;
}

__global__ __launch_bounds__(SL_THREADS) void scene_loss_fwd_kernel(SceneArgs a, float* __restrict__ records) {
  __shared__ float red[SL_WAVES][SL_REC];
  float fl = 0.f, bm = 0.f, br = 0.f, co = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; i < a.P; i += (int64_t)gridDim.x * SL_THREADS) {
    const int32_t s = a.slot[i];
    const float* m = a.means + 3 * i;
    const int64_t r = bg_rank(s, a.n_bg);
    if (s >= 0 && s < a.n_fg) {
      const float y = m[1];
      fl += y < 0.f ? 0.f : y;  // clamp(min = 0), NaN kept
    } else if (r >= 0) {
      const float* ap = a.a_pts + 3 * r;
      bm += (fabsf(m[0] - ap[0]) + fabsf(m[1] - ap[1])) + fabsf(m[2] - ap[2]);
      float4 q = ld4(a.rot, i, a.vec_rot);
      if (a.raw) q = act_normalize(q);
      const float4 ar = ld4(a.a_rot, r, a.vec_anchor);
      br += ((fabsf(q.x - ar.x) + fabsf(q.y - ar.y)) + fabsf(q.z - ar.z)) + fabsf(q.w - ar.w);
    }
    const float* c = a.col + 3 * i;
    const float* pc = a.prev_col + 3 * i;
    co += (fabsf(c[0] - pc[0]) + fabsf(c[1] - pc[1])) + fabsf(c[2] - pc[2]);
  }
  fl = wave_sum(fl);
  bm = wave_sum(bm);
  br = wave_sum(br);
  co = wave_sum(co);
  const int tid = threadIdx.x;
  if ((tid & (WAVE - 1)) == 0) {
    float* r = red[tid / WAVE];
    r[0] = fl; r[1] = bm; r[2] = br; r[3] = co;
  }
  __syncthreads();
  if (tid < SL_REC) {
    float t = red[0][tid];
#pragma unroll
    for (int w = 1; w < SL_WAVES; ++w) t += red[w][tid];
    records[(int64_t)blockIdx.x * SL_REC + tid] = t;
  }
}

__global__ __launch_bounds__(SL_THREADS) void scene_loss_finish_kernel(int groups, int64_t P, int64_t n_fg,
                                                                       int64_t n_bg,
                                                                       const float* __restrict__ records,
                                                                       float* __restrict__ losses) {
  __shared__ double tot[SL_REC];
  const int w = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  double acc = 0.0;
  for (int b = lane; b < groups; b += WAVE) acc += (double)records[(int64_t)b * SL_REC + w];
  acc = wave_sum(acc);
  if (lane == 0) tot[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    // an empty set: 0 / 0 = NaN, torch's empty mean
    losses[0] = (float)(tot[0] / (double)n_fg);
    losses[1] = (float)(tot[1] / (double)n_bg + tot[2] / (double)n_bg);
    losses[2] = (float)(tot[3] / (double)P);
  }
}

// The share of one row in the gradient of a mean over n rows: torch's device
// kernel divides by a host scalar as a product with its fp32 reciprocal.
__device__ inline float mean_share(float g, int64_t n) { return g * (1.0f / (float)n); }

__global__ __launch_bounds__(SL_THREADS) void scene_loss_bwd_kernel(SceneArgs a, const float* __restrict__ dL,
                                                                    float* __restrict__ d_means,
                                                                    float* __restrict__ d_rot,
                                                                    float* __restrict__ d_col, int vec_out) {
  const int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (i >= a.P) return;
  // the three upstream gradients: uniform addresses, scalar loads
  const float gf = mean_share(dL[0], a.n_fg), gb = mean_share(dL[1], a.n_bg), gc = mean_share(dL[2], a.P);
  const int32_t s = a.slot[i];
  const float* m = a.means + 3 * i;
  const int64_t r = bg_rank(s, a.n_bg);
  float dx = 0.f, dy = 0.f, dz = 0.f;
  float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s >= 0 && s < a.n_fg) {
    dy = m[1] >= 0.f ? gf : 0.f;  // clamp's gate, 0 included
  } else if (r >= 0) {
    const float* ap = a.a_pts + 3 * r;
    dx = gb * sgn(m[0] - ap[0]);
    dy = gb * sgn(m[1] - ap[1]);
    dz = gb * sgn(m[2] - ap[2]);
    const float4 q = ld4(a.rot, i, a.vec_rot);
    const float4 qn = a.raw ? act_normalize(q) : q;
    const float4 ar = ld4(a.a_rot, r, a.vec_anchor);
    dq = make_float4(gb * sgn(qn.x - ar.x), gb * sgn(qn.y - ar.y), gb * sgn(qn.z - ar.z), gb * sgn(qn.w - ar.w));
    if (a.raw) dq = act_normalize_bwd(q, dq);
  }
  float* om = d_means + 3 * i;
  om[0] = dx; om[1] = dy; om[2] = dz;
  st4(d_rot, i, vec_out, dq);
  const float* c = a.col + 3 * i;
  const float* pc = a.prev_col + 3 * i;
  float* oc = d_col + 3 * i;
  oc[0] = gc * sgn(c[0] - pc[0]);
  oc[1] = gc * sgn(c[1] - pc[1]);
  oc[2] = gc * sgn(c[2] - pc[2]);
}

__global__ __launch_bounds__(SL_THREADS) void fg_gather_fwd_kernel(int64_t P, int64_t n_fg,
                                                                   const int32_t* __restrict__ slot,
                                                                   const float* __restrict__ means,
                                                                   const float* __restrict__ rot,
                                                                   float* __restrict__ fg_pts,
                                                                   float* __restrict__ fg_rot, int vec_in,
                                                                   int vec_out) {
  const int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (i >= P) return;
  const int64_t s = slot[i];
  if (s < 0 || s >= n_fg) return;
  const float* m = means + 3 * i;
  float* o = fg_pts + 3 * s;
  o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
  st4(fg_rot, s, vec_out, ld4(rot, i, vec_in));
}

// Either compact input may be null (no gradient reached it: zeros), either
// output may be null (not wanted).
__global__ __launch_bounds__(SL_THREADS) void fg_gather_bwd_kernel(int64_t P, int64_t n_fg,
                                                                   const int32_t* __restrict__ slot,
                                                                   const float* __restrict__ d_fg_pts,
                                                                   const float* __restrict__ d_fg_rot,
                                                                   float* __restrict__ d_means,
                                                                   float* __restrict__ d_rot, int vec_in,
                                                                   int vec_out) {
  const int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (i >= P) return;
  const int64_t s = slot[i];
  const bool fg = s >= 0 && s < n_fg;
  if (d_means) {
    float x = 0.f, y = 0.f, z = 0.f;
    if (fg && d_fg_pts) {
      const float* g = d_fg_pts + 3 * s;
      x = g[0]; y = g[1]; z = g[2];
    }
    float* o = d_means + 3 * i;
    o[0] = x; o[1] = y; o[2] = z;
  }
  if (d_rot) st4(d_rot, i, vec_out, fg && d_fg_rot ? ld4(d_fg_rot, s, vec_in) : make_float4(0.f, 0.f, 0.f, 0.f));
}

SceneArgs kernel_args(const gs_scene_loss& a) {
  SceneArgs k{};
  k.P = a.P;
  k.n_fg = a.n_fg;
  k.n_bg = a.n_bg;
  k.slot = a.slot;
  k.means = a.means;
  k.rot = a.rotations;
  k.col = a.colors;
  k.a_pts = a.init_bg_pts;
  k.a_rot = a.init_bg_rot;
  k.prev_col = a.prev_col;
  k.raw = a.raw_rotations != 0;
  k.vec_rot = aligned16(a.rotations);
  k.vec_anchor = aligned16(a.init_bg_rot);
  return k;
}

unsigned row_groups(int64_t P) { return (unsigned)((P + SL_THREADS - 1) / SL_THREADS); }

}  // namespace

extern "C" {

int gs_scene_loss_forward(const gs_scene_loss* args, gs_stream_t stream) {
  if (int e = gs_scene_loss_validate(args, 0, nullptr, nullptr, nullptr, nullptr)) return e;
  const gs_scene_loss& a = *args;
  const SceneLossLayout L(a.P);
  hipStream_t s = (hipStream_t)stream;
  float* records = static_cast<float*>(a.workspace);
  hipLaunchKernelGGL(scene_loss_fwd_kernel, dim3((unsigned)L.groups), dim3(SL_THREADS), 0, s, kernel_args(a), records);
  hipLaunchKernelGGL(scene_loss_finish_kernel, dim3(1), dim3(SL_THREADS), 0, s, (int)L.groups, a.P, a.n_fg, a.n_bg,
                     records, a.losses);
  return launch_status("scene loss forward", 0, s);
}

int gs_scene_loss_backward(const gs_scene_loss* args, const float* dL_dlosses, float* dL_dmeans, float* dL_drotations,
                           float* dL_dcolors, gs_stream_t stream) {
  if (int e = gs_scene_loss_validate(args, 1, dL_dlosses, dL_dmeans, dL_drotations, dL_dcolors)) return e;
  const gs_scene_loss& a = *args;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(scene_loss_bwd_kernel, dim3(row_groups(a.P)), dim3(SL_THREADS), 0, s, kernel_args(a), dL_dlosses,
                     dL_dmeans, dL_drotations, dL_dcolors, (int)aligned16(dL_drotations));
  return launch_status("scene loss backward", 0, s);
}

int gs_fg_gather_forward(int64_t P, int64_t n_fg, const int32_t* slot, const float* means, const float* rotations,
                         float* fg_pts, float* fg_rot, gs_stream_t stream) {
  if (int e = fg_gather_check("fg gather forward", 0, P, n_fg, slot, means, rotations, fg_pts, fg_rot)) return e;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fg_gather_fwd_kernel, dim3(row_groups(P)), dim3(SL_THREADS), 0, s, P, n_fg, slot, means,
                     rotations, fg_pts, fg_rot, (int)aligned16(rotations), (int)aligned16(fg_rot));
  return launch_status("fg gather forward", 0, s);
}

int gs_fg_gather_backward(int64_t P, int64_t n_fg, const int32_t* slot, const float* dL_dfg_pts,
                          const float* dL_dfg_rot, float* dL_dmeans, float* dL_drotations, gs_stream_t stream) {
  if (int e = fg_gather_check("fg gather backward", 1, P, n_fg, slot, dL_dmeans, dL_drotations, dL_dfg_pts,
                              dL_dfg_rot))
    return e;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fg_gather_bwd_kernel, dim3(row_groups(P)), dim3(SL_THREADS), 0, s, P, n_fg, slot, dL_dfg_pts,
                     dL_dfg_rot, dL_dmeans, dL_drotations, (int)aligned16(dL_dfg_rot), (int)aligned16(dL_drotations));
  return launch_status("fg gather backward", 0, s);
}

}  // extern "C"
