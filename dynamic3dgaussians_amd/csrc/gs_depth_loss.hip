// gs_depth_loss.hip -- the masked depth-correlation loss of the reference's
// dynamic training step (dyn_train.py:256-265), forward and backward, for a
// whole camera batch (C ABI: include/gs_depth_loss.h).
//
//   p = 1 / clamp(depth, near, far) over the masked pixels of a camera,
//   loss = 1 - clamp(pearson(p, target), -1, 1).
//
// Both passes stream the planes once.  A workgroup of 256 threads owns chunks
// of DL_CHUNK = 1024 consecutive pixels of one camera (blockIdx.y), chunk
// blockIdx.x and every gridDim.x-th after it (gs_depth_loss_layout.h has the
// workgroup counts); a thread takes four consecutive pixels of a chunk: one
// 16-byte load of the depth, one of the target and one 4-byte load of the mask
// bytes where the camera's planes are aligned and the wave's 256 pixels lie
// inside the plane, scalar loads with bounds checks otherwise (decided per
// wave, so uniform).
//
// Forward: no raw power sums.  A thread centres its values on the first
// masked one and carries {n, mean p, mean g, Sxx, Syy, Sxy}; partial results
// are merged pairwise (Chan et al.: delta = m_b - m_a, S = S_a + S_b +
// delta^2 n_a n_b / n) down the wave (__shfl_down, offsets 32..1), across the
// four waves in order, and one record per workgroup goes to the workspace.
// depth_loss_finish_kernel (one workgroup per camera) merges the camera's
// records in a fixed order and writes the loss and the eight statistics.
// Backward: elementwise over the same decomposition from the statistics and
// the upstream gradient, both read wave-uniformly from device memory.
// No atomics anywhere: the results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_depth_loss.h"
#include "gs_common.h"
#include "gs_depth_loss_layout.h"
#include "gs_launch.h"

using namespace gs;

namespace {

constexpr int DL_WAVES = DL_THREADS / WAVE;
static_assert(DL_VEC == 4 && DL_THREADS % WAVE == 0, "a float4 and a mask word per thread");

struct DepthArgs {
  int64_t HW, chunks;
  const float* depth;
  const float* target;
  const uint8_t* mask;
  int64_t mask_stride;
  float near, far;
  int skip;
};

// Centred moments of a set of (p, g) pairs; the empty set is all zeros.
struct Mom {
  float n, mp, mg, sxx, syy, sxy;
};

// a <- a merged with b.  Empty sides (n = 0, means 0) leave the other side's
// values exactly; equal means add the sums exactly.
__device__ inline void merge(Mom& a, const Mom& b) {
  const float n = a.n + b.n;
  const float f = n > 0.f ? b.n / n : 0.f;
  const float w = a.n * f;  // n_a n_b / n
  const float dp = b.mp - a.mp, dg = b.mg - a.mg;
  a.sxx += b.sxx + dp * dp * w;
  a.syy += b.syy + dg * dg * w;
  a.sxy += b.sxy + dp * dg * w;
  a.mp += dp * f;
  a.mg += dg * f;
  a.n = n;
}

__device__ inline Mom shfl_down_mom(const Mom& a, int o) {
  Mom b;
  b.n = __shfl_down(a.n, o, WAVE);
  b.mp = __shfl_down(a.mp, o, WAVE);
  b.mg = __shfl_down(a.mg, o, WAVE);
  b.sxx = __shfl_down(a.sxx, o, WAVE);
  b.syy = __shfl_down(a.syy, o, WAVE);
  b.sxy = __shfl_down(a.sxy, o, WAVE);
  return b;
}

// The workgroup's merged moments, valid in thread 0: lane 0 of each wave after
// the shuffle tree (lane l takes lane l + o for o = 32 .. 1), then the waves
// in index order.
__device__ inline Mom block_merge(Mom a, float (*red)[DL_REC]) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const Mom b = shfl_down_mom(a, o);
    if ((int)(threadIdx.x & (WAVE - 1)) + o < WAVE) merge(a, b);
  }
  const int tid = threadIdx.x;
  if ((tid & (WAVE - 1)) == 0) {
    float* r = red[tid / WAVE];
    r[0] = a.n; r[1] = a.mp; r[2] = a.mg; r[3] = a.sxx; r[4] = a.syy; r[5] = a.sxy;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < DL_WAVES; ++w) merge(a, Mom{red[w][0], red[w][1], red[w][2], red[w][3], red[w][4], red[w][5]});
  }
  return a;
}

// The planes of camera blockIdx.y and whether they take the 16-byte path.
struct Planes {
  const float* d;
  const float* g;
  const uint8_t* m;
  bool aligned;
};
__device__ inline Planes planes_of(const DepthArgs& a, const float* extra) {
  const int64_t b = blockIdx.y;
  Planes p;
  p.d = a.depth + b * a.HW;
  p.g = a.target + b * a.HW;
  p.m = a.mask ? a.mask + b * a.mask_stride : nullptr;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p.d) | reinterpret_cast<uintptr_t>(p.g) |
                         reinterpret_cast<uintptr_t>(extra);
  p.aligned = (bits & 15u) == 0 && (reinterpret_cast<uintptr_t>(p.m) & 3u) == 0;
  return p;
}

// The thread's four pixels of chunk c: depth, target and the in-mask flags
// (false past the end of the plane).  Returns whether the wave took the
// 16-byte path (the backward stores the same way).
__device__ inline bool load4(const Planes& pl, int64_t HW, int64_t c, float (&d)[DL_VEC], float (&g)[DL_VEC],
                             bool (&in)[DL_VEC], int64_t& i0) {
  const int tid = threadIdx.x;
  const int64_t wave0 = c * DL_CHUNK + (int64_t)(tid / WAVE) * (WAVE * DL_VEC);
  i0 = c * DL_CHUNK + (int64_t)tid * DL_VEC;
  const bool fast = pl.aligned && wave0 + WAVE * DL_VEC <= HW;  // wave-uniform
  if (fast) {
    const float4 dv = *reinterpret_cast<const float4*>(pl.d + i0);
    const float4 gv = *reinterpret_cast<const float4*>(pl.g + i0);
    const uint32_t mw = pl.m ? *reinterpret_cast<const uint32_t*>(pl.m + i0) : 0x01010101u;
    d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
    g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
#pragma unroll
    for (int j = 0; j < DL_VEC; ++j) in[j] = ((mw >> (8 * j)) & 0xFFu) != 0;
  } else {
#pragma unroll
    for (int j = 0; j < DL_VEC; ++j) {
      const int64_t i = i0 + j;
      d[j] = g[j] = 0.f;
      in[j] = false;
      if (i < HW) {
        d[j] = pl.d[i];
        g[j] = pl.g[i];
        in[j] = pl.m ? pl.m[i] != 0 : true;
      }
    }
  }
  return fast;
}

__device__ inline float inv_clamped(float d, float near, float far) {
  // torch.clamp: min(max(d, near), far) with NaN propagated
  const float c = d != d ? d : fminf(fmaxf(d, near), far);
  return 1.f / c;
}

// The moments of a thread's four pixels, centred on the first masked value:
// equal values give exactly zero sums.
__device__ inline Mom segment_moments(const float (&d)[DL_VEC], const float (&g)[DL_VEC], const bool (&in)[DL_VEC],
                                      float near, float far) {
  float p[DL_VEC], q[DL_VEC], n = 0.f, kp = 0.f, kg = 0.f;
#pragma unroll
  for (int j = 0; j < DL_VEC; ++j) {
    p[j] = inv_clamped(d[j], near, far);
    if (in[j] && n == 0.f) {
      kp = p[j];
      kg = g[j];
    }
    n += in[j] ? 1.f : 0.f;
  }
  float sp = 0.f, sg = 0.f;
#pragma unroll
  for (int j = 0; j < DL_VEC; ++j) {
    p[j] = in[j] ? p[j] - kp : 0.f;
    q[j] = in[j] ? g[j] - kg : 0.f;
    sp += p[j];
    sg += q[j];
  }
  const float rn = n > 0.f ? 1.f / n : 0.f;
  const float op = sp * rn, og = sg * rn;  // the means' offsets from the pivot
  Mom t{n, kp + op, kg + og, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < DL_VEC; ++j) {
    const float ep = in[j] ? p[j] - op : 0.f, eg = in[j] ? q[j] - og : 0.f;
    t.sxx = fmaf(ep, ep, t.sxx);
    t.syy = fmaf(eg, eg, t.syy);
    t.sxy = fmaf(ep, eg, t.sxy);
  }
  return t;
}

__global__ __launch_bounds__(DL_THREADS) void depth_loss_fwd_kernel(DepthArgs a, float* __restrict__ records) {
  __shared__ float red[DL_WAVES][DL_REC];
  const Planes pl = planes_of(a, nullptr);
  Mom acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // one chunk per step (two chunks loaded ahead of their use measured slower:
  // DESIGN.md 9.8)
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    float d[DL_VEC], g[DL_VEC];
    bool in[DL_VEC];
    int64_t i0;
    load4(pl, a.HW, c, d, g, in, i0);
    merge(acc, segment_moments(d, g, in, a.near, a.far));
  }
  acc = block_merge(acc, red);
  if (threadIdx.x == 0) {
    float* r = records + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * DL_REC;
    r[0] = acc.n; r[1] = acc.mp; r[2] = acc.mg; r[3] = acc.sxx; r[4] = acc.syy; r[5] = acc.sxy;
  }
}

// One workgroup per camera: thread t merges records t, t + 256, ... in order,
// then the workgroup tree; thread 0 writes the loss and the statistics.
__global__ __launch_bounds__(DL_THREADS) void depth_loss_finish_kernel(int groups, int skip,
                                                                       const float* __restrict__ records,
                                                                       float* __restrict__ losses,
                                                                       float* __restrict__ stats) {
  __shared__ float red[DL_WAVES][DL_REC];
  const float* rec = records + (int64_t)blockIdx.x * groups * DL_REC;
  Mom acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < groups; i += DL_THREADS) {
    const float* r = rec + (int64_t)i * DL_REC;
    merge(acc, Mom{r[0], r[1], r[2], r[3], r[4], r[5]});
  }
  acc = block_merge(acc, red);
  if (threadIdx.x == 0) {
    const bool finite = isfinite(acc.mp) && isfinite(acc.mg) && isfinite(acc.sxx) && isfinite(acc.syy) &&
                        isfinite(acc.sxy);
    const bool valid = finite && acc.n >= 2.f && acc.sxx > 0.f && acc.syy > 0.f;
    // the product of two fp32 sums can leave the fp32 range: fp64 for this one value
    const float r = valid ? (float)((double)acc.sxy / sqrt((double)acc.sxx * (double)acc.syy)) : nanf("");
    float loss = 1.f - fminf(fmaxf(r, -1.f), 1.f);
    if (!valid) loss = skip ? 0.f : nanf("");
    losses[blockIdx.x] = loss;
    float* s = stats + (int64_t)blockIdx.x * DL_STATS;
    s[0] = acc.n; s[1] = acc.mp; s[2] = acc.mg; s[3] = acc.sxx; s[4] = acc.syy; s[5] = acc.sxy;
    s[6] = r;
    s[7] = valid ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(DL_THREADS) void depth_loss_bwd_kernel(DepthArgs a, const float* __restrict__ stats,
                                                                    const float* __restrict__ dL_dloss,
                                                                    float* __restrict__ d_depth) {
  float* out = d_depth + (int64_t)blockIdx.y * a.HW;
  const Planes pl = planes_of(a, out);
  // the camera's scalars: uniform addresses, scalar loads
  const float* s = stats + (int64_t)blockIdx.y * DL_STATS;
  const float mp = s[1], mg = s[2], sxx = s[3], syy = s[4], sxy = s[5], r = s[6];
  const bool valid = s[7] != 0.f;
  const float up = dL_dloss[blockIdx.y];
  // degenerate camera: zeros (skip) or NaN where a gradient would flow; |r| > 1: clamp(r) is flat
  const bool live = valid ? fabsf(r) <= 1.f : !a.skip;
  const float coef = valid ? up * (1.f / sqrtf(sxx)) * (1.f / sqrtf(syy)) : nanf("");
  const float k = sxy / sxx;
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    float d[DL_VEC], g[DL_VEC], v[DL_VEC];
    bool in[DL_VEC];
    int64_t i0;
    const bool fast = load4(pl, a.HW, c, d, g, in, i0);
#pragma unroll
    for (int j = 0; j < DL_VEC; ++j) {
      const bool open = live && in[j] && d[j] >= a.near && d[j] <= a.far;  // torch's clamp gate, inclusive
      const float p = 1.f / d[j];
      v[j] = open ? coef * ((g[j] - mg) - k * (p - mp)) * (p * p) : 0.f;
    }
    if (fast) {
      *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < DL_VEC; ++j)
        if (i0 + j < a.HW) out[i0 + j] = v[j];
    }
  }
}

DepthArgs kernel_args(const gs_depth_loss& a, const DepthLossLayout& L) {
  DepthArgs k{};
  k.HW = L.plane_elems;
  k.chunks = L.chunks;
  k.depth = a.depth;
  k.target = a.target;
  k.mask = a.mask;
  k.mask_stride = a.mask ? a.mask_batch_stride : 0;
  k.near = a.near;
  k.far = a.far;
  k.skip = a.skip_degenerate != 0;
  return k;
}

}  // namespace

extern "C" {

int gs_depth_loss_forward(const gs_depth_loss* args, gs_stream_t stream) {
  if (int e = gs_depth_loss_validate(args, 0, nullptr, nullptr)) return e;
  const gs_depth_loss& a = *args;
  const DepthLossLayout L(a.B, a.H, a.W);
  const DepthArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  float* records = static_cast<float*>(a.workspace);
  hipLaunchKernelGGL(depth_loss_fwd_kernel, dim3((unsigned)L.groups, (unsigned)a.B), dim3(DL_THREADS), 0, s, k,
                     records);
  hipLaunchKernelGGL(depth_loss_finish_kernel, dim3((unsigned)a.B), dim3(DL_THREADS), 0, s, (int)L.groups, k.skip,
                     records, a.losses, a.stats);
  return launch_status("depth loss forward", 0, s);
}

int gs_depth_loss_backward(const gs_depth_loss* args, const float* dL_dloss, float* dL_ddepth, gs_stream_t stream) {
  if (int e = gs_depth_loss_validate(args, 1, dL_dloss, dL_ddepth)) return e;
  const gs_depth_loss& a = *args;
  const DepthLossLayout L(a.B, a.H, a.W);
  const DepthArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_loss_bwd_kernel, dim3((unsigned)L.groups, (unsigned)a.B), dim3(DL_THREADS), 0, s, k,
                     a.stats, dL_dloss, dL_ddepth);
  return launch_status("depth loss backward", 0, s);
}

}  // extern "C"
