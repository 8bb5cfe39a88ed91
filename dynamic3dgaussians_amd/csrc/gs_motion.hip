// gs_motion.hip -- the motion-basis warp (include/gs_motion.h) for gfx950:
// every Gaussian's mean moved by its own blend of K shared SE(3)
// trajectories, forward and backward.
//
// mt_forward_kernel, one launch: one thread per Gaussian, a workgroup of
// MT_THREADS.  The workgroup stages the [K, B, 9] slice of the tables
// (rots | transls at ts) in LDS once and transposes its coefficient rows into
// LDS columns [K][threads + 4] with coalesced loads (K is a run-time value, so
// the row cannot live in registers without scratch); in mode 1 every thread
// then turns its column into the softmax.  The thread loops over the frames:
// a K x 9 blend from LDS (the basis row is a wave-uniform broadcast read),
// cont_6d_to_rmat, the 3 x 4 transform and / or the position.  A position is
// one 12-byte store per lane, a transform three 16-byte stores where the
// pointer allows (12 scalar stores otherwise).
//
// mt_backward_kernel recomputes the blend and the frame per (g, b), pushes
// dR = d_pos (x) mean + d_T[:, :3] and dt = d_pos + d_T[:, 3] back through
// the cross product and both normalisations to v = (d_r6, dt), and keeps
// d_means in registers and the d_coefs column in LDS across the frame loop.
// The basis gradient sum_g c[g, k] v[g, b, :] is contracted per frame inside
// the workgroup: v goes to LDS columns [9][threads + 4], and output (k, j)
// is summed by one thread over the workgroup's Gaussians in index order,
// 16 bytes of each column per step and four partial sums joined as
// (a0 + a1) + (a2 + a3).  The workgroup's result is its slab [B, K, 9] in the
// workspace.  mt_sum_slabs_kernel adds the slabs per output in a fixed order
// (16 interleaved segments, then the segments in order), and
// mt_scatter_kernel writes every element of d_rots / d_transls: the sum of the
// occurrences of its frame in ts in ascending b, or zero.  No atomics
// anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gs_motion.h"
#include "gs_host_util.h"
#include "gs_launch.h"
#include "gs_motion_layout.h"

namespace gs {

namespace {

constexpr float MT_EPS = 1e-12f;  // F.normalize's clamp

struct MotionK {
  int64_t G;
  int K, T, B, mode;
  const float *rots, *transls, *coefs, *means;
  int ts[MT_MAX_B];
};

struct Frame {  // cont_6d_to_rmat of one blended 6-vector, with what its backward needs
  float x[3], y[3], z[3], y1[3];
  float nx, nu, d;  // the two clamped norms and y1 . x
};

__device__ inline float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ inline void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline void frame_of(const float* r, Frame& f) {
  f.nx = fmaxf(sqrtf(dot3(r, r)), MT_EPS);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f.x[i] = r[i] / f.nx;
    f.y1[i] = r[3 + i];
  }
  f.d = dot3(f.y1, f.x);
  float u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = f.y1[i] - f.d * f.x[i];
  f.nu = fmaxf(sqrtf(dot3(u, u)), MT_EPS);
#pragma unroll
  for (int i = 0; i < 3; ++i) f.y[i] = u[i] / f.nu;
  cross3(f.x, f.y, f.z);
}

// v / max(|v|, eps) backwards: n is the clamped norm, o the output
__device__ inline void normalize_bwd(const float* o, float n, const float* g, float* gv) {
  const float s = n > MT_EPS ? dot3(o, g) : 0.f;  // on the clamp the denominator is a constant
#pragma unroll
  for (int i = 0; i < 3; ++i) gv[i] = (g[i] - o[i] * s) / n;
}

// Gradient of the blended 6-vector for the gradients of the frame's columns.
__device__ inline void frame_bwd(const Frame& f, float* gx, float* gy, const float* gz, float* g6) {
  float t[3];
  cross3(f.y, gz, t);  // z = x cross y
#pragma unroll
  for (int i = 0; i < 3; ++i) gx[i] += t[i];
  cross3(gz, f.x, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) gy[i] += t[i];
  float gu[3];
  normalize_bwd(f.y, f.nu, gy, gu);  // y = u / |u|
  const float xgu = dot3(f.x, gu);   // u = y1 - (y1 . x) x
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g6[3 + i] = gu[i] - f.x[i] * xgu;
    gx[i] -= f.d * gu[i] + xgu * f.y1[i];
  }
  normalize_bwd(f.x, f.nx, gx, g6);  // x = x1 / |x1|
}

// The [K, B, 9] slice of the tables at ts into LDS, by the whole workgroup.
__device__ inline void stage_bases(const MotionK& k, float* sB) {
  const int n = k.K * k.B * MT_ROW;
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const int j = e % MT_ROW, kb = e / MT_ROW, b = kb % k.B, kk = kb / k.B;
    const int64_t row = (int64_t)kk * k.T + k.ts[b];
    sB[e] = j < 6 ? k.rots[row * 6 + j] : k.transls[row * 3 + (j - 6)];
  }
}

// The workgroup's coefficient rows into LDS columns sC[k][local g] (zero past
// the last Gaussian), then the softmax of each thread's own column in mode 1.
// Ends with a barrier: every column is final for every thread.
__device__ inline void stage_coefs(const MotionK& k, int64_t g0, int n, int S, float* sC) {
  const int total = (int)blockDim.x * k.K;
  const float* src = k.coefs + g0 * k.K;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int gl = e / k.K, kk = e - gl * k.K;
    sC[kk * S + gl] = gl < n ? src[e] : 0.f;
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (k.mode == GS_MOTION_COEFS_LOGITS && tid < n) {
    float m = sC[tid];
    for (int kk = 1; kk < k.K; ++kk) m = fmaxf(m, sC[kk * S + tid]);
    float sum = 0.f;
    for (int kk = 0; kk < k.K; ++kk) {
      const float e = expf(sC[kk * S + tid] - m);
      sC[kk * S + tid] = e;
      sum += e;
    }
    for (int kk = 0; kk < k.K; ++kk) sC[kk * S + tid] /= sum;
  }
  __syncthreads();
}

__device__ inline void blend(const float* sC, const float* sB, int K, int B, int S, int b, int tid, float* r) {
#pragma unroll
  for (int j = 0; j < MT_ROW; ++j) r[j] = 0.f;
  for (int kk = 0; kk < K; ++kk) {
    const float c = sC[kk * S + tid];
    const float* row = sB + (kk * B + b) * MT_ROW;
#pragma unroll
    for (int j = 0; j < MT_ROW; ++j) r[j] = fmaf(c, row[j], r[j]);
  }
}

// One (g, b): the frame of the blended row r, its transform and / or position.
__device__ inline void emit(const float* r, const float* m, int64_t gb, float* __restrict__ positions,
                            float* __restrict__ transforms, int tf_vec) {
  Frame f;
  frame_of(r, f);
  if (transforms) {
    float* o = transforms + gb * 12;
    if (tf_vec) {
      float4* o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(f.x[0], f.y[0], f.z[0], r[6]);
      o4[1] = make_float4(f.x[1], f.y[1], f.z[1], r[7]);
      o4[2] = make_float4(f.x[2], f.y[2], f.z[2], r[8]);
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        o[4 * i] = f.x[i];
        o[4 * i + 1] = f.y[i];
        o[4 * i + 2] = f.z[i];
        o[4 * i + 3] = r[6 + i];
      }
    }
  }
  if (positions) {
    float* o = positions + gb * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = f.x[i] * m[0] + f.y[i] * m[1] + f.z[i] * m[2] + r[6 + i];
  }
}

__global__ void __launch_bounds__(MT_THREADS) mt_forward_kernel(const MotionK k, float* __restrict__ positions,
                                                                float* __restrict__ transforms, int tf_vec) {
  extern __shared__ float4 mt_lds[];
  const int S = (int)blockDim.x + MT_PAD, tid = threadIdx.x;
  float* sC = reinterpret_cast<float*>(mt_lds);
  float* sB = sC + (size_t)k.K * S;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x;
  const int n = (int)min((int64_t)blockDim.x, k.G - g0);
  stage_bases(k, sB);
  stage_coefs(k, g0, n, S, sC);
  if (tid >= n) return;
  const int64_t g = g0 + tid;
  float m[3] = {0.f, 0.f, 0.f};
  if (k.means) {
    m[0] = k.means[3 * g];
    m[1] = k.means[3 * g + 1];
    m[2] = k.means[3 * g + 2];
  }
  for (int b = 0; b < k.B; ++b) {
    float r[MT_ROW];
    blend(sC, sB, k.K, k.B, S, b, tid, r);
    emit(r, m, g * k.B + b, positions, transforms, tf_vec);
  }
}

#ifdef GS_MOTION_FWD_PAIR
// Timing-only alternative: one lane per (g, b) pair.  The
// stores of a wave are contiguous, the softmax runs once per Gaussian of the
// workgroup's pair range, and the basis row is no longer wave-uniform.
__global__ void __launch_bounds__(MT_THREADS) mt_forward_pair_kernel(const MotionK k, float* __restrict__ positions,
                                                                     float* __restrict__ transforms, int tf_vec) {
  extern __shared__ float4 mt_lds[];
  const int S = (int)blockDim.x + MT_PAD, tid = threadIdx.x;
  float* sC = reinterpret_cast<float*>(mt_lds);
  float* sB = sC + (size_t)k.K * S;
  const int64_t total = k.G * k.B, p0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t gfirst = p0 / k.B, glast = min(total - 1, p0 + (int64_t)blockDim.x - 1) / k.B;
  stage_bases(k, sB);
  stage_coefs(k, gfirst, (int)(glast - gfirst + 1), S, sC);
  const int64_t p = p0 + tid;
  if (p >= total) return;
  const int64_t g = p / k.B;
  const int b = (int)(p - g * k.B);
  float m[3] = {0.f, 0.f, 0.f};
  if (k.means) {
    m[0] = k.means[3 * g];
    m[1] = k.means[3 * g + 1];
    m[2] = k.means[3 * g + 2];
  }
  float r[MT_ROW];
  blend(sC, sB, k.K, k.B, S, b, (int)(g - gfirst), r);
  emit(r, m, p, positions, transforms, tf_vec);
}
#endif

__global__ void __launch_bounds__(MT_THREADS)
    mt_backward_kernel(const MotionK k, const float* __restrict__ d_positions, const float* __restrict__ d_transforms,
                       int tf_vec, float* __restrict__ d_means, float* __restrict__ d_coefs,
                       float* __restrict__ slabs, float* __restrict__ pairs) {
  extern __shared__ float4 mt_lds[];
  const int S = (int)blockDim.x + MT_PAD, tid = threadIdx.x, nthreads = blockDim.x;
  float* sC = reinterpret_cast<float*>(mt_lds);  // [K][S] coefficients
  float* sD = sC + (size_t)k.K * S;              // [K][S] d_coefs
  float* sV = sD + (size_t)k.K * S;              // [9][S] (d_r6, dt) of the current frame
  float* sB = sV + (size_t)MT_ROW * S;           // [K][B][9]
#ifdef GS_MOTION_STORE_SUM
  sB = sV;  // no contraction in this kernel
#endif
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x;
  const int n = (int)min((int64_t)blockDim.x, k.G - g0);
  const bool valid = tid < n;
  const int64_t g = g0 + tid;
  stage_bases(k, sB);
  for (int kk = 0; kk < k.K; ++kk) sD[kk * S + tid] = 0.f;
  stage_coefs(k, g0, n, S, sC);

  float m[3] = {0.f, 0.f, 0.f}, dm[3] = {0.f, 0.f, 0.f};
  if (valid && k.means) {
    m[0] = k.means[3 * g];
    m[1] = k.means[3 * g + 1];
    m[2] = k.means[3 * g + 2];
  }
#ifndef GS_MOTION_STORE_SUM
  const int outputs = k.K * MT_ROW;
  float* slab = slabs + (size_t)blockIdx.x * k.B * outputs;
#endif

  for (int b = 0; b < k.B; ++b) {
    float v[MT_ROW];
#pragma unroll
    for (int j = 0; j < MT_ROW; ++j) v[j] = 0.f;
    if (valid) {
      float r[MT_ROW];
      blend(sC, sB, k.K, k.B, S, b, tid, r);
      Frame f;
      frame_of(r, f);
      const int64_t gb = g * k.B + b;
      float dp[3] = {0.f, 0.f, 0.f};
      if (d_positions) {
        dp[0] = d_positions[3 * gb];
        dp[1] = d_positions[3 * gb + 1];
        dp[2] = d_positions[3 * gb + 2];
      }
      float gx[3], gy[3], gz[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        gx[i] = dp[i] * m[0];
        gy[i] = dp[i] * m[1];
        gz[i] = dp[i] * m[2];
        v[6 + i] = dp[i];
      }
      if (d_transforms) {
        const float* dT = d_transforms + gb * 12;
        float t[12];
        if (tf_vec) {
          const float4* d4 = reinterpret_cast<const float4*>(dT);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float4 q = d4[i];
            t[4 * i] = q.x;
            t[4 * i + 1] = q.y;
            t[4 * i + 2] = q.z;
            t[4 * i + 3] = q.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 12; ++i) t[i] = dT[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          gx[i] += t[4 * i];
          gy[i] += t[4 * i + 1];
          gz[i] += t[4 * i + 2];
          v[6 + i] += t[4 * i + 3];
        }
      }
      dm[0] += dot3(f.x, dp);  // R^T d_pos
      dm[1] += dot3(f.y, dp);
      dm[2] += dot3(f.z, dp);
      frame_bwd(f, gx, gy, gz, v);
      for (int kk = 0; kk < k.K; ++kk) {
        const float* row = sB + (kk * k.B + b) * MT_ROW;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < MT_ROW; ++j) a = fmaf(row[j], v[j], a);
        sD[kk * S + tid] += a;
      }
    }
#ifdef GS_MOTION_STORE_SUM
    if (valid) {
      float* o = pairs + (g * k.B + b) * MT_ROW;
#pragma unroll
      for (int j = 0; j < MT_ROW; ++j) o[j] = v[j];
    }
#else
    __syncthreads();  // the previous frame's contraction has read sV
#pragma unroll
    for (int j = 0; j < MT_ROW; ++j) sV[j * S + tid] = v[j];
    __syncthreads();
    // slab[b][k][j] = sum over the workgroup's Gaussians of c[g, k] v[g, j], in index order
    for (int o = tid; o < outputs; o += nthreads) {
      const int kk = o / MT_ROW, j = o - kk * MT_ROW;
      const float4* c4 = reinterpret_cast<const float4*>(sC + kk * S);
      const float4* v4 = reinterpret_cast<const float4*>(sV + j * S);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int q = 0; q < nthreads / 4; ++q) {
        const float4 c = c4[q], w = v4[q];
        a0 = fmaf(c.x, w.x, a0);
        a1 = fmaf(c.y, w.y, a1);
        a2 = fmaf(c.z, w.z, a2);
        a3 = fmaf(c.w, w.w, a3);
      }
      slab[(size_t)b * outputs + o] = (a0 + a1) + (a2 + a3);
    }
#endif
  }

  if (valid) {
    if (k.mode == GS_MOTION_COEFS_LOGITS) {  // softmax backwards: c (dc - sum c dc)
      float s = 0.f;
      for (int kk = 0; kk < k.K; ++kk) s = fmaf(sC[kk * S + tid], sD[kk * S + tid], s);
      for (int kk = 0; kk < k.K; ++kk) sD[kk * S + tid] = sC[kk * S + tid] * (sD[kk * S + tid] - s);
    }
    if (d_means) {
      d_means[3 * g] = dm[0];
      d_means[3 * g + 1] = dm[1];
      d_means[3 * g + 2] = dm[2];
    }
  }
  __syncthreads();
  const int total = n * k.K;  // the workgroup's d_coefs rows, contiguous
  float* dst = d_coefs + g0 * k.K;
  for (int e = tid; e < total; e += nthreads) {
    const int gl = e / k.K, kk = e - gl * k.K;
    dst[e] = sD[kk * S + gl];
  }
}

#ifdef GS_MOTION_STORE_SUM
// The backward kernel's per-frame contraction, as a function of this pass.
__device__ inline void contract_frame(const float* sC, const float* sV, int S, int K, float* __restrict__ out) {
  const int nthreads = blockDim.x, outputs = K * MT_ROW;
  for (int o = threadIdx.x; o < outputs; o += nthreads) {
    const int kk = o / MT_ROW, j = o - kk * MT_ROW;
    const float4* c4 = reinterpret_cast<const float4*>(sC + kk * S);
    const float4* v4 = reinterpret_cast<const float4*>(sV + j * S);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int q = 0; q < nthreads / 4; ++q) {
      const float4 c = c4[q], w = v4[q];
      a0 = fmaf(c.x, w.x, a0);
      a1 = fmaf(c.y, w.y, a1);
      a2 = fmaf(c.z, w.z, a2);
      a3 = fmaf(c.w, w.w, a3);
    }
    out[o] = (a0 + a1) + (a2 + a3);
  }
}

// Timing-only alternative: the backward stores every (g, b)
// row of (d_r6, dt); this pass reads them back and contracts them with the
// coefficients into the same slabs.
__global__ void __launch_bounds__(MT_THREADS)
    mt_contract_kernel(const MotionK k, const float* __restrict__ pairs, float* __restrict__ slabs) {
  extern __shared__ float4 mt_lds[];
  const int S = (int)blockDim.x + MT_PAD, tid = threadIdx.x;
  float* sC = reinterpret_cast<float*>(mt_lds);
  float* sV = sC + (size_t)k.K * S;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x;
  const int n = (int)min((int64_t)blockDim.x, k.G - g0);
  stage_coefs(k, g0, n, S, sC);
  const int outputs = k.K * MT_ROW;
  float* slab = slabs + (size_t)blockIdx.x * k.B * outputs;
  for (int b = 0; b < k.B; ++b) {
    __syncthreads();
    const float* src = pairs + ((g0 + tid) * k.B + b) * MT_ROW;
#pragma unroll
    for (int j = 0; j < MT_ROW; ++j) sV[j * S + tid] = tid < n ? src[j] : 0.f;
    __syncthreads();
    contract_frame(sC, sV, S, k.K, slab + (size_t)b * outputs);
  }
}
#endif

// sum[o] = the slabs' o-th element added up: segment s takes slabs s, s + 16,
// ... in order, then the 16 segments are added in order.
__global__ void __launch_bounds__(MT_SUM_LANES* MT_SUM_SEGMENTS)
    mt_sum_slabs_kernel(const float* __restrict__ slabs, int64_t blocks, int outputs, float* __restrict__ sum) {
  __shared__ float part[MT_SUM_SEGMENTS][MT_SUM_LANES];
  const int lane = threadIdx.x % MT_SUM_LANES, seg = threadIdx.x / MT_SUM_LANES;
  const int o = blockIdx.x * MT_SUM_LANES + lane;
  float a = 0.f;
  if (o < outputs) {
#pragma unroll 4
    for (int64_t s = seg; s < blocks; s += MT_SUM_SEGMENTS) a += slabs[s * outputs + o];
  }
  part[seg][lane] = a;
  __syncthreads();
  if (seg == 0 && o < outputs) {
    float t = part[0][lane];
#pragma unroll
    for (int s = 1; s < MT_SUM_SEGMENTS; ++s) t += part[s][lane];
    sum[o] = t;
  }
}

// Every element of d_rots [K, T, 6] and d_transls [K, T, 3]: its frame's
// occurrences in ts added in ascending b, zero without one (or without a sum).
__global__ void __launch_bounds__(MT_THREADS)
    mt_scatter_kernel(const MotionK k, const float* __restrict__ sum, float* __restrict__ d_rots,
                      float* __restrict__ d_transls) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)k.K * k.T * MT_ROW) return;
  const int j = (int)(e % MT_ROW);
  const int64_t row = e / MT_ROW;  // kk * T + t
  const int t = (int)(row % k.T), kk = (int)(row / k.T);
  float a = 0.f;
  if (sum) {
    for (int b = 0; b < k.B; ++b)
      if (k.ts[b] == t) a += sum[((size_t)b * k.K + kk) * MT_ROW + j];
  }
  if (j < 6)
    d_rots[row * 6 + j] = a;
  else
    d_transls[row * 3 + (j - 6)] = a;
}

MotionK kernel_args(const gs_motion_desc& d) {
  MotionK k{};
  k.G = d.G;
  k.K = d.K;
  k.T = d.T;
  k.B = d.B;
  k.mode = d.coef_mode;
  k.rots = d.rots;
  k.transls = d.transls;
  k.coefs = d.coefs;
  k.means = d.means;
  for (int b = 0; b < d.B; ++b) k.ts[b] = d.ts[b];
  return k;
}

// A workgroup may use more LDS than the default limit of a launch.
template <typename F>
int allow_lds(F kernel, size_t bytes, const char* what) {
  if (bytes <= 48 * 1024) return 0;
  const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return e == hipSuccess ? 0 : gs_set_error((int)e, "%s: %zu bytes of LDS: %s", what, bytes, hipGetErrorString(e));
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" {

int gs_motion_forward(const gs_motion_desc* desc, float* positions, float* transforms, void* workspace,
                      gs_stream_t stream) {
  if (int e = gs_motion_forward_validate(desc, positions, transforms, workspace)) return e;
  const gs_motion_desc& d = *desc;
  if (d.G == 0) return 0;
  const int64_t blocks = (d.G + MT_THREADS - 1) / MT_THREADS;
  if (blocks > 0x7FFFFFFF) return gs_set_error(-1, "motion forward: too many workgroups (%lld)", (long long)blocks);
  const size_t lds = mt_lds_bytes(d.K, d.B, MT_THREADS, false);
  if (int e = allow_lds(mt_forward_kernel, lds, "motion forward")) return e;
#ifdef GS_MOTION_FWD_PAIR
  const int64_t pair_blocks = (d.G * d.B + MT_THREADS - 1) / MT_THREADS;
  if (pair_blocks > 0x7FFFFFFF) return gs_set_error(-1, "motion forward: too many workgroups");
  if (int e = allow_lds(mt_forward_pair_kernel, lds, "motion forward")) return e;
  hipLaunchKernelGGL(mt_forward_pair_kernel, dim3((unsigned)pair_blocks), dim3(MT_THREADS), lds, (hipStream_t)stream,
                     kernel_args(d), positions, transforms, aligned16(transforms) ? 1 : 0);
#else
  hipLaunchKernelGGL(mt_forward_kernel, dim3((unsigned)blocks), dim3(MT_THREADS), lds, (hipStream_t)stream,
                     kernel_args(d), positions, transforms, aligned16(transforms) ? 1 : 0);
#endif
  return launch_status("motion forward", 0, (hipStream_t)stream);
}

int gs_motion_backward(const gs_motion_desc* desc, const float* d_positions, const float* d_transforms,
                       float* d_means, float* d_coefs, float* d_rots, float* d_transls, void* workspace,
                       gs_stream_t stream) {
  if (int e = gs_motion_backward_validate(desc, d_positions, d_transforms, d_means, d_coefs, d_rots, d_transls,
                                          workspace))
    return e;
  const gs_motion_desc& d = *desc;
  hipStream_t s = (hipStream_t)stream;
  const MotionK k = kernel_args(d);
  const int64_t elems = (int64_t)d.K * d.T * MT_ROW;
  const int64_t scatter_blocks = (elems + MT_THREADS - 1) / MT_THREADS;
  if (scatter_blocks > 0x7FFFFFFF) return gs_set_error(-1, "motion backward: tables of %d x %d are too large", d.K, d.T);
  const float* sum = nullptr;
  if (d.G > 0) {
    const MotionLayout L(d.G, d.K, d.B);
    if (L.blocks > 0x7FFFFFFF)
      return gs_set_error(-1, "motion backward: too many workgroups (%lld)", (long long)L.blocks);
    const int threads = mt_backward_threads(d.K, d.B);
    const size_t lds = mt_lds_bytes(d.K, d.B, threads, true);
    if (int e = allow_lds(mt_backward_kernel, lds, "motion backward")) return e;
    char* ws = static_cast<char*>(workspace);
    float* slabs = reinterpret_cast<float*>(ws + L.slabs);
    float* total = reinterpret_cast<float*>(ws + L.sum);
    float* pairs = nullptr;
#ifdef GS_MOTION_STORE_SUM
    pairs = reinterpret_cast<float*>(ws + L.pairs);
#endif
    hipLaunchKernelGGL(mt_backward_kernel, dim3((unsigned)L.blocks), dim3(threads), lds, s, k, d_positions,
                       d_transforms, aligned16(d_transforms) ? 1 : 0, d_means, d_coefs, slabs, pairs);
#ifdef GS_MOTION_STORE_SUM
    const size_t lds2 = (size_t)(d.K + MT_ROW) * (threads + MT_PAD) * sizeof(float);
    if (int e = allow_lds(mt_contract_kernel, lds2, "motion backward")) return e;
    hipLaunchKernelGGL(mt_contract_kernel, dim3((unsigned)L.blocks), dim3(threads), lds2, s, k, pairs, slabs);
#endif
    const int outputs = (int)L.slab_floats;
    hipLaunchKernelGGL(mt_sum_slabs_kernel, dim3((outputs + MT_SUM_LANES - 1) / MT_SUM_LANES),
                       dim3(MT_SUM_LANES * MT_SUM_SEGMENTS), 0, s, slabs, L.blocks, outputs, total);
    sum = total;
  }
  hipLaunchKernelGGL(mt_scatter_kernel, dim3((unsigned)scatter_blocks), dim3(MT_THREADS), 0, s, k, sum, d_rots,
                     d_transls);
  return launch_status("motion backward", 0, s);
}

}  // extern "C"
