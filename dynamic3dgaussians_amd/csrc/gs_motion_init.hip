// gs_motion_init.hip -- the motion-basis initialisation, forward only (C ABI,
// semantics and byte models: include/gs_motion_init.h): Lloyd's k-means on
// velocity directions or features (motion_utils.py:219-244, 122-162), the
// coefficients 10 exp(-|mean - centre|) (dyn_som.py:64-65) and the weighted
// Procrustes solve per (basis, frame) with its walk over the frames
// (dyn_som.py:76-130).
//
// No floating-point atomic anywhere: every sum has a fixed order, so two calls
// give the same bits.  The only atomic is the 64-bit integer add of a
// workgroup's count of moved labels.
//
// Assign: a thread owns a point and keeps one fp32 accumulator per centre in
// registers (KP = K rounded up to 8, 16, 32 or 64).  Both the workgroup's 256
// points and the centres pass through LDS in chunks of 32 dimensions: the
// global reads of x are 128-byte row segments, the point's own row of the
// tile is read with a stride of 33 words (no bank conflict) and a centre's
// value is one address for the whole wave (a broadcast).  The distance is the
// difference form sum (x - c)^2 added in index order: unit velocity
// directions sit close together and the expanded form would cancel.
//
// Update: two stages.  A workgroup of one wave owns a contiguous slice of
// points and a chunk of 64 dimensions; lane d walks the slice's points in
// order and adds x[p][d] into its own fp64 LDS column of the point's cluster,
// so no two lanes ever add to one word.  The second kernel adds the blocks'
// partial sums in index order, divides in fp64 and rounds to fp32 once.
//
// Procrustes: a workgroup per (basis, chunk of 8 frames) adds the 19 moments
// of its basis's points (32 point lanes per frame, each in its own fixed
// order, then a fixed tree); a thread per basis then walks the frames and
// solves each from its moments (gs_motion_init_solve.h); a third launch, of
// the first one's geometry, adds the residuals of the solved transforms.
//
// The file is compiled without FMA contraction: the squared differences of
// the assign kernel round as written, as the PyTorch restatement's do.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_motion_init.h"
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_motion_init_layout.h"
#include "gs_motion_init_solve.h"

using namespace gs;

namespace {

constexpr int MI_WAVES = MI_THREADS / 64;
constexpr int MI_XS_STRIDE = MI_ASSIGN_DC + 1;  // words per point row of the x tile: odd, so lanes hit distinct banks

template <int KP>
__global__ __launch_bounds__(MI_THREADS) void km_assign_kernel(int64_t N, int D, int K, const float* __restrict__ x,
                                                               const float* __restrict__ centers,
                                                               const uint8_t* __restrict__ valid,
                                                               const int64_t* __restrict__ prev,
                                                               int64_t* __restrict__ labels,
                                                               unsigned long long* __restrict__ moved) {
  __shared__ float xs[MI_THREADS * MI_XS_STRIDE];
  __shared__ float cs[MI_ASSIGN_DC][KP];
  __shared__ int red[MI_WAVES];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * MI_THREADS;
  float acc[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) acc[k] = 0.f;

  for (int d0 = 0; d0 < D; d0 += MI_ASSIGN_DC) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll 4
    for (int j = 0; j < MI_ASSIGN_DC; ++j) {
      const int idx = j * MI_THREADS + tid;
      const int r = idx / MI_ASSIGN_DC, c = idx % MI_ASSIGN_DC;
      const int64_t p = p0 + r;
      const int d = d0 + c;
      xs[r * MI_XS_STRIDE + c] = (p < N && d < D) ? x[p * D + d] : 0.f;
    }
    for (int idx = tid; idx < MI_ASSIGN_DC * KP; idx += MI_THREADS) {
      const int k = idx / MI_ASSIGN_DC, c = idx % MI_ASSIGN_DC;
      const int d = d0 + c;
      cs[c][k] = (k < K && d < D) ? centers[(int64_t)k * D + d] : 0.f;
    }
    __syncthreads();
    const int cmax = D - d0 < MI_ASSIGN_DC ? D - d0 : MI_ASSIGN_DC;
    const float* row = xs + tid * MI_XS_STRIDE;
    for (int c = 0; c < cmax; ++c) {
      const float xv = row[c];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const float df = xv - cs[c][k];
        acc[k] += df * df;
      }
    }
  }

  const int64_t p = p0 + tid;
  int changed = 0;
  if (p < N) {
    float best = acc[0];
    int arg = 0;
#pragma unroll
    for (int k = 1; k < KP; ++k) {
      const bool take = k < K && acc[k] < best;  // strictly: ties stay with the lowest k
      best = take ? acc[k] : best;
      arg = take ? k : arg;
    }
    const int64_t label = (valid && !valid[p]) ? -1 : (int64_t)arg;
    if (prev) changed = prev[p] != label ? 1 : 0;
    labels[p] = label;
  }
  if (moved) {
    changed = wave_sum(changed);
    if ((tid & 63) == 0) red[tid >> 6] = changed;
    __syncthreads();
    if (tid == 0) {
      int total = 0;
#pragma unroll
      for (int w = 0; w < MI_WAVES; ++w) total += red[w];
      if (total) atomicAdd(moved, (unsigned long long)total);
    }
  }
}

__global__ __launch_bounds__(MI_UPDATE_DC) void km_partial_kernel(int64_t N, int D, int K, int64_t slice,
                                                                  const float* __restrict__ x,
                                                                  const int64_t* __restrict__ labels,
                                                                  double* __restrict__ partial,
                                                                  int64_t* __restrict__ pcount) {
  __shared__ double acc[MI_MAX_K][MI_UPDATE_DC];
  __shared__ long long cnt[MI_MAX_K];
  const int lane = threadIdx.x;
  const int d = blockIdx.y * MI_UPDATE_DC + lane;
  const bool live = d < D;
  const bool counts = blockIdx.y == 0 && lane == 0;
  for (int k = 0; k < K; ++k) acc[k][lane] = 0.0;
  if (lane < K) cnt[lane] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * slice;
  const int64_t hi = lo + slice < N ? lo + slice : N;
  auto add = [&](int64_t l, float v) {
    if ((uint64_t)l < (uint64_t)K) {  // labels outside [0, K) are ignored
      if (live) acc[l][lane] += (double)v;
      if (counts) cnt[l] += 1;
    }
  };
  int64_t p = lo;
  constexpr int U = 16;  // loads in flight per lane; the walk itself is bound by the LDS read-modify-write chain
  for (; p + U <= hi; p += U) {  // added in the points' order
    int64_t l[U];
    float v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      l[i] = labels[p + i];
      v[i] = live ? x[(p + i) * D + d] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < U; ++i) add(l[i], v[i]);
  }
  for (; p < hi; ++p) add(labels[p], live ? x[p * D + d] : 0.f);
  __syncthreads();
  if (live)
    for (int k = 0; k < K; ++k) partial[((int64_t)blockIdx.x * K + k) * D + d] = acc[k][lane];
  if (blockIdx.y == 0 && lane < K) pcount[(int64_t)blockIdx.x * K + lane] = cnt[lane];
}

// centers[k][d] = sum over the blocks, in index order, / count; an empty cluster's row is left alone.
__global__ __launch_bounds__(MI_THREADS) void km_reduce_kernel(int64_t blocks, int D, int K,
                                                               const double* __restrict__ partial,
                                                               const int64_t* __restrict__ pcount,
                                                               float* __restrict__ centers,
                                                               int64_t* __restrict__ counts) {
  const int64_t idx = (int64_t)blockIdx.x * MI_THREADS + threadIdx.x;
  if (idx >= (int64_t)K * D) return;
  const int k = (int)(idx / D), d = (int)(idx % D);
  double s = 0.0;
  int64_t c = 0;
  for (int64_t b = 0; b < blocks; ++b) {
    s += partial[(b * K + k) * D + d];
    c += pcount[b * K + k];
  }
  if (c > 0) centers[idx] = (float)(s / (double)c);
  if (d == 0) counts[k] = c;
}

__global__ __launch_bounds__(MI_THREADS) void mi_coefs_kernel(int64_t N, int K, const float* __restrict__ means,
                                                              const float* __restrict__ centers,
                                                              float* __restrict__ coefs) {
  const int64_t i = (int64_t)blockIdx.x * MI_THREADS + threadIdx.x;
  if (i >= N) return;
  const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2];
  float* o = coefs + i * K;
  for (int k = 0; k < K; ++k) {
    const float dx = mx - centers[3 * k], dy = my - centers[3 * k + 1], dz = mz - centers[3 * k + 2];
    o[k] = 10.f * expf(-sqrtf(dx * dx + dy * dy + dz * dz));
  }
}

__device__ inline int64_t clamp_offset(int64_t v, int64_t N) { return v < 0 ? 0 : (v > N ? N : v); }

__global__ __launch_bounds__(MI_THREADS) void mi_moments_kernel(int64_t N, int T, int cano_t,
                                                                const float* __restrict__ tracks,
                                                                const int64_t* __restrict__ order,
                                                                const int64_t* __restrict__ offsets,
                                                                const float* __restrict__ weights,
                                                                const float* __restrict__ conf,
                                                                double* __restrict__ moments) {
  __shared__ double red[MI_THREADS];
  const int tid = threadIdx.x;
  const int f = tid % MI_FRAMES, pl = tid / MI_FRAMES;
  const int k = blockIdx.x;
  const int t = blockIdx.y * MI_FRAMES + f;
  const bool live = t < T;
  const int64_t lo = clamp_offset(offsets[k], N);
  int64_t hi = clamp_offset(offsets[k + 1], N);
  if (hi < lo) hi = lo;
  double m[MI_MOMENTS];
#pragma unroll
  for (int v = 0; v < MI_MOMENTS; ++v) m[v] = 0.0;
  if (live) {
    for (int64_t j = lo + pl; j < hi; j += MI_POINT_LANES) {
      const int64_t id = order[j];
      if ((uint64_t)id >= (uint64_t)N) continue;  // never an address outside tracks
      const int64_t row = id * T;
      double w = 1.0;
      if (weights) w = (double)weights[row + cano_t] * (double)weights[row + t];
      if (conf) w = w * ((double)conf[row + cano_t] + (double)conf[row + t]) * 0.5;
      const float* sp = tracks + (row + cano_t) * 3;
      const float* gp = tracks + (row + t) * 3;
      const float sf[3] = {sp[0], sp[1], sp[2]}, gf[3] = {gp[0], gp[1], gp[2]};
      double s[3], g[3], dd = 0.0, ss = 0.0, gg = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        s[a] = (double)sf[a];
        g[a] = (double)gf[a];
        const double df = s[a] - g[a];
        dd += df * df;
        ss += s[a] * s[a];
        gg += g[a] * g[a];
      }
      m[MI_W] += w;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        m[MI_S + a] += w * s[a];
        m[MI_G + a] += w * g[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) m[MI_SG + 3 * a + b] += w * s[a] * g[b];
      }
      m[MI_SS] += w * ss;
      m[MI_GG] += w * gg;
      m[MI_DD] += w * dd;
    }
  }
  double* out = moments + ((int64_t)k * T + (live ? t : 0)) * MI_MOMENTS;
#pragma unroll
  for (int v = 0; v < MI_MOMENTS; ++v) {
    red[tid] = m[v];
    __syncthreads();
#pragma unroll
    for (int s = MI_POINT_LANES / 2; s > 0; s >>= 1) {
      if (pl < s) red[tid] += red[tid + s * MI_FRAMES];
      __syncthreads();
    }
    if (pl == 0 && live) out[v] = red[tid];
    __syncthreads();
  }
}

struct SolveArgs {
  int T, K, cano_t, rot_dim;
  double min_weight_sum;
  const double* moments;
  double* poses;
  float* rots;
  float* transls;
  float* err_after;
  float* err_before;
  uint8_t* skipped;
};

__global__ __launch_bounds__(64) void mi_solve_kernel(SolveArgs a) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= a.K) return;
  // the state of the frame visited before: everything starts at the identity
  double q[4] = {1.0, 0.0, 0.0, 0.0}, c0[3] = {1.0, 0.0, 0.0}, c1[3] = {0.0, 1.0, 0.0}, tr[3] = {0.0, 0.0, 0.0};
  for (int step = 0; step < a.T; ++step) {
    const int t = step < a.cano_t ? a.cano_t - 1 - step : step;  // cano_t - 1 .. 0, cano_t .. T - 1
    const int64_t kt = (int64_t)k * a.T + t;
    const double* m = a.moments + kt * MI_MOMENTS;
    double mm[MI_MOMENTS];
#pragma unroll
    for (int v = 0; v < MI_MOMENTS; ++v) mm[v] = m[v];
    const bool skip = !(mm[MI_W] >= a.min_weight_sum) || !(mm[MI_W] > 0.0);
    float ea = -1.f, eb = -1.f;
    if (!skip) {
      ProcrustesSolution s;
      mi_procrustes_solve(mm, s);
      const double dot = s.q[0] * q[0] + s.q[1] * q[1] + s.q[2] * q[2] + s.q[3] * q[3];
      const double sign = dot < 0.0 ? -1.0 : 1.0;  // the double cover: the sign nearer to the frame before
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = sign * s.q[r];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        c0[r] = s.R[r][0];
        c1[r] = s.R[r][1];
        tr[r] = s.t[r];
      }
      ea = (float)s.err_after;  // from the moments; mi_residual_kernel replaces it by the direct sum
      eb = (float)s.err_before;
      double* pose = a.poses + kt * MI_POSE;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pose[3 * r + c] = s.R[r][c];
        pose[9 + r] = s.t[r];
      }
    }
    if (a.rot_dim == 4) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a.rots[kt * 4 + r] = (float)q[r];
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        a.rots[kt * 6 + r] = (float)c0[r];
        a.rots[kt * 6 + 3 + r] = (float)c1[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) a.transls[kt * 3 + r] = (float)tr[r];
    a.err_after[kt] = ea;
    a.err_before[kt] = eb;
    a.skipped[kt] = skip ? 1 : 0;
  }
}

// err_after of every solved (basis, frame) as the direct sum of w |R s + t - g|^2: the expansion
// in the moments cancels where the residual is (near) zero, and the square root magnifies that.
// Same geometry and order as mi_moments_kernel.
__global__ __launch_bounds__(MI_THREADS) void mi_residual_kernel(int64_t N, int T, int cano_t,
                                                                 const float* __restrict__ tracks,
                                                                 const int64_t* __restrict__ order,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const float* __restrict__ weights,
                                                                 const float* __restrict__ conf,
                                                                 const double* __restrict__ moments,
                                                                 const double* __restrict__ poses,
                                                                 const uint8_t* __restrict__ skipped,
                                                                 float* __restrict__ err_after) {
  __shared__ double red[MI_THREADS];
  const int tid = threadIdx.x;
  const int f = tid % MI_FRAMES, pl = tid / MI_FRAMES;
  const int k = blockIdx.x;
  const int t = blockIdx.y * MI_FRAMES + f;
  const int64_t kt = (int64_t)k * T + (t < T ? t : 0);
  const bool live = t < T && !skipped[kt];
  const int64_t lo = clamp_offset(offsets[k], N);
  int64_t hi = clamp_offset(offsets[k + 1], N);
  if (hi < lo) hi = lo;
  double sum = 0.0;
  if (live) {
    double P[MI_POSE];
#pragma unroll
    for (int v = 0; v < MI_POSE; ++v) P[v] = poses[kt * MI_POSE + v];
    for (int64_t j = lo + pl; j < hi; j += MI_POINT_LANES) {
      const int64_t id = order[j];
      if ((uint64_t)id >= (uint64_t)N) continue;
      const int64_t row = id * T;
      double w = 1.0;
      if (weights) w = (double)weights[row + cano_t] * (double)weights[row + t];
      if (conf) w = w * ((double)conf[row + cano_t] + (double)conf[row + t]) * 0.5;
      const float* sp = tracks + (row + cano_t) * 3;
      const float* gp = tracks + (row + t) * 3;
      const double s0 = sp[0], s1 = sp[1], s2 = sp[2];
      double r2 = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double d = P[3 * a] * s0 + P[3 * a + 1] * s1 + P[3 * a + 2] * s2 + P[9 + a] - (double)gp[a];
        r2 += d * d;
      }
      sum += w * r2;
    }
  }
  red[tid] = sum;
  __syncthreads();
#pragma unroll
  for (int s = MI_POINT_LANES / 2; s > 0; s >>= 1) {
    if (pl < s) red[tid] += red[tid + s * MI_FRAMES];
    __syncthreads();
  }
  if (pl == 0 && live) err_after[kt] = (float)sqrt(red[tid] / moments[kt * MI_MOMENTS + MI_W]);
}

template <int KP>
void launch_assign(const struct gs_kmeans_assign& a, hipStream_t s) {
  hipLaunchKernelGGL(km_assign_kernel<KP>, dim3((unsigned)mi_blocks(a.N)), dim3(MI_THREADS), 0, s, a.N, a.D, a.K, a.x,
                     a.centers, a.valid, a.prev_labels, a.labels, reinterpret_cast<unsigned long long*>(a.moved));
}

}  // namespace

extern "C" {

int gs_kmeans_assign(const struct gs_kmeans_assign* args, gs_stream_t stream) {
  if (int e = gs_kmeans_assign_validate(args)) return e;
  const struct gs_kmeans_assign& a = *args;
  if (a.N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (a.K <= 8) launch_assign<8>(a, s);
  else if (a.K <= 16) launch_assign<16>(a, s);
  else if (a.K <= 32) launch_assign<32>(a, s);
  else launch_assign<64>(a, s);
  return launch_status("kmeans assign", 0, s);
}

int gs_kmeans_update(const struct gs_kmeans_update* args, gs_stream_t stream) {
  if (int e = gs_kmeans_update_validate(args)) return e;
  const struct gs_kmeans_update& a = *args;
  const KMeansLayout L(a.N, a.K, a.D);
  hipStream_t s = (hipStream_t)stream;
  double* partial = at<double>(a.workspace, L.partial);
  int64_t* pcount = at<int64_t>(a.workspace, L.pcount);
  const unsigned chunks = (unsigned)((a.D + MI_UPDATE_DC - 1) / MI_UPDATE_DC);
  hipLaunchKernelGGL(km_partial_kernel, dim3((unsigned)L.blocks, chunks), dim3(MI_UPDATE_DC), 0, s, a.N, a.D, a.K,
                     L.slice, a.x, a.labels, partial, pcount);
  hipLaunchKernelGGL(km_reduce_kernel, dim3((unsigned)mi_blocks((int64_t)a.K * a.D)), dim3(MI_THREADS), 0, s,
                     L.blocks, a.D, a.K, partial, pcount, a.centers, a.counts);
  return launch_status("kmeans update", 0, s);
}

int gs_coefs_from_centers(const struct gs_coefs_from_centers* args, gs_stream_t stream) {
  if (int e = gs_coefs_from_centers_validate(args)) return e;
  const struct gs_coefs_from_centers& a = *args;
  if (a.N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mi_coefs_kernel, dim3((unsigned)mi_blocks(a.N)), dim3(MI_THREADS), 0, s, a.N, a.K, a.means,
                     a.centers, a.coefs);
  return launch_status("coefs from centers", 0, s);
}

int gs_procrustes(const struct gs_procrustes* args, gs_stream_t stream) {
  if (int e = gs_procrustes_validate(args)) return e;
  const struct gs_procrustes& a = *args;
  const ProcrustesLayout L(a.K, a.T);
  hipStream_t s = (hipStream_t)stream;
  double* moments = at<double>(a.workspace, L.moments);
  const unsigned chunks = (unsigned)((a.T + MI_FRAMES - 1) / MI_FRAMES);
  hipLaunchKernelGGL(mi_moments_kernel, dim3((unsigned)a.K, chunks), dim3(MI_THREADS), 0, s, a.N, a.T, a.cano_t,
                     a.tracks, a.order, a.offsets, a.weights, a.confidences, moments);
  SolveArgs k{};
  k.T = a.T;
  k.K = a.K;
  k.cano_t = a.cano_t;
  k.rot_dim = a.rot_dim;
  k.min_weight_sum = a.min_weight_sum;
  k.moments = moments;
  k.poses = at<double>(a.workspace, L.poses);
  k.rots = a.rots;
  k.transls = a.transls;
  k.err_after = a.err_after;
  k.err_before = a.err_before;
  k.skipped = a.skipped;
  hipLaunchKernelGGL(mi_solve_kernel, dim3((unsigned)((a.K + 63) / 64)), dim3(64), 0, s, k);
  hipLaunchKernelGGL(mi_residual_kernel, dim3((unsigned)a.K, chunks), dim3(MI_THREADS), 0, s, a.N, a.T, a.cano_t,
                     a.tracks, a.order, a.offsets, a.weights, a.confidences, moments, k.poses, a.skipped,
                     a.err_after);
  return launch_status("procrustes", 0, s);
}

}  // extern "C"
