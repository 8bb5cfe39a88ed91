// gs_robust_loss.hip -- the quantile-trimmed squared losses of the reference
// (helpers.py:16-38 masked_mse_loss, ideaII.py:378-384 trimmed_mse_loss) and
// the batched exact quantile under them, forward and backward, for a whole
// batch of planes (C ABI: include/gs_robust_loss.h).
//
// Forward, with a threshold (select != 0):
//   residual   one pass over pred and gt: the fp32 residual plane into the
//              workspace, the count of NaNs, and the histogram of the top 11
//              bits of the residuals' bit patterns (non-negative floats order
//              as their uint32 bits).  The histogram is built in LDS with
//              integer atomics and merged into the plane's global histogram
//              with integer atomics: integer sums do not depend on the order.
//   select<1>  one workgroup per plane walks the histogram: n, the ranks lo
//              and hi and the lerp weight from q, then for each of the two
//              ranks the bin that holds it and the rank that remains inside
//              that bin.  All of it stays on the device.
//   hist<2>, select<2>, hist<3>, select<3>
//              the same for the next 10 and the last 10 bits, re-reading the
//              4-byte residual plane; an element counts for a rank when its
//              upper bits equal that rank's prefix.  Both ranks are carried
//              through the levels (one histogram each; one when the prefixes
//              agree), so v_hi needs no pass of its own.  select<3> holds both
//              order statistics exactly and writes the fp64 threshold.
//   reduce     sum kept m e, the kept count and sum kept m: fp64 in every
//              thread, the wave's lanes by shuffles, the waves in order, one
//              record per workgroup.
//   finish     one thread per plane adds the records in order and writes the
//              loss and the statistics.
// With select = 0 the forward is reduce (from pred and gt) and finish alone.
// Backward: one elementwise launch over pred that recomputes the residual with
// the forward's own function (residual_of), so the kept set is the forward's.
//
// Built with -ffp-contract=off: the residual's sum of squares rounds as
// written, which is how the PyTorch restatement (robust_loss.py) rounds.
// No float atomics anywhere: the results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_robust_loss.h"
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_robust_loss_layout.h"

using namespace gs;

namespace {

constexpr int RL_WAVES = RL_THREADS / WAVE;
constexpr uint32_t INF_BITS = 0x7F800000u;   // keys above it are NaNs (or carry a sign): never in a histogram
constexpr uint32_t OUTSIDE = 0xFFFFFFFFu;    // the plane's value where an element does not take part
// words of a plane's selection state
enum { ST_NAN = 0, ST_DEAD = 1, ST_PREFIX = 2 /* lo, hi */, ST_RANK = 4 /* lo, hi */, ST_SAME = 6, ST_W = 8 /* fp64 */ };

struct RlArgs {
  int64_t N, chunks;
  int R;
  const float* pred;
  const float* gt;
  const uint8_t* mask;
  int64_t mask_stride;
  double q;
  int select, over_masked, normalize, norm_width, skip;
};

// The residual of element i of a plane whose pred and gt start at p and g: R
// squared differences added in index order, divided once.  The forward and the
// backward both call this, so they agree bit for bit.
template <int LAYOUT>
__device__ inline float residual_of(const float* __restrict__ p, const float* __restrict__ g, int64_t i, int64_t N,
                                    int R) {
  if (LAYOUT == GS_ROBUST_VALUES) return p[i] + 0.f;  // -0 becomes +0, whose bits order
  float s = 0.f;
  for (int c = 0; c < R; ++c) {
    const int64_t k = LAYOUT == GS_ROBUST_CHANNELS ? (int64_t)c * N + i : i * R + c;
    const float d = p[k] - g[k];
    s += d * d;
  }
  return s / (float)R;
}

// One count for `bin` from every lane with `valid`.  The lanes that share the
// first valid lane's bin go in as one add of their number (a plane with a long
// run of ties, such as exact zeros, would otherwise serialise on one LDS
// word); the others add one each.  Called by whole waves.
__device__ inline void hist_add(uint32_t* h, uint32_t bin, bool valid) {
  const unsigned long long act = __ballot(valid);
  if (act == 0) return;
  const int leader = __ffsll(act) - 1;
  const uint32_t lb = __shfl(bin, leader, WAVE);
  const bool with_leader = valid && bin == lb;
  const unsigned long long grp = __ballot(with_leader);
  if ((int)(threadIdx.x & (WAVE - 1)) == leader) atomicAdd(&h[lb], (uint32_t)__popcll(grp));
  else if (valid && !with_leader) atomicAdd(&h[bin], 1u);
}

// The workgroup's LDS histogram into the plane's global one: an integer atomic
// per non-empty bin.
__device__ inline void hist_merge(const uint32_t* h, uint32_t* __restrict__ out, int bins) {
  for (int k = threadIdx.x; k < bins; k += RL_THREADS) {
    const uint32_t v = h[k];
    if (v) atomicAdd(&out[k], v);
  }
}

template <int LAYOUT>
__global__ __launch_bounds__(RL_THREADS) void rl_residual_kernel(RlArgs a, uint32_t* __restrict__ state,
                                                                 uint32_t* __restrict__ hist1,
                                                                 float* __restrict__ plane) {
  __shared__ uint32_t h[RL_BINS1];
  const int64_t b = blockIdx.y;
  for (int k = threadIdx.x; k < RL_BINS1; k += RL_THREADS) h[k] = 0;
  __syncthreads();
  const int64_t per = LAYOUT == GS_ROBUST_VALUES ? a.N : a.N * a.R;
  const float* p = a.pred + b * per;
  const float* g = LAYOUT == GS_ROBUST_VALUES ? nullptr : a.gt + b * per;
  const uint8_t* m = a.mask ? a.mask + b * a.mask_stride : nullptr;
  uint32_t* out = LAYOUT == GS_ROBUST_VALUES ? nullptr : reinterpret_cast<uint32_t*>(plane + b * a.N);
  uint32_t nans = 0;
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < RL_UNROLL; ++j) {
      const int64_t i = c * RL_CHUNK + j * RL_THREADS + threadIdx.x;
      bool valid = false;
      uint32_t key = 0;
      if (i < a.N) {
        const bool part = !a.over_masked || m[i] != 0;
        key = f_bits(residual_of<LAYOUT>(p, g, i, a.N, a.R));
        if (out) out[i] = part ? key : OUTSIDE;
        valid = part && key <= INF_BITS;
        nans += part && key > INF_BITS;
      }
      hist_add(h, key >> (RL_BITS2 + RL_BITS3), valid);
    }
  }
  __syncthreads();
  hist_merge(h, hist1 + b * RL_BINS1, RL_BINS1);
  nans = wave_sum(nans);
  if ((threadIdx.x & (WAVE - 1)) == 0 && nans) atomicAdd(&state[b * RL_STATE_WORDS + ST_NAN], nans);
}

// Levels 2 and 3: the histogram of the level's 10 bits over the elements whose
// upper bits equal the prefix of rank lo (hist[b][0]) or, where it differs, of
// rank hi (hist[b][1]).
template <int LEVEL>
__global__ __launch_bounds__(RL_THREADS) void rl_hist_kernel(int64_t N, int64_t chunks, const float* __restrict__ values,
                                                             const uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ hist) {
  constexpr int BINS = LEVEL == 2 ? RL_BINS2 : RL_BINS3;
  constexpr int SHIFT = LEVEL == 2 ? RL_BITS3 : 0;          // the level's digit starts at this bit
  constexpr int UPPER = LEVEL == 2 ? RL_BITS2 + RL_BITS3 : RL_BITS3;  // the prefix is everything above it
  __shared__ uint32_t h[2][BINS];
  const int64_t b = blockIdx.y;
  const uint32_t* st = state + b * RL_STATE_WORDS;
  if (st[ST_DEAD]) return;  // uniform
  const uint32_t plo = st[ST_PREFIX], phi = st[ST_PREFIX + 1];
  const bool same = st[ST_SAME] != 0;
  for (int k = threadIdx.x; k < 2 * BINS; k += RL_THREADS) (&h[0][0])[k] = 0;
  __syncthreads();
  const float* v = values + b * N;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < RL_UNROLL; ++j) {
      const int64_t i = c * RL_CHUNK + j * RL_THREADS + threadIdx.x;
      uint32_t key = OUTSIDE;
      if (i < N) key = f_bits(v[i] + 0.f);
      const bool ok = key <= INF_BITS;
      const uint32_t up = key >> UPPER, digit = (key >> SHIFT) & (BINS - 1);
      hist_add(h[0], digit, ok && up == plo);
      if (!same) hist_add(h[1], digit, ok && up == phi);  // uniform
    }
  }
  __syncthreads();
  hist_merge(h[0], hist + b * 2 * BINS, BINS);
  if (!same) hist_merge(h[1], hist + (b * 2 + 1) * BINS, BINS);
}

// One workgroup per plane: the bin of `hs` (BINS counts in LDS, `part` the
// sums of each thread's PER consecutive bins) that holds rank k, and the rank
// inside it.  Thread 0 only.
template <int BINS>
__device__ inline void find_rank(const uint32_t* hs, const uint32_t* part, uint32_t k, uint32_t& bin, uint32_t& rem) {
  constexpr int PER = BINS / RL_THREADS;
  uint32_t cum = 0;
  int t = 0;
  while (t < RL_THREADS - 1 && cum + part[t] <= k) cum += part[t++];
  int j = t * PER;
  while (j < t * PER + PER - 1 && cum + hs[j] <= k) cum += hs[j++];
  bin = (uint32_t)j;
  rem = k - cum;
}

template <int LEVEL>
__global__ __launch_bounds__(RL_THREADS) void rl_select_kernel(double q, uint32_t* __restrict__ state,
                                                               const uint32_t* __restrict__ hist,
                                                               double* __restrict__ stats) {
  constexpr int BINS = LEVEL == 1 ? RL_BINS1 : LEVEL == 2 ? RL_BINS2 : RL_BINS3;
  constexpr int PER = BINS / RL_THREADS;
  constexpr int BITS = LEVEL == 1 ? RL_BITS1 : LEVEL == 2 ? RL_BITS2 : RL_BITS3;
  __shared__ uint32_t hs[BINS];
  __shared__ uint32_t part[RL_THREADS];
  const int64_t b = blockIdx.x;
  uint32_t* st = state + b * RL_STATE_WORDS;
  double* out = stats + b * RL_STATS;
  const int tid = threadIdx.x;
  if (LEVEL > 1 && st[ST_DEAD]) return;  // uniform
  const bool same = LEVEL > 1 && st[ST_SAME] != 0;
  uint32_t prefix[2] = {0, 0}, rank[2] = {0, 0};
  for (int s = 0; s < 2; ++s) {  // rank lo, then rank hi
    const uint32_t* src = LEVEL == 1 ? hist + b * BINS : hist + (b * 2 + (same ? 0 : s)) * BINS;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const uint32_t v = src[tid * PER + j];
      hs[tid * PER + j] = v;
      sum += v;
    }
    part[tid] = sum;
    __syncthreads();
    if (tid != 0) continue;
    if (LEVEL == 1 && s == 0) {
      uint32_t n = 0;
      for (int t = 0; t < RL_THREADS; ++t) n += part[t];
      const uint32_t nans = st[ST_NAN];
      out[1] = 0.0;
      out[2] = 0.0;
      out[3] = (double)nans;
      if (nans != 0 || n == 0) {
        st[ST_DEAD] = 1;
        out[0] = nan("");
      } else {
        const double r = q * (double)(n - 1);
        const double lo = floor(r);
        const uint32_t ilo = (uint32_t)lo, ihi = ilo + 1 < n ? ilo + 1 : n - 1;
        *reinterpret_cast<double*>(st + ST_W) = r - lo;
        st[ST_RANK] = ilo;
        st[ST_RANK + 1] = ihi;
      }
    }
    if (st[ST_DEAD]) continue;
    uint32_t bin, rem;
    find_rank<BINS>(hs, part, st[ST_RANK + s], bin, rem);
    prefix[s] = ((LEVEL == 1 ? 0u : st[ST_PREFIX + s]) << BITS) | bin;
    rank[s] = rem;
  }
  if (tid != 0 || st[ST_DEAD]) return;
  st[ST_PREFIX] = prefix[0];
  st[ST_PREFIX + 1] = prefix[1];
  st[ST_RANK] = rank[0];
  st[ST_RANK + 1] = rank[1];
  st[ST_SAME] = prefix[0] == prefix[1];
  if (LEVEL == 3) {  // the prefixes are the two order statistics' bits
    const double vlo = (double)bits_f(prefix[0]), vhi = (double)bits_f(prefix[1]);
    const double w = *reinterpret_cast<const double*>(st + ST_W);
    out[0] = vlo + w * (vhi - vlo);
  }
}

// FROM_PLANE: e from the residual plane, kept iff it takes part and
// (double)e < thr.  Otherwise (select = 0) e from pred and gt and every
// participating element is kept.
template <int LAYOUT, bool FROM_PLANE>
__global__ __launch_bounds__(RL_THREADS) void rl_reduce_kernel(RlArgs a, const float* __restrict__ plane,
                                                               const double* __restrict__ stats,
                                                               double* __restrict__ partials) {
  __shared__ double red[RL_WAVES][RL_PART];
  const int64_t b = blockIdx.y;
  const float* p = FROM_PLANE ? plane + b * a.N : a.pred + b * a.N * a.R;
  const float* g = FROM_PLANE ? nullptr : a.gt + b * a.N * a.R;
  const uint8_t* m = a.mask ? a.mask + b * a.mask_stride : nullptr;
  const double thr = FROM_PLANE ? stats[b * RL_STATS] : 0.0;
  double S = 0.0, cnt = 0.0, cm = 0.0, nans = 0.0;
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < RL_UNROLL; ++j) {
      const int64_t i = c * RL_CHUNK + j * RL_THREADS + threadIdx.x;
      if (i >= a.N) continue;
      const bool mb = m ? m[i] != 0 : true;
      const bool part = a.over_masked ? mb : true;
      const float e = FROM_PLANE ? p[i] : residual_of<LAYOUT>(p, g, i, a.N, a.R);
      const bool kept = part && (FROM_PLANE ? (double)e < thr : true);
      if (kept) {
        cnt += 1.0;
        cm += mb ? 1.0 : 0.0;
        S += (double)(e * (mb ? 1.f : 0.f));  // the reference's (e * mask)[kept]
      }
      if (!FROM_PLANE) nans += part && e != e;
    }
  }
  S = wave_sum(S);
  cnt = wave_sum(cnt);
  cm = wave_sum(cm);
  nans = wave_sum(nans);
  const int tid = threadIdx.x;
  if ((tid & (WAVE - 1)) == 0) {
    double* r = red[tid / WAVE];
    r[0] = S; r[1] = cnt; r[2] = cm; r[3] = nans;
  }
  __syncthreads();
  if (tid < RL_PART) {
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < RL_WAVES; ++w) v += red[w][tid];
    partials[((int64_t)b * gridDim.x + blockIdx.x) * RL_PART + tid] = v;
  }
}

// The denominator of a plane from its kept count and masked kept count.
__device__ inline double denominator(int normalize, int norm_width, double cnt, double cm) {
  return normalize ? (double)norm_width * cm + 1e-8 : cnt;
}

__global__ void rl_finish_kernel(int B, int groups, int select, int normalize, int norm_width, int skip,
                                 const double* __restrict__ partials, float* __restrict__ losses,
                                 double* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* r = partials + (int64_t)b * groups * RL_PART;
  double S = 0.0, cnt = 0.0, cm = 0.0, nans = 0.0;
  for (int i = 0; i < groups; ++i) {
    S += r[i * RL_PART];
    cnt += r[i * RL_PART + 1];
    cm += r[i * RL_PART + 2];
    nans += r[i * RL_PART + 3];
  }
  double* s = stats + (int64_t)b * RL_STATS;
  if (!select) {
    s[0] = INFINITY;
    s[3] = nans;
  }
  s[1] = cnt;
  s[2] = cm;
  const double D = denominator(normalize, norm_width, cnt, cm);
  float loss = (float)(S / D);  // 0/0 = NaN for an empty kept set without normalize
  if (!normalize && cnt == 0.0 && skip) loss = 0.f;
  losses[b] = loss;
}

template <int LAYOUT>
__global__ __launch_bounds__(RL_THREADS) void rl_bwd_kernel(RlArgs a, const double* __restrict__ stats,
                                                            const float* __restrict__ dL_dloss,
                                                            float* __restrict__ d_pred) {
  const int64_t b = blockIdx.y;
  const int64_t per = a.N * a.R;
  const float* p = a.pred + b * per;
  const float* g = a.gt + b * per;
  float* out = d_pred + b * per;
  const uint8_t* m = a.mask ? a.mask + b * a.mask_stride : nullptr;
  // the plane's scalars: uniform addresses
  const double* s = stats + b * RL_STATS;
  const double thr = s[0];
  const double D = denominator(a.normalize, a.norm_width, s[1], s[2]);
  const double scale = (double)dL_dloss[b] * 2.0 / ((double)a.R * D);
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < RL_UNROLL; ++j) {
      const int64_t i = c * RL_CHUNK + j * RL_THREADS + threadIdx.x;
      if (i >= a.N) continue;
      const bool mb = m ? m[i] != 0 : true;
      bool live = mb;  // kept and masked; over_masked only narrows `kept` to masked elements
      if (live && a.select) live = (double)residual_of<LAYOUT>(p, g, i, a.N, a.R) < thr;
      for (int ch = 0; ch < a.R; ++ch) {
        const int64_t k = LAYOUT == GS_ROBUST_CHANNELS ? (int64_t)ch * a.N + i : i * a.R + ch;
        out[k] = live ? (float)(scale * ((double)p[k] - (double)g[k])) : 0.f;
      }
    }
  }
}

RlArgs kernel_args(const gs_robust_loss& a, const RobustLossLayout& L) {
  RlArgs k{};
  k.N = a.N;
  k.chunks = L.chunks;
  k.R = a.R;
  k.pred = a.pred;
  k.gt = a.gt;
  k.mask = a.mask;
  k.mask_stride = a.mask ? a.mask_batch_stride : 0;
  k.q = a.quantile;
  k.select = a.select != 0;
  k.over_masked = a.over_masked != 0;
  k.normalize = a.normalize != 0;
  k.norm_width = a.norm_width;
  k.skip = a.skip_degenerate != 0;
  return k;
}

}  // namespace

extern "C" {

int gs_robust_loss_forward(const gs_robust_loss* args, gs_stream_t stream) {
  if (int e = gs_robust_loss_validate(args, 0, nullptr, nullptr)) return e;
  const gs_robust_loss& a = *args;
  const bool values = a.layout == GS_ROBUST_VALUES;
  const RobustLossLayout L(a.B, a.N, !values);
  const RlArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* state = at<uint32_t>(a.workspace, L.state);
  uint32_t* hist1 = at<uint32_t>(a.workspace, L.hist1);
  uint32_t* hist2 = at<uint32_t>(a.workspace, L.hist2);
  uint32_t* hist3 = at<uint32_t>(a.workspace, L.hist3);
  double* partials = at<double>(a.workspace, L.partials);
  float* plane = values ? nullptr : at<float>(a.workspace, L.plane);
  const dim3 grid((unsigned)L.groups, (unsigned)a.B), block(RL_THREADS);
  if (k.select) {
    if (hipMemsetAsync(a.workspace, 0, L.zero_bytes, s) != hipSuccess) return launch_status("robust loss forward", 0, s);
    if (a.layout == GS_ROBUST_CHANNELS)
      hipLaunchKernelGGL(rl_residual_kernel<GS_ROBUST_CHANNELS>, grid, block, 0, s, k, state, hist1, plane);
    else if (a.layout == GS_ROBUST_ROWS)
      hipLaunchKernelGGL(rl_residual_kernel<GS_ROBUST_ROWS>, grid, block, 0, s, k, state, hist1, plane);
    else
      hipLaunchKernelGGL(rl_residual_kernel<GS_ROBUST_VALUES>, grid, block, 0, s, k, state, hist1, plane);
    const float* vals = values ? a.pred : plane;
    hipLaunchKernelGGL(rl_select_kernel<1>, dim3((unsigned)a.B), block, 0, s, k.q, state, hist1, a.stats);
    hipLaunchKernelGGL(rl_hist_kernel<2>, grid, block, 0, s, k.N, k.chunks, vals, state, hist2);
    hipLaunchKernelGGL(rl_select_kernel<2>, dim3((unsigned)a.B), block, 0, s, k.q, state, hist2, a.stats);
    hipLaunchKernelGGL(rl_hist_kernel<3>, grid, block, 0, s, k.N, k.chunks, vals, state, hist3);
    hipLaunchKernelGGL(rl_select_kernel<3>, dim3((unsigned)a.B), block, 0, s, k.q, state, hist3, a.stats);
    if (values) return launch_status("robust loss forward", 0, s);
    hipLaunchKernelGGL((rl_reduce_kernel<GS_ROBUST_CHANNELS, true>), grid, block, 0, s, k, plane, a.stats, partials);
  } else if (a.layout == GS_ROBUST_CHANNELS) {
    hipLaunchKernelGGL((rl_reduce_kernel<GS_ROBUST_CHANNELS, false>), grid, block, 0, s, k, plane, a.stats, partials);
  } else {
    hipLaunchKernelGGL((rl_reduce_kernel<GS_ROBUST_ROWS, false>), grid, block, 0, s, k, plane, a.stats, partials);
  }
  hipLaunchKernelGGL(rl_finish_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, (int)a.B, (int)L.groups,
                     k.select, k.normalize, k.norm_width, k.skip, partials, a.losses, a.stats);
  return launch_status("robust loss forward", 0, s);
}

int gs_robust_loss_backward(const gs_robust_loss* args, const float* dL_dloss, float* dL_dpred, gs_stream_t stream) {
  if (int e = gs_robust_loss_validate(args, 1, dL_dloss, dL_dpred)) return e;
  const gs_robust_loss& a = *args;
  const RobustLossLayout L(a.B, a.N, true);
  const RlArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.groups, (unsigned)a.B), block(RL_THREADS);
  if (a.layout == GS_ROBUST_CHANNELS)
    hipLaunchKernelGGL(rl_bwd_kernel<GS_ROBUST_CHANNELS>, grid, block, 0, s, k, a.stats, dL_dloss, dL_dpred);
  else
    hipLaunchKernelGGL(rl_bwd_kernel<GS_ROBUST_ROWS>, grid, block, 0, s, k, a.stats, dL_dloss, dL_dpred);
  return launch_status("robust loss backward", 0, s);
}

}  // extern "C"
