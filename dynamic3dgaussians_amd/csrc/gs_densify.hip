// gs_densify.hip -- densification (include/gs_densify.h): the reference's
// clone / split / prune pass (external.py:244-292) with the Adam moments that
// move with every row, as one classification, one prefix scan and one gather.
//
// gs_densify_plan, three launches, reduce-then-scan (no workgroup ever waits
// on another, no atomics):
//   dn_classify_kernel  one workgroup per DN_BLOCK Gaussians: the flag byte of
//                       each, and the workgroup's four set sizes
//   dn_scan_sums_kernel ONE workgroup: exclusive scan of the per-workgroup
//                       sizes in passes of DN_TILE with a running carry; the
//                       four totals
//   dn_rank_kernel      one workgroup per DN_BLOCK Gaussians: exclusive ranks
//                       = the workgroup's offsets + a scan inside the workgroup
// The four counters of a Gaussian travel as four 16-bit fields of one 64-bit
// word through the in-workgroup scan (a workgroup holds DN_BLOCK = 1024
// Gaussians, so no field can carry into the next).
//
// gs_densify_apply, one launch: workgroups walk a flattened chunk space over
// the tensor table (kernel argument, <= 16 entries) and the three statistics
// arrays.  Every source element is read once and written to at most
// n_split rows; rows of a block stay in source order, so neighbouring lanes
// write neighbouring addresses.  A tensor whose width is a multiple of 4 and
// whose six pointers are 16-byte aligned moves as float4; every other tensor
// (widths 1 and 3, rows at odd offsets of a larger buffer) moves float by
// float.  This file is built with -ffp-contract=off: the split formulas keep
// the operation order of the PyTorch statement.
#include <hip/hip_runtime.h>

#include "../../include/gs_densify.h"
#include "gs_common.h"
#include "gs_densify_layout.h"
#include "gs_host_util.h"
#include "gs_launch.h"

namespace gs {

namespace {

struct PlanK {
  int64_t P;
  const float *accum, *denom, *log_scales, *logit;
  float thresh, clone_max, min_opacity, big, split_div;
  int big_on;
};

// the four set memberships of a flag byte, one per 16-bit field
__device__ inline uint64_t member_bits(unsigned f) {
  const bool split = f & GS_DENSIFY_SPLIT, prune = f & GS_DENSIFY_PRUNE;
  uint64_t m = 0;
  if (!split && !prune) m |= 1ull << (16 * GS_DENSIFY_KEPT_ORIGINALS);
  if ((f & GS_DENSIFY_CLONE) && !prune) m |= 1ull << (16 * GS_DENSIFY_KEPT_CLONES);
  if (split) m |= 1ull << (16 * GS_DENSIFY_ALL_SPLITS);
  if (split && !(f & GS_DENSIFY_PRUNE_SPLIT)) m |= 1ull << (16 * GS_DENSIFY_KEPT_SPLITS);
  return m;
}

__device__ inline int4 unpack4(uint64_t v) {
  return make_int4((int)(v & 0xFFFF), (int)((v >> 16) & 0xFFFF), (int)((v >> 32) & 0xFFFF), (int)(v >> 48));
}

__device__ inline unsigned classify(const PlanK& k, int64_t i) {
  float g = k.accum[i] / k.denom[i];
  if (g != g) g = 0.f;  // grads[grads.isnan()] = 0
  const float* ls = k.log_scales + 3 * i;
  const float s = fmaxf(fmaxf(expf(ls[0]), expf(ls[1])), expf(ls[2]));
  const bool hot = g >= k.thresh;
  unsigned f = 0;
  if (hot && s <= k.clone_max) f |= GS_DENSIFY_CLONE;
  if (hot && s > k.clone_max) f |= GS_DENSIFY_SPLIT;
  const bool faint = 1.f / (1.f + expf(-k.logit[i])) < k.min_opacity;
  if (faint || (k.big_on && s > k.big)) f |= GS_DENSIFY_PRUNE;
  if (faint || (k.big_on && s / k.split_div > k.big)) f |= GS_DENSIFY_PRUNE_SPLIT;
  return f;
}

// Exclusive scan of one 64-bit value per thread over the workgroup's
// DN_THREADS threads; *total = the workgroup's sum.  sh holds one word per wave.
__device__ inline uint64_t block_excl_scan64(uint64_t x, uint64_t* sh, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t inc = wave_incl_scan(x, lane);
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < DN_THREADS / 64; ++w) {
    if (w < wave) before += sh[w];
    all += sh[w];
  }
  __syncthreads();  // sh may be reused by the caller's next scan
  *total = all;
  return before + inc - x;
}

__global__ void __launch_bounds__(DN_THREADS) dn_classify_kernel(const PlanK k, uint8_t* __restrict__ flags,
                                                                int4* __restrict__ sums) {
  __shared__ uint64_t sh[DN_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * DN_BLOCK;
  uint64_t mine = 0;
#pragma unroll
  for (int j = 0; j < DN_ITEMS; ++j) {
    const int64_t i = base + j * DN_THREADS + threadIdx.x;
    if (i < k.P) {
      const unsigned f = classify(k, i);
      flags[i] = (uint8_t)f;
      mine += member_bits(f);
    }
  }
  uint64_t total;
  block_excl_scan64(mine, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = unpack4(total);
}

// One workgroup.  sums [blocks] become exclusive offsets in place.
__global__ void __launch_bounds__(DN_THREADS) dn_scan_sums_kernel(int64_t blocks, int4* __restrict__ sums,
                                                                 int64_t* __restrict__ counts) {
  __shared__ int sh[4][DN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry[4] = {0, 0, 0, 0};
  for (int64_t tile = 0; tile < blocks; tile += DN_TILE) {
    // DN_ITEMS consecutive sums per thread
    int4 v[DN_ITEMS];
    int mine[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < DN_ITEMS; ++j) {
      const int64_t b = tile + (int64_t)threadIdx.x * DN_ITEMS + j;
      v[j] = b < blocks ? sums[b] : make_int4(0, 0, 0, 0);
      mine[0] += v[j].x; mine[1] += v[j].y; mine[2] += v[j].z; mine[3] += v[j].w;
    }
    int excl[4], all[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int inc = wave_incl_scan(mine[c], lane);
      if (lane == 63) sh[c][wave] = inc;
      excl[c] = inc - mine[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int before = 0, sum = 0;
#pragma unroll
      for (int w = 0; w < DN_THREADS / 64; ++w) {
        if (w < wave) before += sh[c][w];
        sum += sh[c][w];
      }
      excl[c] += before + carry[c];
      all[c] = sum;
    }
    __syncthreads();
    int4 run = make_int4(excl[0], excl[1], excl[2], excl[3]);
#pragma unroll
    for (int j = 0; j < DN_ITEMS; ++j) {
      const int64_t b = tile + (int64_t)threadIdx.x * DN_ITEMS + j;
      if (b < blocks) sums[b] = run;
      run.x += v[j].x; run.y += v[j].y; run.z += v[j].z; run.w += v[j].w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) carry[c] += all[c];
  }
  if (threadIdx.x == 0) {
    counts[0] = carry[0]; counts[1] = carry[1]; counts[2] = carry[2]; counts[3] = carry[3];
  }
}

__global__ void __launch_bounds__(DN_THREADS) dn_rank_kernel(int64_t P, const uint8_t* __restrict__ flags,
                                                            const int4* __restrict__ sums,
                                                            int4* __restrict__ ranks) {
  __shared__ uint64_t sh[DN_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * DN_BLOCK + (int64_t)threadIdx.x * DN_ITEMS;  // consecutive items
  uint64_t m[DN_ITEMS], mine = 0;
#pragma unroll
  for (int j = 0; j < DN_ITEMS; ++j) {
    m[j] = base + j < P ? member_bits(flags[base + j]) : 0ull;
    mine += m[j];
  }
  uint64_t total;
  uint64_t run = block_excl_scan64(mine, sh, &total);
  const int4 off = sums[blockIdx.x];
#pragma unroll
  for (int j = 0; j < DN_ITEMS; ++j) {
    if (base + j < P) {
      const int4 r = unpack4(run);
      ranks[base + j] = make_int4(off.x + r.x, off.y + r.y, off.z + r.z, off.w + r.w);
    }
    run += m[j];
  }
}

// ---- apply ----

constexpr int DA_UNROLL = 4;
constexpr int DA_CHUNK = DN_THREADS * DA_UNROLL;  // units (floats or float4s) per workgroup

struct ApplyK {
  int64_t P, P_new;
  int64_t ko, kc, as, ks;  // the four totals
  const uint8_t* flags;
  const int4* ranks;
  const float* noise;
  const float *log_scales, *rotations;  // sources of the tensors with those roles
  float* stats[3];
  float split_div, opacity_reset;
  int reset_opacity, n_tensors;
  int64_t chunk_start[GS_DENSIFY_MAX_TENSORS + 2];  // prefix of per-tensor chunk counts, then the statistics
  gs_densify_tensor t[GS_DENSIFY_MAX_TENSORS];
  uint32_t vec_mask;  // bit t: tensor t moves as float4
};

// Destination rows of source Gaussian i: up to two (an original and its clone,
// or the two copies of a split); -1 = none.  Every row is checked against its
// block's size, so no count the caller passes can place a row outside
// [0, P_new).
struct Rows {
  int64_t a, b;
  bool split;
  int64_t noise_a, noise_b;
};

__device__ inline Rows rows_of(const ApplyK& k, int64_t i) {
  const unsigned f = k.flags[i];
  const int4 r = k.ranks[i];
  Rows o;
  o.a = o.b = -1;
  o.noise_a = o.noise_b = 0;
  o.split = f & GS_DENSIFY_SPLIT;
  if (o.split) {
    if (!(f & GS_DENSIFY_PRUNE_SPLIT) && r.w >= 0 && r.w < k.ks && r.z >= 0 && r.z < k.as) {
      o.a = k.ko + k.kc + r.w;
      o.b = o.a + k.ks;
      o.noise_a = r.z;
      o.noise_b = k.as + r.z;
    }
  } else if (!(f & GS_DENSIFY_PRUNE)) {
    if (r.x >= 0 && r.x < k.ko) o.a = r.x;
    if ((f & GS_DENSIFY_CLONE) && r.y >= 0 && r.y < k.kc) o.b = k.ko + r.y;
  }
  return o;
}

// component c of R(q / |q|) (exp(log_scales) * z): build_rotation's element
// formulas (external.py:61-78) and the row-times-vector sum of torch.bmm
__device__ inline float split_offset(const ApplyK& k, int64_t i, int c, int64_t noise_row) {
  const float* q = k.rotations + 4 * i;
  const float* ls = k.log_scales + 3 * i;
  const float* z = k.noise + 3 * noise_row;
  const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, w = q[3] / norm;
  const float v0 = expf(ls[0]) * z[0], v1 = expf(ls[1]) * z[1], v2 = expf(ls[2]) * z[2];
  float m0, m1, m2;
  if (c == 0) {
    m0 = 1.f - 2.f * (y * y + w * w); m1 = 2.f * (x * y - r * w); m2 = 2.f * (x * w + r * y);
  } else if (c == 1) {
    m0 = 2.f * (x * y + r * w); m1 = 1.f - 2.f * (x * x + w * w); m2 = 2.f * (y * w - r * x);
  } else {
    m0 = 2.f * (x * w - r * y); m1 = 2.f * (y * w + r * x); m2 = 1.f - 2.f * (x * x + y * y);
  }
  return m0 * v0 + m1 * v1 + m2 * v2;
}

// e / w, in 32 bits where the tensor allows (a 64-bit division is a long instruction sequence)
__device__ inline int64_t row_of(int64_t e, int w, int64_t units) {
  return units <= 0xFFFFFFFFll ? (int64_t)((uint32_t)e / (uint32_t)w) : e / w;
}

__global__ void __launch_bounds__(DN_THREADS) dn_apply_kernel(const ApplyK k) {
  const int64_t c = blockIdx.x;
  if (c >= k.chunk_start[k.n_tensors]) {  // the statistics: zeros at the new length
    const int64_t base = (c - k.chunk_start[k.n_tensors]) * DA_CHUNK;
#pragma unroll
    for (int u = 0; u < DA_UNROLL; ++u) {
      const int64_t e = base + (int64_t)u * DN_THREADS + threadIdx.x;
      if (e < k.P_new) {
#pragma unroll
        for (int s = 0; s < 3; ++s)
          if (k.stats[s]) k.stats[s][e] = 0.f;
      }
    }
    return;
  }
  int t = 0;
  while (t + 1 < k.n_tensors && c >= k.chunk_start[t + 1]) ++t;
  const gs_densify_tensor& T = k.t[t];
  const int64_t base = (c - k.chunk_start[t]) * DA_CHUNK;
  const int w = T.width;
  const bool has_src_m = T.src_exp_avg != nullptr, has_dst_m = T.dst_exp_avg != nullptr;
  if ((k.vec_mask >> t) & 1u) {  // plain rows of float4s
    const int w4 = w >> 2;
    const int64_t units = k.P * w4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < DA_UNROLL; ++u) {
      const int64_t e = base + (int64_t)u * DN_THREADS + threadIdx.x;
      if (e >= units) continue;
      const int64_t i = row_of(e, w4, units);
      const int col = (int)(e - i * w4);
      const Rows R = rows_of(k, i);
      if (R.a < 0 && R.b < 0) continue;
      const float4 p = reinterpret_cast<const float4*>(T.src)[e];
      if (R.a >= 0) {
        const int64_t d = R.a * w4 + col;
        reinterpret_cast<float4*>(T.dst)[d] = p;
        if (has_dst_m) {
          const bool keep = !R.split && has_src_m;  // an original keeps its moments
          float4 m = zero, v = zero;
          if (keep) {
            m = reinterpret_cast<const float4*>(T.src_exp_avg)[e];
            v = reinterpret_cast<const float4*>(T.src_exp_avg_sq)[e];
          }
          reinterpret_cast<float4*>(T.dst_exp_avg)[d] = m;
          reinterpret_cast<float4*>(T.dst_exp_avg_sq)[d] = v;
        }
      }
      if (R.b >= 0) {
        const int64_t d = R.b * w4 + col;
        reinterpret_cast<float4*>(T.dst)[d] = p;
        if (has_dst_m) {
          reinterpret_cast<float4*>(T.dst_exp_avg)[d] = zero;
          reinterpret_cast<float4*>(T.dst_exp_avg_sq)[d] = zero;
        }
      }
    }
    return;
  }
  const int64_t units = k.P * w;
  const int role = T.role;
#pragma unroll
  for (int u = 0; u < DA_UNROLL; ++u) {
    const int64_t e = base + (int64_t)u * DN_THREADS + threadIdx.x;
    if (e >= units) continue;
    const int64_t i = row_of(e, w, units);
    const int col = (int)(e - i * w);
    const Rows R = rows_of(k, i);
    if (R.a < 0 && R.b < 0) continue;
    const float p = T.src[e];
    float pa = p, pb = p;
    bool keep = !R.split && has_src_m;
    if (role == GS_DENSIFY_ROLE_LOGIT_OPACITIES && k.reset_opacity) {
      pa = pb = k.opacity_reset;
      keep = false;
    } else if (R.split && role == GS_DENSIFY_ROLE_MEANS) {
      pa = p + split_offset(k, i, col, R.noise_a);
      pb = p + split_offset(k, i, col, R.noise_b);
    } else if (R.split && role == GS_DENSIFY_ROLE_LOG_SCALES) {
      pa = pb = logf(expf(p) / k.split_div);
    }
    if (R.a >= 0) {
      const int64_t d = R.a * w + col;
      T.dst[d] = pa;
      if (has_dst_m) {
        T.dst_exp_avg[d] = keep ? T.src_exp_avg[e] : 0.f;
        T.dst_exp_avg_sq[d] = keep ? T.src_exp_avg_sq[e] : 0.f;
      }
    }
    if (R.b >= 0) {
      const int64_t d = R.b * w + col;
      T.dst[d] = pb;
      if (has_dst_m) {
        T.dst_exp_avg[d] = 0.f;
        T.dst_exp_avg_sq[d] = 0.f;
      }
    }
  }
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" {

int gs_densify_plan(const gs_densify_plan_args* args, gs_stream_t stream) {
  if (int e = gs_densify_plan_validate(args)) return e;
  const gs_densify_plan_args& a = *args;
  if (a.P == 0) return 0;
  const DensifyLayout L(a.P);
  PlanK k{};
  k.P = a.P;
  k.accum = a.grad_accum;
  k.denom = a.denom;
  k.log_scales = a.log_scales;
  k.logit = a.logit_opacities;
  k.thresh = a.grad_thresh;
  k.clone_max = a.clone_max_scale;
  k.min_opacity = a.prune_min_opacity;
  k.big = a.prune_max_scale;
  k.big_on = a.prune_max_scale > 0.f;
  k.split_div = (float)(0.8 * a.n_split);
  char* ws = static_cast<char*>(a.workspace);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  int4* ranks = reinterpret_cast<int4*>(ws + L.ranks);
  int4* sums = reinterpret_cast<int4*>(ws + L.sums);
  int64_t* counts = reinterpret_cast<int64_t*>(ws + L.counts);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dn_classify_kernel, dim3((unsigned)L.blocks), dim3(DN_THREADS), 0, s, k, flags, sums);
  hipLaunchKernelGGL(dn_scan_sums_kernel, dim3(1), dim3(DN_THREADS), 0, s, L.blocks, sums, counts);
  hipLaunchKernelGGL(dn_rank_kernel, dim3((unsigned)L.blocks), dim3(DN_THREADS), 0, s, a.P, flags, sums, ranks);
  return launch_status("densify plan", 0, s);
}

int gs_densify_apply(const gs_densify_apply_args* args, gs_stream_t stream) {
  if (int e = gs_densify_apply_validate(args)) return e;
  const gs_densify_apply_args& a = *args;
  const int64_t P_new = gs_densify_new_count(a.counts, a.n_split);
  if (a.P == 0 || P_new == 0) return 0;
  const DensifyLayout L(a.P);
  ApplyK k{};
  k.P = a.P;
  k.P_new = P_new;
  k.ko = a.counts[GS_DENSIFY_KEPT_ORIGINALS];
  k.kc = a.counts[GS_DENSIFY_KEPT_CLONES];
  k.as = a.counts[GS_DENSIFY_ALL_SPLITS];
  k.ks = a.counts[GS_DENSIFY_KEPT_SPLITS];
  const char* ws = static_cast<const char*>(a.workspace);
  k.flags = reinterpret_cast<const uint8_t*>(ws + L.flags);
  k.ranks = reinterpret_cast<const int4*>(ws + L.ranks);
  k.noise = a.noise;
  k.split_div = (float)(0.8 * a.n_split);
  k.opacity_reset = a.opacity_reset;
  k.reset_opacity = a.reset_opacity != 0;
  k.n_tensors = a.n_tensors;
  int64_t c = 0;
  for (int t = 0; t < a.n_tensors; ++t) {
    const gs_densify_tensor& x = a.t[t];
    k.t[t] = x;
    if (x.role == GS_DENSIFY_ROLE_LOG_SCALES) k.log_scales = x.src;
    if (x.role == GS_DENSIFY_ROLE_ROTATIONS) k.rotations = x.src;
    // the rotations' own rows are a plain copy; the other roles have widths 1 and 3
    const bool plain = x.role == GS_DENSIFY_ROLE_PLAIN || x.role == GS_DENSIFY_ROLE_ROTATIONS;
    const bool vec = plain && (x.width & 3) == 0 && aligned16(x.src) && aligned16(x.src_exp_avg) &&
               aligned16(x.src_exp_avg_sq) && aligned16(x.dst) && aligned16(x.dst_exp_avg) &&
               aligned16(x.dst_exp_avg_sq);
    if (vec) k.vec_mask |= 1u << t;
    const int64_t units = vec ? a.P * (x.width >> 2) : a.P * x.width;
    k.chunk_start[t] = c;
    c += (units + DA_CHUNK - 1) / DA_CHUNK;
  }
  k.chunk_start[a.n_tensors] = c;
  bool any_stats = false;
  for (int s = 0; s < 3; ++s) {
    k.stats[s] = a.stats[s];
    any_stats = any_stats || a.stats[s];
  }
  if (any_stats) c += (P_new + DA_CHUNK - 1) / DA_CHUNK;
  k.chunk_start[a.n_tensors + 1] = c;
  if (c == 0) return 0;
  if (c > 0x7FFFFFFF) return gs_set_error(-1, "densify apply: too many workgroups (%lld)", (long long)c);
  hipLaunchKernelGGL(dn_apply_kernel, dim3((unsigned)c), dim3(DN_THREADS), 0, (hipStream_t)stream, k);
  return launch_status("densify apply", 0, (hipStream_t)stream);
}

}  // extern "C"
