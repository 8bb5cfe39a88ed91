// gs_feature_knn.hip -- exact cosine top-k in feature space (C ABI, definition
// and the certificate: include/gs_feature_knn.h; sizes and the bound:
// gs_feature_knn_layout.h).
//
//   fk_normalize_kernel  xh = fl32(x / max(|x|, 1e-12)), fp64, a thread per row,
//                        rows and channels padded with zeros
//   fk_pieces_kernel     xh's three bf16 pieces in operand order:
//                        pc[((tile * nks + ks) * 3 + piece) * 64 + lane] holds
//                        xh[32 tile + (lane & 31)][16 ks + 8 (lane >> 5) + 0..7]
//                        -- the A operand of a query tile and the B operand of
//                        a database tile alike
//   fk_scan_kernel       a workgroup = 4 waves = 4 query tiles of 32 rows (their
//                        pieces in registers) x one database chunk, walked in
//                        32-row tiles through a double-buffered LDS stage.  The
//                        accumulator of lane l, register i is query row
//                        (i & 3) + 8 (i >> 2) + 4 (l >> 5) against database row
//                        l & 31.  A value that passes its row's threshold is
//                        appended to the row's LDS buffer (an integer LDS
//                        atomic hands out the slot); a row holding more than
//                        FK_CAP - 32 entries is merged by its wave down to the
//                        kp best by (st, index) and its threshold rises to the
//                        kp-th.  What is kept is the set of the kp largest keys
//                        seen: it does not depend on the order of arrival.
//   fk_rerank_kernel     a wave per query: exact fp64 similarities of what the
//                        chunks kept, k rounds of arg-max, the certificate
//   fk_fallback_kernel   a fixed grid over the device-side list of the rows
//                        the certificate refused: exact fp64 top-k over the
//                        whole database, each dot product formed once
//
// A row's buffers belong to one wave, so the scan needs no workgroup barrier
// beyond the stage's.  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_feature_knn.h"
#include "gs_feature_knn_layout.h"
#include "gs_launch.h"
#include "gs_split_mfma.h"

using namespace gs;
using namespace gs::smf;

namespace {

typedef unsigned long long u64;

__device__ inline int acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// floats as unsigned integers of the same order (-0 below +0)
__device__ inline uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float ord2f(uint32_t o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu)); }
// larger key = better: st descending, then index ascending.  Never 0.
__device__ inline u64 make_key(float s, uint32_t j) { return ((u64)f2ord(s) << 32) | (u64)(0xffffffffu - j); }
__device__ inline float key_sim(u64 k) { return ord2f((uint32_t)(k >> 32)); }
__device__ inline int key_index(u64 k) { return (int)(0xffffffffu - (uint32_t)k); }

// the lanes of one wave hand LDS data to each other
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline bool better(double s1, int i1, double s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// ------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void fk_normalize_kernel(int64_t rows, int64_t rows_pad, int E, int e_pad,
                                                           const float* __restrict__ x, float* __restrict__ xh) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows_pad) return;
  float* o = xh + r * e_pad;
  if (r >= rows) {
    for (int c = 0; c < e_pad; ++c) o[c] = 0.f;
    return;
  }
  const float* xi = x + r * E;
  double ss = 0.0;
  for (int c = 0; c < E; ++c) {
    const double v = (double)xi[c];
    ss += v * v;
  }
  const double den = fmax(sqrt(ss), 1e-12);
  for (int c = 0; c < e_pad; ++c) o[c] = c < E ? (float)((double)xi[c] / den) : 0.f;
}

__global__ __launch_bounds__(256) void fk_pieces_kernel(int64_t tiles, int nks, int e_pad, const float* __restrict__ xh,
                                                        u32x4* __restrict__ pc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= tiles * nks * 64) return;
  const int lane = (int)(idx & 63);
  const int64_t frag = idx >> 6, tile = frag / nks;
  const int ks = (int)(frag % nks);
  const float* src = xh + (tile * FK_TILE + (lane & 31)) * e_pad + 16 * ks + 8 * (lane >> 5);
  const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  bsplit s;
  split_bf16(v, s);
#pragma unroll
  for (int i = 0; i < NSP; ++i) pc[(frag * NSP + i) * 64 + lane] = __builtin_bit_cast(u32x4, s.p[i]);
}

// ------------------------------------------------------------------ scan
struct FkScan {
  int M, N, S, kp, self;
  int64_t L, qtiles;
  const u32x4 *pq, *pd;
  float* cand_s;
  int* cand_i;
  int* cnt;
  float* theta;
};

// One wave merges row buffer b (n <= FK_CAP entries, n > kp) down to its kp
// largest keys, sorted descending, and returns nothing: the kp-th is the new
// threshold.
__device__ inline void scan_merge_row(u64* b, int* cntp, u64* thp, int kp, int lane) {
  const int n = *cntp;
  const u64 e0 = lane < n ? b[lane] : 0, e1 = lane + 64 < n ? b[lane + 64] : 0;
  int r0 = 0, r1 = 0;
  for (int f = 0; f < n; ++f) {
    const u64 kf = b[f];
    r0 += kf > e0;
    r1 += kf > e1;
  }
  wave_sync();
  if (lane < n && r0 < kp) {
    b[r0] = e0;
    if (r0 == kp - 1) *thp = e0;
  }
  if (lane + 64 < n && r1 < kp) {
    b[r1] = e1;
    if (r1 == kp - 1) *thp = e1;
  }
  if (lane == 0) *cntp = kp;
  wave_sync();
}

template <int NKS>
__global__ __launch_bounds__(FK_THREADS) void fk_scan_kernel(const FkScan a) {
  constexpr int FR = NKS * NSP * 64;                          // 16-byte words of one database tile
  constexpr int PF = (FR + FK_THREADS - 1) / FK_THREADS;      // of which a thread moves PF
  __shared__ u32x4 stage[2][FR];
  __shared__ u64 buf[FK_ROW_BLOCK][FK_CAP];
  __shared__ u64 thkey[FK_ROW_BLOCK];                         // 0: nothing was dropped yet
  __shared__ int cnt[FK_ROW_BLOCK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, col = lane & 31;
  const int64_t qt = (int64_t)blockIdx.x * FK_WAVES + wave;
  const bool active = qt < a.qtiles;
  const int chunk = blockIdx.y;
  const int64_t lo = (int64_t)chunk * a.L;
  const int64_t hi = lo + a.L < a.N ? lo + a.L : a.N;
  const float inf = __builtin_inff();

  for (int r = tid; r < FK_ROW_BLOCK; r += FK_THREADS) {
    cnt[r] = 0;
    thkey[r] = 0;
  }
  bsplit A[NKS];
  float th[16];
  if (active) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int p = 0; p < NSP; ++p)
        A[ks].p[p] = __builtin_bit_cast(bf16x8, a.pq[((qt * NKS + ks) * NSP + p) * 64 + lane]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) th[i] = active && qt * FK_TILE + acc_row(i, hh) < a.M ? -inf : inf;
  __syncthreads();

  if (lo < hi) {
    const int64_t t0 = lo / FK_TILE, t1 = (hi + FK_TILE - 1) / FK_TILE;
    u32x4 pre[PF];
#pragma unroll
    for (int m = 0; m < PF; ++m)
      if (tid + m * FK_THREADS < FR) stage[0][tid + m * FK_THREADS] = a.pd[t0 * FR + tid + m * FK_THREADS];
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
      const int cur = (int)((t - t0) & 1);
      const bool more = t + 1 < t1;
      if (more) {
#pragma unroll
        for (int m = 0; m < PF; ++m)
          if (tid + m * FK_THREADS < FR) pre[m] = a.pd[(t + 1) * FR + tid + m * FK_THREADS];
      }
      if (active) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          bsplit B;
#pragma unroll
          for (int p = 0; p < NSP; ++p) B.p[p] = __builtin_bit_cast(bf16x8, stage[cur][(ks * NSP + p) * 64 + lane]);
          acc = mfma_split(A[ks], B, acc);
        }
        const int64_t j = t * FK_TILE + col;
        const bool jin = j >= lo && j < hi;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (acc[i] >= th[i]) {  // rare once the threshold has risen
            const int rl = acc_row(i, hh), r = wave * FK_TILE + rl;
            if (jin && !(a.self && qt * FK_TILE + rl == j)) {
              const u64 key = make_key(acc[i], (uint32_t)j);
              if (key > thkey[r]) {
                const int slot = atomicAdd(&cnt[r], 1);
                if (slot < FK_CAP) buf[r][slot] = key;  // always: a row enters a step with <= FK_CAP - 32 entries
              }
            }
          }
        }
        wave_sync();
        const int mine = lane < FK_TILE ? cnt[wave * FK_TILE + lane] : 0;
        u64 full = __ballot(mine > FK_CAP - FK_TILE);
        if (full) {
          while (full) {
            const int r = wave * FK_TILE + (__ffsll((long long)full) - 1);
            full &= full - 1;
            scan_merge_row(buf[r], &cnt[r], &thkey[r], a.kp, lane);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const u64 tk = thkey[wave * FK_TILE + acc_row(i, hh)];
            if (th[i] != inf && tk) th[i] = key_sim(tk);
          }
        }
      }
      if (more) {
#pragma unroll
        for (int m = 0; m < PF; ++m)
          if (tid + m * FK_THREADS < FR) stage[cur ^ 1][tid + m * FK_THREADS] = pre[m];
      }
      __syncthreads();
    }
  }

  if (!active) return;
  for (int rl = 0; rl < FK_TILE; ++rl) {
    const int64_t q = qt * FK_TILE + rl;
    if (q >= a.M) break;
    const int r = wave * FK_TILE + rl;
    wave_sync();
    if (cnt[r] > a.kp) scan_merge_row(buf[r], &cnt[r], &thkey[r], a.kp, lane);
    const int n = cnt[r];
    const int64_t o = q * a.S + chunk;
    if (lane < a.kp) {
      const u64 key = lane < n ? buf[r][lane] : 0;
      a.cand_s[o * a.kp + lane] = lane < n ? key_sim(key) : -inf;
      a.cand_i[o * a.kp + lane] = lane < n ? key_index(key) : -1;
    }
    if (lane == 0) {
      a.cnt[o] = n;
      a.theta[o] = thkey[r] ? key_sim(thkey[r]) : -inf;
    }
  }
}

// ------------------------------------------------------------------ exact similarities
// s = sum_c q[c] * row[c] in fp64, c ascending (the padding adds +0)
__device__ inline double fk_dot(const double* q, const float* __restrict__ row, int e_pad) {
  double s = 0.0;
  for (int c = 0; c < e_pad; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    s = fma(q[c], (double)v.x, s);
    s = fma(q[c + 1], (double)v.y, s);
    s = fma(q[c + 2], (double)v.z, s);
    s = fma(q[c + 3], (double)v.w, s);
  }
  return s;
}

struct FkRerank {
  int M, S, k, kp, e_pad;
  double bound;
  const float *xq, *xd;
  const float* cand_s;
  const int* cand_i;
  const int* cnt;
  const float* theta;
  double* sim;
  int64_t* index;
  int* list;
  u64* counts;  // [0] certified, [1] on the list
};

__global__ __launch_bounds__(64) void fk_rerank_kernel(const FkRerank a) {
  __shared__ double ss[FK_RERANK_MAX];
  __shared__ int si[FK_RERANK_MAX];
  __shared__ double qv[GS_FKNN_MAX_E];
  __shared__ double res_s[GS_KNN_MAX_K];
  __shared__ int res_i[GS_KNN_MAX_K];
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  for (int c = lane; c < a.e_pad; c += 64) qv[c] = (double)a.xq[q * a.e_pad + c];
  __syncthreads();
  int n = 0;
  float thmax = -__builtin_inff();
  for (int c = 0; c < a.S; ++c) {
    const int64_t o = q * a.S + c;
    const int cn = a.cnt[o];
    thmax = fmaxf(thmax, a.theta[o]);
    if (lane < cn) {
      const int j = a.cand_i[o * a.kp + lane];
      ss[n + lane] = fk_dot(qv, a.xd + (int64_t)j * a.e_pad, a.e_pad);
      si[n + lane] = j;
    }
    n += cn;
  }
  __syncthreads();
  for (int r = 0; r < a.k; ++r) {
    double bs = -__builtin_inf();
    int bi = 0x7fffffff, bp = -1;
    for (int p = lane; p < n; p += 64) {
      const int i = si[p];
      if (i >= 0 && (bp < 0 || better(ss[p], i, bs, bi))) {
        bs = ss[p];
        bi = i;
        bp = p;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64), op = __shfl_xor(bp, o, 64);
      if (op >= 0 && (bp < 0 || better(os, oi, bs, bi))) {
        bs = os;
        bi = oi;
        bp = op;
      }
    }
    if (lane == 0) {
      res_s[r] = bp >= 0 ? bs : -__builtin_inf();
      res_i[r] = bp >= 0 ? bi : -1;
      if (bp >= 0) si[bp] = -1;
    }
    __syncthreads();
  }
  const bool certified = thmax == -__builtin_inff() || res_s[a.k - 1] > (double)thmax + a.bound;
  if (certified) {
    if (lane < a.k) {
      a.sim[q * a.k + lane] = res_s[lane];
      a.index[q * a.k + lane] = res_i[lane];
    }
    if (lane == 0) atomicAdd(&a.counts[0], 1ull);
  } else if (lane == 0) {
    a.list[atomicAdd(&a.counts[1], 1ull)] = (int)q;
  }
}

// ------------------------------------------------------------------ fallback
struct FkFallback {
  int N, k, e_pad, self;
  const float *xq, *xd;
  const int* list;
  const u64* counts;
  double* sim;
  int64_t* index;
};

// the whole workgroup sorts the n <= FK_FALLBACK_CAP buffered entries' best k to the front
__device__ inline void fb_merge(double* bs, int* bi, int* cntp, double* ths, int* thi, int k, int tid) {
  constexpr int PER = FK_FALLBACK_CAP / FK_THREADS;
  const int n = *cntp;
  double es[PER];
  int ei[PER], rk[PER];
#pragma unroll
  for (int m = 0; m < PER; ++m) {
    const int p = tid + m * FK_THREADS;
    es[m] = p < n ? bs[p] : 0.0;
    ei[m] = p < n ? bi[p] : 0;
    rk[m] = 0;
  }
  for (int f = 0; f < n; ++f) {
    const double fs = bs[f];
    const int fi = bi[f];
#pragma unroll
    for (int m = 0; m < PER; ++m) rk[m] += better(fs, fi, es[m], ei[m]);
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; ++m) {
    if (tid + m * FK_THREADS < n && rk[m] < k) {
      bs[rk[m]] = es[m];
      bi[rk[m]] = ei[m];
      if (rk[m] == k - 1) {
        *ths = es[m];
        *thi = ei[m];
      }
    }
  }
  if (tid == 0) *cntp = n < k ? n : k;
  __syncthreads();
}

__global__ __launch_bounds__(FK_THREADS) void fk_fallback_kernel(const FkFallback a) {
  __shared__ double bs[FK_FALLBACK_CAP];
  __shared__ int bi[FK_FALLBACK_CAP];
  __shared__ double qv[GS_FKNN_MAX_E];
  __shared__ double ths;
  __shared__ int thi, cnt;
  const int tid = threadIdx.x;
  const int64_t listed = (int64_t)a.counts[1];
  for (int64_t li = blockIdx.x; li < listed; li += gridDim.x) {
    const int64_t q = a.list[li];
    __syncthreads();  // the previous row's readers are done
    for (int c = tid; c < a.e_pad; c += FK_THREADS) qv[c] = (double)a.xq[q * a.e_pad + c];
    if (tid == 0) {
      ths = -__builtin_inf();
      thi = 0x7fffffff;
      cnt = 0;
    }
    __syncthreads();
    for (int64_t base = 0; base < a.N; base += FK_THREADS) {
      const int64_t j = base + tid;
      if (j < a.N && !(a.self && j == q)) {
        const double s = fk_dot(qv, a.xd + j * a.e_pad, a.e_pad);
        if (better(s, (int)j, ths, thi)) {
          const int slot = atomicAdd(&cnt, 1);
          if (slot < FK_FALLBACK_CAP) {  // always: a step starts with <= FK_FALLBACK_CAP - 256 entries
            bs[slot] = s;
            bi[slot] = (int)j;
          }
        }
      }
      __syncthreads();
      const bool full = cnt > FK_FALLBACK_CAP - FK_THREADS;
      __syncthreads();  // everyone has read cnt before the next step adds to it
      if (full) fb_merge(bs, bi, &cnt, &ths, &thi, a.k, tid);
    }
    fb_merge(bs, bi, &cnt, &ths, &thi, a.k, tid);
    if (tid < a.k) {
      a.sim[q * a.k + tid] = tid < cnt ? bs[tid] : -__builtin_inf();
      a.index[q * a.k + tid] = tid < cnt ? bi[tid] : -1;
    }
  }
}

__global__ void fk_stats_kernel(const u64* counts, int64_t* stats) {
  if (threadIdx.x < 2) stats[threadIdx.x] = (int64_t)counts[threadIdx.x];
}

void prepare(hipStream_t s, int64_t rows, int E, int e_pad, int nks, const float* x, float* xh, u32x4* pc) {
  const int64_t tiles = fk_tiles(rows), rows_pad = tiles * FK_TILE, frags = tiles * nks * 64;
  hipLaunchKernelGGL(fk_normalize_kernel, dim3((unsigned)((rows_pad + 255) / 256)), dim3(256), 0, s, rows, rows_pad, E,
                     e_pad, x, xh);
  hipLaunchKernelGGL(fk_pieces_kernel, dim3((unsigned)((frags + 255) / 256)), dim3(256), 0, s, tiles, nks, e_pad, xh, pc);
}

template <int NKS>
void launch_scan(dim3 grid, hipStream_t s, const FkScan& k) {
  hipLaunchKernelGGL(fk_scan_kernel<NKS>, grid, dim3(FK_THREADS), 0, s, k);
}

}  // namespace

extern "C" int gs_feature_knn(const gs_feature_knn_args* g, gs_stream_t stream) {
  if (int rc = gs_feature_knn_validate(g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool self = !g->queries;
  const FeatureKnnLayout L(g->M, g->N, g->E, g->k, g->splits, self);
  void* ws = g->workspace;
  float* xh_d = at<float>(ws, L.off_xh_d);
  float* xh_q = at<float>(ws, L.off_xh_q);
  u32x4* pc_d = at<u32x4>(ws, L.off_pc_d);
  u32x4* pc_q = at<u32x4>(ws, L.off_pc_q);
  u64* counts = at<u64>(ws, L.off_counts);
  hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(u64), s);
  if (e != hipSuccess) return gs_set_error((int)e, "feature knn: %s", hipGetErrorString(e));
  prepare(s, g->N, g->E, L.e_pad, L.nks, g->feats, xh_d, pc_d);
  if (!self) prepare(s, g->M, g->E, L.e_pad, L.nks, g->queries, xh_q, pc_q);

  FkScan k;
  k.M = g->M; k.N = g->N; k.S = L.S; k.kp = L.kp; k.self = self;
  k.L = fk_chunk_rows(g->N, L.S); k.qtiles = L.qtiles;
  k.pq = pc_q; k.pd = pc_d;
  k.cand_s = at<float>(ws, L.off_cand_s); k.cand_i = at<int>(ws, L.off_cand_i);
  k.cnt = at<int>(ws, L.off_cnt); k.theta = at<float>(ws, L.off_theta);
  const dim3 grid((unsigned)fk_row_blocks(g->M), (unsigned)L.S);
  switch (L.nks) {
    case 1: launch_scan<1>(grid, s, k); break;
    case 2: launch_scan<2>(grid, s, k); break;
    case 3: launch_scan<3>(grid, s, k); break;
    case 4: launch_scan<4>(grid, s, k); break;
    case 5: launch_scan<5>(grid, s, k); break;
    case 6: launch_scan<6>(grid, s, k); break;
    case 7: launch_scan<7>(grid, s, k); break;
    default: launch_scan<8>(grid, s, k); break;
  }
  if (g->cand_sim) {
    const size_t n = (size_t)g->M * L.S;
    hipMemcpyAsync(g->cand_sim, k.cand_s, n * L.kp * sizeof(float), hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(g->cand_index, k.cand_i, n * L.kp * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(g->cand_count, k.cnt, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(g->cand_theta, k.theta, n * sizeof(float), hipMemcpyDeviceToDevice, s);
  }

  FkRerank r;
  r.M = g->M; r.S = L.S; r.k = g->k; r.kp = L.kp; r.e_pad = L.e_pad;
  r.bound = fk_bound(g->E);
  r.xq = xh_q; r.xd = xh_d;
  r.cand_s = k.cand_s; r.cand_i = k.cand_i; r.cnt = k.cnt; r.theta = k.theta;
  r.sim = g->sim; r.index = g->index;
  r.list = at<int>(ws, L.off_list); r.counts = counts;
  hipLaunchKernelGGL(fk_rerank_kernel, dim3((unsigned)g->M), dim3(64), 0, s, r);

  FkFallback f;
  f.N = g->N; f.k = g->k; f.e_pad = L.e_pad; f.self = self;
  f.xq = xh_q; f.xd = xh_d; f.list = r.list; f.counts = counts;
  f.sim = g->sim; f.index = g->index;
  hipLaunchKernelGGL(fk_fallback_kernel, dim3(FK_FALLBACK_GRID), dim3(FK_THREADS), 0, s, f);
  if (g->stats) hipLaunchKernelGGL(fk_stats_kernel, dim3(1), dim3(64), 0, s, counts, g->stats);
  return launch_status("feature knn", 0, s);
}
