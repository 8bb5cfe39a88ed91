// gs_feature_pca.hip -- feature-map PCA colouring (C ABI and arithmetic:
// include/gs_feature_pca.h): channel moments with the Gram matrix on the matrix
// cores, a one-workgroup fp64 eigensolve, and the project / offset / colour
// passes.
//
// Moments.  A workgroup of four waves owns one run of at most FP_CHUNK pixels of
// one image and walks it FP_PIX pixels per step.  A step stages the [C, 128]
// slice in LDS (coalesced plane reads), a thread per pixel forms x' in place
// (the norm over the channels, the shift, 0 off the fit set), and the waves
// contract over the pixels: the operand fragment of channel tile t for a k-step
// of 16 pixels is lane (r, hh) <- x'[32 t + r][16 ks + 8 hh + 0..7], the same
// registers whether the tile's rows or its columns are meant, so a diagonal
// tile passes one split as both operands.  C <= 32: one tile, the waves take
// two k-steps each and their accumulators are summed through LDS in wave order
// at the end.  C > 32: the upper-triangle tiles are dealt out over the waves
// (tile q to wave q mod 4), each wave walking all eight k-steps for its tiles.
// S is a fixed-order row sum over the same LDS image (2 to 8 threads a channel).
// Every thread loads its share of the next step's slice into registers before
// the block works on the current one.
// A block writes one slab; two finishing launches add the slabs to the fp64
// state in slab order.  The shift pass is the same walk without the matrix
// product and with fp64 row sums.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_feature_pca.h"
#include "gs_feature_pca_layout.h"
#include "gs_launch.h"
#include "gs_split_mfma.h"
#include "gs_sym_eig.h"

using namespace gs;
using namespace gs::smf;

namespace {

struct FpArgs {
  int C, mask_per_image, normalize, stride;
  int64_t hw;
  const float* x;
  const uint8_t* mask;
  const float* shift;
  float* slabs;      // GRAM: [slabs][C*C + C + 1]
  double* partials;  // shift pass: [slabs][C + 1]
};

__device__ inline int acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

__device__ inline void lds8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// the q-th tile of the upper triangle of an NT x NT tile grid, row by row
template <int NT>
__device__ inline void tile_of(int q, int& ti, int& tj) {
  ti = 0;
  int rem = q;
#pragma unroll
  for (int i = 0; i < NT; ++i)
    if (ti == i && rem >= NT - i) {  // row i holds NT - i tiles
      rem -= NT - i;
      ti = i + 1;
    }
  tj = ti + rem;
}

// NT: channel tiles of 32.  GRAM: the moments pass; else the shift pass.
template <int NT, bool GRAM>
__global__ __launch_bounds__(FP_THREADS) void fp_moments_kernel(const FpArgs a) {
  constexpr int NTILES = NT * (NT + 1) / 2;
  constexpr int TPW = NT == 1 ? 1 : (NTILES + FP_WAVES - 1) / FP_WAVES;
  constexpr int TPC = NT == 1 ? 8 : (NT == 2 ? 4 : 2);  // threads per channel of the S pass
  __shared__ __align__(16) float xl[32 * NT][FP_LD];
  __shared__ float sh[32 * NT];
  __shared__ int cl[FP_PIX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int b = blockIdx.y, C = a.C;
  const int64_t hw = a.hw, begin = (int64_t)blockIdx.x * FP_CHUNK;
  const float* xb = a.x + (int64_t)b * C * hw;
  const uint8_t* mb = a.mask ? a.mask + (a.mask_per_image ? (int64_t)b * hw : 0) : nullptr;
  if (tid < 32 * NT) sh[tid] = GRAM && tid < C ? a.shift[tid] : 0.f;

  f32x16 acc[GRAM ? TPW : 1];
#pragma unroll
  for (int t = 0; t < (GRAM ? TPW : 1); ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  float s32 = 0.f;
  double s64 = 0.0;
  int cnt = 0;
  const int col = tid & (FP_PIX - 1), half = tid >> 7;

  // this thread's 16 NT values of a step's slice and its pixel's fit-set flag, loaded one step
  // ahead: the next slice is in flight while the block works on the current one
  float nx[16 * NT];
  bool npart;
  auto fetch = [&](int64_t p) {
#pragma unroll
    for (int i = 0; i < 16 * NT; ++i) {
      const int f = half + 2 * i;
      nx[i] = f < C && p < hw ? xb[(int64_t)f * hw + p] : 0.f;
    }
    npart = p < hw && (!mb || mb[p] != 0) && (uint32_t)p % (uint32_t)a.stride == 0;
  };
  fetch(begin + col);

  for (int step = 0; step < FP_STEPS; ++step) {
    const int64_t p0 = begin + (int64_t)step * FP_PIX;
    if (p0 >= hw) break;  // uniform over the block
    __syncthreads();  // the previous step's readers of xl are done (and sh is written)
#pragma unroll
    for (int i = 0; i < 16 * NT; ++i) xl[half + 2 * i][col] = nx[i];
    const bool part = npart;
    if (step + 1 < FP_STEPS && p0 + FP_PIX < hw) fetch(p0 + FP_PIX + col);  // uniform over the block
    __syncthreads();
    float den = 1.f;
    if (a.normalize) {
      float ss = 0.f;
      for (int c = 0; c < C; ++c) ss += xl[c][col] * xl[c][col];
      den = fmaxf(sqrtf(ss), 1e-12f);
      __syncthreads();  // both halves have read the column before either rewrites it
    }
    for (int c = half; c < C; c += FP_THREADS / FP_PIX) {
      const float v = xl[c][col];
      const float xh = a.normalize ? v / den : v;
      xl[c][col] = part ? xh - sh[c] : 0.f;
    }
    if (half == 0) cnt += part ? 1 : 0;
    __syncthreads();

    {  // S: TPC threads a channel, each its run of pixels in ascending order, then a butterfly
      const int c = tid / TPC, sub = tid % TPC;
      if (c < 32 * NT) {  // whole waves
        float s = 0.f;
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < FP_PIX / TPC / 8; ++q) {
          float v[8];
          lds8(&xl[c][FP_PIX / TPC * sub + 8 * q], v);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (GRAM) s += v[j];
            else d += (double)v[j];
          }
        }
#pragma unroll
        for (int o = 1; o < TPC; o <<= 1) {
          if (GRAM) s += __shfl_xor(s, o);
          else d += __shfl_xor(d, o);
        }
        if (GRAM) s32 += s;
        else s64 += d;
      }
    }
    if (GRAM) {
      if (NT == 1) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          float v[8];
          lds8(&xl[r][16 * (2 * wave + kk) + 8 * hh], v);
          bsplit X;
          split_bf16(v, X);
          acc[0] = mfma_split(X, X, acc[0]);
        }
      } else {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int q = wave + FP_WAVES * t;
          if (q < NTILES) {  // uniform over the wave
            int ti, tj;
            tile_of<NT>(q, ti, tj);
#pragma unroll 2
            for (int ks = 0; ks < FP_PIX / 16; ++ks) {
              float v[8];
              bsplit X;
              lds8(&xl[32 * ti + r][16 * ks + 8 * hh], v);
              split_bf16(v, X);
              if (ti == tj) {
                acc[t] = mfma_split(X, X, acc[t]);
              } else {
                bsplit Y;
                lds8(&xl[32 * tj + r][16 * ks + 8 * hh], v);
                split_bf16(v, Y);
                acc[t] = mfma_split(X, Y, acc[t]);
              }
            }
          }
        }
      }
    }
  }

  const int64_t slab_id = (int64_t)b * gridDim.x + blockIdx.x;
  __syncthreads();
  if (half == 0) cl[col] = cnt;
  if (GRAM) {
    float* slab = a.slabs + slab_id * ((int64_t)C * C + C + 1);
    if (NT == 1) {
      float* red = &xl[0][0];  // [4][32][32] floats of the 32 x 132
#pragma unroll
      for (int i = 0; i < 16; ++i) red[(wave * 32 + acc_row(i, hh)) * 32 + r] = acc[0][i];
      __syncthreads();
      for (int e = tid; e < 1024; e += FP_THREADS) {
        const int row = e >> 5, cc = e & 31;
        const float s = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
        if (row < C && cc < C) slab[row * C + cc] = s;
      }
    } else {
      __syncthreads();
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int q = wave + FP_WAVES * t;
        if (q < NTILES) {
          int ti, tj;
          tile_of<NT>(q, ti, tj);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int row = 32 * ti + acc_row(i, hh), cc = 32 * tj + r;
            if (row < C && cc < C) slab[row * C + cc] = acc[t][i];
          }
        }
      }
    }
    if (tid % TPC == 0 && tid / TPC < C) slab[C * C + tid / TPC] = s32;
    if (tid == 0) {
      int n = 0;
      for (int i = 0; i < FP_PIX; ++i) n += cl[i];
      slab[C * C + C] = (float)n;  // <= FP_CHUNK, exact
    }
  } else {
    __syncthreads();
    double* part = a.partials + slab_id * (C + 1);
    if (tid % TPC == 0 && tid / TPC < C) part[tid / TPC] = s64;
    if (tid == 0) {
      int n = 0;
      for (int i = 0; i < FP_PIX; ++i) n += cl[i];
      part[C] = (double)n;
    }
  }
}

// out[g][e] = sum of in[s][e] over the slabs s of group g, in slab order, fp64.  C > 0: the
// elements are a moments slab, whose entries below the diagonal no block need have written
// (M[i][j] is taken from the upper entry): they are neither read nor written here.
template <class T>
__global__ void fp_group_sum_kernel(int64_t slabs, int64_t elems, int C, const T* in, double* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= elems) return;
  if (C > 0 && e < (int64_t)C * C && e / C > e % C) return;
  const int64_t s0 = (int64_t)blockIdx.y * FP_GROUP;
  double s = 0.0;
  for (int k = 0; k < FP_GROUP; ++k)
    if (s0 + k < slabs) s += (double)in[(s0 + k) * elems + e];
  out[(int64_t)blockIdx.y * elems + e] = s;
}

// state += the groups in group order; M[i][j] and M[j][i] from the upper entry
__global__ void fp_state_add_kernel(int C, int64_t groups, const double* g, double* state) {
  const int64_t elems = (int64_t)C * C + C + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= elems) return;
  int64_t src = e, dst;
  if (e < (int64_t)C * C) {
    const int i = (int)(e / C), j = (int)(e % C);
    src = i <= j ? e : (int64_t)j * C + i;
    dst = 1 + C + e;
  } else if (e < (int64_t)C * C + C) {
    dst = 1 + (e - (int64_t)C * C);
  } else {
    dst = 0;
  }
  double s = 0.0;
  for (int64_t k = 0; k < groups; ++k) s += g[k * elems + src];
  state[dst] += s;
}

// shift[c] = fl32(sum xh[c] / n) from the shift pass's groups
__global__ void fp_shift_kernel(int C, int64_t groups, const double* g, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, n = 0.0;
  for (int64_t k = 0; k < groups; ++k) {
    s += g[k * (C + 1) + c];
    n += g[k * (C + 1) + C];
  }
  shift[c] = n > 0.0 ? (float)(s / n) : 0.f;
}

// mean and one covariance entry from the state
__device__ inline double fp_mean(const double* state, const float* shift, int c) {
  const double n = state[0];
  return (double)shift[c] + (n > 0.0 ? state[1 + c] / n : 0.0);
}
__device__ inline double fp_cov(const double* state, int C, int ddof, int i, int j) {
  const double n = state[0];
  if (!(n > (double)ddof)) return 0.0;
  const double di = state[1 + i] / n, dj = state[1 + j] / n;
  return (state[1 + C + (int64_t)i * C + j] - (n * di) * dj) / (n - (double)ddof);
}

__global__ void fp_cov_kernel(int C, int ddof, const double* state, const float* shift, double* mean, double* cov) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C * C) return;
  cov[e] = fp_cov(state, C, ddof, e / C, e % C);
  if (e < C) mean[e] = fp_mean(state, shift, e);
}

// One workgroup.  LDS: A and V live in `lds`; else in the workspace.
template <bool LDS>
__global__ __launch_bounds__(FP_EIG_THREADS) void fp_fit_kernel(int C, int k, int ddof, const double* state,
                                                                const float* shift, double* ws, double* mean,
                                                                float* mean_f32, double* evals, double* evecs,
                                                                double* components, float* components_f32,
                                                                int32_t* status) {
  constexpr int NE = LDS ? FP_EIG_LDS_ORDER : 2;
  __shared__ double lds[2 * NE * (NE + 1)];
  __shared__ double rot[3 * GS_FPCA_MAX_C / 2];
  __shared__ double red[2 * FP_EIG_THREADS];
  __shared__ int pq[GS_FPCA_MAX_C];
  const int tid = threadIdx.x, ne = fp_even(C), ld = fp_eig_ld(C);
  double* A = LDS ? lds : ws;
  double* V = A + ne * ld;
  const bool empty = !(state[0] > (double)ddof);
  for (int c = tid; c < C; c += FP_EIG_THREADS) {
    const double m = fp_mean(state, shift, c);
    mean[c] = m;
    mean_f32[c] = (float)m;
  }
  for (int e = tid; e < ne * ne; e += FP_EIG_THREADS) {
    const int i = e / ne, j = e % ne;
    A[i * ld + j] = i < C && j < C ? fp_cov(state, C, ddof, i, j) : 0.0;
  }
  __syncthreads();
  SymEigScratch w{rot, pq, red, 0};
  int sweeps = 0;
  if (!empty) sweeps = sym_eig_jacobi(ne, A, V, ld, w, GS_FPCA_MAX_SWEEPS, tid, FP_EIG_THREADS);  // uniform branch
  const int st = empty ? 1 : (sweeps == SYM_EIG_NOT_FINITE ? 3 : (sweeps < 0 ? 2 : 0));
  sym_eig_sorted(C, A, V, ld, w, evals, evecs, st == 1 || st == 3, tid, FP_EIG_THREADS);
  for (int e = tid; e < k * C; e += FP_EIG_THREADS) {
    const double v = st ? 0.0 : evecs[e];  // this thread's own writes or a synchronised one's
    components[e] = v;
    components_f32[e] = (float)v;
  }
  if (tid == 0) *status = st;
}

struct FpProjArgs {
  int C, k, mask_per_image, normalize, gx;
  int64_t hw;
  const float *x, *comp, *mean;
  const uint8_t* mask;
  float *t, *partials;
};

template <int K>
__global__ __launch_bounds__(FP_PROJ_PIX) void fp_project_kernel(const FpProjArgs a) {
  __shared__ float vl[GS_FPCA_MAX_K * GS_FPCA_MAX_C];
  __shared__ float ml[GS_FPCA_MAX_C];
  __shared__ float rl[FP_PROJ_PIX / 64][GS_FPCA_MAX_K][2];
  const int tid = threadIdx.x, b = blockIdx.y, C = a.C;
  constexpr int k = K;
  for (int e = tid; e < k * C; e += FP_PROJ_PIX) vl[e] = a.comp[e];
  for (int e = tid; e < C; e += FP_PROJ_PIX) ml[e] = a.mean[e];
  __syncthreads();
  const int64_t hw = a.hw, p = (int64_t)blockIdx.x * FP_PROJ_PIX + tid;
  const float* xb = a.x + (int64_t)b * C * hw;
  const uint8_t* mb = a.mask ? a.mask + (a.mask_per_image ? (int64_t)b * hw : 0) : nullptr;
  const bool in = p < hw, part = in && (!mb || mb[p] != 0);
  float t[K];
#pragma unroll
  for (int j = 0; j < K; ++j) t[j] = 0.f;
  if (part) {
    float den = 1.f;
    if (a.normalize) {
      float ss = 0.f;
      for (int c0 = 0; c0 < C; c0 += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = c0 + i < C ? xb[(int64_t)(c0 + i) * hw + p] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) ss += v[i] * v[i];  // the padding adds +0
      }
      den = fmaxf(sqrtf(ss), 1e-12f);
    }
    for (int c0 = 0; c0 < C; c0 += 8) {  // eight planes in flight, added in channel order
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = c0 + i < C ? xb[(int64_t)(c0 + i) * hw + p] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = c0 + i;
        if (c < C) {
          const float d = (a.normalize ? v[i] / den : v[i]) - ml[c];
#pragma unroll
          for (int j = 0; j < K; ++j) t[j] += d * vl[j * C + c];
        }
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (in) a.t[((int64_t)b * k + j) * hw + p] = t[j];
    float lo = part ? t[j] : INFINITY, hi = part ? t[j] : -INFINITY;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o));
      hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) {
      rl[wave][j][0] = lo;
      rl[wave][j][1] = hi;
    }
  }
  __syncthreads();
  if (tid < k) {
    float lo = rl[0][tid][0], hi = rl[0][tid][1];
    for (int wv = 1; wv < FP_PROJ_PIX / 64; ++wv) {
      lo = fminf(lo, rl[wv][tid][0]);
      hi = fmaxf(hi, rl[wv][tid][1]);
    }
    float* o = a.partials + (((int64_t)b * a.gx + blockIdx.x) * k + tid) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

// tmin, tmax [B, k] from the blocks' partials: a workgroup per (image, component), every thread
// its partials in block order, then the threads in thread order; 0 / 0 for no pixel
__global__ __launch_bounds__(FP_PROJ_PIX) void fp_range_kernel(int k, int gx, const float* partials, float* tmin,
                                                              float* tmax) {
  __shared__ float rl[FP_PROJ_PIX][2];
  const int e = blockIdx.x, b = e / k, j = e % k, tid = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < gx; i += FP_PROJ_PIX) {
    const float* o = partials + (((int64_t)b * gx + i) * k + j) * 2;
    lo = fminf(lo, o[0]);
    hi = fmaxf(hi, o[1]);
  }
  rl[tid][0] = lo;
  rl[tid][1] = hi;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < FP_PROJ_PIX; ++i) {
    lo = fminf(lo, rl[i][0]);
    hi = fmaxf(hi, rl[i][1]);
  }
  const bool none = lo > hi;
  tmin[e] = none ? 0.f : lo;
  tmax[e] = none ? 0.f : hi;
}

__global__ __launch_bounds__(FP_PROJ_PIX) void fp_offset_kernel(int64_t hw, const float* t, const float* sub, float* u) {
  const int64_t p = (int64_t)blockIdx.x * FP_PROJ_PIX + threadIdx.x;
  if (p >= hw) return;
  const int64_t o = (int64_t)blockIdx.y * hw + p;
  u[o] = t[o] - sub[blockIdx.y];
}

__global__ __launch_bounds__(FP_PROJ_PIX) void fp_colour_kernel(int64_t hw, int mask_per_image, int out_uint8, int clamp,
                                                               const float* t, const uint8_t* mask, const double* lo,
                                                               const double* hi, void* out) {
  const int64_t p = (int64_t)blockIdx.x * FP_PROJ_PIX + threadIdx.x;
  if (p >= hw) return;
  const int b = blockIdx.y;
  const uint8_t* mb = mask ? mask + (mask_per_image ? (int64_t)b * hw : 0) : nullptr;
  const bool part = !mb || mb[p] != 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double l = lo[b * 3 + j], h = hi[b * 3 + j];
    double v = 0.0;
    if (part && h != l) v = ((double)t[((int64_t)b * 3 + j) * hw + p] - l) / (h - l);
    if (clamp || out_uint8) v = v > 0.0 ? (v < 1.0 ? v : 1.0) : 0.0;  // NaN -> 0
    if (out_uint8) static_cast<uint8_t*>(out)[((int64_t)b * hw + p) * 3 + j] = (uint8_t)(int)(255.0 * v);
    else static_cast<float*>(out)[((int64_t)b * 3 + j) * hw + p] = (float)v;
  }
}

template <int NT, bool GRAM>
void launch_moments(dim3 grid, hipStream_t s, const FpArgs& k) {
  hipLaunchKernelGGL((fp_moments_kernel<NT, GRAM>), grid, dim3(FP_THREADS), 0, s, k);
}
template <bool GRAM>
void launch_moments_nt(int nt, dim3 grid, hipStream_t s, const FpArgs& k) {
  if (nt == 1) launch_moments<1, GRAM>(grid, s, k);
  else if (nt == 2) launch_moments<2, GRAM>(grid, s, k);
  else if (nt == 3) launch_moments<3, GRAM>(grid, s, k);
  else launch_moments<4, GRAM>(grid, s, k);
}

}  // namespace

extern "C" {

int gs_feature_pca_update(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_UPDATE)) return e;
  hipStream_t s = (hipStream_t)stream;
  const FeaturePcaUpdateLayout L(g->B, g->C, g->H, g->W);
  FpArgs k;
  k.C = g->C; k.mask_per_image = g->mask_per_image; k.normalize = g->normalize; k.stride = g->sample_stride;
  k.hw = (int64_t)g->H * g->W;
  k.x = g->x; k.mask = g->mask; k.shift = g->shift;
  k.slabs = at<float>(g->workspace, L.off_slabs);
  k.partials = at<double>(g->workspace, L.off_mean);
  const int nt = fp_channel_tiles(g->C);
  const dim3 grid((unsigned)L.chunks, (unsigned)g->B);
  if (g->compute_shift) {
    const int64_t e = g->C + 1;
    double* mg = at<double>(g->workspace, L.off_mean_groups);
    launch_moments_nt<false>(nt, grid, s, k);
    hipLaunchKernelGGL((fp_group_sum_kernel<double>), dim3((unsigned)((e + 255) / 256), (unsigned)L.groups), dim3(256),
                       0, s, L.slabs, e, 0, k.partials, mg);
    hipLaunchKernelGGL(fp_shift_kernel, dim3((g->C + 127) / 128), dim3(128), 0, s, g->C, L.groups, mg, g->shift);
  }
  double* gs = at<double>(g->workspace, L.off_groups);
  launch_moments_nt<true>(nt, grid, s, k);
  hipLaunchKernelGGL((fp_group_sum_kernel<float>), dim3((unsigned)((L.slab_elems + 255) / 256), (unsigned)L.groups),
                     dim3(256), 0, s, L.slabs, L.slab_elems, g->C, k.slabs, gs);
  hipLaunchKernelGGL(fp_state_add_kernel, dim3((unsigned)((L.slab_elems + 255) / 256)), dim3(256), 0, s, g->C, L.groups,
                     gs, g->state);
  return launch_status("feature pca update", 0, s);
}

int gs_feature_pca_covariance(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_COVARIANCE)) return e;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fp_cov_kernel, dim3((g->C * g->C + 255) / 256), dim3(256), 0, s, g->C, g->ddof, g->state, g->shift,
                     g->mean, g->cov);
  return launch_status("feature pca covariance", 0, s);
}

int gs_feature_pca_fit(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_FIT)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (g->C <= FP_EIG_LDS_ORDER)
    hipLaunchKernelGGL((fp_fit_kernel<true>), dim3(1), dim3(FP_EIG_THREADS), 0, s, g->C, g->k, g->ddof, g->state, g->shift,
                       static_cast<double*>(nullptr), g->mean, g->mean_f32, g->evals, g->evecs, g->components,
                       g->components_f32, g->status);
  else
    hipLaunchKernelGGL((fp_fit_kernel<false>), dim3(1), dim3(FP_EIG_THREADS), 0, s, g->C, g->k, g->ddof, g->state,
                       g->shift, static_cast<double*>(g->workspace), g->mean, g->mean_f32, g->evals, g->evecs,
                       g->components, g->components_f32, g->status);
  return launch_status("feature pca fit", 0, s);
}

int gs_feature_pca_project(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_PROJECT)) return e;
  hipStream_t s = (hipStream_t)stream;
  FpProjArgs k;
  k.C = g->C; k.k = g->k; k.mask_per_image = g->mask_per_image; k.normalize = g->normalize;
  k.gx = (int)fp_proj_blocks(g->H, g->W);
  k.hw = (int64_t)g->H * g->W;
  k.x = g->x; k.comp = g->proj_components; k.mean = g->proj_mean; k.mask = g->mask;
  k.t = g->t; k.partials = static_cast<float*>(g->workspace);
  const dim3 grid((unsigned)k.gx, (unsigned)g->B);
  switch (g->k) {
    case 1: hipLaunchKernelGGL(fp_project_kernel<1>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 2: hipLaunchKernelGGL(fp_project_kernel<2>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 3: hipLaunchKernelGGL(fp_project_kernel<3>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 4: hipLaunchKernelGGL(fp_project_kernel<4>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 5: hipLaunchKernelGGL(fp_project_kernel<5>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 6: hipLaunchKernelGGL(fp_project_kernel<6>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    case 7: hipLaunchKernelGGL(fp_project_kernel<7>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
    default: hipLaunchKernelGGL(fp_project_kernel<8>, grid, dim3(FP_PROJ_PIX), 0, s, k); break;
  }
  hipLaunchKernelGGL(fp_range_kernel, dim3((unsigned)(g->B * g->k)), dim3(FP_PROJ_PIX), 0, s, g->k, k.gx, k.partials,
                     g->tmin, g->tmax);
  return launch_status("feature pca project", 0, s);
}

int gs_feature_pca_offset(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_OFFSET)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = (int64_t)g->H * g->W;
  // planes (b, j) on y, in rows of at most 65535
  const int64_t planes = (int64_t)g->B * g->k;
  for (int64_t y0 = 0; y0 < planes; y0 += 65535) {
    const int64_t ny = planes - y0 < 65535 ? planes - y0 : 65535;
    hipLaunchKernelGGL(fp_offset_kernel, dim3((unsigned)fp_proj_blocks(g->H, g->W), (unsigned)ny), dim3(FP_PROJ_PIX), 0,
                       s, hw, g->t + y0 * hw, g->sub + y0, g->u + y0 * hw);
  }
  return launch_status("feature pca offset", 0, s);
}

int gs_feature_pca_colour(const gs_feature_pca* g, gs_stream_t stream) {
  if (int e = gs_feature_pca_validate(g, GS_FPCA_PASS_COLOUR)) return e;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fp_colour_kernel, dim3((unsigned)fp_proj_blocks(g->H, g->W), (unsigned)g->B), dim3(FP_PROJ_PIX), 0,
                     s, (int64_t)g->H * g->W, g->mask_per_image, g->out_uint8, g->clamp, g->t, g->mask, g->lo, g->hi,
                     g->out);
  return launch_status("feature pca colour", 0, s);
}

}  // extern "C"
