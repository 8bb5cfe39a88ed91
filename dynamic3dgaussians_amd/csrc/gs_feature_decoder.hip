// gs_feature_decoder.hip -- the fused 1x1 feature decoder and its L1 loss on
// the matrix cores (C ABI and arithmetic: include/gs_feature_decoder.h).
//
// One tile body for all four passes.  A workgroup of four waves takes 128
// consecutive pixels of one camera per step, a wave 32 of them: the pixel is
// on the lane (lane & 31), the rows of a 32-row tile of output channels are in
// the 16 accumulator registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)),
// so every register is a coalesced row segment of y / target / d_y.
//
//   W x        A = W's fragments (split once per call by fd_prep_kernel, in
//              operand order, read from the workspace), B = x from the LDS
//              image of the step's [F_in, 128] slice, split once per step.
//              Six piece products per k-step of 16.
//   S          sign((acc + bias) - target) in registers (loss backward), or
//              d_y loaded into the same layout (plain backward).
//   W^T S      sums over S's row index: the accumulator registers 8s .. 8s+7
//              are the B fragment of k-step s with no lane movement; W^T's
//              fragments are built in that permuted k order (element j of lane
//              half hh is row 16 s + 8 (j >> 2) + 4 hh + (j & 3)).  Three piece
//              products per k-step for the sign tile (exact in bf16), six for
//              d_y.
//   S (m x)^T  sums over S's lane index: S goes through LDS once ([row][pixel]
//              floats), and the wave that owns the row tile (ct mod 4) reads
//              it back as the A fragment against B = m x from the LDS image of
//              x.  Its d_W tiles stay in registers over the block's whole walk
//              (<= 16384 floats per block); d_b is a fixed-order sum over the
//              same LDS rows.
//
// Every block writes one slab, the loss pass one fp64 partial; a finishing
// launch sums them in fp64 in index order.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_feature_decoder.h"
#include "gs_feature_decoder_layout.h"
#include "gs_launch.h"
#include "gs_split_mfma.h"

using namespace gs;
using namespace gs::smf;

namespace {

struct FdArgs {
  int B, F_in, C_out, nct, gx, mask_per_camera;
  int64_t hw, tiles;
  const float *x, *bias, *target, *mask, *up, *d_y;
  float *y, *d_x;
  const u32x4 *wf, *wt;
  double* partials;
  float* slabs;
  int64_t slab_floats;
};

__device__ inline int acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// W's bf16 pieces in operand order, once per call: thread = (fragment, lane).
//   wf[(ct * 2 nft + ks) * 3 + piece][lane]: W[32 ct + r][16 ks + 8 hh + j]
//   wt[((ct * 2 + s) * nft + ft) * 3 + piece][lane]:
//       W[32 ct + 16 s + 8 (j >> 2) + 4 hh + (j & 3)][32 ft + r]
__global__ __launch_bounds__(FD_THREADS) void fd_prep_kernel(int F_in, int C_out, int nct, int nft, const float* W,
                                                             u32x4* wf, u32x4* wt) {
  const int idx = blockIdx.x * FD_THREADS + threadIdx.x;
  if (idx >= nct * 2 * nft * 64) return;
  const int lane = idx & 63, frag = idx >> 6, r = lane & 31, hh = lane >> 5;
  float v[8];
  bsplit s;
  if (wf) {
    const int ct = frag / (2 * nft), ks = frag % (2 * nft), c = 32 * ct + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = 16 * ks + 8 * hh + j;
      v[j] = c < C_out && f < F_in ? W[c * F_in + f] : 0.f;
    }
    split_bf16(v, s);
#pragma unroll
    for (int i = 0; i < NSP; ++i) wf[(frag * NSP + i) * 64 + lane] = __builtin_bit_cast(u32x4, s.p[i]);
  }
  if (wt) {
    const int ft = frag % nft, sk = (frag / nft) % 2, ct = frag / (2 * nft), f = 32 * ft + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 32 * ct + 16 * sk + 8 * (j >> 2) + 4 * hh + (j & 3);
      v[j] = c < C_out && f < F_in ? W[c * F_in + f] : 0.f;
    }
    split_bf16(v, s);
#pragma unroll
    for (int i = 0; i < NSP; ++i) wt[(frag * NSP + i) * 64 + lane] = __builtin_bit_cast(u32x4, s.p[i]);
  }
}

__device__ inline void load_frag(const u32x4* base, int frag, int lane, bsplit& s) {
#pragma unroll
  for (int i = 0; i < NSP; ++i) s.p[i] = __builtin_bit_cast(bf16x8, base[(frag * NSP + i) * 64 + lane]);
}

__device__ inline void lds8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

constexpr int MODE_DECODE = GS_FD_PASS_DECODE, MODE_LOSS = GS_FD_PASS_LOSS, MODE_SIGN = GS_FD_PASS_LOSS_BACKWARD,
              MODE_UP = GS_FD_PASS_BACKWARD;

// NFT: f-tiles of 32 (k of W x padded to 32 NFT); NCT4: ceil(row tiles / 4),
// the row tiles a wave owns in the backward.
template <int MODE, int NFT, int NCT4>
__global__ __launch_bounds__(FD_THREADS) void fd_kernel(const FdArgs a) {
  constexpr bool BWD = MODE == MODE_SIGN || MODE == MODE_UP;
  constexpr bool PRODUCT = MODE != MODE_UP;  // W x is formed
  constexpr int NKS = 2 * NFT;
  __shared__ __align__(16) float xl[32 * NFT][FD_LD];
  __shared__ __align__(16) float sl[BWD ? FD_ROWS : 1][FD_LD];
  __shared__ __align__(16) float ml[FD_PIX];
  __shared__ double red[MODE == MODE_LOSS ? FD_THREADS : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int b = blockIdx.y;
  const int64_t hw = a.hw;
  float scale = 1.f;
  if (MODE == MODE_SIGN) scale = a.up[b] / (float)((int64_t)a.C_out * hw);
  const float* xb = a.x + (int64_t)b * a.F_in * hw;
  const float* mb = a.mask ? a.mask + (a.mask_per_camera ? (int64_t)b * hw : 0) : nullptr;

  f32x16 dW[BWD ? NCT4 : 1][NFT];
  float db[BWD ? NCT4 : 1];
#pragma unroll
  for (int q = 0; q < (BWD ? NCT4 : 1); ++q) {
    db[q] = 0.f;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
      for (int i = 0; i < 16; ++i) dW[q][ft][i] = 0.f;
  }
  double dsum = 0.0;

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += a.gx) {
    const int64_t p0 = tile * FD_PIX;
    __syncthreads();  // the previous step's readers of xl, ml and sl are done
    {
      const int64_t p = p0 + (tid & (FD_PIX - 1));
      for (int f = tid >> 7; f < 32 * NFT; f += FD_THREADS / FD_PIX)
        xl[f][tid & (FD_PIX - 1)] = f < a.F_in && p < hw ? xb[(int64_t)f * hw + p] : 0.f;
      if (tid < FD_PIX) ml[tid] = p < hw ? (mb ? mb[p] : 1.f) : 0.f;
    }
    __syncthreads();
    const int col = 32 * wave + r;
    const int64_t px = p0 + col;
    const bool pin = px < hw;
    const float mpx = ml[col];

    bsplit xp[PRODUCT ? NKS : 1];
    if (PRODUCT) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xl[16 * ks + 8 * hh + j][col];
        split_bf16(v, xp[ks]);
      }
    }
    f32x16 dx[BWD ? NFT : 1];
#pragma unroll
    for (int ft = 0; ft < (BWD ? NFT : 1); ++ft)
#pragma unroll
      for (int i = 0; i < 16; ++i) dx[ft][i] = 0.f;
    float lsum = 0.f;

    // backward: ct = 4 ct4 + wq with ct4 unrolled (the owner's d_W tiles are registers); the
    // forward passes keep nothing per row tile and walk ct in one rolled loop
    const int inner = BWD ? FD_WAVES : a.nct;
#pragma unroll
    for (int ct4 = 0; ct4 < (BWD ? NCT4 : 1); ++ct4) {
#pragma unroll 1
      for (int wq = 0; wq < inner; ++wq) {
        const int ct = FD_WAVES * ct4 + wq;
        if (ct >= a.nct) break;  // uniform over the block
        f32x16 S;
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = 0.f;
        if (PRODUCT) {
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks) {
            bsplit A;
            load_frag(a.wf, ct * NKS + ks, lane, A);
            S = mfma_split(A, xp[ks], S);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int c = 32 * ct + acc_row(i, hh);
          const bool in = c < a.C_out && pin;
          const int64_t o = ((int64_t)b * a.C_out + c) * hw + px;
          if (MODE == MODE_UP) {
            S[i] = in ? a.d_y[o] : 0.f;
          } else {
            const float y = S[i] + (a.bias && c < a.C_out ? a.bias[c] : 0.f);
            if (MODE == MODE_DECODE) {
              if (in) a.y[o] = y;
            } else {
              const float res = y - (in ? a.target[o] : 0.f);
              if (MODE == MODE_LOSS) lsum += mpx * fabsf(res);
              else S[i] = res > 0.f ? 1.f : (res < 0.f ? -1.f : 0.f);
            }
          }
        }
        if (BWD) {
          // d_x += W^T S: S's registers are the B fragments
#pragma unroll
          for (int sk = 0; sk < 2; ++sk) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = S[8 * sk + j];
            if (MODE == MODE_SIGN) {
              const bf16x8 sb = pack_exact(v);
#pragma unroll
              for (int ft = 0; ft < NFT; ++ft) {
                bsplit A;
                load_frag(a.wt, (ct * 2 + sk) * NFT + ft, lane, A);
                dx[ft] = mfma_split_exact(A, sb, dx[ft]);
              }
            } else {
              bsplit sb;
              split_bf16(v, sb);
#pragma unroll
              for (int ft = 0; ft < NFT; ++ft) {
                bsplit A;
                load_frag(a.wt, (ct * 2 + sk) * NFT + ft, lane, A);
                dx[ft] = mfma_split(A, sb, dx[ft]);
              }
            }
          }
          // d_W, d_b += S (m x)^T: S through LDS, the row tile's owner reads it back
          __syncthreads();  // the previous round's owner is done with sl
#pragma unroll
          for (int i = 0; i < 16; ++i) sl[acc_row(i, hh)][col] = S[i];
          __syncthreads();
          if (wave == wq) {
#pragma unroll 2
            for (int kk = 0; kk < FD_PIX / 16; ++kk) {
              const int k0 = 16 * kk + 8 * hh;
              float sa[8], m8[8];
              lds8(&sl[r][k0], sa);
              lds8(&ml[k0], m8);
              bf16x8 Ae;
              bsplit As;
              if (MODE == MODE_SIGN) Ae = pack_exact(sa);
              else split_bf16(sa, As);
#pragma unroll
              for (int ft = 0; ft < NFT; ++ft) {
                float xm[8];
                lds8(&xl[32 * ft + r][k0], xm);
#pragma unroll
                for (int j = 0; j < 8; ++j) xm[j] = xm[j] * m8[j];
                bsplit Bx;
                split_bf16(xm, Bx);
                if (MODE == MODE_SIGN) dW[ct4][ft] = mfma_exact_split(Ae, Bx, dW[ct4][ft]);
                else dW[ct4][ft] = mfma_split(As, Bx, dW[ct4][ft]);
              }
            }
            float sdb = 0.f;  // this half's 64 pixels in ascending order
            for (int q = 0; q < FD_PIX / 16; ++q) {
              float sa[8], m8[8];
              lds8(&sl[r][64 * hh + 8 * q], sa);
              lds8(&ml[64 * hh + 8 * q], m8);
#pragma unroll
              for (int j = 0; j < 8; ++j) sdb += sa[j] * m8[j];
            }
            sdb += __shfl_xor(sdb, 32);
            db[ct4] += sdb;
          }
        }
      }
    }
    if (MODE == MODE_LOSS) dsum += (double)lsum;
    if (BWD) {
      const float sm = scale * mpx;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int f = 32 * ft + acc_row(i, hh);
          if (f < a.F_in && pin)
            a.d_x[((int64_t)b * a.F_in + f) * hw + px] = MODE == MODE_SIGN ? sm * dx[ft][i] : dx[ft][i];
        }
    }
  }

  if (MODE == MODE_LOSS) {
    red[tid] = dsum;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < FD_THREADS; ++i) s += red[i];
      a.partials[(int64_t)b * a.gx + blockIdx.x] = s;
    }
  }
  if (BWD) {
    float* slab = a.slabs + ((int64_t)b * a.gx + blockIdx.x) * a.slab_floats;
#pragma unroll
    for (int ct4 = 0; ct4 < NCT4; ++ct4) {
      const int ct = FD_WAVES * ct4 + wave;
      if (ct >= a.nct) continue;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int c = 32 * ct + acc_row(i, hh), f = 32 * ft + r;
          if (c < a.C_out && f < a.F_in) slab[c * a.F_in + f] = scale * dW[ct4][ft][i];
        }
      if (hh == 0 && 32 * ct + r < a.C_out) slab[a.C_out * a.F_in + 32 * ct + r] = scale * db[ct4];
    }
  }
}

// loss[b] = sum of the camera's partials in index order, fp64, over N
__global__ void fd_loss_finish_kernel(int B, int gx, double N, const double* partials, float* loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < gx; ++i) s += partials[(int64_t)b * gx + i];
  loss[b] = (float)(s / N);
}

// d_W, d_b = sum of the slabs in slab order, fp64
__global__ void fd_slab_reduce_kernel(int64_t slabs, int64_t slab_floats, int64_t CF, const float* slab, float* d_W,
                                      float* d_b) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= slab_floats) return;
  double s = 0.0;
  for (int64_t k = 0; k < slabs; ++k) s += (double)slab[k * slab_floats + e];
  if (e < CF) d_W[e] = (float)s;
  else if (d_b) d_b[e - CF] = (float)s;
}

template <int MODE, int NFT>
void launch_nct4(int nct4, dim3 grid, hipStream_t s, const FdArgs& k) {
  constexpr bool BWD = MODE == MODE_SIGN || MODE == MODE_UP;
  if (!BWD || nct4 == 1) hipLaunchKernelGGL((fd_kernel<MODE, NFT, 1>), grid, dim3(FD_THREADS), 0, s, k);
  else if (nct4 == 2) hipLaunchKernelGGL((fd_kernel<MODE, NFT, BWD ? 2 : 1>), grid, dim3(FD_THREADS), 0, s, k);
  else if (nct4 == 3) hipLaunchKernelGGL((fd_kernel<MODE, NFT, BWD ? 3 : 1>), grid, dim3(FD_THREADS), 0, s, k);
  else hipLaunchKernelGGL((fd_kernel<MODE, NFT, BWD ? 4 : 1>), grid, dim3(FD_THREADS), 0, s, k);
}

template <int MODE>
int run(const gs_feature_decoder* g, gs_stream_t stream) {
  if (int e = gs_feature_decoder_validate(g, MODE)) return e;
  constexpr bool BWD = MODE == MODE_SIGN || MODE == MODE_UP;
  const FeatureDecoderLayout L(g->B, g->F_in, g->C_out, g->h, g->w, MODE);
  hipStream_t s = (hipStream_t)stream;
  FdArgs k;
  k.B = g->B; k.F_in = g->F_in; k.C_out = g->C_out;
  k.nct = fd_row_tiles(g->C_out);
  k.gx = (int)L.gx;
  k.mask_per_camera = g->mask_per_camera;
  k.hw = (int64_t)g->h * g->w;
  k.tiles = fd_tiles(g->h, g->w);
  k.x = g->x; k.bias = g->bias; k.target = g->target;
  k.mask = MODE == MODE_LOSS || MODE == MODE_SIGN ? g->mask : nullptr;
  k.up = g->up; k.d_y = g->d_y; k.y = g->y; k.d_x = g->d_x;
  u32x4* wf = MODE != MODE_UP ? at<u32x4>(g->workspace, L.off_wf) : nullptr;
  u32x4* wt = BWD ? at<u32x4>(g->workspace, L.off_wt) : nullptr;
  k.wf = wf; k.wt = wt;
  k.partials = MODE == MODE_LOSS ? at<double>(g->workspace, L.off_partials) : nullptr;
  k.slabs = BWD ? at<float>(g->workspace, L.off_slabs) : nullptr;
  k.slab_floats = (int64_t)L.slab_floats;
  const int nft = fd_f_tiles(g->F_in), nct4 = (k.nct + FD_WAVES - 1) / FD_WAVES;
  const int prep = k.nct * 2 * nft * 64;
  hipLaunchKernelGGL(fd_prep_kernel, dim3((prep + FD_THREADS - 1) / FD_THREADS), dim3(FD_THREADS), 0, s, g->F_in,
                     g->C_out, k.nct, nft, g->weight, wf, wt);
  const dim3 grid((unsigned)k.gx, (unsigned)g->B);
  if (nft == 1) launch_nct4<MODE, 1>(nct4, grid, s, k);
  else launch_nct4<MODE, 2>(nct4, grid, s, k);
  if (MODE == MODE_LOSS)
    hipLaunchKernelGGL(fd_loss_finish_kernel, dim3((g->B + 63) / 64), dim3(64), 0, s, g->B, k.gx,
                       (double)g->C_out * (double)k.hw, k.partials, g->loss);
  if (BWD)
    hipLaunchKernelGGL(fd_slab_reduce_kernel, dim3((unsigned)((L.slab_floats + 255) / 256)), dim3(256), 0, s,
                       (int64_t)L.slabs, (int64_t)L.slab_floats, (int64_t)g->C_out * g->F_in, k.slabs, g->d_weight,
                       g->d_bias);
  static const char* const WHAT[4] = {"feature decoder forward", "feature decoder loss forward",
                                      "feature decoder loss backward", "feature decoder backward"};
  return launch_status(WHAT[MODE], 0, s);
}

}  // namespace

extern "C" {

int gs_feature_decoder_forward(const gs_feature_decoder* args, gs_stream_t stream) {
  return run<MODE_DECODE>(args, stream);
}
int gs_feature_decoder_loss_forward(const gs_feature_decoder* args, gs_stream_t stream) {
  return run<MODE_LOSS>(args, stream);
}
int gs_feature_decoder_loss_backward(const gs_feature_decoder* args, gs_stream_t stream) {
  return run<MODE_SIGN>(args, stream);
}
int gs_feature_decoder_backward(const gs_feature_decoder* args, gs_stream_t stream) {
  return run<MODE_UP>(args, stream);
}

}  // extern "C"
