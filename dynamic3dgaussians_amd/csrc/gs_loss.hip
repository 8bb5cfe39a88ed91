// gs_loss.hip -- the fused photometric loss (L1 + SSIM) of the reference's
// training step (train.py:161-183; helpers.py:110-111; external.py:90-133),
// forward and backward, for a whole camera batch (C ABI: include/gs_loss.h).
//
// One workgroup of 256 threads owns one 32 x 32 tile of one (image, channel)
// plane.  Forward: the tile of x = (gain * image + offset) * mask and
// y = target * mask is staged in LDS with its 5-pixel halo (zero outside the
// image: the conv2d zero padding), the 11-tap window runs along the rows for
// the five maps x, y, xx, yy, xy (LDS to LDS) and down the columns (LDS to
// registers, four rows of one column per thread, each staged value feeding up
// to four outputs).  From the five window sums every pixel gets its SSIM
// value and the three derivative maps
//   P = d m / d mu1 (with the sigmas' dependence on mu1),
//   Q = d m / d (w * xx),   R = d m / d (w * xy),
// which are kept in the workspace.  Backward: the same two passes over P, Q, R
// (the window is symmetric, so the transposed convolution is the same one)
// give  d(sum m)/dx = w*P + 2 x w*Q + y w*R;  the L1 sign and the chain to
// image / gain / offset are applied in the same kernel.
//
// Sums: each workgroup reduces its own pixels (wave shuffles, then the four
// waves in order) and writes one partial per sum to the workspace; a second
// small kernel adds the partials of an image (or of a plane) in a fixed order
// in fp64.  No atomics anywhere: the results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_loss.h"
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_loss_layout.h"

using namespace gs;

namespace {

constexpr float PL_C1 = 0.01f * 0.01f, PL_C2 = 0.03f * 0.03f;
constexpr int PL_ROWS = PL_TILE * PL_TILE / PL_THREADS;  // output rows per thread (4)
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr int PL_STAGE = (PL_IN * PL_IN + PL_THREADS - 1) / PL_THREADS;  // staged pixels per thread (7)
static_assert(PL_THREADS % 64 == 0 && PL_THREADS % PL_TILE == 0 && PL_ROWS * PL_THREADS == PL_TILE * PL_TILE,
              "tile / workgroup geometry");

struct PhotoArgs {
  int Ch, H, W, tiles_x, tiles;
  const float* image;
  const float* target;
  const float* mask;
  const float* gain;
  const float* offset;
  int64_t mask_stride;
  float l1_n, ssim_n;  // l1_weight / (Ch H W), ssim_weight / (Ch H W): the backward's factors
  float w[PL_TAPS];    // the 1-D window
};

// Where a workgroup works: plane, image, tile origin.
struct TilePos {
  int64_t plane;
  int b, ox, oy;
};
__device__ inline TilePos tile_pos(const PhotoArgs& a) {
  TilePos t;
  const int64_t bid = blockIdx.x;
  t.plane = bid / a.tiles;
  const int tile = (int)(bid - t.plane * a.tiles);
  const int ty = tile / a.tiles_x;
  t.oy = ty * PL_TILE;
  t.ox = (tile - ty * a.tiles_x) * PL_TILE;
  t.b = (int)(t.plane / a.Ch);
  return t;
}

// x = (gain * image + offset) * mask as three separately rounded operations,
// the way the PyTorch expression rounds them: forward and backward see the
// same x, and sign(x - y) agrees with the reference at the kink of |x - y|.
__device__ inline float corrected(float g, float v, float o, float m) {
  return __fmul_rn(__fadd_rn(__fmul_rn(g, v), o), m);
}

// Workgroup sums of two values in a fixed order; thread 0 writes out[0..1].
__device__ inline void block_sum2(float u, float v, float (*red)[PL_WAVES], float* out) {
  u = wave_sum(u);
  v = wave_sum(v);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = u;
    red[1][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float su = red[0][0], sv = red[1][0];
#pragma unroll
    for (int i = 1; i < PL_WAVES; ++i) {
      su += red[0][i];
      sv += red[1][i];
    }
    out[0] = su;
    out[1] = sv;
  }
}

// Column pass: thread (col, r0) adds the window down the column for its
// PL_ROWS consecutive output rows of N maps staged as sh[N][PL_IN][PL_TILE].
template <int N>
__device__ inline void column_pass(const float (*sh)[PL_IN][PL_TILE], const PhotoArgs& a, int col, int r0,
                                   float (&acc)[PL_ROWS][N]) {
#pragma unroll
  for (int q = 0; q < PL_ROWS; ++q)
#pragma unroll
    for (int m = 0; m < N; ++m) acc[q][m] = 0.f;
#pragma unroll
  for (int j = 0; j < PL_ROWS + PL_TAPS - 1; ++j) {
    float v[N];
#pragma unroll
    for (int m = 0; m < N; ++m) v[m] = sh[m][r0 + j][col];
#pragma unroll
    for (int q = 0; q < PL_ROWS; ++q) {
      const int k = j - q;
      if (k >= 0 && k < PL_TAPS) {
#pragma unroll
        for (int m = 0; m < N; ++m) acc[q][m] = fmaf(a.w[k], v[m], acc[q][m]);
      }
    }
  }
}

__global__ __launch_bounds__(PL_THREADS) void pl_fwd_kernel(PhotoArgs a, int64_t map_stride, float* __restrict__ pqr,
                                                            float* __restrict__ partial) {
  __shared__ float sx[PL_IN][PL_IN + 1], sy[PL_IN][PL_IN + 1];
  __shared__ float sh[5][PL_IN][PL_TILE];
  __shared__ float red[2][PL_WAVES];
  const int tid = threadIdx.x;
  const TilePos t = tile_pos(a);
  const int64_t HW = (int64_t)a.H * a.W;
  const float* im = a.image + t.plane * HW;
  const float* tg = a.target + t.plane * HW;
  const float* mk = a.mask ? a.mask + (int64_t)t.b * a.mask_stride : nullptr;
  const float g = a.gain ? a.gain[t.plane] : 1.f, o = a.offset ? a.offset[t.plane] : 0.f;

  // stage the tile: every load of the thread's PL_STAGE pixels is issued before
  // the first is used (one round trip to memory, not PL_STAGE)
  float vi[PL_STAGE], vt[PL_STAGE], vm[PL_STAGE];
#pragma unroll
  for (int s = 0; s < PL_STAGE; ++s) {
    const int i = tid + s * PL_THREADS, r = i / PL_IN, c = i - r * PL_IN;
    const int gy = t.oy - PL_HALO + r, gx = t.ox - PL_HALO + c;
    vi[s] = vt[s] = 0.f;
    vm[s] = 1.f;
    if (i < PL_IN * PL_IN && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const int64_t p = (int64_t)gy * a.W + gx;
      vi[s] = im[p];
      vt[s] = tg[p];
      if (mk) vm[s] = mk[p];
    } else {
      vm[s] = 0.f;  // outside the image x and y are 0 whatever the offset
    }
  }
#pragma unroll
  for (int s = 0; s < PL_STAGE; ++s) {
    const int i = tid + s * PL_THREADS, r = i / PL_IN, c = i - r * PL_IN;
    if (i < PL_IN * PL_IN) {
      sx[r][c] = corrected(g, vi[s], o, vm[s]);
      sy[r][c] = vt[s] * vm[s];
    }
  }
  __syncthreads();

  // row pass: five window sums per (staged row, output column)
  for (int i = tid; i < PL_IN * PL_TILE; i += PL_THREADS) {
    const int r = i / PL_TILE, c = i % PL_TILE;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int k = 0; k < PL_TAPS; ++k) {
      const float xv = sx[r][c + k], yv = sy[r][c + k];
      const float wx = a.w[k] * xv, wy = a.w[k] * yv;
      s0 += wx;
      s1 += wy;
      s2 = fmaf(wx, xv, s2);
      s3 = fmaf(wy, yv, s3);
      s4 = fmaf(wx, yv, s4);
    }
    sh[0][r][c] = s0;
    sh[1][r][c] = s1;
    sh[2][r][c] = s2;
    sh[3][r][c] = s3;
    sh[4][r][c] = s4;
  }
  __syncthreads();

  const int col = tid % PL_TILE, r0 = (tid / PL_TILE) * PL_ROWS;
  float acc[PL_ROWS][5];
  column_pass<5>(sh, a, col, r0, acc);

  float l1 = 0.f, ss = 0.f;
  const int gx = t.ox + col;
#pragma unroll
  for (int q = 0; q < PL_ROWS; ++q) {
    const int gy = t.oy + r0 + q;
    if (gx < a.W && gy < a.H) {
      const float mu1 = acc[q][0], mu2 = acc[q][1];
      const float s11 = acc[q][2] - mu1 * mu1, s22 = acc[q][3] - mu2 * mu2, s12 = acc[q][4] - mu1 * mu2;
      const float N1 = 2.f * mu1 * mu2 + PL_C1, N2 = 2.f * s12 + PL_C2;
      const float D1 = mu1 * mu1 + mu2 * mu2 + PL_C1, D2 = s11 + s22 + PL_C2;
      const float A = N1 * N2, iD = 1.f / (D1 * D2);
      ss += A * iD;
      l1 += fabsf(sx[r0 + q + PL_HALO][col + PL_HALO] - sy[r0 + q + PL_HALO][col + PL_HALO]);
      const float P = 2.f * iD * (mu2 * (N2 - N1) + mu1 * A * (1.f / D2 - 1.f / D1));
      const float Q = -A * iD / D2;
      const float R = 2.f * N1 * iD;
      float* out = pqr + t.plane * HW + (int64_t)gy * a.W + gx;
      out[0] = P;
      out[map_stride] = Q;
      out[2 * map_stride] = R;
    }
  }
  block_sum2(l1, ss, red, partial + 2 * (int64_t)blockIdx.x);
}

// losses[b] from the image's partials, added in index order (fp64).
__global__ __launch_bounds__(PL_THREADS) void pl_fwd_final_kernel(int64_t per_image, double n, float l1_weight,
                                                                  float ssim_weight, const float* __restrict__ partial,
                                                                  float* __restrict__ losses) {
  __shared__ double red[2][PL_THREADS];
  const int tid = threadIdx.x;
  const float* p = partial + 2 * per_image * (int64_t)blockIdx.x;
  double u = 0.0, v = 0.0;
  for (int64_t i = tid; i < per_image; i += PL_THREADS) {
    u += (double)p[2 * i];
    v += (double)p[2 * i + 1];
  }
  red[0][tid] = u;
  red[1][tid] = v;
  __syncthreads();
  for (int s = PL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0)
    losses[blockIdx.x] = (float)((double)l1_weight * (red[0][0] / n) + (double)ssim_weight * (1.0 - red[1][0] / n));
}

__global__ __launch_bounds__(PL_THREADS) void pl_bwd_kernel(PhotoArgs a, int64_t map_stride,
                                                            const float* __restrict__ pqr,
                                                            const float* __restrict__ dL_dloss,
                                                            float* __restrict__ d_image, float* __restrict__ partial) {
  __shared__ float sp[3][PL_IN][PL_IN + 1];
  __shared__ float sh[3][PL_IN][PL_TILE];
  __shared__ float red[2][PL_WAVES];
  const int tid = threadIdx.x;
  const TilePos t = tile_pos(a);
  const int64_t HW = (int64_t)a.H * a.W;
  const float* maps = pqr + t.plane * HW;
  const float* im = a.image + t.plane * HW;
  const float* tg = a.target + t.plane * HW;
  const float* mk = a.mask ? a.mask + (int64_t)t.b * a.mask_stride : nullptr;
  const int col = tid % PL_TILE, r0 = (tid / PL_TILE) * PL_ROWS;
  const int gx = t.ox + col;

  // the thread's own pixels (used after the two passes): loaded up front
  float iv[PL_ROWS], tv[PL_ROWS], mv[PL_ROWS];
#pragma unroll
  for (int q = 0; q < PL_ROWS; ++q) {
    const int gy = t.oy + r0 + q;
    iv[q] = tv[q] = 0.f;
    mv[q] = 1.f;
    if (gx < a.W && gy < a.H) {
      const int64_t p = (int64_t)gy * a.W + gx;
      iv[q] = im[p];
      tv[q] = tg[p];
      if (mk) mv[q] = mk[p];
    }
  }

  float vp[PL_STAGE][3];  // all loads first, as in the forward
#pragma unroll
  for (int s = 0; s < PL_STAGE; ++s) {
    const int i = tid + s * PL_THREADS, r = i / PL_IN, c = i - r * PL_IN;
    const int gy = t.oy - PL_HALO + r, gx = t.ox - PL_HALO + c;
    vp[s][0] = vp[s][1] = vp[s][2] = 0.f;
    if (i < PL_IN * PL_IN && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const float* in = maps + (int64_t)gy * a.W + gx;
      vp[s][0] = in[0];
      vp[s][1] = in[map_stride];
      vp[s][2] = in[2 * map_stride];
    }
  }
#pragma unroll
  for (int s = 0; s < PL_STAGE; ++s) {
    const int i = tid + s * PL_THREADS, r = i / PL_IN, c = i - r * PL_IN;
    if (i < PL_IN * PL_IN) {
      sp[0][r][c] = vp[s][0];
      sp[1][r][c] = vp[s][1];
      sp[2][r][c] = vp[s][2];
    }
  }
  __syncthreads();

  for (int i = tid; i < PL_IN * PL_TILE; i += PL_THREADS) {
    const int r = i / PL_TILE, c = i % PL_TILE;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < PL_TAPS; ++k) {
      s0 = fmaf(a.w[k], sp[0][r][c + k], s0);
      s1 = fmaf(a.w[k], sp[1][r][c + k], s1);
      s2 = fmaf(a.w[k], sp[2][r][c + k], s2);
    }
    sh[0][r][c] = s0;
    sh[1][r][c] = s1;
    sh[2][r][c] = s2;
  }
  __syncthreads();

  float acc[PL_ROWS][3];
  column_pass<3>(sh, a, col, r0, acc);

  const float g = a.gain ? a.gain[t.plane] : 1.f, o = a.offset ? a.offset[t.plane] : 0.f;
  const float up = dL_dloss[t.b];
  float dg = 0.f, dofs = 0.f;
#pragma unroll
  for (int q = 0; q < PL_ROWS; ++q) {
    const int gy = t.oy + r0 + q;
    if (gx < a.W && gy < a.H) {
      const float m = mv[q];
      const float x = corrected(g, iv[q], o, m), y = tv[q] * m;
      const float dssim = acc[q][0] + 2.f * x * acc[q][1] + y * acc[q][2];
      const float d = x - y;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);  // torch.abs: derivative 0 at 0
      const float dx = up * (a.l1_n * sgn - a.ssim_n * dssim) * m;
      d_image[t.plane * HW + (int64_t)gy * a.W + gx] = g * dx;
      dg = fmaf(iv[q], dx, dg);
      dofs += dx;
    }
  }
  block_sum2(dg, dofs, red, partial + 2 * (int64_t)blockIdx.x);
}

// d gain / d offset of one plane from its tiles' partials, in tile order (fp64).
__global__ __launch_bounds__(64) void pl_bwd_final_kernel(int tiles, const float* __restrict__ partial,
                                                          float* __restrict__ d_gain, float* __restrict__ d_offset) {
  __shared__ double red[2][64];
  const int tid = threadIdx.x;
  const float* p = partial + 2 * (int64_t)tiles * blockIdx.x;
  double u = 0.0, v = 0.0;
  for (int i = tid; i < tiles; i += 64) {
    u += (double)p[2 * i];
    v += (double)p[2 * i + 1];
  }
  red[0][tid] = u;
  red[1][tid] = v;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (d_gain) d_gain[blockIdx.x] = (float)red[0][0];
    if (d_offset) d_offset[blockIdx.x] = (float)red[1][0];
  }
}

PhotoArgs kernel_args(const gs_photo_loss& a, const PhotoLossLayout& L) {
  PhotoArgs k{};
  k.Ch = a.Ch;
  k.H = a.H;
  k.W = a.W;
  k.tiles_x = (int)L.tiles_x;
  k.tiles = (int)L.tiles;
  k.image = a.image;
  k.target = a.target;
  k.mask = a.mask;
  k.gain = a.gain;
  k.offset = a.offset;
  k.mask_stride = a.mask ? a.mask_batch_stride : 0;
  const double n = (double)a.Ch * a.H * a.W;
  k.l1_n = (float)((double)a.l1_weight / n);
  k.ssim_n = (float)((double)a.ssim_weight / n);
  // external.py:90-92: exp(-(i - 5)^2 / (2 sigma^2)) rounded to fp32, normalised in fp32
  float gsum = 0.f;
  for (int i = 0; i < PL_TAPS; ++i) {
    k.w[i] = (float)exp(-(double)((i - PL_HALO) * (i - PL_HALO)) / (2.0 * 1.5 * 1.5));
    gsum += k.w[i];
  }
  for (int i = 0; i < PL_TAPS; ++i) k.w[i] /= gsum;
  return k;
}

}  // namespace

extern "C" {

int gs_photo_loss_forward(const gs_photo_loss* args, gs_stream_t stream) {
  if (int e = gs_photo_loss_validate(args, 0, nullptr, nullptr, nullptr, nullptr)) return e;
  const gs_photo_loss& a = *args;
  const PhotoLossLayout L(a.B, a.Ch, a.H, a.W);
  const PhotoArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(a.workspace);
  float* pqr = reinterpret_cast<float*>(ws + L.pqr);
  float* partial = reinterpret_cast<float*>(ws + L.fwd_partial);
  hipLaunchKernelGGL(pl_fwd_kernel, dim3((unsigned)L.blocks), dim3(PL_THREADS), 0, s, k,
                     L.planes * L.plane_elems, pqr, partial);
  hipLaunchKernelGGL(pl_fwd_final_kernel, dim3((unsigned)a.B), dim3(PL_THREADS), 0, s, (int64_t)a.Ch * L.tiles,
                     (double)a.Ch * a.H * a.W, a.l1_weight, a.ssim_weight, partial, a.losses);
  return launch_status("photometric loss forward", 0, s);
}

int gs_photo_loss_backward(const gs_photo_loss* args, const float* dL_dloss, float* dL_dimage, float* dL_dgain,
                           float* dL_doffset, gs_stream_t stream) {
  if (int e = gs_photo_loss_validate(args, 1, dL_dloss, dL_dimage, dL_dgain, dL_doffset)) return e;
  const gs_photo_loss& a = *args;
  const PhotoLossLayout L(a.B, a.Ch, a.H, a.W);
  const PhotoArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(a.workspace);
  const float* pqr = reinterpret_cast<const float*>(ws + L.pqr);
  float* partial = reinterpret_cast<float*>(ws + L.bwd_partial);
  hipLaunchKernelGGL(pl_bwd_kernel, dim3((unsigned)L.blocks), dim3(PL_THREADS), 0, s, k, L.planes * L.plane_elems,
                     pqr, dL_dloss, dL_dimage, partial);
  if (dL_dgain || dL_doffset)
    hipLaunchKernelGGL(pl_bwd_final_kernel, dim3((unsigned)L.planes), dim3(64), 0, s, (int)L.tiles, partial,
                       dL_dgain, dL_doffset);
  return launch_status("photometric loss backward", 0, s);
}

}  // extern "C"
