// gs_metrics.hip -- the evaluation metrics of the reference's quality reports
// (external.py:85-87 calc_psnr; metrics.py:14-43, 82-129 compute_psnr / mPSNR;
// :334-424 mSSIM; :222-250, 523-551 mask_iou / MaskIoU) for a whole camera
// batch, forward only (C ABI: include/gs_metrics.h).
//
// gs_image_metrics: one workgroup of 256 threads owns one 32 x 32 tile of one
// (image, channel) plane, in the design of gs_loss.hip.  The tile of pred,
// target and mask is staged in LDS with the 10 pixels to its right and below
// (the window is "valid": output (y, x) covers inputs (y..y+10, x..x+10), so
// there is no padding and nothing outside the image reaches an output).  The
// masked window runs along the rows for the five maps p, t, pp, tt, pt (LDS to
// LDS, each rescaled by 11 / n, with the pass's output mask as a sixth map) and
// down the columns (LDS to registers, four rows of one column per thread);
// every output pixel then gets its SSIM value.  The three plain sums (squared
// error, absolute error, mask) are taken over the tile's own 32 x 32 input
// pixels from the same staged tile: the tiling covers H x W, so the last 10
// rows and columns, which no output tile owns, are summed by workgroups that
// skip the two passes.
//
// Sums: each workgroup reduces its own pixels (wave_sum, then the four waves in
// order) and writes four partials to the workspace; a second small kernel adds
// the partials of an image in a fixed order in fp64.  No atomics: the results
// are bit-reproducible.  The file is compiled without FMA contraction, so the
// map of pred == target is 1 exactly (numerator and denominator round alike).
//
// HBM bytes, from shapes: (2 Ch + 1) floats read per pixel per image, 16 bytes
// written per workgroup; halo re-reads are expected to hit in cache.
//
// gs_mask_iou: a workgroup counts one chunk of one image with integer adds
// (wave_sum of int, one 64-bit integer atomic per workgroup and count into the
// zeroed out[b]): exact, so the order does not matter.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_metrics.h"
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_metrics_layout.h"

using namespace gs;

namespace {

constexpr float MT_C1 = 0.01f * 0.01f, MT_C2 = 0.03f * 0.03f;
constexpr int MT_ROWS = MT_TILE * MT_TILE / MT_THREADS;  // output rows per thread (4)
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_STAGE = (MT_IN * MT_IN + MT_THREADS - 1) / MT_THREADS;  // staged pixels per thread (7)
constexpr int MT_MAPS = 5;  // p, t, pp, tt, pt
static_assert(MT_THREADS % 64 == 0 && MT_THREADS % MT_TILE == 0 && MT_ROWS * MT_THREADS == MT_TILE * MT_TILE,
              "tile / workgroup geometry");

struct MetricArgs {
  int Ch, H, W, tiles_x, tiles, want_ssim;
  const float* pred;
  const float* target;
  const float* mask;
  int64_t mask_stride;
  float w[MT_TAPS];  // the 1-D window
};

// Workgroup sums of MT_SUMS values in a fixed order; thread 0 writes out[0..MT_SUMS).
__device__ inline void block_sums(float (&v)[MT_SUMS], float (*red)[MT_WAVES], float* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < MT_SUMS; ++i) {
    v[i] = wave_sum(v[i]);
    if ((tid & 63) == 0) red[i][tid >> 6] = v[i];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < MT_SUMS; ++i) {
      float s = red[i][0];
#pragma unroll
      for (int k = 1; k < MT_WAVES; ++k) s += red[i][k];
      out[i] = s;
    }
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_image_kernel(MetricArgs a, float* __restrict__ partial) {
  __shared__ float sp[MT_IN][MT_IN + 1], st[MT_IN][MT_IN + 1], sm[MT_IN][MT_IN + 1];
  __shared__ float sh[MT_MAPS + 1][MT_IN][MT_TILE];  // the row pass's five maps and its output mask
  __shared__ float red[MT_SUMS][MT_WAVES];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int64_t plane = bid / a.tiles;
  const int tile = (int)(bid - plane * a.tiles);
  const int ty = tile / a.tiles_x;
  const int oy = ty * MT_TILE, ox = (tile - ty * a.tiles_x) * MT_TILE;
  const int b = (int)(plane / a.Ch);
  const int ch = (int)(plane - (int64_t)b * a.Ch);
  const int64_t HW = (int64_t)a.H * a.W;
  const float* pr = a.pred + plane * HW;
  const float* tg = a.target + plane * HW;
  const float* mk = a.mask ? a.mask + (int64_t)b * a.mask_stride : nullptr;
  // block-uniform: does this tile hold an output position at all?
  const bool ssim = a.want_ssim && ox < a.W - (MT_TAPS - 1) && oy < a.H - (MT_TAPS - 1);

  // stage the tile (own pixels only when there is no window to run): every load of the
  // thread's MT_STAGE pixels is issued before the first is used
  float vp[MT_STAGE], vt[MT_STAGE], vm[MT_STAGE];
#pragma unroll
  for (int s = 0; s < MT_STAGE; ++s) {
    const int i = tid + s * MT_THREADS, r = i / MT_IN, c = i - r * MT_IN;
    const int gy = oy + r, gx = ox + c;
    vp[s] = vt[s] = vm[s] = 0.f;  // outside the image: masked out, never under a valid window
    if (i < MT_IN * MT_IN && gy < a.H && gx < a.W && (ssim || (r < MT_TILE && c < MT_TILE))) {
      const int64_t p = (int64_t)gy * a.W + gx;
      vp[s] = pr[p];
      vt[s] = tg[p];
      vm[s] = mk ? mk[p] : 1.f;
    }
  }
#pragma unroll
  for (int s = 0; s < MT_STAGE; ++s) {
    const int i = tid + s * MT_THREADS, r = i / MT_IN, c = i - r * MT_IN;
    if (i < MT_IN * MT_IN) {
      sp[r][c] = vp[s];
      st[r][c] = vt[s];
      sm[r][c] = vm[s];
    }
  }
  __syncthreads();

  const int col = tid % MT_TILE, r0 = (tid / MT_TILE) * MT_ROWS;
  float sums[MT_SUMS] = {0.f, 0.f, 0.f, 0.f};
  // the three plain sums over the thread's own input pixels (zero outside the image)
#pragma unroll
  for (int q = 0; q < MT_ROWS; ++q) {
    const float m = sm[r0 + q][col];
    const float d = (sp[r0 + q][col] - st[r0 + q][col]) * m;
    sums[0] = fmaf(d, d, sums[0]);
    sums[1] += fabsf(d);
    if (ch == 0) sums[2] += m;  // the mask has no channels: counted once per image
  }

  if (ssim) {
    // row pass: five masked window sums per (staged row, output column), rescaled by 11 / n
    for (int i = tid; i < MT_IN * MT_TILE; i += MT_THREADS) {
      const int r = i / MT_TILE, c = i % MT_TILE;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, n = 0.f;
#pragma unroll
      for (int k = 0; k < MT_TAPS; ++k) {
        const float p = sp[r][c + k], t = st[r][c + k], m = sm[r][c + k];
        const float wm = a.w[k] * m;
        s0 = fmaf(wm, p, s0);
        s1 = fmaf(wm, t, s1);
        s2 = fmaf(wm, p * p, s2);
        s3 = fmaf(wm, t * t, s3);
        s4 = fmaf(wm, p * t, s4);
        n += m;
      }
      const float on = n != 0.f ? 1.f : 0.f;
      const float f = n != 0.f ? (float)MT_TAPS / n : 0.f;
      sh[0][r][c] = s0 * f;
      sh[1][r][c] = s1 * f;
      sh[2][r][c] = s2 * f;
      sh[3][r][c] = s3 * f;
      sh[4][r][c] = s4 * f;
      sh[5][r][c] = on;
    }
    __syncthreads();

    // column pass: the row pass's maps are 0 where its mask is 0, so the masked window sum
    // is the plain one; the count of the mask gives the second rescale
    float acc[MT_ROWS][MT_MAPS + 1];
#pragma unroll
    for (int q = 0; q < MT_ROWS; ++q)
#pragma unroll
      for (int m = 0; m <= MT_MAPS; ++m) acc[q][m] = 0.f;
#pragma unroll
    for (int j = 0; j < MT_ROWS + MT_TAPS - 1; ++j) {
      float v[MT_MAPS + 1];
#pragma unroll
      for (int m = 0; m <= MT_MAPS; ++m) v[m] = sh[m][r0 + j][col];
#pragma unroll
      for (int q = 0; q < MT_ROWS; ++q) {
        const int k = j - q;
        if (k >= 0 && k < MT_TAPS) {
#pragma unroll
          for (int m = 0; m < MT_MAPS; ++m) acc[q][m] = fmaf(a.w[k], v[m], acc[q][m]);
          acc[q][MT_MAPS] += v[MT_MAPS];
        }
      }
    }

    const int gx = ox + col;
#pragma unroll
    for (int q = 0; q < MT_ROWS; ++q) {
      const int gy = oy + r0 + q;
      if (gx < a.W - (MT_TAPS - 1) && gy < a.H - (MT_TAPS - 1)) {
        const float n = acc[q][MT_MAPS];
        const float f = n != 0.f ? (float)MT_TAPS / n : 0.f;
        const float mu0 = acc[q][0] * f, mu1 = acc[q][1] * f;
        const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
        const float s00 = fmaxf(acc[q][2] * f - mu00, 0.f), s11 = fmaxf(acc[q][3] * f - mu11, 0.f);
        const float s = acc[q][4] * f - mu01;
        const float s01 = copysignf(fminf(sqrtf(s00 * s11), fabsf(s)), s);  // sign(s) min(...): 0 where s is 0
        const float numer = (2.f * mu01 + MT_C1) * (2.f * s01 + MT_C2);
        const float denom = (mu00 + mu11 + MT_C1) * (s00 + s11 + MT_C2);
        sums[3] += numer / denom;
      }
    }
  }
  block_sums(sums, red, partial + MT_SUMS * bid);
}

// out[b] from the image's partials, added in index order (fp64).
__global__ __launch_bounds__(MT_THREADS) void mt_image_final_kernel(int64_t per_image, double ssim_n,
                                                                    const float* __restrict__ partial,
                                                                    float* __restrict__ out) {
  __shared__ double red[MT_SUMS][MT_THREADS];
  const int tid = threadIdx.x;
  const float* p = partial + MT_SUMS * per_image * (int64_t)blockIdx.x;
  double v[MT_SUMS] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < per_image; i += MT_THREADS) {
#pragma unroll
    for (int k = 0; k < MT_SUMS; ++k) v[k] += (double)p[MT_SUMS * i + k];
  }
#pragma unroll
  for (int k = 0; k < MT_SUMS; ++k) red[k][tid] = v[k];
  __syncthreads();
  for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < MT_SUMS; ++k) red[k][tid] += red[k][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* o = out + MT_SUMS * (int64_t)blockIdx.x;
    o[0] = (float)red[0][0];
    o[1] = (float)red[1][0];
    o[2] = (float)red[2][0];
    o[3] = ssim_n > 0.0 ? (float)(red[3][0] / ssim_n) : 0.f;
  }
}

__global__ __launch_bounds__(MT_IOU_THREADS) void mt_iou_kernel(int64_t n, const float* __restrict__ pred,
                                                                const float* __restrict__ target, float threshold,
                                                                unsigned long long* __restrict__ out) {
  __shared__ int red[2][MT_IOU_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * n;
  const int64_t lo = (int64_t)blockIdx.x * MT_IOU_CHUNK;
  const int64_t hi = lo + MT_IOU_CHUNK < n ? lo + MT_IOU_CHUNK : n;
  int both = 0, either = 0;
  for (int64_t i = lo + tid; i < hi; i += MT_IOU_THREADS) {
    const bool p = pred[base + i] > threshold, t = target[base + i] > threshold;
    both += (p && t) ? 1 : 0;
    either += (p || t) ? 1 : 0;
  }
  both = wave_sum(both);
  either = wave_sum(either);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = both;
    red[1][tid >> 6] = either;
  }
  __syncthreads();
  if (tid == 0) {
    int sb = 0, se = 0;
#pragma unroll
    for (int k = 0; k < MT_IOU_THREADS / 64; ++k) {
      sb += red[0][k];
      se += red[1][k];
    }
    // integer adds commute exactly: the counts do not depend on the workgroups' order
    if (sb) atomicAdd(out + 2 * (int64_t)blockIdx.y, (unsigned long long)sb);
    if (se) atomicAdd(out + 2 * (int64_t)blockIdx.y + 1, (unsigned long long)se);
  }
}

MetricArgs kernel_args(const struct gs_image_metrics& a, const ImageMetricsLayout& L) {
  MetricArgs k{};
  k.Ch = a.Ch;
  k.H = a.H;
  k.W = a.W;
  k.tiles_x = (int)L.tiles_x;
  k.tiles = (int)L.tiles;
  k.want_ssim = a.want_ssim ? 1 : 0;
  k.pred = a.pred;
  k.target = a.target;
  k.mask = a.mask;
  k.mask_stride = a.mask ? a.mask_batch_stride : 0;
  // metrics.py:368-376: exp(-0.5 ((k - 5) / sigma)^2), normalised; taken in fp64, rounded once
  double w[MT_TAPS], sum = 0.0;
  for (int i = 0; i < MT_TAPS; ++i) {
    const double d = (i - MT_TAPS / 2) / 1.5;
    w[i] = exp(-0.5 * d * d);
    sum += w[i];
  }
  for (int i = 0; i < MT_TAPS; ++i) k.w[i] = (float)(w[i] / sum);
  return k;
}

}  // namespace

extern "C" {

int gs_image_metrics(const struct gs_image_metrics* args, gs_stream_t stream) {
  if (int e = gs_image_metrics_validate(args)) return e;
  const struct gs_image_metrics& a = *args;
  const ImageMetricsLayout L(a.B, a.Ch, a.H, a.W);
  const MetricArgs k = kernel_args(a, L);
  hipStream_t s = (hipStream_t)stream;
  float* partial = at<float>(a.workspace, L.partial);
  const double ssim_n = a.want_ssim ? (double)a.Ch * (a.H - (MT_TAPS - 1)) * (a.W - (MT_TAPS - 1)) : 0.0;
  hipLaunchKernelGGL(mt_image_kernel, dim3((unsigned)L.blocks), dim3(MT_THREADS), 0, s, k, partial);
  hipLaunchKernelGGL(mt_image_final_kernel, dim3((unsigned)a.B), dim3(MT_THREADS), 0, s, (int64_t)a.Ch * L.tiles,
                     ssim_n, partial, a.out);
  return launch_status("image metrics", 0, s);
}

int gs_mask_iou(int32_t B, int64_t n, const float* pred, const float* target, float threshold, int64_t* out,
                gs_stream_t stream) {
  if (int e = gs_mask_iou_validate(B, n, pred, target, threshold, out)) return e;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(out, 0, sizeof(int64_t) * 2 * (size_t)B, s);
  if (err != hipSuccess) return gs_set_error((int)err, "mask IoU: %s", hipGetErrorString(err));
  const unsigned chunks = (unsigned)((n + MT_IOU_CHUNK - 1) / MT_IOU_CHUNK);
  hipLaunchKernelGGL(mt_iou_kernel, dim3(chunks, (unsigned)B), dim3(MT_IOU_THREADS), 0, s, n, pred, target,
                     threshold, reinterpret_cast<unsigned long long*>(out));
  return launch_status("mask IoU", 0, s);
}

}  // extern "C"
