// gs_resample.hip -- the bilinear resample between a render and a prior of
// another size (the reference's F.interpolate(..., mode='bilinear') calls:
// revise_train.py:100-104, dyn_double.py:303), forward and backward, for
// B * Ch independent planes (C ABI: include/gs_resample.h).
//
// Both passes are pure streaming.  A thread owns RS_VEC = 4 consecutive x of
// one row of the side it WRITES (the output in the forward, the input's
// gradient in the backward), computes that row's and those columns' taps and
// weights once from the shared axis function (gs_resample_layout.h), and then
// walks the planes blockIdx.y, blockIdx.y + gridDim.y, ... with them: the
// index arithmetic is paid once per thread, not once per plane, and the loads
// of consecutive planes are independent.  Stores are one 16-byte store where
// the four elements exist and their address is 16-byte aligned (decided per
// thread and plane from the address itself, so planes with odd H*W and rows
// with W % 4 != 0 are handled), scalar stores otherwise.
//
// Forward: a gather of the four taps.
// Backward: a gather too.  i0(o) is non-decreasing, so the outputs whose
// lower tap is i are the contiguous range [first[i], first[i + 1]); input i
// receives l1 from the range of i - 1, l0 from its own, and both at the
// clamped last index.  resample_first_kernel writes the two `first` tables
// (rows, columns) into the workspace, the backward kernel reads them.  Terms
// are summed in ascending (oy, ox) order: per output row the x terms, then the
// row's y weight.  No atomics, no memset: elements no output taps get 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_resample.h"
#include "gs_launch.h"
#include "gs_resample_layout.h"

using namespace gs;

namespace {

static_assert(RS_VEC == 4, "a float4 per thread");

struct ResampleArgs {
  int H, W, h, w, align;
  float sy, sx;  // resample_scale of the rows and of the columns, from the host
  int64_t planes;
};

__device__ inline void store4(float* p, const float (&v)[RS_VEC], int n) {
  if (n == RS_VEC && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < RS_VEC; ++j)
      if (j < n) p[j] = v[j];
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_fwd_kernel(ResampleArgs a, const float* __restrict__ x,
                                                                  float* __restrict__ y) {
  const int wq = (a.w + RS_VEC - 1) / RS_VEC;
  const int64_t q = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (q >= (int64_t)a.h * wq) return;
  const int oy = (int)(q / wq), ox0 = (int)(q - (int64_t)oy * wq) * RS_VEC;
  const int n = a.w - ox0 < RS_VEC ? a.w - ox0 : RS_VEC;
  const AxisTap ty = resample_tap(a.sy, a.H, oy, a.align);
  AxisTap tx[RS_VEC];
#pragma unroll
  for (int j = 0; j < RS_VEC; ++j)  // past the row's end: the last column again, never stored
    tx[j] = resample_tap(a.sx, a.W, ox0 + j < a.w ? ox0 + j : a.w - 1, a.align);
  const int64_t HW = (int64_t)a.H * a.W, hw = (int64_t)a.h * a.w;
  const int64_t r0 = (int64_t)ty.i0 * a.W, r1 = (int64_t)ty.i1 * a.W, out = (int64_t)oy * a.w + ox0;
  for (int64_t p = blockIdx.y; p < a.planes; p += gridDim.y) {
    const float* top = x + p * HW + r0;
    const float* bot = x + p * HW + r1;
    float v[RS_VEC];
#pragma unroll
    for (int j = 0; j < RS_VEC; ++j) {
      const float t = tx[j].l0 * top[tx[j].i0] + tx[j].l1 * top[tx[j].i1];
      const float b = tx[j].l0 * bot[tx[j].i0] + tx[j].l1 * bot[tx[j].i1];
      v[j] = ty.l0 * t + ty.l1 * b;
    }
    store4(y + p * hw + out, v, n);
  }
}

// One thread per output row, then one per output column: the entries of
// first_y / first_x that output owns (resample_first_of).
__global__ __launch_bounds__(RS_THREADS) void resample_first_kernel(ResampleArgs a, int32_t* __restrict__ first_y,
                                                                    int32_t* __restrict__ first_x) {
  const int t = blockIdx.x * RS_THREADS + threadIdx.x;
  if (t < a.h)
    resample_first_of(a.sy, a.H, a.h, t, a.align, first_y);
  else if (t - a.h < a.w)
    resample_first_of(a.sx, a.W, a.w, t - a.h, a.align, first_x);
}

// Sum over ox of wx(ox) * g[ox] for input column ix of one output row, for the
// RS_PB planes of a step at once (same taps and weights, independent loads):
// [xa, xb) are the outputs whose upper tap is ix, [xb, xc) those whose lower
// tap is ix; `last` (ix = W - 1): the upper tap of these is clamped onto ix too.
__device__ inline void row_terms(const ResampleArgs& a, const float* const (&g)[RS_PB], int xa, int xb, int xc,
                                 bool last, float (&s)[RS_PB]) {
#pragma unroll
  for (int u = 0; u < RS_PB; ++u) s[u] = 0.f;
  for (int ox = xa; ox < xb; ++ox) {
    const float l1 = resample_tap(a.sx, a.W, ox, a.align).l1;
#pragma unroll
    for (int u = 0; u < RS_PB; ++u) s[u] = fmaf(l1, g[u][ox], s[u]);
  }
  for (int ox = xb; ox < xc; ++ox) {
    const AxisTap t = resample_tap(a.sx, a.W, ox, a.align);
#pragma unroll
    for (int u = 0; u < RS_PB; ++u) {
      const float gv = g[u][ox];
      s[u] = fmaf(t.l0, gv, s[u]);
      if (last) s[u] = fmaf(t.l1, gv, s[u]);
    }
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_bwd_kernel(ResampleArgs a, const int32_t* __restrict__ first_y,
                                                                  const int32_t* __restrict__ first_x,
                                                                  const float* __restrict__ g, float* __restrict__ d_x) {
  const int Wq = (a.W + RS_VEC - 1) / RS_VEC;
  const int64_t q = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (q >= (int64_t)a.H * Wq) return;
  const int iy = (int)(q / Wq), ix0 = (int)(q - (int64_t)iy * Wq) * RS_VEC;
  const int n = a.W - ix0 < RS_VEC ? a.W - ix0 : RS_VEC;
  const int yb = first_y[iy], yc = first_y[iy + 1], ya = iy > 0 ? first_y[iy - 1] : yb;
  const bool last_y = iy == a.H - 1;
  int xa[RS_VEC], xb[RS_VEC], xc[RS_VEC];
#pragma unroll
  for (int j = 0; j < RS_VEC; ++j) {  // past the row's end: the last column again, never stored
    const int ix = ix0 + j < a.W ? ix0 + j : a.W - 1;
    xb[j] = first_x[ix];
    xc[j] = first_x[ix + 1];
    xa[j] = ix > 0 ? first_x[ix - 1] : xb[j];
  }
  const int64_t HW = (int64_t)a.H * a.W, hw = (int64_t)a.h * a.w;
  const int64_t out = (int64_t)iy * a.W + ix0;
  // RS_PB planes per step: p0, p0 + gridDim.y, ...; past the last plane a slot reads p0 again and stores nothing
  for (int64_t p0 = blockIdx.y; p0 < a.planes; p0 += (int64_t)gridDim.y * RS_PB) {
    const float* gp[RS_PB];
#pragma unroll
    for (int u = 0; u < RS_PB; ++u) {
      const int64_t p = p0 + (int64_t)u * gridDim.y;
      gp[u] = g + (p < a.planes ? p : p0) * hw;
    }
    float v[RS_PB][RS_VEC];
#pragma unroll
    for (int u = 0; u < RS_PB; ++u)
#pragma unroll
      for (int j = 0; j < RS_VEC; ++j) v[u][j] = 0.f;
    for (int oy = ya; oy < yc; ++oy) {
      const AxisTap t = resample_tap(a.sy, a.H, oy, a.align);
      const float* row[RS_PB];
#pragma unroll
      for (int u = 0; u < RS_PB; ++u) row[u] = gp[u] + (int64_t)oy * a.w;
      const bool lower = oy >= yb;  // iy is this row's lower tap (else its upper one)
#pragma unroll
      for (int j = 0; j < RS_VEC; ++j) {
        float s[RS_PB];
        row_terms(a, row, xa[j], xb[j], xc[j], ix0 + j >= a.W - 1, s);
#pragma unroll
        for (int u = 0; u < RS_PB; ++u) {
          v[u][j] = fmaf(lower ? t.l0 : t.l1, s[u], v[u][j]);
          if (lower && last_y) v[u][j] = fmaf(t.l1, s[u], v[u][j]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RS_PB; ++u) {
      const int64_t p = p0 + (int64_t)u * gridDim.y;
      if (p < a.planes) store4(d_x + p * HW + out, v[u], n);
    }
  }
}

ResampleArgs kernel_args(const gs_resample& a) {
  ResampleArgs k{};
  k.H = a.H; k.W = a.W; k.h = a.h; k.w = a.w;
  k.align = a.align_corners != 0;
  k.sy = resample_scale(a.H, a.h, k.align);
  k.sx = resample_scale(a.W, a.w, k.align);
  k.planes = (int64_t)a.B * a.Ch;
  return k;
}

}  // namespace

extern "C" {

int gs_resample_forward(const gs_resample* args, gs_stream_t stream) {
  if (int e = gs_resample_validate(args, 0, nullptr, nullptr)) return e;
  const ResampleArgs k = kernel_args(*args);
  const int64_t groups = resample_groups(k.h, k.w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resample_fwd_kernel, dim3((unsigned)groups, (unsigned)resample_fwd_plane_groups(k.planes)),
                     dim3(RS_THREADS), 0, s, k, args->x, args->y);
  return launch_status("resample forward", 0, s);
}

int gs_resample_backward(const gs_resample* args, const float* d_y, float* d_x, gs_stream_t stream) {
  if (int e = gs_resample_validate(args, 1, d_y, d_x)) return e;
  const ResampleArgs k = kernel_args(*args);
  const ResampleLayout L(k.H, k.W);
  int32_t* first_y = at<int32_t>(args->workspace, L.off_first_y);
  int32_t* first_x = at<int32_t>(args->workspace, L.off_first_x);
  const int64_t groups = resample_groups(k.H, k.W);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resample_first_kernel, dim3((unsigned)((k.h + k.w + RS_THREADS - 1) / RS_THREADS)),
                     dim3(RS_THREADS), 0, s, k, first_y, first_x);
  hipLaunchKernelGGL(resample_bwd_kernel, dim3((unsigned)groups, (unsigned)resample_bwd_plane_groups(k.planes, groups)),
                     dim3(RS_THREADS), 0, s, k, first_y, first_x, d_y, d_x);
  return launch_status("resample backward", 0, s);
}

}  // extern "C"
