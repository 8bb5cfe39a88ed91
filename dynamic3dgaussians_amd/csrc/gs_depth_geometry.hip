// gs_depth_geometry.hip -- geometry on depth maps for a whole camera batch,
// forward only (C ABI and the formulas: include/gs_depth_geometry.h): the point
// z-buffer of the reference's unproject_image (metrics.py:131-213) and its
// abs-rel score, dense and sparse unprojection (dyn_utils.py:442-480,
// ideaII.py:102-121, dyn_som.py:276-286), the flow a depth map induces between
// two cameras (ideaII.py:135-157) and the bilinear border sampler under
// warp_flow / accumulate_flows (ideaII.py:159-206).
//
// Every kernel is one thread per output element (or per point), 256 threads a
// workgroup, the batch on the grid's y extent, so the camera's matrices are
// wave-uniform loads.  All of them stream: what bounds them is HBM traffic
// (byte models in the header) except the z-buffer's second launch, whose cost
// is B * P scattered 32-bit integer min atomics.
//
// The z-buffer's bounds test is done on the rounded float coordinates with
// comparisons that are false for NaN, before any conversion to int: NaN, inf
// and coordinates beyond the int range never become an index.  The sampler
// replaces a NaN coordinate by 0 for addressing and writes NaN.
//
// The file is compiled without FMA contraction: every product and sum below
// rounds as written, as the PyTorch restatement's elementwise form does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_depth_geometry.h"
#include "gs_common.h"
#include "gs_depth_geometry_layout.h"
#include "gs_launch.h"

using namespace gs;

namespace {

constexpr int DG_WAVES = DG_THREADS / 64;
constexpr uint32_t DG_INF_BITS = 0x7F800000u;  // +inf: the largest bit pattern of a positive float

// rows 0..2 of a row-major 4 x 4 matrix applied to (x, y, z, 1)
__device__ inline void affine(const float* __restrict__ M, float x, float y, float z, float& ox, float& oy,
                              float& oz) {
  ox = M[0] * x + M[1] * y + M[2] * z + M[3];
  oy = M[4] * x + M[5] * y + M[6] * z + M[7];
  oz = M[8] * x + M[9] * y + M[10] * z + M[11];
}

// a row-major 3 x 3 matrix applied to (x, y, z)
__device__ inline void mul3(const float* __restrict__ K, float x, float y, float z, float& ox, float& oy,
                            float& oz) {
  ox = K[0] * x + K[1] * y + K[2] * z;
  oy = K[3] * x + K[4] * y + K[5] * z;
  oz = K[6] * x + K[7] * y + K[8] * z;
}

__global__ __launch_bounds__(DG_THREADS) void dg_fill_inf_kernel(int64_t plane, uint32_t* __restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (i < plane) depth[(int64_t)blockIdx.y * plane + i] = DG_INF_BITS;
}

__global__ __launch_bounds__(DG_THREADS) void dg_point_depth_kernel(int64_t P, int H, int W,
                                                                    const float* __restrict__ points,
                                                                    int64_t stride, const float* __restrict__ w2c,
                                                                    const float* __restrict__ K,
                                                                    uint32_t* __restrict__ depth) {
  const int b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (p >= P) return;
  const float* pt = points + (int64_t)b * stride + 3 * p;
  float cx, cy, cz, qx, qy, qz;
  affine(w2c + 16 * b, pt[0], pt[1], pt[2], cx, cy, cz);
  if (!(cz > 0.f)) return;  // behind the camera, on its plane, or NaN
  mul3(K + 9 * b, cx, cy, cz, qx, qy, qz);
  const float fu = rintf(qx / qz), fv = rintf(qy / qz);  // round half to even, as torch.round
  // in float, before any conversion: false for NaN, +-inf and everything outside the image
  if (!(fu >= 0.f && fu < (float)W && fv >= 0.f && fv < (float)H)) return;
  const int64_t idx = ((int64_t)b * H + (int)fv) * W + (int)fu;
  // cz > 0: positive floats order as their bit patterns
  atomicMin(depth + idx, __float_as_uint(cz));
}

__global__ __launch_bounds__(DG_THREADS) void dg_abs_rel_kernel(int64_t plane, const float* __restrict__ est,
                                                                const float* __restrict__ gt,
                                                                const float* __restrict__ exclude,
                                                                int64_t exclude_stride,
                                                                double* __restrict__ partial) {
  __shared__ double red[2][DG_WAVES];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * plane;
  const float* ex = exclude ? exclude + (int64_t)blockIdx.y * exclude_stride : nullptr;
  const int64_t lo = (int64_t)blockIdx.x * DG_CHUNK;
  const int64_t hi = lo + DG_CHUNK < plane ? lo + DG_CHUNK : plane;
  double sum = 0.0, cnt = 0.0;
  for (int64_t i = lo + tid; i < hi; i += DG_THREADS) {
    const float e = est[base + i], g = gt[base + i];
    const bool ok = fabsf(e) < INFINITY && g > 0.f && !(ex && ex[i] == 1.f);  // |NaN| < inf is false
    if (ok) {
      sum += (double)(fabsf(g - e) / g);  // the term in fp32, as the reference
      cnt += 1.0;
    }
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sum;
    red[1][tid >> 6] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double s = red[0][0], c = red[1][0];
#pragma unroll
    for (int k = 1; k < DG_WAVES; ++k) {
      s += red[0][k];
      c += red[1][k];
    }
    double* o = partial + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = s;
    o[1] = c;
  }
}

// out[b] = {sum, count} from the image's partials, added in index order.
__global__ __launch_bounds__(DG_THREADS) void dg_abs_rel_final_kernel(int64_t chunks,
                                                                      const double* __restrict__ partial,
                                                                      double* __restrict__ out) {
  __shared__ double red[2][DG_THREADS];
  const int tid = threadIdx.x;
  const double* p = partial + 2 * chunks * (int64_t)blockIdx.x;
  double s = 0.0, c = 0.0;
  for (int64_t i = tid; i < chunks; i += DG_THREADS) {
    s += p[2 * i];
    c += p[2 * i + 1];
  }
  red[0][tid] = s;
  red[1][tid] = c;
  __syncthreads();
  for (int k = DG_THREADS / 2; k > 0; k >>= 1) {
    if (tid < k) {
      red[0][tid] += red[0][tid + k];
      red[1][tid] += red[1][tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[2 * (int64_t)blockIdx.x] = red[0][0];
    out[2 * (int64_t)blockIdx.x + 1] = red[1][0];
  }
}

// (x, y) of pixel i of image b: its (column, row), or xy[b][i] when given
__device__ inline void pixel_xy(const float* __restrict__ xy, int64_t g, int64_t i, int W, float& x, float& y) {
  if (xy) {
    x = xy[2 * g];
    y = xy[2 * g + 1];
  } else {
    const int64_t r = i / W;
    x = (float)(i - r * W);
    y = (float)r;
  }
}

__global__ __launch_bounds__(DG_THREADS) void dg_unproject_kernel(int64_t plane, int W,
                                                                  const float* __restrict__ depth,
                                                                  const float* __restrict__ xy,
                                                                  const float* __restrict__ Kinv,
                                                                  const float* __restrict__ c2w,
                                                                  float* __restrict__ xyz) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (i >= plane) return;
  const int64_t g = (int64_t)b * plane + i;
  float x, y, rx, ry, rz, wx, wy, wz;
  pixel_xy(xy, g, i, W, x, y);
  mul3(Kinv + 9 * b, x, y, 1.f, rx, ry, rz);
  const float d = depth[g];
  affine(c2w + 16 * b, d * rx, d * ry, d * rz, wx, wy, wz);
  xyz[3 * g] = wx;
  xyz[3 * g + 1] = wy;
  xyz[3 * g + 2] = wz;
}

__global__ __launch_bounds__(DG_THREADS) void dg_flow_kernel(int64_t plane, int W, const float* __restrict__ depth1,
                                                             const float* __restrict__ Kinv1,
                                                             const float* __restrict__ T,
                                                             const float* __restrict__ K2, float* __restrict__ flow,
                                                             uint8_t* __restrict__ valid) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (i >= plane) return;
  const int64_t g = (int64_t)b * plane + i;
  float x, y, rx, ry, rz, cx, cy, cz, qx, qy, qz;
  pixel_xy(nullptr, g, i, W, x, y);
  mul3(Kinv1 + 9 * b, x, y, 1.f, rx, ry, rz);
  const float d = depth1[g];
  affine(T + 16 * b, d * rx, d * ry, d * rz, cx, cy, cz);
  mul3(K2 + 9 * b, cx, cy, cz, qx, qy, qz);
  const float den = qz < 1e-7f ? 1e-7f : qz;  // clamp(min=1e-7); a NaN stays a NaN
  flow[2 * (int64_t)b * plane + i] = qx / den - x;
  flow[(2 * (int64_t)b + 1) * plane + i] = qy / den - y;
  if (valid) valid[g] = (d > 0.f && qz > 1e-7f) ? 1 : 0;
}

struct SampleArgs {
  int Ch, H, W, w, mode, add;
  int64_t N;
  const float* src;
  const float* coords;
  float* out;
};

// clamp to [0, hi] with comparisons: a NaN passes through
__device__ inline float clamp_keep_nan(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

__global__ __launch_bounds__(DG_THREADS) void dg_sample_kernel(SampleArgs a) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (n >= a.N) return;
  float x, y, dx = 0.f, dy = 0.f;
  if (a.mode == GS_SAMPLE_POINTS) {
    const float* c = a.coords + 2 * ((int64_t)b * a.N + n);
    x = c[0];
    y = c[1];
  } else {
    const int64_t r = n / a.w;
    dx = a.coords[2 * (int64_t)b * a.N + n];
    dy = a.coords[(2 * (int64_t)b + 1) * a.N + n];
    x = (float)(n - r * a.w) + dx;
    y = (float)r + dy;
  }
  const bool bad = !(x == x) || !(y == y);  // a NaN coordinate: address pixel (0, 0), write NaN
  x = bad ? 0.f : clamp_keep_nan(x, (float)(a.W - 1));
  y = bad ? 0.f : clamp_keep_nan(y, (float)(a.H - 1));
  // x in [0, W - 1] here, so the conversions are in range
  int x0 = (int)floorf(x), y0 = (int)floorf(y);
  x0 = a.W > 1 ? (x0 < a.W - 2 ? x0 : a.W - 2) : 0;
  y0 = a.H > 1 ? (y0 < a.H - 2 ? y0 : a.H - 2) : 0;
  const int sx = a.W > 1 ? 1 : 0;
  const int64_t sy = a.H > 1 ? a.W : 0;
  const float tx = x - (float)x0, ty = y - (float)y0;
  const float w00 = (1.f - tx) * (1.f - ty), w01 = tx * (1.f - ty), w10 = (1.f - tx) * ty, w11 = tx * ty;
  const int64_t plane = (int64_t)a.H * a.W;
  const float* s = a.src + (int64_t)b * a.Ch * plane + (int64_t)y0 * a.W + x0;
  float* o = a.out + (int64_t)b * a.Ch * a.N + n;
  for (int ch = 0; ch < a.Ch; ++ch, s += plane, o += a.N) {
    float v = s[0] * w00 + s[sx] * w01 + s[sy] * w10 + s[sy + sx] * w11;
    if (a.add) v = (ch == 0 ? dx : dy) + v;
    *o = bad ? NAN : v;
  }
}

}  // namespace

extern "C" {

int gs_point_depth(const struct gs_point_depth* args, gs_stream_t stream) {
  if (int e = gs_point_depth_validate(args)) return e;
  const struct gs_point_depth& a = *args;
  hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)a.H * a.W;
  uint32_t* bits = reinterpret_cast<uint32_t*>(a.depth);
  hipLaunchKernelGGL(dg_fill_inf_kernel, dim3((unsigned)dg_blocks(plane), (unsigned)a.B), dim3(DG_THREADS), 0, s,
                     plane, bits);
  if (a.P > 0)
    hipLaunchKernelGGL(dg_point_depth_kernel, dim3((unsigned)dg_blocks(a.P), (unsigned)a.B), dim3(DG_THREADS), 0, s,
                       a.P, a.H, a.W, a.points, a.points_batch_stride, a.w2c, a.K, bits);
  return launch_status("point depth", 0, s);
}

int gs_depth_abs_rel(const struct gs_depth_abs_rel* args, gs_stream_t stream) {
  if (int e = gs_depth_abs_rel_validate(args)) return e;
  const struct gs_depth_abs_rel& a = *args;
  const DepthAbsRelLayout L(a.B, a.H, a.W);
  hipStream_t s = (hipStream_t)stream;
  double* partial = at<double>(a.workspace, L.partial);
  hipLaunchKernelGGL(dg_abs_rel_kernel, dim3((unsigned)L.chunks, (unsigned)a.B), dim3(DG_THREADS), 0, s,
                     L.plane_elems, a.est, a.gt, a.exclude, a.exclude ? a.exclude_batch_stride : 0, partial);
  hipLaunchKernelGGL(dg_abs_rel_final_kernel, dim3((unsigned)a.B), dim3(DG_THREADS), 0, s, L.chunks, partial, a.out);
  return launch_status("depth abs-rel", 0, s);
}

int gs_depth_unproject(const struct gs_depth_unproject* args, gs_stream_t stream) {
  if (int e = gs_depth_unproject_validate(args)) return e;
  const struct gs_depth_unproject& a = *args;
  hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)a.H * a.W;
  hipLaunchKernelGGL(dg_unproject_kernel, dim3((unsigned)dg_blocks(plane), (unsigned)a.B), dim3(DG_THREADS), 0, s,
                     plane, a.W, a.depth, a.xy, a.Kinv, a.c2w, a.xyz);
  return launch_status("depth unproject", 0, s);
}

int gs_depth_flow(const struct gs_depth_flow* args, gs_stream_t stream) {
  if (int e = gs_depth_flow_validate(args)) return e;
  const struct gs_depth_flow& a = *args;
  hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)a.H * a.W;
  hipLaunchKernelGGL(dg_flow_kernel, dim3((unsigned)dg_blocks(plane), (unsigned)a.B), dim3(DG_THREADS), 0, s, plane,
                     a.W, a.depth1, a.Kinv1, a.T, a.K2, a.flow, a.valid);
  return launch_status("depth flow", 0, s);
}

int gs_sample_bilinear(const struct gs_sample_bilinear* args, gs_stream_t stream) {
  if (int e = gs_sample_bilinear_validate(args)) return e;
  const struct gs_sample_bilinear& a = *args;
  hipStream_t s = (hipStream_t)stream;
  SampleArgs k{};
  k.Ch = a.Ch;
  k.H = a.H;
  k.W = a.W;
  k.w = a.mode == GS_SAMPLE_DISPLACEMENT ? a.w : 1;
  k.mode = a.mode;
  k.add = a.add_displacement ? 1 : 0;
  k.N = a.N;
  k.src = a.src;
  k.coords = a.coords;
  k.out = a.out;
  hipLaunchKernelGGL(dg_sample_kernel, dim3((unsigned)dg_blocks(a.N), (unsigned)a.B), dim3(DG_THREADS), 0, s, k);
  return launch_status("sample bilinear", 0, s);
}

}  // extern "C"
