// gs_project.h -- the projection pieces shared by the preprocess kernels
// (gs_preprocess.hip), the camera-gradient kernel (gs_camera_grad.hip) and the
// track projection (gs_track.hip): point transforms, the pixel convention, the
// EWA setup of computeCov2D and the SH constants.  These files are compiled
// with -ffp-contract=off, so every expression keeps the operation order of the
// CPU oracle (oracle/gs_oracle.c).
#pragma once

#include "gs_common.h"

namespace gs {

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f,
                SH_C2_2 = 0.31539156525252005f, SH_C2_3 = -1.0925484305920792f,
                SH_C2_4 = 0.5462742152960396f;
constexpr float SH_C3_0 = -0.5900435899266435f, SH_C3_1 = 2.890611442640554f,
                SH_C3_2 = -0.4570457994644658f, SH_C3_3 = 0.3731763325901154f,
                SH_C3_4 = -0.4570457994644658f, SH_C3_5 = 1.445305721320277f,
                SH_C3_6 = -0.5900435899266435f;

struct V3 { float x, y, z; };

__device__ inline V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }

// transformPoint4x3 (auxiliary.h:58-66); m = column-major 4x4.
__device__ inline V3 xf43(const float* __restrict__ m, V3 p) {
  return V3{m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
            m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
            m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]};
}
__device__ inline float4 xf44(const float* __restrict__ m, V3 p) {
  return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                     m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                     m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14],
                     m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

// ndc2Pix in double (double literals at auxiliary.h:43).
__device__ inline float ndc_to_pix(float v, int S) {
  return (float)((((double)v + 1.0) * (double)S - 1.0) * 0.5);
}

// Shared EWA setup (forward.cu:75-118 / backward.cu:166-211).
struct Ewa {
  float t[3], txtz, tytz, lxp, lxn, lyp, lyn;
  float a[2][3];
};
__device__ inline void ewa_setup(V3 mean, const float* __restrict__ view, int W, int H, float cx,
                                 float cy, float fx, float fy, float tfx, float tfy, Ewa& e) {
  V3 t = xf43(view, mean);
  e.lxp = ((float)W - cx) / fx + 0.3f * tfx;
  e.lxn = cx / fx + 0.3f * tfx;
  e.lyp = ((float)H - cy) / fy + 0.3f * tfy;
  e.lyn = cy / fy + 0.3f * tfy;
  e.txtz = t.x / t.z;
  e.tytz = t.y / t.z;
  t.x = fminf(e.lxp, fmaxf(-e.lxn, e.txtz)) * t.z;
  t.y = fminf(e.lyp, fmaxf(-e.lyn, e.tytz)) * t.z;
  e.t[0] = t.x; e.t[1] = t.y; e.t[2] = t.z;
  const float j00 = fx / t.z, j02 = -(fx * t.x) / (t.z * t.z);
  const float j11 = fy / t.z, j12 = -(fy * t.y) / (t.z * t.z);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    e.a[0][r] = view[4 * r] * j00 + view[1 + 4 * r] * 0.0f + view[2 + 4 * r] * j02;
    e.a[1][r] = view[4 * r] * 0.0f + view[1 + 4 * r] * j11 + view[2 + 4 * r] * j12;
  }
}
__device__ inline void ewa_cov2d(const Ewa& e, const float c3[6], float out[3]) {
  const float v[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
  float u[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      u[i][k] = e.a[i][0] * v[0][k] + e.a[i][1] * v[1][k] + e.a[i][2] * v[2][k];
  const float a = u[0][0] * e.a[0][0] + u[0][1] * e.a[0][1] + u[0][2] * e.a[0][2];
  const float b = u[1][0] * e.a[0][0] + u[1][1] * e.a[0][1] + u[1][2] * e.a[0][2];
  const float c = u[1][0] * e.a[1][0] + u[1][1] * e.a[1][1] + u[1][2] * e.a[1][2];
  out[0] = a + 0.3f; out[1] = b; out[2] = c + 0.3f;
}

}  // namespace gs
