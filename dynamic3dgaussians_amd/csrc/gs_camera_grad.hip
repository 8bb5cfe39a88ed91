// gs_camera_grad.hip -- gradients of the cameras of a batch (view matrix,
// projection matrix, camera position; include/gs_camera_grad.h): the terms
// preprocess_bwd_kernel (gs_preprocess.hip) forms per (camera, Gaussian) pair,
// multiplied by the homogeneous mean and reduced over the Gaussians instead of
// multiplied by the camera and written per Gaussian.  No reference analogue.
//
// HBM-bound like the preprocess kernels: per visible pair the 64-B
// accumulation record, the conic (a 64-B render-record line), radius, mean
// and 3D covariance, ~100 B per pair of which the radius (4 B) is read for
// the culled pairs too.
//
// Compiled with -ffp-contract=off: the per-pair terms follow
// preprocess_bwd_kernel's operation order in fp32 (they are the same
// numbers); only their products with the mean and the sums are fp64.
//
// Reduction, fixed order and no atomics: a thread adds its CG_ITEMS pairs in
// fp64 registers, wave_sum over the wave, the four waves in order through
// LDS, one fp64 record per (camera, workgroup); camera_grad_finish_kernel adds
// a camera's records in index order and rounds once to fp32.
#include "gs_camera_grad_layout.h"
#include "gs_common.h"
#include "gs_kernels.h"
#include "gs_project.h"

namespace gs {

// The view-direction part of computeColorFromSH's backward (backward.cu:20-139,
// sh_bwd in gs_preprocess.hip without the coefficient gradients): dL/dmean
// through dir = (mean - campos) / |mean - campos|; dL/dcampos is its negative.
__device__ inline void sh_dir_grad(int deg, int M, V3 mean, V3 cp, const float* __restrict__ shs, int g,
                                   uint8_t clampbits, const float dcolor[3], float dmean[3]) {
  const float dox = mean.x - cp.x, doy = mean.y - cp.y, doz = mean.z - cp.z;
  const float len = sqrtf(dox * dox + doy * doy + doz * doz);
  const float x = dox / len, y = doy / len, z = doz / len;
  const float* sh = shs + (size_t)g * M * 3;
  float dRGB[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) dRGB[ch] = dcolor[ch] * (((clampbits >> ch) & 1) ? 0.0f : 1.0f);
  float ddx[3] = {0, 0, 0}, ddy[3] = {0, 0, 0}, ddz[3] = {0, 0, 0};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#define S(i) sh[3 * (i) + ch]
    if (deg > 0) {
      ddx[ch] = -SH_C1 * S(3); ddy[ch] = -SH_C1 * S(1); ddz[ch] = SH_C1 * S(2);
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        ddx[ch] += SH_C2_0 * y * S(4) + SH_C2_2 * 2.f * -x * S(6) + SH_C2_3 * z * S(7) + SH_C2_4 * 2.f * x * S(8);
        ddy[ch] += SH_C2_0 * x * S(4) + SH_C2_1 * z * S(5) + SH_C2_2 * 2.f * -y * S(6) + SH_C2_4 * 2.f * -y * S(8);
        ddz[ch] += SH_C2_1 * y * S(5) + SH_C2_2 * 2.f * 2.f * z * S(6) + SH_C2_3 * x * S(7);
        if (deg > 2) {
          ddx[ch] += (SH_C3_0 * S(9) * 3.f * 2.f * xy + SH_C3_1 * S(10) * yz + SH_C3_2 * S(11) * -2.f * xy +
                      SH_C3_3 * S(12) * -3.f * 2.f * xz + SH_C3_4 * S(13) * (-3.f * xx + 4.f * zz - yy) +
                      SH_C3_5 * S(14) * 2.f * xz + SH_C3_6 * S(15) * 3.f * (xx - yy));
          ddy[ch] += (SH_C3_0 * S(9) * 3.f * (xx - yy) + SH_C3_1 * S(10) * xz +
                      SH_C3_2 * S(11) * (-3.f * yy + 4.f * zz - xx) + SH_C3_3 * S(12) * -3.f * 2.f * yz +
                      SH_C3_4 * S(13) * -2.f * xy + SH_C3_5 * S(14) * -2.f * yz + SH_C3_6 * S(15) * -3.f * 2.f * xy);
          ddz[ch] += (SH_C3_1 * S(10) * xy + SH_C3_2 * S(11) * 4.f * 2.f * yz +
                      SH_C3_3 * S(12) * 3.f * (2.f * zz - xx - yy) + SH_C3_4 * S(13) * 4.f * 2.f * xz +
                      SH_C3_5 * S(14) * (xx - yy));
        }
      }
    }
#undef S
  }
  const float dd0 = ddx[0] * dRGB[0] + ddx[1] * dRGB[1] + ddx[2] * dRGB[2];
  const float dd1 = ddy[0] * dRGB[0] + ddy[1] * dRGB[1] + ddy[2] * dRGB[2];
  const float dd2 = ddz[0] * dRGB[0] + ddz[1] * dRGB[1] + ddz[2] * dRGB[2];
  // dnormvdv (auxiliary.h:107-117)
  const float s2 = dox * dox + doy * doy + doz * doz;
  const float inv = 1.0f / sqrtf(s2 * s2 * s2);
  dmean[0] = ((s2 - dox * dox) * dd0 - doy * dox * dd1 - doz * dox * dd2) * inv;
  dmean[1] = (-dox * doy * dd0 + (s2 - doy * doy) * dd1 - doz * doy * dd2) * inv;
  dmean[2] = (-dox * doz * dd0 - doy * doz * dd1 + (s2 - doz * doz) * dd2) * inv;
}

// Grid (chunks of CG_CHUNK Gaussians) x C.  SH: the view-direction term is
// compiled in (launched when a.shs is set with degree > 0).
template <bool SH>
__global__ __launch_bounds__(CG_THREADS) void camera_grad_kernel(CameraGradArgs a, CamBatch cb) {
  const int c = blockIdx.y, tid = threadIdx.x;
  const float* __restrict__ v = cb.view + 16 * c;
  const float* __restrict__ pr = cb.proj + 16 * c;
  const float c_x = cb.c_x[c], c_y = cb.c_y[c], tan_fovx = cb.tanx[c], tan_fovy = cb.tany[c];
  const float hy = (float)a.H / (2.0f * tan_fovy);  // CR/rasterizer_impl.cu:398-399
  const float hx = (float)a.W / (2.0f * tan_fovx);
  const float* __restrict__ recs = shift_bytes(a.rec, c * cb.geom_stride);
  // sv[3 i + j]: dL_dview[4 i + j], j = 0..2; sp[3 i + k]: dL_dproj[4 i + (0, 1, 3)[k]]
  double sv[CG_VIEW], sp[CG_PROJ], sc[CG_POS];
#pragma unroll
  for (int i = 0; i < CG_VIEW; ++i) sv[i] = 0.0;
#pragma unroll
  for (int i = 0; i < CG_PROJ; ++i) sp[i] = 0.0;
#pragma unroll
  for (int i = 0; i < CG_POS; ++i) sc[i] = 0.0;
  for (int it = 0; it < CG_ITEMS; ++it) {
    const int64_t g64 = (int64_t)blockIdx.x * CG_CHUNK + it * CG_THREADS + tid;
    if (g64 >= a.P) break;
    const int g = (int)g64;
    if (a.radii[(size_t)c * a.P + g] <= 0) continue;
    const float* acc = a.acc + ((size_t)c * a.P + g) * ACC_STRIDE;
    const float* rec = recs + (size_t)REC * g;
    const float4 con = reinterpret_cast<const float4*>(rec)[0];  // x, y, a, b
    const float ccn = rec[R_CC];
    const V3 mean = ld3(a.means3D + mean_offset(cb, c, g));
    float c3v[6];
    {
      const float* c3 = a.cov3D_precomp ? a.cov3D_precomp + 6 * (size_t)g : a.cov3D + 6 * (size_t)g;
#pragma unroll
      for (int i = 0; i < 6; ++i) c3v[i] = c3[i];
    }
    // from here to dty: preprocess_bwd_kernel's expressions (compat = fixed)
    const float sex = acc[A_MX], sey = acc[A_MY];
    const float am0 = (-con.z * sex - con.w * sey) * (0.5f * (float)a.W);
    const float am1 = (-ccn * sey - con.w * sex) * (0.5f * (float)a.H);
    const float dcx = -0.5f * acc[A_CA], dcy = -0.5f * acc[A_CB], dcz = -0.5f * acc[A_CC];
    Ewa e;
    ewa_setup(mean, v, a.W, a.H, c_x, c_y, hx, hy, tan_fovx, tan_fovy, e);
    const float xg = (e.txtz < -e.lxn || e.txtz > e.lxp) ? 0.f : 1.f;
    const float yg = (e.tytz < -e.lyn || e.tytz > e.lyp) ? 0.f : 1.f;
    float cov[3];
    ewa_cov2d(e, c3v, cov);
    const float ca = cov[0], cb2 = cov[1], cc = cov[2];
    const float denom = ca * cc - cb2 * cb2;
    float da = 0, db = 0, dc = 0;
    const float d2inv = 1.0f / ((denom * denom) + 0.0000001f);
    const float(&A)[2][3] = e.a;
    if (d2inv != 0) {
      da = d2inv * (-cc * cc * dcx + 2 * cb2 * cc * dcy + (denom - ca * cc) * dcz);
      dc = d2inv * (-ca * ca * dcz + 2 * ca * cb2 * dcy + (denom - ca * cc) * dcx);
      db = d2inv * 2 * (cb2 * cc * dcx - (denom + 2 * cb2 * cb2) * dcy + ca * cb2 * dcz);
    }
    const float V[3][3] = {{c3v[0], c3v[1], c3v[2]}, {c3v[1], c3v[3], c3v[4]}, {c3v[2], c3v[4], c3v[5]}};
    float dT0[3], dT1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float r0 = A[0][0] * V[k][0] + A[0][1] * V[k][1] + A[0][2] * V[k][2];
      const float r1 = A[1][0] * V[k][0] + A[1][1] * V[k][1] + A[1][2] * V[k][2];
      dT0[k] = 2 * r0 * da + r1 * db;
      dT1[k] = 2 * r1 * dc + r0 * db;
    }
    const float dJ00 = v[0] * dT0[0] + v[4] * dT0[1] + v[8] * dT0[2];
    const float dJ02 = v[2] * dT0[0] + v[6] * dT0[1] + v[10] * dT0[2];
    const float dJ11 = v[1] * dT1[0] + v[5] * dT1[1] + v[9] * dT1[2];
    const float dJ12 = v[2] * dT1[0] + v[6] * dT1[1] + v[10] * dT1[2];
    const float tz = 1.f / e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    const float dtx = xg * -hx * tz2 * dJ02;
    const float dty = yg * -hy * tz2 * dJ12;
    // A coordinate in the frustum clamp (Q9: t_x = limit * t_z) has j02 = -hx limit / t_z, whose t_z
    // derivative is ONE hx t_x / t_z^3, not the two of the unclamped -hx t_x / t_z^2: the exact
    // derivative, where preprocess_bwd_kernel keeps the reference's factor 2 for both (the same number
    // for every Gaussian inside the clamp).
    const float dtz = -hx * tz2 * dJ00 - hy * tz2 * dJ11 + ((1.f + xg) * hx * e.t[0]) * tz3 * dJ02 +
                      ((1.f + yg) * hy * e.t[1]) * tz3 * dJ12;
    // the camera's side of the chain rule, in fp64
    const double p[4] = {(double)mean.x, (double)mean.y, (double)mean.z, 1.0};
    // view, through t = p V (the depth is t_2)
    const double dt[3] = {(double)dtx, (double)dty, (double)dtz + (double)acc[A_DEPTH]};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) sv[3 * i + j] += p[i] * dt[j];
    // view, through the EWA rows a0[r] = v[4r] j00 + v[4r+2] j02, a1[r] = v[4r+1] j11 + v[4r+2] j12
    // (ewa_setup's J entries, recomputed from its clamped t)
    const double j00 = hx / e.t[2], j02 = -(hx * e.t[0]) / (e.t[2] * e.t[2]);
    const double j11 = hy / e.t[2], j12 = -(hy * e.t[1]) / (e.t[2] * e.t[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      sv[3 * r + 0] += j00 * (double)dT0[r];
      sv[3 * r + 1] += j11 * (double)dT1[r];
      sv[3 * r + 2] += j02 * (double)dT0[r] + j12 * (double)dT1[r];
    }
    // projection, through the NDC mean (h_0, h_1) / (h_3 + 1e-7)
    const float4 mh = xf44(pr, mean);
    const double mw = 1.0f / (mh.w + 0.0000001f);
    const double g0 = mw * (double)am0, g1 = mw * (double)am1;
    const double g3 = -(mw * mw) * ((double)mh.x * (double)am0 + (double)mh.y * (double)am1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sp[3 * i + 0] += p[i] * g0;
      sp[3 * i + 1] += p[i] * g1;
      sp[3 * i + 2] += p[i] * g3;
    }
    if (SH) {
      const uint8_t* clamped = shift_bytes(a.clamped, c * cb.geom_stride);
      const float dcol[3] = {acc[A_R], acc[A_G], acc[A_B]};
      float dm[3];
      sh_dir_grad(a.D, a.M, mean, ld3(cb.campos + 3 * c), a.shs, g, clamped[g], dcol, dm);
#pragma unroll
      for (int i = 0; i < 3; ++i) sc[i] -= (double)dm[i];
    }
  }
  // the workgroup's record: lanes, then the four waves in order
  __shared__ double part[CG_THREADS / WAVE][CG_LIVE];
  const int wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
  for (int i = 0; i < CG_VIEW; ++i) {
    const double s = wave_sum(sv[i]);
    if (lane == 0) part[wave][i] = s;
  }
#pragma unroll
  for (int i = 0; i < CG_PROJ; ++i) {
    const double s = wave_sum(sp[i]);
    if (lane == 0) part[wave][CG_VIEW + i] = s;
  }
#pragma unroll
  for (int i = 0; i < CG_POS; ++i) {
    const double s = wave_sum(sc[i]);
    if (lane == 0) part[wave][CG_VIEW + CG_PROJ + i] = s;
  }
  __syncthreads();
  if (tid < CG_REC) {
    double s = 0.0;
    if (tid < CG_LIVE) {
      s = part[0][tid];
#pragma unroll
      for (int w = 1; w < CG_THREADS / WAVE; ++w) s += part[w][tid];
    }
    a.records[((size_t)c * gridDim.x + blockIdx.x) * CG_REC + tid] = s;
  }
}

// One wave per camera: lane l owns one output element (16 view, 16
// projection, 3 position), adds its component of the camera's `chunks`
// records in index order and rounds to fp32; the elements the forward does
// not read (view column 3, projection column 2) are zeros.
__global__ __launch_bounds__(WAVE) void camera_grad_finish_kernel(const double* __restrict__ records, int chunks,
                                                                  float* __restrict__ dview, float* __restrict__ dproj,
                                                                  float* __restrict__ dcampos) {
  const int c = blockIdx.x, l = threadIdx.x;
  int src = -1;
  float* dst = nullptr;
  if (l < 16) {
    const int i = l >> 2, j = l & 3;
    src = j < 3 ? 3 * i + j : -1;
    dst = dview + 16 * c + l;
  } else if (l < 32) {
    const int m = l - 16, i = m >> 2, j = m & 3;
    src = j == 2 ? -1 : CG_VIEW + 3 * i + (j == 3 ? 2 : j);
    dst = dproj + 16 * c + m;
  } else if (l < 32 + CG_POS) {
    src = CG_VIEW + CG_PROJ + (l - 32);
    dst = dcampos + 3 * c + (l - 32);
  }
  if (!dst) return;
  double s = 0.0;
  if (src >= 0) {
    const double* r = records + (size_t)c * chunks * CG_REC + src;
    for (int k = 0; k < chunks; ++k) s += r[(size_t)k * CG_REC];
  }
  *dst = (float)s;
}

void launch_camera_grad(const CameraGradArgs& a, const CamBatch& cb, hipStream_t s) {
  const int chunks = (int)camera_grad_chunks(a.P);
  if (chunks > 0) {
    const dim3 grid(chunks, cb.C), block(CG_THREADS);
    if (a.shs && a.D > 0) hipLaunchKernelGGL((camera_grad_kernel<true>), grid, block, 0, s, a, cb);
    else hipLaunchKernelGGL((camera_grad_kernel<false>), grid, block, 0, s, a, cb);
  }
  hipLaunchKernelGGL(camera_grad_finish_kernel, dim3(cb.C), dim3(WAVE), 0, s, a.records, chunks, a.dview, a.dproj,
                     a.dcampos);
}

}  // namespace gs
