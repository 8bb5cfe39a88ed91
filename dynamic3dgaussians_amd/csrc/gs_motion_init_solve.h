// gs_motion_init_solve.h -- the weighted Procrustes solve of one (basis,
// frame) from its 19 fp64 moments (include/gs_motion_init.h): Horn's
// symmetric 4 x 4 matrix of the centred cross-covariance and its largest
// eigenvector by cyclic Jacobi sweeps.  Plain C++ in fp64 with every loop of
// constant extent, so the 4 x 4 matrices stay in registers on the device; the
// same text compiles for the host.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define GS_MI_HD __host__ __device__ inline
#else
#define GS_MI_HD inline
#endif

namespace gs {

// Order of the moments of one (basis, frame).
enum { MI_W = 0, MI_S = 1, MI_G = 4, MI_SG = 7, MI_SS = 16, MI_GG = 17, MI_DD = 18 };

struct ProcrustesSolution {
  double q[4];     // unit quaternion (w, x, y, z)
  double R[3][3];  // its rotation: g ~ R s + t
  double t[3];
  double err_after, err_before;
};

// One Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into V's columns.
template <int P, int Q>
GS_MI_HD void mi_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  // |theta| beyond 1e150 would overflow its square: t = 1 / (2 theta) there
  const double at = fabs(theta);
  double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double arp = A[r][P], arq = A[r][Q];
    A[r][P] = c * arp - s * arq;
    A[r][Q] = s * arp + c * arq;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double apr = A[P][r], aqr = A[Q][r];
    A[P][r] = c * apr - s * aqr;
    A[Q][r] = s * apr + c * aqr;
  }
  A[P][Q] = 0.0;
  A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = c * vrp - s * vrq;
    V[r][Q] = s * vrp + c * vrq;
  }
}

// m: the 19 moments with m[MI_W] > 0.  Finite for finite moments; R is a proper rotation
// whatever the rank of the points (a zero covariance gives the identity).
GS_MI_HD void mi_procrustes_solve(const double* m, ProcrustesSolution& o) {
  const double W = m[MI_W], inv = 1.0 / W;
  double cs[3], cg[3], C[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] = m[MI_S + a] * inv;
    cg[a] = m[MI_G + a] * inv;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a][b] = m[MI_SG + 3 * a + b] * inv - cs[a] * cg[b];  // sum w (s - cs)_a (g - cg)_b / W

  double A[4][4], V[4][4];
  A[0][0] = C[0][0] + C[1][1] + C[2][2];
  A[1][1] = C[0][0] - C[1][1] - C[2][2];
  A[2][2] = -C[0][0] + C[1][1] - C[2][2];
  A[3][3] = -C[0][0] - C[1][1] + C[2][2];
  A[0][1] = A[1][0] = C[1][2] - C[2][1];
  A[0][2] = A[2][0] = C[2][0] - C[0][2];
  A[0][3] = A[3][0] = C[0][1] - C[1][0];
  A[1][2] = A[2][1] = C[0][1] + C[1][0];
  A[1][3] = A[3][1] = C[2][0] + C[0][2];
  A[2][3] = A[3][2] = C[1][2] + C[2][1];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;

  for (int sweep = 0; sweep < 24; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] +
                       A[1][3] * A[1][3] + A[2][3] * A[2][3];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
    if (!(off > 1e-40 * diag)) break;  // also leaves on NaN
    mi_jacobi_rotate<0, 1>(A, V);
    mi_jacobi_rotate<0, 2>(A, V);
    mi_jacobi_rotate<0, 3>(A, V);
    mi_jacobi_rotate<1, 2>(A, V);
    mi_jacobi_rotate<1, 3>(A, V);
    mi_jacobi_rotate<2, 3>(A, V);
  }
  // the column of the largest eigenvalue, the first of equal ones
  double best = A[0][0];
  double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const bool take = A[c][c] > best;
    best = take ? A[c][c] : best;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = take ? V[r][c] : q[r];
  }
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(n > 0.0)) {  // never for finite moments: V stays orthogonal
    q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; n = 1.0;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) o.q[r] = q[r] / n;
  const double w = o.q[0], x = o.q[1], y = o.q[2], z = o.q[3];
  o.R[0][0] = 1.0 - 2.0 * (y * y + z * z); o.R[0][1] = 2.0 * (x * y - w * z); o.R[0][2] = 2.0 * (x * z + w * y);
  o.R[1][0] = 2.0 * (x * y + w * z); o.R[1][1] = 1.0 - 2.0 * (x * x + z * z); o.R[1][2] = 2.0 * (y * z - w * x);
  o.R[2][0] = 2.0 * (x * z - w * y); o.R[2][1] = 2.0 * (y * z + w * x); o.R[2][2] = 1.0 - 2.0 * (x * x + y * y);
  double cross = 0.0, ss = m[MI_SS] * inv, gg = m[MI_GG] * inv;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o.t[a] = cg[a] - (o.R[a][0] * cs[0] + o.R[a][1] * cs[1] + o.R[a][2] * cs[2]);
    ss -= cs[a] * cs[a];
    gg -= cg[a] * cg[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) cross += o.R[a][b] * C[b][a];
  }
  // sum w |R (s - cs) - (g - cg)|^2 / W, expanded
  const double ea = ss + gg - 2.0 * cross, eb = m[MI_DD] * inv;
  o.err_after = sqrt(ea > 0.0 ? ea : 0.0);
  o.err_before = sqrt(eb > 0.0 ? eb : 0.0);
}

}  // namespace gs
