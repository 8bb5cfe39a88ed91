// gs_spectral_small.h -- the order-B dense problems of the spectral embedding
// (include/gs_spectral.h): the SVQB transform of a Gram matrix, the
// Rayleigh-Ritz rotation of H = X^T S X, the coefficients of one step of the
// scaled Chebyshev filter and the counter-based start block.  Written for one
// workgroup on top of gs_sym_eig.h: every routine is called by all `nt`
// threads with their index `tid`.  The same text compiles for the host with
// nt = 1 (gs_spectral_host.cpp, tools/spectral_host_sanitize.c), as
// gs_motion_init_solve.h does.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gs_sym_eig.h"

namespace gs {

constexpr int SP_MAX_SWEEPS = 30;
constexpr double SP_RANK_TOL = 0x1p-40;  // a direction at or under SP_RANK_TOL * L_max is replaced
constexpr int sp_even(int B) { return B + (B & 1); }
constexpr int sp_ld(int B) { return sp_even(B) + 1; }  // odd: gs_sym_eig.h's transposed writes

GS_EIG_HD uint64_t sp_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// x(seed, e, i, j) of include/gs_spectral.h: in (-1, 1), never 0
GS_EIG_HD double sp_start(uint64_t seed, uint32_t epoch, int64_t i, int j) {
  const uint64_t h = sp_mix(sp_mix(seed + ((uint64_t)epoch + 1) * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)i * 128 + (uint64_t)j));
  return ((double)(h >> 12) + 0.5) * 0x1p-51 - 1.0;
}

GS_EIG_HD bool sp_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// SVQB: G [B, B] the Gram matrix X^T X (its upper triangle is read).  With
// D = diag(G) and D^-1/2 G D^-1/2 = Q L Q^T, T = D^-1/2 Q L^-1/2 makes
// (X T)^T (X T) = I.  A direction with L <= SP_RANK_TOL * L_max (a zero column
// of X among them) gets a zero column of T and replaced = 1.  A, V [ne, ld]
// work matrices, scale [ne]; T [B, B] and replaced [B] may be global memory.
GS_EIG_HD void sp_svqb(int B, const double* G, double* A, double* V, SymEigScratch& w, double* scale, double* T,
                       int32_t* replaced, int tid, int nt) {
  const int ne = sp_even(B), ld = sp_ld(B);
  for (int i = tid; i < ne; i += nt) {
    const double d = i < B ? G[i * B + i] : 0.0;
    scale[i] = d > 0.0 && sp_finite(d) ? 1.0 / sqrt(d) : 0.0;
  }
  EIG_SYNC();
  for (int e = tid; e < ne * ne; e += nt) {
    const int i = e / ne, j = e % ne;
    double v = 0.0;
    if (i < B && j < B) {
      if (i == j)
        v = scale[i] > 0.0 ? 1.0 : 0.0;
      else
        v = scale[i] * G[i < j ? i * B + j : j * B + i] * scale[j];
    }
    A[i * ld + j] = v;
  }
  EIG_SYNC();
  const int sweeps = sym_eig_jacobi(ne, A, V, ld, w, SP_MAX_SWEEPS, tid, nt);
  double lmax = 0.0;
  for (int k = 0; k < B; ++k) {  // every thread the same maximum
    const double l = A[k * ld + k];
    if (l > lmax) lmax = l;
  }
  for (int k = tid; k < B; k += nt) {
    const double l = A[k * ld + k];
    const bool ok = sweeps != SYM_EIG_NOT_FINITE && lmax > 0.0 && sp_finite(l) && l > SP_RANK_TOL * lmax;
    replaced[k] = ok ? 0 : 1;
    const double inv = ok ? 1.0 / sqrt(l) : 0.0;
    for (int i = 0; i < B; ++i) T[i * B + k] = ok ? scale[i] * V[k * ld + i] * inv : 0.0;
  }
  EIG_SYNC();
}

// Rayleigh-Ritz: H [B, B] = X^T (S X), symmetrised by reading each pair once
// from the upper triangle.  theta [B] descending (ties by index), Q [B, B]
// with column j the j-th Ritz vector; evecs [B, B] is scratch.  Zeros when H
// is not finite.
GS_EIG_HD void sp_ritz(int B, const double* H, double* A, double* V, SymEigScratch& w, double* evecs, double* theta,
                       double* Q, int tid, int nt) {
  const int ne = sp_even(B), ld = sp_ld(B);
  for (int e = tid; e < ne * ne; e += nt) {
    const int i = e / ne, j = e % ne;
    A[i * ld + j] = i < B && j < B ? H[i < j ? i * B + j : j * B + i] : 0.0;
  }
  EIG_SYNC();
  const int sweeps = sym_eig_jacobi(ne, A, V, ld, w, SP_MAX_SWEEPS, tid, nt);
  sym_eig_sorted(B, A, V, ld, w, theta, evecs, sweeps == SYM_EIG_NOT_FINITE, tid, nt);
  for (int e = tid; e < B * B; e += nt) Q[(e % B) * B + e / B] = evecs[e];
  EIG_SYNC();
}

// Step s (1 .. m) of the scaled Chebyshev filter that damps [-1, theta_B] and
// is scaled at theta_1 (Zhou and Saad's three-term form: no coefficient
// grows with the degree): Y_s = alpha (S Y_{s-1}) + beta Y_{s-1} + gamma Y_{s-2},
// Y_0 = X.  The damped interval is never narrower than 2^-10.
struct ChebStep {
  double alpha, beta, gamma;
};
GS_EIG_HD ChebStep sp_cheb_step(double theta_1, double theta_B, int s) {
  const double a = -1.0;
  double b = theta_B;
  if (!(b > a + 0x1p-10)) b = a + 0x1p-10;
  if (!(b < 1.0)) b = 1.0;
  double a0 = theta_1;
  if (!(a0 > b)) a0 = b;
  if (!(a0 < 1.0)) a0 = 1.0;
  const double e = (b - a) / 2.0, c = (b + a) / 2.0;
  double sigma = e / (a0 - c);  // a0 - c >= e > 0: sigma in (0, 1]
  const double tau = 2.0 / sigma;
  ChebStep r;
  r.alpha = sigma / e;
  r.beta = -c * r.alpha;
  r.gamma = 0.0;
  for (int i = 2; i <= s; ++i) {
    const double sn = 1.0 / (tau - sigma);  // tau - sigma >= 1
    r.alpha = 2.0 * sn / e;
    r.beta = -c * r.alpha;
    r.gamma = -sigma * sn;
    sigma = sn;
  }
  return r;
}

}  // namespace gs
