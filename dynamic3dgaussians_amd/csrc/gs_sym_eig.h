// gs_sym_eig.h -- cyclic Jacobi in fp64 for a symmetric matrix of runtime
// order (include/gs_feature_pca.h: fit).  Written for one workgroup: every
// routine is called by all `nt` threads of the group with their index `tid`,
// and EIG_SYNC() separates the phases.  The same text compiles for the host
// with nt = 1 and an empty EIG_SYNC, as gs_motion_init_solve.h does.
//
// The order is padded to an even ne (a zero row and column, which no rotation
// ever touches: its off-diagonal entries stay exactly 0).  A sweep is ne - 1
// steps of the round-robin ordering: step s pairs (ne - 1, s) and, for
// k = 1 .. ne/2 - 1, ((s + k) mod (ne - 1), (s - k) mod (ne - 1)), so the ne/2
// rotations of a step touch disjoint rows and columns and commute.  A step is
//   1. a thread per pair: the rotation (c, s, t) that annihilates A[p][q];
//   2. a thread per pair of pairs (a <= b): the 2 x 2 block A[{pa,qa}][{pb,qb}]
//      becomes Ja^T (block) Jb and is also written transposed, so A stays
//      bit-symmetric; a thread per (pair, entry): the two eigenvector rows of V.
// The sweep loop ends at the compile-time cap or when off(A)^2 <= 2^-104 ||A||_F^2.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_EIG_HD __host__ __device__ inline
#else
#define GS_EIG_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define EIG_SYNC() __syncthreads()
#else
#define EIG_SYNC() ((void)0)
#endif

namespace gs {

struct SymEigScratch {
  double* rot;   // [3 * ne/2]: c, s, t of the step's pairs
  int* pq;       // [2 * ne/2]: p < q of the step's pairs; later [ne]: the sorted order
  double* red;   // [2 * nt]: per-thread partial norms
  int64_t rotations;  // non-trivial rotations applied (thread 0's count is the total on the host)
};

enum { SYM_EIG_NOT_FINITE = -2 };

GS_EIG_HD void sym_eig_pair(int ne, int step, int k, int& p, int& q) {
  const int n1 = ne - 1;
  int i, j;
  if (k == 0) {
    i = n1;
    j = step;
  } else {
    i = (step + k) % n1;
    j = (step + n1 - k) % n1;
  }
  p = i < j ? i : j;
  q = i < j ? j : i;
}

// A [ne, ne] (leading dimension ld) symmetric on entry, diagonal (to the
// tolerance) on exit; V [ne, ne] its eigenvectors in rows (a rotation updates two rows of V, so
// the threads of a row walk consecutive addresses).  An odd ld keeps the
// transposed writes of A off one LDS bank.  Returns the
// number of sweeps run, -1 when `max_sweeps` were run without reaching the
// tolerance, or SYM_EIG_NOT_FINITE when ||A||_F^2 is NaN or infinite (an entry
// is, or the squares overflow): nothing is rotated then.
GS_EIG_HD int sym_eig_jacobi(int ne, double* A, double* V, int ld, SymEigScratch& w, int max_sweeps, int tid, int nt) {
  const int m = ne / 2;
  for (int e = tid; e < ne * ne; e += nt) V[(e / ne) * ld + e % ne] = e / ne == e % ne ? 1.0 : 0.0;
  w.rotations = 0;
  EIG_SYNC();
  int sweeps = -1;
  for (int sweep = 0; sweep <= max_sweeps; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int e = tid; e < ne * ne; e += nt) {
      const double v = A[(e / ne) * ld + e % ne];
      all += v * v;
      if (e / ne != e % ne) off += v * v;
    }
    w.red[2 * tid] = off;
    w.red[2 * tid + 1] = all;
    EIG_SYNC();
    off = 0.0;
    all = 0.0;
    for (int i = 0; i < nt; ++i) {  // every thread the same sums in the same order
      off += w.red[2 * i];
      all += w.red[2 * i + 1];
    }
    EIG_SYNC();
    if (!(all <= 1.7976931348623157e308)) {  // NaN or infinite: every thread sees the same sums
      sweeps = SYM_EIG_NOT_FINITE;
      break;
    }
    if (!(off > 0x1p-104 * all)) {
      sweeps = sweep;
      break;
    }
    if (sweep == max_sweeps) break;
    for (int step = 0; step < ne - 1; ++step) {
      for (int k = tid; k < m; k += nt) {
        int p, q;
        sym_eig_pair(ne, step, k, p, q);
        const double apq = A[p * ld + q];
        double c = 1.0, s = 0.0, t = 0.0;
        if (apq != 0.0) {
          const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
          // |theta| beyond 1e150 would overflow its square: t = 1 / (2 theta) there
          const double at = fabs(theta);
          t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
          if (theta < 0.0) t = -t;
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
          ++w.rotations;
        }
        w.rot[3 * k] = c;
        w.rot[3 * k + 1] = s;
        w.rot[3 * k + 2] = t;
        w.pq[2 * k] = p;
        w.pq[2 * k + 1] = q;
      }
      EIG_SYNC();
      for (int e = tid; e < m * m; e += nt) {
        const int a = e / m, b = e % m;
        if (a > b) continue;
        const int pa = w.pq[2 * a], qa = w.pq[2 * a + 1];
        const double ca = w.rot[3 * a], sa = w.rot[3 * a + 1];
        if (a == b) {
          const double apq = A[pa * ld + qa], t = w.rot[3 * a + 2];
          A[pa * ld + pa] = A[pa * ld + pa] - t * apq;
          A[qa * ld + qa] = A[qa * ld + qa] + t * apq;
          A[pa * ld + qa] = 0.0;
          A[qa * ld + pa] = 0.0;
          continue;
        }
        const int pb = w.pq[2 * b], qb = w.pq[2 * b + 1];
        const double cb = w.rot[3 * b], sb = w.rot[3 * b + 1];
        const double x00 = A[pa * ld + pb], x01 = A[pa * ld + qb], x10 = A[qa * ld + pb], x11 = A[qa * ld + qb];
        // columns by Jb, then rows by Ja^T
        const double y00 = cb * x00 - sb * x01, y01 = sb * x00 + cb * x01;
        const double y10 = cb * x10 - sb * x11, y11 = sb * x10 + cb * x11;
        const double z00 = ca * y00 - sa * y10, z10 = sa * y00 + ca * y10;
        const double z01 = ca * y01 - sa * y11, z11 = sa * y01 + ca * y11;
        A[pa * ld + pb] = z00; A[pb * ld + pa] = z00;
        A[pa * ld + qb] = z01; A[qb * ld + pa] = z01;
        A[qa * ld + pb] = z10; A[pb * ld + qa] = z10;
        A[qa * ld + qb] = z11; A[qb * ld + qa] = z11;
      }
      for (int e = tid; e < m * ne; e += nt) {
        const int k = e / ne, r = e % ne;
        const int p = w.pq[2 * k], q = w.pq[2 * k + 1];
        const double c = w.rot[3 * k], s = w.rot[3 * k + 1];
        const double vp = V[p * ld + r], vq = V[q * ld + r];  // consecutive threads, consecutive addresses
        V[p * ld + r] = c * vp - s * vq;
        V[q * ld + r] = s * vp + c * vq;
      }
      EIG_SYNC();
    }
  }
  return sweeps;
}

// The eigenpairs of the first n (<= ne) indices in fit's order: descending
// eigenvalue, ties by index; every eigenvector signed so that its entry of
// largest magnitude is positive (the lowest index on a tie).  evals [n],
// evecs [n, n] with row j the j-th eigenvector.  `zero` (uniform over the
// threads): write zeros instead, reading neither A nor V.
GS_EIG_HD void sym_eig_sorted(int n, const double* A, const double* V, int ld, SymEigScratch& w, double* evals,
                              double* evecs, bool zero, int tid, int nt) {
  if (zero) {
    for (int e = tid; e < n * n; e += nt) evecs[e] = 0.0;
    for (int e = tid; e < n; e += nt) evals[e] = 0.0;
    EIG_SYNC();
    return;
  }
  for (int i = tid; i < n; i += nt) w.pq[i] = i;  // the ranks are a permutation for finite eigenvalues
  EIG_SYNC();
  for (int i = tid; i < n; i += nt) {
    const double li = A[i * ld + i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double lj = A[j * ld + j];
      rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
    }
    w.pq[rank] = i;
  }
  EIG_SYNC();
  for (int j = tid; j < n; j += nt) {
    const int i = w.pq[j];
    double best = -1.0, sign = 1.0;
    for (int c = 0; c < n; ++c) {
      const double v = V[i * ld + c];
      if (fabs(v) > best) {
        best = fabs(v);
        sign = v < 0.0 ? -1.0 : 1.0;
      }
    }
    evals[j] = A[i * ld + i];
    for (int c = 0; c < n; ++c) evecs[j * n + c] = sign * V[i * ld + c];
  }
  EIG_SYNC();
}

}  // namespace gs
