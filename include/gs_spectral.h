/* gs_spectral.h -- C ABI of the spectral embedding of a sparse symmetric graph,
 * exported by the same libgsplat_hip.so as gsplat_hip.h.
 *
 * The missing step of the reference's feature clustering (motion_utils.py:57-116
 * similarity_mapping: SpectralClustering(affinity='precomputed') on a dense
 * N x N matrix): the leading eigenvectors of the normalised affinity of the
 * kNN graph that include/gs_feature_knn.h produces, without the matrix.
 *
 *   row_ptr [n + 1] int64, col [nnz] int32, val [nnz] float64: a symmetric
 *   graph in CSR form, columns ascending and unique within a row, every value
 *   finite and >= 0; self loops and empty rows allowed.  Symmetry is the
 *   caller's promise (it is not verified here).
 *
 * Definition:
 *
 *   d_i = sum_j val_ij                fp64, in CSR order
 *   g_i = 1 / sqrt(d_i) where d_i > 0, else 0
 *   S   = diag(g) A diag(g)           symmetric, spectrum in [-1, 1]
 *
 * Output for num_vectors = K:
 *
 *   eigenvalues [K] fp64   the K largest Ritz values theta of S, descending
 *                          (the normalised Laplacian's are 1 - theta)
 *   vectors     [n, K] fp64  orthonormal columns V
 *   embedding   [n, K] fp32  fl32(g_i V[i, j]); with row_normalize every
 *                          non-zero row is divided by its fp64 norm (the sum of
 *                          squares taken in column order) before the rounding;
 *                          +0 where g_i = 0
 *   residuals   [K] fp64   |S v_j - theta_j v_j|_2
 *   status      [4] int32  code, outer iterations run, columns (of the K) with
 *                          residual <= tol, the block width
 *
 * code 0: converged (every residual <= tol).  1: the iteration cap was
 * reached; the best Ritz pairs are returned.  2: a value or a degree is
 * negative or not finite, a column index is out of range, or row_ptr is not
 * a non-decreasing walk of [0, nnz]: every output is zero.  No output is ever
 * NaN.
 *
 * How.  Chebyshev-filtered subspace iteration on a block of
 * B = gs_spectral_block_width(n, K) columns.  One outer iteration: SVQB
 * orthonormalisation (Gram matrix from fixed slabs of rows, diagonal scaling,
 * Jacobi, X <- X D^-1/2 Q L^-1/2; a direction with L <= 2^-40 L_max is
 * replaced by a fresh counter-based column), run twice; W = S X, H = X^T W
 * (each pair taken once, from the upper triangle), Jacobi, theta descending
 * with ties by index, X <- X Q, W <- W Q, the residual norms; then, unless the
 * first K residuals are <= tol, the degree-m Chebyshev filter in Zhou and
 * Saad's scaled three-term form, damping [-1, theta_B] and scaled at theta_1,
 * one fused launch Y = a (S X) + b X + c Z per step.  Convergence is a flag on
 * the device that every later kernel of the call reads first: all launches of
 * the max_outer iterations are enqueued up front, nothing is read back and
 * the host never waits.
 *
 * Every sum is taken in an order that is a function of the sizes alone and
 * there are no float atomics: reruns are bit-identical.  The start block and
 * the replacement columns are
 *
 *   x(seed, e, i, j) = ((double)(mix(mix(seed + (e + 1) 0x9E3779B97F4A7C15)
 *                       ^ (i 128 + j)) >> 12) + 0.5) 2^-51 - 1     in (-1, 1)
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *           z *= 0x94D049BB133111EB; z ^= z >> 31          (64-bit, wrapping)
 *
 * with e = 0 for the start block and e = 1 + 2 t + p for a replacement in
 * pass p of outer iteration t.
 *
 * Limits: 1 <= K <= GS_SPECTRAL_MAX_K, K <= n <= GS_SPECTRAL_MAX_N,
 * 0 <= nnz < 2^31, 1 <= degree <= GS_SPECTRAL_MAX_DEGREE,
 * 1 <= max_outer <= GS_SPECTRAL_MAX_OUTER, tol > 0.
 *
 * The call is asynchronous on `stream` and returns 0 or an error code with
 * gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_SPECTRAL_H
#define GS_SPECTRAL_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_SPECTRAL_MAX_K 64
#define GS_SPECTRAL_MAX_N (1 << 26)
#define GS_SPECTRAL_MAX_DEGREE 64
#define GS_SPECTRAL_MAX_OUTER 1000
#define GS_SPECTRAL_GUARD 8     /* guard columns: B = min(n, 8 ceil((K + 8) / 8)) */
#define GS_SPECTRAL_MAX_B 72

typedef struct gs_spectral_args {
  int32_t n, num_vectors;
  int64_t nnz;
  int32_t degree, max_outer;
  int32_t row_normalize, _pad;
  uint64_t seed;
  double tol;
  const int64_t *row_ptr;  /* [n + 1] */
  const int32_t *col;      /* [nnz] */
  const double *val;       /* [nnz] */
  double *eigenvalues;     /* [K] */
  double *vectors;         /* [n, K] */
  float *embedding;        /* [n, K] */
  double *residuals;       /* [K] */
  int32_t *status;         /* [4] */
  void *workspace;         /* gs_spectral_workspace_bytes bytes, 16-byte aligned */
  uint64_t workspace_bytes;
} gs_spectral_args;

/* sizeof(gs_spectral_args) as the library was compiled (for binding mirrors). */
size_t gs_spectral_struct_bytes(void);

/* The block width: min(n, 8 ceil((K + 8) / 8)); 0 for sizes out of range. */
int32_t gs_spectral_block_width(int32_t n, int32_t K);

/* Workspace of one call (0 for sizes out of range). */
size_t gs_spectral_workspace_bytes(int32_t n, int64_t nnz, int32_t K);

/* The argument check gs_spectral_embedding runs first (host code, no device access). */
int gs_spectral_validate(const gs_spectral_args *args);

/* The host build of the small problems (csrc/gs_spectral_small.h), B <= GS_SPECTRAL_MAX_B.
 * svqb: from the Gram matrix G [B, B] the transform T [B, B] with (X T)^T (X T) = I, and
 * replaced [B] = 1 for a direction that was dropped (its column of T is zero).  ritz: from
 * H [B, B] (its upper triangle is read) theta [B] descending and Q [B, B], column j the j-th
 * Ritz vector.  Return 0 or an error code. */
int gs_spectral_svqb_host(int32_t B, const double *G, double *T, int32_t *replaced);
int gs_spectral_ritz_host(int32_t B, const double *H, double *theta, double *Q);

int gs_spectral_embedding(const gs_spectral_args *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_SPECTRAL_H */
