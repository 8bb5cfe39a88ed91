/* spectral_host_sanitize.c -- stand-alone driver of the spectral embedding's
 * host code (dynamic3dgaussians_amd/csrc/gs_spectral_host.cpp) for a CPU
 * sanitizer build (tests/test_spectral.py compiles this file, gs_host.cpp and
 * gs_spectral_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks -- the validator must
 * accept / refuse each one with a message and dereference none of the
 * pointers, which name heap buffers -- and runs the host build of the small
 * problems (gs_spectral_small.h on gs_sym_eig.h) on a 24 x 24 case, checked
 * against plain triple-loop products.  Exit status 0 and "spectral host
 * sanitize ok" on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_spectral.h"
#include "host_sanitize.h"

static int sp_refused(const gs_spectral_args *a, const char *needle) {
  return refused(gs_spectral_validate(a), needle);
}

/* a fixed pseudo-random sequence in (-1, 1) */
static double next(unsigned long long *s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((*s >> 11) & 0xfffffffffffffull) / 4503599627370496.0 * 2.0 - 1.0;
}

enum { NB = 24, NR = 40 };

static void small_problems(void) {
  static double X[NR][NB], G[NB][NB], T[NB][NB], Y[NR][NB], H[NB][NB], Q[NB][NB], theta[NB];
  int32_t replaced[NB];
  unsigned long long s = 7;
  for (int r = 0; r < NR; ++r)
    for (int j = 0; j < NB; ++j) X[r][j] = next(&s) * (j == 3 ? 1e-3 : 1.0); /* one badly scaled column */
  for (int r = 0; r < NR; ++r) X[r][5] = 0.0;                                  /* a zero column */
  for (int r = 0; r < NR; ++r) X[r][9] = X[r][8];                              /* a repeated column */
  for (int i = 0; i < NB; ++i)
    for (int j = 0; j < NB; ++j) {
      double a = 0.0;
      for (int r = 0; r < NR; ++r) a += X[r][i] * X[r][j];
      G[i][j] = a;
    }
  expect(gs_spectral_svqb_host(NB, &G[0][0], &T[0][0], replaced) == 0, "svqb runs");
  int gone = 0;
  for (int k = 0; k < NB; ++k) gone += replaced[k];
  expect(gone == 2, "the zero column and the repeated one are dropped, nothing else");
  for (int r = 0; r < NR; ++r)
    for (int k = 0; k < NB; ++k) {
      double a = 0.0;
      for (int i = 0; i < NB; ++i) a += X[r][i] * T[i][k];
      Y[r][k] = a;
    }
  double worst = 0.0;
  for (int i = 0; i < NB; ++i)
    for (int j = 0; j < NB; ++j) {
      double a = 0.0;
      for (int r = 0; r < NR; ++r) a += Y[r][i] * Y[r][j];
      const double want = i == j && !replaced[i] ? 1.0 : 0.0;
      if (fabs(a - want) > worst) worst = fabs(a - want);
    }
  /* one SVQB pass: the departure from I is the Gram matrix's rounding, amplified by the
   * scaled condition number, which the 2^-40 rank threshold caps */
  expect(worst < 1e-9, "(X T)^T (X T) = I on the kept directions, 0 on the dropped ones");

  /* Ritz: a symmetric H with a repeated eigenvalue */
  for (int i = 0; i < NB; ++i)
    for (int j = i; j < NB; ++j) H[i][j] = i < 2 ? (i == j ? 0.75 : 0.0) : 0.3 * next(&s); /* 0.75 twice, then a random block */
  for (int i = 1; i < NB; ++i)
    for (int j = 0; j < i; ++j) H[i][j] = 1e300; /* the lower triangle is never read */
  expect(gs_spectral_ritz_host(NB, &H[0][0], theta, &Q[0][0]) == 0, "ritz runs");
  for (int j = 1; j < NB; ++j) expect(theta[j - 1] >= theta[j], "theta descends");
  worst = 0.0;
  double ortho = 0.0;
  for (int j = 0; j < NB; ++j)
    for (int i = 0; i < NB; ++i) {
      double a = 0.0, o = 0.0;
      for (int k = 0; k < NB; ++k) {
        a += (i <= k ? H[i][k] : H[k][i]) * Q[k][j];
        o += Q[k][i] * Q[k][j];
      }
      if (fabs(a - theta[j] * Q[i][j]) > worst) worst = fabs(a - theta[j] * Q[i][j]);
      if (fabs(o - (i == j ? 1.0 : 0.0)) > ortho) ortho = fabs(o - (i == j ? 1.0 : 0.0));
    }
  expect(worst < 1e-13, "H Q = Q diag(theta)");
  expect(ortho < 1e-13, "Q^T Q = I");
  expect(gs_spectral_svqb_host(0, &G[0][0], &T[0][0], replaced) < 0 && gs_spectral_svqb_host(73, &G[0][0], &T[0][0], replaced) < 0,
         "svqb_host refuses an order out of range");
  expect(gs_spectral_ritz_host(NB, NULL, theta, &Q[0][0]) < 0, "ritz_host refuses a null matrix");
  /* order 1 and an odd order: the padding of the Jacobi */
  double g1 = 4.0, t1 = 0.0;
  expect(gs_spectral_svqb_host(1, &g1, &t1, replaced) == 0 && replaced[0] == 0 && fabs(t1 - 0.5) < 1e-15, "order 1");
  double h3[9] = {2, 1, 0, 1, 2, 0, 0, 0, -1}, th3[3], q3[9];
  expect(gs_spectral_ritz_host(3, h3, th3, q3) == 0 && fabs(th3[0] - 3) < 1e-14 && fabs(th3[1] - 1) < 1e-14 &&
             fabs(th3[2] + 1) < 1e-14,
         "order 3");
}

int main(void) {
  const int n = 1500, K = 9;
  const int64_t nnz = 27000;
  expect(gs_spectral_struct_bytes() == sizeof(gs_spectral_args), "struct size");
  expect(gs_spectral_block_width(n, 1) == 16 && gs_spectral_block_width(n, 8) == 16 && gs_spectral_block_width(n, 9) == 24 &&
             gs_spectral_block_width(n, 56) == 64 && gs_spectral_block_width(n, 64) == 72,
         "block width tiers");
  expect(gs_spectral_block_width(10, 3) == 10 && gs_spectral_block_width(1, 1) == 1, "the block is never wider than the space");
  expect(gs_spectral_block_width(n, 0) == 0 && gs_spectral_block_width(n, 65) == 0 && gs_spectral_block_width(3, 4) == 0 &&
             gs_spectral_block_width(GS_SPECTRAL_MAX_N + 1, 4) == 0,
         "block width of a size out of range is 0");
  const size_t ws_bytes = gs_spectral_workspace_bytes(n, nnz, K);
  expect(ws_bytes > (size_t)4 * n * 24 * 8, "covers the four blocks");
  expect(gs_spectral_workspace_bytes(n, nnz, 64) > ws_bytes, "a wider block needs more");
  expect(gs_spectral_workspace_bytes(n, (int64_t)1 << 31, K) == 0 && gs_spectral_workspace_bytes(n, -1, K) == 0 &&
             gs_spectral_workspace_bytes(n, nnz, 65) == 0 && gs_spectral_workspace_bytes(8, nnz, K) == 0,
         "workspace of a size out of range is 0");
  expect(gs_spectral_workspace_bytes(GS_SPECTRAL_MAX_N, 0, 64) > ((size_t)1 << 32), "sizes past 32 bits");

  int64_t *row_ptr = malloc(64);
  int32_t *col = malloc(64), *status = malloc(64);
  double *val = malloc(64), *ev = malloc(64), *vec = malloc(64), *res = malloc(64);
  float *emb = malloc(64);
  void *ws = aligned_alloc(256, 4096);
  if (!row_ptr || !col || !status || !val || !ev || !vec || !res || !emb || !ws) return 2;

  gs_spectral_args good;
  memset(&good, 0, sizeof(good));
  good.n = n; good.num_vectors = K; good.nnz = nnz; good.degree = 8; good.max_outer = 30; good.tol = 1e-8;
  good.row_ptr = row_ptr; good.col = col; good.val = val; good.eigenvalues = ev; good.vectors = vec;
  good.embedding = emb; good.residuals = res; good.status = status;
  good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  expect(gs_spectral_validate(&good) == 0, "plain block");
  gs_spectral_args ok = good;
  ok.row_normalize = 1; ok.seed = ~0ull; expect(gs_spectral_validate(&ok) == 0, "row_normalize, the largest seed");
  ok = good; ok.nnz = 0; ok.col = NULL; ok.val = NULL; expect(gs_spectral_validate(&ok) == 0, "an empty graph needs no col and val");
  ok = good; ok.n = 1; ok.num_vectors = 1; expect(gs_spectral_validate(&ok) == 0, "one node");
  ok = good; ok.num_vectors = 64; ok.degree = 64; ok.max_outer = 1000; ok.workspace_bytes = gs_spectral_workspace_bytes(n, nnz, 64);
  expect(gs_spectral_validate(&ok) == 0, "the limits themselves");

  /* invalid blocks, one fault each */
  gs_spectral_args bad;
  expect(sp_refused(NULL, "null argument block"), "null block");
  bad = good; bad.num_vectors = 0; expect(sp_refused(&bad, "num_vectors must be in"), "K = 0");
  bad = good; bad.num_vectors = 65; expect(sp_refused(&bad, "spectral_embedding_torch"), "K = 65 names the twin");
  bad = good; bad.n = 8; expect(sp_refused(&bad, "n must be in"), "n < K");
  bad = good; bad.n = GS_SPECTRAL_MAX_N + 1; expect(sp_refused(&bad, "n must be in"), "n past the limit");
  bad = good; bad.nnz = -1; expect(sp_refused(&bad, "nnz must be in"), "nnz < 0");
  bad = good; bad.nnz = (int64_t)1 << 31; expect(sp_refused(&bad, "nnz must be in"), "nnz = 2^31");
  bad = good; bad.degree = 0; expect(sp_refused(&bad, "degree must be in"), "degree = 0");
  bad = good; bad.degree = 65; expect(sp_refused(&bad, "degree must be in"), "degree = 65");
  bad = good; bad.max_outer = 0; expect(sp_refused(&bad, "max_outer must be in"), "max_outer = 0");
  bad = good; bad.max_outer = 1001; expect(sp_refused(&bad, "max_outer must be in"), "max_outer = 1001");
  bad = good; bad.tol = 0.0; expect(sp_refused(&bad, "tol must be positive"), "tol = 0");
  bad = good; bad.tol = -1e-8; expect(sp_refused(&bad, "tol must be positive"), "tol < 0");
  bad = good; bad.tol = NAN; expect(sp_refused(&bad, "tol must be positive"), "tol NaN");
  bad = good; bad.row_normalize = 2; expect(sp_refused(&bad, "row_normalize must be"), "row_normalize = 2");
  bad = good; bad.row_ptr = NULL; expect(sp_refused(&bad, "row_ptr is required"), "null row_ptr");
  bad = good; bad.col = NULL; expect(sp_refused(&bad, "col and val are required"), "null col");
  bad = good; bad.val = NULL; expect(sp_refused(&bad, "col and val are required"), "null val");
  bad = good; bad.vectors = NULL; expect(sp_refused(&bad, "are required"), "null vectors");
  bad = good; bad.status = NULL; expect(sp_refused(&bad, "are required"), "null status");
  bad = good; bad.col = (const int32_t *)((const char *)col + 2); expect(sp_refused(&bad, "4-byte aligned"), "misaligned col");
  bad = good; bad.val = (const double *)((const char *)val + 4); expect(sp_refused(&bad, "8-byte aligned"), "misaligned val");
  bad = good; bad.workspace = NULL; expect(sp_refused(&bad, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1; expect(sp_refused(&bad, "needed"), "short workspace");
  bad = good; bad.num_vectors = 64; expect(sp_refused(&bad, "needed"), "a wider block than the workspace was sized for");
  bad = good; bad.workspace = (char *)ws + 8; expect(sp_refused(&bad, "16-byte aligned"), "misaligned workspace");

  small_problems();

  free(row_ptr); free(col); free(status); free(val); free(ev); free(vec); free(res); free(emb); free(ws);
  if (failures) return 1;
  printf("spectral host sanitize ok\n");
  return 0;
}
