/* feature_pca_host_sanitize.c -- stand-alone driver of the feature PCA's host
 * code (dynamic3dgaussians_amd/csrc/gs_feature_pca_host.cpp) for a CPU
 * sanitizer build (tests/test_feature_pca.py compiles this file, gs_host.cpp
 * and gs_feature_pca_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks of all six passes
 * through the validator, which must accept / refuse each one with a message
 * and dereference none of the pointers, and runs the host build of the Jacobi
 * eigensolver (csrc/gs_sym_eig.h) on a few fixed matrices.  Exit status 0 and
 * "feature pca host sanitize ok" on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_feature_pca.h"
#include "host_sanitize.h"

static int fp_refused(const gs_feature_pca *a, int pass, const char *needle) {
  return refused(gs_feature_pca_validate(a, pass), needle);
}

/* A = V diag(lam) V^T reproduced to `tol`, V orthonormal rows, lam descending, signs by the rule */
static int eig_ok(int C, const double *A, double tol) {
  double *lam = malloc(sizeof(double) * C), *vec = malloc(sizeof(double) * C * C);
  int32_t sweeps = -1;
  int64_t rot = -1;
  int ok = lam && vec && gs_feature_pca_eig_host(C, A, lam, vec, &sweeps, &rot) == 0;
  ok = ok && sweeps >= 0 && sweeps <= GS_FPCA_MAX_SWEEPS && rot >= 0 && rot < (int64_t)(sweeps + 1) * C * C;
  for (int i = 0; ok && i < C; ++i) {
    if (i && lam[i] > lam[i - 1]) ok = 0;
    double big = 0.0;
    int arg = 0;
    for (int c = 0; c < C; ++c)
      if (fabs(vec[i * C + c]) > big) { big = fabs(vec[i * C + c]); arg = c; }
    if (!(vec[i * C + arg] > 0.0)) ok = 0;
    for (int j = 0; j < C; ++j) {
      double dot = 0.0, rec = 0.0;
      for (int c = 0; c < C; ++c) {
        dot += vec[i * C + c] * vec[j * C + c];
        rec += lam[c] * vec[c * C + i] * vec[c * C + j];
      }
      if (fabs(dot - (i == j ? 1.0 : 0.0)) > tol || fabs(rec - A[i * C + j]) > tol) ok = 0;
    }
  }
  free(lam); free(vec);
  return ok;
}

int main(void) {
  const int B = 3, C = 32, H = 72, W = 128, k = 3;
  expect(gs_feature_pca_struct_bytes() == sizeof(gs_feature_pca), "struct size");
  expect(gs_feature_pca_max_sweeps() == GS_FPCA_MAX_SWEEPS, "sweep cap");
  expect(gs_feature_pca_n_acc(B, H, W) == GS_FPCA_CHUNK && gs_feature_pca_n_acc(1, 5, 9) == 128 &&
             gs_feature_pca_n_acc(1, 12, 31) == 384 && gs_feature_pca_n_acc(0, H, W) == 0, "n_acc");
  const size_t chunks = (size_t)(H * W + GS_FPCA_CHUNK - 1) / GS_FPCA_CHUNK, slabs = chunks * B, e = C * C + C + 1;
  const size_t ws_up = gs_feature_pca_workspace_bytes(B, C, H, W, 0, GS_FPCA_PASS_UPDATE);
  expect(ws_up >= slabs * e * 4 + e * 8 + slabs * (C + 1) * 8 + (C + 1) * 8 && ws_up < slabs * e * 4 + 2 * e * 8 + slabs * (C + 1) * 16,
         "update: the slabs, one group of them, and the shift pass's pair");
  expect(gs_feature_pca_workspace_bytes(1, 64, 1, 1, 3, GS_FPCA_PASS_FIT) == 0, "fit in LDS up to 64");
  expect(gs_feature_pca_workspace_bytes(1, 65, 1, 1, 3, GS_FPCA_PASS_FIT) == 2 * 66 * 67 * 8, "fit: A and V of the even order, an odd leading dimension");
  const size_t ws_pr = gs_feature_pca_workspace_bytes(B, C, H, W, k, GS_FPCA_PASS_PROJECT);
  expect(ws_pr == (size_t)B * 36 * k * 2 * 4, "project: the blocks' minima and maxima");
  expect(gs_feature_pca_workspace_bytes(B, 129, H, W, k, 0) == 0 && gs_feature_pca_workspace_bytes(B, C, 0, W, k, 0) == 0 &&
             gs_feature_pca_workspace_bytes(B, C, H, W, 9, GS_FPCA_PASS_PROJECT) == 0 &&
             gs_feature_pca_workspace_bytes(B, C, H, W, k, 6) == 0, "workspace of a size out of range or an unknown pass is 0");

  const size_t ws_bytes = (ws_up + 255) / 256 * 256;
  void *ws = aligned_alloc(256, ws_bytes);
  double *d = malloc(64);
  float *f = malloc(64);
  unsigned char *m = malloc(64);
  if (!ws || !d || !f || !m) return 2;

  gs_feature_pca good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.C = C; good.H = H; good.W = W; good.k = k; good.sample_stride = 1; good.ddof = 1;
  good.x = f; good.mask = m + 1; good.shift = f; good.state = d; good.mean = d; good.cov = d; good.evals = d; good.evecs = d;
  good.components = d; good.components_f32 = f; good.mean_f32 = f; good.status = (int32_t *)f; good.proj_components = f;
  good.proj_mean = f; good.t = f; good.tmin = f; good.tmax = f; good.sub = f; good.u = f; good.lo = d; good.hi = d;
  good.out = m + 1; good.out_uint8 = 1;
  good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  for (int pass = 0; pass < 6; ++pass) expect(gs_feature_pca_validate(&good, pass) == 0, "full block");
  gs_feature_pca bare = good;
  bare.mask = NULL; bare.mask_per_image = 1;
  for (int pass = 0; pass < 6; ++pass) expect(gs_feature_pca_validate(&bare, pass) == 0, "no mask");
  gs_feature_pca corner = good;
  corner.B = 1; corner.C = 1; corner.H = 1; corner.W = 1; corner.k = 1;
  for (int pass = 0; pass < 5; ++pass) expect(gs_feature_pca_validate(&corner, pass) == 0, "all ones");
  corner = good; corner.C = 128; corner.k = 8; corner.B = 1; corner.H = 12; corner.W = 31;
  corner.workspace_bytes = (uint64_t)1 << 30; /* a size only: the validator reads no workspace */
  expect(gs_feature_pca_validate(&corner, GS_FPCA_PASS_UPDATE) == 0 && gs_feature_pca_validate(&corner, GS_FPCA_PASS_FIT) == 0 &&
             gs_feature_pca_validate(&corner, GS_FPCA_PASS_PROJECT) == 0, "128 channels, 8 components");
  gs_feature_pca cov = good;
  cov.B = 0; cov.H = 0; cov.W = 0; cov.workspace = NULL; cov.workspace_bytes = 0;
  expect(gs_feature_pca_validate(&cov, GS_FPCA_PASS_COVARIANCE) == 0 && gs_feature_pca_validate(&cov, GS_FPCA_PASS_FIT) == 0,
         "covariance and fit take no image sizes and, in LDS, no workspace");

  /* invalid blocks, one fault each */
  gs_feature_pca bad;
  expect(fp_refused(NULL, 0, "null argument block"), "null block");
  expect(fp_refused(&good, 6, "unknown pass"), "pass 6");
  expect(fp_refused(&good, -1, "unknown pass"), "pass -1");
  bad = good; bad.C = 0; expect(fp_refused(&bad, 0, "C must be in"), "C = 0");
  bad = good; bad.C = 129; expect(fp_refused(&bad, 0, "_torch"), "C = 129 names the twins");
  bad = good; bad.C = 129; expect(fp_refused(&bad, 2, "C must be in"), "C = 129 in fit");
  bad = good; bad.B = 0; expect(fp_refused(&bad, 0, "B must be in"), "B = 0");
  bad = good; bad.B = 65536; expect(fp_refused(&bad, 3, "B must be in"), "B past the grid");
  bad = good; bad.H = 0; expect(fp_refused(&bad, 0, "H, W must be >= 1"), "H = 0");
  bad = good; bad.W = -5; expect(fp_refused(&bad, 5, "H, W must be >= 1"), "W < 0");
  bad = good; bad.H = 65536; bad.W = 32768; expect(fp_refused(&bad, 0, "H * W"), "H * W = 2^31");
  bad = good; bad.B = 65535; bad.H = 32768; bad.W = 32768; expect(fp_refused(&bad, 0, "per call"), "too many slabs for one call");
  bad = good; bad.k = 0; expect(fp_refused(&bad, 2, "k must be in"), "k = 0");
  bad = good; bad.k = 9; expect(fp_refused(&bad, 3, "k must be in"), "k = 9");
  bad = good; bad.C = 2; expect(fp_refused(&bad, 2, "k must be in"), "k > C");
  bad = good; bad.k = 2; expect(fp_refused(&bad, 5, "colour needs k = 3"), "colour with k = 2");
  bad = good; bad.sample_stride = 0; expect(fp_refused(&bad, 0, "sample_stride"), "stride 0");
  bad = good; bad.ddof = -1; expect(fp_refused(&bad, 1, "ddof"), "ddof < 0");
  bad = good; bad.x = NULL; expect(fp_refused(&bad, 0, "x is required"), "null x");
  bad = good; bad.x = NULL; expect(fp_refused(&bad, 3, "x is required"), "null x");
  bad = good; bad.shift = NULL; expect(fp_refused(&bad, 0, "shift is required"), "null shift");
  bad = good; bad.state = NULL; expect(fp_refused(&bad, 0, "state is required"), "null state");
  bad = good; bad.state = NULL; expect(fp_refused(&bad, 1, "state is required"), "null state");
  bad = good; bad.state = NULL; expect(fp_refused(&bad, 2, "state is required"), "null state");
  bad = good; bad.cov = NULL; expect(fp_refused(&bad, 1, "cov is required"), "null cov");
  bad = good; bad.mean = NULL; expect(fp_refused(&bad, 1, "mean is required"), "null mean");
  bad = good; bad.mean_f32 = NULL; expect(fp_refused(&bad, 2, "mean_f32"), "null mean_f32");
  bad = good; bad.evecs = NULL; expect(fp_refused(&bad, 2, "evecs"), "null evecs");
  bad = good; bad.components_f32 = NULL; expect(fp_refused(&bad, 2, "components_f32"), "null components_f32");
  bad = good; bad.status = NULL; expect(fp_refused(&bad, 2, "status is required"), "null status");
  bad = good; bad.proj_mean = NULL; expect(fp_refused(&bad, 3, "proj_mean"), "null proj_mean");
  bad = good; bad.t = NULL; expect(fp_refused(&bad, 3, "t is required"), "null t");
  bad = good; bad.tmax = NULL; expect(fp_refused(&bad, 3, "tmin and tmax"), "null tmax");
  bad = good; bad.sub = NULL; expect(fp_refused(&bad, 4, "sub is required"), "null sub");
  bad = good; bad.u = NULL; expect(fp_refused(&bad, 4, "u is required"), "null u");
  bad = good; bad.lo = NULL; expect(fp_refused(&bad, 5, "lo and hi"), "null lo");
  bad = good; bad.out = NULL; expect(fp_refused(&bad, 5, "out is required"), "null out");
  bad = good; bad.out_uint8 = 0; expect(fp_refused(&bad, 5, "4-byte aligned"), "misaligned float out");
  bad = good; bad.x = (const float *)((const char *)f + 1); expect(fp_refused(&bad, 0, "4-byte aligned"), "misaligned x");
  bad = good; bad.state = (double *)((char *)d + 4); expect(fp_refused(&bad, 0, "8-byte aligned"), "misaligned state");
  bad = good; bad.workspace = NULL; expect(fp_refused(&bad, 0, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_up - 1; expect(fp_refused(&bad, 0, "needed"), "short workspace");
  bad = good; bad.C = 128; bad.workspace_bytes = 2 * 128 * 129 * 8 - 1; expect(fp_refused(&bad, 2, "needed"), "fit above the LDS order");
  bad = good; bad.workspace = (char *)ws + 4; expect(fp_refused(&bad, 3, "16-byte aligned"), "misaligned workspace");

  /* the host build of the eigensolver */
  {
    const double one[1] = {3.5};
    const double two[4] = {2.0, 1.0, 1.0, 2.0};                          /* 3, 1 */
    const double rep[9] = {2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 5.0}; /* diagonal, repeated */
    const double thr[9] = {4.0, -2.0, 0.5, -2.0, 1.0, 3.0, 0.5, 3.0, -6.0};
    expect(eig_ok(1, one, 1e-15), "order 1");
    expect(eig_ok(2, two, 1e-14), "order 2");
    expect(eig_ok(3, rep, 1e-14), "diagonal with a repeated eigenvalue");
    expect(eig_ok(3, thr, 1e-13), "order 3 (odd: padded)");
    for (int n = 31; n <= 33; ++n) {
      double *a = malloc(sizeof(double) * n * n);
      if (!a) return 2;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) a[i * n + j] = a[j * n + i] = sin(1.0 + 3.0 * i + 7.0 * j + (double)i * j) + (i == j ? n : 0);
      expect(eig_ok(n, a, 1e-11), "orders 31, 32, 33");
      free(a);
    }
    double nan3[9] = {1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 3.0}, lam3[3] = {9.0, 9.0, 9.0}, vec3[9];
    nan3[1] = nan3[3] = NAN;
    for (int i = 0; i < 9; ++i) vec3[i] = 9.0;
    int zeros = gs_feature_pca_eig_host(3, nan3, lam3, vec3, NULL, NULL) == 3;
    for (int i = 0; i < 9; ++i) zeros = zeros && vec3[i] == 0.0 && lam3[i % 3] == 0.0;
    expect(zeros, "a NaN entry: status 3 and zeros");
    double lam[1], vec[1];
    expect(refused(gs_feature_pca_eig_host(0, one, lam, vec, NULL, NULL), "C must be in"), "eig: order 0");
    expect(refused(gs_feature_pca_eig_host(129, one, lam, vec, NULL, NULL), "C must be in"), "eig: order 129");
    expect(refused(gs_feature_pca_eig_host(1, NULL, lam, vec, NULL, NULL), "are required"), "eig: null A");
  }

  free(ws); free(d); free(f); free(m);
  if (failures) return 1;
  printf("feature pca host sanitize ok\n");
  return 0;
}
