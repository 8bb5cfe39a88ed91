/* motion_init_host_sanitize.c -- stand-alone driver of the motion
 * initialisation's host validators
 * (dynamic3dgaussians_amd/csrc/gs_motion_init_host.cpp) for a CPU sanitizer
 * build (tests/test_motion_init.py compiles this file, gs_host.cpp and
 * gs_motion_init_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks; the validators must
 * accept / refuse each one with a message and touch nothing they were not
 * given.  The pointers name heap buffers, none of which a validator may
 * dereference.  Exit status 0 and "motion init host sanitize ok" on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_motion_init.h"
#include "host_sanitize.h"

int main(void) {
  const int64_t N = 301;
  const int D = 70, K = 7, T = 12;
  float *x = malloc((size_t)N * D * sizeof(float)), *centers = malloc((size_t)K * D * sizeof(float));
  float *tracks = malloc((size_t)N * T * 3 * sizeof(float)), *w = malloc((size_t)N * T * sizeof(float));
  float *out = malloc((size_t)N * K * sizeof(float) + (size_t)K * T * 6 * sizeof(float));
  int64_t *labels = malloc((size_t)(N + K + 1) * sizeof(int64_t)), *counts = malloc((size_t)K * sizeof(int64_t));
  uint8_t *bytes = malloc((size_t)N + (size_t)K * T);
  const size_t km_bytes = gs_kmeans_workspace_bytes(N, K, D), pr_bytes = gs_procrustes_workspace_bytes(K, T);
  void *ws = aligned_alloc(256, ((km_bytes > pr_bytes ? km_bytes : pr_bytes) + 255) / 256 * 256);
  if (!x || !centers || !tracks || !w || !out || !labels || !counts || !bytes || !ws) return 2;

  /* sizes */
  expect(km_bytes >= (size_t)K * D * sizeof(double) + (size_t)K * sizeof(int64_t), "k-means workspace holds a block");
  expect(gs_kmeans_workspace_bytes(0, K, D) > 0, "N = 0 still sums one block of zeros");
  expect(gs_kmeans_workspace_bytes(N, 65, D) == 0 && gs_kmeans_workspace_bytes(N, 0, D) == 0 &&
             gs_kmeans_workspace_bytes(N, K, 0) == 0 && gs_kmeans_workspace_bytes(-1, K, D) == 0,
         "k-means workspace outside the limits is 0");
  expect(gs_kmeans_workspace_bytes(1000000, 64, 447) <= (size_t)1100 * 64 * 447 * 8, "at most 1024 blocks");
  expect(pr_bytes >= (size_t)K * T * 19 * sizeof(double), "procrustes workspace holds the moments");
  expect(gs_procrustes_workspace_bytes(65, T) == 0 && gs_procrustes_workspace_bytes(K, 0) == 0,
         "procrustes workspace outside the limits is 0");
  expect(gs_kmeans_assign_struct_bytes() == sizeof(struct gs_kmeans_assign) &&
             gs_kmeans_update_struct_bytes() == sizeof(struct gs_kmeans_update) &&
             gs_coefs_from_centers_struct_bytes() == sizeof(struct gs_coefs_from_centers) &&
             gs_procrustes_struct_bytes() == sizeof(struct gs_procrustes), "struct sizes");

  /* assign */
  struct gs_kmeans_assign ga;
  memset(&ga, 0, sizeof(ga));
  ga.N = N; ga.D = D; ga.K = K; ga.x = x; ga.centers = centers; ga.labels = labels;
  struct gs_kmeans_assign a = ga;
  expect(gs_kmeans_assign_validate(&a) == 0, "assign");
  a.valid = bytes; a.prev_labels = labels; a.moved = counts;
  expect(gs_kmeans_assign_validate(&a) == 0, "assign with mask and moved");
  a = ga; a.K = 64; expect(gs_kmeans_assign_validate(&a) == 0, "K = 64");
  a = ga; a.N = 0; a.x = NULL; a.labels = NULL; expect(gs_kmeans_assign_validate(&a) == 0, "N = 0");
  expect(refused(gs_kmeans_assign_validate(NULL), "null argument"), "null block");
  a = ga; a.K = 65; expect(refused(gs_kmeans_assign_validate(&a), "K must be"), "K = 65");
  a = ga; a.K = 0;  expect(refused(gs_kmeans_assign_validate(&a), "K must be"), "K = 0");
  a = ga; a.D = 0;  expect(refused(gs_kmeans_assign_validate(&a), "D must be"), "D = 0");
  a = ga; a.N = -1; expect(refused(gs_kmeans_assign_validate(&a), "N must be"), "N < 0");
  a = ga; a.x = NULL;       expect(refused(gs_kmeans_assign_validate(&a), "x is required"), "null x");
  a = ga; a.centers = NULL; expect(refused(gs_kmeans_assign_validate(&a), "centers are required"), "null centers");
  a = ga; a.labels = NULL;  expect(refused(gs_kmeans_assign_validate(&a), "labels are required"), "null labels");
  a = ga; a.moved = counts; expect(refused(gs_kmeans_assign_validate(&a), "go together"), "moved without prev_labels");
  a = ga; a.x = (const float *)((const char *)x + 2);
  expect(refused(gs_kmeans_assign_validate(&a), "4-byte aligned"), "misaligned x");
  a = ga; a.labels = (int64_t *)((char *)labels + 4);
  expect(refused(gs_kmeans_assign_validate(&a), "8-byte aligned"), "misaligned labels");

  /* update */
  struct gs_kmeans_update gu;
  memset(&gu, 0, sizeof(gu));
  gu.N = N; gu.D = D; gu.K = K; gu.x = x; gu.labels = labels; gu.centers = centers; gu.counts = counts;
  gu.workspace = ws; gu.workspace_bytes = km_bytes;
  struct gs_kmeans_update u = gu;
  expect(gs_kmeans_update_validate(&u) == 0, "update");
  expect(refused(gs_kmeans_update_validate(NULL), "null argument"), "null block");
  u = gu; u.K = 65; expect(refused(gs_kmeans_update_validate(&u), "K must be"), "K = 65");
  u = gu; u.D = -3; expect(refused(gs_kmeans_update_validate(&u), "D must be"), "D < 0");
  u = gu; u.labels = NULL;  expect(refused(gs_kmeans_update_validate(&u), "x and labels"), "null labels");
  u = gu; u.centers = NULL; expect(refused(gs_kmeans_update_validate(&u), "centers are required"), "null centers");
  u = gu; u.counts = NULL;  expect(refused(gs_kmeans_update_validate(&u), "counts are required"), "null counts");
  u = gu; u.workspace = NULL; expect(refused(gs_kmeans_update_validate(&u), "workspace is required"), "null workspace");
  u = gu; u.workspace_bytes = km_bytes - 1; expect(refused(gs_kmeans_update_validate(&u), "needed"), "short workspace");
  u = gu; u.workspace = (char *)ws + 4; expect(refused(gs_kmeans_update_validate(&u), "16-byte"), "misaligned workspace");

  /* coefficients */
  struct gs_coefs_from_centers gc;
  memset(&gc, 0, sizeof(gc));
  gc.N = N; gc.K = K; gc.means = x; gc.centers = centers; gc.coefs = out;
  struct gs_coefs_from_centers c = gc;
  expect(gs_coefs_from_centers_validate(&c) == 0, "coefs");
  c = gc; c.N = 0; c.means = NULL; c.coefs = NULL; expect(gs_coefs_from_centers_validate(&c) == 0, "coefs N = 0");
  expect(refused(gs_coefs_from_centers_validate(NULL), "null argument"), "null block");
  c = gc; c.K = 0; expect(refused(gs_coefs_from_centers_validate(&c), "K must be"), "K = 0");
  c = gc; c.means = NULL;   expect(refused(gs_coefs_from_centers_validate(&c), "means and coefs"), "null means");
  c = gc; c.centers = NULL; expect(refused(gs_coefs_from_centers_validate(&c), "centers are required"), "null centers");

  /* procrustes */
  struct gs_procrustes gp;
  memset(&gp, 0, sizeof(gp));
  gp.N = N; gp.T = T; gp.K = K; gp.cano_t = 5; gp.rot_dim = 6; gp.min_weight_sum = 1.2; gp.tracks = tracks;
  gp.order = labels; gp.offsets = labels + N; gp.rots = out; gp.transls = out; gp.err_after = out; gp.err_before = out;
  gp.skipped = bytes; gp.workspace = ws; gp.workspace_bytes = pr_bytes;
  struct gs_procrustes p = gp;
  expect(gs_procrustes_validate(&p) == 0, "procrustes");
  p.weights = w; p.confidences = w; p.rot_dim = 4; p.cano_t = T - 1;
  expect(gs_procrustes_validate(&p) == 0, "procrustes with weights, quaternions, the last frame");
  p = gp; p.N = 0; p.tracks = NULL; p.order = NULL; expect(gs_procrustes_validate(&p) == 0, "procrustes N = 0");
  p = gp; p.T = 1; p.cano_t = 0; expect(gs_procrustes_validate(&p) == 0, "T = 1");
  expect(refused(gs_procrustes_validate(NULL), "null argument"), "null block");
  p = gp; p.K = 65;      expect(refused(gs_procrustes_validate(&p), "K must be"), "K = 65");
  p = gp; p.T = 0;       expect(refused(gs_procrustes_validate(&p), "T must be"), "T = 0");
  p = gp; p.cano_t = T;  expect(refused(gs_procrustes_validate(&p), "outside"), "cano_t = T");
  p = gp; p.cano_t = -1; expect(refused(gs_procrustes_validate(&p), "outside"), "cano_t < 0");
  p = gp; p.rot_dim = 9; expect(refused(gs_procrustes_validate(&p), "rot_dim"), "rot_dim = 9");
  p = gp; p.min_weight_sum = (double)NAN; expect(refused(gs_procrustes_validate(&p), "NaN"), "NaN threshold");
  p = gp; p.tracks = NULL;  expect(refused(gs_procrustes_validate(&p), "tracks and order"), "null tracks");
  p = gp; p.offsets = NULL; expect(refused(gs_procrustes_validate(&p), "offsets are required"), "null offsets");
  p = gp; p.rots = NULL;    expect(refused(gs_procrustes_validate(&p), "rots and transls"), "null rots");
  p = gp; p.skipped = NULL; expect(refused(gs_procrustes_validate(&p), "skipped are required"), "null skipped");
  p = gp; p.workspace = NULL; expect(refused(gs_procrustes_validate(&p), "workspace is required"), "null workspace");
  p = gp; p.order = (const int64_t *)((const char *)labels + 4);
  expect(refused(gs_procrustes_validate(&p), "8-byte aligned"), "misaligned order");

  free(x); free(centers); free(tracks); free(w); free(out); free(labels); free(counts); free(bytes); free(ws);
  if (failures) return 1;
  printf("motion init host sanitize ok\n");
  return 0;
}
