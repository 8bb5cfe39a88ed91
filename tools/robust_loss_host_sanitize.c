/* robust_loss_host_sanitize.c -- stand-alone driver of the quantile-trimmed
 * losses' host validator (dynamic3dgaussians_amd/csrc/gs_robust_loss_host.cpp)
 * for a CPU sanitizer build (tests/test_robust_loss.py compiles this file,
 * gs_host.cpp and gs_robust_loss_host.cpp with -fsanitize=address,undefined
 * and runs the program).  It walks valid and invalid argument blocks; the
 * validator must accept / refuse each one with a message and touch nothing it
 * was not given.  The pointers name heap buffers of the right size, none of
 * which the validator may dereference.  Exit status 0 and "robust loss host
 * sanitize ok" on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_robust_loss.h"
#include "host_sanitize.h"

static int rl_refused(const gs_robust_loss *a, int backward, const float *up, const float *dp, const char *needle) {
  return refused(gs_robust_loss_validate(a, backward, up, dp), needle);
}

int main(void) {
  const int B = 3, R = 3, N = 37 * 53;
  const size_t n = (size_t)B * R * N;
  const size_t ws_bytes = gs_robust_loss_workspace_bytes(B, N, GS_ROBUST_CHANNELS);
  const size_t ws_values = gs_robust_loss_workspace_bytes(B, N, GS_ROBUST_VALUES);
  /* per plane: 16 state words, 2048 + 2 * 1024 + 2 * 1024 counts, two records of four doubles */
  const size_t head = (size_t)B * (16 + 2048 + 4096) * 4 + (size_t)B * 2 * 4 * 8;
  expect(ws_values == head, "state, histograms and records");
  expect(ws_bytes == (head + (size_t)B * N * 4 + 15) / 16 * 16, "and the residual plane");
  expect(gs_robust_loss_workspace_bytes(B, N, GS_ROBUST_ROWS) == ws_bytes, "rows as channels");
  expect(gs_robust_loss_workspace_bytes(0, N, 0) == 0 && gs_robust_loss_workspace_bytes(B, -4, 0) == 0 &&
             gs_robust_loss_workspace_bytes(B, N, 3) == 0 && gs_robust_loss_workspace_bytes(B, N, -1) == 0,
         "workspace of an empty shape or an unknown layout is 0");
  expect(gs_robust_loss_workspace_bytes(1, 1 << 30, GS_ROBUST_VALUES) == (16 + 2048 + 4096) * 4 + 128 * 4 * 8,
         "capped workgroup count");
  expect(gs_robust_loss_struct_bytes() == sizeof(gs_robust_loss), "struct size");

  float *pred = malloc(n * sizeof(float)), *gt = malloc(n * sizeof(float)), *d_pred = malloc(n * sizeof(float));
  uint8_t *mask = malloc((size_t)B * N + 1);
  float *losses = malloc(B * sizeof(float)), *up = malloc(B * sizeof(float));
  double *stats = malloc((size_t)B * 4 * sizeof(double));
  void *ws = aligned_alloc(256, (ws_bytes + 255) / 256 * 256);
  if (!pred || !gt || !d_pred || !mask || !losses || !up || !stats || !ws) return 2;

  gs_robust_loss good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.R = R; good.N = N; good.layout = GS_ROBUST_CHANNELS;
  good.pred = pred; good.gt = gt;
  good.quantile = 0.9; good.select = 1;
  good.losses = losses; good.stats = stats; good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  expect(gs_robust_loss_validate(&good, 0, NULL, NULL) == 0, "bare forward block");
  expect(gs_robust_loss_validate(&good, 1, up, d_pred) == 0, "bare backward block");
  gs_robust_loss full = good;
  full.mask = mask + 1; /* a byte mask needs no alignment */
  full.mask_batch_stride = 0; full.over_masked = 1; full.normalize = 1; full.norm_width = 53; full.skip_degenerate = 1;
  expect(gs_robust_loss_validate(&full, 0, NULL, NULL) == 0, "shared [N] mask");
  full.mask = mask; full.mask_batch_stride = N;
  expect(gs_robust_loss_validate(&full, 0, NULL, NULL) == 0, "[B, N] mask");
  expect(gs_robust_loss_validate(&full, 1, up, d_pred) == 0, "full backward block");
  gs_robust_loss bw = full; /* the backward needs neither losses nor the workspace */
  bw.losses = NULL; bw.workspace = NULL; bw.workspace_bytes = 0;
  expect(gs_robust_loss_validate(&bw, 1, up, d_pred) == 0, "backward without workspace");
  gs_robust_loss rows = good;
  rows.layout = GS_ROBUST_ROWS; rows.quantile = 1.0;
  expect(gs_robust_loss_validate(&rows, 0, NULL, NULL) == 0, "row layout, q = 1");
  rows.quantile = 0.0; rows.select = 0;
  expect(gs_robust_loss_validate(&rows, 0, NULL, NULL) == 0, "q = 0, no selection");
  gs_robust_loss vals = good;
  vals.layout = GS_ROBUST_VALUES; vals.R = 1; vals.gt = NULL; vals.losses = NULL; vals.workspace_bytes = ws_values;
  expect(gs_robust_loss_validate(&vals, 0, NULL, NULL) == 0, "values: no gt, no losses, the smaller workspace");

  /* invalid blocks, one fault each */
  gs_robust_loss bad;
  expect(rl_refused(NULL, 0, NULL, NULL, "null argument block"), "null block");
  bad = good; bad.layout = 3; expect(rl_refused(&bad, 0, NULL, NULL, "unknown layout"), "layout 3");
  bad = good; bad.B = 0;  expect(rl_refused(&bad, 0, NULL, NULL, "B, R, N must be > 0"), "B = 0");
  bad = good; bad.R = -3; expect(rl_refused(&bad, 0, NULL, NULL, "B, R, N must be > 0"), "R < 0");
  bad = good; bad.N = 0;  expect(rl_refused(&bad, 0, NULL, NULL, "B, R, N must be > 0"), "N = 0");
  bad = good; bad.B = 2; bad.N = 1 << 30; expect(rl_refused(&bad, 0, NULL, NULL, "does not fit int32"), "B * N = 2^31");
  bad = good; bad.B = 70000; bad.N = 4; expect(rl_refused(&bad, 0, NULL, NULL, "too large"), "B past the grid");
  bad = vals; bad.R = 2; expect(rl_refused(&bad, 0, NULL, NULL, "R must be 1"), "values with R = 2");
  bad = vals; bad.select = 0; expect(rl_refused(&bad, 0, NULL, NULL, "needs select"), "values without selection");
  expect(rl_refused(&vals, 1, up, d_pred, "no backward"), "values backward");
  bad = good; bad.pred = NULL; expect(rl_refused(&bad, 0, NULL, NULL, "pred is required"), "null pred");
  bad = good; bad.gt = NULL; expect(rl_refused(&bad, 0, NULL, NULL, "gt is required"), "null gt");
  bad = good; bad.losses = NULL; expect(rl_refused(&bad, 0, NULL, NULL, "losses is required"), "null losses");
  bad = good; bad.stats = NULL; expect(rl_refused(&bad, 0, NULL, NULL, "stats is required"), "null stats");
  bad = good; bad.stats = NULL; expect(rl_refused(&bad, 1, up, d_pred, "stats is required"), "backward, null stats");
  bad = good; bad.pred = (const float *)((const char *)pred + 1);
  expect(rl_refused(&bad, 0, NULL, NULL, "pred and gt must be 4-byte aligned"), "misaligned pred");
  bad = good; bad.gt = (const float *)((const char *)gt + 2);
  expect(rl_refused(&bad, 0, NULL, NULL, "pred and gt must be 4-byte aligned"), "misaligned gt");
  bad = good; bad.stats = (double *)((char *)stats + 4);
  expect(rl_refused(&bad, 0, NULL, NULL, "stats must be 8-byte aligned"), "misaligned stats");
  bad = good; bad.losses = (float *)((char *)losses + 3);
  expect(rl_refused(&bad, 0, NULL, NULL, "losses must be 4-byte aligned"), "misaligned losses");
  bad = good; bad.workspace = NULL;
  expect(rl_refused(&bad, 0, NULL, NULL, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1;
  expect(rl_refused(&bad, 0, NULL, NULL, "needed"), "short workspace");
  bad = good; bad.workspace_bytes = ws_values;
  expect(rl_refused(&bad, 0, NULL, NULL, "needed"), "the values workspace for a loss");
  bad = good; bad.workspace = (char *)ws + 4;
  expect(rl_refused(&bad, 0, NULL, NULL, "16-byte aligned"), "misaligned workspace");
  bad = good; bad.quantile = NAN;      expect(rl_refused(&bad, 0, NULL, NULL, "quantile must be in [0, 1]"), "NaN q");
  bad = good; bad.quantile = INFINITY; expect(rl_refused(&bad, 0, NULL, NULL, "quantile must be in [0, 1]"), "infinite q");
  bad = good; bad.quantile = -1e-9;    expect(rl_refused(&bad, 0, NULL, NULL, "quantile must be in [0, 1]"), "q < 0");
  bad = good; bad.quantile = 1.0 + 1e-9; expect(rl_refused(&bad, 0, NULL, NULL, "quantile must be in [0, 1]"), "q > 1");
  bad = full; bad.mask_batch_stride = 7;
  expect(rl_refused(&bad, 0, NULL, NULL, "mask_batch_stride"), "odd mask stride");
  bad = good; bad.over_masked = 1; expect(rl_refused(&bad, 0, NULL, NULL, "over_masked needs a mask"), "no mask");
  bad = full; bad.norm_width = 0; expect(rl_refused(&bad, 0, NULL, NULL, "norm_width must be > 0"), "width 0");
  expect(rl_refused(&good, 1, NULL, d_pred, "dL_dloss"), "backward without dL_dloss");
  expect(rl_refused(&good, 1, up, NULL, "dL_dpred"), "backward without dL_dpred");
  expect(rl_refused(&good, 1, up, (const float *)((const char *)d_pred + 3), "4-byte aligned"), "misaligned dL_dpred");

  free(pred); free(gt); free(d_pred); free(mask); free(losses); free(up); free(stats); free(ws);
  if (failures) return 1;
  printf("robust loss host sanitize ok\n");
  return 0;
}
