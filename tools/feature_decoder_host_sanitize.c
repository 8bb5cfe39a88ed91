/* feature_decoder_host_sanitize.c -- stand-alone driver of the feature
 * decoder's host validator (dynamic3dgaussians_amd/csrc/gs_feature_decoder_host.cpp)
 * for a CPU sanitizer build (tests/test_feature_decoder.py compiles this file,
 * gs_host.cpp and gs_feature_decoder_host.cpp with -fsanitize=address,undefined
 * and runs the program).  It walks valid and invalid argument blocks of all
 * four passes; the validator must accept / refuse each one with a message and
 * touch nothing it was not given.  The pointers name heap buffers, none of
 * which the validator may dereference.  Exit status 0 and "feature decoder
 * host sanitize ok" on success. */
#include <stdlib.h>

#include "gs_feature_decoder.h"
#include "host_sanitize.h"

static int fd_refused(const gs_feature_decoder *a, int pass, const char *needle) {
  return refused(gs_feature_decoder_validate(a, pass), needle);
}

int main(void) {
  const int B = 3, F = 32, C = 64, h = 72, w = 128;
  const size_t frags = (size_t)2 * 2 * 1 * 3 * 64 * 16; /* 2 row tiles, 2 k-steps, 3 pieces of 64 x 16 bytes */
  const int gx = gs_feature_decoder_grid_x(B, h, w);
  expect(gx == 72, "72 tiles, under GS_FD_GRID / 3 blocks per camera");
  expect(gs_feature_decoder_grid_x(27, 288, 512) == GS_FD_GRID / 27, "GS_FD_GRID / 27 blocks per camera");
  expect(gs_feature_decoder_grid_x(600, 288, 512) == 1, "at least one block per camera");
  expect(gs_feature_decoder_n_t(C) == 32 && gs_feature_decoder_n_t(1) == 16 && gs_feature_decoder_n_t(513) == 0, "n_t");
  expect(gs_feature_decoder_n_acc(B, h, w) == 128 && gs_feature_decoder_n_acc(27, 288, 512) == (1152 + GS_FD_GRID / 27 - 1) / (GS_FD_GRID / 27) * 128, "n_acc");
  expect(gs_feature_decoder_workspace_bytes(B, F, C, h, w, GS_FD_PASS_DECODE) == frags, "decode: W's fragments");
  expect(gs_feature_decoder_workspace_bytes(B, F, C, h, w, GS_FD_PASS_LOSS) == frags + (size_t)B * gx * 8,
         "loss: and the partials");
  const size_t ws_bwd = gs_feature_decoder_workspace_bytes(B, F, C, h, w, GS_FD_PASS_LOSS_BACKWARD);
  expect(ws_bwd == 2 * frags + (size_t)B * gx * (C * F + C) * 4, "loss backward: both fragment sets and the slabs");
  expect(gs_feature_decoder_workspace_bytes(B, F, C, h, w, GS_FD_PASS_BACKWARD) == ws_bwd - frags, "backward");
  expect(gs_feature_decoder_workspace_bytes(0, F, C, h, w, 0) == 0 && gs_feature_decoder_workspace_bytes(B, 65, C, h, w, 0) == 0 &&
             gs_feature_decoder_workspace_bytes(B, F, 513, h, w, 0) == 0 &&
             gs_feature_decoder_workspace_bytes(B, 64, 257, h, w, 0) == 0 &&
             gs_feature_decoder_workspace_bytes(B, F, C, 0, w, 0) == 0 && gs_feature_decoder_workspace_bytes(B, F, C, h, w, 4) == 0,
         "workspace of a size out of range or an unknown pass is 0");
  expect(gs_feature_decoder_workspace_bytes(27, 32, 512, 288, 512, GS_FD_PASS_LOSS_BACKWARD) < ((size_t)64 << 20),
         "slabs sized by the grid at the largest workload");
  expect(gs_feature_decoder_struct_bytes() == sizeof(gs_feature_decoder), "struct size");

  float *x = malloc(64), *wt = malloc(64), *bias = malloc(64), *target = malloc(64), *mask = malloc(64);
  float *up = malloc(64), *d_y = malloc(64), *y = malloc(64), *loss = malloc(64), *d_x = malloc(64);
  float *d_w = malloc(64), *d_b = malloc(64);
  void *ws = aligned_alloc(256, (ws_bwd + 255) / 256 * 256);
  if (!x || !wt || !bias || !target || !mask || !up || !d_y || !y || !loss || !d_x || !d_w || !d_b || !ws) return 2;

  gs_feature_decoder good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.F_in = F; good.C_out = C; good.h = h; good.w = w;
  good.x = x; good.weight = wt; good.bias = bias; good.target = target; good.mask = mask; good.up = up; good.d_y = d_y;
  good.y = y; good.loss = loss; good.d_x = d_x; good.d_weight = d_w; good.d_bias = d_b;
  good.workspace = ws; good.workspace_bytes = ws_bwd;

  /* valid blocks */
  for (int pass = 0; pass < 4; ++pass) expect(gs_feature_decoder_validate(&good, pass) == 0, "full block");
  gs_feature_decoder bare = good;
  bare.bias = NULL; bare.mask = NULL; bare.d_bias = NULL; bare.mask_per_camera = 1;
  for (int pass = 0; pass < 4; ++pass) expect(gs_feature_decoder_validate(&bare, pass) == 0, "no bias, no mask");
  gs_feature_decoder dec = good;
  dec.target = NULL; dec.up = NULL; dec.d_y = NULL; dec.loss = NULL; dec.d_x = NULL; dec.d_weight = NULL;
  dec.workspace_bytes = frags;
  expect(gs_feature_decoder_validate(&dec, GS_FD_PASS_DECODE) == 0, "decode needs x, weight, y and W's fragments only");
  gs_feature_decoder corner = good;
  corner.F_in = 32; corner.C_out = 512;
  corner.workspace_bytes = gs_feature_decoder_workspace_bytes(B, 32, 512, h, w, GS_FD_PASS_DECODE);
  expect(gs_feature_decoder_validate(&corner, GS_FD_PASS_DECODE) == 0, "32 x 512");
  corner.F_in = 64; corner.C_out = 256;
  expect(gs_feature_decoder_validate(&corner, GS_FD_PASS_DECODE) == 0, "64 x 256");
  corner = good; corner.B = 1; corner.F_in = 1; corner.C_out = 1; corner.h = 1; corner.w = 1;
  expect(gs_feature_decoder_validate(&corner, GS_FD_PASS_LOSS_BACKWARD) == 0, "all ones");

  /* invalid blocks, one fault each */
  gs_feature_decoder bad;
  expect(fd_refused(NULL, 0, "null argument block"), "null block");
  expect(fd_refused(&good, 4, "unknown pass"), "pass 4");
  expect(fd_refused(&good, -1, "unknown pass"), "pass -1");
  bad = good; bad.B = 0; expect(fd_refused(&bad, 0, "B must be in"), "B = 0");
  bad = good; bad.B = 65536; expect(fd_refused(&bad, 0, "B must be in"), "B past the grid");
  bad = good; bad.F_in = 0; expect(fd_refused(&bad, 0, "F_in must be in"), "F_in = 0");
  bad = good; bad.F_in = 65; expect(fd_refused(&bad, 1, "decoded_l1_loss_torch"), "F_in = 65 names the twin");
  bad = good; bad.C_out = 0; expect(fd_refused(&bad, 0, "C_out must be in"), "C_out = 0");
  bad = good; bad.C_out = 513; expect(fd_refused(&bad, 2, "decode_features_torch"), "C_out = 513 names the twin");
  bad = good; bad.F_in = 64; bad.C_out = 257; expect(fd_refused(&bad, 3, "F_in * C_out must be <= 16384"), "64 x 257");
  bad = good; bad.F_in = 64; bad.C_out = 257; expect(fd_refused(&bad, 3, "_torch"), "64 x 257 names the twin");
  bad = good; bad.h = 0; expect(fd_refused(&bad, 0, "h, w must be >= 1"), "h = 0");
  bad = good; bad.w = -5; expect(fd_refused(&bad, 0, "h, w must be >= 1"), "w < 0");
  bad = good; bad.h = 65536; bad.w = 32768; expect(fd_refused(&bad, 0, "h * w"), "h * w = 2^31");
  bad = good; bad.weight = NULL; expect(fd_refused(&bad, 0, "weight is required"), "null weight");
  for (int pass = 0; pass < 4; ++pass) {
    bad = good; bad.x = NULL; expect(fd_refused(&bad, pass, "x is required"), "null x");
  }
  bad = good; bad.y = NULL; expect(fd_refused(&bad, GS_FD_PASS_DECODE, "y is required"), "null y");
  bad = good; bad.target = NULL; expect(fd_refused(&bad, GS_FD_PASS_LOSS, "target is required"), "null target");
  bad = good; bad.target = NULL; expect(fd_refused(&bad, GS_FD_PASS_LOSS_BACKWARD, "target is required"), "null target");
  bad = good; bad.loss = NULL; expect(fd_refused(&bad, GS_FD_PASS_LOSS, "loss is required"), "null loss");
  bad = good; bad.up = NULL; expect(fd_refused(&bad, GS_FD_PASS_LOSS_BACKWARD, "up is required"), "null up");
  bad = good; bad.d_y = NULL; expect(fd_refused(&bad, GS_FD_PASS_BACKWARD, "d_y is required"), "null d_y");
  bad = good; bad.d_x = NULL; expect(fd_refused(&bad, GS_FD_PASS_BACKWARD, "d_x is required"), "null d_x");
  bad = good; bad.d_x = NULL; expect(fd_refused(&bad, GS_FD_PASS_LOSS_BACKWARD, "d_x is required"), "null d_x");
  bad = good; bad.d_weight = NULL; expect(fd_refused(&bad, GS_FD_PASS_BACKWARD, "d_weight is required"), "null d_weight");
  bad = good; bad.x = (const float *)((const char *)x + 1); expect(fd_refused(&bad, 0, "4-byte aligned"), "misaligned x");
  bad = good; bad.d_bias = (float *)((char *)d_b + 2); expect(fd_refused(&bad, 3, "4-byte aligned"), "misaligned d_bias");
  bad = good; bad.workspace = NULL; expect(fd_refused(&bad, 0, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bwd - 1;
  expect(fd_refused(&bad, GS_FD_PASS_LOSS_BACKWARD, "needed"), "short workspace");
  bad = good; bad.workspace_bytes = frags; expect(fd_refused(&bad, GS_FD_PASS_LOSS, "needed"), "the decode workspace for a loss");
  bad = good; bad.workspace = (char *)ws + 4; expect(fd_refused(&bad, 0, "16-byte aligned"), "misaligned workspace");

  free(x); free(wt); free(bias); free(target); free(mask); free(up); free(d_y); free(y); free(loss); free(d_x);
  free(d_w); free(d_b); free(ws);
  if (failures) return 1;
  printf("feature decoder host sanitize ok\n");
  return 0;
}
