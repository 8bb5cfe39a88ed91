/* motion_host_sanitize.c -- stand-alone driver of the motion warp's host
 * validators (dynamic3dgaussians_amd/csrc/gs_motion_host.cpp) for a CPU
 * sanitizer build (tests/test_motion.py compiles this file, gs_host.cpp and
 * gs_motion_host.cpp with -fsanitize=address,undefined and runs the program).
 * It walks valid and invalid descriptors; the validators must accept / refuse
 * each one with a message and touch nothing they were not given.  The
 * pointers name heap buffers of the right size, none of which a validator may
 * dereference.  Exit status 0 and "motion host sanitize ok" on success. */
#include <stdlib.h>

#include "gs_motion.h"
#include "host_sanitize.h"

static int fwd_refused(const gs_motion_desc *d, const float *pos, const float *tf, const char *needle) {
  return refused(gs_motion_forward_validate(d, pos, tf, NULL), needle);
}

int main(void) {
  const int64_t G = 301;
  const int K = 7, T = 12, B = 9;
  float *rots = malloc((size_t)K * T * 6 * sizeof(float)), *transls = malloc((size_t)K * T * 3 * sizeof(float));
  float *coefs = malloc((size_t)G * K * sizeof(float)), *means = malloc((size_t)G * 3 * sizeof(float));
  float *pos = malloc((size_t)G * B * 3 * sizeof(float)), *tf = malloc((size_t)G * B * 12 * sizeof(float));
  float *d_rots = malloc((size_t)K * T * 6 * sizeof(float)), *d_transls = malloc((size_t)K * T * 3 * sizeof(float));
  float *d_coefs = malloc((size_t)G * K * sizeof(float)), *d_means = malloc((size_t)G * 3 * sizeof(float));
  const size_t ws_bytes = gs_motion_workspace_bytes(G, K, B, 1);
  void *ws = aligned_alloc(256, (ws_bytes + 255) / 256 * 256);
  if (!rots || !transls || !coefs || !means || !pos || !tf || !d_rots || !d_transls || !d_coefs || !d_means || !ws)
    return 2;

  /* sizes */
  const int block = gs_motion_backward_block(K, B);
  expect(block == 256 && gs_motion_backward_block(64, 32) == 128, "Gaussians per backward workgroup");
  expect(gs_motion_backward_block(0, B) == 0 && gs_motion_backward_block(K, 33) == 0, "no workgroup outside the envelope");
  expect(ws_bytes >= ((size_t)(G + block - 1) / block + 1) * K * B * 9 * sizeof(float), "workspace holds the slabs and their sum");
  expect(gs_motion_workspace_bytes(G, K, B, 0) == 0, "the forward needs no workspace");
  expect(gs_motion_workspace_bytes(0, K, B, 1) == 0 && gs_motion_workspace_bytes(G, 65, B, 1) == 0 &&
             gs_motion_workspace_bytes(G, K, 0, 1) == 0,
         "workspace outside the envelope is 0");
  expect(gs_motion_struct_bytes() == sizeof(gs_motion_desc), "struct size");

  gs_motion_desc good;
  memset(&good, 0, sizeof(good));
  good.G = G; good.K = K; good.T = T; good.B = B; good.coef_mode = GS_MOTION_COEFS_LOGITS;
  good.rots = rots; good.transls = transls; good.coefs = coefs; good.means = means;
  for (int b = 0; b < B; ++b) good.ts[b] = (5 * b) % T;

  /* valid calls */
  expect(gs_motion_forward_validate(&good, pos, NULL, NULL) == 0, "positions only");
  expect(gs_motion_forward_validate(&good, NULL, tf, NULL) == 0, "transforms only");
  expect(gs_motion_forward_validate(&good, pos, tf, NULL) == 0, "both outputs");
  expect(gs_motion_backward_validate(&good, pos, NULL, d_means, d_coefs, d_rots, d_transls, ws) == 0, "backward");
  expect(gs_motion_backward_validate(&good, pos, tf, NULL, d_coefs, d_rots, d_transls, ws) == 0,
         "backward with both upstream gradients and no d_means");
  gs_motion_desc d = good;
  d.means = NULL;
  expect(gs_motion_forward_validate(&d, NULL, tf, NULL) == 0, "transforms without means");
  expect(gs_motion_backward_validate(&d, NULL, tf, NULL, d_coefs, d_rots, d_transls, ws) == 0,
         "transforms' backward without means");
  d = good; d.G = 0; d.coefs = NULL; d.means = NULL;
  expect(gs_motion_forward_validate(&d, pos, NULL, NULL) == 0, "G = 0 forward");
  expect(gs_motion_backward_validate(&d, NULL, NULL, NULL, NULL, d_rots, d_transls, NULL) == 0, "G = 0 backward");
  d = good; d.K = 64; d.B = 32;
  for (int b = 0; b < 32; ++b) d.ts[b] = b % T;
  expect(gs_motion_forward_validate(&d, pos, NULL, NULL) == 0, "the envelope's corner");

  /* invalid calls, one fault each */
  expect(fwd_refused(NULL, pos, NULL, "null descriptor"), "null descriptor");
  d = good; d.rots = NULL;    expect(fwd_refused(&d, pos, NULL, "required"), "null rots");
  d = good; d.transls = NULL; expect(fwd_refused(&d, pos, NULL, "required"), "null transls");
  d = good; d.coefs = NULL;   expect(fwd_refused(&d, pos, NULL, "coefs is required"), "null coefs");
  d = good; d.means = NULL;   expect(fwd_refused(&d, pos, NULL, "needs means"), "positions without means");
  expect(fwd_refused(&good, NULL, NULL, "positions or transforms"), "both outputs null");
  d = good; d.K = 0;   expect(fwd_refused(&d, pos, NULL, "K must be"), "K = 0");
  d = good; d.K = 65;  expect(fwd_refused(&d, pos, NULL, "K must be"), "K = 65");
  d = good; d.B = 0;   expect(fwd_refused(&d, pos, NULL, "B must be"), "B = 0");
  d = good; d.B = 33;  expect(fwd_refused(&d, pos, NULL, "B must be"), "B = 33");
  d = good; d.T = 0;   expect(fwd_refused(&d, pos, NULL, "T must be"), "T = 0");
  d = good; d.G = -1;  expect(fwd_refused(&d, pos, NULL, "G must be"), "G < 0");
  d = good; d.coef_mode = 2; expect(fwd_refused(&d, pos, NULL, "coef_mode"), "unknown mode");
  d = good; d.ts[B - 1] = T;  expect(fwd_refused(&d, pos, NULL, "outside"), "ts[b] = T");
  d = good; d.ts[0] = -1;     expect(fwd_refused(&d, pos, NULL, "outside"), "ts[b] < 0");
  d = good; d.ts[B] = T + 5;  expect(gs_motion_forward_validate(&d, pos, NULL, NULL) == 0, "ts past B is not read");
  d = good; d.coefs = (const float *)((const char *)coefs + 2);
  expect(fwd_refused(&d, pos, NULL, "4-byte aligned"), "misaligned coefs");
  expect(fwd_refused(&good, (const float *)((const char *)pos + 1), NULL, "4-byte aligned"), "misaligned positions");
  expect(gs_motion_forward_validate(&good, NULL, tf + 1, NULL) == 0, "transforms need no 16-byte alignment");

  expect(refused(gs_motion_backward_validate(&good, NULL, NULL, d_means, d_coefs, d_rots, d_transls, ws),
                 "d_positions or d_transforms"), "backward without an upstream gradient");
  expect(refused(gs_motion_backward_validate(&good, pos, NULL, d_means, NULL, d_rots, d_transls, ws), "d_coefs"),
         "backward without d_coefs");
  expect(refused(gs_motion_backward_validate(&good, pos, NULL, d_means, d_coefs, NULL, d_transls, ws), "d_rots"),
         "backward without d_rots");
  expect(refused(gs_motion_backward_validate(&good, pos, NULL, d_means, d_coefs, d_rots, d_transls, NULL),
                 "workspace is required"), "backward without workspace");
  expect(refused(gs_motion_backward_validate(&good, pos, NULL, d_means, d_coefs, d_rots, d_transls, (char *)ws + 4),
                 "16-byte"), "misaligned workspace");
  expect(refused(gs_motion_backward_validate(&good, pos, NULL, d_means, (float *)((char *)d_coefs + 3), d_rots,
                                             d_transls, ws), "4-byte aligned"), "misaligned d_coefs");
  d = good; d.means = NULL;
  expect(refused(gs_motion_backward_validate(&d, pos, NULL, NULL, d_coefs, d_rots, d_transls, ws), "needs means"),
         "d_positions without means");

  free(rots); free(transls); free(coefs); free(means); free(pos); free(tf);
  free(d_rots); free(d_transls); free(d_coefs); free(d_means); free(ws);
  if (failures) return 1;
  printf("motion host sanitize ok\n");
  return 0;
}
