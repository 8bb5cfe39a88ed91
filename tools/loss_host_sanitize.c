/* loss_host_sanitize.c -- stand-alone driver of the photometric loss's host
 * validator (dynamic3dgaussians_amd/csrc/gs_loss_host.cpp) for a CPU
 * sanitizer build (tests/test_image_loss.py compiles this file, gs_host.cpp
 * and gs_loss_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks; the validator must
 * accept / refuse each one with a message and touch nothing it was not given.
 * The pointers name heap buffers of the right size, none of which the
 * validator may dereference.  Exit status 0 and "loss host sanitize ok" on
 * success. */
#include <math.h>
#include <stdlib.h>

#include "gs_loss.h"
#include "host_sanitize.h"

static int loss_refused(const gs_photo_loss *a, int backward, const float *up, const float *di, const float *dg,
                        const float *dofs, const char *needle) {
  return refused(gs_photo_loss_validate(a, backward, up, di, dg, dofs), needle);
}

int main(void) {
  const int B = 2, Ch = 3, H = 37, W = 53;
  const size_t n = (size_t)B * Ch * H * W;
  const size_t ws_bytes = gs_photo_loss_workspace_bytes(B, Ch, H, W);
  expect(ws_bytes >= 3 * n * sizeof(float), "workspace holds three planes");
  expect(gs_photo_loss_workspace_bytes(0, Ch, H, W) == 0 && gs_photo_loss_workspace_bytes(B, Ch, -4, W) == 0,
         "workspace of an empty shape is 0");
  expect(gs_photo_loss_struct_bytes() == sizeof(gs_photo_loss), "struct size");

  float *image = malloc(n * sizeof(float)), *target = malloc(n * sizeof(float));
  float *d_image = malloc(n * sizeof(float));
  float *mask = malloc((size_t)B * H * W * sizeof(float));
  float *gain = malloc((size_t)B * Ch * sizeof(float)), *offset = malloc((size_t)B * Ch * sizeof(float));
  float *d_gain = malloc((size_t)B * Ch * sizeof(float)), *d_offset = malloc((size_t)B * Ch * sizeof(float));
  float *losses = malloc(B * sizeof(float)), *up = malloc(B * sizeof(float));
  void *ws = aligned_alloc(256, ws_bytes);
  if (!image || !target || !d_image || !mask || !gain || !offset || !d_gain || !d_offset || !losses || !up || !ws)
    return 2;

  gs_photo_loss good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.Ch = Ch; good.H = H; good.W = W;
  good.image = image; good.target = target;
  good.l1_weight = 0.8f; good.ssim_weight = 0.2f;
  good.losses = losses; good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks: bare, with every optional input, forward and backward */
  expect(gs_photo_loss_validate(&good, 0, NULL, NULL, NULL, NULL) == 0, "bare forward block");
  gs_photo_loss full = good;
  full.mask = mask; full.mask_batch_stride = (int64_t)H * W; full.gain = gain; full.offset = offset;
  expect(gs_photo_loss_validate(&full, 0, NULL, NULL, NULL, NULL) == 0, "full forward block");
  expect(gs_photo_loss_validate(&full, 1, up, d_image, d_gain, d_offset) == 0, "full backward block");
  expect(gs_photo_loss_validate(&good, 1, up, d_image, NULL, NULL) == 0, "backward without correction");
  full.mask_batch_stride = 0;
  expect(gs_photo_loss_validate(&full, 0, NULL, NULL, NULL, NULL) == 0, "shared [H, W] mask");

  /* invalid blocks, one fault each */
  gs_photo_loss bad;
  expect(loss_refused(NULL, 0, NULL, NULL, NULL, NULL, "null argument block"), "null block");
  bad = good; bad.B = 0;   expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "must be > 0"), "B = 0");
  bad = good; bad.Ch = -3; expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "must be > 0"), "Ch < 0");
  bad = good; bad.H = 0;   expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "must be > 0"), "H = 0");
  bad = good; bad.W = -1;  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "must be > 0"), "W < 0");
  bad = good; bad.image = NULL;  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "required"), "null image");
  bad = good; bad.target = NULL; expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "required"), "null target");
  bad = good; bad.losses = NULL; expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "required"), "null losses");
  bad = good; bad.image = (const float *)((const char *)image + 1);
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "4-byte aligned"), "misaligned image");
  bad = good; bad.target = (const float *)((const char *)target + 2);
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "4-byte aligned"), "misaligned target");
  bad = good; bad.workspace = NULL;
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1;
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "needed"), "short workspace");
  bad = good; bad.l1_weight = NAN;
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "finite"), "NaN l1_weight");
  bad = good; bad.ssim_weight = INFINITY;
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "finite"), "infinite ssim_weight");
  bad = full; bad.mask_batch_stride = 7;
  expect(loss_refused(&bad, 0, NULL, NULL, NULL, NULL, "mask_batch_stride"), "odd mask stride");
  expect(loss_refused(&good, 1, NULL, d_image, NULL, NULL, "dL_dloss"), "backward without dL_dloss");
  expect(loss_refused(&good, 1, up, NULL, NULL, NULL, "dL_dimage"), "backward without dL_dimage");
  expect(loss_refused(&good, 1, up, (const float *)((const char *)d_image + 3), NULL, NULL, "4-byte aligned"),
         "misaligned dL_dimage");

  free(image); free(target); free(d_image); free(mask); free(gain); free(offset); free(d_gain); free(d_offset);
  free(losses); free(up); free(ws);
  if (failures) return 1;
  printf("loss host sanitize ok\n");
  return 0;
}
