/* metrics_host_sanitize.c -- stand-alone driver of the evaluation metrics'
 * host validators (dynamic3dgaussians_amd/csrc/gs_metrics_host.cpp) for a CPU
 * sanitizer build (tests/test_metrics.py compiles this file, gs_host.cpp and
 * gs_metrics_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks; the validators must
 * accept / refuse each one with a message and touch nothing they were not
 * given.  The pointers name heap buffers of the right size, none of which the
 * validators may dereference.  Exit status 0 and "metrics host sanitize ok"
 * on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_metrics.h"
#include "host_sanitize.h"

int main(void) {
  const int B = 2, Ch = 3, H = 45, W = 77;
  const size_t n = (size_t)B * Ch * H * W;
  const size_t ws_bytes = gs_image_metrics_workspace_bytes(B, Ch, H, W);
  /* 2 x 3 tiles of 32 x 32 cover 45 x 77; four floats per workgroup */
  expect(ws_bytes >= (size_t)B * Ch * 2 * 3 * 4 * sizeof(float), "workspace holds every workgroup's partials");
  expect(gs_image_metrics_workspace_bytes(0, Ch, H, W) == 0 && gs_image_metrics_workspace_bytes(B, Ch, -4, W) == 0 &&
             gs_image_metrics_workspace_bytes(B, -1, H, W) == 0 && gs_image_metrics_workspace_bytes(B, Ch, H, 0) == 0,
         "workspace of an empty shape is 0");
  expect(gs_image_metrics_struct_bytes() == sizeof(struct gs_image_metrics), "struct size");

  float *pred = malloc(n * sizeof(float)), *target = malloc(n * sizeof(float));
  float *mask = malloc((size_t)B * H * W * sizeof(float));
  float *out = malloc((size_t)B * 4 * sizeof(float));
  int64_t *counts = malloc((size_t)B * 2 * sizeof(int64_t));
  void *ws = aligned_alloc(256, ws_bytes);
  if (!pred || !target || !mask || !out || !counts || !ws) return 2;

  struct gs_image_metrics good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.Ch = Ch; good.H = H; good.W = W;
  good.pred = pred; good.target = target;
  good.want_ssim = 1;
  good.out = out; good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  expect(gs_image_metrics_validate(&good) == 0, "bare block");
  struct gs_image_metrics full = good;
  full.mask = mask; full.mask_batch_stride = (int64_t)H * W;
  expect(gs_image_metrics_validate(&full) == 0, "per-image masks");
  full.mask_batch_stride = 0;
  expect(gs_image_metrics_validate(&full) == 0, "shared [H, W] mask");
  struct gs_image_metrics tiny = good;
  tiny.H = 9; tiny.W = 7; tiny.want_ssim = 0;
  expect(gs_image_metrics_validate(&tiny) == 0, "sums only below the window's size");
  tiny = good; tiny.H = 11; tiny.W = 11;
  expect(gs_image_metrics_validate(&tiny) == 0, "one window");

  /* invalid blocks, one fault each */
  struct gs_image_metrics bad;
  expect(refused(gs_image_metrics_validate(NULL), "null argument block"), "null block");
  bad = good; bad.B = 0;   expect(refused(gs_image_metrics_validate(&bad), "must be > 0"), "B = 0");
  bad = good; bad.Ch = -3; expect(refused(gs_image_metrics_validate(&bad), "must be > 0"), "Ch < 0");
  bad = good; bad.H = 0;   expect(refused(gs_image_metrics_validate(&bad), "must be > 0"), "H = 0");
  bad = good; bad.W = -1;  expect(refused(gs_image_metrics_validate(&bad), "must be > 0"), "W < 0");
  bad = good; bad.pred = NULL;   expect(refused(gs_image_metrics_validate(&bad), "required"), "null pred");
  bad = good; bad.target = NULL; expect(refused(gs_image_metrics_validate(&bad), "required"), "null target");
  bad = good; bad.out = NULL;    expect(refused(gs_image_metrics_validate(&bad), "out is required"), "null out");
  bad = good; bad.pred = (const float *)((const char *)pred + 1);
  expect(refused(gs_image_metrics_validate(&bad), "4-byte aligned"), "misaligned pred");
  bad = full; bad.mask_batch_stride = 7;
  expect(refused(gs_image_metrics_validate(&bad), "mask_batch_stride"), "odd mask stride");
  bad = good; bad.workspace = NULL;
  expect(refused(gs_image_metrics_validate(&bad), "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1;
  expect(refused(gs_image_metrics_validate(&bad), "needed"), "short workspace");
  bad = good; bad.H = 10;
  expect(refused(gs_image_metrics_validate(&bad), "no window fits"), "SSIM with H < 11");
  bad = good; bad.W = 10;
  expect(refused(gs_image_metrics_validate(&bad), "no window fits"), "SSIM with W < 11");
  bad = good; bad.B = 1 << 20; bad.Ch = 1 << 10; bad.H = 1 << 10; bad.W = 1 << 10;
  expect(refused(gs_image_metrics_validate(&bad), "too large"), "more workgroups than a grid holds");

  /* mask IoU */
  const int64_t px = (int64_t)H * W;
  expect(gs_mask_iou_validate(B, px, pred, target, 0.9f, counts) == 0, "mask IoU block");
  expect(gs_mask_iou_validate(B, px, pred, target, 0.f, counts) == 0, "mask IoU at threshold 0");
  expect(refused(gs_mask_iou_validate(0, px, pred, target, 0.9f, counts), "must be > 0"), "IoU B = 0");
  expect(refused(gs_mask_iou_validate(B, 0, pred, target, 0.9f, counts), "must be > 0"), "IoU n = 0");
  expect(refused(gs_mask_iou_validate(1 << 20, px, pred, target, 0.9f, counts), "too large"), "IoU B too large");
  expect(refused(gs_mask_iou_validate(B, px, NULL, target, 0.9f, counts), "required"), "IoU null pred");
  expect(refused(gs_mask_iou_validate(B, px, pred, NULL, 0.9f, counts), "required"), "IoU null target");
  expect(refused(gs_mask_iou_validate(B, px, pred, target, 0.9f, NULL), "out is required"), "IoU null out");
  expect(refused(gs_mask_iou_validate(B, px, pred, target, NAN, counts), "NaN"), "IoU NaN threshold");
  expect(refused(gs_mask_iou_validate(B, px, (const float *)((const char *)pred + 2), target, 0.9f, counts),
                 "4-byte aligned"), "IoU misaligned pred");
  expect(refused(gs_mask_iou_validate(B, px, pred, target, 0.9f, (const int64_t *)((const char *)counts + 4)),
                 "8-byte aligned"), "IoU misaligned out");

  free(pred); free(target); free(mask); free(out); free(counts); free(ws);
  if (failures) return 1;
  printf("metrics host sanitize ok\n");
  return 0;
}
