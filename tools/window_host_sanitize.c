/* window_host_sanitize.c -- stand-alone driver of the temporal-window
 * validator (dynamic3dgaussians_amd/csrc/gs_window_host.cpp) for a CPU
 * sanitizer build (tests/test_window.py compiles this file, gs_host.cpp and
 * gs_window_host.cpp with -fsanitize=address,undefined and runs the program).
 * It walks valid and invalid windows; the validator must accept / refuse each
 * one with a message and read exactly the C frames it was given: every frame
 * array is a heap block of exactly C entries, so a read past it is an ASan
 * report.  Exit status 0 and "window host sanitize ok" on success. */
#include <stdlib.h>

#include "gs_window.h"
#include "host_sanitize.h"

/* a heap copy of n frames (exactly n entries) */
static int32_t *frames_of(const int32_t *src, int n) {
  int32_t *f = malloc(n > 0 ? (size_t)n * sizeof(int32_t) : 1);
  if (!f) exit(2);
  memcpy(f, src, (size_t)n * sizeof(int32_t));
  return f;
}

static int check(int B, const int32_t *src, int C) {
  int32_t *f = frames_of(src, C);
  gs_window w;
  w.B = B;
  w.cam_frame = f;
  const int r = gs_check_window(&w, C);
  free(f);
  return r;
}

int main(void) {
  /* valid windows */
  const int32_t one[1] = {0};
  const int32_t gaps[4] = {0, 0, 2, 2};
  int32_t all[GS_WINDOW_MAX_FRAMES];
  for (int i = 0; i < GS_WINDOW_MAX_FRAMES; ++i) all[i] = i;
  expect(check(1, one, 1) == 0, "C = 1, B = 1");
  expect(check(64, one, 1) == 0, "C = 1 in a 64-frame window");
  expect(check(3, gaps, 4) == 0, "a frame without cameras");
  expect(check(GS_WINDOW_MAX_FRAMES, all, GS_WINDOW_MAX_FRAMES) == 0, "64 frames, one camera each");
  const int32_t same[5] = {2, 2, 2, 2, 2};
  expect(check(3, same, 5) == 0, "every camera at the last frame");

  /* invalid windows, one fault each */
  expect(refused(gs_check_window(NULL, 1), "null window"), "null window");
  gs_window w;
  w.B = 2;
  w.cam_frame = NULL;
  expect(refused(gs_check_window(&w, 1), "null cam_frame"), "null frame array");
  expect(refused(check(0, one, 1), "B must be in [1, 64]"), "B = 0");
  expect(refused(check(65, one, 1), "B must be in [1, 64]"), "B = 65");
  expect(refused(check(-1, one, 1), "B must be"), "B < 0");
  const int32_t at_b[3] = {0, 1, 2};
  expect(refused(check(2, at_b, 3), "cam_frame[2] = 2 is outside [0, 2)"), "a frame equal to B");
  const int32_t neg[2] = {-1, 0};
  expect(refused(check(2, neg, 2), "cam_frame[0] = -1 is outside"), "a negative frame");
  const int32_t dec[3] = {0, 1, 0};
  expect(refused(check(2, dec, 3), "non-decreasing"), "a decreasing pair");
  const int32_t dec2[2] = {1, 0};
  expect(refused(check(2, dec2, 2), "cam_frame[1] = 0 after 1"), "[1, 0]");
  expect(refused(check(1, one, 0), "camera count"), "C = 0");
  /* the first C frames only: what follows them is not the validator's */
  const int32_t tail[3] = {0, 1, 7};
  int32_t *f = frames_of(tail, 3);
  w.B = 2;
  w.cam_frame = f;
  expect(gs_check_window(&w, 2) == 0, "frames past C are not read");
  free(f);

  if (failures) return 1;
  printf("window host sanitize ok\n");
  return 0;
}
