/* track_host_sanitize.c -- stand-alone driver of the tracking ops' host code
 * (dynamic3dgaussians_amd/csrc/gs_track_host.cpp: the argument validators
 * gs_check_contributors and gs_check_track_project) for a CPU sanitizer
 * build: compile this file, gs_host.cpp and gs_track_host.cpp with
 * -fsanitize=address,undefined and run the program, on the CPU (DESIGN.md
 * 9.14 gives the command; tests/test_tracking.py runs it, never on a GPU
 * machine).  It walks valid and invalid argument sets; the validators must
 * accept / refuse each one with a message and touch none of the buffers: the
 * outputs are heap blocks of exactly the size the call would write.  Exit
 * status 0 and "track host sanitize ok" on success. */
#include <stdint.h>
#include <stdlib.h>

#include "gs_track.h"
#include "host_sanitize.h"

static void *block(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

/* gs_check_contributors on freshly allocated outputs of C x K x H x W elements (when that is a sane size) */
static int contributors(int64_t P, int32_t C, int32_t W, int32_t H, int32_t K) {
  size_t n = 1;
  if (C > 0 && C <= 64 && K > 0 && K <= 4 && W > 0 && H > 0 && W <= 4096 && H <= 4096)
    n = (size_t)C * (size_t)K * (size_t)W * (size_t)H;
  int32_t *id = block(sizeof(int32_t) * n);
  float *w = block(sizeof(float) * n);
  const int r = gs_check_contributors(P, C, W, H, K, id, w);
  free(id);
  free(w);
  return r;
}

static int project(int64_t P, int32_t T, int32_t C, int64_t N) {
  size_t n = 1;
  if (T > 0 && T <= 1024 && C > 0 && C <= 64 && N > 0 && N <= 65536) n = (size_t)T * (size_t)C * (size_t)N;
  if (n > ((size_t)1 << 20)) n = 1; /* a large valid shape: the validator reads no buffer, a token block will do */
  int32_t *ids = block(sizeof(int32_t) * (size_t)(N > 0 && N <= 65536 ? N : 1));
  float *uv = block(sizeof(float) * 2 * n), *depth = block(sizeof(float) * n);
  uint8_t *inside = block(n);
  const int r = gs_check_track_project(P, T, C, N, ids, uv, depth, inside);
  free(ids); free(uv); free(depth); free(inside);
  return r;
}

int main(void) {
  /* contributor maps: valid argument sets */
  expect(contributors(2000, 1, 128, 96, 1) == 0, "one camera, K = 1");
  expect(contributors(2000, 3, 100, 70, 4) == 0, "three cameras, K = 4");
  expect(contributors(300000, 64, 16, 16, 3) == 0, "C = 64, K = 3");
  expect(contributors(0, 2, 128, 96, 2) == 0, "P = 0");
  expect(gs_check_contributors(2000, 2, 0, 96, 2, NULL, NULL) == 0, "W = 0: nothing to write, no output needed");
  expect(gs_check_contributors(2000, 2, 128, 0, 2, NULL, NULL) == 0, "H = 0: nothing to write, no output needed");

  /* invalid ones, one fault each */
  expect(refused(contributors(2000, 1, 128, 96, 0), "K = 0 outside 1..4"), "K = 0");
  expect(refused(contributors(2000, 1, 128, 96, 5), "K = 5 outside 1..4"), "K = 5");
  expect(refused(contributors(2000, 1, 128, 96, -1), "outside 1..4"), "K < 0");
  expect(refused(contributors(2000, 0, 128, 96, 1), "camera batch size 0 outside 1..64"), "C = 0");
  expect(refused(contributors(2000, 65, 128, 96, 1), "camera batch size 65 outside 1..64"), "C = 65");
  expect(refused(contributors(-1, 1, 128, 96, 1), "P must be"), "P < 0");
  expect(refused(contributors((int64_t)1 << 31, 1, 128, 96, 1), "P must be"), "P = 2^31");
  expect(refused(contributors(2000, 1, -128, 96, 1), "must not be negative"), "W < 0");
  expect(refused(contributors(2000, 1, 128, -96, 1), "must not be negative"), "H < 0");
  int32_t ids4[4];
  float w4[5];
  expect(refused(gs_check_contributors(10, 1, 2, 2, 1, NULL, w4), "are required"), "a null top_id");
  expect(refused(gs_check_contributors(10, 1, 2, 2, 1, ids4, NULL), "are required"), "a null top_w");
  expect(refused(gs_check_contributors(10, 1, 2, 2, 1, (int32_t *)((char *)ids4 + 2), w4), "4-byte aligned"),
         "a misaligned top_id");
  expect(refused(gs_check_contributors(10, 1, 2, 2, 1, ids4, (float *)((char *)w4 + 1)), "4-byte aligned"),
         "a misaligned top_w");
  expect(gs_check_contributors(10, 1, 2, 2, 1, ids4, w4) == 0, "the same set, valid");
  /* the largest image sizes: 64 x 4 x 2^31 x 2^31 elements overflow 2^62 and are refused, not wrapped */
  expect(refused(gs_check_contributors(10, 64, 2147483647, 2147483647, 4, ids4, w4), "exceed 2^62"),
         "an element count past 2^62");

  /* track projection: valid argument sets */
  expect(project(2000, 3, 3, 17) == 0, "T = 3, C = 3, N = 17");
  expect(project(300000, 150, 27, 4096) == 0, "the benchmark shape");
  expect(project(0, 2, 2, 5) == 0, "P = 0");
  expect(gs_check_track_project(2000, 0, 3, 17, NULL, NULL, NULL, NULL) == 0, "T = 0: nothing to write");
  expect(gs_check_track_project(2000, 3, 3, 0, NULL, NULL, NULL, NULL) == 0, "N = 0: nothing to write");

  /* invalid ones */
  expect(refused(project(2000, -1, 3, 17), "T must not be negative"), "T < 0");
  expect(refused(project(2000, 3, 3, -17), "N must not be negative"), "N < 0");
  expect(refused(project(2000, 3, 0, 17), "camera batch size 0 outside 1..64"), "C = 0");
  expect(refused(project(2000, 3, 65, 17), "camera batch size 65 outside 1..64"), "C = 65");
  expect(refused(project(-3, 3, 3, 17), "P must be"), "P < 0");
  expect(refused(project((int64_t)1 << 31, 3, 3, 17), "P must be"), "P = 2^31");
  float uv8[9], d4[5];
  uint8_t in4[4];
  expect(refused(gs_check_track_project(10, 1, 1, 4, NULL, uv8, d4, in4), "ids are required"), "null ids");
  expect(refused(gs_check_track_project(10, 1, 1, 4, ids4, NULL, d4, in4), "are required"), "a null uv");
  expect(refused(gs_check_track_project(10, 1, 1, 4, ids4, uv8, NULL, in4), "are required"), "a null depth");
  expect(refused(gs_check_track_project(10, 1, 1, 4, ids4, uv8, d4, NULL), "are required"), "a null inside");
  /* uv8 is 4-byte aligned; one of uv8 and uv8 + 1 is not 8-byte aligned */
  float *uv_odd = ((uintptr_t)uv8 & 7u) ? uv8 : uv8 + 1;
  expect(refused(gs_check_track_project(10, 1, 1, 4, ids4, uv_odd, d4, in4), "8-byte aligned"), "a misaligned uv");
  expect(refused(gs_check_track_project(10, 1, 1, 4, ids4, ((uintptr_t)uv8 & 7u) ? uv8 + 1 : uv8,
                                        (float *)((char *)d4 + 2), in4), "4-byte aligned"), "a misaligned depth");
  expect(refused(gs_check_track_project(10, 2147483647, 64, (int64_t)1 << 40, ids4, uv8, d4, in4), "exceed 2^62"),
         "an element count past 2^62");

  if (failures) return 1;
  printf("track host sanitize ok\n");
  return 0;
}
