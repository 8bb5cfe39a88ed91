/* resample_host_sanitize.c -- stand-alone driver of the bilinear resample's
 * host code (dynamic3dgaussians_amd/csrc/gs_resample_host.cpp) for a CPU
 * sanitizer build (tests/test_resample.py compiles this file, gs_host.cpp and
 * gs_resample_host.cpp with -fsanitize=address,undefined and runs the
 * program).  It walks valid and invalid argument blocks through the validator,
 * which must accept / refuse each one with a message and touch nothing it was
 * not given, and runs the axis export over the edge sizes into heap buffers
 * of exactly O, O and I + 1 elements, checking what the tables must satisfy.
 * Exit status 0 and "resample host sanitize ok" on success. */
#include <math.h>
#include <stdlib.h>

#include "gs_resample.h"
#include "host_sanitize.h"

static int rs_refused(const gs_resample *a, int backward, const float *dy, const float *dx, const char *needle) {
  return refused(gs_resample_validate(a, backward, dy, dx), needle);
}

/* one axis: exact-size buffers, then the invariants of the tables */
static void axis(int I, int O, int align) {
  int32_t *i0 = malloc((size_t)O * sizeof(int32_t)), *first = malloc(((size_t)I + 1) * sizeof(int32_t));
  float *l1 = malloc((size_t)O * sizeof(float));
  if (!i0 || !first || !l1) exit(2);
  for (int i = 0; i <= I; ++i) first[i] = -1;
  expect(gs_resample_axis(I, O, align, i0, l1, first) == 0, "axis export");
  int ok = first[0] == 0 && first[I] == O;
  for (int o = 0; o < O; ++o) {
    ok = ok && i0[o] >= 0 && i0[o] < I && l1[o] >= 0.f && l1[o] < 1.f + 1e-3f;
    ok = ok && (o == 0 || i0[o] >= i0[o - 1]);
    ok = ok && first[i0[o]] <= o && o < first[i0[o] + 1];
  }
  for (int i = 0; i < I; ++i) ok = ok && first[i] >= 0 && first[i] <= first[i + 1];
  if (I == O)
    for (int o = 0; o < O; ++o) ok = ok && i0[o] == o && l1[o] == 0.f;
  if (!ok) fprintf(stderr, "axis %d -> %d align %d\n", I, O, align);
  expect(ok, "axis tables: taps in range, first a non-decreasing partition of [0, O)");
  /* any of the three pointers may be absent */
  expect(gs_resample_axis(I, O, align, NULL, l1, NULL) == 0 && gs_resample_axis(I, O, align, NULL, NULL, first) == 0,
         "axis export with absent tables");
  free(i0); free(first); free(l1);
}

int main(void) {
  const int B = 2, Ch = 3, H = 37, W = 53, h = 12, w = 31;
  const size_t nx = (size_t)B * Ch * H * W, ny = (size_t)B * Ch * h * w;
  const size_t ws_bytes = gs_resample_workspace_bytes(H, W);
  expect(ws_bytes == 160 + 224, "first_y [38] and first_x [54] as int32, each padded to 16 bytes");
  expect(gs_resample_workspace_bytes(0, W) == 0 && gs_resample_workspace_bytes(H, -1) == 0 &&
             gs_resample_workspace_bytes(32769, W) == 0,
         "workspace of a size out of range is 0");
  expect(gs_resample_workspace_bytes(32768, 32768) == 2 * 131088, "largest workspace");
  expect(gs_resample_struct_bytes() == sizeof(gs_resample), "struct size");

  float *x = malloc(nx * sizeof(float)), *d_x = malloc(nx * sizeof(float));
  float *y = malloc(ny * sizeof(float)), *d_y = malloc(ny * sizeof(float));
  void *ws = aligned_alloc(256, (ws_bytes + 255) / 256 * 256);
  if (!x || !d_x || !y || !d_y || !ws) return 2;

  gs_resample good;
  memset(&good, 0, sizeof(good));
  good.B = B; good.Ch = Ch; good.H = H; good.W = W; good.h = h; good.w = w;
  good.x = x; good.y = y; good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  expect(gs_resample_validate(&good, 0, NULL, NULL) == 0, "forward block");
  expect(gs_resample_validate(&good, 1, d_y, d_x) == 0, "backward block");
  gs_resample v = good;
  v.align_corners = 1; v.workspace = NULL; v.workspace_bytes = 0; /* the forward needs no workspace */
  expect(gs_resample_validate(&v, 0, NULL, NULL) == 0, "forward without workspace");
  v = good; v.x = NULL; v.y = NULL; /* the backward needs neither x nor y */
  expect(gs_resample_validate(&v, 1, d_y, d_x) == 0, "backward without x and y");
  v = good; v.H = v.W = v.h = v.w = 1;
  expect(gs_resample_validate(&v, 0, NULL, NULL) == 0, "1 x 1 -> 1 x 1");
  v = good; v.H = v.W = v.h = v.w = 32768; v.workspace_bytes = gs_resample_workspace_bytes(32768, 32768);
  expect(gs_resample_validate(&v, 0, NULL, NULL) == 0, "largest sizes");

  /* invalid blocks, one fault each */
  gs_resample bad;
  expect(rs_refused(NULL, 0, NULL, NULL, "null argument block"), "null block");
  bad = good; bad.B = 0;   expect(rs_refused(&bad, 0, NULL, NULL, "B, Ch must be > 0"), "B = 0");
  bad = good; bad.Ch = -2; expect(rs_refused(&bad, 0, NULL, NULL, "B, Ch must be > 0"), "Ch < 0");
  bad = good; bad.H = 0;     expect(rs_refused(&bad, 0, NULL, NULL, "H, W must be in"), "H = 0");
  bad = good; bad.W = 32769; expect(rs_refused(&bad, 0, NULL, NULL, "H, W must be in"), "W too large");
  bad = good; bad.h = -1;    expect(rs_refused(&bad, 0, NULL, NULL, "h, w must be in"), "h < 0");
  bad = good; bad.w = 40000; expect(rs_refused(&bad, 1, d_y, d_x, "h, w must be in"), "w too large");
  bad = good; bad.x = NULL; expect(rs_refused(&bad, 0, NULL, NULL, "x is required"), "null x");
  bad = good; bad.y = NULL; expect(rs_refused(&bad, 0, NULL, NULL, "y is required"), "null y");
  bad = good; bad.x = (const float *)((const char *)x + 1);
  expect(rs_refused(&bad, 0, NULL, NULL, "x and y must be 4-byte aligned"), "misaligned x");
  bad = good; bad.y = (float *)((char *)y + 2);
  expect(rs_refused(&bad, 0, NULL, NULL, "x and y must be 4-byte aligned"), "misaligned y");
  expect(rs_refused(&good, 1, NULL, d_x, "d_y is required"), "backward without d_y");
  expect(rs_refused(&good, 1, d_y, NULL, "d_x is required"), "backward without d_x");
  expect(rs_refused(&good, 1, d_y, (const float *)((const char *)d_x + 3), "4-byte aligned"), "misaligned d_x");
  bad = good; bad.workspace = NULL;
  expect(rs_refused(&bad, 1, d_y, d_x, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1;
  expect(rs_refused(&bad, 1, d_y, d_x, "needed"), "short workspace");
  bad = good; bad.workspace = (char *)ws + 4;
  expect(rs_refused(&bad, 1, d_y, d_x, "16-byte aligned"), "misaligned workspace");

  /* the axis export over the edge sizes */
  static const int sizes[] = {1, 2, 3, 7, 8, 12, 16, 37, 288, 512, 800, 801, 1080, 32768};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      axis(sizes[a], sizes[b], 0);
      axis(sizes[a], sizes[b], 1);
    }
  expect(refused(gs_resample_axis(0, 4, 0, NULL, NULL, NULL), "I, O must be in"), "axis I = 0");
  expect(refused(gs_resample_axis(4, 32769, 1, NULL, NULL, NULL), "I, O must be in"), "axis O too large");

  free(x); free(d_x); free(y); free(d_y); free(ws);
  if (failures) return 1;
  printf("resample host sanitize ok\n");
  return 0;
}
