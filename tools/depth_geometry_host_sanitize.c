/* depth_geometry_host_sanitize.c -- stand-alone driver of the depth-map
 * geometry's host validators and size functions
 * (dynamic3dgaussians_amd/csrc/gs_depth_geometry_host.cpp) for a CPU
 * sanitizer build (tests/test_depth_geometry.py compiles this file,
 * gs_host.cpp and gs_depth_geometry_host.cpp with
 * -fsanitize=address,undefined and runs the program).  It walks valid and
 * invalid argument blocks; the validators must accept / refuse each one with
 * a message and touch nothing they were not given.  The pointers name heap
 * buffers of the right size, none of which the validators may dereference.
 * Exit status 0 and "depth geometry host sanitize ok" on success. */
#include <stdlib.h>

#include "gs_depth_geometry.h"
#include "host_sanitize.h"

int main(void) {
  const int B = 2, Ch = 3, H = 37, W = 53;
  const int64_t P = 4097, N = 257;
  const size_t px = (size_t)B * H * W;
  const size_t ws_bytes = gs_depth_abs_rel_workspace_bytes(B, H, W);
  expect(ws_bytes >= (size_t)B * 2 * sizeof(double), "workspace holds a partial pair per image at least");
  expect(gs_depth_abs_rel_workspace_bytes(27, 800, 800) >= (size_t)27 * 157 * 2 * sizeof(double),
         "workspace of 27 x 800 x 800: 157 chunks of 4096 pixels per image");
  expect(gs_depth_abs_rel_workspace_bytes(0, H, W) == 0 && gs_depth_abs_rel_workspace_bytes(B, -4, W) == 0 &&
             gs_depth_abs_rel_workspace_bytes(B, H, 0) == 0,
         "workspace of an empty shape is 0");
  expect(gs_point_depth_struct_bytes() == sizeof(struct gs_point_depth), "point depth struct size");
  expect(gs_depth_abs_rel_struct_bytes() == sizeof(struct gs_depth_abs_rel), "abs-rel struct size");
  expect(gs_depth_unproject_struct_bytes() == sizeof(struct gs_depth_unproject), "unproject struct size");
  expect(gs_depth_flow_struct_bytes() == sizeof(struct gs_depth_flow), "flow struct size");
  expect(gs_sample_bilinear_struct_bytes() == sizeof(struct gs_sample_bilinear), "sampler struct size");

  float *points = malloc((size_t)B * P * 3 * sizeof(float));
  float *m4 = malloc((size_t)B * 16 * sizeof(float)), *m3 = malloc((size_t)B * 9 * sizeof(float));
  float *map = malloc(px * sizeof(float)), *map2 = malloc(px * sizeof(float)), *mask = malloc(px * sizeof(float));
  float *big = malloc(px * Ch * sizeof(float)), *xy = malloc((size_t)B * N * 2 * sizeof(float));
  float *outp = malloc((size_t)B * Ch * N * sizeof(float));
  double *sums = malloc((size_t)B * 2 * sizeof(double));
  uint8_t *valid = malloc(px);
  void *ws = aligned_alloc(256, ws_bytes);
  if (!points || !m4 || !m3 || !map || !map2 || !mask || !big || !xy || !outp || !sums || !valid || !ws) return 2;

  /* gs_point_depth */
  struct gs_point_depth pd;
  memset(&pd, 0, sizeof(pd));
  pd.P = P; pd.B = B; pd.H = H; pd.W = W;
  pd.points = points; pd.w2c = m4; pd.K = m3; pd.depth = map;
  expect(gs_point_depth_validate(&pd) == 0, "shared cloud");
  struct gs_point_depth pb = pd;
  pb.points_batch_stride = P * 3;
  expect(gs_point_depth_validate(&pb) == 0, "a cloud per camera");
  pb = pd; pb.P = 0; pb.points = NULL;
  expect(gs_point_depth_validate(&pb) == 0, "empty cloud");
  expect(refused(gs_point_depth_validate(NULL), "null argument block"), "point depth null block");
  pb = pd; pb.B = 0;  expect(refused(gs_point_depth_validate(&pb), "must be > 0"), "point depth B = 0");
  pb = pd; pb.H = -1; expect(refused(gs_point_depth_validate(&pb), "must be > 0"), "point depth H < 0");
  pb = pd; pb.W = 0;  expect(refused(gs_point_depth_validate(&pb), "must be > 0"), "point depth W = 0");
  pb = pd; pb.W = 1 << 20; expect(refused(gs_point_depth_validate(&pb), "too large"), "point depth W too large");
  pb = pd; pb.B = 1 << 17; expect(refused(gs_point_depth_validate(&pb), "too large"), "point depth B too large");
  pb = pd; pb.P = -1; expect(refused(gs_point_depth_validate(&pb), "P must be"), "point depth P < 0");
  pb = pd; pb.points = NULL; expect(refused(gs_point_depth_validate(&pb), "points are required"), "null points");
  pb = pd; pb.w2c = NULL; expect(refused(gs_point_depth_validate(&pb), "required"), "null w2c");
  pb = pd; pb.K = NULL; expect(refused(gs_point_depth_validate(&pb), "required"), "null K");
  pb = pd; pb.depth = NULL; expect(refused(gs_point_depth_validate(&pb), "depth is required"), "null depth");
  pb = pd; pb.points = (const float *)((const char *)points + 2);
  expect(refused(gs_point_depth_validate(&pb), "4-byte aligned"), "misaligned points");
  pb = pd; pb.points_batch_stride = 7;
  expect(refused(gs_point_depth_validate(&pb), "points_batch_stride"), "odd cloud stride");
  pb = pd; pb.points_batch_stride = P;
  expect(refused(gs_point_depth_validate(&pb), "points_batch_stride"), "cloud stride P, not P*3");

  /* gs_depth_abs_rel */
  struct gs_depth_abs_rel ar;
  memset(&ar, 0, sizeof(ar));
  ar.B = B; ar.H = H; ar.W = W;
  ar.est = map; ar.gt = map2; ar.out = sums; ar.workspace = ws; ar.workspace_bytes = ws_bytes;
  expect(gs_depth_abs_rel_validate(&ar) == 0, "abs-rel without exclude");
  struct gs_depth_abs_rel ab = ar;
  ab.exclude = mask; ab.exclude_batch_stride = (int64_t)H * W;
  expect(gs_depth_abs_rel_validate(&ab) == 0, "abs-rel with per-image exclude");
  ab.exclude_batch_stride = 0;
  expect(gs_depth_abs_rel_validate(&ab) == 0, "abs-rel with a shared exclude");
  ab.exclude_batch_stride = 5;
  expect(refused(gs_depth_abs_rel_validate(&ab), "exclude_batch_stride"), "odd exclude stride");
  expect(refused(gs_depth_abs_rel_validate(NULL), "null argument block"), "abs-rel null block");
  ab = ar; ab.B = 0;  expect(refused(gs_depth_abs_rel_validate(&ab), "must be > 0"), "abs-rel B = 0");
  ab = ar; ab.H = 0;  expect(refused(gs_depth_abs_rel_validate(&ab), "must be > 0"), "abs-rel H = 0");
  ab = ar; ab.W = -3; expect(refused(gs_depth_abs_rel_validate(&ab), "must be > 0"), "abs-rel W < 0");
  ab = ar; ab.est = NULL; expect(refused(gs_depth_abs_rel_validate(&ab), "required"), "abs-rel null est");
  ab = ar; ab.gt = NULL;  expect(refused(gs_depth_abs_rel_validate(&ab), "required"), "abs-rel null gt");
  ab = ar; ab.out = NULL; expect(refused(gs_depth_abs_rel_validate(&ab), "out is required"), "abs-rel null out");
  ab = ar; ab.out = (double *)((char *)sums + 4);
  expect(refused(gs_depth_abs_rel_validate(&ab), "8-byte aligned"), "abs-rel misaligned out");
  ab = ar; ab.workspace = NULL;
  expect(refused(gs_depth_abs_rel_validate(&ab), "workspace is required"), "abs-rel null workspace");
  ab = ar; ab.workspace_bytes = ws_bytes - 1;
  expect(refused(gs_depth_abs_rel_validate(&ab), "needed"), "abs-rel short workspace");

  /* gs_depth_unproject */
  struct gs_depth_unproject un;
  memset(&un, 0, sizeof(un));
  un.B = B; un.H = H; un.W = W;
  un.depth = map; un.Kinv = m3; un.c2w = m4; un.xyz = big;
  expect(gs_depth_unproject_validate(&un) == 0, "dense unprojection");
  struct gs_depth_unproject ub = un;
  ub.H = 1; ub.W = (int32_t)N; ub.xy = xy;
  expect(gs_depth_unproject_validate(&ub) == 0, "unprojection at given coordinates");
  expect(refused(gs_depth_unproject_validate(NULL), "null argument block"), "unproject null block");
  ub = un; ub.B = -1; expect(refused(gs_depth_unproject_validate(&ub), "must be > 0"), "unproject B < 0");
  ub = un; ub.H = 0;  expect(refused(gs_depth_unproject_validate(&ub), "must be > 0"), "unproject H = 0");
  ub = un; ub.depth = NULL; expect(refused(gs_depth_unproject_validate(&ub), "depth is required"), "unproject null depth");
  ub = un; ub.Kinv = NULL;  expect(refused(gs_depth_unproject_validate(&ub), "required"), "unproject null Kinv");
  ub = un; ub.c2w = NULL;   expect(refused(gs_depth_unproject_validate(&ub), "required"), "unproject null c2w");
  ub = un; ub.xyz = NULL;   expect(refused(gs_depth_unproject_validate(&ub), "xyz is required"), "unproject null xyz");
  ub = un; ub.xy = (const float *)((const char *)xy + 1);
  expect(refused(gs_depth_unproject_validate(&ub), "4-byte aligned"), "unproject misaligned xy");

  /* gs_depth_flow */
  struct gs_depth_flow fl;
  memset(&fl, 0, sizeof(fl));
  fl.B = B; fl.H = H; fl.W = W;
  fl.depth1 = map; fl.Kinv1 = m3; fl.T = m4; fl.K2 = m3; fl.flow = big;
  expect(gs_depth_flow_validate(&fl) == 0, "flow without valid");
  struct gs_depth_flow fb = fl;
  fb.valid = valid;
  expect(gs_depth_flow_validate(&fb) == 0, "flow with valid");
  expect(refused(gs_depth_flow_validate(NULL), "null argument block"), "flow null block");
  fb = fl; fb.W = 0; expect(refused(gs_depth_flow_validate(&fb), "must be > 0"), "flow W = 0");
  fb = fl; fb.H = 1 << 16; expect(refused(gs_depth_flow_validate(&fb), "too large"), "flow H too large");
  fb = fl; fb.depth1 = NULL; expect(refused(gs_depth_flow_validate(&fb), "depth1 is required"), "flow null depth1");
  fb = fl; fb.Kinv1 = NULL;  expect(refused(gs_depth_flow_validate(&fb), "required"), "flow null Kinv1");
  fb = fl; fb.T = NULL;      expect(refused(gs_depth_flow_validate(&fb), "required"), "flow null T");
  fb = fl; fb.K2 = NULL;     expect(refused(gs_depth_flow_validate(&fb), "required"), "flow null K2");
  fb = fl; fb.flow = NULL;   expect(refused(gs_depth_flow_validate(&fb), "flow is required"), "flow null flow");
  fb = fl; fb.T = (const float *)((const char *)m4 + 2);
  expect(refused(gs_depth_flow_validate(&fb), "4-byte aligned"), "flow misaligned T");

  /* gs_sample_bilinear */
  struct gs_sample_bilinear sa;
  memset(&sa, 0, sizeof(sa));
  sa.B = B; sa.Ch = Ch; sa.H = H; sa.W = W;
  sa.mode = GS_SAMPLE_POINTS; sa.N = N;
  sa.src = big; sa.coords = xy; sa.out = outp;
  expect(gs_sample_bilinear_validate(&sa) == 0, "point sampling");
  struct gs_sample_bilinear sd = sa;
  sd.Ch = 2; sd.mode = GS_SAMPLE_DISPLACEMENT; sd.h = 5; sd.w = 7; sd.N = 35; sd.coords = map; sd.out = map2;
  expect(gs_sample_bilinear_validate(&sd) == 0, "displacement sampling");
  sd.add_displacement = 1;
  expect(gs_sample_bilinear_validate(&sd) == 0, "displacement sampling, accumulated");
  struct gs_sample_bilinear sb = sd;
  sb.Ch = 3; expect(refused(gs_sample_bilinear_validate(&sb), "add_displacement"), "accumulate with Ch != 2");
  sb = sa; sb.add_displacement = 1;
  expect(refused(gs_sample_bilinear_validate(&sb), "add_displacement"), "accumulate in point mode");
  sb = sd; sb.N = 36; expect(refused(gs_sample_bilinear_validate(&sb), "h*w"), "displacement N != h*w");
  sb = sd; sb.h = 0;  expect(refused(gs_sample_bilinear_validate(&sb), "h, w must be"), "displacement h = 0");
  expect(refused(gs_sample_bilinear_validate(NULL), "null argument block"), "sampler null block");
  sb = sa; sb.Ch = 0;  expect(refused(gs_sample_bilinear_validate(&sb), "Ch must be > 0"), "sampler Ch = 0");
  sb = sa; sb.B = 0;   expect(refused(gs_sample_bilinear_validate(&sb), "must be > 0"), "sampler B = 0");
  sb = sa; sb.H = -2;  expect(refused(gs_sample_bilinear_validate(&sb), "must be > 0"), "sampler H < 0");
  sb = sa; sb.mode = 2; expect(refused(gs_sample_bilinear_validate(&sb), "mode must be"), "sampler bad mode");
  sb = sa; sb.N = 0;   expect(refused(gs_sample_bilinear_validate(&sb), "N must be"), "sampler N = 0");
  sb = sa; sb.src = NULL;    expect(refused(gs_sample_bilinear_validate(&sb), "src is required"), "sampler null src");
  sb = sa; sb.coords = NULL; expect(refused(gs_sample_bilinear_validate(&sb), "coords are required"), "sampler null coords");
  sb = sa; sb.out = NULL;    expect(refused(gs_sample_bilinear_validate(&sb), "out is required"), "sampler null out");
  sb = sa; sb.out = (float *)((char *)outp + 3);
  expect(refused(gs_sample_bilinear_validate(&sb), "4-byte aligned"), "sampler misaligned out");

  free(points); free(m4); free(m3); free(map); free(map2); free(mask); free(big); free(xy); free(outp); free(sums);
  free(valid); free(ws);
  if (failures) return 1;
  printf("depth geometry host sanitize ok\n");
  return 0;
}
