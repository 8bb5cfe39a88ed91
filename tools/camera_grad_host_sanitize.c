/* camera_grad_host_sanitize.c -- stand-alone driver of the camera gradients'
 * host code (dynamic3dgaussians_amd/csrc/gs_camera_grad_host.cpp: the
 * workspace size and the argument validator gs_check_camera_grad) for a CPU
 * sanitizer build: compile this file, gs_host.cpp and gs_camera_grad_host.cpp
 * with -fsanitize=address,undefined and run the program, on the CPU, by hand
 * (DESIGN.md 9.13 gives the command; it is not run from pytest and never on a
 * GPU machine).  It walks valid and invalid argument sets; the validator must
 * accept / refuse each one with a message and touch none of the buffers: the
 * workspace is a heap block of exactly the reported size and the outputs are
 * heap blocks of C x 16 / C x 16 / C x 3 floats.  Exit status 0 and
 * "camera grad host sanitize ok" on success. */
#include <stdint.h>
#include <stdlib.h>

#include "gs_camera_grad.h"
#include "host_sanitize.h"

static void *block(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

/* the validator on freshly allocated buffers; short = bytes withheld from the workspace's declared size */
static int check(int64_t P, int32_t C, int compat, size_t shortfall) {
  const size_t need = gs_camera_grad_workspace_bytes(P, C);
  const int32_t c = C > 0 && C <= GS_CAMERA_GRAD_MAX_CAMS ? C : 1;
  void *ws = block(need);
  float *dv = block(sizeof(float) * 16 * (size_t)c), *dp = block(sizeof(float) * 16 * (size_t)c);
  float *dc = block(sizeof(float) * 3 * (size_t)c);
  const int r = gs_check_camera_grad(P, C, compat, ws, need - shortfall, dv, dp, dc);
  free(ws); free(dv); free(dp); free(dc);
  return r;
}

int main(void) {
  /* the workspace size: one 256-B record per (camera, 2048 Gaussians) */
  expect(gs_camera_grad_workspace_bytes(0, 3) == 0, "P = 0 needs no workspace");
  expect(gs_camera_grad_workspace_bytes(-5, 3) == 0, "P < 0 needs no workspace");
  expect(gs_camera_grad_workspace_bytes(1, 1) == 256, "one record");
  expect(gs_camera_grad_workspace_bytes(2048, 1) == 256, "a full chunk is one record");
  expect(gs_camera_grad_workspace_bytes(2049, 1) == 512, "a ragged second chunk");
  expect(gs_camera_grad_workspace_bytes(300000, 27) == (size_t)256 * 147 * 27, "the headline shape");
  expect(gs_camera_grad_workspace_bytes(100, 0) == 0 && gs_camera_grad_workspace_bytes(100, 65) == 0,
         "no size for an invalid camera count");
  expect(gs_camera_grad_workspace_bytes(2147483647, 64) == (size_t)256 * 1048576 * 64, "the largest call");

  /* valid argument sets */
  expect(check(800, 3, 1, 0) == 0, "P = 800, C = 3");
  expect(check(1, 1, 1, 0) == 0, "P = 1, C = 1");
  expect(check(300000, 64, 1, 0) == 0, "C = 64");
  float out[16 + 16 + 3];
  expect(gs_check_camera_grad(0, 2, 1, NULL, 0, out, out, out) == 0, "P = 0: no workspace needed, none checked");

  /* invalid ones, one fault each */
  expect(refused(check(800, 0, 1, 0), "camera batch size 0 outside 1..64"), "C = 0");
  expect(refused(check(800, 65, 1, 0), "camera batch size 65 outside 1..64"), "C = 65");
  expect(refused(check(800, -1, 1, 0), "outside 1..64"), "C < 0");
  expect(refused(check(-1, 1, 1, 0), "P must be"), "P < 0");
  expect(refused(check((int64_t)1 << 31, 1, 1, 0), "P must be"), "P = 2^31");
  expect(refused(check(800, 3, 0, 0), "compat 0 is refused"), "reference compat");
  expect(refused(check(800, 3, 2, 0), "compat 2 is refused"), "an unknown compat");
  expect(refused(check(800, 3, 1, 1), "workspace of 767 bytes, 768 needed"), "a workspace one byte short");
  void *ws = block(256);
  expect(refused(gs_check_camera_grad(800, 1, 1, NULL, 256, out, out, out), "workspace is required"),
         "a null workspace");
  expect(refused(gs_check_camera_grad(800, 1, 1, (char *)ws + 4, 256, out, out, out), "16-byte aligned"),
         "a misaligned workspace");
  expect(refused(gs_check_camera_grad(800, 1, 1, ws, 256, NULL, out, out), "are required"), "a null dL_dview");
  expect(refused(gs_check_camera_grad(800, 1, 1, ws, 256, out, NULL, out), "are required"), "a null dL_dproj");
  expect(refused(gs_check_camera_grad(800, 1, 1, ws, 256, out, out, NULL), "are required"), "a null dL_dcampos");
  expect(refused(gs_check_camera_grad(800, 1, 1, ws, 256, (float *)((char *)out + 1), out, out), "4-byte aligned"),
         "a misaligned output");
  expect(gs_check_camera_grad(800, 1, 1, ws, 256, out, out, out) == 0, "the same set, valid");
  free(ws);

  if (failures) return 1;
  printf("camera grad host sanitize ok\n");
  return 0;
}
