/* scene_loss_host_sanitize.c -- stand-alone driver of the scene regularisers'
 * host validator (dynamic3dgaussians_amd/csrc/gs_scene_loss_host.cpp) for a
 * CPU sanitizer build (tests/test_scene_loss.py compiles this file,
 * gs_host.cpp and gs_scene_loss_host.cpp with -fsanitize=address,undefined
 * and runs the program).  It walks valid and invalid argument blocks; the
 * validator must accept / refuse each one with a message and touch nothing it
 * was not given.  The pointers name heap buffers of the right size, none of
 * which the validator may dereference.  Exit status 0 and "scene loss host
 * sanitize ok" on success. */
#include <stdlib.h>

#include "gs_scene_loss.h"
#include "host_sanitize.h"

static int sl_refused(const gs_scene_loss *a, int backward, const float *up, const float *dm, const float *dr,
                      const float *dc, const char *needle) {
  return refused(gs_scene_loss_validate(a, backward, up, dm, dr, dc), needle);
}

int main(void) {
  const int64_t P = 1000, n_fg = 439, n_bg = P - n_fg;
  const size_t ws_bytes = gs_scene_loss_workspace_bytes(P);
  expect(ws_bytes == 4 * 4 * sizeof(float), "four records of four floats for 1000 rows");
  expect(gs_scene_loss_workspace_bytes(0) == 0 && gs_scene_loss_workspace_bytes(-5) == 0,
         "workspace of an empty table is 0");
  expect(gs_scene_loss_workspace_bytes(1) == 4 * sizeof(float), "one record for one row");
  expect(gs_scene_loss_workspace_bytes(2048 * 256) == 2048 * 4 * sizeof(float), "the last uncapped count");
  expect(gs_scene_loss_workspace_bytes((int64_t)1 << 30) == 2048 * 4 * sizeof(float), "capped workgroup count");
  expect(gs_scene_loss_struct_bytes() == sizeof(gs_scene_loss), "struct size");

  int32_t *slot = malloc(P * sizeof(int32_t));
  float *means = malloc(P * 3 * sizeof(float)), *rot = malloc(P * 4 * sizeof(float));
  float *col = malloc(P * 3 * sizeof(float)), *prev_col = malloc(P * 3 * sizeof(float));
  float *bg_pts = malloc(n_bg * 3 * sizeof(float)), *bg_rot = malloc(n_bg * 4 * sizeof(float));
  float *d_means = malloc(P * 3 * sizeof(float)), *d_rot = malloc(P * 4 * sizeof(float));
  float *d_col = malloc(P * 3 * sizeof(float));
  float *losses = malloc(3 * sizeof(float)), *up = malloc(3 * sizeof(float));
  void *ws = aligned_alloc(256, (ws_bytes + 255) / 256 * 256);
  if (!slot || !means || !rot || !col || !prev_col || !bg_pts || !bg_rot || !d_means || !d_rot || !d_col || !losses ||
      !up || !ws)
    return 2;

  gs_scene_loss good;
  memset(&good, 0, sizeof(good));
  good.P = P; good.n_fg = n_fg; good.n_bg = n_bg;
  good.slot = slot; good.means = means; good.rotations = rot; good.colors = col;
  good.init_bg_pts = bg_pts; good.init_bg_rot = bg_rot; good.prev_col = prev_col;
  good.losses = losses; good.workspace = ws; good.workspace_bytes = ws_bytes;

  /* valid blocks */
  expect(gs_scene_loss_validate(&good, 0, NULL, NULL, NULL, NULL) == 0, "forward block");
  expect(gs_scene_loss_validate(&good, 1, up, d_means, d_rot, d_col) == 0, "backward block");
  gs_scene_loss v = good;
  v.raw_rotations = 1;
  v.rotations = rot + 1; /* 4 bytes past a 16-byte boundary: the scalar path, not an error */
  expect(gs_scene_loss_validate(&v, 0, NULL, NULL, NULL, NULL) == 0, "raw rotations at a 4-byte offset");
  v = good; v.losses = NULL; v.workspace = NULL; v.workspace_bytes = 0; /* the backward needs neither */
  expect(gs_scene_loss_validate(&v, 1, up, d_means, d_rot, d_col) == 0, "backward without workspace");
  v = good; v.n_fg = P; v.n_bg = 0; v.init_bg_pts = NULL; v.init_bg_rot = NULL;
  expect(gs_scene_loss_validate(&v, 0, NULL, NULL, NULL, NULL) == 0, "no background, no anchors");
  v = good; v.n_fg = 0; v.n_bg = P;
  expect(gs_scene_loss_validate(&v, 0, NULL, NULL, NULL, NULL) == 0, "no foreground");

  /* invalid blocks, one fault each */
  gs_scene_loss bad;
  expect(sl_refused(NULL, 0, NULL, NULL, NULL, NULL, "null argument block"), "null block");
  bad = good; bad.P = 0;   expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "P must be in"), "P = 0");
  bad = good; bad.P = -7;  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "P must be in"), "P < 0");
  bad = good; bad.P = (int64_t)1 << 31;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "P must be in"), "P past int32");
  bad = good; bad.n_fg = -1; bad.n_bg = P + 1;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "n_fg and n_bg must be >= 0"), "n_fg < 0");
  bad = good; bad.n_bg = -1; bad.n_fg = P + 1;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "n_fg and n_bg must be >= 0"), "n_bg < 0");
  bad = good; bad.n_fg = n_fg + 1;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "n_fg + n_bg must equal P"), "one row too many");
  bad = good; bad.n_bg = n_bg - 1;
  expect(sl_refused(&bad, 1, up, d_means, d_rot, d_col, "n_fg + n_bg must equal P"), "one row short, backward");
  bad = good; bad.slot = NULL;      expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "slot is required"), "null slot");
  bad = good; bad.means = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "means, rotations and colors are required"), "null means");
  bad = good; bad.rotations = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "means, rotations and colors are required"), "null rotations");
  bad = good; bad.colors = NULL;
  expect(sl_refused(&bad, 1, up, d_means, d_rot, d_col, "means, rotations and colors are required"), "null colors");
  bad = good; bad.prev_col = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "prev_col is required"), "null prev_col");
  bad = good; bad.init_bg_pts = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "init_bg_pts and init_bg_rot are required"), "null init_bg_pts");
  bad = good; bad.init_bg_rot = NULL;
  expect(sl_refused(&bad, 1, up, d_means, d_rot, d_col, "init_bg_pts and init_bg_rot are required"),
         "null init_bg_rot");
  bad = good; bad.means = (const float *)((const char *)means + 2);
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "every table must be 4-byte aligned"), "misaligned means");
  bad = good; bad.slot = (const int32_t *)((const char *)slot + 1);
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "every table must be 4-byte aligned"), "misaligned slot");
  bad = good; bad.losses = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "losses is required"), "null losses");
  bad = good; bad.losses = (float *)((char *)losses + 3);
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "losses must be 4-byte aligned"), "misaligned losses");
  bad = good; bad.workspace = NULL;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_bytes - 1;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "needed"), "short workspace");
  bad = good; bad.workspace = (char *)ws + 4;
  expect(sl_refused(&bad, 0, NULL, NULL, NULL, NULL, "16-byte aligned"), "misaligned workspace");
  expect(sl_refused(&good, 1, NULL, d_means, d_rot, d_col, "dL_dlosses is required"), "backward without dL_dlosses");
  expect(sl_refused(&good, 1, up, NULL, d_rot, d_col, "are required"), "backward without dL_dmeans");
  expect(sl_refused(&good, 1, up, d_means, NULL, d_col, "are required"), "backward without dL_drotations");
  expect(sl_refused(&good, 1, up, d_means, d_rot, NULL, "are required"), "backward without dL_dcolors");
  expect(sl_refused(&good, 1, up, d_means, (const float *)((const char *)d_rot + 2), d_col, "4-byte aligned"),
         "misaligned dL_drotations");

  free(slot); free(means); free(rot); free(col); free(prev_col); free(bg_pts); free(bg_rot);
  free(d_means); free(d_rot); free(d_col); free(losses); free(up); free(ws);
  if (failures) return 1;
  printf("scene loss host sanitize ok\n");
  return 0;
}
