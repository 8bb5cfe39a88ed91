/* gs_scene_loss.h -- C ABI of the scene regularisers and the foreground split
 * of the reference's per-step loss, exported by the same libgsplat_hip.so as
 * gsplat_hip.h.
 *
 * Replaces the PyTorch remainder of the reference's `if not
 * is_initial_timestep:` block (train.py:253-282): the four boolean-index
 * gathers `x[is_fg]` / `x[~is_fg]` (each a nonzero whose count the host waits
 * for) and the floor / bg / soft_col_cons terms, over the P rows of the
 * Gaussian tables:
 *
 *   floor         = mean over fg of max(y, 0)                      (y = means[i, 1])
 *   bg            = mean over bg of sum_3 |means[i] - init_bg_pts[r]|
 *                 + mean over bg of sum_4 |rot[i]   - init_bg_rot[r]|
 *   soft_col_cons = mean over all P of sum_3 |colors[i] - prev_col[i]|
 *
 * The split is the int32 table `slot` [P], built once per sequence: slot[i] =
 * r >= 0 for the r-th foreground row, -1 - r for the r-th background row, the
 * ranks in row order.  Slot r therefore addresses row r of what the reference
 * made with `x[is_fg]` / `x[~is_fg]` (init_bg_pts, init_bg_rot, the neighbour
 * graph).  n_fg + n_bg = P.  An empty set gives NaN like torch's empty mean.
 *
 * raw_rotations != 0: `rotations` holds unnormalised quaternions and the
 * kernels apply F.normalize (q / max(|q|, 1e-12)) themselves, forward and
 * backward, in the operation order of the preprocess kernels' GS_FLAG_ACTIVATE
 * path.
 *
 * The backward follows torch's autograd at the kinks: |x| has gradient
 * sign(x), 0 at 0; max(y, 0) passes the gradient where y >= 0, y == 0
 * included; a mean over N rows hands every row g * (1 / N), the reciprocal
 * rounded to fp32 first (how torch's device kernel divides by a host
 * scalar).  Every element of the three gradient tables is written exactly
 * once.  No atomics anywhere: two calls on the same inputs give the same
 * bits.
 *
 * Everything is contiguous fp32 device memory (slot: int32), 4-byte aligned;
 * rows are loaded 16 bytes at a time where the base pointers allow it.  All
 * calls are asynchronous on `stream`, read nothing back and never
 * synchronise; return 0 or an error code with gs_last_error() set (as
 * gsplat_hip.h). */
#ifndef GS_SCENE_LOSS_H
#define GS_SCENE_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_scene_loss {
  int64_t P;                 /* rows of the tables (> 0) */
  int64_t n_fg, n_bg;        /* foreground / background rows, n_fg + n_bg = P */
  const int32_t *slot;       /* [P] the split */
  const float *means;        /* [P, 3] */
  const float *rotations;    /* [P, 4] normalised, or raw with raw_rotations */
  const float *colors;       /* [P, 3] */
  const float *init_bg_pts;  /* [n_bg, 3] (may be NULL when n_bg = 0) */
  const float *init_bg_rot;  /* [n_bg, 4] (may be NULL when n_bg = 0) */
  const float *prev_col;     /* [P, 3] */
  int32_t raw_rotations;     /* 0: rotations are unit quaternions; else normalise them here */
  int32_t _pad;
  float *losses;             /* [3] floor, bg, soft_col_cons; written by the forward */
  void *workspace;           /* gs_scene_loss_workspace_bytes(P) bytes (forward only) */
  uint64_t workspace_bytes;  /* size of the buffer behind `workspace` */
} gs_scene_loss;

/* sizeof(gs_scene_loss) as the library was compiled (for binding mirrors). */
size_t gs_scene_loss_struct_bytes(void);

/* Workspace of one forward: four fp32 partial sums {floor, bg means, bg
 * rotations, colour} per workgroup of the forward's grid.  0 for P <= 0. */
size_t gs_scene_loss_workspace_bytes(int64_t P);

/* The argument check both entry points run first (host code, no device
 * access).  backward = 0 ignores the four gradient pointers; backward != 0
 * ignores losses and the workspace. */
int gs_scene_loss_validate(const gs_scene_loss *args, int backward, const float *dL_dlosses,
                           const float *dL_dmeans, const float *dL_drotations, const float *dL_dcolors);

/* losses[0:3] = floor, bg, soft_col_cons. */
int gs_scene_loss_forward(const gs_scene_loss *args, gs_stream_t stream);

/* dL_dmeans [P, 3], dL_drotations [P, 4], dL_dcolors [P, 3] (every element
 * written, never accumulated) for the upstream gradients dL_dlosses [3]
 * (device memory). */
int gs_scene_loss_backward(const gs_scene_loss *args, const float *dL_dlosses, float *dL_dmeans,
                           float *dL_drotations, float *dL_dcolors, gs_stream_t stream);

/* fg_pts [n_fg, 3], fg_rot [n_fg, 4]: the rows with slot >= 0, copied to their
 * slots (`means[is_fg]`, `rotations[is_fg]`). */
int gs_fg_gather_forward(int64_t P, int64_t n_fg, const int32_t *slot, const float *means,
                         const float *rotations, float *fg_pts, float *fg_rot, gs_stream_t stream);

/* dL_dmeans [P, 3], dL_drotations [P, 4] in full: a foreground row gets its
 * compact row of dL_dfg_pts / dL_dfg_rot, a background row zeros.  A NULL
 * compact table stands for "no gradient reached it" (zeros); a NULL output is
 * not written. */
int gs_fg_gather_backward(int64_t P, int64_t n_fg, const int32_t *slot, const float *dL_dfg_pts,
                          const float *dL_dfg_rot, float *dL_dmeans, float *dL_drotations,
                          gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_SCENE_LOSS_H */
