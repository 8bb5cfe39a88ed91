/* gs_densify.h -- C ABI of densification (clone, split, prune and the Adam
 * state that moves with every row), exported by the same libgsplat_hip.so as
 * gsplat_hip.h.
 *
 * Replaces the reference's densify() (external.py:244-292) -- three rounds of
 * boolean-mask indexing and torch.cat over every parameter and both Adam
 * moments -- by one classification, one prefix scan and one gather:
 *
 *   gs_densify_plan    classifies every Gaussian, ranks it in the four sets
 *                      below and leaves the four totals in device memory
 *   (the caller reads the totals back: the pass's only synchronisation, and
 *    allocates the outputs)
 *   gs_densify_apply   ONE launch that writes every output tensor, both
 *                      moments of each, and zero-fills the new statistics
 *
 * Classification of Gaussian i, in the reference's order of tests:
 *   g     = grad_accum[i] / denom[i], NaN -> 0 (Inf stays)
 *   s     = max_k exp(log_scales[i, k])
 *   clone = g >= grad_thresh && s <= clone_max_scale
 *   split = g >= grad_thresh && s >  clone_max_scale
 *   prune(s') = 1 / (1 + exp(-logit_opacities[i])) < prune_min_opacity
 *               || (prune_max_scale > 0 && s' > prune_max_scale)
 *   an original and its clone are pruned by prune(s), the copies of a split
 *   by prune(s / (0.8 n_split)).
 *
 * Output rows, each block in source-index order (the reference's order):
 *   [ kept originals | kept clones | kept split copy 0 | kept split copy 1 ]
 * Originals keep parameter and moments bit for bit; clones copy the parameter
 * with zero moments; copy j of the split source with all-split rank r uses
 * noise row j * n_split_all + r:
 *   mean       += R(q / |q|) (exp(log_scales) * z)      (external.py:61-78)
 *   log_scales  = log(exp(log_scales) / (0.8 n_split))
 * everything else copied, moments zero.
 *
 * Everything is fp32 device memory, 4-byte aligned; rows need no wider
 * alignment.  Both calls are asynchronous on `stream`, never synchronise and
 * use no atomics: the same inputs give the same bits.  They return 0 or an
 * error code with gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_DENSIFY_H
#define GS_DENSIFY_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_DENSIFY_MAX_TENSORS 16
#define GS_DENSIFY_N_SPLIT 2   /* the only supported n_split (external.py:262) */

/* flag byte of a Gaussian (gs_densify_plan's first output) */
#define GS_DENSIFY_CLONE 1u
#define GS_DENSIFY_SPLIT 2u
#define GS_DENSIFY_PRUNE 4u        /* prune(s): the original and its clone */
#define GS_DENSIFY_PRUNE_SPLIT 8u  /* prune(s / (0.8 n_split)): the split copies */

/* the sets a Gaussian is ranked in; also the order of the four totals */
#define GS_DENSIFY_KEPT_ORIGINALS 0  /* !split && !prune */
#define GS_DENSIFY_KEPT_CLONES 1     /* clone && !prune */
#define GS_DENSIFY_ALL_SPLITS 2      /* split */
#define GS_DENSIFY_KEPT_SPLITS 3     /* split && !prune_split */

/* roles of a per-Gaussian tensor in gs_densify_apply */
#define GS_DENSIFY_ROLE_PLAIN 0
#define GS_DENSIFY_ROLE_MEANS 1            /* width 3 */
#define GS_DENSIFY_ROLE_LOG_SCALES 2       /* width 3 */
#define GS_DENSIFY_ROLE_ROTATIONS 3        /* width 4, (r, x, y, z), not normalised */
#define GS_DENSIFY_ROLE_LOGIT_OPACITIES 4  /* width 1 */

typedef struct gs_densify_plan_args {
  int64_t P;                    /* Gaussians (>= 0) */
  const float *grad_accum;      /* [P] */
  const float *denom;           /* [P] */
  const float *log_scales;      /* [P, 3] */
  const float *logit_opacities; /* [P] */
  float grad_thresh;            /* 0.0002 */
  float clone_max_scale;        /* 0.01 scene_radius */
  float prune_min_opacity;      /* 0.005, 0.25 at i = 5000 */
  float prune_max_scale;        /* 0.1 scene_radius; <= 0 disables the test */
  int32_t n_split;              /* GS_DENSIFY_N_SPLIT */
  int32_t _pad;
  void *workspace;              /* gs_densify_workspace_bytes(P) bytes, 16-byte aligned */
  uint64_t workspace_bytes;     /* size of the buffer behind `workspace` */
} gs_densify_plan_args;

typedef struct gs_densify_tensor {
  const float *src;             /* [P, width] */
  const float *src_exp_avg;     /* [P, width] or NULL: read as zero */
  const float *src_exp_avg_sq;
  float *dst;                   /* [P_new, width] */
  float *dst_exp_avg;           /* [P_new, width] or NULL: not written */
  float *dst_exp_avg_sq;
  int32_t width;                /* floats per Gaussian (> 0) */
  int32_t role;                 /* GS_DENSIFY_ROLE_* */
} gs_densify_tensor;

typedef struct gs_densify_apply_args {
  int64_t P;                    /* as planned */
  int64_t counts[4];            /* the plan's totals, as read back */
  const void *workspace;        /* the plan's workspace, unchanged since */
  uint64_t workspace_bytes;
  int32_t n_split;              /* GS_DENSIFY_N_SPLIT */
  int32_t n_tensors;            /* <= GS_DENSIFY_MAX_TENSORS; each non-plain role exactly once */
  const float *noise;           /* [n_split * counts[ALL_SPLITS], 3]; NULL only without splits */
  float *stats[3];              /* [P_new] each or NULL: zero-filled */
  int32_t reset_opacity;        /* != 0: every output logit opacity = opacity_reset, moments 0 */
  float opacity_reset;          /* log(0.01 / 0.99) (external.py:288-290) */
  gs_densify_tensor t[GS_DENSIFY_MAX_TENSORS];
} gs_densify_apply_args;

/* sizeof of each struct as the library was compiled (for binding mirrors). */
size_t gs_densify_plan_struct_bytes(void);
size_t gs_densify_tensor_struct_bytes(void);
size_t gs_densify_apply_struct_bytes(void);

/* Workspace of one plan + apply pair: the four totals, the flag bytes, four
 * ranks per Gaussian and four sums per scan workgroup.  0 for P <= 0. */
size_t gs_densify_workspace_bytes(int64_t P);
/* Byte offsets into the workspace: the four int64 totals, the flag bytes [P]
 * and the ranks [P, 4] int32 (in the order of the sets above). */
size_t gs_densify_counts_offset(int64_t P);
size_t gs_densify_flags_offset(int64_t P);
size_t gs_densify_ranks_offset(int64_t P);
/* Gaussians one scan workgroup covers, and block sums one pass of the
 * block-sum scan covers (for tests of the boundaries). */
int64_t gs_densify_scan_block(void);
int64_t gs_densify_scan_tile(void);
/* P_new = kept originals + kept clones + n_split * kept splits. */
int64_t gs_densify_new_count(const int64_t counts[4], int32_t n_split);

/* The argument checks the two entry points run first (host code, no device
 * access). */
int gs_densify_plan_validate(const gs_densify_plan_args *args);
int gs_densify_apply_validate(const gs_densify_apply_args *args);

/* Flags, ranks and totals into the workspace.  P = 0 makes no launch. */
int gs_densify_plan(const gs_densify_plan_args *args, gs_stream_t stream);

/* Every output tensor, its moments and the statistics in one launch.
 * P = 0 or P_new = 0 makes no launch. */
int gs_densify_apply(const gs_densify_apply_args *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_DENSIFY_H */
