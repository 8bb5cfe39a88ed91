/* gs_resample.h -- C ABI of the bilinear resample, exported by the same
 * libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the F.interpolate(..., mode='bilinear') call the reference puts
 * between a render and a prior that is not at render resolution
 * (revise_train.py:100-104 and sanity_feature.py:428,442,487 for the feature
 * maps, align_corners=True; dyn_double.py:303 and dyn_base.py:136 for the
 * depth, align_corners=False), forward and backward, for B * Ch independent
 * planes at once: x [B, Ch, H, W] -> y [B, Ch, h, w], contiguous fp32.
 *
 * Per axis with input size I, output size O and output index o, in fp32:
 *
 *   align_corners != 0:  scale = O > 1 ? (float)(I - 1) / (float)(O - 1) : 0
 *                        src   = scale * o
 *   align_corners == 0:  scale = (float)I / (float)O
 *                        src   = max(0, fmaf(scale, o + 0.5f, -0.5f))
 *   i0 = min((int)src, I - 1)   i1 = min(i0 + 1, I - 1)
 *   l1 = src - (float)i0        l0 = 1 - l1
 *
 *   y[oy, ox] = l0y * (l0x * x[i0y, i0x] + l1x * x[i0y, i1x])
 *             + l1y * (l0x * x[i1y, i0x] + l1x * x[i1y, i1x])
 *
 * The fmaf is part of the contract: it is what torch's CPU kernel computes.
 * Equal sizes give a bit-exact copy in both modes, forward and backward.
 *
 * The backward is the exact adjoint with the same taps and weights, in gather
 * form: every element of d_x is written exactly once (zeros where no output
 * taps it, never accumulated, no memset needed), there are no atomics, and the
 * terms of an element are summed in ascending (oy, ox) order, so two calls on
 * the same inputs give the same bits.  It needs the workspace
 * (gs_resample_workspace_bytes): two small tables of first output indices per
 * input row and column.  The forward uses no workspace.
 *
 * 1 <= H, W, h, w <= 32768; B, Ch >= 1.  All calls are asynchronous on
 * `stream`, read nothing back, never allocate and never synchronise; return 0
 * or an error code with gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_RESAMPLE_H
#define GS_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_resample {
  int32_t B, Ch;             /* planes: B * Ch, each resampled on its own (both > 0) */
  int32_t H, W;              /* input rows, columns */
  int32_t h, w;              /* output rows, columns */
  int32_t align_corners;     /* 0: half-pixel centres; else the corner pixels map onto each other */
  const float *x;            /* [B, Ch, H, W], read by the forward only */
  float *y;                  /* [B, Ch, h, w], written by the forward only */
  void *workspace;           /* gs_resample_workspace_bytes(H, W) bytes (backward only) */
  uint64_t workspace_bytes;  /* size of the buffer behind `workspace` */
} gs_resample;

/* sizeof(gs_resample) as the library was compiled (for binding mirrors). */
size_t gs_resample_struct_bytes(void);

/* Workspace of one backward: first_y [H + 1] and first_x [W + 1] as int32,
 * each padded to 16 bytes.  0 for sizes out of range. */
size_t gs_resample_workspace_bytes(int32_t H, int32_t W);

/* The argument check both entry points run first (host code, no device
 * access).  backward = 0 needs x and y and ignores the workspace and the two
 * gradient pointers; backward != 0 needs the workspace and the two gradient
 * pointers and ignores x and y. */
int gs_resample_validate(const gs_resample *args, int backward, const float *d_y, const float *d_x);

/* The axis function above as host code (no device access), for one axis:
 * i0 [O] and l1 [O] of every output index, and first [I + 1] with first[i] the
 * smallest o whose i0 is >= i (O where there is none), so that the outputs
 * whose lower tap is i are [first[i], first[i + 1]).  Any of the three
 * pointers may be NULL. */
int gs_resample_axis(int32_t I, int32_t O, int32_t align_corners, int32_t *i0, float *l1, int32_t *first);

/* y from x. */
int gs_resample_forward(const gs_resample *args, gs_stream_t stream);

/* d_x [B, Ch, H, W] (every element written, never accumulated) from the
 * upstream gradient d_y [B, Ch, h, w]. */
int gs_resample_backward(const gs_resample *args, const float *d_y, float *d_x, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_RESAMPLE_H */
