/* gs_feature_decoder.h -- C ABI of the fused 1x1 feature decoder and its L1
 * distillation loss, exported by the same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the reference's "speedup" route (revise_train.py:50-53, 102-103,
 * 126; utils/loss_utils.py:17-18)
 *
 *   feature_map = cnn_decoder(feature_map)          # a 1x1 convolution with bias
 *   Ll1_feature = l1_loss(feature_map, gt_feature_map)
 *
 * without ever creating the decoded [B, C_out, h, w] map.  Contiguous fp32:
 *
 *   x      [B, F_in, h, w]   planar
 *   weight [C_out, F_in]
 *   bias   [C_out]           optional (NULL: 0)
 *   target [B, C_out, h, w]
 *   mask   [h, w] or [B, h, w], optional float weights m >= 0 (NULL: 1)
 *
 * With p over the h * w pixels and N = C_out * h * w:
 *
 *   y[b,c,p]   = bias[c] + sum_f weight[c,f] * x[b,f,p]
 *   r          = y - target
 *   loss[b]    = sum_{c,p} m[p] * |r[b,c,p]| / N
 *   s[b,c,p]   = sign(r) in {-1, 0, +1}   (sign(0) = 0)
 *   d_x[b,f,p] = up[b]/N * m[p] * sum_c weight[c,f] * s[b,c,p]
 *   d_W[c,f]   = sum_b up[b]/N * sum_p s[b,c,p] * m[p] * x[b,f,p]
 *   d_b[c]     = sum_b up[b]/N * sum_p s[b,c,p] * m[p]
 *
 * and for the plain decode with an upstream gradient g = d_y:
 *
 *   d_x = W^T g      d_W = sum g x^T      d_b = sum g
 *
 * Every contraction runs on the matrix cores and is fp32-equivalent: both
 * operands are split into three bf16 pieces (each product carried to 2^-24
 * relative, six piece products; three where one operand, the sign tile, is
 * exact in bf16) and accumulated in fp32.  The epilogue rounds as written:
 * (acc + bias) - target, then m * |r|.  Loss sums and the final d_W / d_b sums
 * are taken in fp64 in a fixed order.  No float atomics, no read-back; nothing
 * is allocated or synchronised; two calls on the same inputs give the same
 * bits.  The loss backward recomputes r with the forward's function, so its
 * signs are the forward's by construction.
 *
 * Tile: GS_FD_TILE_ROWS output channels by GS_FD_TILE_PIXELS pixels per
 * workgroup step (one pixel per lane of each of its four waves, 32 pixels a
 * wave), k over F_in zero-padded to 32.
 * Grid rule: gridDim = (gx, B) with gx = min(tiles, max(1, G / B)), tiles =
 * ceil(h*w / GS_FD_TILE_PIXELS), G = GS_FD_GRID for the two backward passes
 * (gs_feature_decoder_grid_x; two workgroups per compute unit, each with one
 * slab) and GS_FD_GRID_FORWARD for the two forward passes; block (bx, b)
 * walks the tiles bx, bx + gx, ... of camera b in that order.
 * n_t (gs_feature_decoder_n_t): a thread adds n_t = 16 * ceil(C_out / 32)
 * terms m|r| in fp32 per tile before the sum goes to fp64.
 * n_acc (gs_feature_decoder_n_acc): the pixels one block walks,
 * ceil(tiles / gx) * GS_FD_TILE_PIXELS: the fp32 additions behind one element
 * of a block's slab [C_out, F_in] + [C_out].
 *
 * Limits: 1 <= F_in <= 64, 1 <= C_out <= 512, F_in * C_out <= 16384,
 * 1 <= B <= 65535, h, w >= 1, h * w < 2^31 - 128.  Plane offsets are 64-bit.
 * Byte and flop models per pixel (slabs and partials not counted):
 *   forward fused : 4 (F_in + C_out) + 4 (mask) bytes,  2 F_in C_out flops
 *   backward fused: 4 (F_in + C_out) + 4 read, 4 F_in written,  6 F_in C_out flops
 *
 * All calls are asynchronous on `stream`; return 0 or an error code with
 * gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_FEATURE_DECODER_H
#define GS_FEATURE_DECODER_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_FD_TILE_ROWS 32
#define GS_FD_TILE_PIXELS 128
#define GS_FD_GRID 512
#define GS_FD_GRID_FORWARD 1024
#define GS_FD_MAX_F_IN 64
#define GS_FD_MAX_C_OUT 512
#define GS_FD_MAX_WEIGHTS 16384

/* `pass` of gs_feature_decoder_workspace_bytes / gs_feature_decoder_validate. */
#define GS_FD_PASS_DECODE 0        /* gs_feature_decoder_forward */
#define GS_FD_PASS_LOSS 1          /* gs_feature_decoder_loss_forward */
#define GS_FD_PASS_LOSS_BACKWARD 2 /* gs_feature_decoder_loss_backward */
#define GS_FD_PASS_BACKWARD 3      /* gs_feature_decoder_backward */

typedef struct gs_feature_decoder {
  int32_t B, F_in, C_out;    /* cameras, rendered channels, decoded channels */
  int32_t h, w;              /* rows, columns of every map */
  int32_t mask_per_camera;   /* 0: mask is [h, w]; else [B, h, w] */
  const float *x;            /* [B, F_in, h, w] */
  const float *weight;       /* [C_out, F_in] */
  const float *bias;         /* [C_out] or NULL */
  const float *target;       /* [B, C_out, h, w] (loss passes) */
  const float *mask;         /* see mask_per_camera, or NULL (loss passes) */
  const float *up;           /* [B] upstream gradient of loss (loss backward) */
  const float *d_y;          /* [B, C_out, h, w] upstream gradient of y (backward) */
  float *y;                  /* [B, C_out, h, w] (decode) */
  float *loss;               /* [B] (loss forward) */
  float *d_x;                /* [B, F_in, h, w], every element written (backward passes) */
  float *d_weight;           /* [C_out, F_in] (backward passes) */
  float *d_bias;             /* [C_out] or NULL (backward passes) */
  void *workspace;           /* gs_feature_decoder_workspace_bytes bytes, 16-byte aligned */
  uint64_t workspace_bytes;  /* size of the buffer behind `workspace` */
} gs_feature_decoder;

/* sizeof(gs_feature_decoder) as the library was compiled (for binding mirrors). */
size_t gs_feature_decoder_struct_bytes(void);

/* Workspace of one pass: the weight's bf16 pieces in matrix-operand order, the
 * loss forward's fp64 partials [B, gx], the backward's slabs [B * gx][C_out *
 * F_in + C_out] (sized by the grid, never by the pixels).  0 for sizes out of
 * range. */
size_t gs_feature_decoder_workspace_bytes(int32_t B, int32_t F_in, int32_t C_out, int32_t h, int32_t w, int32_t pass);

/* gx of the backward's grid rule; n_t and n_acc as defined above.  0 for sizes out of range. */
int32_t gs_feature_decoder_grid_x(int32_t B, int32_t h, int32_t w);
int32_t gs_feature_decoder_n_t(int32_t C_out);
int64_t gs_feature_decoder_n_acc(int32_t B, int32_t h, int32_t w);

/* The argument check every entry point runs first (host code, no device access). */
int gs_feature_decoder_validate(const gs_feature_decoder *args, int32_t pass);

/* y. */
int gs_feature_decoder_forward(const gs_feature_decoder *args, gs_stream_t stream);
/* loss[B]. */
int gs_feature_decoder_loss_forward(const gs_feature_decoder *args, gs_stream_t stream);
/* d_x, d_weight, d_bias of sum_b up[b] * loss[b]; up is read on the device. */
int gs_feature_decoder_loss_backward(const gs_feature_decoder *args, gs_stream_t stream);
/* d_x, d_weight, d_bias of the plain decode from d_y. */
int gs_feature_decoder_backward(const gs_feature_decoder *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_FEATURE_DECODER_H */
