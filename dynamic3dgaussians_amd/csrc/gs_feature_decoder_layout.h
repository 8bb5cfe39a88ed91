// gs_feature_decoder_layout.h -- sizes, grid rule and workspace layout of the
// fused feature decoder (include/gs_feature_decoder.h), written once for the
// kernels (gs_feature_decoder.hip) and the host-only validator
// (gs_feature_decoder_host.cpp).  Plain C++ on the host, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/gs_feature_decoder.h"

namespace gs {

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = 4;
constexpr int FD_ROWS = GS_FD_TILE_ROWS;    // one 32x32 accumulator tile of rows
constexpr int FD_PIX = GS_FD_TILE_PIXELS;   // 32 pixels per wave
constexpr int FD_LD = FD_PIX + 4;           // LDS row stride in floats (16-byte aligned rows)
constexpr int FD_FRAG_BYTES = 3 * 64 * 16;  // one operand fragment: 3 pieces x 64 lanes x 8 bf16

inline bool fd_sizes_ok(int64_t B, int64_t F_in, int64_t C_out, int64_t h, int64_t w) {
  return B >= 1 && B <= 65535 && F_in >= 1 && F_in <= GS_FD_MAX_F_IN && C_out >= 1 && C_out <= GS_FD_MAX_C_OUT &&
         F_in * C_out <= GS_FD_MAX_WEIGHTS && h >= 1 && w >= 1 && h * w < 2147483647LL - FD_PIX;
}

inline int fd_row_tiles(int C_out) { return (C_out + FD_ROWS - 1) / FD_ROWS; }  // nct
inline int fd_f_tiles(int F_in) { return (F_in + 31) / 32; }                    // nft: k is padded to 32 * nft
inline int64_t fd_tiles(int64_t h, int64_t w) { return (h * w + FD_PIX - 1) / FD_PIX; }
inline bool fd_is_backward(int pass) { return pass == GS_FD_PASS_LOSS_BACKWARD || pass == GS_FD_PASS_BACKWARD; }
inline int64_t fd_grid_x(int64_t B, int64_t h, int64_t w, int pass) {
  int64_t g = (fd_is_backward(pass) ? GS_FD_GRID : GS_FD_GRID_FORWARD) / B;
  if (g < 1) g = 1;
  const int64_t t = fd_tiles(h, w);
  return g < t ? g : t;
}

// Workspace: the forward operand fragments of W ([nct][2 nft] fragments: rows
// of a row tile by one k-step of 16), the transposed fragments for W^T S
// ([nct][2][nft]: the 32 rows of f-tile ft by one k-step of 16 rows of S in
// the accumulator's permuted order), the loss partials, the slabs.
struct FeatureDecoderLayout {
  size_t off_wf, off_wt, off_partials, off_slabs, total;  // bytes
  size_t slab_floats;
  int64_t gx, slabs;
  FeatureDecoderLayout(int64_t B, int F_in, int C_out, int64_t h, int64_t w, int pass) {
    const size_t frags = (size_t)fd_row_tiles(C_out) * 2 * fd_f_tiles(F_in) * FD_FRAG_BYTES;
    gx = fd_grid_x(B, h, w, pass);
    slabs = gx * B;
    slab_floats = (size_t)C_out * F_in + C_out;
    const bool bwd = fd_is_backward(pass);
    size_t o = 0;
    off_wf = o;
    o += pass == GS_FD_PASS_BACKWARD ? 0 : frags;
    off_wt = o;
    o += bwd ? frags : 0;
    off_partials = o;
    o += pass == GS_FD_PASS_LOSS ? ((size_t)slabs * sizeof(double) + 15) / 16 * 16 : 0;
    off_slabs = o;
    o += bwd ? ((size_t)slabs * slab_floats * sizeof(float) + 15) / 16 * 16 : 0;
    total = o;
  }
};

}  // namespace gs
