// gs_spectral_layout.h -- sizes, the block-width and slab rules and the
// workspace layout of the spectral embedding (include/gs_spectral.h), written
// once for the kernels (gs_spectral.hip) and the host-only validator
// (gs_spectral_host.cpp).  Plain C++ on the host, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/gs_spectral.h"

namespace gs {

constexpr int SP_THREADS = 256;
constexpr int SP_EIG_THREADS = 512;     // the small problems' one workgroup
constexpr int SP_MAX_B = GS_SPECTRAL_MAX_B;
constexpr int SP_CHUNK = 32;            // rows staged in LDS by the Gram and rotate kernels
constexpr int SP_MIN_SLAB = 256;        // rows of a slab at least
constexpr int SP_MAX_SLABS = 1024;      // slabs at most: the partial sums stay under 1024 B^2 doubles
// control words (int32) at off_ctrl
enum { SP_CTRL_DONE = 0, SP_CTRL_FINAL = 1, SP_CTRL_BAD = 2, SP_CTRL_WORDS = 64 };

static_assert(SP_MAX_B == 8 * ((GS_SPECTRAL_MAX_K + GS_SPECTRAL_GUARD + 7) / 8), "the widest block");

inline bool sp_sizes_ok(int64_t n, int64_t nnz, int64_t K) {
  return K >= 1 && K <= GS_SPECTRAL_MAX_K && n >= K && n <= GS_SPECTRAL_MAX_N && nnz >= 0 && nnz < ((int64_t)1 << 31);
}
inline int sp_block_width(int64_t n, int K) {
  const int64_t b = 8 * ((K + GS_SPECTRAL_GUARD + 7) / 8);
  return (int)(n < b ? n : b);
}
// Rows of a slab: a function of n alone, a multiple of SP_CHUNK.
inline int64_t sp_slab_rows(int64_t n) {
  int64_t r = (n + SP_MAX_SLABS - 1) / SP_MAX_SLABS;
  r = (r + SP_CHUNK - 1) / SP_CHUNK * SP_CHUNK;
  return r < SP_MIN_SLAB ? SP_MIN_SLAB : r;
}
inline int64_t sp_slabs(int64_t n) { return (n + sp_slab_rows(n) - 1) / sp_slab_rows(n); }
inline size_t sp_pad256(size_t v) { return (v + 255) / 256 * 256; }

// The workspace: degrees and their inverse roots, four [n, B] blocks, the
// slabs' partial sums, the small problems' matrices and the control words.
struct SpectralLayout {
  size_t off_d, off_g, off_blk[4], off_part, off_rpart, off_gram, off_rot, off_evec, off_theta, off_repl, off_ctrl,
      total;  // bytes
  int B;
  int64_t slab_rows, slabs;
  SpectralLayout(int64_t n, int K) {
    B = sp_block_width(n, K);
    slab_rows = sp_slab_rows(n);
    slabs = sp_slabs(n);
    const size_t bb = (size_t)B * B * sizeof(double);
    size_t o = 0;
    off_d = o;
    o += sp_pad256((size_t)n * sizeof(double));
    off_g = o;
    o += sp_pad256((size_t)n * sizeof(double));
    for (int i = 0; i < 4; ++i) {
      off_blk[i] = o;
      o += sp_pad256((size_t)n * B * sizeof(double));
    }
    off_part = o;
    o += sp_pad256((size_t)slabs * bb);
    off_rpart = o;
    o += sp_pad256((size_t)slabs * B * sizeof(double));
    off_gram = o;
    o += sp_pad256(bb);
    off_rot = o;
    o += sp_pad256(bb);
    off_evec = o;
    o += sp_pad256(bb);
    off_theta = o;
    o += sp_pad256((size_t)B * sizeof(double));
    off_repl = o;
    o += sp_pad256((size_t)B * sizeof(int32_t));
    off_ctrl = o;
    o += sp_pad256(SP_CTRL_WORDS * sizeof(int32_t));
    total = o;
  }
};

}  // namespace gs
