// gs_feature_knn_layout.h -- sizes, the chunk rule, the certificate's bound and
// the workspace layout of the cosine top-k search (include/gs_feature_knn.h),
// written once for the kernels (gs_feature_knn.hip) and the host-only
// validator (gs_feature_knn_host.cpp).  Plain C++ on the host, no HIP
// dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/gs_feature_knn.h"

namespace gs {

constexpr int FK_THREADS = 256;
constexpr int FK_WAVES = 4;
constexpr int FK_TILE = GS_FKNN_TILE;            // rows of one matrix tile (queries and database alike)
constexpr int FK_ROW_BLOCK = GS_FKNN_ROW_BLOCK;  // query rows of a scan workgroup: one tile per wave
constexpr int FK_SLACK = GS_FKNN_SLACK;
constexpr int FK_MAX_KP = GS_KNN_MAX_K + FK_SLACK;  // 48: what a (query, chunk) keeps at most
// A row's LDS candidate buffer.  One scan step appends at most FK_TILE entries to a row, and a
// row is merged down to kp <= FK_MAX_KP as soon as it holds more than FK_CAP - FK_TILE: a slot
// is always free.
constexpr int FK_CAP = 96;
constexpr int FK_TARGET_BLOCKS = 512;            // the chunk rule fills the chip twice over
constexpr int FK_MIN_CHUNK_TILES = 4;
constexpr int FK_RERANK_MAX = GS_FKNN_MAX_SPLITS * FK_MAX_KP;  // candidates of one query at most
constexpr int FK_FALLBACK_GRID = 1024;
constexpr int FK_FALLBACK_CAP = 1024;            // the fallback's LDS buffer (entries)

static_assert(FK_ROW_BLOCK == FK_WAVES * FK_TILE, "one query tile per wave");
static_assert(FK_CAP - FK_TILE >= FK_MAX_KP, "a merged row has room for one more step");
static_assert(FK_FALLBACK_CAP - FK_THREADS >= GS_KNN_MAX_K, "a merged fallback buffer has room for one more step");

inline bool fk_sizes_ok(int64_t M, int64_t N, int64_t E, int64_t k) {
  return M >= 1 && M <= GS_FKNN_MAX_ROWS && N >= 1 && N <= GS_FKNN_MAX_ROWS && E >= 1 && E <= GS_FKNN_MAX_E &&
         k >= 1 && k <= GS_KNN_MAX_K;
}
constexpr int fk_e_pad(int E) { return (E + 15) / 16 * 16; }
constexpr int fk_ksteps(int E) { return (E + 15) / 16; }
inline int64_t fk_tiles(int64_t rows) { return (rows + FK_TILE - 1) / FK_TILE; }
inline int64_t fk_row_blocks(int64_t M) { return (M + FK_ROW_BLOCK - 1) / FK_ROW_BLOCK; }
inline size_t fk_pad256(size_t n) { return (n + 255) / 256 * 256; }

// The database chunks of the scan: enough workgroups for the chip when the
// query blocks alone are too few, every chunk at least FK_MIN_CHUNK_TILES tiles.
inline int fk_splits(int64_t M, int64_t N) {
  const int64_t qb = fk_row_blocks(M);
  int64_t s = (FK_TARGET_BLOCKS + qb - 1) / qb;
  const int64_t most = fk_tiles(N) / FK_MIN_CHUNK_TILES;
  if (s > most) s = most;
  if (s > GS_FKNN_MAX_SPLITS) s = GS_FKNN_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}
// rows of a chunk: chunk c is [c L, min(N, (c + 1) L))
inline int64_t fk_chunk_rows(int64_t N, int S) { return (N + S - 1) / S; }

// |st - s| <= fk_bound(E).  n = 6 E_pad exact piece products
// are added into an fp32 accumulator in an order and a rounding mode the
// matrix core does not document: taken as no worse than truncation of every
// partial sum to 24 bits (2^-23 relative) in any order, (n - 1) 2^-23 sum|t|
// to first order, and doubled.  sum|t| <= (1 + 2^-8)^2 sum_c |xh_ic xh_jc|
// <= 1.01 (Cauchy-Schwarz on unit rows, fp32-rounded).  The piece products
// that are never formed and the pieces' own remainders are <= 2^-25 per unit
// of |xh_ic xh_jc|.
inline double fk_bound(int E) {
  const double n = 6.0 * fk_e_pad(E);
  return 1.01 * (2.0 * n * 1.1920928955078125e-07 + 2.98023223876953125e-08);
}

// The workspace: xh and its pieces for the database (and the queries), what
// the scan kept, the fallback list and its counters.
struct FeatureKnnLayout {
  size_t off_xh_d, off_pc_d, off_xh_q, off_pc_q, off_cand_s, off_cand_i, off_cnt, off_theta, off_list, off_counts,
      total;  // bytes
  int S, kp, e_pad, nks;
  int64_t dtiles, qtiles;
  FeatureKnnLayout(int64_t M, int64_t N, int E, int k, int splits, bool self) {
    S = splits > 0 ? splits : fk_splits(M, N);
    kp = k + FK_SLACK;
    e_pad = fk_e_pad(E);
    nks = fk_ksteps(E);
    dtiles = fk_tiles(N);
    qtiles = fk_tiles(M);
    const size_t row = (size_t)e_pad * sizeof(float);          // xh of one row
    const size_t pieces = (size_t)e_pad * 3 * sizeof(uint16_t);  // its three bf16 pieces
    size_t o = 0;
    off_xh_d = o;
    o += fk_pad256((size_t)dtiles * FK_TILE * row);
    off_pc_d = o;
    o += fk_pad256((size_t)dtiles * FK_TILE * pieces);
    off_xh_q = self ? off_xh_d : o;
    if (!self) o += fk_pad256((size_t)qtiles * FK_TILE * row);
    off_pc_q = self ? off_pc_d : o;
    if (!self) o += fk_pad256((size_t)qtiles * FK_TILE * pieces);
    off_cand_s = o;
    o += fk_pad256((size_t)M * S * kp * sizeof(float));
    off_cand_i = o;
    o += fk_pad256((size_t)M * S * kp * sizeof(int32_t));
    off_cnt = o;
    o += fk_pad256((size_t)M * S * sizeof(int32_t));
    off_theta = o;
    o += fk_pad256((size_t)M * S * sizeof(float));
    off_list = o;
    o += fk_pad256((size_t)M * sizeof(int32_t));
    off_counts = o;
    o += 256;  // certified, fallback (two 64-bit counters)
    total = o;
  }
};

}  // namespace gs
