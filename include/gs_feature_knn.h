/* gs_feature_knn.h -- C ABI of the exact cosine top-k search in feature space,
 * exported by the same libgsplat_hip.so as gsplat_hip.h.
 *
 * Replaces the reference's two dense N x N searches
 * (feature_rendering/feature_utils.py:7-16: F.normalize, tensor @ tensor.T,
 * topk(k + 1), first hit dropped; motion_utils.py:57-116 similarity_mapping:
 * feats @ feats.T handed to a clustering) without the N x N matrix.
 *
 *   feats    [N, E] fp32, the database
 *   queries  [M, E] fp32, or NULL: the database rows themselves (M = N), a
 *            row never its own neighbour (excluded by index)
 *
 * Definition (the device and a channel loop in numpy agree bit for bit):
 *
 *   norm_i = sqrt(sum_c (double)x_ic^2)           fp64, c ascending
 *   xh_ic  = fl32((double)x_ic / max(norm_i, 1e-12))
 *   s_ij   = sum_c (double)xh_ic (double)xh_jc    fp64, c ascending (every
 *            product is exact, so an FMA and a multiply-add give the same bits)
 *
 * Result per query: the k database rows of largest s, ordered by (s
 * descending, index ascending); sim [M, k] fp64, index [M, k] int64; where
 * fewer than k rows exist the tail is (-inf, -1).
 *
 * How.  prepare writes xh (fp32, E padded with zeros to a multiple of 16,
 * the rows to a multiple of GS_FKNN_TILE) and its three bf16 pieces in
 * matrix-operand order.  scan forms approximate similarities st on the matrix cores (six
 * piece products per k-step of 16, fp32 accumulation, gs_split_mfma.h) and
 * keeps, per (query, database chunk), the k + GS_FKNN_SLACK largest by
 * (st descending, index ascending) and the threshold theta = the last kept
 * one, so every row not kept has st <= theta.  rerank evaluates s exactly on
 * the kept rows; the k-th exact value c_k certifies the query when
 * c_k > max_chunks theta + gs_feature_knn_bound(E) (|st - s| <= that bound,
 * DESIGN.md 9.20), or when no chunk dropped anything.  Every other query is
 * put on a device-side list that a fixed grid walks: exact fp64 top-k over
 * the whole database.  Both paths return the unique answer of a total
 * order: reruns are bit-identical.  No float atomics, no read-back, no host
 * synchronisation.
 *
 * Limits: 1 <= E <= GS_FKNN_MAX_E, 1 <= k <= GS_KNN_MAX_K, 1 <= N, M <=
 * GS_FKNN_MAX_ROWS, 0 <= splits <= GS_FKNN_MAX_SPLITS (0: chosen by
 * gs_feature_knn_splits).  Features must be finite.
 *
 * All calls are asynchronous on `stream` and return 0 or an error code with
 * gs_last_error() set (as gsplat_hip.h). */
#ifndef GS_FEATURE_KNN_H
#define GS_FEATURE_KNN_H

#include <stddef.h>
#include <stdint.h>

#include "gs_knn.h"
#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_FKNN_MAX_E 128
#define GS_FKNN_MAX_ROWS (1 << 26)
#define GS_FKNN_MAX_SPLITS 32
#define GS_FKNN_SLACK 16      /* the scan keeps k + GS_FKNN_SLACK rows per (query, chunk) */
#define GS_FKNN_ROW_BLOCK 128 /* query rows of one scan workgroup */
#define GS_FKNN_TILE 32       /* database rows of one scan step */

typedef struct gs_feature_knn_args {
  int32_t N, M, E, k;
  int32_t splits;          /* 0: gs_feature_knn_splits(M, N, E, k) */
  int32_t _pad;
  const float *feats;      /* [N, E] */
  const float *queries;    /* [M, E], or NULL: feats, self excluded (M must equal N) */
  double *sim;             /* [M, k] */
  int64_t *index;          /* [M, k] */
  int64_t *stats;          /* [2] rows certified, rows sent to the fallback; or NULL */
  /* debug (all four or none): what the scan kept, before the rerank.  S = the splits in use,
   * kp = k + GS_FKNN_SLACK; entries past cand_count are (-inf, -1). */
  float *cand_sim;         /* [M, S, kp] */
  int32_t *cand_index;     /* [M, S, kp] */
  int32_t *cand_count;     /* [M, S] */
  float *cand_theta;       /* [M, S], -inf where the chunk dropped nothing */
  void *workspace;         /* gs_feature_knn_workspace_bytes bytes, 16-byte aligned */
  uint64_t workspace_bytes;
} gs_feature_knn_args;

/* sizeof(gs_feature_knn_args) as the library was compiled (for binding mirrors). */
size_t gs_feature_knn_struct_bytes(void);

/* The database chunks of the scan: a pure function of the sizes (0 for sizes out of range). */
int32_t gs_feature_knn_splits(int32_t M, int32_t N, int32_t E, int32_t k);

/* Workspace of one call; self != 0: no queries (M = N).  splits as in the struct.  0 for sizes out of range. */
size_t gs_feature_knn_workspace_bytes(int32_t M, int32_t N, int32_t E, int32_t k, int32_t splits, int32_t self);

/* The certificate's bound on |st - s| for E channels (0 for E out of range). */
double gs_feature_knn_bound(int32_t E);

/* E padded to the matrix cores' k-step. */
int32_t gs_feature_knn_e_pad(int32_t E);

/* The argument check gs_feature_knn runs first (host code, no device access). */
int gs_feature_knn_validate(const gs_feature_knn_args *args);

int gs_feature_knn(const gs_feature_knn_args *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_FEATURE_KNN_H */
