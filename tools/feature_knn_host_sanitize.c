/* feature_knn_host_sanitize.c -- stand-alone driver of the cosine top-k
 * search's host validator (dynamic3dgaussians_amd/csrc/gs_feature_knn_host.cpp)
 * for a CPU sanitizer build (tests/test_feature_knn.py compiles this file,
 * gs_host.cpp and gs_feature_knn_host.cpp with -fsanitize=address,undefined
 * and runs the program).  It walks valid and invalid argument blocks; the
 * validator must accept / refuse each one with a message and touch nothing it
 * was not given.  The pointers name heap buffers, none of which the validator
 * may dereference.  Exit status 0 and "feature knn host sanitize ok" on
 * success. */
#include <stdlib.h>

#include "gs_feature_knn.h"
#include "host_sanitize.h"

static int fk_refused(const gs_feature_knn_args *a, const char *needle) {
  return refused(gs_feature_knn_validate(a), needle);
}

int main(void) {
  const int N = 2049, M = 300, E = 35, k = 8;
  expect(gs_feature_knn_struct_bytes() == sizeof(gs_feature_knn_args), "struct size");
  expect(gs_feature_knn_e_pad(E) == 48 && gs_feature_knn_e_pad(128) == 128 && gs_feature_knn_e_pad(129) == 0, "e_pad");
  expect(gs_feature_knn_bound(E) > 0 && gs_feature_knn_bound(E) < 1e-3 && gs_feature_knn_bound(0) == 0, "bound");
  expect(gs_feature_knn_bound(128) > gs_feature_knn_bound(16), "the bound grows with the products summed");
  expect(gs_feature_knn_splits(300000, 300000, 32, 20) == 1, "no split when the query blocks fill the chip");
  expect(gs_feature_knn_splits(16, 300000, 32, 20) == GS_FKNN_MAX_SPLITS, "a few queries: the most chunks");
  expect(gs_feature_knn_splits(M, N, E, k) == 16, "65 tiles: 16 chunks of at least four");
  expect(gs_feature_knn_splits(0, N, E, k) == 0 && gs_feature_knn_splits(M, N, 129, k) == 0 &&
             gs_feature_knn_splits(M, N, E, 33) == 0,
         "splits of a size out of range is 0");
  const size_t ws_q = gs_feature_knn_workspace_bytes(M, N, E, k, 0, 0);
  const size_t ws_self = gs_feature_knn_workspace_bytes(N, N, E, k, 0, 1);
  /* xh and its pieces: 2080 padded rows of 48 channels, 4 + 6 bytes a channel */
  expect(ws_q > (size_t)2080 * 48 * 10 + (size_t)320 * 48 * 10 && ws_self > (size_t)2080 * 48 * 10, "covers xh and the pieces");
  expect(gs_feature_knn_workspace_bytes(M, N, E, k, 8, 0) < gs_feature_knn_workspace_bytes(M, N, E, k, 16, 0) &&
             gs_feature_knn_workspace_bytes(M, N, E, k, 16, 0) == ws_q,
         "the candidates grow with the chunks; 0 is the rule's count");
  expect(gs_feature_knn_workspace_bytes(M, N, E, k, 0, 1) == 0, "a self search has M = N");
  expect(gs_feature_knn_workspace_bytes(M, N, E, k, 33, 0) == 0 && gs_feature_knn_workspace_bytes(M, N, E, k, -1, 0) == 0 &&
             gs_feature_knn_workspace_bytes(M, 0, E, k, 0, 0) == 0,
         "workspace of a size out of range is 0");
  expect(gs_feature_knn_workspace_bytes(GS_FKNN_MAX_ROWS, GS_FKNN_MAX_ROWS, 128, 32, 0, 1) > ((size_t)1 << 32),
         "sizes past 32 bits");

  float *feats = malloc(64), *queries = malloc(64), *cs = malloc(64), *ct = malloc(64);
  double *sim = malloc(64);
  int64_t *index = malloc(64), *stats = malloc(64);
  int32_t *ci = malloc(64), *cc = malloc(64);
  void *ws = aligned_alloc(256, 4096);
  if (!feats || !queries || !cs || !ct || !sim || !index || !stats || !ci || !cc || !ws) return 2;

  gs_feature_knn_args good;
  memset(&good, 0, sizeof(good));
  good.N = N; good.M = M; good.E = E; good.k = k;
  good.feats = feats; good.queries = queries; good.sim = sim; good.index = index; good.stats = stats;
  good.workspace = ws; good.workspace_bytes = ws_q;

  /* valid blocks */
  expect(gs_feature_knn_validate(&good) == 0, "query block");
  gs_feature_knn_args ok = good;
  ok.stats = NULL; expect(gs_feature_knn_validate(&ok) == 0, "no stats");
  ok = good; ok.queries = NULL; ok.M = N; ok.workspace_bytes = ws_self; expect(gs_feature_knn_validate(&ok) == 0, "self block");
  ok = good; ok.cand_sim = cs; ok.cand_index = ci; ok.cand_count = cc; ok.cand_theta = ct;
  expect(gs_feature_knn_validate(&ok) == 0, "debug block");
  ok = good; ok.splits = 3; expect(gs_feature_knn_validate(&ok) == 0, "fewer chunks fit the same workspace");
  ok = good; ok.N = 1; ok.M = 1; ok.E = 1; ok.k = 1; expect(gs_feature_knn_validate(&ok) == 0, "all ones");
  ok = good; ok.E = 128; ok.k = 32; ok.workspace_bytes = gs_feature_knn_workspace_bytes(M, N, 128, 32, 0, 0);
  expect(gs_feature_knn_validate(&ok) == 0, "the limits themselves");

  /* invalid blocks, one fault each */
  gs_feature_knn_args bad;
  expect(fk_refused(NULL, "null argument block"), "null block");
  bad = good; bad.E = 0; expect(fk_refused(&bad, "E must be in"), "E = 0");
  bad = good; bad.E = 129; expect(fk_refused(&bad, "feature_knn_torch"), "E = 129 names the twin");
  bad = good; bad.k = 0; expect(fk_refused(&bad, "k must be in"), "k = 0");
  bad = good; bad.k = 33; expect(fk_refused(&bad, "feature_knn_torch"), "k = 33 names the twin");
  bad = good; bad.N = 0; expect(fk_refused(&bad, "N must be in"), "N = 0");
  bad = good; bad.N = -4; expect(fk_refused(&bad, "N must be in"), "N < 0");
  bad = good; bad.M = GS_FKNN_MAX_ROWS + 1; expect(fk_refused(&bad, "M must be in"), "M past the limit");
  bad = good; bad.queries = NULL; expect(fk_refused(&bad, "M must equal N"), "self search with M != N");
  bad = good; bad.splits = 33; expect(fk_refused(&bad, "splits must be in"), "splits = 33");
  bad = good; bad.splits = -1; expect(fk_refused(&bad, "splits must be in"), "splits < 0");
  bad = good; bad.feats = NULL; expect(fk_refused(&bad, "feats is required"), "null feats");
  bad = good; bad.sim = NULL; expect(fk_refused(&bad, "sim and index are required"), "null sim");
  bad = good; bad.index = NULL; expect(fk_refused(&bad, "sim and index are required"), "null index");
  bad = good; bad.cand_sim = cs; expect(fk_refused(&bad, "go together"), "one debug pointer");
  bad = good; bad.cand_sim = cs; bad.cand_index = ci; bad.cand_count = cc; expect(fk_refused(&bad, "go together"), "three");
  bad = good; bad.feats = (const float *)((const char *)feats + 2); expect(fk_refused(&bad, "4-byte aligned"), "misaligned feats");
  bad = good; bad.sim = (double *)((char *)sim + 4); expect(fk_refused(&bad, "8-byte aligned"), "misaligned sim");
  bad = good; bad.stats = (int64_t *)((char *)stats + 4); expect(fk_refused(&bad, "8-byte aligned"), "misaligned stats");
  bad = good; bad.workspace = NULL; expect(fk_refused(&bad, "workspace is required"), "null workspace");
  bad = good; bad.workspace_bytes = ws_q - 1; expect(fk_refused(&bad, "needed"), "short workspace");
  bad = good; bad.splits = 32; expect(fk_refused(&bad, "needed"), "more chunks than the workspace was sized for");
  bad = good; bad.workspace = (char *)ws + 8; expect(fk_refused(&bad, "16-byte aligned"), "misaligned workspace");

  free(feats); free(queries); free(cs); free(ct); free(sim); free(index); free(stats); free(ci); free(cc); free(ws);
  if (failures) return 1;
  printf("feature knn host sanitize ok\n");
  return 0;
}
