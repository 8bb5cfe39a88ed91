// gs_feature_knn_host.cpp -- host-only part of the cosine top-k search's C ABI
// (include/gs_feature_knn.h): the struct size, the chunk rule, the workspace
// size, the certificate's bound and the argument validator gs_feature_knn
// runs before it enqueues anything.  Plain C++ with no HIP dependency, so the
// same file is linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/feature_knn_host_sanitize.c (tests/test_feature_knn.py).
#include <stdint.h>

#include "../../include/gs_feature_knn.h"
#include "gs_feature_knn_layout.h"
#include "gs_host_util.h"

using namespace gs;

namespace {
const char* const WHO = "feature knn";
const char* const TWIN = "feature_knn_torch takes any size";
}  // namespace

extern "C" {

size_t gs_feature_knn_struct_bytes(void) { return sizeof(gs_feature_knn_args); }

int32_t gs_feature_knn_splits(int32_t M, int32_t N, int32_t E, int32_t k) {
  return fk_sizes_ok(M, N, E, k) ? fk_splits(M, N) : 0;
}

size_t gs_feature_knn_workspace_bytes(int32_t M, int32_t N, int32_t E, int32_t k, int32_t splits, int32_t self) {
  if (!fk_sizes_ok(M, N, E, k) || splits < 0 || splits > GS_FKNN_MAX_SPLITS || (self && M != N)) return 0;
  return FeatureKnnLayout(M, N, E, k, splits, self != 0).total;
}

double gs_feature_knn_bound(int32_t E) { return E >= 1 && E <= GS_FKNN_MAX_E ? fk_bound(E) : 0.0; }

int32_t gs_feature_knn_e_pad(int32_t E) { return E >= 1 && E <= GS_FKNN_MAX_E ? fk_e_pad(E) : 0; }

int gs_feature_knn_validate(const gs_feature_knn_args* a) {
  if (!a) return gs_set_error(-1, "%s: null argument block", WHO);
  if (a->E < 1 || a->E > GS_FKNN_MAX_E)
    return gs_set_error(-1, "%s: E must be in [1, %d] (got %d); %s", WHO, GS_FKNN_MAX_E, a->E, TWIN);
  if (a->k < 1 || a->k > GS_KNN_MAX_K)
    return gs_set_error(-1, "%s: k must be in [1, %d] (got %d); %s", WHO, GS_KNN_MAX_K, a->k, TWIN);
  if (a->N < 1 || a->N > GS_FKNN_MAX_ROWS)
    return gs_set_error(-1, "%s: N must be in [1, %d] (got %d)", WHO, GS_FKNN_MAX_ROWS, a->N);
  if (a->M < 1 || a->M > GS_FKNN_MAX_ROWS)
    return gs_set_error(-1, "%s: M must be in [1, %d] (got %d)", WHO, GS_FKNN_MAX_ROWS, a->M);
  if (!a->queries && a->M != a->N)
    return gs_set_error(-1, "%s: without queries M must equal N (got %d, %d)", WHO, a->M, a->N);
  if (a->splits < 0 || a->splits > GS_FKNN_MAX_SPLITS)
    return gs_set_error(-1, "%s: splits must be in [0, %d] (got %d)", WHO, GS_FKNN_MAX_SPLITS, a->splits);
  if (!a->feats) return gs_set_error(-1, "%s: feats is required", WHO);
  if (!a->sim || !a->index) return gs_set_error(-1, "%s: sim and index are required", WHO);
  const int debug = (a->cand_sim != nullptr) + (a->cand_index != nullptr) + (a->cand_count != nullptr) +
                    (a->cand_theta != nullptr);
  if (debug != 0 && debug != 4)
    return gs_set_error(-1, "%s: cand_sim, cand_index, cand_count and cand_theta go together", WHO);
  const void* const p4[] = {a->feats, a->queries, a->cand_sim, a->cand_index, a->cand_count, a->cand_theta};
  for (const void* p : p4)
    if (!aligned4(p)) return gs_set_error(-1, "%s: every pointer must be 4-byte aligned", WHO);
  const void* const p8[] = {a->sim, a->index, a->stats};
  for (const void* p : p8)
    if (reinterpret_cast<uintptr_t>(p) & 7u)
      return gs_set_error(-1, "%s: sim, index and stats must be 8-byte aligned", WHO);
  return check_workspace(WHO, a->workspace, a->workspace_bytes,
                         FeatureKnnLayout(a->M, a->N, a->E, a->k, a->splits, !a->queries).total);
}

}  // extern "C"
