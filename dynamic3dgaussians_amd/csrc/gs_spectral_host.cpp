// gs_spectral_host.cpp -- host-only part of the spectral embedding's C ABI
// (include/gs_spectral.h): the struct size, the block-width rule, the
// workspace size, the argument validator gs_spectral_embedding runs before it
// enqueues anything, and the host build of the small problems
// (gs_spectral_small.h).  Plain C++ with no HIP dependency, so the same file
// is linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/spectral_host_sanitize.c (tests/test_spectral.py).
#include <stdint.h>

#include <vector>

#include "../../include/gs_spectral.h"
#include "gs_host_util.h"
#include "gs_spectral_layout.h"
#include "gs_spectral_small.h"

using namespace gs;

namespace {
const char* const WHO = "spectral embedding";
const char* const TWIN = "spectral_embedding_torch takes any size";

struct HostSmall {
  std::vector<double> A, V, rot, red, scale, evecs;
  std::vector<int> pq;
  SymEigScratch w;
  explicit HostSmall(int B)
      : A((size_t)sp_even(B) * sp_ld(B)), V(A.size()), rot(3 * sp_even(B) / 2 + 3), red(2), scale(sp_even(B)),
        evecs((size_t)B * B), pq(sp_even(B) + 2), w{rot.data(), pq.data(), red.data(), 0} {}
};
}  // namespace

extern "C" {

size_t gs_spectral_struct_bytes(void) { return sizeof(gs_spectral_args); }

int32_t gs_spectral_block_width(int32_t n, int32_t K) { return sp_sizes_ok(n, 0, K) ? sp_block_width(n, K) : 0; }

size_t gs_spectral_workspace_bytes(int32_t n, int64_t nnz, int32_t K) {
  return sp_sizes_ok(n, nnz, K) ? SpectralLayout(n, K).total : 0;
}

int gs_spectral_validate(const gs_spectral_args* a) {
  if (!a) return gs_set_error(-1, "%s: null argument block", WHO);
  if (a->num_vectors < 1 || a->num_vectors > GS_SPECTRAL_MAX_K)
    return gs_set_error(-1, "%s: num_vectors must be in [1, %d] (got %d); %s", WHO, GS_SPECTRAL_MAX_K, a->num_vectors,
                        TWIN);
  if (a->n < a->num_vectors || a->n > GS_SPECTRAL_MAX_N)
    return gs_set_error(-1, "%s: n must be in [num_vectors, %d] (got n = %d, num_vectors = %d)", WHO,
                        GS_SPECTRAL_MAX_N, a->n, a->num_vectors);
  if (a->nnz < 0 || a->nnz >= ((int64_t)1 << 31))
    return gs_set_error(-1, "%s: nnz must be in [0, 2^31) (got %lld)", WHO, (long long)a->nnz);
  if (a->degree < 1 || a->degree > GS_SPECTRAL_MAX_DEGREE)
    return gs_set_error(-1, "%s: degree must be in [1, %d] (got %d)", WHO, GS_SPECTRAL_MAX_DEGREE, a->degree);
  if (a->max_outer < 1 || a->max_outer > GS_SPECTRAL_MAX_OUTER)
    return gs_set_error(-1, "%s: max_outer must be in [1, %d] (got %d)", WHO, GS_SPECTRAL_MAX_OUTER, a->max_outer);
  if (!(a->tol > 0.0) || !sp_finite(a->tol)) return gs_set_error(-1, "%s: tol must be positive and finite", WHO);
  if (a->row_normalize != 0 && a->row_normalize != 1)
    return gs_set_error(-1, "%s: row_normalize must be 0 or 1 (got %d)", WHO, a->row_normalize);
  if (!a->row_ptr) return gs_set_error(-1, "%s: row_ptr is required", WHO);
  if (a->nnz > 0 && (!a->col || !a->val)) return gs_set_error(-1, "%s: col and val are required", WHO);
  if (!a->eigenvalues || !a->vectors || !a->embedding || !a->residuals || !a->status)
    return gs_set_error(-1, "%s: eigenvalues, vectors, embedding, residuals and status are required", WHO);
  const void* const p4[] = {a->col, a->embedding, a->status};
  for (const void* p : p4)
    if (!aligned4(p)) return gs_set_error(-1, "%s: col, embedding and status must be 4-byte aligned", WHO);
  const void* const p8[] = {a->row_ptr, a->val, a->eigenvalues, a->vectors, a->residuals};
  for (const void* p : p8)
    if (reinterpret_cast<uintptr_t>(p) & 7u)
      return gs_set_error(-1, "%s: row_ptr, val, eigenvalues, vectors and residuals must be 8-byte aligned", WHO);
  return check_workspace(WHO, a->workspace, a->workspace_bytes, SpectralLayout(a->n, a->num_vectors).total);
}

int gs_spectral_svqb_host(int32_t B, const double* G, double* T, int32_t* replaced) {
  if (B < 1 || B > GS_SPECTRAL_MAX_B || !G || !T || !replaced)
    return gs_set_error(-1, "%s: svqb_host takes 1 <= B <= %d and three arrays", WHO, GS_SPECTRAL_MAX_B);
  HostSmall s(B);
  sp_svqb(B, G, s.A.data(), s.V.data(), s.w, s.scale.data(), T, replaced, 0, 1);
  return 0;
}

int gs_spectral_ritz_host(int32_t B, const double* H, double* theta, double* Q) {
  if (B < 1 || B > GS_SPECTRAL_MAX_B || !H || !theta || !Q)
    return gs_set_error(-1, "%s: ritz_host takes 1 <= B <= %d and three arrays", WHO, GS_SPECTRAL_MAX_B);
  HostSmall s(B);
  sp_ritz(B, H, s.A.data(), s.V.data(), s.w, s.evecs.data(), theta, Q, 0, 1);
  return 0;
}

}  // extern "C"
