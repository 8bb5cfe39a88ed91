// gs_feature_pca_host.cpp -- host-only part of the feature-map PCA's C ABI
// (include/gs_feature_pca.h): the struct size, the workspace sizes, the
// documented constants, the argument validator that every entry point of
// gs_feature_pca.hip runs before it enqueues anything, and the host build of
// the eigensolver (gs_sym_eig.h).  Plain C++ with no HIP dependency, so the
// same file is linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/feature_pca_host_sanitize.c (tests/test_feature_pca.py).
#include <stdint.h>

#include <vector>

#include "../../include/gs_feature_pca.h"
#include "gs_feature_pca_layout.h"
#include "gs_host_util.h"
#include "gs_sym_eig.h"

using namespace gs;

namespace {
const char* const PASS_NAME[6] = {"feature pca update",  "feature pca covariance", "feature pca fit",
                                  "feature pca project", "feature pca offset",     "feature pca colour"};
const char* const TWINS = "the _torch twins of feature_pca take any size";
}  // namespace

extern "C" {

size_t gs_feature_pca_struct_bytes(void) { return sizeof(gs_feature_pca); }

size_t gs_feature_pca_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t pass) {
  if (!fp_sizes_ok(B, C, H, W)) return 0;
  switch (pass) {
    case GS_FPCA_PASS_UPDATE: return FeaturePcaUpdateLayout(B, C, H, W).total;
    case GS_FPCA_PASS_FIT: return fp_fit_workspace(C);
    case GS_FPCA_PASS_PROJECT: return fp_k_ok(C, k) ? fp_project_workspace(B, H, W, k) : 0;
    default: return 0;
  }
}

int64_t gs_feature_pca_n_acc(int32_t B, int32_t H, int32_t W) {
  if (!fp_sizes_ok(B, 1, H, W)) return 0;
  const int64_t padded = ((int64_t)H * W + FP_PIX - 1) / FP_PIX * FP_PIX;
  return padded < FP_CHUNK ? padded : FP_CHUNK;
}

int32_t gs_feature_pca_max_sweeps(void) { return GS_FPCA_MAX_SWEEPS; }

int gs_feature_pca_validate(const gs_feature_pca* a, int32_t pass) {
  if (!a) return gs_set_error(-1, "feature pca: null argument block");
  if (pass < 0 || pass > 5) return gs_set_error(-1, "feature pca: unknown pass %d", pass);
  const char* who = PASS_NAME[pass];
  const bool images = pass != GS_FPCA_PASS_COVARIANCE && pass != GS_FPCA_PASS_FIT;
  if (a->C < 1 || a->C > GS_FPCA_MAX_C)
    return gs_set_error(-1, "%s: C must be in [1, %d] (got %d); %s", who, GS_FPCA_MAX_C, a->C, TWINS);
  if (images) {
    if (a->B < 1 || a->B > 65535) return gs_set_error(-1, "%s: B must be in [1, 65535] (got %d)", who, a->B);
    if (a->H < 1 || a->W < 1 || !fp_sizes_ok(a->B, a->C, a->H, a->W))
      return gs_set_error(-1, "%s: H, W must be >= 1 with H * W < 2^31 - %d (got %d, %d); %s", who, FP_CHUNK, a->H,
                          a->W, TWINS);
  }
  const bool uses_k = pass >= GS_FPCA_PASS_FIT;
  if (uses_k && !fp_k_ok(a->C, a->k))
    return gs_set_error(-1, "%s: k must be in [1, min(C, %d)] (got %d with C = %d)", who, GS_FPCA_MAX_K, a->k, a->C);
  if (pass == GS_FPCA_PASS_COLOUR && a->k != 3) return gs_set_error(-1, "%s: colour needs k = 3 (got %d)", who, a->k);
  if (pass == GS_FPCA_PASS_UPDATE && a->sample_stride < 1)
    return gs_set_error(-1, "%s: sample_stride must be >= 1 (got %d)", who, a->sample_stride);
  if ((pass == GS_FPCA_PASS_COVARIANCE || pass == GS_FPCA_PASS_FIT) && a->ddof < 0)
    return gs_set_error(-1, "%s: ddof must be >= 0 (got %d)", who, a->ddof);
  size_t need = 0;
  switch (pass) {
    case GS_FPCA_PASS_UPDATE:
      if (!a->x) return gs_set_error(-1, "%s: x is required", who);
      if (!a->shift) return gs_set_error(-1, "%s: shift is required", who);
      if (!a->state) return gs_set_error(-1, "%s: state is required", who);
      if (FeaturePcaUpdateLayout(a->B, a->C, a->H, a->W).groups > 65535)
        return gs_set_error(-1, "%s: B * ceil(H * W / %d) must be <= %d per call (got B = %d, H * W = %lld)", who,
                            FP_CHUNK, 65535 * FP_GROUP, a->B, (long long)a->H * a->W);
      need = FeaturePcaUpdateLayout(a->B, a->C, a->H, a->W).total;
      break;
    case GS_FPCA_PASS_COVARIANCE:
      if (!a->shift) return gs_set_error(-1, "%s: shift is required", who);
      if (!a->state) return gs_set_error(-1, "%s: state is required", who);
      if (!a->mean) return gs_set_error(-1, "%s: mean is required", who);
      if (!a->cov) return gs_set_error(-1, "%s: cov is required", who);
      break;
    case GS_FPCA_PASS_FIT:
      if (!a->shift) return gs_set_error(-1, "%s: shift is required", who);
      if (!a->state) return gs_set_error(-1, "%s: state is required", who);
      if (!a->mean || !a->mean_f32) return gs_set_error(-1, "%s: mean and mean_f32 are required", who);
      if (!a->evals || !a->evecs) return gs_set_error(-1, "%s: evals and evecs are required", who);
      if (!a->components || !a->components_f32)
        return gs_set_error(-1, "%s: components and components_f32 are required", who);
      if (!a->status) return gs_set_error(-1, "%s: status is required", who);
      need = fp_fit_workspace(a->C);
      break;
    case GS_FPCA_PASS_PROJECT:
      if (!a->x) return gs_set_error(-1, "%s: x is required", who);
      if (!a->proj_components || !a->proj_mean)
        return gs_set_error(-1, "%s: proj_components and proj_mean are required", who);
      if (!a->t) return gs_set_error(-1, "%s: t is required", who);
      if (!a->tmin || !a->tmax) return gs_set_error(-1, "%s: tmin and tmax are required", who);
      need = fp_project_workspace(a->B, a->H, a->W, a->k);
      break;
    case GS_FPCA_PASS_OFFSET:
      if (!a->t) return gs_set_error(-1, "%s: t is required", who);
      if (!a->sub) return gs_set_error(-1, "%s: sub is required", who);
      if (!a->u) return gs_set_error(-1, "%s: u is required", who);
      break;
    default:
      if (!a->t) return gs_set_error(-1, "%s: t is required", who);
      if (!a->lo || !a->hi) return gs_set_error(-1, "%s: lo and hi are required", who);
      if (!a->out) return gs_set_error(-1, "%s: out is required", who);
      if (!a->out_uint8 && !aligned4(a->out)) return gs_set_error(-1, "%s: every pointer must be 4-byte aligned", who);
      break;
  }
  const void* const p4[] = {a->x, a->shift, a->components_f32, a->mean_f32, a->status, a->proj_components,
                            a->proj_mean, a->t, a->tmin, a->tmax, a->sub, a->u};
  for (const void* p : p4)
    if (!aligned4(p)) return gs_set_error(-1, "%s: every pointer must be 4-byte aligned", who);
  const void* const p8[] = {a->state, a->mean, a->cov, a->evals, a->evecs, a->components, a->lo, a->hi};
  for (const void* p : p8)
    if (reinterpret_cast<uintptr_t>(p) & 7u)
      return gs_set_error(-1, "%s: every fp64 pointer must be 8-byte aligned", who);
  return check_workspace(who, a->workspace, a->workspace_bytes, need);
}

int gs_feature_pca_eig_host(int32_t C, const double* A, double* evals, double* evecs, int32_t* sweeps,
                            int64_t* rotations) {
  if (C < 1 || C > GS_FPCA_MAX_C)
    return gs_set_error(-1, "feature pca eig: C must be in [1, %d] (got %d)", GS_FPCA_MAX_C, C);
  if (!A || !evals || !evecs) return gs_set_error(-1, "feature pca eig: A, evals and evecs are required");
  const int ne = fp_even(C);
  std::vector<double> a((size_t)ne * ne, 0.0), v((size_t)ne * ne, 0.0), rot(3 * (size_t)ne / 2), red(2);
  std::vector<int> pq((size_t)ne);
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) a[(size_t)i * ne + j] = A[(size_t)i * C + j];
  SymEigScratch w{rot.data(), pq.data(), red.data(), 0};
  const int s = sym_eig_jacobi(ne, a.data(), v.data(), ne, w, GS_FPCA_MAX_SWEEPS, 0, 1);
  if (rotations) *rotations = w.rotations;
  const bool finite = s != SYM_EIG_NOT_FINITE;
  if (sweeps) *sweeps = !finite ? 0 : (s < 0 ? GS_FPCA_MAX_SWEEPS : s);
  sym_eig_sorted(C, a.data(), v.data(), ne, w, evals, evecs, !finite, 0, 1);
  return !finite ? 3 : (s < 0 ? 2 : 0);
}

}  // extern "C"
