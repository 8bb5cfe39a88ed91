// gs_depth_geometry_host.cpp -- host-only part of the depth-map geometry's C
// ABI (include/gs_depth_geometry.h): struct sizes, the abs-rel workspace size
// and the argument validators that the entry points (gs_depth_geometry.hip)
// run before they enqueue anything.  Plain C++ with no HIP dependency, so the
// same file is linked into libgsplat_hip.so and into the CPU sanitizer program
// tools/depth_geometry_host_sanitize.c (tests/test_depth_geometry.py).
#include <stdint.h>

#include "../../include/gs_depth_geometry.h"
#include "gs_depth_geometry_layout.h"
#include "gs_host_util.h"

using namespace gs;

namespace {

// B, H, W of a per-pixel call.
int check_image_shape(const char* who, int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return gs_set_error(-1, "%s: B, H, W must be > 0 (got %d, %d, %d)", who, B, H, W);
  if (B > DG_MAX_B || H > DG_MAX_SIDE || W > DG_MAX_SIDE)
    return gs_set_error(-1, "%s: batch of %d x %d x %d is too large (B <= %d, H, W <= %d)", who, B, H, W, DG_MAX_B,
                        DG_MAX_SIDE);
  return 0;
}

}  // namespace

extern "C" {

size_t gs_point_depth_struct_bytes(void) { return sizeof(struct gs_point_depth); }
size_t gs_depth_abs_rel_struct_bytes(void) { return sizeof(struct gs_depth_abs_rel); }
size_t gs_depth_unproject_struct_bytes(void) { return sizeof(struct gs_depth_unproject); }
size_t gs_depth_flow_struct_bytes(void) { return sizeof(struct gs_depth_flow); }
size_t gs_sample_bilinear_struct_bytes(void) { return sizeof(struct gs_sample_bilinear); }

size_t gs_depth_abs_rel_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return DepthAbsRelLayout(B, H, W).total;
}

int gs_point_depth_validate(const struct gs_point_depth* a) {
  if (!a) return gs_set_error(-1, "point depth: null argument block");
  if (int e = check_image_shape("point depth", a->B, a->H, a->W)) return e;
  if (a->P < 0 || a->P > DG_MAX_N)
    return gs_set_error(-1, "point depth: P must be in [0, 2^36] (got %lld)", (long long)a->P);
  if (a->P > 0 && !a->points) return gs_set_error(-1, "point depth: points are required when P > 0");
  if (!a->w2c || !a->K) return gs_set_error(-1, "point depth: w2c and K are required");
  if (!a->depth) return gs_set_error(-1, "point depth: depth is required");
  if (!aligned4(a->points) || !aligned4(a->w2c) || !aligned4(a->K) || !aligned4(a->depth))
    return gs_set_error(-1, "point depth: points, w2c, K and depth must be 4-byte aligned");
  if (a->points_batch_stride != 0 && a->points_batch_stride != a->P * 3)
    return gs_set_error(-1, "point depth: points_batch_stride must be 0 or P*3 = %lld (got %lld)",
                        (long long)(a->P * 3), (long long)a->points_batch_stride);
  return 0;
}

int gs_depth_abs_rel_validate(const struct gs_depth_abs_rel* a) {
  if (!a) return gs_set_error(-1, "depth abs-rel: null argument block");
  if (int e = check_image_shape("depth abs-rel", a->B, a->H, a->W)) return e;
  const DepthAbsRelLayout L(a->B, a->H, a->W);
  if (!a->est || !a->gt) return gs_set_error(-1, "depth abs-rel: est and gt are required");
  if (!a->out) return gs_set_error(-1, "depth abs-rel: out is required");
  if (!aligned4(a->est) || !aligned4(a->gt) || !aligned4(a->exclude))
    return gs_set_error(-1, "depth abs-rel: est, gt and exclude must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(a->out) & 7u) != 0)
    return gs_set_error(-1, "depth abs-rel: out must be 8-byte aligned");
  if (a->exclude && a->exclude_batch_stride != 0 && a->exclude_batch_stride != L.plane_elems)
    return gs_set_error(-1, "depth abs-rel: exclude_batch_stride must be 0 or H*W = %lld (got %lld)",
                        (long long)L.plane_elems, (long long)a->exclude_batch_stride);
  return check_workspace("depth abs-rel", a->workspace, a->workspace_bytes, L.total);
}

int gs_depth_unproject_validate(const struct gs_depth_unproject* a) {
  if (!a) return gs_set_error(-1, "depth unproject: null argument block");
  if (int e = check_image_shape("depth unproject", a->B, a->H, a->W)) return e;
  if (!a->depth) return gs_set_error(-1, "depth unproject: depth is required");
  if (!a->Kinv || !a->c2w) return gs_set_error(-1, "depth unproject: Kinv and c2w are required");
  if (!a->xyz) return gs_set_error(-1, "depth unproject: xyz is required");
  if (!aligned4(a->depth) || !aligned4(a->xy) || !aligned4(a->Kinv) || !aligned4(a->c2w) || !aligned4(a->xyz))
    return gs_set_error(-1, "depth unproject: depth, xy, Kinv, c2w and xyz must be 4-byte aligned");
  return 0;
}

int gs_depth_flow_validate(const struct gs_depth_flow* a) {
  if (!a) return gs_set_error(-1, "depth flow: null argument block");
  if (int e = check_image_shape("depth flow", a->B, a->H, a->W)) return e;
  if (!a->depth1) return gs_set_error(-1, "depth flow: depth1 is required");
  if (!a->Kinv1 || !a->T || !a->K2) return gs_set_error(-1, "depth flow: Kinv1, T and K2 are required");
  if (!a->flow) return gs_set_error(-1, "depth flow: flow is required");
  if (!aligned4(a->depth1) || !aligned4(a->Kinv1) || !aligned4(a->T) || !aligned4(a->K2) || !aligned4(a->flow))
    return gs_set_error(-1, "depth flow: depth1, Kinv1, T, K2 and flow must be 4-byte aligned");
  return 0;
}

int gs_sample_bilinear_validate(const struct gs_sample_bilinear* a) {
  if (!a) return gs_set_error(-1, "sample bilinear: null argument block");
  if (a->Ch <= 0) return gs_set_error(-1, "sample bilinear: Ch must be > 0 (got %d)", a->Ch);
  if (int e = check_image_shape("sample bilinear", a->B, a->H, a->W)) return e;
  if ((int64_t)a->Ch * a->H * a->W > ((int64_t)1 << 40))
    return gs_set_error(-1, "sample bilinear: source of %d x %d x %d is too large", a->Ch, a->H, a->W);
  if (a->mode != GS_SAMPLE_POINTS && a->mode != GS_SAMPLE_DISPLACEMENT)
    return gs_set_error(-1, "sample bilinear: mode must be GS_SAMPLE_POINTS or GS_SAMPLE_DISPLACEMENT (got %d)",
                        a->mode);
  if (a->N <= 0 || a->N > DG_MAX_N)
    return gs_set_error(-1, "sample bilinear: N must be in [1, 2^36] (got %lld)", (long long)a->N);
  if (a->mode == GS_SAMPLE_DISPLACEMENT) {
    if (a->h <= 0 || a->w <= 0 || a->h > DG_MAX_SIDE || a->w > DG_MAX_SIDE)
      return gs_set_error(-1, "sample bilinear: h, w must be in [1, %d] (got %d, %d)", DG_MAX_SIDE, a->h, a->w);
    if (a->N != (int64_t)a->h * a->w)
      return gs_set_error(-1, "sample bilinear: N must be h*w = %lld in displacement mode (got %lld)",
                          (long long)a->h * a->w, (long long)a->N);
  }
  if (a->add_displacement && (a->mode != GS_SAMPLE_DISPLACEMENT || a->Ch != 2))
    return gs_set_error(-1, "sample bilinear: add_displacement needs displacement mode and Ch == 2");
  if (!a->src) return gs_set_error(-1, "sample bilinear: src is required");
  if (!a->coords) return gs_set_error(-1, "sample bilinear: coords are required");
  if (!a->out) return gs_set_error(-1, "sample bilinear: out is required");
  if (!aligned4(a->src) || !aligned4(a->coords) || !aligned4(a->out))
    return gs_set_error(-1, "sample bilinear: src, coords and out must be 4-byte aligned");
  return 0;
}

}  // extern "C"
