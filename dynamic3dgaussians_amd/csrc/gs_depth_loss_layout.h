// gs_depth_loss_layout.h -- workgroup decomposition and workspace layout of
// the depth-correlation loss (gs_depth_loss.hip), shared with its host-only
// validator (gs_depth_loss_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int DL_THREADS = 256;
constexpr int DL_VEC = 4;                        // pixels per thread and chunk: one 16-byte load of d and of g
constexpr int DL_CHUNK = DL_THREADS * DL_VEC;    // pixels per workgroup and chunk
// Workgroups per camera, both passes: one per chunk up to 128; past that a
// workgroup walks the camera's chunks with stride `groups`.  The 800 x 800
// rig plane has 625 chunks, so 27 x 128 workgroups (13.5 per CU) of five
// chunks each: a workgroup's merge tree costs as much as several chunks of
// streaming (a workgroup per chunk measured slower), and the
// finisher merges at most 128 records per camera, one per thread of its
// first two waves.
constexpr int DL_MAX_GROUPS = 128;
constexpr int DL_REC = 6;                        // floats per record: n, mean p, mean g, Sxx, Syy, Sxy
constexpr int DL_STATS = 8;                      // floats per camera in `stats`

struct DepthLossLayout {
  int64_t plane_elems, chunks, groups;  // per camera
  size_t total;                         // bytes: the records [B, groups, DL_REC] and nothing else
  DepthLossLayout(int64_t B, int64_t H, int64_t W) {
    plane_elems = H * W;
    chunks = (plane_elems + DL_CHUNK - 1) / DL_CHUNK;
    groups = chunks < DL_MAX_GROUPS ? chunks : DL_MAX_GROUPS;
    total = sizeof(float) * DL_REC * (size_t)B * (size_t)groups;
  }
};

}  // namespace gs
