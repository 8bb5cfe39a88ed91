// gs_camera_grad_layout.h -- reduction geometry and workspace layout of the
// camera-gradient kernels (gs_camera_grad.hip), shared with their host-only
// validator (gs_camera_grad_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int CG_THREADS = 256;
constexpr int CG_ITEMS = 8;                         // Gaussians per thread
constexpr int CG_CHUNK = CG_THREADS * CG_ITEMS;     // Gaussians per workgroup
constexpr int CG_VIEW = 12, CG_PROJ = 12, CG_POS = 3;
constexpr int CG_LIVE = CG_VIEW + CG_PROJ + CG_POS; // 27 sums per (camera, workgroup)
constexpr int CG_REC = 32;                          // doubles per record (256 B)
constexpr int CG_MAX_CAMS = 64;                     // gs_common.h GS_MAX_CAMS

// workgroups (= records) per camera
inline int64_t camera_grad_chunks(int64_t P) { return P > 0 ? (P + CG_CHUNK - 1) / CG_CHUNK : 0; }
inline size_t camera_grad_bytes(int64_t P, int32_t C) {
  if (C < 1 || C > CG_MAX_CAMS) return 0;
  return sizeof(double) * CG_REC * (size_t)camera_grad_chunks(P) * (size_t)C;
}

}  // namespace gs
