// gs_scene_loss_layout.h -- workgroup decomposition and workspace layout of
// the scene regularisers (gs_scene_loss.hip), shared with their host-only
// validator (gs_scene_loss_host.cpp).  Plain C++, no HIP dependency.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gs {

constexpr int SL_THREADS = 256;
// The forward's grid: a workgroup per 256 rows up to SL_MAX_GROUPS, past that
// the workgroups walk the rows with stride groups * 256.  The cap is 8 x the
// MI355X's 256 CUs: a CU holds 32 waves, eight workgroups of four, so 2048
// workgroups are exactly what the chip keeps resident at once and a larger
// grid would only queue behind them.  It also bounds the workspace (32 KiB)
// and the finisher's loop (eight records per lane) whatever P is.  The rig's
// 300k rows take 1172 workgroups: below the cap, one row per thread.
constexpr int SL_CUS = 256;
constexpr int SL_GROUPS_PER_CU = 8;
constexpr int SL_MAX_GROUPS = SL_GROUPS_PER_CU * SL_CUS;
constexpr int SL_REC = 4;  // floats per workgroup record: floor, bg means, bg rotations, colour

struct SceneLossLayout {
  int64_t groups;  // the forward's workgroups
  size_t total;    // bytes: the records [groups, SL_REC] and nothing else
  explicit SceneLossLayout(int64_t P) {
    const int64_t g = (P + SL_THREADS - 1) / SL_THREADS;
    groups = g < SL_MAX_GROUPS ? g : SL_MAX_GROUPS;
    total = sizeof(float) * SL_REC * (size_t)groups;
  }
};

// slot holds ranks as int32 (-1 - r for the background), so P is at most
// 2^31 - 1; the one-thread-per-row grids (backward, gather) then fit a grid
// dimension with room to spare.
constexpr int64_t SL_MAX_ROWS = ((int64_t)1 << 31) - 1;

// The argument check of gs_fg_gather_forward / _backward (gs_scene_loss_host.cpp;
// for the backward the [P] pair are the outputs and the [n_fg] pair the inputs,
// and any of the four may be null).
int fg_gather_check(const char* who, int backward, int64_t P, int64_t n_fg, const void* slot, const void* means,
                    const void* rotations, const void* fg_pts, const void* fg_rot);

}  // namespace gs
