// gs_window_host.cpp -- host-only part of the temporal-window camera batch's
// C ABI (include/gs_window.h): the window validator that the *_window entry
// points (gs_api.hip) run before they enqueue anything.  Plain C++ with no HIP
// dependency, so the same file is linked into libgsplat_hip.so and into the
// CPU sanitizer program tools/window_host_sanitize.c (tests/test_window.py).
#include <stdint.h>

#include "../../include/gs_window.h"
#include "gs_meta.h"

extern "C" int gs_check_window(const gs_window* w, int32_t C) {
  if (!w) return gs_set_error(-1, "window: null window");
  if (w->B < 1 || w->B > GS_WINDOW_MAX_FRAMES)
    return gs_set_error(-1, "window: B must be in [1, %d] frames (got %d)", GS_WINDOW_MAX_FRAMES, w->B);
  if (C < 1) return gs_set_error(-1, "window: camera count %d < 1", C);
  if (!w->cam_frame) return gs_set_error(-1, "window: null cam_frame");
  for (int32_t c = 0; c < C; ++c) {
    const int32_t f = w->cam_frame[c];
    if (f < 0 || f >= w->B)
      return gs_set_error(-1, "window: cam_frame[%d] = %d is outside [0, %d)", c, f, w->B);
    if (c > 0 && f < w->cam_frame[c - 1])
      return gs_set_error(-1, "window: cam_frame must be non-decreasing (cam_frame[%d] = %d after %d): sort the "
                              "cameras by frame", c, f, w->cam_frame[c - 1]);
  }
  return 0;
}
