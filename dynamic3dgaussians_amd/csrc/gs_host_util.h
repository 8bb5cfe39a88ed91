// gs_host_util.h -- pointer checks shared by the argument validators.  Plain
// C++ with no HIP dependency: the host-only translation units that include it
// are also built into the CPU sanitizer programs (tools/*_host_sanitize.c).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gs_meta.h"

namespace gs {

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A caller's workspace of `have` bytes against the `need` bytes of the op's
// layout (need = 0: the op uses none, nothing is checked).
inline int check_workspace(const char* who, const void* ws, uint64_t have, size_t need) {
  if (need == 0) return 0;
  if (!ws) return gs_set_error(-1, "%s: workspace is required (%zu bytes)", who, need);
  if (have < need)
    return gs_set_error(-1, "%s: workspace of %llu bytes, %zu needed", who, (unsigned long long)have, need);
  if (!aligned16(ws)) return gs_set_error(-1, "%s: workspace must be 16-byte aligned", who);
  return 0;
}

}  // namespace gs
