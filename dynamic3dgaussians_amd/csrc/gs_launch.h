// gs_launch.h -- what every entry point that launches kernels shares: the
// post-launch status check and typed pointers into a carved buffer.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gs_meta.h"

namespace gs {

// Post-launch check: always catch launch errors; with `debug`, also
// synchronise and surface asynchronous faults (the reference's CHECK_CUDA
// debug mode, CR/auxiliary.h:172-179).
inline int launch_status(const char* what, int debug, hipStream_t s) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && debug) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return gs_set_error((int)e, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

template <class T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
template <class T>
const T* at(const void* base, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }

}  // namespace gs
