// Host-side plumbing shared by the translation units behind the C ABI: workspace carving and the error channel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/lasso_hip.h"

namespace lasso {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Carves a caller-owned workspace into 256-byte aligned regions, in the order of the take() calls.  A null base gives
// null pointers and the same offsets: the *_workspace_bytes queries carve nothing and read bytes().
struct Arena {
  char* base;
  size_t off = 0;
  size_t min_take = 0;      // smallest region (the convolution workspaces keep empty tensors apart: 4)
  explicit Arena(void* b, size_t min_take_ = 0) : base(static_cast<char*>(b)), min_take(min_take_) {}
  template <class T = float>
  T* take(size_t bytes) {
    char* r = base ? base + off : nullptr;
#ifdef LASSO_ARENA_OBSERVER      // tools/arena_check.hip: sees every region, to touch its first and last byte
    LASSO_ARENA_OBSERVER(r, std::max(bytes, min_take));
#endif
    off += align_up(std::max(bytes, min_take));
    return reinterpret_cast<T*>(r);
  }
  size_t bytes() const { return off; }
};

// Leaves the detail text of a failure for lasso_hip_last_error() (thread-local, lasso_hip.hip) and returns `status`.
int fail(int status, const char* fmt, ...);

#define LASSO_HIP_TRY(expr)                                                                  \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return ::lasso::fail(LASSO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

// `bytes` from device memory to the host, and the wait for them: the one read of a chunk's sums or of a kernel's result words
inline int read_back(void* host, const void* dev, size_t bytes, hipStream_t st) {
  LASSO_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace lasso
