// Device helpers shared by the float64 translation units (gemm_f64.hip, conv_f64.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace lasso {
namespace f64 {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// sum of v over the workgroup's 256 threads in a fixed tree; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ATen's softshrink, u > lam ? u - lam : (u < -lam ? u + lam : 0), evaluated as u - clamp(u, -lam, lam) like the fp32
// kernels (tile_device.hpp): u - lam and u - (-lam) are the same IEEE operations, u - u is +0 (for -0 and at the ties
// |u| == lam as well), +-Inf - (+-lam) stays +-Inf -- and a NaN u stays NaN as in ATen (fmax drops it, the subtraction
// brings it back), where the ternary sent it to 0.
__device__ __forceinline__ double softshrink(double u, double lam) {
  return u - fmin(fmax(u, -lam), lam);
}

}  // namespace f64
}  // namespace lasso
