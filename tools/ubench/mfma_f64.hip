// Micro-benchmark: the sustained rate of v_mfma_f64_16x16x4_f64 on gfx950 -- independent accumulator chains in
// registers, no memory traffic -- so that the share of peak quoted for the float64 GEMM (csrc/gemm_f64.hip)
// is against a MEASURED ceiling.
//   ./mfma_f64   -> one JSON line per (chains per wave, waves per SIMD): the whole-chip TFLOP/s from HIP events (every CU
//                   busy) and the clock64 ticks per MFMA and SIMD of one CU -- from the first wave's start to the last
//                   wave's end over the MFMAs a SIMD issued in between (the waves of a SIMD do not finish together: the
//                   oldest one is served first, so one wave's own span says nothing about the SIMD)
// Build: hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma_f64.hip -o tools/ubench/mfma_f64
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHECK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

template <int CHAINS>
__global__ __launch_bounds__(1024) void k(double* out, int iters, long long* cyc) {
  f64x4 acc[CHAINS];
  for (int i = 0; i < CHAINS; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  __syncthreads();
  const long long t0 = clock64();
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
  }
  const long long t1 = clock64();
  double s = 0.0;
  for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0) {          // every wave's start and end
    cyc[((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 2] = t0;
    cyc[((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 2 + 1] = t1;
  }
}

template <int CHAINS>
int run(int waves_per_simd, int cus, double* out, long long* cyc) {
  const int threads = 256 * waves_per_simd, iters = 20000;        // 4 SIMDs per CU, one workgroup per CU
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k<CHAINS>, dim3(cus), dim3(threads), 0, 0, out, 2000, cyc);   // warm-up
  CHECK(hipDeviceSynchronize());
  float best = 1e30f;
  long long c0 = 0, stamps[32];
  for (int rep = 0; rep < 5; ++rep) {
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k<CHAINS>, dim3(cus), dim3(threads), 0, 0, out, iters, cyc);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best) {
      best = ms;
      CHECK(hipMemcpy(stamps, cyc, sizeof(long long) * 2 * (threads / 64), hipMemcpyDeviceToHost));   // workgroup 0
      long long lo = stamps[0], hi = stamps[1];
      for (int w = 1; w < threads / 64; ++w) { lo = stamps[2 * w] < lo ? stamps[2 * w] : lo; hi = stamps[2 * w + 1] > hi ? stamps[2 * w + 1] : hi; }
      c0 = hi - lo;
    }
  }
  const double mfmas_per_wave = (double)iters * 4 * CHAINS;
  const double flop = mfmas_per_wave * 2048.0 * (threads / 64) * cus;       // 16 x 16 x 4 x 2 per MFMA
  printf("{\"chains\": %d, \"waves_per_simd\": %d, \"cus\": %d, \"ms\": %.4f, \"tflops\": %.2f, "
         "\"clock64_ticks_per_mfma_per_simd\": %.2f}\n",
         CHAINS, waves_per_simd, cus, best, flop / best / 1e9, (double)c0 / (mfmas_per_wave * waves_per_simd));
  fflush(stdout);
  return 0;
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  double* out;
  long long* cyc;
  CHECK(hipMalloc(&out, (size_t)cus * 1024 * sizeof(double)));
  CHECK(hipMalloc(&cyc, (size_t)cus * 32 * sizeof(long long)));
  for (int w = 1; w <= 4; w *= 2) {
    if (run<1>(w, cus, out, cyc) || run<2>(w, cus, out, cyc) || run<4>(w, cus, out, cyc) || run<8>(w, cus, out, cyc)) return 1;
  }
  CHECK(hipFree(out));
  CHECK(hipFree(cyc));
  return 0;
}
