// The inverse of a solver's explicit k x k Hessian, one matrix for the whole batch (own.hip, split_bregman.hip):
//   Hinv = (W^T W / scale + shift I)^-1
// in double through the library's own Gram and Cholesky, rounded to float once.  A header of its own beside
// solver_common.hpp so that only the two solvers that launch these kernels carry them.
#pragma once
#include "solver_common.hpp"

namespace lasso {
namespace solver {
namespace {

// the double stage: W widened, its Gram (and the Gram entry point's second product, unused), the identity, the inverse
struct HinvStage {
  double *Wd, *G, *Gx, *I, *Hd;
  void* ridge;
  size_t ridge_bytes;
};

HinvStage carve_hinv(Arena& a, int64_t d, int64_t k) {
  HinvStage w;
  const size_t kk8 = (size_t)k * k * 8;
  w.Wd = a.take<double>((size_t)d * k * 8);
  w.G = a.take<double>(kk8);
  w.Gx = a.take<double>((size_t)k * 8);
  w.I = a.take<double>(kk8);
  w.Hd = a.take<double>(kk8);
  w.ridge_bytes = lasso_ridge_f64_workspace_bytes(k, k);
  w.ridge = a.take<char>(w.ridge_bytes);
  return w;
}

__global__ __launch_bounds__(256) void widen_kernel(const float* __restrict__ W, int64_t ldw, double* __restrict__ Wd, int d, int k) {
  const int64_t total = (int64_t)d * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    Wd[i] = (double)W[(i / k) * ldw + (i % k)];
}

// G = G / scale, I = the identity
__global__ __launch_bounds__(256) void scale_identity_kernel(double* __restrict__ G, double* __restrict__ I, int k, double scale) {
  const int64_t total = (int64_t)k * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    G[i] = G[i] / scale;
    I[i] = (i / k) == (i % k) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void narrow_kernel(const double* __restrict__ S, float* __restrict__ Dst, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) Dst[i] = (float)S[i];
}

// Hinv [k][k] of the dictionary w [d][k] (pitch ldw); returns lasso_ridge_solve_f64's status.  With info_out the call
// waits for the pivots' verdict (0, or 1 + the first pivot that is not positive).  Without, nothing is read: the verdict
// stays in the word behind the ridge workspace -- a bad pivot is replaced by 1 and the factorisation goes on, nothing
// faults meanwhile.
int build_hinv(const float* w, int64_t ldw, int d, int k, double scale, double shift, const HinvStage& s, float* Hinv,
               int32_t* info_out, hipStream_t st) {
  const int64_t kk = (int64_t)k * k;
  hipLaunchKernelGGL(widen_kernel, dim3(ew_grid((int64_t)d * k)), dim3(256), 0, st, w, ldw, s.Wd, d, k);
  LASSO_HIP_TRY(hipGetLastError());
  // (the Gram entry point also forms Z^T X: one column of W stands for X, its product is not used)
  if (int e = lasso_gram_accumulate_f64(s.Wd, k, s.Wd, k, d, 1, k, s.G, s.Gx, nullptr, 0, st)) return e;
  hipLaunchKernelGGL(scale_identity_kernel, dim3(ew_grid(kk)), dim3(256), 0, st, s.G, s.I, k, scale);
  LASSO_HIP_TRY(hipGetLastError());
  if (int e = lasso_ridge_solve_f64(s.G, s.I, s.Hd, k, k, k, shift, info_out, s.ridge, s.ridge_bytes, st)) return e;
  hipLaunchKernelGGL(narrow_kernel, dim3(ew_grid(kk)), dim3(256), 0, st, s.Hd, Hinv, kk);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

}  // namespace
}  // namespace solver
}  // namespace lasso
