// What the batch solvers on the fp32 MFMA GEMM share (gpsr_driver.hpp, own.hip, iter_ridge.hip, split_bregman.hip,
// interior_point.hip): the fixed-order reductions, the launch rules, and the shell of every "main loop of gemm.hip plus an
// epilogue of the solver's own" product, written once:
//   Tile          where a thread's accumulator fragments lie in the block, and its operands through buffer descriptors
//   gemm_kernel   A advanced to its rung, gemm_nt_accumulate (gemm_mainloop.hpp), the Tile, then the epilogue E
//   launch_gemm   128 x 128 or 64 x 64 blocks; LDS-DMA, 16-byte buffer loads or scalar loads of the operands
// An epilogue E is a plain struct of kernel arguments with the field a_stride (per rung offset of the A operand) and
//   template <int BM, int BN> __device__ void run(const Tile<BM, BN>&, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const
// which walks the fragments in the order (mi, nj, rg), does its loads, arithmetic and stores, and (where it sums) ends
// with block_fold into t.partial(part).  The two plain products every solver needs are here: StoreEpi, Resid0Epi.
// All sums: per thread, wave butterfly, the four waves, block partial (double) -- then ONE workgroup folds the partials
// in a fixed order (fold_partials): no float atomics, two solves of the same arguments are bitwise equal.
// Everything sits in an unnamed namespace: each translation unit carries its own copy of what it uses.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"
#include "gemm_mainloop.hpp"

namespace lasso {
namespace solver {
namespace {

using gemm_detail::f32x4;

constexpr int kPart = 8;              // doubles per block partial
constexpr int kEwBlocks = 1024;       // most blocks of an element-wise launch

// sums s[NS] and maxima mx[NM] of a block of 256 threads in a fixed order -> out[NS + NM] by thread 0
template <int NS, int NM>
__device__ __forceinline__ void block_fold(double (&s)[NS > 0 ? NS : 1], float (&mx)[NM > 0 ? NM : 1], double* red /* [4][8] */,
                                           double* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] += __shfl_xor(s[i], off);
#pragma unroll
    for (int i = 0; i < NM; ++i) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], off));
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) red[w * 8 + i] = s[i];
#pragma unroll
    for (int i = 0; i < NM; ++i) red[w * 8 + NS + i] = (double)mx[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) out[i] = (red[i] + red[8 + i]) + (red[16 + i] + red[24 + i]);
#pragma unroll
    for (int i = 0; i < NM; ++i) out[NS + i] = fmax(fmax(red[NS + i], red[8 + NS + i]), fmax(red[16 + NS + i], red[24 + NS + i]));
  }
}

// ---- one-workgroup folds of the block partials (fixed order) --------------------------------------------------------
// out[i] (shared) = sum (i < ns) or max over the blocks' partial i
__device__ __forceinline__ void fold_partials(const double* __restrict__ part, int nblocks, int ns, int nm, double* red /* [256] */,
                                              double* out /* [kPart] */) {
  for (int i = 0; i < ns + nm; ++i) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
      const double v = part[(int64_t)b * kPart + i];
      a = i < ns ? a + v : fmax(a, v);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] = i < ns ? red[threadIdx.x] + red[threadIdx.x + h] : fmax(red[threadIdx.x], red[threadIdx.x + h]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[i] = red[0];
    __syncthreads();
  }
}

// ---- the shell of a product with an epilogue ---------------------------------------------------------------------------
// The block (blockIdx.y, blockIdx.x) of C = A B^T as one of its 256 threads sees it: wave (wr, wc) owns a quarter, and
// fragment (mi, nj) of it holds, in register rg, the element
//   row (BM / 2) wr + 16 mi + 4 q + rg of the block,  column j0 + (BN / 2) wc + 16 nj + l15 of C.
// The epilogue's operands go through buffer descriptors of the tile's rows, as in gemm.hip: an element outside C gets
// the offset kOutside, which is beyond every descriptor -- it reads 0 and its store is dropped.
template <int BM, int BN>
struct Tile {
  static constexpr int MI = BM / 32, NJ = BN / 32;
  static constexpr unsigned kOutside = 0xfffffff0u;
  int i0, j0, rows_valid, nn, wr, wc, l15, q;

  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* base, int64_t ld) const {
    const int64_t bytes = (int64_t)rows_valid * ld * 4;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (int64_t)i0 * ld), 0,
                                             (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff), 0x00020000);
  }
  // byte offset of register rg of fragment (mi, nj) in an operand of row pitch ld
  __device__ __forceinline__ unsigned off(int mi, int nj, int rg, int64_t ld) const {
    const int rl = (BM / 2) * wr + 16 * mi + 4 * q + rg, cc = j0 + (BN / 2) * wc + 16 * nj + l15;
    unsigned o = (rl < rows_valid && cc < nn) ? (unsigned)(rl * (int)ld + cc) * 4u : kOutside;
    asm volatile("" : "+v"(o));           // (opaque: with the bounds visible every element got a branch of its own, gemm.hip)
    return o;
  }
  // ... of the whole row block mi
  __device__ __forceinline__ void offs(int mi, int64_t ld, unsigned (&o)[NJ][4]) const {
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) o[nj][rg] = off(mi, nj, rg, ld);
  }
  // is the element an offset stands for inside C?  (The LDS-DMA form of the main loop clamps rows beyond the operand
  // instead of zeroing them, so a sum must leave those accumulators out.)
  static __device__ __forceinline__ bool inside(unsigned o) { return o != kOutside; }
  static __device__ __forceinline__ float ld32(__amdgpu_buffer_rsrc_t rs, unsigned o) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0));
  }
  static __device__ __forceinline__ void st32(float v, __amdgpu_buffer_rsrc_t rs, unsigned o) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, o, 0, 0);
  }
  // this block's partial in part [rungs][blocks][kPart]
  static __device__ __forceinline__ double* partial(double* part) {
    return part + ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kPart;
  }
};

// An epilogue may have `__device__ bool skip() const`: true -> the whole launch does nothing (a stop flag on the device,
// conjgrad.hip).  Epilogues without it compile to what they were.
template <class E, class = void> struct has_skip : std::false_type {};
template <class E> struct has_skip<E, std::void_t<decltype(std::declval<const E&>().skip())>> : std::true_type {};

// C = A B^T on the block (blockIdx.y, blockIdx.x), rung blockIdx.z; A [m][kk], B [nn][kk]; C goes to the epilogue
template <int BM, int BN, bool VEC, bool DMA, class E>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                      int64_t ldb, int m, int nn, int kk, E ep) {
  constexpr int MI = BM / 32, NJ = BN / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int i0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if constexpr (has_skip<E>::value)
    if (ep.skip()) return;
  A += (int64_t)blockIdx.z * ep.a_stride;
  f32x4 acc[MI][NJ] = {};
  gemm_detail::gemm_nt_accumulate<BM, BN, VEC, DMA>(A, lda, B, ldb, m, nn, kk, i0, j0, smem, acc);
  const Tile<BM, BN> t = {i0, j0, min(BM, m - i0), nn, w >> 1, w & 1, lane & 15, lane >> 4};
  ep.run(t, acc, smem);
}

// Out [m][nn] (pitch ldo) = C
struct StoreEpi {
  float* Out; int64_t ldo;
  int64_t a_stride;
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char*) const {
    const __amdgpu_buffer_rsrc_t ors = t.rsrc(Out, ldo);
#pragma unroll
    for (int mi = 0; mi < BM / 32; ++mi)
#pragma unroll
      for (int nj = 0; nj < BN / 32; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) t.st32(acc[mi][nj][rg], ors, t.off(mi, nj, rg, ldo));
  }
};

// Out [m][nn] (pitch ldo) = C - Y, block partials {sum of its squares} (the partial keeps the width GPSR's folds gave
// it: two sums and four maxima, all but the first zero)
struct Resid0Epi {
  const float* Y; int64_t ldy;
  float* Out; int64_t ldo;
  double* part;                       // [blocks][kPart]
  int64_t a_stride;
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int NJ = BN / 32;
    const __amdgpu_buffer_rsrc_t yrs = t.rsrc(Y, ldy), ors = t.rsrc(Out, ldo);
    float s0 = 0.0f;
#pragma unroll
    for (int mi = 0; mi < BM / 32; ++mi) {
      float y[NJ][4];
      unsigned oo[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          y[nj][rg] = t.ld32(yrs, t.off(mi, nj, rg, ldy));
          oo[nj][rg] = t.off(mi, nj, rg, ldo);
        }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const float r = __fsub_rn(acc[mi][nj][rg], y[nj][rg]);
          if (t.inside(oo[nj][rg])) s0 += __fmul_rn(r, r);
          t.st32(r, ors, oo[nj][rg]);
        }
    }
    double s[2] = {(double)s0, 0.0};
    float mx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    block_fold<2, 4>(s, mx, reinterpret_cast<double*>(smem), t.partial(part));
  }
};

// ---- element-wise kernels more than one solver launches ---------------------------------------------------------------
// (Templates for one reason: a __global__ function in an unnamed namespace is emitted into every object that includes
// this header, launched or not; an instantiation only where it is launched.)
// out (pitch ldo) = Z, packed [n][k] -- or zeros
template <int = 0>
__global__ __launch_bounds__(256) void copy_out_kernel(const float* __restrict__ Z, float* __restrict__ out, int64_t ldo, int n,
                                                       int k, int zero) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    out[(i / k) * ldo + (i % k)] = zero ? 0.0f : Z[i];
}

// Z, packed [n][k] = S (pitch ld0)
template <int = 0>
__global__ __launch_bounds__(256) void init_packed_kernel(const float* __restrict__ S, int64_t ld0, float* __restrict__ Z, int n, int k) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    Z[i] = S[(i / k) * ld0 + (i % k)];
}

// ---- launchers -------------------------------------------------------------------------------------------------------
int ew_grid(int64_t total) { return (int)std::max<int64_t>(1, std::min<int64_t>(kEwBlocks, (total + 1023) / 1024)); }

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    cus = 1;
  return cus;
}

// 128 x 128 blocks while they still give every CU two workgroups, 64 x 64 otherwise (and for a very wide row pitch)
int block_side(int m, int nn, int64_t ldmax, int cus) {
  const int64_t blocks = (int64_t)((m + 127) / 128) * ((nn + 127) / 128);
  return (blocks >= 2 * (int64_t)cus && ldmax * 128 * 4 < ((int64_t)1 << 31)) ? 128 : 64;
}
int gemm_parts(int m, int nn, int side) { return ((m + side - 1) / side) * ((nn + side - 1) / side); }

template <int BS, bool VEC, bool DMA, class E>
hipError_t launch_one(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const E& ep, int rungs,
                      hipStream_t st) {
  constexpr int lds = 2 * (BS + BS) * 128;
  if (lds > 48 * 1024)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&gemm_kernel<BS, BS, VEC, DMA, E>), lds); e != hipSuccess)
      return e;
  const dim3 grid((nn + BS - 1) / BS, (m + BS - 1) / BS, rungs);
  hipLaunchKernelGGL((gemm_kernel<BS, BS, VEC, DMA, E>), grid, dim3(256), lds, st, A, lda, B, ldb, m, nn, kk, ep);
  return hipGetLastError();
}

// `rungs` products in one launch, their A operands ep.a_stride apart.  The three operand forms of the main loop: LDS-DMA
// (contraction a multiple of 32), 16-byte buffer loads (a multiple of 4, aligned operands), scalar loads
template <class E>
hipError_t launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const E& ep, int side,
                       int rungs, hipStream_t st) {
  const bool vec = kk % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 &&
                   (ep.a_stride % 4) == 0;
  const bool dma = vec && kk % 32 == 0 && lda * side * 4 < ((int64_t)1 << 31) && ldb * side * 4 < ((int64_t)1 << 31);
  if (side == 128) {
    if (dma) return launch_one<128, true, true>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
    if (vec) return launch_one<128, true, false>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
    return launch_one<128, false, false>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  }
  if (dma) return launch_one<64, true, true>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  if (vec) return launch_one<64, true, false>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  return launch_one<64, false, false>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
}

}  // namespace
}  // namespace solver
}  // namespace lasso
