// Main loop of the fp32 MFMA NT GEMM (gemm.hip), shared with the kernels that give it other epilogues (gpsr.hip):
// the BM x BN block of A B^T at (i0, j0) accumulated into 16x16 MFMA fragments.  See gemm.hip for the staging scheme.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lasso {
namespace gemm_detail {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz_off(int row, int chunk) {   // bytes inside a [rows][128 B] tile
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// rows of `src` [rows x kk] (ld) starting at r0, columns k0 + 4*chunk .. +3 -> v (zero outside)
template <bool VEC>
__device__ __forceinline__ f32x4 load_chunk4(const float* __restrict__ src, int64_t ld, int row, int rows,
                                             int kcol, int kk) {
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (row < rows) {
    const float* p = src + (int64_t)row * ld + kcol;
    if constexpr (VEC) {
      if (kcol < kk) v = *(const f32x4*)p;          // kk % 4 == 0: the chunk is all in or all out
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (kcol + e < kk) v[e] = p[e];
    }
  }
  return v;
}

// one LDS-DMA instruction: 64 lanes x 16 bytes from src + voff (per lane) to the 1 KiB at LDS address `lds_addr`
// (lane-linear), no registers in between (see tile_device.hpp: dma_step)
__device__ __forceinline__ void gemm_dma_piece(const float* src, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:0\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(src), "s"(lds_addr)
      : "memory");
}

// acc[mi][nj][rg]: row (BM/2) wr + 16 mi + 4 q + rg, column (BN/2) wc + 16 nj + l15 of the block (w = wave, wr = w >> 1,
// wc = w & 1, l15 = lane & 15, q = lane >> 4).  smem: 2 (BM + BN) 128 bytes of dynamic LDS, free again on return (the last
// chunk ends with a barrier).  DMA as for gemm_nt_kernel.
template <int BM, int BN, bool VEC, bool DMA>
__device__ __forceinline__ void gemm_nt_accumulate(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                   int64_t ldb, int m, int nn, int kk, int i0, int j0, char* smem,
                                                   f32x4 (&acc)[BM / 32][BN / 32]) {
  constexpr int MI = BM / 32, NJ = BN / 32;          // 16x16 blocks per wave: MI x NJ
  constexpr int PA = BM / 32, PB = BN / 32;          // staged 16-byte chunks per thread and operand
  char* const sa = smem;                             // [2][BM * 128]
  char* const sb = smem + 2 * BM * 128;              // [2][BN * 128]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int l15 = lane & 15, q = lane >> 4;
  // staging map: thread -> chunk (tid & 7) of rows (tid >> 3) + 32 h
  const int srow = tid >> 3, sch = tid & 7;
  f32x4 ga[PA], gb[PB];
  // (VEC: 16-byte buffer loads from descriptors of the block's rows of A and B, the offset out of range beyond the rows /
  // beyond kk -- reads 0 --, offsets opaque: no branch per chunk, the batch leaves as a batch; the launcher checks
  // ld BM 4 < 2^31)
  const int rows_a = min(BM, m - i0), rows_b = min(BN, nn - j0);
  auto rows_rsrc = [&](const float* base, int64_t ld, int r0, int rows) {
    const int64_t bytes = (int64_t)rows * ld * 4;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (int64_t)r0 * ld), 0,
                                             (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff), 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t ars = rows_rsrc(A, lda, i0, rows_a), brs = rows_rsrc(B, ldb, j0, rows_b);
  auto fetch = [&](int k0) {
    if constexpr (VEC) {
      const int kc = k0 + 4 * sch;
#pragma unroll
      for (int h = 0; h < PA; ++h) {
        unsigned o = (srow + 32 * h < rows_a && kc < kk) ? (unsigned)((srow + 32 * h) * (int)lda + kc) * 4u : 0xfffffff0u;
        asm volatile("" : "+v"(o));
        ga[h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, o, 0, 0));
      }
#pragma unroll
      for (int h = 0; h < PB; ++h) {
        unsigned o = (srow + 32 * h < rows_b && kc < kk) ? (unsigned)((srow + 32 * h) * (int)ldb + kc) * 4u : 0xfffffff0u;
        asm volatile("" : "+v"(o));
        gb[h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brs, o, 0, 0));
      }
    } else {
#pragma unroll
      for (int h = 0; h < PA; ++h) ga[h] = load_chunk4<VEC>(A, lda, i0 + srow + 32 * h, m, k0 + 4 * sch, kk);
#pragma unroll
      for (int h = 0; h < PB; ++h) gb[h] = load_chunk4<VEC>(B, ldb, j0 + srow + 32 * h, nn, k0 + 4 * sch, kk);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int h = 0; h < PA; ++h) *(f32x4*)(sa + buf * BM * 128 + swz_off(srow + 32 * h, sch)) = ga[h];
#pragma unroll
    for (int h = 0; h < PB; ++h) *(f32x4*)(sb + buf * BN * 128 + swz_off(srow + 32 * h, sch)) = gb[h];
  };
  // DMA: per-lane byte offsets inside the block's rows (row clamped to the last valid one: its results are dropped)
  unsigned va[PA], vb[PB];
  const int wdma = __builtin_amdgcn_readfirstlane(w);
  if constexpr (DMA) {
#pragma unroll
    for (int h = 0; h < PA; ++h) {
      const int r = srow + 32 * h, c = sch ^ ((r >> 1) & 7);
      va[h] = (unsigned)((int64_t)min(r, m - 1 - i0) * lda * 4 + c * 16);
    }
#pragma unroll
    for (int h = 0; h < PB; ++h) {
      const int r = srow + 32 * h, c = sch ^ ((r >> 1) & 7);
      vb[h] = (unsigned)((int64_t)min(r, nn - 1 - j0) * ldb * 4 + c * 16);
    }
  }
  auto dma = [&](int k0, int buf) {
    const float* const abase = A + (int64_t)i0 * lda + k0;
    const float* const bbase = B + (int64_t)j0 * ldb + k0;
    const unsigned la = (unsigned)(uintptr_t)(sa + buf * BM * 128) + (unsigned)(8 * wdma) * 128u;
    const unsigned lb = (unsigned)(uintptr_t)(sb + buf * BN * 128) + (unsigned)(8 * wdma) * 128u;
#pragma unroll
    for (int h = 0; h < PA; ++h) gemm_dma_piece(abase, va[h], la + 32 * 128 * h);
#pragma unroll
    for (int h = 0; h < PB; ++h) gemm_dma_piece(bbase, vb[h], lb + 32 * 128 * h);
  };
  if constexpr (DMA) {
    dma(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): this wave's pieces are in LDS
  } else {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < kk; k0 += 32) {
    const bool more = k0 + 32 < kk;
    if (more) {
      if constexpr (DMA) dma(k0 + 32, buf ^ 1);
      else fetch(k0 + 32);
    }
    const char* const ta = sa + buf * BM * 128;
    const char* const tb = sb + buf * BN * 128;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      f32x4 a[MI], b[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = *(const f32x4*)(ta + swz_off((BM / 2) * wr + 16 * mi + l15, 4 * ss + q));
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) b[nj] = *(const f32x4*)(tb + swz_off((BN / 2) * wc + 16 * nj + l15, 4 * ss + q));
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[nj][j], acc[mi][nj], 0, 0, 0);
    }
    if constexpr (DMA) {
      __builtin_amdgcn_s_waitcnt(0x0F70);    // vmcnt(0)
    } else {
      if (more) stash(buf ^ 1);
    }
    __syncthreads();
    buf ^= 1;
  }
}

}  // namespace gemm_detail
}  // namespace lasso
