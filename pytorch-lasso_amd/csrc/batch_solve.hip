// One dense system per batch entry, A_i x_i = b_i (the reference's lasso/linear/utils.py:43-58 batch_cholesky_solve):
// the drivers behind lasso_batch_chol_solve and lasso_batch_lu_solve, for float and double.
//
// Cholesky route (the hot path).  Only the lower triangle of each A_i is read, in 32 x 32 blocks; a system is padded
// to a multiple of 32 with the identity and a zero right-hand side, so the factorisation carries no bounds test (the
// substitutions stop at row D: 0 * Inf of a non-finite right-hand side must not come back from the padding).  The block scheme
// is the one rows_kernel (iter_ridge.hip) documents, here without the support compaction and with the
// element type a template parameter:
//   diagonal block   one wave, lane r = row r in 32 registers, the pivot row broadcast with v_readlane (no barrier)
//   panel            one thread per row below: X L_JJ^T = A_IJ by substitution in registers, L_JJ broadcast from LDS
//   trailing update  A_IK -= L_IJ L_KJ^T, one 32 x 32 tile per wave at a time on v_mfma_f32_16x16x4_f32 or
//                    v_mfma_f64_16x16x4_f64 (the same A/B lane layout; C/D row 4 q + g in float, q + 4 g in double)
//   L y = b, L^T x = y   the diagonal block in registers, the blocks below (above) one thread per row
// Three tiers:
//   wave     D <= 32: one wave per system, four systems per workgroup, each in its own slice of LDS; the diagonal-block
//            routine and the two in-register substitutions only, ordered by wave-scope fences: no workgroup barrier
//   LDS      one workgroup per system (grid-stride), the packed triangle in LDS with row stride 33 elements, sized by
//            the launch: 4224 B (float) or 8448 B (double) x nb (nb + 1) / 2 -- float to D = 256 (152,064 B), double to
//            D = 160 (15 blocks, 126,720 B; the 21 blocks of D = 192 do not fit a CU's 163,840 B)
//   general  the triangle in a per-workgroup slice of the workspace; the diagonal block and the factored panel of the
//            current block column staged in LDS, so the MFMA operands never come from memory.  A fixed number of
//            workgroups walks the batch: the scratch is a fixed budget, never B D^2.  float to D = 1024, double to
//            D = 512 (a 1024-row double panel would be 270 KB).
// A pivot that is not positive (or NaN) is replaced by 1 and recorded per system as 1 + its index by a plain vector
// store: no data-dependent loop, and bad data cannot fault a kernel.  fold_kernel (one workgroup) leaves one record: the
// lowest bad system and its minor.  No atomics: two calls with the same arguments give the same bits.
//
// LU route (the cold path: what the reference does with the WHOLE batch once one factorisation failed).  One workgroup
// per system on a copy of the full matrix in its slice of the workspace: right-looking LU with partial pivoting, one
// column at a time -- the pivot is the first entry of largest magnitude (wave shuffles, then four candidates through
// LDS), the rows are exchanged, then each row below is scaled and updated by one wave.  The right-hand side rides along
// as one more column, which is the forward substitution; the back substitution follows.  A pivot that is exactly zero
// is recorded and replaced by 1; a NaN pivot is no error and leaves that system's solution NaN.
//
// The device routines repeat those of rows_kernel (folding both onto one header is a follow-up that
// has to keep rows_kernel's register budget).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"

namespace lasso {
namespace batch_solve {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kNB = 32;                       // block side of the packed triangle
constexpr int kRS = 33;                       // row stride of a block in LDS (elements)
constexpr int kWaveCap = 32;                  // largest D of the wave tier
constexpr int kLoads = 8;                     // loads of the triangle a thread keeps in flight
constexpr size_t kScratchBudget = (size_t)256 << 20;   // general tier and LU: bytes of per-workgroup matrices, at most
constexpr int kScratchWgs = 256;              // ... and workgroups, at most

template <class T> struct Caps;
template <> struct Caps<float> { static constexpr int lds = 256, general = 1024; };
template <> struct Caps<double> { static constexpr int lds = 160, general = 512; };

// the one record the host reads
struct Record {
  int bad_system, bad_minor;                  // lowest system with a flag (-1: none) and 1 + the index of its pivot
};

__host__ __device__ __forceinline__ int tri(int b) { return (b * (b + 1)) >> 1; }

__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
__device__ __forceinline__ double lane_bcast(double v, int src_lane) {
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float r_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double r_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float r_sqrt(float a) { return __fsqrt_rn(a); }
__device__ __forceinline__ double r_sqrt(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ float r_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double r_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float r_abs(float a) { return fabsf(a); }
__device__ __forceinline__ double r_abs(double a) { return fabs(a); }
__device__ __forceinline__ float r_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double r_fma(double a, double b, double c) { return fma(a, b, c); }

template <class T> struct Mma;
template <> struct Mma<float> {
  using Acc = f32x4;
  static __device__ __forceinline__ Acc run(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int q, int g) { return 4 * q + g; }
};
template <> struct Mma<double> {
  using Acc = f64x4;
  static __device__ __forceinline__ Acc run(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int q, int g) { return q + 4 * g; }
};

// orders the LDS traffic of ONE wave (what its lanes wrote is what its lanes read next); no workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <class T>
struct Args {
  const T* A; int64_t batch_stride, lda;      // [nbatch][d][d], lower triangle (Cholesky) or all of it (LU)
  const T* B; int64_t ldb;                    // [nbatch][d]
  T* X; int64_t ldx;                          // out [nbatch][d]
  int* piv;                                   // out [nbatch]: 0, or 1 + index of the first bad pivot
  T* scratch; int64_t scratch_stride;         // general tier, LU: one matrix per workgroup (elements)
  int nbatch, d, nb;                          // nb = ceil(d / 32)
};

// ---- the three routines on a diagonal block, run by one whole wave (lanes 32..63 repeat rows 0..31, store nothing) ----
// DJ: the block in LDS (row stride kRS), factored in place, zeros above the diagonal; G: a second copy to keep (row
// stride kNB) or null; base: index of the block's first pivot; bad: 1 + index of the first bad pivot so far
template <class T>
__device__ __forceinline__ void factor_diag(T* DJ, T* G, int lane, int base, int& bad) {
  int r = lane & 31;
  asm volatile("" : "+v"(r));                 // (keeps the 32 lane predicates below out of scalar registers across the row loop)
  T av[kNB];
#pragma unroll
  for (int c = 0; c < kNB; ++c) av[c] = DJ[r * kRS + c];
#pragma unroll
  for (int cc = 0; cc < kNB; ++cc) {
    const T pv = av[cc];
    const T piv = lane_bcast(pv, cc);
    T root = r_sqrt(piv);
    if (!(piv > (T)0)) {
      if (!bad) bad = base + cc + 1;
      root = (T)1;
    }
    const T l = r == cc ? root : r_div(pv, root);
    av[cc] = l;
#pragma unroll
    for (int c2 = cc + 1; c2 < kNB; ++c2) {
      av[c2] = r_fma(-l, lane_bcast(l, c2), av[c2]);
      if ((c2 & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (bounds the broadcasts in flight: each holds a scalar register)
    }
  }
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < kNB; ++c) {
      const T v = c <= r ? av[c] : (T)0;
      DJ[r * kRS + c] = v;
      if (G) G[r * kNB + c] = v;
    }
  }
}

// L_JJ y = b on b[0..31]; LJ: the factored block, row stride RS
template <class T>
__device__ __forceinline__ void fwd_diag(const T* LJ, int RS, T* b, int lane) {
  int r = lane & 31;
  asm volatile("" : "+v"(r));
  T lr[kNB];
#pragma unroll
  for (int c = 0; c < kNB; ++c) lr[c] = LJ[r * RS + c];
  T bv = b[r];
#pragma unroll
  for (int c = 0; c < kNB; ++c) {
    const T yc = r_div(lane_bcast(bv, c), lane_bcast(lr[c], c));
    if (r == c) bv = yc;
    else if (r > c) bv = r_fma(-lr[c], yc, bv);
    if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  }
  if (lane < 32) b[r] = bv;
}

// L_JJ^T x = y on b[0..31]; nv: rows of the block that belong to the system -- the padding rows behind them hold
// 0 * (whatever the right-hand side held) after fwd_diag and are kept out of the rows that count
template <class T>
__device__ __forceinline__ void bwd_diag(const T* LJ, int RS, T* b, int lane, int nv) {
  int r = lane & 31;
  asm volatile("" : "+v"(r));
  asm volatile("" : "+v"(nv));                // (as r: 32 uniform predicates would each take a scalar register)
  T lc[kNB];                                  // column r of L_JJ
#pragma unroll
  for (int c = 0; c < kNB; ++c) lc[c] = LJ[c * RS + r];
  T bv = b[r];
#pragma unroll
  for (int c = kNB - 1; c >= 0; --c) {
    const T zc = r_div(lane_bcast(bv, c), lane_bcast(lc[c], c));
    if (r == c) bv = zc;
    else if (r < c && c < nv) bv = r_fma(-lc[c], zc, bv);
    if ((c & 7) == 0) __builtin_amdgcn_sched_barrier(0);
  }
  if (lane < 32) b[r] = bv;
}

// element (i, j), j <= i, of the padded system: the identity beyond d; the strict upper triangle is never read
template <class T>
__device__ __forceinline__ T lower_elem(const T* A, int64_t lda, int d, int i, int j) {
  T v = i == j ? (T)1 : (T)0;
  if (i < d && j <= i) v = A[(int64_t)i * lda + j];
  return v;
}

// ---- wave tier: d <= 32, one wave per system ----
template <class T>
__global__ __launch_bounds__(256) void wave_kernel(Args<T> a) {
  __shared__ T sm[4][kNB * kRS + kNB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T* const L = sm[w];
  T* const b = L + kNB * kRS;
  for (int64_t sys = (int64_t)blockIdx.x * 4 + w; sys < a.nbatch; sys += (int64_t)gridDim.x * 4) {
    const T* const A = a.A + sys * a.batch_stride;
    for (int e = lane; e < kNB * kNB; e += 64) {
      const int r = e >> 5, c = e & 31;
      L[r * kRS + c] = c <= r ? lower_elem(A, a.lda, a.d, r, c) : (T)0;
    }
    if (lane < kNB) b[lane] = lane < a.d ? a.B[sys * a.ldb + lane] : (T)0;
    wave_sync();
    int bad = 0;
    factor_diag<T>(L, nullptr, lane, 0, bad);
    wave_sync();
    fwd_diag<T>(L, kRS, b, lane);
    wave_sync();
    bwd_diag<T>(L, kRS, b, lane, a.d);
    wave_sync();
    if (lane < a.d) a.X[sys * a.ldx + lane] = b[lane];
    if (lane == 0) a.piv[sys] = bad;
    wave_sync();                              // (L and b are rewritten by the next system)
  }
}

// ---- LDS and general tiers: one workgroup per system (grid-stride) ----
template <class T, bool LDS>
__global__ __launch_bounds__(256) void block_kernel(Args<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RS = LDS ? kRS : kNB;         // row stride of a block of M
  constexpr int BS = kNB * RS;                // elements per block of M
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int nbr = a.nb, sp = nbr * kNB;
  T* const smem_t = reinterpret_cast<T*>(smem);
  T* cur = smem_t;
  T* M;                                       // the packed lower triangle: block (bi, bj) at tri(bi) + bj
  T* P = nullptr;                             // general tier: the factored panel, row i at P + i * kRS
  T* D = nullptr;                             // general tier: the diagonal block (row stride kRS)
  if constexpr (LDS) {
    M = cur;
    cur += (size_t)tri(nbr) * BS;
  } else {
    M = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    D = cur;
    cur += kNB * kRS;
    P = cur;
    cur += (size_t)sp * kRS;
  }
  T* const b = cur;                           // right-hand side, then the solution [sp]

  for (int64_t sys = blockIdx.x; sys < a.nbatch; sys += gridDim.x) {
    const T* const A = a.A + sys * a.batch_stride;
    for (int i = tid; i < sp; i += 256) b[i] = i < a.d ? a.B[sys * a.ldb + i] : (T)0;
    // ---- the lower triangle, the identity on the padding ----
    // (a block row at a time, eight loads of a thread in flight before the first store: one workgroup owns the CU on
    // the larger systems, so nothing else hides the latency of this read)
    for (int bi = 0; bi < nbr; ++bi) {
      T* const brow = M + (size_t)tri(bi) * BS;
      const int cnt = (bi + 1) * kNB * kNB;   // elements of blocks (bi, 0 .. bi)
      for (int e0 = tid; e0 < cnt; e0 += 256 * kLoads) {
        T v[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
          const int e = e0 + 256 * u;
          const int i = bi * kNB + ((e >> 5) & 31), j = (e >> 10) * kNB + (e & 31);
          v[u] = (e < cnt && j <= i) ? lower_elem(A, a.lda, a.d, i, j) : (T)0;
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
          const int e = e0 + 256 * u;
          if (e < cnt) brow[(size_t)(e >> 10) * BS + ((e >> 5) & 31) * RS + (e & 31)] = v[u];
        }
      }
    }
    __syncthreads();

    int bad = 0;                              // (wave 0) 1 + index of the first bad pivot
    // ---- blocked right-looking Cholesky ----
    for (int J = 0; J < nbr; ++J) {
      T* const MJJ = M + (size_t)(tri(J) + J) * BS;
      T* DJ = MJJ;                            // the diagonal block, row stride kRS
      if constexpr (!LDS) {
        for (int e = tid; e < kNB * kNB; e += 256) D[(e >> 5) * kRS + (e & 31)] = MJJ[e];
        DJ = D;
        __syncthreads();
      }
      if (w == 0) factor_diag<T>(DJ, LDS ? (T*)nullptr : MJJ, lane, J * kNB, bad);
      __syncthreads();
      // panel: row i of the blocks below, X L_JJ^T = A.  (L_JJ through a vector offset: 528 uniform addresses would
      // each take a scalar register across the loop)
      int djo = (int)(DJ - smem_t);
      asm volatile("" : "+v"(djo));
      const T* const dj = smem_t + djo;
      for (int i = (J + 1) * kNB + tid; i < sp; i += 256) {
        T* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * RS;
        T x[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) x[c] = src[c];
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          T acc = x[c];
#pragma unroll
          for (int j = 0; j < c; ++j) acc = r_fma(-x[j], dj[c * kRS + j], acc);
          x[c] = r_div(acc, dj[c * kRS + c]);
        }
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          src[c] = x[c];
          if constexpr (!LDS) P[i * kRS + c] = x[c];
        }
      }
      __syncthreads();
      // trailing update: tile (I, K), J < K <= I, one wave per tile
      const int nrem = nbr - J - 1;
      const int ntiles = tri(nrem);
      for (int t = w; t < ntiles; t += 4) {
        int ii = 0;
        while (tri(ii + 1) <= t) ++ii;
        const int I = J + 1 + ii, K = J + 1 + (t - tri(ii));
        T av[2][8], bv[2][8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int k0 = 0; k0 < 8; ++k0) {
            const int ri = I * kNB + 16 * h + l15, rk = K * kNB + 16 * h + l15, c = 4 * k0 + q;
            if constexpr (LDS) {
              av[h][k0] = M[(size_t)(tri(I) + J) * BS + (ri & 31) * RS + c];
              bv[h][k0] = M[(size_t)(tri(K) + J) * BS + (rk & 31) * RS + c];
            } else {
              av[h][k0] = P[ri * kRS + c];
              bv[h][k0] = P[rk * kRS + c];
            }
          }
        T* const dst = M + (size_t)(tri(I) + K) * BS;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) {
            typename Mma<T>::Acc acc = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
            for (int k0 = 0; k0 < 8; ++k0) acc = Mma<T>::run(av[ti][k0], bv[tj][k0], acc);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              T* const p = dst + (16 * ti + Mma<T>::row(q, g)) * RS + 16 * tj + l15;
              *p = r_sub(*p, acc[g]);
            }
          }
      }
      __syncthreads();
    }

    // ---- L y = b ----
    for (int J = 0; J < nbr; ++J) {
      const T* const MJJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) fwd_diag<T>(MJJ, RS, b + J * kNB, lane);
      __syncthreads();
      for (int i = (J + 1) * kNB + tid; i < a.d; i += 256) {    // (the padding rows stay 0: a non-finite b must not reach them)
        const T* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * RS;
        T acc = b[i];
#pragma unroll 8
        for (int c = 0; c < kNB; ++c) acc = r_fma(-src[c], b[J * kNB + c], acc);
        b[i] = acc;
      }
      __syncthreads();
    }
    // ---- L^T x = y ----
    for (int J = nbr - 1; J >= 0; --J) {
      const T* const MJJ = M + (size_t)(tri(J) + J) * BS;
      const int nv = min(kNB, a.d - J * kNB);   // (below 32 in the last block only)
      if (w == 0) bwd_diag<T>(MJJ, RS, b + J * kNB, lane, nv);
      __syncthreads();
      for (int i = tid; i < J * kNB; i += 256) {
        const T* const src = M + (size_t)(tri(J) + (i >> 5)) * BS + (i & 31);
        T acc = b[i];
#pragma unroll 8
        for (int c = 0; c < nv; ++c) acc = r_fma(-src[c * RS], b[J * kNB + c], acc);
        b[i] = acc;
      }
      __syncthreads();
    }
    for (int i = tid; i < a.d; i += 256) a.X[sys * a.ldx + i] = b[i];
    if (tid == 0) a.piv[sys] = bad;
    __syncthreads();                          // (b and M are rewritten by the next system)
  }
}

// ---- LU with partial pivoting: one workgroup per system (grid-stride), the matrix in its slice of the workspace ----
template <class T>
__global__ __launch_bounds__(256) void lu_kernel(Args<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ T cand_v[4];
  __shared__ int cand_i[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int d = a.d;
  T* const b = reinterpret_cast<T*>(smem);    // right-hand side [d]
  T* const x = b + d;                         // solution [d]
  T* const M = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;   // [d][d]
  for (int64_t sys = blockIdx.x; sys < a.nbatch; sys += gridDim.x) {
    const T* const A = a.A + sys * a.batch_stride;
    for (int i = w; i < d; i += 4)
      for (int j = lane; j < d; j += 64) M[(int64_t)i * d + j] = A[(int64_t)i * a.lda + j];
    for (int i = tid; i < d; i += 256) b[i] = a.B[sys * a.ldb + i];
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < d; ++k) {
      // the first entry of largest magnitude in column k, rows k .. d - 1 (a NaN is never larger)
      T best = (T)-1;
      int at = d;
      for (int i = k + tid; i < d; i += 256) {
        const T v = r_abs(M[(int64_t)i * d + k]);
        if (v > best) { best = v; at = i; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const T ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(at, off);
        if (ov > best || (ov == best && oi < at)) { best = ov; at = oi; }
      }
      if (lane == 0) { cand_v[w] = best; cand_i[w] = at; }
      __syncthreads();
      best = cand_v[0];
      at = cand_i[0];
#pragma unroll
      for (int c = 1; c < 4; ++c) {
        const T ov = cand_v[c];
        const int oi = cand_i[c];
        if (ov > best || (ov == best && oi < at)) { best = ov; at = oi; }
      }
      const int p = at < d ? at : k;          // (a column of NaN: no exchange, the NaN pivot stays)
      if (p != k) {
        for (int j = k + tid; j < d; j += 256) {
          const T u = M[(int64_t)k * d + j], v = M[(int64_t)p * d + j];
          M[(int64_t)k * d + j] = v;
          M[(int64_t)p * d + j] = u;
        }
        if (tid == 0) { const T u = b[k]; b[k] = b[p]; b[p] = u; }
      }
      __syncthreads();
      T pv = M[(int64_t)k * d + k];
      if (pv == (T)0) {
        if (!bad) bad = k + 1;
        pv = (T)1;
      }
      const T bk = b[k];
      // row i below: l = M[i][k] / pivot, row i -= l * row k, b[i] -= l * b[k]; one wave per row
      for (int i = k + 1 + w; i < d; i += 4) {
        const T l = r_div(M[(int64_t)i * d + k], pv);
        for (int j = k + 1 + lane; j < d; j += 64)
          M[(int64_t)i * d + j] = r_fma(-l, M[(int64_t)k * d + j], M[(int64_t)i * d + j]);
        if (lane == 0) b[i] = r_fma(-l, bk, b[i]);
      }
      __syncthreads();
    }
    // U x = y, a column at a time
    for (int k = d - 1; k >= 0; --k) {
      T pv = M[(int64_t)k * d + k];
      if (pv == (T)0) pv = (T)1;
      const T xk = r_div(b[k], pv);
      if (tid == 0) x[k] = xk;
      for (int i = tid; i < k; i += 256) b[i] = r_fma(-M[(int64_t)i * d + k], xk, b[i]);
      __syncthreads();
    }
    for (int i = tid; i < d; i += 256) a.X[sys * a.ldx + i] = x[i];
    if (tid == 0) a.piv[sys] = bad;
    __syncthreads();                          // (b, x and M are rewritten by the next system)
  }
}

// the one record: the lowest system with a flag and its minor
__global__ __launch_bounds__(256) void fold_kernel(const int* __restrict__ piv, int n, Record* __restrict__ rec) {
  __shared__ int low[256];
  int first = n;
  for (int i = threadIdx.x; i < n; i += 256)
    if (piv[i] != 0 && i < first) first = i;
  low[threadIdx.x] = first;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) low[threadIdx.x] = min(low[threadIdx.x], low[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec->bad_system = low[0] < n ? low[0] : -1;
    rec->bad_minor = low[0] < n ? piv[low[0]] : 0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
template <class T> size_t tri_bytes(int nb) { return (size_t)nb * (nb + 1) / 2 * kNB * kNB * sizeof(T); }   // one scratch triangle

template <class T> size_t block_lds_bytes(bool lds_tier, int nb) {
  const size_t sp = (size_t)nb * kNB;
  const size_t mat = lds_tier ? (size_t)nb * (nb + 1) / 2 * kNB * kRS : sp * kRS + kNB * kRS;
  return (mat + sp) * sizeof(T);
}

template <class T> int tier_of(int d) {
  return d <= kWaveCap ? LASSO_BATCH_TIER_WAVE : d <= Caps<T>::lds ? LASSO_BATCH_TIER_LDS : LASSO_BATCH_TIER_GENERAL;
}

// workgroups that share the scratch budget, `each` bytes apiece
int budget_wgs(int64_t nbatch, size_t each) {
  const int64_t fit = (int64_t)(kScratchBudget / each);
  return (int)std::max<int64_t>(1, std::min<int64_t>({nbatch, fit, (int64_t)kScratchWgs}));
}

template <class T> int chol_wgs(int64_t nbatch, int d) {
  if (tier_of<T>(d) != LASSO_BATCH_TIER_GENERAL) return 0;
  return budget_wgs(nbatch, tri_bytes<T>((d + kNB - 1) / kNB));
}

template <class T> int lu_wgs(int64_t nbatch, int d) { return budget_wgs(nbatch, (size_t)d * d * sizeof(T)); }

struct Space {
  int* piv;
  Record* rec;
  void* scratch;
  size_t bytes;
};

template <class T> Space carve(void* base, int64_t nbatch, int d) {
  Space s;
  Arena a(base);
  s.piv = a.take<int>((size_t)nbatch * 4);
  s.rec = a.take<Record>(sizeof(Record));
  const size_t chol = (size_t)chol_wgs<T>(nbatch, d) * tri_bytes<T>((d + kNB - 1) / kNB);
  const size_t lu = (size_t)lu_wgs<T>(nbatch, d) * d * d * sizeof(T);
  s.scratch = a.take<char>(std::max(chol, lu));
  s.bytes = a.bytes();
  return s;
}

template <class T>
int finish(const Space& ws, int nbatch, lasso_batch_solve_result* res, hipStream_t st) {
  hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(256), 0, st, (const int*)ws.piv, nbatch, ws.rec);
  LASSO_HIP_TRY(hipGetLastError());
  Record h;
  if (int s = read_back(&h, ws.rec, sizeof(Record), st)) return s;
  res->bad_system = h.bad_system;
  res->bad_minor = h.bad_minor;
  return LASSO_OK;
}

template <class T>
Args<T> make_args(const void* a, int64_t batch_stride, int64_t lda, const void* b, int64_t ldb, void* x, int64_t ldx,
                  int64_t nbatch, int64_t d, const Space& ws) {
  Args<T> r = {};
  r.A = (const T*)a; r.batch_stride = batch_stride; r.lda = lda;
  r.B = (const T*)b; r.ldb = ldb;
  r.X = (T*)x; r.ldx = ldx;
  r.piv = ws.piv; r.scratch = (T*)ws.scratch;
  r.nbatch = (int)nbatch; r.d = (int)d; r.nb = ((int)d + kNB - 1) / kNB;
  return r;
}

template <class T>
int chol_t(const void* a, int64_t batch_stride, int64_t lda, const void* b, int64_t ldb, void* x, int64_t ldx, int64_t nbatch,
           int64_t d, lasso_batch_solve_result* res, void* workspace, hipStream_t st) {
  const Space ws = carve<T>(workspace, nbatch, (int)d);
  Args<T> r = make_args<T>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, ws);
  const int tier = tier_of<T>((int)d);
  res->tier = tier;
  if (tier == LASSO_BATCH_TIER_WAVE) {
    const int grid = (int)std::min<int64_t>((nbatch + 3) / 4, 1 << 20);
    hipLaunchKernelGGL(wave_kernel<T>, dim3(grid), dim3(256), 0, st, r);
  } else if (tier == LASSO_BATCH_TIER_LDS) {
    const size_t lds = block_lds_bytes<T>(true, r.nb);
    if (lds > 48 * 1024)
      if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&block_kernel<T, true>), lds); e != hipSuccess)
        return fail(LASSO_ERR_HIP, "batch solve: %s", hipGetErrorString(e));
    const int grid = (int)std::min<int64_t>(nbatch, 1 << 20);
    hipLaunchKernelGGL((block_kernel<T, true>), dim3(grid), dim3(256), lds, st, r);
  } else {
    const size_t lds = block_lds_bytes<T>(false, r.nb);
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&block_kernel<T, false>), lds); e != hipSuccess)
      return fail(LASSO_ERR_HIP, "batch solve: %s", hipGetErrorString(e));
    r.scratch_stride = (int64_t)(tri_bytes<T>(r.nb) / sizeof(T));
    hipLaunchKernelGGL((block_kernel<T, false>), dim3(chol_wgs<T>(nbatch, (int)d)), dim3(256), lds, st, r);
  }
  LASSO_HIP_TRY(hipGetLastError());
  return finish<T>(ws, (int)nbatch, res, st);
}

template <class T>
int lu_t(const void* a, int64_t batch_stride, int64_t lda, const void* b, int64_t ldb, void* x, int64_t ldx, int64_t nbatch,
         int64_t d, lasso_batch_solve_result* res, void* workspace, hipStream_t st) {
  const Space ws = carve<T>(workspace, nbatch, (int)d);
  Args<T> r = make_args<T>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, ws);
  res->tier = tier_of<T>((int)d);
  r.scratch_stride = d * d;
  const size_t lds = (size_t)2 * d * sizeof(T);
  hipLaunchKernelGGL(lu_kernel<T>, dim3(lu_wgs<T>(nbatch, (int)d)), dim3(256), lds, st, r);
  LASSO_HIP_TRY(hipGetLastError());
  return finish<T>(ws, (int)nbatch, res, st);
}

}  // namespace

int tier_cap(int dtype, int tier) {
  if (tier == LASSO_BATCH_TIER_WAVE) return kWaveCap;
  if (tier == LASSO_BATCH_TIER_LDS) return dtype == LASSO_F64 ? Caps<double>::lds : Caps<float>::lds;
  if (tier == LASSO_BATCH_TIER_GENERAL) return dtype == LASSO_F64 ? Caps<double>::general : Caps<float>::general;
  return 0;
}

int general_workgroups(int64_t nbatch, int64_t d, int dtype) {
  return dtype == LASSO_F64 ? chol_wgs<double>(nbatch, (int)d) : chol_wgs<float>(nbatch, (int)d);
}

size_t workspace_bytes(int64_t nbatch, int64_t d, int dtype) {
  return (dtype == LASSO_F64 ? carve<double>(nullptr, nbatch, (int)d) : carve<float>(nullptr, nbatch, (int)d)).bytes + 256;
}

int chol(const void* a, int64_t batch_stride, int64_t lda, const void* b, int64_t ldb, void* x, int64_t ldx, int64_t nbatch,
         int64_t d, int dtype, lasso_batch_solve_result* res, void* workspace, hipStream_t st) {
  return dtype == LASSO_F64 ? chol_t<double>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, res, workspace, st)
                            : chol_t<float>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, res, workspace, st);
}

int lu(const void* a, int64_t batch_stride, int64_t lda, const void* b, int64_t ldb, void* x, int64_t ldx, int64_t nbatch,
       int64_t d, int dtype, lasso_batch_solve_result* res, void* workspace, hipStream_t st) {
  return dtype == LASSO_F64 ? lu_t<double>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, res, workspace, st)
                            : lu_t<float>(a, batch_stride, lda, b, ldb, x, ldx, nbatch, d, res, workspace, st);
}

}  // namespace batch_solve
}  // namespace lasso
