// float64 M-step: update_dict / update_dict_ridge (dict_learning.py:56-123) for float64 tensors, in Gram form like
// mstep.hip / ridge.hip.  Every product on v_mfma_f64_16x16x4_f64; every value, norm, pivot and comparison an IEEE
// double (sqrt and division correctly rounded, no contraction); no atomics on data and every sum in a fixed order,
// so two calls with the same arguments give the same bits.
//
//   gram_tn_f64_kernel      C = P^T Q over the n rows (A = Z^T Z, B = Z^T X): the double form of gram_tn_kernel
//                           (mstep.hip) with the operand layout of gemm_f64_nt_kernel / syrk_f64_kernel: 64 x 64
//                           blocks, 4 waves x (32 x 32), the rows in chunks of 16 through double-buffered LDS, LDS rows
//                           padded by one double.  sym: blocks bj >= bi only, mirrored.  Large n: blockIdx.z = a slab
//                           of rows, its partial product to scratch, fold_gram_f64_kernel sums the slabs in order.
//   the atom sweep (plain blocked form of the head of mstep.hip; neither the persistent nor the pipelined one):
//     U = B - A D^T          gemm_f64_nt_kernel<sub> (gemm_f64.hip; D [d][k] is its [nn][kk] operand)
//     sweep_block_f64_kernel the 32 atoms of a block in order, one feature per thread: u_j corrected by the atoms
//                           already updated inside the block, clamp, norm, ||u|| < eps flags the atom (its effective
//                           new atom is 0), else d_j = u / ||u||
//     U[j' > block] -= A[j', block] dD[block]     gemm_f64_nt_kernel<sub> again (dD [32][d] is its [kk][nn] operand)
//   fill_degenerate_f64_kernel / zero_columns_f64_kernel: the double forms of their namesakes in mstep.hip.
//   ridge: V = ((A + lam I)^-1 B)^T by a right-looking blocked Cholesky with B^T carried along (ridge.hip's scheme,
//   simple form): per 64-wide block column chol_diag_f64_kernel (the diagonal block, in LDS), chol_panel_f64_kernel
//   (rows below it, B^T included: X L_jj^T = S by substitution, a row per thread), the trailing update
//   S -= P P^T on gemm_f64_nt_kernel<sub>; then the back substitution V L = Y^T, block columns last to first:
//   one gemm_f64_nt_kernel<sub> with the finished columns, ridge_back_f64_kernel inside the block.
//   Not carried over from ridge.hip: the look-ahead factorisation inside the update launch, the panel recomputed per
//   block, the explicit inverses of the diagonal blocks (here: substitution with divisions), the LDS-DMA ring.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>

#include "lasso_kernels.h"
#include "host_util.hpp"

namespace lasso {
namespace f64 {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGB = 64, kGK = 16, kGRS = kGK + 1;
constexpr int kGramSplitMinRows = 2048;     // below: one pass, no partial slabs
constexpr int kGramRowsPerSplit = 1024;     // a slab has at least this many rows

// C[pc x qc] (+ slab blockIdx.z) = P[n_lo .. n_hi)^T Q[n_lo .. n_hi).  mirror (sym, one slab): the kernel writes the
// lower triangle itself -- the elements right of the diagonal, transposed (a diagonal block's own lower half is not
// stored, so C is symmetric bit for bit by construction).
__global__ __launch_bounds__(256) void gram_tn_f64_kernel(const double* __restrict__ P, int64_t ldp, int pc,
                                                          const double* __restrict__ Q, int64_t ldq, int qc, int n,
                                                          double* __restrict__ C, int64_t ldc, int sym, int mirror,
                                                          int rows_per_split, int64_t split_stride) {
  if (sym && blockIdx.x < blockIdx.y) return;
  __shared__ double sp[2][kGB][kGRS], sq[2][kGB][kGRS];
  const int n_lo = blockIdx.z * rows_per_split;
  const int rows = min(rows_per_split, n - n_lo);
  P += (int64_t)n_lo * ldp;
  Q += (int64_t)n_lo * ldq;
  C += (int64_t)blockIdx.z * split_stride;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.y * kGB, j0 = blockIdx.x * kGB;
  const int iw = 32 * (w >> 1), jw = 32 * (w & 1);
  // loaders: column lc of the block, rows lt + 4 h of the chunk; consecutive threads read consecutive addresses
  const int lc = tid & 63, lt = tid >> 6;
  const bool pin = i0 + lc < pc, qin = j0 + lc < qc;
  double rp[4], rq[4];
  auto load = [&](int t0) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int t = t0 + lt + 4 * h;
      rp[h] = (pin && t < rows) ? P[(int64_t)t * ldp + i0 + lc] : 0.0;
      rq[h] = (qin && t < rows) ? Q[(int64_t)t * ldq + j0 + lc] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      sp[buf][lc][lt + 4 * h] = rp[h];
      sq[buf][lc][lt + 4 * h] = rq[h];
    }
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int nc = (rows + kGK - 1) / kGK;
  load(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nc;
    if (more) load((c + 1) * kGK);
#pragma unroll
    for (int ks = 0; ks < kGK / 4; ++ks) {
      const double a0 = sp[buf][iw + l15][4 * ks + q], a1 = sp[buf][iw + 16 + l15][4 * ks + q];
      const double b0 = sq[buf][jw + l15][4 * ks + q], b1 = sq[buf][jw + 16 + l15][4 * ks + q];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);         // (everyone left this buffer at the barrier that ended chunk c - 1)
    __syncthreads();
  }
  const bool diag = sym && blockIdx.x == blockIdx.y;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
    if (row >= pc || col >= qc) continue;
    const double v = acc[e >> 3][(e >> 2) & 1][e & 3];
    if (mirror) {
      if (diag && col < row) continue;
      C[(int64_t)row * ldc + col] = v;
      if (col != row) C[(int64_t)col * ldc + row] = v;
    } else {
      C[(int64_t)row * ldc + col] = v;
    }
  }
}

// C[r][c] = sum of the slabs' [r][c] in slab order; sym: both triangles from the slabs' elements right of the diagonal
// (the only blocks the product wrote)
__global__ __launch_bounds__(256) void fold_gram_f64_kernel(const double* __restrict__ part, int splits,
                                                            int64_t split_stride, int rows, int cols,
                                                            double* __restrict__ C, int64_t ldc, int sym) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * cols) return;
  const int r = (int)(idx / cols), c = (int)(idx % cols);
  const int64_t src = (sym && c < r) ? (int64_t)c * cols + r : (int64_t)r * cols + c;
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += part[(int64_t)s * split_stride + src];
  C[(int64_t)r * ldc + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int kJB = kSweepBlock;
struct SweepF64 {
  const double* A; int64_t lda;          // [k][k]
  double* U; int64_t ldu;                // [k][d]   B - A D^T, kept current for the blocks still to come
  double* D; int64_t ldd;                // [d][k]   the dictionary, updated in place
  double* dD;                            // [kJB][d] new - old atoms of the block (trailing update's operand)
  int* degenerate; int* ndeg;
  int k, d;
  double eps; int positive;
};

// sum over the wave, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// The atoms [j0, j0 + 32) in order; NW waves, thread = feature (d <= 64 NW).  Per atom one barrier: the squared norm
// is the sum of the waves' sums in wave order.  A thread's column of the block's U rows is its own: the atoms go in
// micro-blocks of kMB, whose U values, old atoms and deltas sit in registers; the block's rows below a micro-block
// are corrected in memory behind it (u -= A[b][a] delta_a, a ascending: the order of the one-by-one sweep).
constexpr int kMB = 8;
template <int NW>
__global__ __launch_bounds__(64 * NW) void sweep_block_f64_kernel(const SweepF64 p, int j0) {
  __shared__ double sA[kJB][kJB + 1];
  __shared__ double red[2][NW];
  const int tid = threadIdx.x, f = tid;
  const bool live = f < p.d;
  const int nb = min(kJB, p.k - j0);
  for (int e = tid; e < kJB * kJB; e += 64 * NW) {
    const int a = e / kJB, b = e % kJB;
    sA[a][b] = (a < nb && b < nb) ? p.A[(int64_t)(j0 + a) * p.lda + j0 + b] : 0.0;
  }
  double* const drow = p.D + (int64_t)(live ? f : 0) * p.ldd + j0;        // D[f][j0 ..]
  double* const ucol = p.U + (int64_t)j0 * p.ldu + (live ? f : 0);        // U[j0 ..][f]
  __syncthreads();
  unsigned degmask = 0;
#pragma unroll 1
  for (int s = 0; s < kJB; s += kMB) {
    double u[kMB], dold[kMB], dl[kMB];
#pragma unroll
    for (int i = 0; i < kMB; ++i) {
      const bool on = live && s + i < nb;
      u[i] = on ? ucol[(int64_t)(s + i) * p.ldu] : 0.0;
      dold[i] = on ? drow[s + i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kMB; ++i) {
      const int a = s + i;
      double v = u[i] + sA[a][a] * dold[i];                            // u_j = U_j + A_jj d_j   (:85-86)
      if (p.positive) v = v != v ? v : fmax(v, 0.0);                   // :87-88 (clamp_ keeps a NaN, fmax drops it)
      const double ws = wave_sum(v * v);
      if ((tid & 63) == 0) red[i & 1][tid >> 6] = ws;
      __syncthreads();
      double ss = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) ss += red[i & 1][w];
      const double nrm = sqrt(ss);                                     // :91
      const bool deg = nrm < p.eps;                                    // :92 (uniform over the workgroup)
      const double dnew = deg ? 0.0 : v / nrm;                         // :100
      dl[i] = dnew - dold[i];
      if (deg && a < nb) degmask |= 1u << a;
      dold[i] = dnew;
#pragma unroll
      for (int i2 = i + 1; i2 < kMB; ++i2) u[i2] = u[i2] - sA[s + i2][a] * dl[i];   // :101, inside the micro-block
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < kMB; ++i) {
        if (s + i < nb) drow[s + i] = dold[i];
        p.dD[(int64_t)(s + i) * p.d + f] = s + i < nb ? dl[i] : 0.0;
      }
      for (int b = s + kMB; b < nb; ++b) {
        double x = ucol[(int64_t)b * p.ldu];
#pragma unroll
        for (int i = 0; i < kMB; ++i) x = x - sA[b][s + i] * dl[i];
        ucol[(int64_t)b * p.ldu] = x;
      }
    }
  }
  if (tid < nb) p.degenerate[j0 + tid] = (int)((degmask >> tid) & 1u);
  if (tid == 0) *p.ndeg = (j0 == 0 ? 0 : *p.ndeg) + __popc(degmask);   // (the blocks run one after another)
}

// the i-th flagged atom (atom order) = pool row i, clamped if `positive`, normalised (dict_learning.py:93-96)
__global__ __launch_bounds__(256) void fill_degenerate_f64_kernel(double* __restrict__ D, int64_t ldd, int d, int k,
                                                                  const int* __restrict__ degenerate,
                                                                  const double* __restrict__ pool, int pool_rows,
                                                                  int64_t pool_ld, int positive) {
  __shared__ double sh[256];
  int i = 0;
  for (int j = 0; j < k; ++j) {
    if (!degenerate[j]) continue;                       // uniform over the block
    const double* row = pool + (int64_t)min(i, pool_rows - 1) * pool_ld;
    double part = 0.0;
    for (int dd = threadIdx.x; dd < d; dd += 256) {
      double g = row[dd];
      if (positive) g = fmax(g, 0.0);
      part += g * g;
    }
    sh[threadIdx.x] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    const double nrm = sqrt(sh[0]);
    __syncthreads();
    for (int dd = threadIdx.x; dd < d; dd += 256) {
      double g = row[dd];
      if (positive) g = fmax(g, 0.0);
      D[(int64_t)dd * ldd + j] = g / nrm;
    }
    ++i;
  }
}

// Z[:, j] = 0 for flagged atoms (dict_learning.py:98)
__global__ __launch_bounds__(256) void zero_columns_f64_kernel(double* __restrict__ Z, int64_t ldz, int64_t n, int k,
                                                               const int* __restrict__ degenerate) {
  const int64_t total = n * k;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c = (int)(idx % k);
    if (degenerate[c]) Z[(idx / k) * ldz + c] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int kRB = 64, kRLd = kRB + 1;
constexpr int kRidgeMaxK = 4096;

// S [k + d][k]: rows < k = A + lam I, rows >= k = B^T
__global__ __launch_bounds__(256) void ridge_setup_f64_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                              double* __restrict__ S, int k, int d, double lam,
                                                              int* __restrict__ info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *info = 0;
  const int64_t total = (int64_t)(k + d) * k;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int r = (int)(idx / k), c = (int)(idx % k);
    double v;
    if (r < k) {
      v = A[idx];
      if (r == c) v = v + lam;
    } else {
      v = B[(int64_t)c * d + (r - k)];
    }
    S[idx] = v;
  }
}

// the diagonal block [c0, c0 + nb) of a block column into the LDS tile t; beyond nb the identity
__device__ __forceinline__ void load_diag(const double* __restrict__ S, int64_t ld, int c0, int nb, double (*t)[kRLd],
                                          int nthreads) {
  for (int e = threadIdx.x; e < kRB * kRB; e += nthreads) {
    const int r = e / kRB, c = e % kRB;
    t[r][c] = (r < nb && c < nb) ? S[(int64_t)(c0 + r) * ld + c0 + c] : (r == c ? 1.0 : 0.0);
  }
}

// Cholesky factor of the diagonal block, column by column in LDS; one workgroup.  A pivot that is not positive (or NaN):
// *info = 1 + its index (the first one stays), the factorisation goes on with 1 in its place.
__global__ __launch_bounds__(256) void chol_diag_f64_kernel(double* __restrict__ S, int64_t ld, int c0, int nb,
                                                            int* __restrict__ info) {
  __shared__ double t[kRB][kRLd];
  const int tid = threadIdx.x;
  load_diag(S, ld, c0, nb, t, 256);
  __syncthreads();
  const int r = tid & 63, g = tid >> 6;
  for (int c = 0; c < nb; ++c) {
    const double piv = t[c][c];
    const bool bad = !(piv > 0.0);
    const double s = bad ? 1.0 : sqrt(piv);
    if (bad && tid == 0 && *info == 0) *info = 1 + c0 + c;
    __syncthreads();                                     // everyone has read the pivot
    if (g == 0) {
      if (r == c) t[c][c] = s;
      else if (r > c) t[r][c] = t[r][c] / s;
    }
    __syncthreads();
    if (r > c) {
      const double lrc = t[r][c];
      for (int cc = c + 1 + g; cc <= r; cc += 4) t[r][cc] = t[r][cc] - lrc * t[cc][c];
    }
    __syncthreads();
  }
  for (int e = tid; e < kRB * kRB; e += 256) {
    const int rr = e / kRB, c = e % kRB;
    if (rr < nb && c <= rr) S[(int64_t)(c0 + rr) * ld + c0 + c] = t[rr][c];
  }
}

// rows [r0, r1) of block column c0: X L^T = S by forward substitution, a row per thread (L = the factored diagonal
// block), 16 columns at a time in registers; the columns already solved are read back from the row itself
constexpr int kRS = 16;
__global__ __launch_bounds__(256) void chol_panel_f64_kernel(double* S, int64_t ld, int c0, int nb, int r0, int r1) {
  __shared__ double t[kRB][kRLd];
  load_diag(S, ld, c0, nb, t, 256);
  __syncthreads();
  const int r = r0 + blockIdx.x * 256 + threadIdx.x;
  if (r >= r1) return;
  double* const row = S + (int64_t)r * ld + c0;
#pragma unroll 1
  for (int s = 0; s < nb; s += kRS) {
    double x[kRS];
#pragma unroll
    for (int i = 0; i < kRS; ++i) x[i] = s + i < nb ? row[s + i] : 0.0;
    for (int tt = 0; tt < s; ++tt) {
      const double xp = row[tt];
#pragma unroll
      for (int i = 0; i < kRS; ++i) x[i] = x[i] - xp * t[s + i][tt];
    }
#pragma unroll
    for (int i = 0; i < kRS; ++i) {
      x[i] = x[i] / t[s + i][s + i];
#pragma unroll
      for (int i2 = i + 1; i2 < kRS; ++i2) x[i2] = x[i2] - x[i] * t[s + i2][s + i];
    }
#pragma unroll
    for (int i = 0; i < kRS; ++i)
      if (s + i < nb) row[s + i] = x[i];
  }
}

// columns [c0, c0 + nb) of V (the finished columns to their right already subtracted): X L = Y by backward
// substitution, a row of V per thread, 16 columns at a time from the last to the first
__global__ __launch_bounds__(256) void ridge_back_f64_kernel(double* V, int64_t ldv, int d, const double* S, int64_t ld,
                                                             int c0, int nb) {
  __shared__ double t[kRB][kRLd];
  load_diag(S, ld, c0, nb, t, 256);
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= d) return;
  double* const row = V + (int64_t)r * ldv + c0;
#pragma unroll 1
  for (int s = (nb - 1) / kRS * kRS; s >= 0; s -= kRS) {
    double x[kRS];
#pragma unroll
    for (int i = 0; i < kRS; ++i) x[i] = s + i < nb ? row[s + i] : 0.0;
    for (int tt = s + kRS; tt < nb; ++tt) {
      const double xp = row[tt];
#pragma unroll
      for (int i = 0; i < kRS; ++i) x[i] = x[i] - xp * t[tt][s + i];
    }
#pragma unroll
    for (int i = kRS - 1; i >= 0; --i) {
      x[i] = x[i] / t[s + i][s + i];
#pragma unroll
      for (int i2 = 0; i2 < i; ++i2) x[i2] = x[i2] - x[i] * t[s + i][s + i2];
    }
#pragma unroll
    for (int i = 0; i < kRS; ++i)
      if (s + i < nb) row[s + i] = x[i];
  }
}

}  // namespace

// Row slabs of the two products: none below kGramSplitMinRows rows; else enough to give every CU two workgroups of
// the smaller product, each slab at least kGramRowsPerSplit rows, at most kGramF64MaxSplits.
int gram_splits(int64_t n, int64_t d, int64_t k, int cus) {
  if (n < kGramSplitMinRows) return 1;
  const int64_t kb = (k + kGB - 1) / kGB, db = (d + kGB - 1) / kGB;
  const int64_t blocks = std::max<int64_t>(1, std::min(kb * (kb + 1) / 2, kb * db));
  const int64_t want = (2 * (int64_t)std::max(cus, 1) + blocks - 1) / blocks;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, n / kGramRowsPerSplit, (int64_t)kGramF64MaxSplits}));
}

size_t gram_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  (void)n;
  return (size_t)kGramF64MaxSplits * (align_up((size_t)k * k * 8) + align_up((size_t)k * d * 8));
}

hipError_t launch_gram(const double* Z, int64_t ldz, const double* X, int64_t ldx, int n, int d, int k, double* A,
                       double* B, double* scratch, int splits, hipStream_t st) {
  const unsigned kb = (unsigned)((k + kGB - 1) / kGB), db = (unsigned)((d + kGB - 1) / kGB);
  if (kb > 65535u || db > 65535u) return hipErrorInvalidValue;
  if (!scratch || splits < 1) splits = 1;
  splits = std::min(splits, kGramF64MaxSplits);
  if (splits == 1) {
    hipLaunchKernelGGL(gram_tn_f64_kernel, dim3(kb, kb, 1), dim3(256), 0, st, Z, ldz, k, Z, ldz, k, n, A, (int64_t)k, 1, 1,
                       n, (int64_t)0);
    hipLaunchKernelGGL(gram_tn_f64_kernel, dim3(db, kb, 1), dim3(256), 0, st, Z, ldz, k, X, ldx, d, n, B, (int64_t)d, 0, 0,
                       n, (int64_t)0);
    return hipGetLastError();
  }
  const int rps = ((n + splits - 1) / splits + kGK - 1) / kGK * kGK;
  splits = (n + rps - 1) / rps;                            // (no empty slab)
  const int64_t sa = (int64_t)(align_up((size_t)k * k * 8) / 8), sb = (int64_t)(align_up((size_t)k * d * 8) / 8);
  double* const pa = scratch;
  double* const pb = scratch + (int64_t)kGramF64MaxSplits * sa;
  hipLaunchKernelGGL(gram_tn_f64_kernel, dim3(kb, kb, (unsigned)splits), dim3(256), 0, st, Z, ldz, k, Z, ldz, k, n, pa,
                     (int64_t)k, 1, 0, rps, sa);
  hipLaunchKernelGGL(gram_tn_f64_kernel, dim3(db, kb, (unsigned)splits), dim3(256), 0, st, Z, ldz, k, X, ldx, d, n, pb,
                     (int64_t)d, 0, 0, rps, sb);
  const int64_t ea = (int64_t)k * k, eb = (int64_t)k * d;
  hipLaunchKernelGGL(fold_gram_f64_kernel, dim3((unsigned)((ea + 255) / 256)), dim3(256), 0, st, pa, splits, sa, k, k, A,
                     (int64_t)k, 1);
  hipLaunchKernelGGL(fold_gram_f64_kernel, dim3((unsigned)((eb + 255) / 256)), dim3(256), 0, st, pb, splits, sb, k, d, B,
                     (int64_t)d, 0);
  return hipGetLastError();
}

size_t sweep_count_offset(int64_t d, int64_t k) {
  return align_up((size_t)k * d * 8) + align_up((size_t)kJB * d * 8);
}
size_t sweep_workspace_bytes(int64_t d, int64_t k) { return sweep_count_offset(d, k) + 256; }

hipError_t launch_sweep(const double* A, const double* B, double* D, int64_t ldd, int d, int k, double eps, int positive,
                        int* degenerate, void* workspace, hipStream_t st) {
  if (d > kSweepMaxD || k > kSweepMaxK) return hipErrorInvalidValue;
  char* const base = static_cast<char*>(workspace);
  SweepF64 p;
  p.A = A; p.lda = k;
  p.U = reinterpret_cast<double*>(base); p.ldu = d;
  p.D = D; p.ldd = ldd;
  p.dD = reinterpret_cast<double*>(base + align_up((size_t)k * d * 8));
  p.degenerate = degenerate;
  p.ndeg = reinterpret_cast<int*>(base + sweep_count_offset(d, k));
  p.k = k; p.d = d; p.eps = eps; p.positive = positive;
  // U[j][f] = B[j][f] - sum_i A[j][i] D[f][i]
  if (hipError_t e = launch_gemm_sub(A, k, D, ldd, 0, B, d, p.U, d, k, d, k, st); e != hipSuccess) return e;
  for (int j0 = 0; j0 < k; j0 += kJB) {
    if (d <= 256) hipLaunchKernelGGL(sweep_block_f64_kernel<4>, dim3(1), dim3(256), 0, st, p, j0);
    else if (d <= 512) hipLaunchKernelGGL(sweep_block_f64_kernel<8>, dim3(1), dim3(512), 0, st, p, j0);
    else hipLaunchKernelGGL(sweep_block_f64_kernel<16>, dim3(1), dim3(1024), 0, st, p, j0);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int below = k - j0 - kJB;
    if (below > 0)       // U[j' >= j0 + 32] -= A[j', block] dD
      if (hipError_t e = launch_gemm_sub(A + (int64_t)(j0 + kJB) * k + j0, k, p.dD, d, 1, p.U + (int64_t)(j0 + kJB) * d, d,
                                         p.U + (int64_t)(j0 + kJB) * d, d, below, d, kJB, st);
          e != hipSuccess)
        return e;
  }
  return hipSuccess;
}

hipError_t launch_fill_degenerate(double* D, int64_t ldd, int d, int k, const int* degenerate, const double* pool,
                                  int pool_rows, int64_t pool_ld, int positive, hipStream_t st) {
  hipLaunchKernelGGL(fill_degenerate_f64_kernel, dim3(1), dim3(256), 0, st, D, ldd, d, k, degenerate, pool, pool_rows,
                     pool_ld, positive);
  return hipGetLastError();
}

hipError_t launch_zero_columns(double* Z, int64_t ldz, int64_t n, int k, const int* degenerate, hipStream_t st) {
  const int64_t total = n * k;
  if (total <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(zero_columns_f64_kernel, dim3(grid), dim3(256), 0, st, Z, ldz, n, k, degenerate);
  return hipGetLastError();
}

size_t ridge_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0 || k > kRidgeMaxK) return 0;
  return align_up((size_t)(k + d) * k * 8);
}

hipError_t launch_ridge_solve(const double* A, const double* B, double* V, int64_t ldv, int d, int k, double lam,
                              void* workspace, int* info_dev, hipStream_t st) {
  if (k > kRidgeMaxK) return hipErrorInvalidValue;
  double* const S = static_cast<double*>(workspace);
  const int64_t ld = k;
  const int64_t total = (int64_t)(k + d) * k;
  hipLaunchKernelGGL(ridge_setup_f64_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, st,
                     A, B, S, k, d, lam, info_dev);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  for (int c0 = 0; c0 < k; c0 += kRB) {
    const int nb = std::min(kRB, k - c0), c1 = c0 + nb, below = k + d - c1;
    hipLaunchKernelGGL(chol_diag_f64_kernel, dim3(1), dim3(256), 0, st, S, ld, c0, nb, info_dev);
    hipLaunchKernelGGL(chol_panel_f64_kernel, dim3((unsigned)((below + 255) / 256)), dim3(256), 0, st, S, ld, c0, nb, c1,
                       k + d);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (c1 < k)          // S[c1.., c1..k) -= P P[0 .. k - c1)^T, P = S[c1.., c0..c1)
      if (hipError_t e = launch_gemm_sub(S + (int64_t)c1 * ld + c0, ld, S + (int64_t)c1 * ld + c0, ld, 0,
                                         S + (int64_t)c1 * ld + c1, ld, S + (int64_t)c1 * ld + c1, ld, below, k - c1, nb, st);
          e != hipSuccess)
        return e;
  }
  // rows k.. of S = Y^T = B^T L^-T; V L = Y^T, block columns from the last to the first
  if (hipError_t e = hipMemcpy2DAsync(V, (size_t)ldv * 8, S + (int64_t)k * ld, (size_t)ld * 8, (size_t)k * 8, (size_t)d,
                                      hipMemcpyDeviceToDevice, st);
      e != hipSuccess)
    return e;
  for (int c0 = (k - 1) / kRB * kRB; c0 >= 0; c0 -= kRB) {
    const int nb = std::min(kRB, k - c0), c1 = c0 + nb;
    if (c1 < k)          // V[:, c0..c1) -= V[:, c1..k) L[c1..k, c0..c1)
      if (hipError_t e = launch_gemm_sub(V + c1, ldv, S + (int64_t)c1 * ld + c0, ld, 1, V + c0, ldv, V + c0, ldv, d, nb, k - c1, st);
          e != hipSuccess)
        return e;
    hipLaunchKernelGGL(ridge_back_f64_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, V, ldv, d, S, ld, c0, nb);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace f64
}  // namespace lasso
