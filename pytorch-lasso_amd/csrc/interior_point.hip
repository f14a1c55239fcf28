// The interior-point lasso solver (Schmidt 2005, section 2.3; Chen, Donoho, Saunders 2001; the reference's
// lasso/linear/solvers/interior_point.py) on the HIP path: the driver behind lasso_interior_point_solve and
// lasso_interior_point_rows.  The code is split z = z+ - z-, z+, z- >= 0, with dual slacks s+, s- and the dual variable
// lambda [n][d]; the reference carries the dictionary twice, W_pn = [W, -W].  Here the halves share one W:
//   lambda W_pn = [t, -t]             t = lambda W, one product (the halves are exact negations of it)
//   z W_pn^T    = (z+ - z-) W^T       one product on the difference of the halves
//   M           = I + W_pn diag(d) W_pn^T = I + W diag(c) W^T,  c = d+ + d-,  d = z / s
// Per iteration every row solves M dlambda = rhs, a d x d system (the reference builds an [n, 2k, d] intermediate and an
// [n, d, d] batch for it; nothing here is n d^2).
//
// newton_rows_kernel is the hot path: one workgroup of 256 threads per row.  It forms the lower triangle of M in 32 x 32
// blocks on v_mfma_f32_16x16x4_f32 (instances for at most 2, 4 and 8 block rows): wave w owns the 16 x 16 tile (w >> 1, w & 1) of EVERY block and keeps all of them
// (36 x 4 accumulator registers at d = 256) in registers across one single pass over k, so W is read once per row.  W
// goes through LDS in chunks of 32 atoms (row stride 36 floats: the 64 lanes of an operand read hit 64 banks), double
// buffered with the next chunk's loads in flight; the A operand is scaled by c as it is read.  The staging area is the
// space the triangle takes afterwards: the blocks go to LDS (block (I, J) at I (I + 1) / 2 + J, row stride 33), the unit
// diagonal is added -- the padding up to a multiple of 32 is the identity with a zero right-hand side -- and the
// blocked right-looking Cholesky and the two substitutions of iter_ridge.hip follow for the one right-hand side.  The
// kernel has no data-dependent loop or index and cannot fault on bad data; a pivot that is not positive (or NaN) is not
// repaired: its root is NaN and so is that row's result.
//
// The four batch products of an iteration (lambda W, (z+ - z-) W^T, the rhs product, dlambda W) are the GEMM of
// solver_common.hpp with its store epilogue.  The element-wise steps are two passes: pre_kernel (residuals,
// the generalised inverse, c and the operand of the rhs product) and update_kernel, one workgroup per row (directions,
// ratio minima, the damped steps, clamps, mu and the row's three ratios).  stat_kernel, one workgroup, folds the rows'
// ratios in double in a fixed order into the iteration's record: no float atomics, two solves of the same arguments are
// bitwise equal.  The host reads one record per iteration, and with tol <= 0 (the stop test cannot pass) none at all:
// the records stay on the device and are fetched in batches for the trace.
#include "solver_common.hpp"

namespace lasso {
namespace interior_point {
namespace {

using namespace solver;

constexpr int kNB = 32;                       // block side of the packed triangle
constexpr int kRS = 33;                       // row stride of a block in LDS (floats)
constexpr int kMaxNB = 8;                     // block rows at d = 256
constexpr int kKC = 32;                       // atoms per staged chunk of W
constexpr int kKS = 36;                       // row stride of a staged chunk (floats)
constexpr int kHist = 1024;                   // iteration records the workspace holds
constexpr int kRowStat = 8;                   // doubles per row: prim, dual, gap ratios, sum z, sum lambda^2

// one iteration's record (device; the host reads it once per iteration, or in batches with tol <= 0)
struct Rec {
  double prim, dual, gap, obj;
  int stop, pad;
};
// the start's verdict
struct Start {
  double obj0, bad;
};

__device__ __forceinline__ int tri(int b) { return (b * (b + 1)) >> 1; }

__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// torch's min / max / clamp hand a NaN on; fminf / fmaxf drop it
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float clamp0(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float ginv(float s, float eps) { return fabsf(s) < eps ? 0.0f : __fdiv_rn(1.0f, s); }

// min over the block's 256 threads in a fixed order, NaN handed on; red [4]
__device__ __forceinline__ float block_nan_min(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nan_min(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return nan_min(nan_min(red[0], red[1]), nan_min(red[2], red[3]));
}

struct RowsArgs {
  const float* W; int64_t ldw;                // the dictionary [d][k]
  const float* Cw; int64_t ldc;               // per-row weights c [n][k]
  const float* B1; int64_t ldb1;              // right-hand side [n][d] ...
  const float* B2; int64_t ldb2;              // ... minus this one (nullable)
  float* Y; int64_t ldy;                      // out [n][d]
  int n, d, k, nb;                            // nb = ceil(d / 32)
  int vec;                                    // W rows may be read as float4
};

// One workgroup per row (grid-stride): y = (I + W diag(c) W^T)^-1 (b1 - b2).  NBT = the most block rows the instance
// holds in registers (2, 4 or 8): at d <= 64 the 3 x 4 accumulators leave room for three workgroups per CU, whose
// serial chains (the diagonal blocks, the substitutions) then hide behind each other.
template <int NBT>
__global__ __launch_bounds__(256) void newton_rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BS = kNB * kRS;               // floats per block of M
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int ti = w >> 1, tj = w & 1;          // this wave's 16 x 16 tile of every block
  const int nb = a.nb, sp = nb * kNB;
  float* const smem_f = reinterpret_cast<float*>(smem);
  float* const b = smem_f;                    // right-hand side, then the solution [256]
  float* const cs = smem_f + kMaxNB * kNB;    // the chunk's weights [2][kKC]
  float* const M = cs + 2 * kKC;              // the packed lower triangle; before it, the staged chunks [2][sp][kKS]
  const int nch = (a.k + kKC - 1) / kKC;
  const int srow = tid >> 3, scol = (tid & 7) * 4;   // staging: thread t moves 4 atoms of row srow + 32 p

  for (int row = blockIdx.x; row < a.n; row += gridDim.x) {
    const float* const crow = a.Cw + (int64_t)row * a.ldc;
    f32x4 acc[NBT * (NBT + 1) / 2];
#pragma unroll
    for (int t = 0; t < NBT * (NBT + 1) / 2; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float4 stage[NBT];
    float cstage = 0.0f;
    auto fetch = [&](int ch) {                // chunk ch of W (zero beyond d and k) and of c into registers
      const int l0 = ch * kKC + scol;
#pragma unroll
      for (int p = 0; p < NBT; ++p) {
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        const int r = srow + 32 * p;
        if (p < nb && r < a.d) {
          const float* const src = a.W + (int64_t)r * a.ldw + l0;
          if (a.vec) {
            if (l0 < a.k) v = *reinterpret_cast<const float4*>(src);
          } else {
            if (l0 < a.k) v.x = src[0];
            if (l0 + 1 < a.k) v.y = src[1];
            if (l0 + 2 < a.k) v.z = src[2];
            if (l0 + 3 < a.k) v.w = src[3];
          }
        }
        stage[p] = v;
      }
      if (tid < kKC) cstage = ch * kKC + tid < a.k ? crow[ch * kKC + tid] : 0.0f;
    };
    auto put = [&](int buf) {
      float* const dst = M + (size_t)buf * sp * kKS;
#pragma unroll
      for (int p = 0; p < NBT; ++p)
        if (p < nb) *reinterpret_cast<float4*>(dst + (srow + 32 * p) * kKS + scol) = stage[p];
      if (tid < kKC) cs[buf * kKC + tid] = cstage;
    };
    __syncthreads();                          // (the previous row's solution and triangle have been read)
    fetch(0);
    put(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      const int buf = ch & 1;
      if (ch + 1 < nch) fetch(ch + 1);
      const float* const src = M + (size_t)buf * sp * kKS;
#pragma unroll 2
      for (int kk = 0; kk < kKC / 4; ++kk) {
        const float cv = cs[buf * kKC + 4 * kk + q];
        float av[NBT], bv[NBT];
#pragma unroll
        for (int I = 0; I < NBT; ++I)
          if (I < nb) {
            av[I] = __fmul_rn(src[(I * kNB + 16 * ti + l15) * kKS + 4 * kk + q], cv);
            bv[I] = src[(I * kNB + 16 * tj + l15) * kKS + 4 * kk + q];
          }
#pragma unroll
        for (int I = 0; I < NBT; ++I)
          if (I < nb) {
#pragma unroll
            for (int J = 0; J <= I; ++J)
              acc[I * (I + 1) / 2 + J] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[I], bv[J], acc[I * (I + 1) / 2 + J], 0, 0, 0);
          }
      }
      if (ch + 1 < nch) put(buf ^ 1);
      __syncthreads();
    }
    // ---- the triangle to LDS (over the staging area: every wave is past its last operand read), + I ----
#pragma unroll
    for (int I = 0; I < NBT; ++I)
      if (I < nb) {
#pragma unroll
        for (int J = 0; J <= I; ++J) {
          float* const dst = M + (size_t)(tri(I) + J) * BS;
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int r = 16 * ti + 4 * q + rg, c = 16 * tj + l15;
            float v = acc[I * (I + 1) / 2 + J][rg];
            if (I == J && r == c) v = __fadd_rn(v, 1.0f);
            dst[r * kRS + c] = v;
          }
        }
      }
    for (int i = tid; i < sp; i += 256) {
      float v = 0.0f;
      if (i < a.d) {
        v = a.B1[(int64_t)row * a.ldb1 + i];
        if (a.B2) v = __fsub_rn(v, a.B2[(int64_t)row * a.ldb2 + i]);
      }
      b[i] = v;
    }
    __syncthreads();

    // ---- blocked right-looking Cholesky (iter_ridge.hip's LDS tier) ----
    for (int J = 0; J < nb; ++J) {
      float* const DJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) {
        int r = lane & 31;                    // (lanes 32..63 repeat rows 0..31 and store nothing)
        asm volatile("" : "+v"(r));         // (keeps the 32 lane predicates below out of scalar registers across the row loop)
        float av[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) av[c] = DJ[r * kRS + c];
#pragma unroll
        for (int cc = 0; cc < kNB; ++cc) {
          const float pv = av[cc];
          const float piv = lane_bcast(pv, cc);
          const float root = piv > 0.0f ? __fsqrt_rn(piv) : __builtin_nanf("");
          const float l = r == cc ? root : __fdiv_rn(pv, root);
          av[cc] = l;
#pragma unroll
          for (int c2 = cc + 1; c2 < kNB; ++c2) {
            av[c2] = fmaf(-l, lane_bcast(l, c2), av[c2]);
            if ((c2 & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (bounds the broadcasts in flight: each holds a scalar register)
          }
        }
        if (lane < 32) {
#pragma unroll
          for (int c = 0; c < kNB; ++c) DJ[r * kRS + c] = c <= r ? av[c] : 0.0f;
        }
      }
      __syncthreads();
      // panel: row i of the blocks below, X L_JJ^T = A.  (L_JJ through a vector offset: 528 uniform addresses would
      // each take a scalar register across the loop)
      int djo = (int)(DJ - smem_f);
      asm volatile("" : "+v"(djo));
      const float* const dj = smem_f + djo;
      for (int i = (J + 1) * kNB + tid; i < sp; i += 256) {
        float* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * kRS;
        float x[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) x[c] = src[c];
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          float s = x[c];
#pragma unroll
          for (int j = 0; j < c; ++j) s = fmaf(-x[j], dj[c * kRS + j], s);
          x[c] = __fdiv_rn(s, dj[c * kRS + c]);
        }
#pragma unroll
        for (int c = 0; c < kNB; ++c) src[c] = x[c];
      }
      __syncthreads();
      // trailing update: tile (I, K), J < K <= I, one wave per tile
      const int nrem = nb - J - 1;
      const int ntiles = tri(nrem);
      for (int t = w; t < ntiles; t += 4) {
        int ii = 0;
        while (tri(ii + 1) <= t) ++ii;        // (t < 28: at most seven steps, bounded by the shape alone)
        const int I = J + 1 + ii, K = J + 1 + (t - tri(ii));
        float av[2][8], bv[2][8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int k0 = 0; k0 < 8; ++k0) {
            const int rr = 16 * h + l15, c = 4 * k0 + q;
            av[h][k0] = M[(size_t)(tri(I) + J) * BS + rr * kRS + c];
            bv[h][k0] = M[(size_t)(tri(K) + J) * BS + rr * kRS + c];
          }
        float* const dst = M + (size_t)(tri(I) + K) * BS;
#pragma unroll
        for (int ai = 0; ai < 2; ++ai)
#pragma unroll
          for (int aj = 0; aj < 2; ++aj) {
            f32x4 u = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k0 = 0; k0 < 8; ++k0) u = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ai][k0], bv[aj][k0], u, 0, 0, 0);
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              float* const p = dst + (16 * ai + 4 * q + rg) * kRS + 16 * aj + l15;
              *p = __fsub_rn(*p, u[rg]);
            }
          }
      }
      __syncthreads();
    }

    // ---- L y = b ----
    for (int J = 0; J < nb; ++J) {
      const float* const MJJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) {
        int r = lane & 31;
        asm volatile("" : "+v"(r));
        float lr[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) lr[c] = MJJ[r * kRS + c];
        float bvv = b[J * kNB + r];
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          const float yc = __fdiv_rn(lane_bcast(bvv, c), lane_bcast(lr[c], c));
          if (r == c) bvv = yc;
          else if (r > c) bvv = fmaf(-lr[c], yc, bvv);
          if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 32) b[J * kNB + r] = bvv;
      }
      __syncthreads();
      for (int i = (J + 1) * kNB + tid; i < sp; i += 256) {
        const float* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * kRS;
        float s = b[i];
#pragma unroll 8
        for (int c = 0; c < kNB; ++c) s = fmaf(-src[c], b[J * kNB + c], s);
        b[i] = s;
      }
      __syncthreads();
    }
    // ---- L^T x = y ----
    for (int J = nb - 1; J >= 0; --J) {
      const float* const MJJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) {
        int r = lane & 31;
        asm volatile("" : "+v"(r));
        float lc[kNB];                        // column r of L_JJ
#pragma unroll
        for (int c = 0; c < kNB; ++c) lc[c] = MJJ[c * kRS + r];
        float bvv = b[J * kNB + r];
#pragma unroll
        for (int c = kNB - 1; c >= 0; --c) {
          const float zc = __fdiv_rn(lane_bcast(bvv, c), lane_bcast(lc[c], c));
          if (r == c) bvv = zc;
          else if (r < c) bvv = fmaf(-lc[c], zc, bvv);
          if ((c & 7) == 0) __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 32) b[J * kNB + r] = bvv;
      }
      __syncthreads();
      for (int i = tid; i < J * kNB; i += 256) {
        const float* const src = M + (size_t)(tri(J) + (i >> 5)) * BS + (i & 31);
        float s = b[i];
#pragma unroll 8
        for (int c = 0; c < kNB; ++c) s = fmaf(-src[c * kRS], b[J * kNB + c], s);
        b[i] = s;
      }
      __syncthreads();
    }
    for (int i = tid; i < a.d; i += 256) a.Y[(int64_t)row * a.ldy + i] = b[i];
  }
}

// ---- the start: interior_point.py:38-69 ------------------------------------------------------------------------------
// z+ = relu(z0) + 0.1, z- = relu(-z0) + 0.1 (Z [n][2k]), sgn = sign(z0) (= sign(z0+) - sign(z0-)); partials {bad entries}
__global__ __launch_bounds__(256) void start_z_kernel(const float* __restrict__ Z0, int64_t ld0, float* __restrict__ Z,
                                                      float* __restrict__ SGN, int n, int k, double* __restrict__ part) {
  __shared__ double red[32];
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / k, j = i % k;
    const float v = Z0[r * ld0 + j];
    const float zp = __fadd_rn(v > 0.0f ? v : (v != v ? v : 0.0f), 0.1f);
    const float zn = __fadd_rn(v < 0.0f ? -v : (v != v ? v : 0.0f), 0.1f);
    Z[r * 2 * k + j] = zp;
    Z[r * 2 * k + k + j] = zn;
    SGN[i] = v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v);     // (0 and NaN as they are)
    s[0] += (zp > 0.0f && zn > 0.0f) ? 0.0 : 1.0;
  }
  block_fold<1, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// one workgroup per row: omega = 1.1 max |y W|, lambda = alpha y / omega, mu = barrier_init
__global__ __launch_bounds__(256) void start_lambda_kernel(const float* __restrict__ YW, const float* __restrict__ Y,
                                                           float* __restrict__ LAM, float* __restrict__ MU, int n, int d, int k,
                                                           float alpha, float mu0) {
  __shared__ float red[4];
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    float m = 0.0f;
    for (int j = threadIdx.x; j < k; j += 256) m = nan_max(m, fabsf(YW[(int64_t)row * k + j]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = nan_max(m, __shfl_xor(m, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
    const float omega = __fmul_rn(1.1f, m);
    for (int i = threadIdx.x; i < d; i += 256)
      LAM[(int64_t)row * d + i] = __fdiv_rn(__fmul_rn(alpha, Y[(int64_t)row * d + i]), omega);
    if (threadIdx.x == 0) MU[row] = mu0;
  }
}

// s+ = alpha - t, s- = alpha + t, zd = z+ - z-; partials {bad entries, sum z, sum lambda^2}
__global__ __launch_bounds__(256) void start_s_kernel(const float* __restrict__ T, const float* __restrict__ Z, float* __restrict__ S,
                                                      float* __restrict__ ZD, const float* __restrict__ LAM, int n, int d, int k,
                                                      float alpha, double* __restrict__ part) {
  __shared__ double red[32];
  double s[3] = {0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  const int64_t nk = (int64_t)n * k, nd = (int64_t)n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk + nd; i += (int64_t)gridDim.x * 256) {
    if (i < nk) {
      const int64_t r = i / k, j = i % k;
      const float t = T[i];
      const float sp = __fsub_rn(alpha, t), sn = __fadd_rn(alpha, t);
      const float zp = Z[r * 2 * k + j], zn = Z[r * 2 * k + k + j];
      S[r * 2 * k + j] = sp;
      S[r * 2 * k + k + j] = sn;
      ZD[i] = __fsub_rn(zp, zn);
      s[0] += (sp > 0.0f && sn > 0.0f && -alpha < t && t < alpha) ? 0.0 : 1.0;
      s[1] += (double)zp + (double)zn;
    } else {
      const double l = (double)LAM[i - nk];
      s[2] += l * l;
    }
  }
  block_fold<3, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

__global__ __launch_bounds__(256) void start_fold_kernel(const double* __restrict__ part_z, int nb_z, const double* __restrict__ part_s,
                                                         int nb_s, double alpha, Start* __restrict__ out) {
  __shared__ double red[256], a[kPart], b[kPart];
  fold_partials(part_z, nb_z, 1, 0, red, a);
  fold_partials(part_s, nb_s, 3, 0, red, b);
  if (threadIdx.x == 0) {
    out->bad = a[0] + b[0];
    out->obj0 = alpha * b[1] + 0.5 * b[2];
  }
}

// ---- an iteration's element-wise passes ------------------------------------------------------------------------------
struct Half { float ra, rc, sinv, dd; };
// the KKT residuals and the scaling of one entry of a half (sgn = -1 for the positive half: ra = sgn t - s + alpha)
__device__ __forceinline__ Half half_of(float tsgn, float z, float s, float mu, float alpha, float eps) {
  Half h;
  h.ra = __fadd_rn(__fsub_rn(tsgn, s), alpha);
  h.rc = __fsub_rn(mu, __fmul_rn(z, s));
  h.sinv = ginv(s, eps);
  h.dd = __fmul_rn(h.sinv, z);
  return h;
}

// over [n,k]: c = d+ + d-, g = (s_inv rc - d ra)+ - (s_inv rc - d ra)-;  over [n,d]: rb = x - (z+ - z-) W^T - lambda
__global__ __launch_bounds__(256) void pre_kernel(const float* __restrict__ T, const float* __restrict__ Z, const float* __restrict__ S,
                                                  const float* __restrict__ MU, float* __restrict__ Cw, float* __restrict__ G,
                                                  const float* __restrict__ X, int64_t ldx, const float* __restrict__ ZW,
                                                  const float* __restrict__ LAM, float* __restrict__ RB, int n, int d, int k,
                                                  float alpha, float eps) {
  const int64_t nk = (int64_t)n * k, nd = (int64_t)n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk + nd; i += (int64_t)gridDim.x * 256) {
    if (i < nk) {
      const int64_t r = i / k, j = i % k;
      const float t = T[i], mu = MU[r];
      const Half p = half_of(-t, Z[r * 2 * k + j], S[r * 2 * k + j], mu, alpha, eps);
      const Half m = half_of(t, Z[r * 2 * k + k + j], S[r * 2 * k + k + j], mu, alpha, eps);
      Cw[i] = __fadd_rn(p.dd, m.dd);
      G[i] = __fsub_rn(__fsub_rn(__fmul_rn(p.sinv, p.rc), __fmul_rn(p.dd, p.ra)),
                       __fsub_rn(__fmul_rn(m.sinv, m.rc), __fmul_rn(m.dd, m.ra)));
    } else {
      const int64_t e = i - nk, r = e / d, j = e % d;
      RB[e] = __fsub_rn(__fsub_rn(X[r * ldx + j], ZW[e]), LAM[e]);
    }
  }
}

// One workgroup per row: d_s, d_z, the ratio minima, the damped steps on z, s, lambda, mu, the clamps, zd = z+ - z- and
// the row's figures {prim, dual, gap ratios, sum z, sum lambda^2} (ra and rb of BEFORE the update, z, s, lambda of after)
__global__ __launch_bounds__(256) void update_kernel(const float* __restrict__ T, const float* __restrict__ U, float* __restrict__ Z,
                                                     float* __restrict__ S, float* __restrict__ MU, float* __restrict__ LAM,
                                                     const float* __restrict__ DL, const float* __restrict__ RB, float* __restrict__ ZD,
                                                     double* __restrict__ rowstat, int n, int d, int k, float alpha, float eps) {
  __shared__ float redf[4];
  __shared__ double red[32], tot[8];
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    float* const z = Z + (int64_t)row * 2 * k;
    float* const s = S + (int64_t)row * 2 * k;
    const float* const t = T + (int64_t)row * k;
    const float* const u = U + (int64_t)row * k;
    const float mu = MU[row];
    float bz = INFINITY, bs = INFINITY;
    for (int j = threadIdx.x; j < k; j += 256) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float tv = h ? t[j] : -t[j], uv = h ? u[j] : -u[j];
        const float zv = z[h * k + j], sv = s[h * k + j];
        const Half e = half_of(tv, zv, sv, mu, alpha, eps);
        const float ds = __fadd_rn(e.ra, uv);                      // ra - dlambda W_pn
        const float dz = __fmul_rn(e.sinv, __fsub_rn(e.rc, __fmul_rn(zv, ds)));
        bz = nan_min(bz, dz >= 0.0f ? INFINITY : __fdiv_rn(-zv, dz));
        bs = nan_min(bs, ds >= 0.0f ? INFINITY : __fdiv_rn(-sv, ds));
      }
    }
    bz = block_nan_min(bz, redf);
    bs = block_nan_min(bs, redf);
    bz = bz > 1.0f ? 1.0f : bz;
    bs = bs > 1.0f ? 1.0f : bs;
    const float stz = __fmul_rn(0.99f, bz), sts = __fmul_rn(0.99f, bs);
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // sum z^2, sum z s, sum ra^2, sum z, (then) sum lambda^2 and sum rb^2
    for (int j = threadIdx.x; j < k; j += 256) {
      float zn[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float tv = h ? t[j] : -t[j], uv = h ? u[j] : -u[j];
        const float zv = z[h * k + j], sv = s[h * k + j];
        const Half e = half_of(tv, zv, sv, mu, alpha, eps);
        const float ds = __fadd_rn(e.ra, uv);
        const float dz = __fmul_rn(e.sinv, __fsub_rn(e.rc, __fmul_rn(zv, ds)));
        const float z1 = clamp0(__fadd_rn(zv, __fmul_rn(stz, dz)));
        const float s1 = clamp0(__fadd_rn(sv, __fmul_rn(sts, ds)));
        z[h * k + j] = z1;
        s[h * k + j] = s1;
        zn[h] = z1;
        a[0] += (double)z1 * (double)z1;
        a[1] += (double)z1 * (double)s1;
        a[2] += (double)e.ra * (double)e.ra;
        a[3] += (double)z1;
      }
      ZD[(int64_t)row * k + j] = __fsub_rn(zn[0], zn[1]);
    }
    double c[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < d; i += 256) {
      const int64_t o = (int64_t)row * d + i;
      const float l1 = __fadd_rn(LAM[o], __fmul_rn(sts, DL[o]));
      LAM[o] = l1;
      c[0] += (double)l1 * (double)l1;
      const double rb = (double)RB[o];
      c[1] += rb * rb;
    }
    double sums[6] = {a[0], a[1], a[2], a[3], c[0], c[1]};
    float nomax[1] = {0.0f};
    block_fold<6, 0>(sums, nomax, red, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
      const float mn = nan_min(bz, bs);
      MU[row] = __fmul_rn(mu, __fsub_rn(1.0f, mn > 0.99f ? 0.99f : mn));
      const double zn2 = sqrt(tot[0]), ln2 = sqrt(tot[4]);
      double* const o = rowstat + (int64_t)row * kRowStat;
      o[0] = sqrt(tot[5]) / (1.0 + zn2);
      o[1] = sqrt(tot[2]) / (1.0 + ln2);
      o[2] = tot[1] / (1.0 + zn2 * ln2);
      o[3] = tot[3];
      o[4] = tot[4];
    }
    __syncthreads();                          // (tot and red are rewritten by the next row)
  }
}

// one workgroup: the means over rows of the three ratios, obj = alpha sum z + 0.5 sum lambda^2, and the stop verdict
__global__ __launch_bounds__(256) void stat_kernel(const double* __restrict__ rowstat, int n, double alpha, double tol,
                                                   Rec* __restrict__ rec) {
  __shared__ double red[256];
  double out[5];
  for (int i = 0; i < 5; ++i) {
    double a = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) a += rowstat[(int64_t)r * kRowStat + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    out[i] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec->prim = out[0] / n;
    rec->dual = out[1] / n;
    rec->gap = out[2] / n;
    rec->obj = alpha * out[3] + 0.5 * out[4];
    rec->stop = (rec->prim < tol && rec->dual < tol && rec->gap < tol) ? 1 : 0;   // (a NaN mean never stops the loop)
    rec->pad = 0;
  }
}

// z = z+ - z- to the caller's tensor
__global__ __launch_bounds__(256) void copy_out_kernel(const float* __restrict__ ZD, float* __restrict__ out, int64_t ldo, int n, int k) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    out[(i / k) * ldo + (i % k)] = ZD[i];
}

// ---- launchers -------------------------------------------------------------------------------------------------------
size_t rows_lds_bytes(int nb) {
  const size_t triangle = (size_t)nb * (nb + 1) / 2 * kNB * kRS * 4;
  const size_t staging = (size_t)2 * nb * kNB * kKS * 4;
  return ((size_t)kMaxNB * kNB + 2 * kKC) * 4 + std::max(triangle, staging);
}

template <int NBT>
hipError_t launch_rows_as(const RowsArgs& a, int per_cu, hipStream_t st) {
  const size_t lds = rows_lds_bytes(a.nb);
  if (lds > 48 * 1024)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&newton_rows_kernel<NBT>), lds); e != hipSuccess) return e;
  const int grid = (int)std::min<int64_t>(a.n, (int64_t)per_cu * device_cus());
  hipLaunchKernelGGL(newton_rows_kernel<NBT>, dim3(grid), dim3(256), lds, st, a);
  return hipGetLastError();
}

// workgroups per CU of the grid: twice what the instance's registers and LDS let reside (3, 2, 1)
hipError_t launch_rows(RowsArgs a, hipStream_t st) {
  a.nb = (a.d + kNB - 1) / kNB;
  a.vec = (a.k % 4 == 0 && a.ldw % 4 == 0 && ((uintptr_t)a.W & 15) == 0) ? 1 : 0;
  if (a.nb <= 2) return launch_rows_as<2>(a, 6, st);
  if (a.nb <= 4) return launch_rows_as<4>(a, 4, st);
  return launch_rows_as<8>(a, 2, st);
}

int row_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(n, 4 * kEwBlocks)); }

struct Space {
  float *Wt, *Z, *S, *T, *U, *ZD, *Cw, *G, *LAM, *DL, *RB, *Q, *ZW, *MU;
  double *rowstat, *part_a, *part_b;
  Rec* rec;
  Start* start;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4;
  w.Wt = a.take((size_t)k * d * 4);
  w.Z = a.take(2 * nk);
  w.S = a.take(2 * nk);
  w.T = a.take(nk);
  w.U = a.take(nk);
  w.ZD = a.take(nk);
  w.Cw = a.take(nk);
  w.G = a.take(nk);
  w.LAM = a.take(nd);
  w.DL = a.take(nd);
  w.RB = a.take(nd);
  w.Q = a.take(nd);
  w.ZW = a.take(nd);
  w.MU = a.take((size_t)n * 4);
  w.rowstat = a.take<double>((size_t)n * kRowStat * 8);
  w.part_a = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.part_b = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.rec = a.take<Rec>(sizeof(Rec) * kHist);
  w.start = a.take<Start>(sizeof(Start));
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int rows(const float* w, int64_t ldw, const float* c, int64_t ldc, const float* b, int64_t ldb, float* y, int64_t ldy, int64_t n,
         int64_t d, int64_t k, hipStream_t st) {
  RowsArgs a = {};
  a.W = w; a.ldw = ldw; a.Cw = c; a.ldc = ldc; a.B1 = b; a.ldb1 = ldb; a.Y = y; a.ldy = ldy;
  a.n = (int)n; a.d = (int)d; a.k = (int)k;
  LASSO_HIP_TRY(launch_rows(a, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha_d, const lasso_interior_point_options& o,
          lasso_interior_point_result* res, void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const Space ws = carve(workspace, n, d, k);
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  // LASSO_FORCE_BLOCKS_128 (tests): 128 x 128 blocks below the size at which block_side takes them
  const bool force128 = (o.reserved & LASSO_FORCE_BLOCKS_128) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // products [n,d]
  const int64_t nk = (int64_t)n * k, nd = (int64_t)n * d;
  const int gk = ew_grid(nk), gkd = ew_grid(nk + nd), gr = row_grid(n);
  const float alpha = (float)alpha_d, eps = (float)o.eps;
  lasso_interior_point_trace* const tr = res->trace;

  // [n][d] x W -> [n][k] (on W^T [k][d]) and [n][k] x W^T -> [n][d]
  auto times_w = [&](const float* A, float* out) -> hipError_t {
    return launch_gemm(A, d, ws.Wt, d, n, k, d, StoreEpi{out, k, 0}, side_k, 1, st);
  };
  auto times_wt = [&](const float* A, float* out) -> hipError_t {
    return launch_gemm(A, k, w, ldw, n, d, k, StoreEpi{out, d, 0}, side_d, 1, st);
  };

  // ---- the start ----
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));
  hipLaunchKernelGGL(start_z_kernel, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, ws.G, n, k, ws.part_a);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(times_wt(ws.G, ws.Q));                      // y = sign(z0) W^T
  LASSO_HIP_TRY(times_w(ws.Q, ws.T));                       // y W
  hipLaunchKernelGGL(start_lambda_kernel, dim3(gr), dim3(256), 0, st, ws.T, ws.Q, ws.LAM, ws.MU, n, d, k, alpha, (float)o.barrier_init);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(times_w(ws.LAM, ws.T));                     // t = lambda W
  hipLaunchKernelGGL(start_s_kernel, dim3(gkd), dim3(256), 0, st, ws.T, ws.Z, ws.S, ws.ZD, ws.LAM, n, d, k, alpha, ws.part_b);
  hipLaunchKernelGGL(start_fold_kernel, dim3(1), dim3(256), 0, st, ws.part_a, gk, ws.part_b, gkd, alpha_d, ws.start);
  LASSO_HIP_TRY(hipGetLastError());
  Start hs;
  if (int s = read_back(&hs, ws.start, sizeof(Start), st)) return s;   // the one read of the start's flag
  res->obj0 = hs.obj0;
  if (!(hs.bad == 0.0)) {
    res->status = LASSO_INTERIOR_POINT_BAD_START;
    return fail(LASSO_ERR_BAD_ARG, "interior point: the start is not interior (z > 0, s > 0, -alpha < lambda W < alpha)");
  }

  // ---- the iterations ----
  const bool can_stop = o.tol > 0.0;
  std::vector<Rec> hist(kHist);
  int n_iter = 0, flushed = 0, status = LASSO_INTERIOR_POINT_MAXITER;
  auto flush = [&]() -> int {                 // the records [flushed, n_iter) to the trace
    if (tr && n_iter > flushed) {
      if (int s = read_back(hist.data(), ws.rec, sizeof(Rec) * (size_t)(n_iter - flushed), st)) return s;
      for (int i = flushed; i < n_iter && i < tr->capacity; ++i) {
        tr->obj[i] = hist[i - flushed].obj;
        tr->prim_feas[i] = hist[i - flushed].prim;
        tr->dual_feas[i] = hist[i - flushed].dual;
        tr->gap[i] = hist[i - flushed].gap;
      }
    }
    flushed = n_iter;
    return LASSO_OK;
  };
  while (n_iter < o.maxiter) {
    if (n_iter > 0) LASSO_HIP_TRY(times_w(ws.LAM, ws.T));
    LASSO_HIP_TRY(times_wt(ws.ZD, ws.ZW));
    hipLaunchKernelGGL(pre_kernel, dim3(gkd), dim3(256), 0, st, ws.T, ws.Z, ws.S, ws.MU, ws.Cw, ws.G, x, ldx, ws.ZW, ws.LAM, ws.RB,
                       n, d, k, alpha, eps);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(times_wt(ws.G, ws.Q));
    RowsArgs a = {};
    a.W = w; a.ldw = ldw; a.Cw = ws.Cw; a.ldc = k; a.B1 = ws.RB; a.ldb1 = d; a.B2 = ws.Q; a.ldb2 = d; a.Y = ws.DL; a.ldy = d;
    a.n = n; a.d = d; a.k = k;
    LASSO_HIP_TRY(launch_rows(a, st));
    LASSO_HIP_TRY(times_w(ws.DL, ws.U));
    hipLaunchKernelGGL(update_kernel, dim3(gr), dim3(256), 0, st, ws.T, ws.U, ws.Z, ws.S, ws.MU, ws.LAM, ws.DL, ws.RB, ws.ZD,
                       ws.rowstat, n, d, k, alpha, eps);
    Rec* const slot = ws.rec + (n_iter - flushed);
    hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.rowstat, n, alpha_d, o.tol, slot);
    LASSO_HIP_TRY(hipGetLastError());
    ++n_iter;
    if (can_stop) {
      if (int s = read_back(hist.data(), slot, sizeof(Rec), st)) return s;
      if (tr && n_iter <= tr->capacity) {
        tr->obj[n_iter - 1] = hist[0].obj;
        tr->prim_feas[n_iter - 1] = hist[0].prim;
        tr->dual_feas[n_iter - 1] = hist[0].dual;
        tr->gap[n_iter - 1] = hist[0].gap;
      }
      flushed = n_iter;
      if (hist[0].stop) {
        status = LASSO_INTERIOR_POINT_CONVERGED;
        break;
      }
    } else if (n_iter - flushed == kHist) {
      if (int s = flush()) return s;
    }
  }
  if (int s = flush()) return s;
  res->n_iter = n_iter;
  res->status = status;
  hipLaunchKernelGGL(copy_out_kernel, dim3(gk), dim3(256), 0, st, ws.ZD, zout, ldz, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace interior_point
}  // namespace lasso
