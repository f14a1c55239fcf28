// Iterated ridge regression for the lasso (Schmidt 2005, section 2.5; the reference's
// lasso/linear/solvers/iterative_ridge.py) on the HIP path: the driver behind lasso_iter_ridge_solve and
// lasso_iter_ridge_rows.  Each iteration solves, for every row of the batch, the ridge system on that row's support
//   (G[S,S] + diag(alpha / |z_S| + tikhonov)) z_S = (x W)_S,   S = {j : |z_j| >= eps},   G = W^T W,
// where the reference builds and factors one masked k x k matrix per row at full size.  The masked rows and columns
// of that matrix are zero with `tikhonov` on the diagonal and a zero right-hand side, so its solution restricted to
// S is the solution of the compacted system and 0 elsewhere.
//
// rows_kernel is the hot path: one workgroup per row.  It compacts the support in index order, gathers the lower
// triangle of G[S,S] in 32 x 32 blocks, runs a blocked right-looking Cholesky and the two substitutions, and scatters
// z_sol (masked entries get a literal 0).  Per block column J:
//   diagonal block   wave 0, lane r = row r in 32 registers, the pivot row broadcast with v_readlane (no barrier)
//   panel            one thread per row below: X L_JJ^T = A_IJ by substitution in registers, L_JJ broadcast from LDS
//   trailing update  A_IK -= L_IJ L_KJ^T, one 32 x 32 tile per wave at a time on v_mfma_f32_16x16x4_f32
// so a block column costs three barriers whatever its width.  Two tiers share that code:
//   LDS tier (support <= kCap = 256): the packed triangle lives in LDS (row stride 33 floats), sized by the launch
//     from the batch's largest support: 4224 B x nb (nb + 1) / 2 for nb = ceil(s / 32) block rows, 152 KB at s = 256.
//   general tier (support <= 1024): the triangle lives in a per-workgroup scratch of the workspace; the factored panel
//     of the current block column (all rows x 32) and the diagonal block are staged in LDS, so the MFMA operands never
//     come from memory.  A fixed number of workgroups walks the rows: the scratch is a fixed budget, not n k^2.
// A pivot that is not positive (or NaN) is recorded per row as 1 + its index in the compacted system and replaced by
// 1: the kernel has no data-dependent loop and cannot fault on bad data.  The driver folds the flags (lowest row wins).
//
// Everything else is the GEMM of solver_common.hpp with its two plain epilogues (G, x W, the residual with
// its sum of squares, q = p W^T) and element-wise passes whose sums are folded in double in a fixed order: no float
// atomics, two solves of the same arguments are bitwise equal.  The host reads one control block per iteration (and one
// per Brent evaluation).  With the line search, f(t) = 0.5 (|r|^2 + 2 t <r,q> + t^2 |q|^2) + alpha sum |z + t p| from
// three sums taken once per iteration: a Brent evaluation is one pass over [n,k], never a product.
#include "solver_common.hpp"
#include "brent_host.hpp"

namespace lasso {
namespace iter_ridge {
namespace {

using namespace solver;

constexpr int kNB = 32;                       // block side of the packed triangle
constexpr int kRS = 33;                       // row stride of a block in LDS (floats)
constexpr int kCap = 256;                     // largest support of the LDS tier
constexpr size_t kScratchBudget = (size_t)256 << 20;   // general tier: bytes of per-workgroup triangles, at most
constexpr int kScratchRows = 256;             // ... and workgroups, at most

// control block (device; the host reads it once per iteration / Brent evaluation)
struct Ctl {
  double sum_upd, nan_upd, l1, rr, f;         // sum |update|, NaN entries of update, |z|_1, |z W^T - x|^2, objective
  double rq, qq;                              // line search: <r, q>, |q|^2
  double ft;                                  // line search: objective of the last trial
  double ssum;                                // entries of the new z with |z| >= eps
  int smax;                                   // ... the most in one row
  int bad_row, bad_minor, pad;                // lowest row with a bad pivot (-1: none) and its leading minor
};

__device__ __forceinline__ int tri(int b) { return (b * (b + 1)) >> 1; }

__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

struct RowsArgs {
  const float* G; int64_t ldg;                // W^T W [k][k]
  const float* RHS; int64_t ldr;              // x W [n][k]
  const float* Z; int64_t ldz;                // the current code [n][k]
  float* ZS; int64_t ldzs;                    // out: z_sol [n][k]
  int* piv;                                   // out [n]: 0, 1 + index of the first bad pivot, -1 support beyond the launch
  float* scratch; int64_t scratch_stride;     // general tier: one packed triangle per workgroup
  int n, k, nbmax;                            // nbmax: block rows the launch has room for
  float alpha, tikhonov, eps;
};

// One workgroup per row (grid-stride).  LDS: the triangle in LDS; otherwise in a.scratch, panel and diagonal block in LDS.
template <bool LDS>
__global__ __launch_bounds__(256) void rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RS = LDS ? kRS : kNB;         // row stride of a block of M
  constexpr int BS = kNB * RS;                // floats per block of M
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int sp_max = a.nbmax * kNB;
  float* const smem_f = reinterpret_cast<float*>(smem);
  float* cur = smem_f;
  float* M;                                   // the packed lower triangle: block (bi, bj) at tri(bi) + bj
  float* P = nullptr;                         // general tier: the factored panel, row i at P + i * kRS
  float* D = nullptr;                         // general tier: the diagonal block (row stride kRS)
  if constexpr (LDS) {
    M = cur;
    cur += (size_t)tri(a.nbmax) * BS;
  } else {
    M = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    D = cur;
    cur += kNB * kRS;
    P = cur;
    cur += (size_t)sp_max * kRS;
  }
  float* const b = cur;                       // right-hand side, then the solution [sp_max]
  cur += sp_max;
  int* const scan = reinterpret_cast<int*>(cur);   // [256]
  cur += 256;
  unsigned short* const idx = reinterpret_cast<unsigned short*>(cur);   // support indices in index order [sp_max]

  for (int row = blockIdx.x; row < a.n; row += gridDim.x) {
    const float* const z = a.Z + (int64_t)row * a.ldz;
    float* const zs = a.ZS + (int64_t)row * a.ldzs;
    // ---- the support, compacted in index order: thread t owns entries 4t .. 4t + 3 ----
    bool in[4];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * tid + e;
      in[e] = false;
      if (j < a.k) {
        in[e] = !(fabsf(z[j]) < a.eps);       // (a NaN entry is on the support: its pivot reports it)
        if (!in[e]) zs[j] = 0.0f;
      }
      cnt += in[e] ? 1 : 0;
    }
    scan[tid] = cnt;
    __syncthreads();
    int ts = tid;
    asm volatile("" : "+v"(ts));              // (keeps the eight predicates of the scan out of scalar registers)
    for (int off = 1; off < 256; off <<= 1) {
      const int v = ts >= off ? scan[ts - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int s = scan[255];
    const int base = scan[tid] - cnt;
    __syncthreads();                          // (scan is rewritten by the next row)
    if (s > sp_max || s == 0) {               // no room (the driver sized the launch: not reached) / nothing to solve
      if (s > sp_max) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (in[e]) zs[4 * tid + e] = 0.0f;
      }
      if (tid == 0) a.piv[row] = s == 0 ? 0 : -1;
      continue;
    }
    {
      int o = base;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (in[e]) idx[o++] = (unsigned short)(4 * tid + e);
    }
    __syncthreads();
    const int nbr = (s + kNB - 1) / kNB, sp = nbr * kNB;
    for (int i = tid; i < sp; i += 256) b[i] = i < s ? a.RHS[(int64_t)row * a.ldr + idx[i]] : 0.0f;
    // ---- gather G[S,S] + diag(alpha / |z_S| + tikhonov), the identity on the padding ----
    for (int bi = 0; bi < nbr; ++bi)
      for (int bj = 0; bj <= bi; ++bj) {
        float* const blk = M + (size_t)(tri(bi) + bj) * BS;
        for (int e = tid; e < kNB * kNB; e += 256) {
          const int r = e >> 5, c = e & 31;
          const int i = bi * kNB + r, j = bj * kNB + c;
          float v = i == j ? 1.0f : 0.0f;
          if (i < s && j < s) {
            const int gi = idx[i], gj = idx[j];
            v = a.G[(int64_t)gi * a.ldg + gj];
            if (i == j) v = __fadd_rn(v, __fadd_rn(__fdiv_rn(a.alpha, fabsf(z[gi])), a.tikhonov));
          }
          blk[r * RS + c] = v;
        }
      }
    __syncthreads();

    int bad = 0;                              // (wave 0) 1 + index of the first bad pivot
    // ---- blocked right-looking Cholesky ----
    for (int J = 0; J < nbr; ++J) {
      float* const MJJ = M + (size_t)(tri(J) + J) * BS;
      float* DJ = MJJ;                        // the diagonal block, row stride kRS
      if constexpr (!LDS) {
        for (int e = tid; e < kNB * kNB; e += 256) D[(e >> 5) * kRS + (e & 31)] = MJJ[e];
        DJ = D;
        __syncthreads();
      }
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
          float root = __fsqrt_rn(piv);
          if (!(piv > 0.0f)) {
            if (!bad) bad = J * kNB + cc + 1;
            root = 1.0f;
          }
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
          for (int c = 0; c < kNB; ++c) {
            const float v = c <= r ? av[c] : 0.0f;
            DJ[r * kRS + c] = v;
            if constexpr (!LDS) MJJ[r * RS + c] = v;
          }
        }
      }
      __syncthreads();
      // panel: row i of the blocks below, X L_JJ^T = A.  (L_JJ through a vector offset: 528 uniform addresses would
      // each take a scalar register across the loop)
      int djo = (int)(DJ - smem_f);
      asm volatile("" : "+v"(djo));
      const float* const dj = smem_f + djo;
      for (int i = (J + 1) * kNB + tid; i < sp; i += 256) {
        float* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * RS;
        float x[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) x[c] = src[c];
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          float acc = x[c];
#pragma unroll
          for (int j = 0; j < c; ++j) acc = fmaf(-x[j], dj[c * kRS + j], acc);
          x[c] = __fdiv_rn(acc, dj[c * kRS + c]);
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
        float av[2][8], bv[2][8];
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
        float* const dst = M + (size_t)(tri(I) + K) * BS;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k0 = 0; k0 < 8; ++k0) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ti][k0], bv[tj][k0], acc, 0, 0, 0);
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              float* const p = dst + (16 * ti + 4 * q + rg) * RS + 16 * tj + l15;
              *p = __fsub_rn(*p, acc[rg]);
            }
          }
      }
      __syncthreads();
    }

    // ---- L y = b ----
    for (int J = 0; J < nbr; ++J) {
      const float* const MJJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) {
        int r = lane & 31;
        asm volatile("" : "+v"(r));
        float lr[kNB];
#pragma unroll
        for (int c = 0; c < kNB; ++c) lr[c] = MJJ[r * RS + c];
        float bv = b[J * kNB + r];
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          const float yc = __fdiv_rn(lane_bcast(bv, c), lane_bcast(lr[c], c));
          if (r == c) bv = yc;
          else if (r > c) bv = fmaf(-lr[c], yc, bv);
          if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 32) b[J * kNB + r] = bv;
      }
      __syncthreads();
      for (int i = (J + 1) * kNB + tid; i < sp; i += 256) {
        const float* const src = M + (size_t)(tri(i >> 5) + J) * BS + (i & 31) * RS;
        float acc = b[i];
#pragma unroll 8
        for (int c = 0; c < kNB; ++c) acc = fmaf(-src[c], b[J * kNB + c], acc);
        b[i] = acc;
      }
      __syncthreads();
    }
    // ---- L^T z = y ----
    for (int J = nbr - 1; J >= 0; --J) {
      const float* const MJJ = M + (size_t)(tri(J) + J) * BS;
      if (w == 0) {
        int r = lane & 31;
        asm volatile("" : "+v"(r));
        float lc[kNB];                        // column r of L_JJ
#pragma unroll
        for (int c = 0; c < kNB; ++c) lc[c] = MJJ[c * RS + r];
        float bv = b[J * kNB + r];
#pragma unroll
        for (int c = kNB - 1; c >= 0; --c) {
          const float zc = __fdiv_rn(lane_bcast(bv, c), lane_bcast(lc[c], c));
          if (r == c) bv = zc;
          else if (r < c) bv = fmaf(-lc[c], zc, bv);
          if ((c & 7) == 0) __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 32) b[J * kNB + r] = bv;
      }
      __syncthreads();
      for (int i = tid; i < J * kNB; i += 256) {
        const float* const src = M + (size_t)(tri(J) + (i >> 5)) * BS + (i & 31);
        float acc = b[i];
#pragma unroll 8
        for (int c = 0; c < kNB; ++c) acc = fmaf(-src[c * RS], b[J * kNB + c], acc);
        b[i] = acc;
      }
      __syncthreads();
    }
    for (int i = tid; i < s; i += 256) zs[idx[i]] = b[i];
    if (tid == 0) a.piv[row] = bad;
    __syncthreads();                          // (b and idx are rewritten by the next row)
  }
}

// p = z_sol - z over every entry (in place in the z_sol buffer)
__global__ __launch_bounds__(256) void dir_kernel(float* __restrict__ ZS, const float* __restrict__ Z, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    ZS[i] = __fsub_rn(ZS[i], Z[i]);
}

// The accept step, one wave per row.  mode 0 (no line search): update = z_sol - z, z = where(mask, z, z_sol);
// mode 1: update = p t, z = where(mask, z, z + update); mode 2: z is only measured.  mask = |z| < eps of the OLD z.
// partials {sum |update|, NaN entries of update, support of the new z, |new z|_1; the largest support of a row}
__global__ __launch_bounds__(256) void accept_kernel(float* __restrict__ Z, int64_t ldz, const float* __restrict__ S, int n, int k,
                                                     float eps, int mode, float t, double* __restrict__ part) {
  __shared__ double red[32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  float mx[1] = {0.0f};
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < n; row += (int64_t)gridDim.x * 4) {
    int cnt = 0;
    for (int j = lane; j < k; j += 64) {
      const float z = Z[row * ldz + j];
      float zn = z;
      if (mode != 2) {
        const float sv = S[row * k + j];
        const bool mask = fabsf(z) < eps;
        const float upd = mode == 1 ? __fmul_rn(sv, t) : __fsub_rn(sv, z);
        zn = mask ? z : (mode == 1 ? __fadd_rn(z, upd) : sv);
        s[0] += (double)fabsf(upd);
        s[1] += upd != upd ? 1.0 : 0.0;
        Z[row * ldz + j] = zn;
      }
      s[3] += (double)fabsf(zn);
      cnt += fabsf(zn) < eps ? 0 : 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) s[2] += (double)cnt;
    mx[0] = fmaxf(mx[0], (float)cnt);
  }
  block_fold<4, 1>(s, mx, red, part + (int64_t)blockIdx.x * kPart);
}

// partials {|r|^2, <r,q>, |q|^2} over [n,d]
__global__ __launch_bounds__(256) void quad_kernel(const float* __restrict__ R, const float* __restrict__ Q, int64_t total,
                                                   double* __restrict__ part) {
  __shared__ double red[32];
  double s[3] = {0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const double r = (double)R[i], qv = (double)Q[i];
    s[0] += r * r;
    s[1] += r * qv;
    s[2] += qv * qv;
  }
  block_fold<3, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

__global__ __launch_bounds__(256) void quad_fold_kernel(const double* __restrict__ part, int nb, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 3, 0, red, a);
  if (threadIdx.x == 0) {
    ctl->rr = a[0];
    ctl->rq = a[1];
    ctl->qq = a[2];
  }
}

// partial {sum |z + t p|} over [n,k]
__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ Z, const float* __restrict__ P, int64_t total, float t,
                                                 double* __restrict__ part) {
  __shared__ double red[32];
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    s[0] += (double)fabsf(__fmaf_rn(t, P[i], Z[i]));
  block_fold<1, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// f(t) = 0.5 (|r|^2 + 2 t <r,q> + t^2 |q|^2) + alpha sum |z + t p|
__global__ __launch_bounds__(256) void trial_fold_kernel(const double* __restrict__ part, int nb, double t, double alpha,
                                                         Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) ctl->ft = 0.5 * (ctl->rr + 2.0 * t * ctl->rq + t * t * ctl->qq) + alpha * a[0];
}

// the iteration's control block: the accept step's sums, |r|^2 of the new z (part_r != null) and the pivot flags
__global__ __launch_bounds__(256) void stat_kernel(const double* __restrict__ part_a, int nb_a, const double* __restrict__ part_r,
                                                   int nb_r, const int* __restrict__ piv, int n, double alpha,
                                                   Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], r[kPart];
  __shared__ int low[256];
  fold_partials(part_a, nb_a, 4, 1, red, a);
  if (part_r) fold_partials(part_r, nb_r, 1, 0, red, r);
  int first = n;                              // the lowest row with a flag
  if (piv)
    for (int i = threadIdx.x; i < n; i += 256)
      if (piv[i] != 0 && i < first) first = i;
  low[threadIdx.x] = first;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) low[threadIdx.x] = min(low[threadIdx.x], low[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl->sum_upd = a[0];
    ctl->nan_upd = a[1];
    ctl->ssum = a[2];
    ctl->l1 = a[3];
    ctl->smax = (int)a[4];
    if (part_r) {
      ctl->rr = r[0];
      ctl->f = 0.5 * r[0] + alpha * a[3];
    }
    ctl->bad_row = low[0] < n ? low[0] : -1;
    ctl->bad_minor = low[0] < n ? piv[low[0]] : 0;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
size_t tri_bytes(int nb) { return (size_t)nb * (nb + 1) / 2 * kNB * kNB * 4; }            // one scratch triangle

size_t lds_bytes(bool lds_tier, int nb) {
  const size_t sp = (size_t)nb * kNB;
  const size_t mat = lds_tier ? (size_t)nb * (nb + 1) / 2 * kNB * kRS * 4 : (sp * kRS + kNB * kRS) * 4;
  return mat + sp * 4 + 256 * 4 + sp * 2;
}

// workgroups of the general tier for a code of k entries: as many triangles as the budget holds
int scratch_rows(int64_t n, int k) {
  if (k <= kCap) return 0;
  const int nb = (k + kNB - 1) / kNB;
  const int64_t fit = (int64_t)(kScratchBudget / tri_bytes(nb));
  return (int)std::max<int64_t>(1, std::min<int64_t>({n, fit, (int64_t)kScratchRows}));
}

// z_sol of every row for a batch whose largest support is smax
hipError_t launch_rows(RowsArgs a, int smax, int rows_cap, hipStream_t st) {
  const int nb = std::max(1, (smax + kNB - 1) / kNB);
  a.nbmax = nb;
  if (smax <= kCap) {
    const size_t lds = lds_bytes(true, nb);
    if (lds > 48 * 1024)
      if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&rows_kernel<true>), lds); e != hipSuccess) return e;
    const int grid = (int)std::min<int64_t>(a.n, 1 << 20);
    hipLaunchKernelGGL(rows_kernel<true>, dim3(grid), dim3(256), lds, st, a);
  } else {
    const size_t lds = lds_bytes(false, nb);
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&rows_kernel<false>), lds); e != hipSuccess) return e;
    a.scratch_stride = (int64_t)(tri_bytes((a.k + kNB - 1) / kNB) / 4);
    hipLaunchKernelGGL(rows_kernel<false>, dim3(std::min(a.n, rows_cap)), dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

int accept_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kEwBlocks, (n + 3) / 4)); }

struct Space {
  float *Wt, *G, *RHS, *Z, *ZS, *R, *Q, *scratch;
  int* piv;
  double *part_r, *part_a, *part_e;
  Ctl* ctl;
  int rows_cap;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4;
  w.Wt = a.take((size_t)k * d * 4);
  w.G = a.take((size_t)k * k * 4);
  w.RHS = a.take(nk);
  w.Z = a.take(nk);
  w.ZS = a.take(nk);
  w.R = a.take(nd);
  w.Q = a.take(nd);
  w.piv = a.take<int>((size_t)n * 4);
  w.part_r = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8);
  w.part_a = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.part_e = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.ctl = a.take<Ctl>(sizeof(Ctl));
  w.rows_cap = scratch_rows(n, (int)k);
  w.scratch = a.take((size_t)w.rows_cap * tri_bytes(((int)k + kNB - 1) / kNB));
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int rows(const float* g, int64_t ldg, const float* rhs, int64_t ldr, const float* z, int64_t ldz, float* zsol, int64_t ldzs,
         int64_t n64, int64_t k64, double alpha, double tikhonov, double eps, int64_t* bad_row, int32_t* bad_minor,
         int32_t* support_max, void* workspace, hipStream_t st) {
  const int n = (int)n64, k = (int)k64;
  const Space ws = carve(workspace, n, 1, k);
  Ctl h;
  // the largest support sizes the launch
  hipLaunchKernelGGL(accept_kernel, dim3(accept_grid(n)), dim3(256), 0, st, const_cast<float*>(z), ldz, (const float*)nullptr, n, k,
                     (float)eps, 2, 0.0f, ws.part_a);
  hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_a, accept_grid(n), (const double*)nullptr, 0,
                     (const int*)nullptr, n, alpha, ws.ctl);
  LASSO_HIP_TRY(hipGetLastError());
  if (int s = read_back(&h, ws.ctl, sizeof(Ctl), st)) return s;
  if (support_max) *support_max = h.smax;
  RowsArgs a = {};
  a.G = g; a.ldg = ldg; a.RHS = rhs; a.ldr = ldr; a.Z = z; a.ldz = ldz; a.ZS = zsol; a.ldzs = ldzs;
  a.piv = ws.piv; a.scratch = ws.scratch; a.n = n; a.k = k;
  a.alpha = (float)alpha; a.tikhonov = (float)tikhonov; a.eps = (float)eps;
  LASSO_HIP_TRY(launch_rows(a, h.smax, ws.rows_cap, st));
  hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_a, accept_grid(n), (const double*)nullptr, 0,
                     (const int*)ws.piv, n, alpha, ws.ctl);
  LASSO_HIP_TRY(hipGetLastError());
  if (int s = read_back(&h, ws.ctl, sizeof(Ctl), st)) return s;
  *bad_row = h.bad_row;
  *bad_minor = h.bad_minor;
  return LASSO_OK;
}

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha, const lasso_iter_ridge_options& o, lasso_iter_ridge_result* res,
          void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const Space ws = carve(workspace, n, d, k);
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  // LASSO_FORCE_BLOCKS_128 (tests): 128 x 128 blocks below the size at which block_side takes them
  const bool force128 = (o.reserved & LASSO_FORCE_BLOCKS_128) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // products [n,d]
  const int pd = gemm_parts(n, d, side_d);
  const int64_t nk = (int64_t)n * k, nd = (int64_t)n * d;
  const int gk = ew_grid(nk), gd = ew_grid(nd), ga = accept_grid(n);
  const float eps = (float)o.eps;
  const double budget = (double)nk * o.tol;   // the reference's tol = z0.numel() * tol
  lasso_iter_ridge_trace* const tr = res->trace;

  // ---- once per solve: G = W^T W, rhs = x W ----
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));
  LASSO_HIP_TRY(launch_gemm(ws.Wt, d, ws.Wt, d, k, k, d, StoreEpi{ws.G, k, 0}, 64, 1, st));
  LASSO_HIP_TRY(launch_gemm(x, ldx, ws.Wt, d, n, k, d, StoreEpi{ws.RHS, k, 0}, side_k, 1, st));
  Ctl h;
  memset(&h, 0, sizeof(h));
  auto fetch = [&]() -> int { return read_back(&h, ws.ctl, sizeof(Ctl), st); };
  // r = z W^T - x with the block partials of |r|^2
  auto residual = [&]() -> hipError_t {
    return launch_gemm(ws.Z, k, w, ldw, n, d, k, Resid0Epi{x, ldx, ws.R, d, ws.part_r, 0}, side_d, 1, st);
  };
  auto stat = [&](bool flags) -> int {
    hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_a, ga, (const double*)ws.part_r, pd,
                       flags ? (const int*)ws.piv : (const int*)nullptr, n, alpha, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    return fetch();
  };

  hipLaunchKernelGGL(init_packed_kernel<>, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, n, k);
  hipLaunchKernelGGL(accept_kernel, dim3(ga), dim3(256), 0, st, ws.Z, (int64_t)k, (const float*)nullptr, n, k, eps, 2, 0.0f,
                     ws.part_a);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(residual());
  if (int s = stat(false)) return s;
  res->f0 = res->f_final = h.f;
  double fval = h.f;
  int status = LASSO_ITER_RIDGE_MAXITER, n_iter = 0;
  while (n_iter < o.maxiter) {
    RowsArgs a = {};
    a.G = ws.G; a.ldg = k; a.RHS = ws.RHS; a.ldr = k; a.Z = ws.Z; a.ldz = k; a.ZS = ws.ZS; a.ldzs = k;
    a.piv = ws.piv; a.scratch = ws.scratch; a.n = n; a.k = k;
    a.alpha = (float)alpha; a.tikhonov = (float)o.tikhonov; a.eps = eps;
    LASSO_HIP_TRY(launch_rows(a, h.smax, ws.rows_cap, st));
    double t = 1.0;
    int ls_evals = 0;
    if (o.line_search) {
      hipLaunchKernelGGL(dir_kernel, dim3(gk), dim3(256), 0, st, ws.ZS, ws.Z, nk);
      LASSO_HIP_TRY(hipGetLastError());
      LASSO_HIP_TRY(launch_gemm(ws.ZS, k, w, ldw, n, d, k, StoreEpi{ws.Q, d, 0}, side_d, 1, st));
      hipLaunchKernelGGL(quad_kernel, dim3(gd), dim3(256), 0, st, ws.R, ws.Q, nd, ws.part_e);
      hipLaunchKernelGGL(quad_fold_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gd, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      BoundedMin search(0.0, 10.0, 1e-5, 500);
      while (!search.finished()) {
        const double tt = search.next();
        const float tf = (float)tt;
        hipLaunchKernelGGL(l1_kernel, dim3(gk), dim3(256), 0, st, ws.Z, ws.ZS, nk, tf, ws.part_e);
        hipLaunchKernelGGL(trial_fold_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gk, (double)tf, alpha, ws.ctl);
        LASSO_HIP_TRY(hipGetLastError());
        if (int s = fetch()) return s;
        if (tr) {
          if (tr->eval_count < tr->eval_capacity) {
            tr->eval_iter[tr->eval_count] = n_iter + 1;
            tr->eval_t[tr->eval_count] = tt;
            tr->eval_f[tr->eval_count] = h.ft;
          }
          ++tr->eval_count;
        }
        search.tell(h.ft);
        if (!isfinite(h.ft)) break;           // (a NaN objective would walk the search to its evaluation limit)
      }
      t = search.best_x();
      fval = search.best_f();
      ls_evals = search.evaluations();
    }
    hipLaunchKernelGGL(accept_kernel, dim3(ga), dim3(256), 0, st, ws.Z, (int64_t)k, (const float*)ws.ZS, n, k, eps,
                       o.line_search ? 1 : 0, (float)t, ws.part_a);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(residual());
    if (int s = stat(true)) return s;
    if (h.bad_row >= 0) {
      res->bad_row = h.bad_row;
      res->bad_minor = h.bad_minor;
      res->n_iter = n_iter;
      if (h.bad_minor < 0) return fail(LASSO_ERR_HIP, "iterated ridge: row %d outgrew the launch", h.bad_row);
      return fail(LASSO_ERR_BAD_ARG, "iterated ridge: the system of row %d is not positive definite (leading minor %d)",
                  h.bad_row, h.bad_minor);
    }
    if (!o.line_search) fval = h.f;
    ++n_iter;
    if (tr && n_iter <= tr->capacity) {
      tr->f[n_iter - 1] = fval;
      tr->update[n_iter - 1] = h.sum_upd;
      tr->t[n_iter - 1] = t;
      tr->ls_evals[n_iter - 1] = ls_evals;
      tr->support_max[n_iter - 1] = h.smax;
      tr->support_mean[n_iter - 1] = h.ssum / (double)n;
    }
    res->f_final = fval;
    if ((float)h.sum_upd <= (float)budget) {  // the reference compares float32 values
      status = LASSO_ITER_RIDGE_CONVERGED;
      break;
    }
    if (fval != fval || h.nan_upd > 0.0) {
      status = LASSO_ITER_RIDGE_NAN;
      break;
    }
  }
  res->n_iter = n_iter;
  res->status = status;
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, ws.Z, zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace iter_ridge
}  // namespace lasso
