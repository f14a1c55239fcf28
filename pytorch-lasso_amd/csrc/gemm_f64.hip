// float64 tensors on the HIP path (LASSO_F64): the general-GEMM form of the FISTA solve, the objective and
// init='transpose' in IEEE double on v_mfma_f64_16x16x4_f64 -- arithmetic, accumulation, soft-threshold, momentum,
// the stop rule's sum and the line search's F / Q sums; no fp32 value anywhere.
//
//   gemm_f64_nt_kernel<EPI, BT>:  acc[m][nn] = sum_t A[i][t] * B(j, t),   B(j, t) = B[j*ldb + t]  (BT = false)
//                                                                                   B[t*ldb + j]  (BT = true: the
//   dictionary W [d][k] serves both products of an iteration as it is -- no transposed copy)
//     EPI_SUB   C = C0 - acc   (C0 = nullptr: -acc)      residual x - y W^T; gradient r W = -(x - y W^T) W
//     EPI_PLAIN C = acc                                   init='transpose': x W
//     EPI_PROX  u = y + lr*acc (acc = -(gradient)), z+ = S_lam(u), y+ = z+ + coef (z+ - z), the workgroup's sum of
//               |z - z+| to dpart[block]; the gradient block never goes to memory
//   One workgroup (4 waves) per 64 x 64 block of C, a 32 x 32 quadrant (2 x 2 MFMA blocks, 4 independent accumulator
//   chains) per wave; the contraction in chunks of 16 through LDS, double-buffered: the global loads of chunk c+1 are
//   issued before the MFMAs of chunk c and stored to the other buffer behind them, one barrier per chunk.  LDS rows
//   are padded to 17 doubles (as syrk_f64_kernel pads: a lane's fragment read walks rows, stride 17 spreads the banks);
//   2 operands x 2 buffers x 64 x 17 x 8 = 34816 bytes.  Operands are loaded one double per lane (guarded on ragged edges), so any
//   m, nn, kk >= 1, any leading dimension and any 8-byte alignment work.
//   MFMA f64 layouts (NOT tile_device.hpp's fp32 maps): A/B one double per lane, row lane&15, contraction lane>>4;
//   C/D col = lane&15, row = (lane>>4) + 4*reg.
// Every reduction runs in a fixed order (strided per thread, a tree per workgroup, a one-workgroup pass over the
// partials): no atomics, a solve is bitwise reproducible.
// The fused one-kernel solve (fista_tile_sp_kernel) has no double form: its 16 x 1024 z-tile alone would be 128 KB of
// the 160 KB LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <type_traits>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"
#include "stoprule_host.hpp"
#include "f64_device.hpp"

namespace lasso {
namespace f64 {
namespace {

constexpr int kBM = 64, kBN = 64, kKC = 16, kRS = kKC + 1;
constexpr int kGrid = kSumGrid;       // workgroups (and partial sums per set) of the element-wise kernels
constexpr int kMaxTrials = 1000;      // ista.py:17 (maxiter=1000)
enum { EPI_SUB = 0, EPI_PLAIN = 1, EPI_PROX = 2 };

struct GemmArgs {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  const double* C0; int64_t ldc0;
  double* C; int64_t ldc;             // EPI_PROX: z (read and written)
  double* Y; int64_t ldy;             // EPI_PROX: y (read and written)
  double lr, lam, coef;
  double* dpart;
  int m, nn, kk;
};

template <int EPI, bool BT>
__global__ __launch_bounds__(256) void gemm_f64_nt_kernel(const GemmArgs g) {
  __shared__ double sa[2][kBM][kRS], sb[2][kBN][kRS];
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.x * kBM, j0 = blockIdx.y * kBN;
  const int iw = 32 * (w >> 1), jw = 32 * (w & 1);
  // loaders: 4 doubles of each operand per thread and chunk; consecutive threads read consecutive addresses
  const int ar = tid >> 4, ac = tid & 15;                 // A (and B, BT = false): rows ar + 16 h, contraction ac
  const int bj = tid & 63, bt = tid >> 6;                 // B, BT = true: column bj, contraction bt + 4 h
  double ra[4], rb[4];
  // interior blocks (the common case) load unguarded; a block on a ragged edge, and the tail chunk of the contraction,
  // take the guarded form (out-of-range elements are zeros)
  const bool interior = i0 + kBM <= g.m && j0 + kBN <= g.nn;
  auto load = [&](int t0) {
    if (interior && t0 + kKC <= g.kk) {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        ra[h] = g.A[(int64_t)(i0 + ar + 16 * h) * g.lda + t0 + ac];
        if constexpr (BT) rb[h] = g.B[(int64_t)(t0 + bt + 4 * h) * g.ldb + j0 + bj];
        else rb[h] = g.B[(int64_t)(j0 + ar + 16 * h) * g.ldb + t0 + ac];
      }
      return;
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int r = i0 + ar + 16 * h, t = t0 + ac;
      ra[h] = (r < g.m && t < g.kk) ? g.A[(int64_t)r * g.lda + t] : 0.0;
      if constexpr (BT) {
        const int j = j0 + bj, tb = t0 + bt + 4 * h;
        rb[h] = (j < g.nn && tb < g.kk) ? g.B[(int64_t)tb * g.ldb + j] : 0.0;
      } else {
        const int j = j0 + ar + 16 * h;
        rb[h] = (j < g.nn && t < g.kk) ? g.B[(int64_t)j * g.ldb + t] : 0.0;
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      sa[buf][ar + 16 * h][ac] = ra[h];
      if constexpr (BT) sb[buf][bj][bt + 4 * h] = rb[h];
      else sb[buf][ar + 16 * h][ac] = rb[h];
    }
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int nc = (g.kk + kKC - 1) / kKC;
  load(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nc;
    if (more) load((c + 1) * kKC);
#pragma unroll
    for (int ks = 0; ks < kKC / 4; ++ks) {
      const double a0 = sa[buf][iw + l15][4 * ks + q], a1 = sa[buf][iw + 16 + l15][4 * ks + q];
      const double b0 = sb[buf][jw + l15][4 * ks + q], b1 = sb[buf][jw + 16 + l15][4 * ks + q];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);         // (everyone left this buffer at the barrier that ended chunk c - 1)
    __syncthreads();
  }
  double dsum = 0.0;
  // GUARD = false (interior blocks): no branch between the elements, so their loads go out together
  auto epilogue = [&](auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    double zv[16], yv[16];            // EPI_PROX / EPI_SUB: every load of the block in front of its first store
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
      zv[e] = yv[e] = 0.0;
      if (GUARD && (row >= g.m || col >= g.nn)) continue;
      if constexpr (EPI == EPI_SUB) {
        if (g.C0) zv[e] = g.C0[(int64_t)row * g.ldc0 + col];
      } else if constexpr (EPI == EPI_PROX) {
        zv[e] = g.C[(int64_t)row * g.ldc + col];
        yv[e] = g.Y[(int64_t)row * g.ldy + col];
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
      if (GUARD && (row >= g.m || col >= g.nn)) continue;
      const double v = acc[e >> 3][(e >> 2) & 1][e & 3];
      if constexpr (EPI == EPI_SUB) {
        g.C[(int64_t)row * g.ldc + col] = zv[e] - v;
      } else if constexpr (EPI == EPI_PLAIN) {
        g.C[(int64_t)row * g.ldc + col] = v;
      } else {
        const double z = zv[e];
        const double u = yv[e] + g.lr * v;                         // y - lr * gradient (ista.py:90), v = -gradient
        const double zn = softshrink(u, g.lam);
        dsum += fabs(z - zn);                                      // :93
        g.C[(int64_t)row * g.ldc + col] = zn;
        g.Y[(int64_t)row * g.ldy + col] = zn + g.coef * (zn - z);  // :100 (ISTA: coef = 0)
      }
    }
  };
  if (interior) epilogue(std::false_type{});
  else epilogue(std::true_type{});
  if constexpr (EPI == EPI_PROX) {
    const double s = block_sum(dsum, red);
    if (tid == 0) g.dpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

template <int EPI, bool BT>
hipError_t launch_gemm(const GemmArgs& g, hipStream_t st) {
  if (g.m <= 0 || g.nn <= 0) return hipSuccess;
  const dim3 grid((unsigned)((g.m + kBM - 1) / kBM), (unsigned)((g.nn + kBN - 1) / kBN));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_f64_nt_kernel<EPI, BT>), grid, dim3(256), 0, st, g);
  return hipGetLastError();
}

int64_t prox_parts(int64_t n, int64_t k) { return ((n + kBM - 1) / kBM) * ((k + kBN - 1) / kBN); }

// C = C0 - A B^T with B [nn][kk] (residual: A = y [n][k], B = W [d][k])
hipError_t gemm_sub(const double* A, int64_t lda, const double* B, int64_t ldb, const double* C0, int64_t ldc0, double* C,
                    int64_t ldc, int m, int nn, int kk, hipStream_t st) {
  GemmArgs g{A, lda, B, ldb, C0, ldc0, C, ldc, nullptr, 0, 0.0, 0.0, 0.0, nullptr, m, nn, kk};
  return launch_gemm<EPI_SUB, false>(g, st);
}

// out[s] = sum of parts[s*count .. s*count + count) in a fixed order; one workgroup per set
__global__ __launch_bounds__(256) void reduce_sets_kernel(const double* __restrict__ parts, int64_t count,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const double* const p = parts + (int64_t)blockIdx.x * count;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) v += p[i];
  const double s = block_sum(v, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// part[b] = sum of v[i]^2 over the elements of workgroup b (grid-stride)
__global__ __launch_bounds__(256) void sumsq_kernel(const double* __restrict__ v, int64_t total, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) s += v[i] * v[i];
  const double r = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// part[b] = sum |Z| over the elements of workgroup b (objective's l1 term), Z [n][k] with pitch ldz
__global__ __launch_bounds__(256) void sumabs_kernel(const double* __restrict__ Z, int64_t ldz, int64_t n, int64_t k,
                                                     double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  const int64_t total = n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    s += fabs(Z[(i / k) * ldz + i % k]);
  const double r = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// line-search trial (ista.py:40, :31-35): cand = S_lam(p - lr g); partial sums of |cand|, dz g, dz^2 (dz = cand - p)
// to part[0 .. 3*grid)
__global__ __launch_bounds__(256) void trial_kernel(const double* __restrict__ P, const double* __restrict__ G,
                                                    double* __restrict__ Cand, int64_t total, double lr, double lam,
                                                    double* __restrict__ part) {
  __shared__ double red[256];
  double l1 = 0.0, dzg = 0.0, dz2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const double p = P[i], gr = G[i];
    const double c = softshrink(p - lr * gr, lam);
    Cand[i] = c;
    const double dz = c - p;
    l1 += fabs(c);
    dzg += dz * gr;
    dz2 += dz * dz;
  }
  const double a = block_sum(l1, red);
  __syncthreads();
  const double b = block_sum(dzg, red);
  __syncthreads();
  const double c = block_sum(dz2, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = a;
    part[gridDim.x + blockIdx.x] = b;
    part[2 * gridDim.x + blockIdx.x] = c;
  }
}

// end of an outer line-search iteration: z+ = cand; sum |z - z+|; y+ = z+ + coef (z+ - z)   (ista.py:93, :100-102)
__global__ __launch_bounds__(256) void finish_kernel(double* __restrict__ Z, int64_t ldz, double* __restrict__ Y,
                                                     const double* __restrict__ Cand, int64_t n, int64_t k, double coef,
                                                     double* __restrict__ dpart) {
  __shared__ double red[256];
  double s = 0.0;
  const int64_t total = n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    double* const zp = Z + (i / k) * ldz + i % k;
    const double z = *zp, zn = Cand[i];
    s += fabs(z - zn);
    *zp = zn;
    Y[i] = zn + coef * (zn - z);
  }
  const double r = block_sum(s, red);
  if (threadIdx.x == 0) dpart[blockIdx.x] = r;
}

// sums = {sum r^2, sum |z|} from the two sets of partials; loss = (0.5 sum r^2 + alpha sum |z|) / n  (dict_learning.py:10-13)
__global__ __launch_bounds__(256) void objective_finish_kernel(const double* __restrict__ part, int64_t count, double alpha,
                                                               double n_total, double* __restrict__ sums,
                                                               double* __restrict__ loss64, float* __restrict__ loss32) {
  __shared__ double red[256];
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) { a += part[i]; b += part[count + i]; }
  const double rss = block_sum(a, red);
  __syncthreads();
  const double l1 = block_sum(b, red);
  if (threadIdx.x == 0) {
    if (sums) { sums[0] = rss; sums[1] = l1; }
    const double loss = (0.5 * rss + alpha * l1) / n_total;
    if (loss64) *loss64 = loss;
    if (loss32) *loss32 = (float)loss;
  }
}

struct Workspace {
  double* Y; double* NR; double* G; double* dpart; double* delta;
  double* C; double* part; double* sums;          // line search only
  double* Yc;                                     // y at the head of a speculated chunk (z's checkpoint lives in G)
  size_t bytes;
};

Workspace carve(void* base, int64_t n, int64_t d, int64_t k, bool backtrack, bool with_state) {
  Workspace w;
  Arena a(base);
  w.Y = a.take<double>((size_t)n * k * 8);
  w.NR = a.take<double>((size_t)n * d * 8);
  w.G = (backtrack || with_state) ? a.take<double>((size_t)n * k * 8) : nullptr;
  w.dpart = a.take<double>((size_t)std::max<int64_t>(kGrid, prox_parts(n, k)) * 8);
  w.delta = a.take<double>(64 * 8);
  w.C = w.part = w.sums = nullptr;
  if (backtrack) {
    w.C = a.take<double>((size_t)n * k * 8);
    w.part = a.take<double>((size_t)5 * kGrid * 8);
    w.sums = a.take<double>(256);
  }
  w.Yc = with_state ? a.take<double>((size_t)n * k * 8) : nullptr;
  w.bytes = a.bytes();
  return w;
}

int start_state(const double* z0, int64_t ldz0, double* zout, int64_t ldz, double* Y, int64_t n, int64_t k,
                hipStream_t st) {
  if (z0) {
    if (z0 != zout || ldz0 != ldz)
      LASSO_HIP_TRY(hipMemcpy2DAsync(zout, ldz * 8, z0, ldz0 * 8, k * 8, n, hipMemcpyDeviceToDevice, st));
  } else {
    LASSO_HIP_TRY(hipMemset2DAsync(zout, ldz * 8, 0, k * 8, n, st));
  }
  LASSO_HIP_TRY(hipMemcpy2DAsync(Y, k * 8, zout, ldz * 8, k * 8, n, hipMemcpyDeviceToDevice, st));
  return LASSO_OK;
}

}  // namespace

// C = C0 - A B^T for the float64 M-step (mstep_f64.hip); b_t = 0: B [nn][kk], else B [kk][nn].  C may be C0: a
// workgroup loads its block of C0 in front of its first store, and no other workgroup touches that block.
hipError_t launch_gemm_sub(const double* A, int64_t lda, const double* B, int64_t ldb, int b_t, const double* C0,
                           int64_t ldc0, double* C, int64_t ldc, int m, int nn, int kk, hipStream_t st) {
  GemmArgs g{A, lda, B, ldb, C0, ldc0, C, ldc, nullptr, 0, 0.0, 0.0, 0.0, nullptr, m, nn, kk};
  return b_t ? launch_gemm<EPI_SUB, true>(g, st) : launch_gemm<EPI_SUB, false>(g, st);
}

// C [m][nn] = A [m][kk] B, B [kk][nn] (conv_f64.hip's explicit synthesis: COLS = Ym W)
hipError_t launch_gemm_plain(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int m,
                             int nn, int kk, hipStream_t st) {
  GemmArgs g{A, lda, B, ldb, nullptr, 0, C, ldc, nullptr, 0, 0.0, 0.0, 0.0, nullptr, m, nn, kk};
  return launch_gemm<EPI_PLAIN, true>(g, st);
}

hipError_t launch_reduce_sets(const double* parts, int64_t count, int sets, double* out, hipStream_t st) {
  hipLaunchKernelGGL(reduce_sets_kernel, dim3(sets), dim3(256), 0, st, parts, count, out);
  return hipGetLastError();
}

// loss = (0.5 sum R^2 + alpha sum |Z|) / n_total from R [nd] and Z [n][k] (pitch ldz); part: 2 kSumGrid doubles
hipError_t launch_objective_sums(const double* R, int64_t nd, const double* Z, int64_t ldz, int64_t n, int64_t k,
                                 double* part, double alpha, double n_total, double* sums, double* loss64, float* loss32,
                                 hipStream_t st) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(kGrid), dim3(256), 0, st, R, nd, part);
  hipLaunchKernelGGL(sumabs_kernel, dim3(kGrid), dim3(256), 0, st, Z, ldz, n, k, part + kGrid);
  hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(256), 0, st, part, (int64_t)kGrid, alpha, n_total, sums,
                     loss64, loss32);
  return hipGetLastError();
}

size_t solve_workspace_bytes(int64_t n, int64_t d, int64_t k, int maxiter, double tol, int stop_mode, int backtrack) {
  const bool with_state = !backtrack && tol > 0.0 && (stop_mode & 0xFF) != LASSO_STOP_NONE && maxiter > 0;
  return carve(nullptr, n, d, k, backtrack != 0, with_state).bytes;
}

const char* solve_kernel_name(int backtrack) {
  return backtrack ? "lasso::f64::gemm_f64_nt_kernel<sub> + lasso::f64::trial_kernel (fp64 MFMA, unfused line search)"
                   : "lasso::f64::gemm_f64_nt_kernel<sub> + lasso::f64::gemm_f64_nt_kernel<prox> (fp64 MFMA, unfused)";
}

// Fixed-step solve.  The stop rule (ista.py:93) is read once per chunk of speculated iterations, as the fp32 unfused
// path does (speculate_stop_rule in stoprule_host.hpp): every iteration's sum stays on the device as a double, the host compares
// doubles; a stop inside a chunk restores the chunk's head and replays exactly the iterations up to the stop -- the
// kernels sum in a fixed order, so the replay is bitwise the state the reference stops in.
int solve(const double* x, int64_t ldx, const double* w, int64_t ldw, const double* z0, int64_t ldz0, double* zout,
          int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha, double lr, int fast, int maxiter, double tol,
          int32_t* iters_out, double* last_delta_out, void* workspace, size_t ws_bytes, hipStream_t st) {
  const bool stop = tol > 0.0 && maxiter > 0;
  const Workspace ws = carve(workspace, n, d, k, false, stop);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (n > INT32_MAX - kBM || d > INT32_MAX - kBN || k > INT32_MAX - kBN || (k + kBN - 1) / kBN > 65535 ||
      (d + kBN - 1) / kBN > 65535)
    return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  if (int s = start_state(z0, ldz0, zout, ldz, ws.Y, n, k, st)) return s;
  const double budget = stop_budget<double>(n, k, tol);                    // z0.numel() * tol (ista.py:64)
  const double lam = alpha * lr;
  const int64_t parts = prox_parts(n, k);
  Momentum64 mom;
  auto iterate = [&](double* delta_slot) -> int {
    const double coef = mom.next(fast);                                     // :98-99
    // NR = x - y W^T (= -r);  the gradient r W = -(NR W) stays in the second product's accumulators
    LASSO_HIP_TRY(gemm_sub(ws.Y, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));
    GemmArgs g{ws.NR, d, w, ldw, nullptr, 0, zout, ldz, ws.Y, k, lr, lam, coef, ws.dpart, (int)n, (int)k, (int)d};
    LASSO_HIP_TRY((launch_gemm<EPI_PROX, true>(g, st)));
    if (delta_slot) {
      hipLaunchKernelGGL(reduce_sets_kernel, dim3(1), dim3(256), 0, st, ws.dpart, parts, delta_slot);
      LASSO_HIP_TRY(hipGetLastError());
    }
    return LASSO_OK;
  };
  double last = NAN;
  int it = 0;
  if (!stop) {
    for (; it < maxiter; ++it)
      if (int s = iterate(nullptr)) return s;
  } else {
    // z's checkpoint at the head of a chunk lives in G, y's in Yc
    auto save = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpy2DAsync(ws.G, k * 8, zout, ldz * 8, k * 8, n, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Yc, ws.Y, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto restore = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpy2DAsync(zout, ldz * 8, ws.G, k * 8, k * 8, n, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Y, ws.Yc, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto read = [&](double* host, int c) -> int { return read_back(host, ws.delta, sizeof(double) * c, st); };
    if (int s = speculate_stop_rule<double>(maxiter, budget, ws.delta, &mom.t, iterate, save, restore,
                                            [] { return (int)LASSO_OK; }, read, &it, &last, "lasso_fista_solve_f64"))
      return s;
  }
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return LASSO_OK;
}

// The line search of ista.py:17-54 in double: per outer iteration the gradient at p (two products), then per trial one
// element-wise launch (candidate + three sums), one product (its residual) and the sum of squares; the five sums go to
// the host as doubles and F <= Q (:45) is decided there in the reference's own order of operations.
int solve_backtracking(const double* x, int64_t ldx, const double* w, int64_t ldw, const double* z0, int64_t ldz0,
                       double* zout, int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha, double lr0, int fast,
                       int maxiter, double tol, double eta, int32_t* iters_out, double* last_delta_out,
                       int32_t* trials_out, double* accepted_lr_out, double* accepted_f_out, void* workspace,
                       size_t ws_bytes, hipStream_t st) {
  const Workspace ws = carve(workspace, n, d, k, true, false);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (n > INT32_MAX - kBM || d > INT32_MAX - kBN || k > INT32_MAX - kBN || (k + kBN - 1) / kBN > 65535 ||
      (d + kBN - 1) / kBN > 65535)
    return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  if (int s = start_state(z0, ldz0, zout, ldz, ws.Y, n, k, st)) return s;
  const double budget = stop_budget<double>(n, k, tol);
  bool warned = false;
  Momentum64 mom;
  double last = NAN;
  int it = 0;
  for (; it < maxiter; ++it) {
    const double coef = mom.next(fast);                                               // :98-99 (ISTA: y == z)
    // NR = x - p W^T (= -r0, :22);  G = r0 W (:24);  part[0 ..) = sum r0^2 (:23)
    LASSO_HIP_TRY(gemm_sub(ws.Y, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));
    {
      GemmArgs g{ws.NR, d, w, ldw, nullptr, 0, ws.G, k, nullptr, 0, 0.0, 0.0, 0.0, nullptr, (int)n, (int)k, (int)d};
      LASSO_HIP_TRY((launch_gemm<EPI_SUB, true>(g, st)));
    }
    hipLaunchKernelGGL(sumsq_kernel, dim3(kGrid), dim3(256), 0, st, ws.NR, n * d, ws.part);
    StepLadder ladder{lr0, eta, alpha};
    double f_acc = NAN, lr_acc = lr0;
    int t = 0, trials = 0;
    for (;;) {
      const bool give_up = t >= kMaxTrials;
      const double lr_t = give_up ? lr0 : ladder.lr;                                    // :48-52
      hipLaunchKernelGGL(trial_kernel, dim3(kGrid), dim3(256), 0, st, ws.Y, ws.G, ws.C, n * k, lr_t, alpha * lr_t,
                         ws.part + 2 * kGrid);                                          // :40, :31-35
      LASSO_HIP_TRY(hipGetLastError());
      LASSO_HIP_TRY(gemm_sub(ws.C, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));  // :27
      hipLaunchKernelGGL(sumsq_kernel, dim3(kGrid), dim3(256), 0, st, ws.NR, n * d, ws.part + kGrid);
      hipLaunchKernelGGL(reduce_sets_kernel, dim3(5), dim3(256), 0, st, ws.part, (int64_t)kGrid, ws.sums);
      LASSO_HIP_TRY(hipGetLastError());
      double hs[5];                                     // {sum r0^2, sum r1^2, sum |z1|, sum dz g, sum dz^2}
      LASSO_HIP_TRY(hipMemcpyAsync(hs, ws.sums, sizeof(hs), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
      const LineSearchVerdict<double> v = line_search_verdict<double>(hs, alpha, lr_t, give_up);   // :23, :28, :32-35
      if (give_up) warned = true;
      if (v.accepted) {                                                                 // :45
        trials = give_up ? kMaxTrials : t + 1;
        f_acc = v.F; lr_acc = lr_t;
        break;
      }
      ladder.descend();                                                                 // :47
      ++t;
    }
    hipLaunchKernelGGL(finish_kernel, dim3(kGrid), dim3(256), 0, st, zout, ldz, ws.Y, ws.C, n, k, coef, ws.dpart);
    hipLaunchKernelGGL(reduce_sets_kernel, dim3(1), dim3(256), 0, st, ws.dpart, (int64_t)kGrid, ws.delta);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(hipMemcpyAsync(&last, ws.delta, sizeof(double), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    if (trials_out) trials_out[it] = trials;
    if (accepted_lr_out) accepted_lr_out[it] = lr_acc;
    if (accepted_f_out) accepted_f_out[it] = f_acc;
    if (tol > 0.0 && last <= budget) { ++it; break; }                                   // :93-95
  }
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return warned ? fail(LASSO_WARN_LINESEARCH, "backtracking line search failed; reverted to lr0") : LASSO_OK;
}

size_t objective_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  (void)k;
  return align_up((size_t)std::max<int64_t>(n, 1) * d * 8) + align_up((size_t)2 * kGrid * 8) + 256;
}

// loss = (0.5 ||x - z W^T||^2 + alpha ||z||_1) / n_total in double; sums (nullable) = {sum r^2, sum |z|}
int objective(const double* x, int64_t ldx, const double* w, int64_t ldw, const double* z, int64_t ldz, int64_t n,
              int64_t d, int64_t k, double alpha, double* loss64, float* loss32, double* sums, void* workspace,
              size_t ws_bytes, hipStream_t st) {
  if (ws_bytes < objective_workspace_bytes(n, d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", objective_workspace_bytes(n, d, k));
  if (n > INT32_MAX - kBM || d > INT32_MAX - kBN || k > INT32_MAX - kBN || (d + kBN - 1) / kBN > 65535)
    return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  if (n == 0) return LASSO_OK;
  char* base = static_cast<char*>(workspace);
  double* R = reinterpret_cast<double*>(base);
  double* part = reinterpret_cast<double*>(base + align_up((size_t)n * d * 8));
  double* own = part + 2 * kGrid;
  LASSO_HIP_TRY(gemm_sub(z, ldz, w, ldw, x, ldx, R, d, (int)n, (int)d, (int)k, st));
  LASSO_HIP_TRY(launch_objective_sums(R, n * d, z, ldz, n, k, part, alpha, (double)n, sums ? sums : own, loss64, loss32, st));
  return LASSO_OK;
}

// z0 [n][k] = x [n][d] W [d][k]   (init='transpose', sparse_encode.py:24-25)
int init_transpose(const double* x, int64_t ldx, const double* w, int64_t ldw, double* z0, int64_t ldz, int64_t n,
                   int64_t d, int64_t k, hipStream_t st) {
  if (n > INT32_MAX - kBM || d > INT32_MAX - kBN || k > INT32_MAX - kBN || (k + kBN - 1) / kBN > 65535)
    return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  GemmArgs g{x, ldx, w, ldw, nullptr, 0, z0, ldz, nullptr, 0, 0.0, 0.0, 0.0, nullptr, (int)n, (int)k, (int)d};
  LASSO_HIP_TRY((launch_gemm<EPI_PLAIN, true>(g, st)));
  return LASSO_OK;
}

}  // namespace f64
}  // namespace lasso
