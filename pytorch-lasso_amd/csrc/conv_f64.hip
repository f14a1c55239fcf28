// float64 tensors on the convolutional path (LASSO_F64): ista_conv2d (lasso/conv2d/ista.py:7-49), its objective, the
// reverse pass of the unrolled solve and the Toeplitz bound (lip_const.py:96-135) in IEEE double on
// v_mfma_f64_16x16x4_f64 -- every value, sum, threshold, momentum step and stop-rule comparison; no fp32 value anywhere.
// Codes are held as rows Zm [M = N Hz Wz][K] for the whole solve, as the fp32 path holds them.
//
//   conv_grad_prox_f64_kernel<EPI>   g = conv2d(r, W) as an implicit GEMM: rows = code pixels, columns = atoms, the
//       contraction over the C kh kw taps in (c, a, b) order.  The A operand of a contraction chunk is gathered from the
//       NCHW image r straight into LDS (taps outside the image are zeros; stride and padding live in the index
//       arithmetic only) -- the patch matrix [M][C kh kw] is never formed.  Body of gemm_f64_nt_kernel: 64 x 64 block,
//       4 waves x (32 x 32), four accumulator chains per wave, chunks of 16 taps double-buffered through LDS rows padded
//       to 17 doubles (2 operands x 2 buffers x 64 x 17 x 8 = 34816 bytes, + 2048 for the block sum).  A wave gathers the
//       taps w, w + 4, w + 8, w + 12 of a chunk for the block's 64 pixels: the tap is wave-uniform (decoded on the
//       scalar unit), the lanes walk the pixels (consecutive addresses along a code row at stride 1).
//         EPI_PROX  u = y - lr g, z+ = S_{alpha lr}(u), y+ = z+ + coef (z+ - z), the block's sum |z - z+| to dpart
//         EPI_ADD   G = add_to + g (add_to nullable): the reverse pass's yb = ub + conv2d(rb, W)
//   synthesis r = conv_transpose2d(y, W) - x, explicit form: COLS [M][C kh kw] = Ym W on gemm_f64_nt_kernel<plain>
//       (gemm_f64.hip; W [K][C kh kw] is its [kk][nn] operand), then conv_residual_f64_kernel adds the overlapping
//       columns of every image pixel in gather form, in (a, b) order, minus x (x nullable).  No atomics.
//   conv_wgrad_f64_kernel   dW [K][C kh kw] += gb^T P(r_i) + y_i^T P(rb) as ONE implicit TN product over the 2M rows,
//       the patches gathered from the images into LDS (gram_tn_f64_kernel's body); the rows are cut into slabs of a
//       bounded scratch, a slab adds every iteration of the reverse pass into its own partial tile (plain
//       read-modify-write) and conv_wgrad_fold_f64_kernel sums the slabs in slab order at the end.
// Every reduction runs in a fixed order: two calls with the same arguments give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"
#include "linesearch_host.hpp"
#include "stoprule_host.hpp"
#include "f64_device.hpp"

namespace lasso {
namespace f64 {
namespace {

constexpr int kCB = 64, kCT = 16, kCRS = kCT + 1;   // block edge, taps per chunk, LDS row pitch
enum { EPI_PROX = 0, EPI_ADD = 1 };

struct ConvGradArgs {
  const double* R;          // [N][C][H][W]
  const double* Wt;         // [K][C kh kw]
  const double* add_to;     // EPI_ADD: [M][K] or null
  double* G;                // EPI_ADD: [M][K]
  double* Z; double* Y;     // EPI_PROX: [M][K], read and written
  double lr, lam, coef;
  double* dpart;
  ConvGeom g;
  int M, ckk;
};

template <int EPI>
__global__ __launch_bounds__(256) void conv_grad_prox_f64_kernel(const ConvGradArgs p) {
  __shared__ double sa[2][kCB][kCRS], sb[2][kCB][kCRS];
  __shared__ double red[256];
  const ConvGeom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.x * kCB, j0 = blockIdx.y * kCB;
  const int iw = 32 * (w >> 1), jw = 32 * (w & 1);
  const int M = p.M, K = g.K, ckk = p.ckk, khw = g.kh * g.kw;
  // A: this lane's pixel of the block (decoded once), the wave's taps w + 4 h of a chunk
  const int arow = i0 + lane;
  const bool rowok = arow < M;
  int n = 0, u = 0, v = 0;
  if (rowok) {
    const int P = g.Hz * g.Wz;
    n = arow / P;
    const int rem = arow - n * P;
    u = rem / g.Wz;
    v = rem - u * g.Wz;
  }
  const int iu = u * g.sh - g.ph, jv = v * g.sw - g.pw;
  const double* const img = p.R + (int64_t)n * g.C * g.H * g.W;
  // B: 4 doubles per thread and chunk, atoms ar + 16 h, tap ac
  const int ar = tid >> 4, ac = tid & 15;
  double ra[4], rb[4];
  // interior blocks load W unguarded; a block on a ragged edge of M or K, and the tail chunk of the taps, take the
  // guarded form (out-of-range elements are zeros).  The image bounds are checked always: that is the padding.
  const bool interior = i0 + kCB <= M && j0 + kCB <= K;
  auto load = [&](int t0) {
    const bool full = interior && t0 + kCT <= ckk;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int t = t0 + w + 4 * h;
      const int c = t / khw, rem = t - c * khw, a = rem / g.kw, b = rem - a * g.kw;
      const int ii = iu + a, jj = jv + b;
      const bool ok = (full || (rowok && t < ckk)) && (unsigned)ii < (unsigned)g.H && (unsigned)jj < (unsigned)g.W;
      ra[h] = ok ? img[((int64_t)c * g.H + ii) * g.W + jj] : 0.0;
    }
    if (full) {
#pragma unroll
      for (int h = 0; h < 4; ++h) rb[h] = p.Wt[(int64_t)(j0 + ar + 16 * h) * ckk + t0 + ac];
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int j = j0 + ar + 16 * h, t = t0 + ac;
        rb[h] = (j < K && t < ckk) ? p.Wt[(int64_t)j * ckk + t] : 0.0;
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      sa[buf][lane][w + 4 * h] = ra[h];
      sb[buf][ar + 16 * h][ac] = rb[h];
    }
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int nc = (ckk + kCT - 1) / kCT;
  load(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nc;
    if (more) load((c + 1) * kCT);
#pragma unroll
    for (int ks = 0; ks < kCT / 4; ++ks) {
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
    double zv[16], yv[16];            // every load of the block in front of its first store
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
      zv[e] = yv[e] = 0.0;
      if (GUARD && (row >= M || col >= K)) continue;
      if constexpr (EPI == EPI_ADD) {
        if (p.add_to) zv[e] = p.add_to[(int64_t)row * K + col];
      } else {
        zv[e] = p.Z[(int64_t)row * K + col];
        yv[e] = p.Y[(int64_t)row * K + col];
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
      if (GUARD && (row >= M || col >= K)) continue;
      const double gr = acc[e >> 3][(e >> 2) & 1][e & 3];
      if constexpr (EPI == EPI_ADD) {
        p.G[(int64_t)row * K + col] = zv[e] + gr;
      } else {
        const double z = zv[e];
        const double u = yv[e] - p.lr * gr;                        // ista.py:28-29 (conv2d)
        const double zn = softshrink(u, p.lam);
        dsum += fabs(z - zn);                                      // :44
        p.Z[(int64_t)row * K + col] = zn;
        p.Y[(int64_t)row * K + col] = zn + p.coef * (zn - z);      // :42 (ISTA: coef = 0)
      }
    }
  };
  if (interior) epilogue(std::false_type{});
  else epilogue(std::true_type{});
  if constexpr (EPI == EPI_PROX) {
    const double s = block_sum(dsum, red);
    if (tid == 0) p.dpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// r[n][c][i][j] = sum over the taps (a, b) and code pixels (u, v) with u sh - ph + a == i, v sw - pw + b == j of
// COLS[(n, u, v)][(c, a, b)], minus x[n][c][i][j] (x nullable): conv_transpose2d's overlap-add, one image element per
// thread, its terms in (a, b) order
__global__ __launch_bounds__(256) void conv_residual_f64_kernel(const double* __restrict__ cols,
                                                                const double* __restrict__ x, double* __restrict__ r,
                                                                const ConvGeom g, int64_t total) {
  const int ckk = g.C * g.kh * g.kw;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % g.W), i = (int)((e / g.W) % g.H);
    const int64_t nc = e / ((int64_t)g.W * g.H);
    const int c = (int)(nc % g.C);
    const int64_t n = nc / g.C;
    double s = 0.0;
    for (int a = 0; a < g.kh; ++a) {
      const int iu = i + g.ph - a;
      if (iu < 0 || iu % g.sh != 0) continue;
      const int u = iu / g.sh;
      if (u >= g.Hz) continue;
      for (int b = 0; b < g.kw; ++b) {
        const int jv = j + g.pw - b;
        if (jv < 0 || jv % g.sw != 0) continue;
        const int v = jv / g.sw;
        if (v >= g.Wz) continue;
        s += cols[((n * g.Hz + u) * g.Wz + v) * ckk + (c * g.kh + a) * g.kw + b];
      }
    }
    r[e] = x ? s - x[e] : s;
  }
}

struct ConvWgradArgs {
  const double* A0; const double* A1;   // [M][K]: gb, y_i
  const double* I0; const double* I1;   // [N][C][H][W]: r_i, rb
  double* part;                         // [slabs][K][C kh kw]
  ConvGeom g;
  int M, ckk, rows_per_slab, accumulate;
};

// part[slab] (+)= A0^T P(I0) + A1^T P(I1) over the slab's rows: block (taps, atoms, slab), the rows in chunks of 16 --
// the chunks of the first term, then those of the second, into the same accumulators.  A wave stages the rows
// w + 4 h of a chunk (wave-uniform: decoded on the scalar unit); a lane owns one atom of A and one tap of the patches.
__global__ __launch_bounds__(256) void conv_wgrad_f64_kernel(const ConvWgradArgs p) {
  __shared__ double sp[2][kCB][kCRS], sq[2][kCB][kCRS];
  const ConvGeom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.y * kCB, j0 = blockIdx.x * kCB;
  const int iw = 32 * (w >> 1), jw = 32 * (w & 1);
  const int K = g.K, ckk = p.ckk, P = g.Hz * g.Wz;
  const int m_lo = blockIdx.z * p.rows_per_slab;
  const int rows = min(p.rows_per_slab, p.M - m_lo);
  const int nc1 = (rows + kCT - 1) / kCT, nc = 2 * nc1;
  const bool pin = i0 + lane < K, qin = j0 + lane < ckk;
  int ta = 0, tb = 0;
  int64_t toff = 0;
  if (qin) {
    const int t = j0 + lane, c = t / (g.kh * g.kw), rem = t - c * g.kh * g.kw;
    ta = rem / g.kw;
    tb = rem - ta * g.kw;
    toff = ((int64_t)c * g.H + ta) * g.W + tb;
  }
  const int64_t chw = (int64_t)g.C * g.H * g.W;
  double rp[4], rq[4];
  auto load = [&](int ch) {
    const int term = ch >= nc1 ? 1 : 0;
    const double* const A = term ? p.A1 : p.A0;
    const double* const I = term ? p.I1 : p.I0;
    const int r0 = (ch - term * nc1) * kCT + w;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int r = r0 + 4 * h;
      const bool ok = r < rows;
      const int m = ok ? m_lo + r : 0;
      const int n = m / P, rem = m - n * P, u = rem / g.Wz, v = rem - u * g.Wz;
      const int iu = u * g.sh - g.ph, jv = v * g.sw - g.pw;
      rp[h] = (ok && pin) ? A[(int64_t)m * K + i0 + lane] : 0.0;
      const bool in = ok && qin && (unsigned)(iu + ta) < (unsigned)g.H && (unsigned)(jv + tb) < (unsigned)g.W;
      rq[h] = in ? I[n * chw + (int64_t)iu * g.W + jv + toff] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      sp[buf][lane][w + 4 * h] = rp[h];
      sq[buf][lane][w + 4 * h] = rq[h];
    }
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  load(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nc;
    if (more) load(c + 1);
#pragma unroll
    for (int ks = 0; ks < kCT / 4; ++ks) {
      const double a0 = sp[buf][iw + l15][4 * ks + q], a1 = sp[buf][iw + 16 + l15][4 * ks + q];
      const double b0 = sq[buf][jw + l15][4 * ks + q], b1 = sq[buf][jw + 16 + l15][4 * ks + q];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
  double* const part = p.part + (int64_t)blockIdx.z * K * ckk;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = i0 + iw + 16 * (e >> 3) + q + 4 * (e & 3), col = j0 + jw + 16 * ((e >> 2) & 1) + l15;
    if (row >= K || col >= ckk) continue;
    double* const o = part + (int64_t)row * ckk + col;
    const double v = acc[e >> 3][(e >> 2) & 1][e & 3];
    *o = p.accumulate ? *o + v : v;
  }
}

// gw[e] = sum over the slabs, in slab order, of part[s][e]
__global__ __launch_bounds__(256) void conv_wgrad_fold_f64_kernel(const double* __restrict__ part, int slabs,
                                                                  int64_t words, double* __restrict__ gw) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < words; e += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int sp = 0; sp < slabs; ++sp) s += part[sp * words + e];
    gw[e] = s;
  }
}

// to_rows: src [N][K][P] -> dst (and dst2, nullable) [N P][K]; else src [N P][K] -> dst [N][K][P]
__global__ __launch_bounds__(256) void conv_relayout_f64_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                double* __restrict__ dst2, int K, int P, int64_t total,
                                                                int to_rows) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    // e walks the destination
    if (to_rows) {
      const int k = (int)(e % K);
      const int64_t m = e / K, n = m / P, pix = m % P;
      const double v = src[(n * K + k) * P + pix];
      dst[e] = v;
      if (dst2) dst2[e] = v;
    } else {
      const int64_t pix = e % P, nk = e / P, n = nk / K;
      const int k = (int)(nk % K);
      dst[e] = src[(n * P + pix) * K + k];
    }
  }
}

// reverse of the momentum step and the prox: zb_{i+1} += (1 + c) yb; zb_i = -c yb;
// ub = [z_{i+1} != 0] zb_{i+1}; gb = -lr ub
__global__ __launch_bounds__(256) void conv_bw_prox_f64_kernel(double* __restrict__ zb_next, double* __restrict__ zb_cur,
                                                               const double* __restrict__ yb,
                                                               const double* __restrict__ z_next, double* __restrict__ ub,
                                                               double* __restrict__ gb, int64_t total, double c, double lr) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const double y = yb[i];
    const double zn = zb_next[i] + (1.0 + c) * y;
    zb_next[i] = zn;
    zb_cur[i] = -c * y;
    const double u = z_next[i] != 0.0 ? zn : 0.0;
    ub[i] = u;
    gb[i] = -lr * u;
  }
}

// y = z + c (z - z_prev)      (z_prev == nullptr: y = z)
__global__ __launch_bounds__(256) void conv_bw_point_f64_kernel(const double* __restrict__ z,
                                                                const double* __restrict__ z_prev, double* __restrict__ y,
                                                                int64_t total, double c) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const double v = z[i];
    y[i] = z_prev ? v + c * (v - z_prev[i]) : v;
  }
}

// a += s * b
__global__ __launch_bounds__(256) void conv_axpy_f64_kernel(double* __restrict__ a, const double* __restrict__ b, double s,
                                                            int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) a[i] += s * b[i];
}

// lip_const.py:96-135 in double.  taps [O][I][T] through the strides (so, si) (T = ksize^2; O <= I after the
// reference's swap).  One workgroup per o: power(o, f) = sum_i (sum_t tap cos(phase[t][f]))^2 + (... sin ...)^2,
// out[o] = max_f power; phase[t][f] = w0[f] h0[t] + w1[f] h1[t], the grid freq[i] = 2 pi i / (sample - 1).
// max(a, b) of two powers (>= +0) that keeps a NaN like torch.max (lip_const.py:131); fmax drops it
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(256) void conv_lip_grid_f64_kernel(double* __restrict__ freq, int sample) {
  for (int i = threadIdx.x; i < sample; i += 256) freq[i] = (2.0 * M_PI * (double)i) / (double)(sample - 1);
}

__global__ __launch_bounds__(256) void conv_lip_f64_kernel(const double* __restrict__ taps, int64_t so, int64_t si, int I,
                                                           int ks, int padding, const double* __restrict__ freq,
                                                           int sample, double* __restrict__ out_max) {
  __shared__ double sred[256];
  const int T = ks * ks;
  const double* const tp = taps + (int64_t)blockIdx.x * so;
  double best = 0.0;
  for (int f = threadIdx.x; f < sample * sample; f += 256) {
    const double w0 = freq[f / sample], w1 = freq[f % sample];
    double power = 0.0, power_im = 0.0;
    for (int i = 0; i < I; ++i) {
      double re = 0.0, im = 0.0;
      for (int t = 0; t < T; ++t) {
        const double h0 = 1.0 + (double)(padding - ks + t / ks), h1 = 1.0 + (double)(padding - ks + t % ks);
        const double ph = w0 * h0 + w1 * h1;
        const double tap = tp[(int64_t)i * si + t];
        re += tap * cos(ph);
        im += tap * sin(ph);
      }
      power += re * re;             // :128-130: the two sums of squares apart, then their sum
      power_im += im * im;
    }
    best = nan_max(best, power + power_im);
  }
  sred[threadIdx.x] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sred[threadIdx.x] = nan_max(sred[threadIdx.x], sred[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out_max[blockIdx.x] = sred[0];
}

__global__ void conv_lip_sum_f64_kernel(const double* __restrict__ maxes, int O, int take_sqrt, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int o = 0; o < O; ++o) s += maxes[o];
    out[0] = take_sqrt ? sqrt(s) : s;
  }
}

unsigned grid_for(int64_t total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096)); }

struct Dims {
  int64_t M, ckk, mk, img, kc, parts;
  explicit Dims(const ConvGeom& g)
      : M((int64_t)g.N * g.Hz * g.Wz), ckk((int64_t)g.C * g.kh * g.kw), mk(M * g.K),
        img((int64_t)g.N * g.C * g.H * g.W), kc(ckk * g.K),
        parts(((M + kCB - 1) / kCB) * ((g.K + kCB - 1) / kCB)) {}
};

int check_reach(const ConvGeom& g) {
  const Dims d(g);
  if (d.M > INT32_MAX - kCB || (g.K + kCB - 1) / kCB > 65535 || (d.ckk + kCB - 1) / kCB > 65535)
    return fail(LASSO_ERR_UNSUPPORTED, "convolution problem too large");
  return LASSO_OK;
}

// r = conv_transpose2d(Ym, W) - x (x nullable) through COLS [M][C kh kw]
int synthesis(const double* Ym, const double* w, const double* x, double* cols, double* r, const ConvGeom& g,
              hipStream_t st) {
  const Dims d(g);
  LASSO_HIP_TRY(launch_gemm_plain(Ym, g.K, w, d.ckk, cols, d.ckk, (int)d.M, (int)d.ckk, g.K, st));
  hipLaunchKernelGGL(conv_residual_f64_kernel, dim3(grid_for(d.img)), dim3(256), 0, st, cols, x, r, g, d.img);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

template <int EPI>
int gradient(const ConvGradArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.M + kCB - 1) / kCB), (unsigned)((a.g.K + kCB - 1) / kCB));
  hipLaunchKernelGGL((conv_grad_prox_f64_kernel<EPI>), grid, dim3(256), 0, st, a);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

int relayout(const double* src, double* dst, double* dst2, const ConvGeom& g, int to_rows, hipStream_t st) {
  const Dims d(g);
  hipLaunchKernelGGL(conv_relayout_f64_kernel, dim3(grid_for(d.mk)), dim3(256), 0, st, src, dst, dst2, g.K, g.Hz * g.Wz,
                     d.mk, to_rows);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

struct ConvWs {
  double* Zm; double* Ym; double* COLS; double* R; double* dpart; double* delta; double* part; double* sums;
  double* Zc; double* Yc;       // (z, y) at the head of a speculated chunk of iterations
  size_t bytes;
};

ConvWs carve_conv(void* base, const ConvGeom& g) {
  const Dims d(g);
  ConvWs w;
  Arena a(base, 8);
  w.Zm = a.take<double>((size_t)d.mk * 8);
  w.Ym = a.take<double>((size_t)d.mk * 8);
  w.COLS = a.take<double>((size_t)d.M * d.ckk * 8);
  w.R = a.take<double>((size_t)d.img * 8);
  w.dpart = a.take<double>((size_t)d.parts * 8);
  w.delta = a.take<double>(64 * 8);
  w.part = a.take<double>((size_t)2 * kSumGrid * 8);
  w.sums = a.take<double>(256);
  w.Zc = a.take<double>((size_t)d.mk * 8);
  w.Yc = a.take<double>((size_t)d.mk * 8);
  w.bytes = a.bytes();
  return w;
}

// Slabs of the M rows of the weight gradient: at least 512 rows each, at most 64 slabs and 64 MiB of partial tiles.
// A function of the geometry alone, so that dW has the same bits on every device.
void wgrad_slabs(const ConvGeom& g, int* slabs, int* rows_per_slab) {
  const Dims d(g);
  const int64_t by_bytes = std::max<int64_t>(1, ((int64_t)64 << 20) / std::max<int64_t>(d.kc * 8, 1));
  const int64_t s = std::max<int64_t>(1, std::min<int64_t>({(d.M + 511) / 512, 64, by_bytes}));
  const int64_t rows = std::max<int64_t>(kCT, ((d.M + s - 1) / s + kCT - 1) / kCT * kCT);
  *rows_per_slab = (int)rows;
  *slabs = (int)std::max<int64_t>(1, (d.M + rows - 1) / rows);
}

struct ConvBwWs {
  double* zbA; double* zbB; double* yb; double* ub; double* gb; double* y;     // [M][K]
  double* R; double* RB;                                                       // r_i, rb [N][C][H][W]
  double* COLS; double* part;
  size_t bytes;
};

ConvBwWs carve_conv_bw(void* base, const ConvGeom& g) {
  const Dims d(g);
  ConvBwWs w;
  Arena a(base, 8);
  const size_t mk = (size_t)d.mk * 8, img = (size_t)d.img * 8;
  w.zbA = a.take<double>(mk); w.zbB = a.take<double>(mk); w.yb = a.take<double>(mk); w.ub = a.take<double>(mk);
  w.gb = a.take<double>(mk); w.y = a.take<double>(mk);
  w.R = a.take<double>(img); w.RB = a.take<double>(img);
  w.COLS = a.take<double>((size_t)d.M * d.ckk * 8);
  int slabs, rows;
  wgrad_slabs(g, &slabs, &rows);
  w.part = a.take<double>((size_t)slabs * d.kc * 8);
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t conv_workspace_bytes(const ConvGeom& g) { return carve_conv(nullptr, g).bytes; }
size_t conv_backward_workspace_bytes(const ConvGeom& g) { return carve_conv_bw(nullptr, g).bytes; }
size_t conv_lip_workspace_bytes(int64_t K, int64_t C, int sample) {
  return align_up((size_t)sample * 8) + align_up((size_t)std::min(K, C) * 8) + 256;
}

// The two products as another driver takes them (conv_lanczos.hip): the very launches conv_backward makes, one image or
// many.  img = conv_transpose2d(Ym, W) through cols [M][C kh kw]; G [M][K] = conv2d(img, W).
int launch_conv_synthesis(const double* Ym, const double* w, double* cols, double* img, const ConvGeom& g, hipStream_t st) {
  if (int s = check_reach(g)) return s;
  return synthesis(Ym, w, nullptr, cols, img, g, st);
}
int launch_conv_gradient(const double* img, const double* w, double* G, const ConvGeom& g, hipStream_t st) {
  if (int s = check_reach(g)) return s;
  const Dims d(g);
  const ConvGradArgs a{img, w, nullptr, G, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr, g, (int)d.M, (int)d.ckk};
  return gradient<EPI_ADD>(a, st);
}

// The stop rule (ista.py:44-46) is read once per chunk of speculated iterations (speculate_stop_rule);
// a stop inside a chunk restores the chunk's head and replays exactly the iterations up to the stop.  With a trace the
// count is fixed (no stop rule) and every iterate is kept.
int conv_solve(const double* x, const double* w, const double* z0, double* zout, const ConvGeom& g, double alpha, double lr,
               int fast, int maxiter, double tol, double* trace, int32_t* iters_out, double* last_delta_out,
               void* workspace, size_t ws_bytes, hipStream_t st) {
  const ConvWs ws = carve_conv(workspace, g);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (int s = check_reach(g)) return s;
  if (iters_out) *iters_out = 0;
  if (last_delta_out) *last_delta_out = NAN;
  if (g.N == 0) return LASSO_OK;
  const Dims d(g);
  if (z0) {
    if (int s = relayout(z0, ws.Zm, ws.Ym, g, 1, st)) return s;        // y0 = z0 in the same pass
  } else {
    LASSO_HIP_TRY(hipMemsetAsync(ws.Zm, 0, (size_t)d.mk * 8, st));
    LASSO_HIP_TRY(hipMemsetAsync(ws.Ym, 0, (size_t)d.mk * 8, st));
  }
  if (trace) LASSO_HIP_TRY(hipMemcpyAsync(trace, ws.Zm, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
  const bool stop = !trace && tol > 0.0 && maxiter > 0;
  const double budget = stop_budget<double>(d.M, g.K, tol);              // ista.py:16
  const double lam = alpha * lr;
  Momentum64 mom;
  int it = 0;
  auto iterate = [&](double* delta_slot) -> int {
    const double coef = mom.next(fast);                                   // :41-42
    if (int s = synthesis(ws.Ym, w, x, ws.COLS, ws.R, g, st)) return s;   // :19
    const ConvGradArgs a{ws.R, w, nullptr, nullptr, ws.Zm, ws.Ym, lr, lam, coef, ws.dpart, g, (int)d.M, (int)d.ckk};
    if (int s = gradient<EPI_PROX>(a, st)) return s;                      // :20, :29, :42, :44
    if (delta_slot) LASSO_HIP_TRY(launch_reduce_sets(ws.dpart, d.parts, 1, delta_slot, st));
    return LASSO_OK;
  };
  double last = NAN;
  if (!stop) {
    for (; it < maxiter; ++it) {
      if (int s = iterate(nullptr)) return s;
      if (trace)
        LASSO_HIP_TRY(hipMemcpyAsync(trace + (int64_t)(it + 1) * d.mk, ws.Zm, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
    }
  } else {
    auto save = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Zc, ws.Zm, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Yc, ws.Ym, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto restore = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Zm, ws.Zc, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Ym, ws.Yc, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto read = [&](double* host, int c) -> int { return read_back(host, ws.delta, sizeof(double) * c, st); };
    if (int s = speculate_stop_rule<double>(maxiter, budget, ws.delta, &mom.t, iterate, save, restore,
                                            [] { return (int)LASSO_OK; }, read, &it, &last, "lasso_conv_ista_solve_f64"))
      return s;
  }
  if (zout)
    if (int s = relayout(ws.Zm, zout, nullptr, g, 0, st)) return s;
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return LASSO_OK;
}

// (0.5 ||x - conv_transpose2d(z, W)||^2 + alpha ||z||_1) / N   (ista.py:23-26), double partials folded in a fixed order
int conv_objective(const double* x, const double* w, const double* z, const ConvGeom& g, double alpha, double* loss64,
                   float* loss32, void* workspace, size_t ws_bytes, hipStream_t st) {
  const ConvWs ws = carve_conv(workspace, g);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (int s = check_reach(g)) return s;
  const Dims d(g);
  if (int s = relayout(z, ws.Zm, nullptr, g, 1, st)) return s;
  if (int s = synthesis(ws.Zm, w, x, ws.COLS, ws.R, g, st)) return s;
  LASSO_HIP_TRY(launch_objective_sums(ws.R, d.img, ws.Zm, g.K, d.M, g.K, ws.part, alpha, (double)g.N, ws.sums, loss64,
                                      loss32, st));
  return LASSO_OK;
}

// Reverse pass of the unrolled solve, iteration i from the last to the first:
//     ub = [z_{i+1} != 0] zb_{i+1} ;  gb = -lr ub ;  rb = conv_transpose2d(gb, W)
//     yb_i = ub + conv2d(rb, W) ;  xb -= rb ;  dW += gb^T P(r_i) + y_i^T P(rb)
// Two syntheses and one add-epilogue gradient per iteration (one synthesis without grad_w).  No host synchronisation.
int conv_backward(const double* x, const double* w, const double* trace, const double* grad_z, const ConvGeom& g, double lr,
                  int fast, int iterations, double* gx, double* gw, double* gz0, void* workspace, size_t ws_bytes,
                  hipStream_t st) {
  const ConvBwWs ws = carve_conv_bw(workspace, g);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (int s = check_reach(g)) return s;
  const Dims d(g);
  if (gx && d.img > 0) LASSO_HIP_TRY(hipMemsetAsync(gx, 0, (size_t)d.img * 8, st));
  if (gw && (iterations == 0 || g.N == 0)) LASSO_HIP_TRY(hipMemsetAsync(gw, 0, (size_t)d.kc * 8, st));
  if (g.N == 0) return LASSO_OK;
  if (iterations == 0) {                       // z_T = z_0
    if (gz0) LASSO_HIP_TRY(hipMemcpyAsync(gz0, grad_z, (size_t)d.mk * 8, hipMemcpyDeviceToDevice, st));
    return LASSO_OK;
  }
  std::vector<double> coef(iterations);
  Momentum64 mom;
  for (int i = 0; i < iterations; ++i) coef[i] = mom.next(fast);
  int slabs, rows_per_slab;
  wgrad_slabs(g, &slabs, &rows_per_slab);
  double* zb_next = ws.zbA;
  double* zb_cur = ws.zbB;
  if (int s = relayout(grad_z, zb_next, nullptr, g, 1, st)) return s;
  LASSO_HIP_TRY(hipMemsetAsync(ws.yb, 0, (size_t)d.mk * 8, st));
  const unsigned eg = grid_for(d.mk);
  for (int i = iterations - 1; i >= 0; --i) {
    const double* z_next = trace + (int64_t)(i + 1) * d.mk;
    const double* z_i = trace + (int64_t)i * d.mk;
    hipLaunchKernelGGL(conv_bw_prox_f64_kernel, dim3(eg), dim3(256), 0, st, zb_next, zb_cur, ws.yb, z_next, ws.ub, ws.gb,
                       d.mk, coef[i], lr);
    LASSO_HIP_TRY(hipGetLastError());
    if (int s = synthesis(ws.gb, w, nullptr, ws.COLS, ws.RB, g, st)) return s;
    const ConvGradArgs a{ws.RB, w, ws.ub, ws.yb, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr, g, (int)d.M, (int)d.ckk};
    if (int s = gradient<EPI_ADD>(a, st)) return s;
    if (gw) {
      // the point of iteration i, y_i = z_i + c_{i-1} (z_i - z_{i-1}) (y_0 = z_0), and its residual r_i
      hipLaunchKernelGGL(conv_bw_point_f64_kernel, dim3(eg), dim3(256), 0, st, z_i,
                         (i > 0 && fast) ? trace + (int64_t)(i - 1) * d.mk : nullptr, ws.y, d.mk,
                         i > 0 ? coef[i - 1] : 0.0);
      LASSO_HIP_TRY(hipGetLastError());
      if (int s = synthesis(ws.y, w, x, ws.COLS, ws.R, g, st)) return s;
      const ConvWgradArgs wa{ws.gb, ws.y, ws.R, ws.RB, ws.part, g, (int)d.M, (int)d.ckk, rows_per_slab,
                             i != iterations - 1};
      hipLaunchKernelGGL(conv_wgrad_f64_kernel,
                         dim3((unsigned)((d.ckk + kCB - 1) / kCB), (unsigned)((g.K + kCB - 1) / kCB), (unsigned)slabs),
                         dim3(256), 0, st, wa);
      LASSO_HIP_TRY(hipGetLastError());
    }
    if (gx) {                                    // xb -= rb
      hipLaunchKernelGGL(conv_axpy_f64_kernel, dim3(grid_for(d.img)), dim3(256), 0, st, gx, ws.RB, -1.0, d.img);
      LASSO_HIP_TRY(hipGetLastError());
    }
    std::swap(zb_next, zb_cur);
  }
  if (gw) {
    hipLaunchKernelGGL(conv_wgrad_fold_f64_kernel, dim3(grid_for(d.kc)), dim3(256), 0, st, ws.part, slabs, d.kc, gw);
    LASSO_HIP_TRY(hipGetLastError());
  }
  if (gz0) {
    // z0b = zb_0 + yb_0 (y_0 = z_0), back to [N][K][Hz][Wz]
    hipLaunchKernelGGL(conv_axpy_f64_kernel, dim3(eg), dim3(256), 0, st, zb_next, ws.yb, 1.0, d.mk);
    LASSO_HIP_TRY(hipGetLastError());
    if (int s = relayout(zb_next, gz0, nullptr, g, 0, st)) return s;
  }
  return LASSO_OK;
}

int conv_lip_bound(const double* w, int64_t K, int64_t C, int ksize, int padding, int sample, int take_sqrt, double* l_out,
                   void* workspace, size_t ws_bytes, hipStream_t st) {
  if (ws_bytes < conv_lip_workspace_bytes(K, C, sample))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", conv_lip_workspace_bytes(K, C, sample));
  if (sample > 46340 || std::min(K, C) > INT32_MAX / 2 || std::max(K, C) > INT32_MAX / 2)
    return fail(LASSO_ERR_UNSUPPORTED, "bound too large");
  double* const freq = (double*)workspace;
  double* const maxes = (double*)((char*)workspace + align_up((size_t)sample * 8));
  double* const out = (double*)((char*)maxes + align_up((size_t)std::min(K, C) * 8));
  const int T = ksize * ksize;
  const bool swap = K > C;                       // the smaller channel dimension is summed last (:106-107)
  const int O = (int)(swap ? C : K), I = (int)(swap ? K : C);
  const int64_t so = swap ? T : (int64_t)C * T, si = swap ? (int64_t)C * T : T;
  hipLaunchKernelGGL(conv_lip_grid_f64_kernel, dim3(1), dim3(256), 0, st, freq, sample);
  hipLaunchKernelGGL(conv_lip_f64_kernel, dim3(O), dim3(256), 0, st, w, so, si, I, ksize, padding, freq, sample, maxes);
  hipLaunchKernelGGL(conv_lip_sum_f64_kernel, dim3(1), dim3(64), 0, st, maxes, O, take_sqrt, out);
  LASSO_HIP_TRY(hipGetLastError());
  if (l_out) return read_back(l_out, out, sizeof(double), st);
  return LASSO_OK;
}

}  // namespace f64
}  // namespace lasso
