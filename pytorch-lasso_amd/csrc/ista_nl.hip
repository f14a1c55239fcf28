// ISTA / FISTA through a one-layer decoder (the reference's lasso/nonlinear/ista.py:55-128 with
// decoder(z) = act(z W^T + b)) on the fp32 MFMA GEMM: the driver behind lasso_ista_nl_solve, and the entry points
// themselves.  min_z 0.5 |act(z W^T + b) - x|^2 + alpha |z|_1; everything the reference takes from autograd has a closed
// form for this family.  With u = y W^T + b, a = act(u):
//   gradient        g = ((a - x) act'(u)) W
//   Hessian (row i) H_i = W^T diag(c_i) W,   c = act'(u)^2 + (a - x) act''(u)
// Products (solver_common.hpp's gemm_kernel with an epilogue); u, a and g never exist in memory:
//   LinkEpi   y W^T on the accumulators: stores r = (a - x) act'(u), under lr = 'auto' also c; block partials of
//             sum (a - x)^2 when a loss is wanted (then nothing is stored: the loss is taken at z, not at y)
//   ProxEpi   r W on the accumulators: z_next = softshrink(y - t g, alpha t) with t a scalar or a per-row array, the
//             momentum point y_next, block partials of sum |z - z_next|; z and y are updated in place
//   HvLinkEpi v W^T on the accumulators: stores q = (s_row (v W^T)) c -- the row scale s is the normalisation
//             v / max(|v|, 1e-8) of the power iteration (F.normalize), folded in because the product is linear in v
//   HvOutEpi  q W on the accumulators: stores h = H v and the per-row, per-column-block sums of h^2 -- or, last, of
//             v_prev h, without a store
// lr = 'auto' (hessian_2norm, ista.py:26-52, on the rss term at the step's point y): u_0 = the caller's start vector,
// then a_t = H normalise(a_{t-1}) for t = 1 .. 2 power_iters + 1, L_i = normalise(a_{2P-1})_i . a_{2P+1}, t_i = 0.98 / L_i
// (torch's `0.98 / L`: the reciprocal times 0.98f).  rows_kernel folds a row's column-block sums in block order into
// the next scale (or L and t): [n] words, no pass over [n, k].  A row with H_i = 0 gets inf / NaN; nothing is repaired.
//
// The stop rule (ista.py:108-110) runs through speculate_stop_rule (stoprule_host.hpp): one host read per chunk of
// speculated iterations, none with tol <= 0 and no trace.  Every sum: per thread, wave, block partial in double, then
// ONE workgroup in a fixed order -- no float atomics, two solves of the same arguments are bitwise equal.
#include "linesearch_host.hpp"
#include "solver_common.hpp"
#include "stoprule_host.hpp"

namespace lasso {
namespace ista_nl {
namespace {

using namespace solver;

constexpr int kSlots = 64;            // iterations of a speculated chunk (speculate_stop_rule's kChunkMax)
constexpr float kNormEps = 1e-8f;     // F.normalize(..., eps=1e-8), ista.py:45-48

// what an iteration leaves for the host: one record per chunk
struct Slots {
  float delta[kSlots];                // sum |z - z_next|
  double f[kSlots];                   // the objective of z_next (trace->loss == 2)
  double f_edge[2];                   // the objective of z0 and of the returned z
};

// a(u), a'(u), a''(u).  Sigmoid and tanh from e = exp(-|u|) / exp(-2 |u|) <= 1 alone: no logit overflows.
__device__ __forceinline__ void activation(int act, float u, float& a, float& d1, float& d2) {
  if (act == LASSO_ACT_SIGMOID) {
    const float e = expf(-fabsf(u));
    const float den = __fadd_rn(1.0f, e);
    a = __fdiv_rn(u >= 0.0f ? 1.0f : e, den);
    const float om = __fdiv_rn(u >= 0.0f ? e : 1.0f, den);        // 1 - a
    d1 = __fmul_rn(a, om);
    d2 = __fmul_rn(d1, __fsub_rn(om, a));
  } else if (act == LASSO_ACT_TANH) {
    const float e = expf(__fmul_rn(-2.0f, fabsf(u)));
    const float den = __fadd_rn(1.0f, e);
    a = copysignf(__fdiv_rn(__fsub_rn(1.0f, e), den), u);
    d1 = __fdiv_rn(__fmul_rn(4.0f, e), __fmul_rn(den, den));
    d2 = __fmul_rn(__fmul_rn(-2.0f, a), d1);
  } else if (act == LASSO_ACT_RELU) {
    a = u > 0.0f ? u : (u != u ? u : 0.0f);                         // (torch's relu keeps a NaN)
    d1 = u > 0.0f ? 1.0f : 0.0f;                                    // torch's subgradient: 0 at 0
    d2 = 0.0f;
  } else {
    a = u;
    d1 = 1.0f;
    d2 = 0.0f;
  }
}

// byte offset of the tile's row of register rg of row block mi in a per-row array that starts at the tile's first row
template <int BM, int BN>
__device__ __forceinline__ unsigned row_off(const Tile<BM, BN>& t, int mi, int rg) {
  const int rl = (BM / 2) * t.wr + 16 * mi + 4 * t.q + rg;
  return rl < t.rows_valid ? (unsigned)rl * 4u : Tile<BM, BN>::kOutside;
}
template <int BM, int BN>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const Tile<BM, BN>& t, const float* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + t.i0), 0, t.rows_valid * 4, 0x00020000);
}
// ... of the column of fragment nj in a per-column array of nn words
template <int BM, int BN>
__device__ __forceinline__ unsigned col_off(const Tile<BM, BN>& t, int nj) {
  const int cc = t.j0 + (BN / 2) * t.wc + 16 * nj + t.l15;
  return cc < t.nn ? (unsigned)cc * 4u : Tile<BM, BN>::kOutside;
}

// y W^T -> r = (a - x) a'(u) [and c = a'(u)^2 + (a - x) a''(u)], u = y W^T + b; block partials {sum (a - x)^2}
struct LinkEpi {
  const float* X; int64_t ldx;        // the targets x [m][nn]
  const float* bias;                  // [nn], nullable
  float* R;                           // r (ld nn), nullable: the loss alone
  float* Cc;                          // c (ld nn), nullable
  double* part;                       // [blocks][kPart], nullable
  int64_t a_stride;
  int act;

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t xrs = t.rsrc(X, ldx);
    __amdgpu_buffer_rsrc_t rrs = xrs, crs = xrs;
    if (R) rrs = t.rsrc(R, ldn);
    if (Cc) crs = t.rsrc(Cc, ldn);
    float b[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) b[nj] = 0.0f;
    if (bias) {
      const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, t.nn * 4, 0x00020000);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) b[nj] = t.ld32(brs, col_off(t, nj));
    }
    double s[1] = {0.0};
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float x[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) x[nj][rg] = t.ld32(xrs, t.off(mi, nj, rg, ldx));
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const float u = bias ? __fadd_rn(acc[mi][nj][rg], b[nj]) : acc[mi][nj][rg];
          float a, d1, d2;
          activation(act, u, a, d1, d2);
          const float diff = __fsub_rn(a, x[nj][rg]);
          if (part && t.inside(o[nj][rg])) s[0] += (double)__fmul_rn(diff, diff);
          if (R) t.st32(__fmul_rn(diff, d1), rrs, o[nj][rg]);
          if (Cc) t.st32(__fadd_rn(__fmul_rn(d1, d1), __fmul_rn(diff, d2)), crs, o[nj][rg]);
        }
    }
    if (part) {                                                     // (uniform over the launch)
      float nomax[1] = {0.0f};
      block_fold<1, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(part));
    }
  }
};

// torch's relu: a NaN stays
__device__ __forceinline__ float relu_keep_nan(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

// r W = g -> z_next = softshrink(y - t g, alpha t) (ista.py:21-23,95), y_next (:114); block partials {sum |z - z_next|}
struct ProxEpi {
  float* Z;                           // z [m][nn], ld nn: read, then z_next
  float* Y;                           // y: read, then y_next (z_next without momentum)
  const float* Trow;                  // the rows' steps t_i [m], nullable: `step` for every row
  double* part;                       // [blocks][kPart]
  int64_t a_stride;
  float step, thresh;                 // fixed step: (float)lr and (float)(alpha lr)
  float alpha;
  float coef;                         // (t_k - 1) / t_{k+1}
  int fast;

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t zrs = t.rsrc(Z, ldn), yrs = t.rsrc(Y, ldn);
    __amdgpu_buffer_rsrc_t trs = zrs;
    if (Trow) trs = row_rsrc(t, Trow);
    double s[1] = {0.0};
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float tt[4], th[4];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        tt[rg] = Trow ? t.ld32(trs, row_off(t, mi, rg)) : step;
        th[rg] = Trow ? __fmul_rn(alpha, tt[rg]) : thresh;
      }
      float z[NJ][4], y[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          z[nj][rg] = t.ld32(zrs, o[nj][rg]);
          y[nj][rg] = t.ld32(yrs, o[nj][rg]);
        }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const float v = __fsub_rn(y[nj][rg], __fmul_rn(tt[rg], acc[mi][nj][rg]));
          const float sg = (v > 0.0f ? 1.0f : 0.0f) - (v < 0.0f ? 1.0f : 0.0f);
          const float zn = __fmul_rn(sg, relu_keep_nan(__fsub_rn(fabsf(v), th[rg])));
          if (t.inside(o[nj][rg])) s[0] += (double)fabsf(__fsub_rn(z[nj][rg], zn));
          const float yn = fast ? __fadd_rn(zn, __fmul_rn(coef, __fsub_rn(zn, z[nj][rg]))) : zn;
          t.st32(zn, zrs, o[nj][rg]);
          t.st32(yn, yrs, o[nj][rg]);
        }
    }
    float nomax[1] = {0.0f};
    block_fold<1, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(part));
  }
};

// v W^T -> q = (s_row (v W^T)) c
struct HvLinkEpi {
  const float* Cc;                    // c [m][nn], ld nn
  const float* scale;                 // the rows' 1 / max(|v|, 1e-8) [m]
  float* Q;                           // q (ld nn)
  int64_t a_stride;

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char*) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t crs = t.rsrc(Cc, ldn), qrs = t.rsrc(Q, ldn), srs = row_rsrc(t, scale);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float sc[4], c[NJ][4];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) sc[rg] = t.ld32(srs, row_off(t, mi, rg));
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) c[nj][rg] = t.ld32(crs, o[nj][rg]);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          t.st32(__fmul_rn(__fmul_rn(acc[mi][nj][rg], sc[rg]), c[nj][rg]), qrs, o[nj][rg]);
    }
  }
};

// q W = h -> h stored and the rows' sums of h^2 over this block's columns; or (Vp) the rows' sums of v_prev h, no store.
// rowpart [m][gridDim.x]: row i's sum over column block blockIdx.x
struct HvOutEpi {
  float* H;                           // h (ld nn), nullable
  const float* Vp;                    // v_prev (ld nn), nullable
  double* rowpart;
  int64_t a_stride;

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t hrs = t.rsrc(H ? H : Vp, ldn);
    double (*rows)[2] = reinterpret_cast<double (*)[2]>(smem);      // [BM][2]: the two column halves of the block
    __syncthreads();                                                // (the main loop's last reads of the LDS)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float vp[NJ][4];
      if (Vp) {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) vp[nj][rg] = t.ld32(hrs, o[nj][rg]);
      }
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        double s = 0.0;
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
          const float h = acc[mi][nj][rg];
          if (t.inside(o[nj][rg])) s += (double)__fmul_rn(Vp ? vp[nj][rg] : h, h);
          if (!Vp) t.st32(h, hrs, o[nj][rg]);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);       // the 16 lanes that share the row
        if (t.l15 == 0) rows[(BM / 2) * t.wr + 16 * mi + 4 * t.q + rg][t.wc] = s;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < t.rows_valid && (int)threadIdx.x < BM)
      rowpart[(int64_t)(t.i0 + threadIdx.x) * gridDim.x + blockIdx.x] = rows[threadIdx.x][0] + rows[threadIdx.x][1];
  }
};

// a row's column-block sums, in block order.  mode 0: scale_out = 1 / max(sqrt(sum), 1e-8); mode 1: L = scale_prev sum,
// t = (1 / L) 0.98f (torch's `0.98 / L` is L.reciprocal() * 0.98)
__global__ __launch_bounds__(256) void rows_kernel(const double* __restrict__ rowpart, int nbx, int n, int mode,
                                                   const float* __restrict__ scale_prev, float* __restrict__ scale_out,
                                                   float* __restrict__ L, float* __restrict__ T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int b = 0; b < nbx; ++b) a += rowpart[(int64_t)i * nbx + b];
  if (mode == 0) {
    scale_out[i] = __fdiv_rn(1.0f, fmaxf(sqrtf((float)a), kNormEps));
  } else {
    const float l = __fmul_rn(scale_prev[i], (float)a);
    L[i] = l;
    T[i] = __fmul_rn(__fdiv_rn(1.0f, l), 0.98f);
  }
}

// scale[i] = 1 / max(|U_i|, 1e-8) of the rows of U [n][k] (pitch ld): one workgroup per row, a fixed order
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ U, int64_t ld, int k, float* __restrict__ scale) {
  __shared__ double red[256];
  const float* const row = U + (int64_t)blockIdx.x * ld;
  double a = 0.0;
  for (int j = threadIdx.x; j < k; j += 256) a += (double)__fmul_rn(row[j], row[j]);
  red[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) scale[blockIdx.x] = __fdiv_rn(1.0f, fmaxf(sqrtf((float)red[0]), kNormEps));
}

// *slot = sum |z - z_next| of the iteration, as a float32 like the reference's tensor
__global__ __launch_bounds__(256) void delta_kernel(const double* __restrict__ part, int nb, float* __restrict__ slot) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) *slot = (float)a[0];
}

// block partials {sum |z|} of Z, packed
__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ Z, int64_t total, double* __restrict__ part) {
  __shared__ double red[32];
  double s[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) s[0] += (double)fabsf(Z[i]);
  float nomax[1] = {0.0f};
  block_fold<1, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// *out = 0.5 sum (a - x)^2 + alpha sum |z|
__global__ __launch_bounds__(256) void loss_kernel(const double* __restrict__ part_r, int nb_r, const double* __restrict__ part_z,
                                                   int nb_z, double alpha, double* __restrict__ out) {
  __shared__ double red[256], a[kPart], b[kPart];
  fold_partials(part_r, nb_r, 1, 0, red, a);
  fold_partials(part_z, nb_z, 1, 0, red, b);
  if (threadIdx.x == 0) *out = 0.5 * a[0] + alpha * b[0];
}

struct Space {
  float *Wt, *Z, *Y, *Zc, *Yc, *R, *Cc, *Q, *V[2], *S0, *Sc[2], *L, *T;
  double *part_d, *part_k, *part_z, *rowpart;
  Slots* slots;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k, bool lr_auto) {
  Space w = {};
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4, nrow = (size_t)n * 4;
  w.Wt = a.take((size_t)k * d * 4);
  w.Z = a.take(nk);
  w.Y = a.take(nk);
  w.Zc = a.take(nk);
  w.Yc = a.take(nk);
  w.R = a.take(nd);
  // block partials: 64 x 64 blocks give the most
  w.part_d = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8);
  w.part_k = a.take<double>((size_t)gemm_parts((int)n, (int)k, 64) * kPart * 8);
  w.part_z = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.slots = a.take<Slots>(sizeof(Slots));
  if (lr_auto) {
    w.Cc = a.take(nd);
    w.Q = a.take(nd);
    for (int b = 0; b < 2; ++b) w.V[b] = a.take(nk);
    w.S0 = a.take(nrow);
    for (int b = 0; b < 2; ++b) w.Sc[b] = a.take(nrow);
    w.L = a.take(nrow);
    w.T = a.take(nrow);
    w.rowpart = a.take<double>((size_t)n * (size_t)((k + 63) / 64) * 8);
  }
  w.bytes = a.bytes();
  return w;
}

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* z0, int64_t ldz0, float* zout,
          int64_t ldz, const float* u0, int64_t ldu0, int64_t n64, int64_t d64, int64_t k64, double alpha, int act,
          const lasso_ista_nl_options& o, lasso_ista_nl_result* res, lasso_ista_nl_trace* tr, void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const bool lr_auto = o.lr_auto != 0, fast = o.fast != 0;
  const Space ws = carve(workspace, n, d, k, lr_auto);
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw, lr_auto ? ldu0 : 0});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  const bool force128 = (o.reserved & 1) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // products [n,d]
  const int pk = gemm_parts(n, k, side_k), pd = gemm_parts(n, d, side_d);
  const int nbx = (k + side_k - 1) / side_k;
  const int64_t nk = (int64_t)n * k;
  const int gk = ew_grid(nk);
  const int loss_mode = tr ? tr->loss : 0;

  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));
  hipLaunchKernelGGL(init_packed_kernel<>, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipMemcpyAsync(ws.Y, ws.Z, (size_t)nk * 4, hipMemcpyDeviceToDevice, st));
  if (lr_auto) {
    hipLaunchKernelGGL(row_norm_kernel, dim3(n), dim3(256), 0, st, u0, ldu0, k, ws.S0);
    LASSO_HIP_TRY(hipGetLastError());
  }

  // the objective of the z in ws.Z -> *out (device)
  auto loss = [&](double* out) -> int {
    LinkEpi el = {};
    el.X = x; el.ldx = ldx; el.bias = bias; el.part = ws.part_d; el.act = act;
    LASSO_HIP_TRY(launch_gemm(ws.Z, k, w, ldw, n, d, k, el, side_d, 1, st));
    hipLaunchKernelGGL(l1_kernel, dim3(gk), dim3(256), 0, st, ws.Z, nk, ws.part_z);
    LASSO_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, st, ws.part_d, pd, ws.part_z, gk, alpha, out);
    LASSO_HIP_TRY(hipGetLastError());
    return LASSO_OK;
  };
  // hessian_2norm at the point whose c is in ws.Cc: the rows' L and t = 0.98 / L
  auto power = [&]() -> int {
    const int last = 2 * o.power_iters + 1;
    for (int t = 1; t <= last; ++t) {
      HvLinkEpi e1 = {};
      e1.Cc = ws.Cc; e1.Q = ws.Q; e1.scale = t == 1 ? ws.S0 : ws.Sc[(t - 1) & 1];
      if (t == 1) LASSO_HIP_TRY(launch_gemm(u0, ldu0, w, ldw, n, d, k, e1, side_d, 1, st));
      else LASSO_HIP_TRY(launch_gemm(ws.V[(t - 1) & 1], k, w, ldw, n, d, k, e1, side_d, 1, st));
      HvOutEpi e2 = {};
      e2.rowpart = ws.rowpart;
      if (t < last) e2.H = ws.V[t & 1];
      else e2.Vp = ws.V[1];                                     // a_{2P-1}: the v of the last round
      LASSO_HIP_TRY(launch_gemm(ws.Q, d, ws.Wt, d, n, k, d, e2, side_k, 1, st));
      hipLaunchKernelGGL(rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws.rowpart, nbx, n, t < last ? 0 : 1, ws.Sc[1],
                         ws.Sc[t & 1], ws.L, ws.T);
      LASSO_HIP_TRY(hipGetLastError());
    }
    return LASSO_OK;
  };

  Momentum mom;
  const float step = (float)o.lr, thresh = (float)(alpha * o.lr);
  int queued = 0;                                             // iterations of the chunk in flight: the slot of the next one
  auto iterate = [&](float* slot) -> int {
    const float coef = mom.next(fast);
    LinkEpi e1 = {};
    e1.X = x; e1.ldx = ldx; e1.bias = bias; e1.R = ws.R; e1.Cc = lr_auto ? ws.Cc : nullptr; e1.act = act;
    LASSO_HIP_TRY(launch_gemm(ws.Y, k, w, ldw, n, d, k, e1, side_d, 1, st));
    if (lr_auto)
      if (int s = power()) return s;
    ProxEpi e2 = {};
    e2.Z = ws.Z; e2.Y = ws.Y; e2.Trow = lr_auto ? ws.T : nullptr; e2.part = ws.part_k; e2.step = step; e2.thresh = thresh;
    e2.alpha = (float)alpha; e2.coef = coef; e2.fast = fast ? 1 : 0;
    LASSO_HIP_TRY(launch_gemm(ws.R, d, ws.Wt, d, n, k, d, e2, side_k, 1, st));
    if (slot) {
      hipLaunchKernelGGL(delta_kernel, dim3(1), dim3(256), 0, st, ws.part_k, pk, ws.slots->delta + queued);
      LASSO_HIP_TRY(hipGetLastError());
      if (loss_mode > 1)
        if (int s = loss(ws.slots->f + queued)) return s;
      ++queued;
    }
    return LASSO_OK;
  };

  if (loss_mode > 0)
    if (int s = loss(ws.slots->f_edge)) return s;

  Slots host;
  int it = 0, stopped = 0;
  float last = NAN;
  // the sums (and objectives) of the chunk's iterations `first` .. into the trace
  auto record = [&](int first, int c) {
    if (!tr) return;
    for (int j = 0; j < c && first + j < tr->capacity; ++j) {
      if (tr->deltas) tr->deltas[first + j] = (double)host.delta[j];
      if (tr->f && loss_mode > 1) tr->f[first + j] = host.f[j];
    }
  };
  if (!(o.tol > 0.0)) {
    // the rule cannot fire: no host read -- but for a trace, then one per kSlots iterations
    while (it < o.maxiter) {
      const int c = std::min(kSlots, o.maxiter - it);
      queued = 0;
      for (int j = 0; j < c; ++j)
        if (int s = iterate(tr ? ws.slots->delta : nullptr)) return s;
      if (tr) {
        if (int s = read_back(&host, ws.slots, sizeof(Slots), st)) return s;
        record(it, c);
        last = host.delta[c - 1];
      }
      it += c;
    }
  } else {
    const float budget = stop_budget<float>(n, k, o.tol);
    const size_t words = (size_t)nk * 4;
    int done = 0;                                             // iterations behind the chunk in flight
    auto save = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Zc, ws.Z, words, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Yc, ws.Y, words, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto restore = [&]() -> int {
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Z, ws.Zc, words, hipMemcpyDeviceToDevice, st));
      LASSO_HIP_TRY(hipMemcpyAsync(ws.Y, ws.Yc, words, hipMemcpyDeviceToDevice, st));
      return LASSO_OK;
    };
    auto read = [&](float* sums, int c) -> int {
      if (int s = read_back(&host, ws.slots, sizeof(Slots), st)) return s;
      memcpy(sums, host.delta, sizeof(float) * c);
      const int hit = first_stop<float>(sums, c, budget);
      record(done, hit < 0 ? c : hit + 1);
      done += hit < 0 ? c : hit + 1;
      if (hit >= 0) stopped = 1;
      queued = 0;
      return LASSO_OK;
    };
    if (int s = speculate_stop_rule<float>(o.maxiter, budget, ws.slots->delta, &mom.t, iterate, save, restore,
                                           [] { return (int)LASSO_OK; }, read, &it, &last, "lasso_ista_nl_solve"))
      return s;
  }
  if (loss_mode > 0)
    if (int s = loss(ws.slots->f_edge + 1)) return s;
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, ws.Z, zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  if (lr_auto && res->l_dev && it > 0)
    LASSO_HIP_TRY(hipMemcpyAsync(res->l_dev, ws.L, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  if (loss_mode > 0) {
    if (int s = read_back(&host, ws.slots, sizeof(Slots), st)) return s;
    res->f0 = host.f_edge[0];
    res->f_final = host.f_edge[1];
  }
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  res->n_iter = it;
  res->stopped = stopped;
  res->last_delta = last;
  return LASSO_OK;
}

}  // namespace
}  // namespace ista_nl
}  // namespace lasso

using lasso::fail;

extern "C" {

size_t lasso_ista_nl_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int auto_lr) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return 0;
  return lasso::ista_nl::carve(nullptr, n, d, k, auto_lr != 0).bytes + 256;
}

int lasso_ista_nl_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* bias_dev, const void* z0_dev,
                        int64_t ldz0, void* z_out_dev, int64_t ldz, const void* u0_dev, int64_t ldu0, int64_t n, int64_t d,
                        int64_t k, int dtype, double alpha, int activation, const lasso_ista_nl_options* o,
                        lasso_ista_nl_result* res, lasso_ista_nl_trace* trace, void* workspace_dev, size_t workspace_bytes,
                        void* stream) {
  if (activation < LASSO_ACT_IDENTITY || activation > LASSO_ACT_RELU)
    return fail(LASSO_ERR_UNSUPPORTED, "ista_nl: activation %d (LASSO_ACT_IDENTITY .. LASSO_ACT_RELU only)", activation);
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "ista_nl: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (o->maxiter < 0) return fail(LASSO_ERR_BAD_ARG, "maxiter < 0");
  if (o->reserved & ~(int64_t)1) return fail(LASSO_ERR_BAD_ARG, "ista_nl: undefined bit of options.reserved");
  if (o->lr_auto && o->power_iters < 1) return fail(LASSO_ERR_BAD_ARG, "ista_nl: power_iters < 1 with lr_auto");
  if (o->lr_auto && o->power_iters > (1 << 20)) return fail(LASSO_ERR_BAD_ARG, "ista_nl: power_iters > 2^20");
  if (trace && (trace->capacity < 0 || trace->loss < 0 || trace->loss > 2 ||
                (trace->capacity > 0 && trace->loss > 1 && !trace->f)))
    return fail(LASSO_ERR_BAD_ARG, "ista_nl: trace with a negative capacity, an unknown loss mode or a null array");
  res->n_iter = res->stopped = 0;
  res->last_delta = res->f0 = res->f_final = NAN;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (o->lr_auto && !u0_dev) return fail(LASSO_ERR_BAD_ARG, "ista_nl: lr_auto needs the start vector u0");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k || (o->lr_auto && ldu0 < k))
    return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  const size_t need = lasso_ista_nl_workspace_bytes(n, d, k, dtype, o->lr_auto);
  if (workspace_bytes < need) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", need);
  return lasso::ista_nl::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)bias_dev, (const float*)z0_dev,
                               ldz0, (float*)z_out_dev, ldz, (const float*)u0_dev, ldu0, n, d, k, alpha, activation, *o, res,
                               trace, workspace_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
