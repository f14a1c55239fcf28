// Orthant-wise Newton (the reference's lasso/linear/solvers/orthant_wise_newton.py) on the fp32 MFMA GEMM: the driver
// behind lasso_own_solve.  min 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch with the explicit Hessian
// W^T W + 1e-4 I, whose inverse is one k x k matrix for the whole batch (computed once, in double, rounded once).
//
// Every product is the main loop of gemm.hip (gemm_mainloop.hpp) with an epilogue of its own, as in gpsr_driver.hpp:
//   EPI_RESID  resid = z W^T - x stored, block partials of |resid|^2
//   EPI_PGRAD  g = resid W on the accumulators; reads z, stores v = -pseudo-gradient, block partials of sum |z|
//   EPI_DIR    d = project(v Hinv^T, v) stored
//   EPI_TRIAL  |z_t W^T - x|^2 of the candidates z_t (blockIdx.z = rung): block partials only, the [n,d] product of a
//              trial never reaches memory
// and around them trial_kernel (z_t = project(z + t d, eta) for each rung's t, partials of sum |z_t|, <v, z_t - z>,
// |z_t - z|^2), decide_kernel (ONE workgroup folds the partials in a fixed order in double: f(t) as a double, and the
// backtracking verdicts in the reference's fp32 operation order) and accept_kernel (the accepted candidate becomes z).
// eta = where(z == 0, sign(v), sign(z)) is never stored: trial_kernel recomputes it from z and v.  No float atomics: two
// solves of the same arguments are bitwise equal.  One line-search evaluation is trial_kernel + the TRIAL product +
// decide_kernel and one host read of the control block; a backtracking ladder evaluates kRungs step sizes per read.
#include "gpsr_driver.hpp"
#include "brent_host.hpp"

namespace lasso {
namespace own {
namespace {

using gemm_detail::f32x4;
using gpsr::block_fold;
using gpsr::block_side;
using gpsr::device_cus;
using gpsr::ew_grid;
using gpsr::fold_partials;
using gpsr::gemm_parts;
using gpsr::kEwBlocks;
using gpsr::kPart;

constexpr int kRungs = 8;             // step sizes of a backtracking ladder per host read
constexpr double kShift = 1e-4;       // the reference's hess.diagonal().add_(1e-4)

enum { EPI_RESID = 0, EPI_PGRAD, EPI_DIR, EPI_TRIAL };

// control block (device; the host reads it once per decision)
struct Ctl {
  double f;                           // objective of the current z, folded in double
  double rr, l1;                      // its |resid|^2 and |z|_1
  double dz2;                         // |z+ - z|^2 of the accepted candidate
  double ft[kRungs];                  // objective of each rung of the last batch
  double dzt[kRungs];                 // |z_t - z|^2 of each rung
  float fnew[kRungs], bound[kRungs];  // backtracking: the reference's fp32 f+ and f - tol <v, z+ - z>
  float f32;                          // the objective in the reference's fp32 operation order (the backtracking's f)
  int accept;                         // rung of the last batch that was accepted, -1: none
  int bad, pad;                       // a non-finite f+ before any rung held
};

struct Steps { float t[kRungs]; };

struct Epi {
  const float* X; int64_t ldx;        // RESID / TRIAL: the data x [m][nn]
  const float* Z;                     // PGRAD: the code z (ld nn)
  const float* V;                     // DIR: v (ld nn)
  float* Out;                         // RESID: resid, PGRAD: v, DIR: d (ld nn)
  int64_t a_stride;                   // TRIAL: per rung offset of the A operand
  double* part;                       // [rungs][blocks][kPart]
  float alpha;
};

// u where it has the sign of w, a literal zero elsewhere (the reference's project(); sign(0) = 0 on both sides)
__device__ __forceinline__ float keep_sign(float u, bool w_pos, bool w_neg) {
  return ((u > 0.0f && w_pos) || (u < 0.0f && w_neg)) ? u : 0.0f;
}

// C = A B^T on the block (blockIdx.y, blockIdx.x), rung blockIdx.z; A [m][kk], B [nn][kk]
template <int BM, int BN, bool VEC, bool DMA, int MODE>
__global__ __launch_bounds__(256, 2) void own_gemm_kernel(const float* __restrict__ A, int64_t lda,
                                                          const float* __restrict__ B, int64_t ldb, int m, int nn,
                                                          int kk, Epi ep) {
  constexpr int MI = BM / 32, NJ = BN / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int i0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int l15 = lane & 15, q = lane >> 4;
  A += (int64_t)blockIdx.z * ep.a_stride;
  f32x4 acc[MI][NJ] = {};
  gemm_detail::gemm_nt_accumulate<BM, BN, VEC, DMA>(A, lda, B, ldb, m, nn, kk, i0, j0, smem, acc);
  // the epilogue's operands through buffer descriptors of the tile's rows, as in gpsr_gemm_kernel: out of range reads 0
  // and drops the store
  const int rows_valid = min(BM, m - i0);
  auto tile_rsrc = [&](const float* base, int64_t ld) {
    const int64_t bytes = (int64_t)rows_valid * ld * 4;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (int64_t)i0 * ld), 0,
                                             (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff), 0x00020000);
  };
  auto tile_off = [&](int rl, int cc, int64_t ld) {
    unsigned o = (rl < rows_valid && cc < nn) ? (unsigned)(rl * (int)ld + cc) * 4u : 0xfffffff0u;
    asm volatile("" : "+v"(o));
    return o;
  };
  auto ld32 = [](__amdgpu_buffer_rsrc_t rs, unsigned o) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0));
  };
  auto st32 = [](float v, __amdgpu_buffer_rsrc_t rs, unsigned o) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, o, 0, 0);
  };
  float s0 = 0.0f;
  const int64_t ldn = nn;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    unsigned o[NJ][4];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg)
        o[nj][rg] = tile_off((BM / 2) * wr + 16 * mi + 4 * q + rg, j0 + (BN / 2) * wc + 16 * nj + l15, ldn);
    if constexpr (MODE == EPI_RESID || MODE == EPI_TRIAL) {
      const __amdgpu_buffer_rsrc_t xrs = tile_rsrc(ep.X, ep.ldx);
      float x[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          x[nj][rg] = ld32(xrs, tile_off((BM / 2) * wr + 16 * mi + 4 * q + rg, j0 + (BN / 2) * wc + 16 * nj + l15, ep.ldx));
      __amdgpu_buffer_rsrc_t ors = xrs;
      if constexpr (MODE == EPI_RESID) ors = tile_rsrc(ep.Out, ldn);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {       // (the LDS-DMA form clamps rows beyond the operand instead of zeroing them)
          const float r = __fsub_rn(acc[mi][nj][rg], x[nj][rg]);
          if (o[nj][rg] != 0xfffffff0u) s0 += __fmul_rn(r, r);
          if constexpr (MODE == EPI_RESID) st32(r, ors, o[nj][rg]);
        }
    } else if constexpr (MODE == EPI_PGRAD) {
      const __amdgpu_buffer_rsrc_t zrs = tile_rsrc(ep.Z, ldn), ors = tile_rsrc(ep.Out, ldn);
      float z[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) z[nj][rg] = ld32(zrs, o[nj][rg]);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          // pseudo_grad(), orthant_wise_newton.py:10-17: the right derivative if it is negative, the left if it is
          // positive, else 0
          const float zz = z[nj][rg], g = acc[mi][nj][rg];
          const float sg = zz > 0.0f ? ep.alpha : (zz < 0.0f ? -ep.alpha : 0.0f);      // alpha * sign(z)
          const float right = __fadd_rn(g, zz == 0.0f ? ep.alpha : sg);
          const float left = __fadd_rn(g, zz == 0.0f ? -ep.alpha : sg);
          float pg = 0.0f;
          if (right < 0.0f) pg = right;
          if (left > 0.0f) pg = left;
          if (o[nj][rg] != 0xfffffff0u) s0 += fabsf(zz);
          st32(-pg, ors, o[nj][rg]);
        }
    } else {                                   // EPI_DIR
      const __amdgpu_buffer_rsrc_t vrs = tile_rsrc(ep.V, ldn), ors = tile_rsrc(ep.Out, ldn);
      float v[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) v[nj][rg] = ld32(vrs, o[nj][rg]);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          st32(keep_sign(acc[mi][nj][rg], v[nj][rg] > 0.0f, v[nj][rg] < 0.0f), ors, o[nj][rg]);
    }
  }
  if constexpr (MODE != EPI_DIR) {
    double s[1] = {(double)s0};
    float nomax[1] = {0.0f};
    double* const out = ep.part + ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kPart;
    block_fold<1, 0>(s, nomax, reinterpret_cast<double*>(smem), out);
  }
}

// z = z0 (pitch ld0), packed
__global__ __launch_bounds__(256) void init_kernel(const float* __restrict__ S, int64_t ld0, float* __restrict__ Z, int n, int k) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    Z[i] = S[(i / k) * ld0 + (i % k)];
}

// candidates of the rungs blockIdx.y: z_t = project(z + t d, eta); partials {sum |z_t|, <v, z_t - z>, |z_t - z|^2}
__global__ __launch_bounds__(256) void trial_kernel(const float* __restrict__ Z, const float* __restrict__ V,
                                                    const float* __restrict__ D, float* __restrict__ Zc, int64_t total,
                                                    Steps steps, double* __restrict__ part) {
  __shared__ double red[32];
  const float t = steps.t[blockIdx.y];
  float* const zc = Zc + (int64_t)blockIdx.y * total;
  double s[3] = {0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float z = Z[i], v = V[i];
    const bool e_pos = z > 0.0f || (z == 0.0f && v > 0.0f), e_neg = z < 0.0f || (z == 0.0f && v < 0.0f);
    const float zt = keep_sign(__fmaf_rn(t, D[i], z), e_pos, e_neg);
    const float dz = __fsub_rn(zt, z);
    zc[i] = zt;
    s[0] += (double)fabsf(zt);
    s[1] += (double)__fmul_rn(v, dz);
    s[2] += (double)__fmul_rn(dz, dz);
  }
  block_fold<3, 0>(s, nomax, red, part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kPart);
}

// f = 0.5 |resid|^2 + alpha |z|_1 of the current z, from the partials RESID and PGRAD left
__global__ __launch_bounds__(256) void eval_kernel(const double* __restrict__ part_r, int nb_r, const double* __restrict__ part_p,
                                                   int nb_p, double alpha, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], b[kPart];
  fold_partials(part_r, nb_r, 1, 0, red, a);
  fold_partials(part_p, nb_p, 1, 0, red, b);
  if (threadIdx.x == 0) {
    ctl->rr = a[0];
    ctl->l1 = b[0];
    ctl->f = 0.5 * a[0] + alpha * b[0];
    ctl->f32 = __fadd_rn(__fmul_rn(0.5f, (float)a[0]), __fmul_rn((float)alpha, (float)b[0]));
  }
}

// the objective of `count` rungs (product != 0: part_r holds |z_t W^T - x|^2) and, for a backtracking, the
// sufficient-decrease test in the reference's order (orthant_wise_newton.py:23): the first rung with
// f+ <= f - tol <v, z+ - z> is accepted.  product == 0: the one candidate is the step the search chose -- accepted.
__global__ __launch_bounds__(256) void decide_kernel(const double* __restrict__ part_t, int nb_t, const double* __restrict__ part_r,
                                                     int nb_r, int count, int product, int backtrack, double alpha, float tol,
                                                     Ctl* __restrict__ ctl) {
  __shared__ double red[256], t[kPart], r[kPart];
  if (threadIdx.x == 0) {
    ctl->accept = product ? -1 : 0;
    ctl->bad = 0;
  }
  __syncthreads();
  for (int j = 0; j < count; ++j) {
    fold_partials(part_t + (int64_t)j * nb_t * kPart, nb_t, 3, 0, red, t);
    if (product) fold_partials(part_r + (int64_t)j * nb_r * kPart, nb_r, 1, 0, red, r);
    if (threadIdx.x == 0) {
      ctl->dzt[j] = t[2];
      if (!product) {
        ctl->dz2 = t[2];
      } else {
        ctl->ft[j] = 0.5 * r[0] + alpha * t[0];
        if (backtrack) {
          const float fnew = __fadd_rn(__fmul_rn(0.5f, (float)r[0]), __fmul_rn((float)alpha, (float)t[0]));
          const float bound = __fsub_rn(ctl->f32, __fmul_rn(tol, (float)t[1]));
          ctl->fnew[j] = fnew;
          ctl->bound[j] = bound;
          if (ctl->accept < 0 && !ctl->bad) {
            if (fnew <= bound) {
              ctl->accept = j;
              ctl->dz2 = t[2];
            } else if (!isfinite(fnew)) {
              ctl->bad = 1;
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// the accepted candidate becomes z
__global__ __launch_bounds__(256) void accept_kernel(const float* __restrict__ Zc, float* __restrict__ Z, int64_t total,
                                                     const Ctl* __restrict__ ctl) {
  const int rung = ctl->accept;
  if (rung < 0) return;
  const float* const zc = Zc + (int64_t)rung * total;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) Z[i] = zc[i];
}

// ---- Hinv: W in double, the identity, the inverse rounded once ----------------------------------------------------------
__global__ __launch_bounds__(256) void widen_kernel(const float* __restrict__ W, int64_t ldw, double* __restrict__ Wd, int d, int k) {
  const int64_t total = (int64_t)d * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    Wd[i] = (double)W[(i / k) * ldw + (i % k)];
}

__global__ __launch_bounds__(256) void identity_kernel(double* __restrict__ I, int k) {
  const int64_t total = (int64_t)k * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    I[i] = (i / k) == (i % k) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void narrow_kernel(const double* __restrict__ S, float* __restrict__ Dst, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) Dst[i] = (float)S[i];
}

// ---- launchers -------------------------------------------------------------------------------------------------------
template <int BS, bool VEC, bool DMA, int MODE>
hipError_t launch_one(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const Epi& ep, int rungs,
                      hipStream_t st) {
  constexpr int lds = 2 * (BS + BS) * 128;
  if (lds > 48 * 1024)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&own_gemm_kernel<BS, BS, VEC, DMA, MODE>), lds);
        e != hipSuccess)
      return e;
  const dim3 grid((nn + BS - 1) / BS, (m + BS - 1) / BS, rungs);
  hipLaunchKernelGGL((own_gemm_kernel<BS, BS, VEC, DMA, MODE>), grid, dim3(256), lds, st, A, lda, B, ldb, m, nn, kk, ep);
  return hipGetLastError();
}

// the three operand forms of gpsr's launch_gemm: LDS-DMA, 16-byte buffer loads, scalar loads
template <int MODE>
hipError_t launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const Epi& ep, int side,
                       int rungs, hipStream_t st) {
  const bool vec = kk % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 &&
                   (ep.a_stride % 4) == 0;
  const bool dma = vec && kk % 32 == 0 && lda * side * 4 < ((int64_t)1 << 31) && ldb * side * 4 < ((int64_t)1 << 31);
  if (side == 128) {
    if (dma) return launch_one<128, true, true, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
    if (vec) return launch_one<128, true, false, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
    return launch_one<128, false, false, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  }
  if (dma) return launch_one<64, true, true, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  if (vec) return launch_one<64, true, false, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
  return launch_one<64, false, false, MODE>(A, lda, B, ldb, m, nn, kk, ep, rungs, st);
}

struct Space {
  float *Wt, *Hinv, *Z, *V, *D, *R, *Zc;
  double *part_r, *part_p, *part_t;
  Ctl* ctl;
  // the double stage of Hinv
  double *Wd, *A, *B, *I, *Hd;
  void* ridge;
  size_t ridge_bytes;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4, kk8 = (size_t)k * k * 8;
  w.Wt = a.take((size_t)k * d * 4);
  w.Hinv = a.take((size_t)k * k * 4);
  w.Z = a.take(nk);
  w.V = a.take(nk);
  w.D = a.take(nk);
  w.R = a.take(nd);
  w.Zc = a.take(nk * kRungs);
  // block partials: 64 x 64 blocks give the most
  w.part_r = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8 * kRungs);
  w.part_p = a.take<double>((size_t)gemm_parts((int)n, (int)k, 64) * kPart * 8);
  w.part_t = a.take<double>((size_t)kEwBlocks * kPart * 8 * kRungs);
  w.ctl = a.take<Ctl>(sizeof(Ctl));
  w.Wd = a.take<double>((size_t)d * k * 8);
  w.A = a.take<double>(kk8);
  w.B = a.take<double>((size_t)k * 8);
  w.I = a.take<double>(kk8);
  w.Hd = a.take<double>(kk8);
  w.ridge_bytes = lasso_ridge_f64_workspace_bytes(k, k);
  w.ridge = a.take<char>(w.ridge_bytes);
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha, const lasso_own_options& o, lasso_own_result* res,
          void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const Space ws = carve(workspace, n, d, k);
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  const bool force128 = (o.reserved & 1) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // products [n,d]
  const int pk = gemm_parts(n, k, side_k), pd = gemm_parts(n, d, side_d);
  const int64_t nk = (int64_t)n * k;
  const int gk = ew_grid(nk);
  lasso_own_trace* const tr = res->trace;
  if (tr) tr->eval_count = 0;

  // ---- Hinv = (W^T W + 1e-4 I)^-1 in double through the library's own Gram and Cholesky, rounded once ----
  hipLaunchKernelGGL(widen_kernel, dim3(ew_grid((int64_t)d * k)), dim3(256), 0, st, w, ldw, ws.Wd, d, k);
  hipLaunchKernelGGL(identity_kernel, dim3(ew_grid((int64_t)k * k)), dim3(256), 0, st, ws.I, k);
  LASSO_HIP_TRY(hipGetLastError());
  // (the Gram entry point also forms Z^T X: one column of W stands for X, its product is not used)
  if (int s = lasso_gram_accumulate_f64(ws.Wd, k, ws.Wd, k, d, 1, k, ws.A, ws.B, nullptr, 0, st)) return s;
  int32_t info = 0;
  const int rs = lasso_ridge_solve_f64(ws.A, ws.I, ws.Hd, k, k, k, kShift, &info, ws.ridge, ws.ridge_bytes, st);
  res->cholesky_info = info;
  if (rs == LASSO_ERR_BAD_ARG && info != 0)
    return fail(LASSO_ERR_BAD_ARG, "W^T W + 1e-4 I is not positive definite (pivot %d)", (int)info);
  if (rs) return rs;
  hipLaunchKernelGGL(narrow_kernel, dim3(ew_grid((int64_t)k * k)), dim3(256), 0, st, ws.Hd, ws.Hinv, (int64_t)k * k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));

  Ctl h;
  memset(&h, 0, sizeof(h));
  auto fetch = [&]() -> int { return read_back(&h, ws.ctl, sizeof(Ctl), st); };
  // resid, v and f of the z in ws.Z
  auto evaluate = [&]() -> int {
    Epi er = {};
    er.X = x; er.ldx = ldx; er.Out = ws.R; er.part = ws.part_r;
    LASSO_HIP_TRY(launch_gemm<EPI_RESID>(ws.Z, k, w, ldw, n, d, k, er, side_d, 1, st));
    Epi eg = {};
    eg.Z = ws.Z; eg.Out = ws.V; eg.part = ws.part_p; eg.alpha = (float)alpha;
    LASSO_HIP_TRY(launch_gemm<EPI_PGRAD>(ws.R, d, ws.Wt, d, n, k, d, eg, side_k, 1, st));
    hipLaunchKernelGGL(eval_kernel, dim3(1), dim3(256), 0, st, ws.part_r, pd, ws.part_p, pk, alpha, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    return fetch();
  };
  // candidates z_t of `count` step sizes, and (product) their objectives / verdicts; without a product the one candidate
  // is accepted and becomes z
  auto trial = [&](const Steps& steps, int count, bool product, bool backtrack) -> int {
    hipLaunchKernelGGL(trial_kernel, dim3(gk, count), dim3(256), 0, st, ws.Z, ws.V, ws.D, ws.Zc, nk, steps, ws.part_t);
    LASSO_HIP_TRY(hipGetLastError());
    if (product) {
      Epi et = {};
      et.X = x; et.ldx = ldx; et.a_stride = nk; et.part = ws.part_r;
      LASSO_HIP_TRY(launch_gemm<EPI_TRIAL>(ws.Zc, k, w, ldw, n, d, k, et, side_d, count, st));
    }
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(256), 0, st, ws.part_t, gk, ws.part_r, pd, count, product ? 1 : 0,
                       backtrack ? 1 : 0, alpha, (float)o.ls_tol, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    if (!product || backtrack) {
      hipLaunchKernelGGL(accept_kernel, dim3(gk), dim3(256), 0, st, ws.Zc, ws.Z, nk, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
    }
    return product ? fetch() : LASSO_OK;
  };
  auto note_eval = [&](int iter, double t, double f) {
    if (!tr) return;
    if (tr->eval_count < tr->eval_capacity) {
      tr->eval_iter[tr->eval_count] = iter;
      tr->eval_t[tr->eval_count] = t;
      tr->eval_f[tr->eval_count] = f;
    }
    ++tr->eval_count;
  };

  hipLaunchKernelGGL(init_kernel, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  if (int s = evaluate()) return s;
  res->f0 = res->f_final = h.f;
  bool stop = false;
  if (!isfinite(h.f)) {
    res->flags |= LASSO_OWN_NONFINITE;
    stop = true;
  }
  int n_iter = 0;
  while (!stop && n_iter < o.maxiter) {
    Epi ed = {};
    ed.V = ws.V; ed.Out = ws.D;
    LASSO_HIP_TRY(launch_gemm<EPI_DIR>(ws.V, k, ws.Hinv, k, n, k, k, ed, side_k, 1, st));
    double t = o.lr;
    int ls_iters = 0;
    bool applied = false;
    Steps steps = {};
    if (o.line_search == 0) {                               // bounded Brent on t -> f(project(z + t d, eta))
      BoundedMin search(0.0, 10.0, 1e-5, 500);
      while (!search.finished()) {
        const double tt = search.next();
        steps.t[0] = (float)tt;
        if (int s = trial(steps, 1, true, false)) return s;
        note_eval(n_iter + 1, tt, h.ft[0]);
        if (!isfinite(h.ft[0])) { stop = true; break; }
        search.tell(h.ft[0]);
      }
      t = search.best_x();
      ls_iters = search.evaluations();
    } else if (o.line_search == 1) {                        // t = lr, lr decay, ...: kRungs per host read
      bool accepted = false;
      for (int first = 0; first < o.ls_maxiter && !accepted && !stop; ) {
        const int count = std::min(kRungs, o.ls_maxiter - first);
        double tv[kRungs];
        for (int j = 0; j < count; ++j) {
          tv[j] = t;
          steps.t[j] = (float)t;
          t = t * o.ls_decay;                               // the reference's t = t * decay, in double
        }
        if (int s = trial(steps, count, true, true)) return s;
        const int seen = h.accept >= 0 ? h.accept + 1 : count;
        for (int j = 0; j < seen; ++j) note_eval(n_iter + 1, tv[j], h.ft[j]);
        if (h.accept >= 0) {
          accepted = true;
          t = tv[h.accept];
          ls_iters = first + h.accept + 1;
        } else if (h.bad) {
          stop = true;
        }
        first += count;
      }
      if (!accepted && !stop) {                             // 'line search did not converge.': the next rung, unexamined
        res->flags |= LASSO_OWN_LS_NOT_CONVERGED;
        ++res->ls_failures;
        ls_iters = o.ls_maxiter;
      }
      applied = accepted;                                   // (accept_kernel rode behind the ladder)
    }
    if (stop) {                                             // a non-finite trial: z is the last accepted one
      res->flags |= LASSO_OWN_NONFINITE;
      break;
    }
    if (!applied) {                                         // z+ = project(z + t d, eta) of the step the search chose
      steps.t[0] = (float)t;
      if (int s = trial(steps, 1, false, false)) return s;
    }
    if (int s = evaluate()) return s;                       // (reads dz2 of the accepted step along with f)
    ++n_iter;
    const double delta = sqrt(h.dz2);
    if (tr && n_iter <= tr->capacity) {
      tr->t[n_iter - 1] = t;
      tr->ls_iters[n_iter - 1] = ls_iters;
      tr->f[n_iter - 1] = h.f;
      tr->delta_z[n_iter - 1] = delta;
    }
    res->f_final = h.f;
    if (!isfinite(h.f)) {
      res->flags |= LASSO_OWN_NONFINITE;
      break;
    }
    if ((float)delta <= (float)o.xtol) break;               // the reference compares float32 values
  }
  res->n_iter = n_iter;
  hipLaunchKernelGGL(gpsr::copy_out_kernel, dim3(gk), dim3(256), 0, st, ws.Z, zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace own
}  // namespace lasso
