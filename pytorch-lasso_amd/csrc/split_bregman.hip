// Split Bregman (the reference's lasso/linear/solvers/split_bregman.py) on the fp32 MFMA GEMM: the driver behind
// lasso_split_bregman_solve.  min 0.5 |x A^T - y|^2 / alpha + |x|_1 over the whole batch, restated on row-major [n,k]
// state: H = A^T A / alpha + lambd I, whose inverse is one k x k matrix for the whole batch (computed once, in double,
// rounded once), Aty = (y A) / alpha, and per inner iteration
//   X = (Aty + lambd (D - B)) Hinv^T,  D = softshrink(X + B, 1 / lambd)
// with B += tau (X - D) and update = |X - Xold|_F behind the last inner iteration of an outer one.
//
// Every product is solver_common.hpp's gemm_kernel (the main loop of gemm.hip) with an epilogue of its own:
//   EPI_ATY    Aty = (y Wt^T) / alpha stored
//   EPI_INNER  x = T Hinv^T on the accumulators; reads B and Aty at the element, stores ONLY
//              T+ = Aty + lambd (softshrink(x + B) - B): neither X nor D of an inner iteration reaches memory
//   EPI_LAST   the same x; reads Xold, B, Aty at the element, stores X = x, B+ = B + tau (x - D) and
//              T+ = Aty + lambd (D - B+); block partials of sum (x - Xold)^2 and sum |x|
//   EPI_COST   |X W^T - y|^2 (verbose only): block partials, the [n,d] product never reaches memory
// T is the A operand of the next product: every block of a row panel reads whole rows of it while other blocks of the
// panel store T+, so T ping-pongs between two buffers.  X, B and Aty are touched only at the element a thread owns.  D
// never exists in memory: T carries all of it that the next product needs.  All sums: per thread, wave butterfly, the
// four waves, block partial (double), then ONE workgroup folds the partials in a fixed order -- no float atomics, two
// solves of the same arguments are bitwise equal.  No kernel has a data-dependent loop.
#include "hinv_f64.hpp"

namespace lasso {
namespace split_bregman {
namespace {

using namespace solver;

constexpr int kLog = 1024;            // outer iterations whose figures the device keeps between two host reads

enum { EPI_ATY = 0, EPI_INNER, EPI_LAST, EPI_COST };

// what an outer iteration leaves for the host
struct Log { double update, cost; };

struct Epi {
  const float* Aty;                   // INNER / LAST (ld nn)
  float* Bb;                          // INNER: read; LAST: read and written (ld nn)
  float* X;                           // LAST: Xold read, X written (ld nn)
  float* Out;                         // ATY: Aty; INNER / LAST: T+ (ld nn)
  const float* Y; int64_t ldy;        // COST: the data y [m][nn]
  double* part;                       // [blocks][kPart]
  int64_t a_stride;                   // 0: every launch is one product (rungs = 1)
  float lambd, lam, tau, alpha;       // lam = 1 / lambd, the shrinkage threshold
};

__device__ __forceinline__ float shrink(float v, float lam) {
  return v - __builtin_amdgcn_fmed3f(v, -lam, lam);    // == softshrink bit for bit (lam >= 0), as in cd.hip
}

// the epilogue of mode MODE for solver_common.hpp's gemm_kernel
template <int MODE>
struct EpiM : Epi {
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const Epi& ep = *this;
    float s0 = 0.0f, s1 = 0.0f;
    const int64_t ldn = t.nn;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      if constexpr (MODE == EPI_ATY) {
        const __amdgpu_buffer_rsrc_t ors = t.rsrc(ep.Out, ldn);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) t.st32(__fdiv_rn(acc[mi][nj][rg], ep.alpha), ors, o[nj][rg]);
      } else if constexpr (MODE == EPI_COST) {
        const __amdgpu_buffer_rsrc_t yrs = t.rsrc(ep.Y, ep.ldy);
        float y[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) y[nj][rg] = t.ld32(yrs, t.off(mi, nj, rg, ep.ldy));
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const float r = __fsub_rn(acc[mi][nj][rg], y[nj][rg]);
            if (t.inside(o[nj][rg])) s0 += __fmul_rn(r, r);
          }
      } else {                                   // EPI_INNER, EPI_LAST
        const __amdgpu_buffer_rsrc_t ars = t.rsrc(ep.Aty, ldn), brs = t.rsrc(ep.Bb, ldn), trs = t.rsrc(ep.Out, ldn);
        float aty[NJ][4], b[NJ][4], xo[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            aty[nj][rg] = t.ld32(ars, o[nj][rg]);
            b[nj][rg] = t.ld32(brs, o[nj][rg]);
          }
        if constexpr (MODE == EPI_INNER) {
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              const float bb = b[nj][rg];
              const float dn = shrink(__fadd_rn(acc[mi][nj][rg], bb), ep.lam);
              t.st32(__fmaf_rn(ep.lambd, __fsub_rn(dn, bb), aty[nj][rg]), trs, o[nj][rg]);
            }
        } else {
          const __amdgpu_buffer_rsrc_t xrs = t.rsrc(ep.X, ldn);
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) xo[nj][rg] = t.ld32(xrs, o[nj][rg]);
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              const float x = acc[mi][nj][rg], bb = b[nj][rg];
              const float dn = shrink(__fadd_rn(x, bb), ep.lam);
              const float bn = __fmaf_rn(ep.tau, __fsub_rn(x, dn), bb);            // b.add_(x - d, alpha=tau)
              const float dx = __fsub_rn(x, xo[nj][rg]);
              if (t.inside(o[nj][rg])) {
                s0 += __fmul_rn(dx, dx);
                s1 += fabsf(x);
              }
              t.st32(x, xrs, o[nj][rg]);
              t.st32(bn, brs, o[nj][rg]);
              t.st32(__fmaf_rn(ep.lambd, __fsub_rn(dn, bn), aty[nj][rg]), trs, o[nj][rg]);
            }
        }
      }
    }
    if constexpr (MODE == EPI_LAST || MODE == EPI_COST) {
      double s[2] = {(double)s0, (double)s1};
      float nomax[1] = {0.0f};
      block_fold<2, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(ep.part));
    }
  }
};

template <int MODE>
hipError_t launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const Epi& ep, int side,
                       hipStream_t st) {
  return solver::launch_gemm(A, lda, B, ldb, m, nn, kk, EpiM<MODE>{ep}, side, 1, st);
}

// X = x0 (pitch ld0; null: zeros), B = 0
__global__ __launch_bounds__(256) void init_kernel(const float* __restrict__ S, int64_t ld0, float* __restrict__ X,
                                                   float* __restrict__ Bb, int n, int k) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    X[i] = S ? S[(i / k) * ld0 + (i % k)] : 0.0f;
    Bb[i] = 0.0f;
  }
}

// update = |X - Xold|_F and (part_c) cost = 0.5 |X W^T - y|^2 + alpha |X|_1 of an outer iteration, folded in double
__global__ __launch_bounds__(256) void fold_kernel(const double* __restrict__ part_x, int nb_x, const double* __restrict__ part_c,
                                                   int nb_c, double alpha, Log* __restrict__ slot) {
  __shared__ double red[256], a[kPart], c[kPart];
  fold_partials(part_x, nb_x, 2, 0, red, a);
  if (part_c) fold_partials(part_c, nb_c, 1, 0, red, c);
  if (threadIdx.x == 0) {
    slot->update = sqrt(a[0]);
    slot->cost = part_c ? 0.5 * c[0] + alpha * a[1] : 0.0;
  }
}

struct Space {
  float *Wt, *Hinv, *Aty, *T[2], *Bb, *X;
  double *part_x, *part_c;
  Log* log;
  HinvStage hinv;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4;
  w.Wt = a.take((size_t)k * d * 4);
  w.Hinv = a.take((size_t)k * k * 4);
  w.Aty = a.take(nk);
  w.T[0] = a.take(nk);
  w.T[1] = a.take(nk);
  w.Bb = a.take(nk);
  w.X = a.take(nk);
  // block partials: 64 x 64 blocks give the most
  w.part_x = a.take<double>((size_t)gemm_parts((int)n, (int)k, 64) * kPart * 8);
  w.part_c = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8);
  w.log = a.take<Log>(sizeof(Log) * kLog);
  w.hinv = carve_hinv(a, d, k);
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int solve(const float* y, int64_t ldy, const float* w, int64_t ldw, const float* x0, int64_t ldx0, float* xout, int64_t ldx,
          int64_t n64, int64_t d64, int64_t k64, double alpha, const lasso_split_bregman_options& o,
          lasso_split_bregman_result* res, void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const Space ws = carve(workspace, n, d, k);
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldy, ldw});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  const bool force128 = (o.reserved & 1) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // the cost product [n,d]
  const int pk = gemm_parts(n, k, side_k), pd = gemm_parts(n, d, side_d);
  const int gk = ew_grid((int64_t)n * k);
  lasso_split_bregman_trace* const tr = res->trace;
  const bool want_cost = tr && tr->cost;

  // ---- Hinv = (W^T W / alpha + lambd I)^-1 (hinv_f64.hpp).  No info_out: the pivots' verdict waits behind the ridge
  // workspace for the first host read of the loop below ----
  if (int s = build_hinv(w, ldw, d, k, alpha, o.lambd, ws.hinv, ws.Hinv, nullptr, st)) return s;
  const int* const info_dev =
      reinterpret_cast<const int*>(static_cast<const char*>(ws.hinv.ridge) + f64::ridge_workspace_bytes(k, k));
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));
  // ---- Aty = (y W) / alpha; X = x0, B = 0 (D = 0: the first T is Aty itself) ----
  Epi e0 = {};
  e0.Out = ws.Aty; e0.alpha = (float)alpha;
  LASSO_HIP_TRY(launch_gemm<EPI_ATY>(y, ldy, ws.Wt, d, n, k, d, e0, side_k, st));
  hipLaunchKernelGGL(init_kernel, dim3(gk), dim3(256), 0, st, x0, ldx0, ws.X, ws.Bb, n, k);
  LASSO_HIP_TRY(hipGetLastError());

  Epi ep = {};
  ep.Aty = ws.Aty; ep.Bb = ws.Bb; ep.X = ws.X; ep.part = ws.part_x;
  ep.lambd = (float)o.lambd; ep.lam = (float)(1.0 / o.lambd); ep.tau = (float)o.tau;
  const float* t_cur = ws.Aty;
  int t_next = 0;
  // the figures of the iterations [fetched, done) from the device, and -- with the first of them -- the pivots' verdict
  int done = 0, fetched = 0;
  bool have_info = false;
  double update = INFINITY;
  Log host[kLog];
  auto fetch = [&]() -> int {
    int32_t info = 0;
    if (!have_info) LASSO_HIP_TRY(hipMemcpyAsync(&info, info_dev, sizeof(info), hipMemcpyDeviceToHost, st));
    for (int i = fetched; i < done;) {                      // (the ring's slots of a range are contiguous up to its end)
      const int slot = i % kLog, run = std::min(done - i, kLog - slot);
      LASSO_HIP_TRY(hipMemcpyAsync(host + slot, ws.log + slot, sizeof(Log) * run, hipMemcpyDeviceToHost, st));
      i += run;
    }
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    if (!have_info) {
      have_info = true;
      res->cholesky_info = info;
      if (info != 0) return fail(LASSO_ERR_BAD_ARG, "A^T A / alpha + lambd I is not positive definite (pivot %d)", (int)info);
    }
    for (int i = fetched; i < done; ++i) {
      const Log& h = host[i % kLog];
      if (tr && i < tr->capacity) {
        if (tr->update) tr->update[i] = h.update;
        if (tr->cost) tr->cost[i] = h.cost;
      }
      update = h.update;
    }
    fetched = done;
    return LASSO_OK;
  };
  const bool judged = o.tol >= 0.0;                         // a norm is never <= a negative tol: nothing to read
  int itn = 0;
  bool stopped = false;
  for (; itn < o.maxiter; ++itn) {
    if (judged && done > fetched)
      if (int s = fetch()) return s;                        // the one host wait of an outer iteration
    if ((float)update <= (float)o.tol) {                    // the reference compares float32 values; NaN never stops
      stopped = true;
      break;
    }
    if (done - fetched == kLog)
      if (int s = fetch()) return s;
    for (int inner = 0; inner < o.niter_inner; ++inner) {
      ep.Out = ws.T[t_next];
      if (inner + 1 < o.niter_inner)
        LASSO_HIP_TRY(launch_gemm<EPI_INNER>(t_cur, k, ws.Hinv, k, n, k, k, ep, side_k, st));
      else
        LASSO_HIP_TRY(launch_gemm<EPI_LAST>(t_cur, k, ws.Hinv, k, n, k, k, ep, side_k, st));
      t_cur = ws.T[t_next];
      t_next ^= 1;
    }
    if (want_cost) {
      Epi ec = {};
      ec.Y = y; ec.ldy = ldy; ec.part = ws.part_c;
      LASSO_HIP_TRY(launch_gemm<EPI_COST>(ws.X, k, w, ldw, n, d, k, ec, side_d, st));
    }
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(256), 0, st, ws.part_x, pk, want_cost ? ws.part_c : (const double*)nullptr, pd,
                       alpha, ws.log + done % kLog);
    LASSO_HIP_TRY(hipGetLastError());
    ++done;
  }
  if (!stopped) itn = o.maxiter - 1;                         // the reference's loop variable after a loop that ran out
  if (int s = fetch()) return s;
  res->n_iter = done;
  res->itn = itn;
  res->stopped = stopped ? 1 : 0;
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, ws.X, xout, ldx, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace split_bregman
}  // namespace lasso
