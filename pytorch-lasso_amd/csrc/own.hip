// Orthant-wise Newton (the reference's lasso/linear/solvers/orthant_wise_newton.py) on the fp32 MFMA GEMM: the driver
// behind lasso_own_solve.  min 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch with the explicit Hessian
// W^T W + 1e-4 I, whose inverse is one k x k matrix for the whole batch (computed once, in double, rounded once).
//
// Every product is solver_common.hpp's gemm_kernel (the main loop of gemm.hip) with an epilogue of its own:
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
#include "hinv_f64.hpp"
#include "brent_host.hpp"

namespace lasso {
namespace own {
namespace {

using namespace solver;

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

// the epilogue of mode MODE for solver_common.hpp's gemm_kernel
template <int MODE>
struct EpiM : Epi {
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const Epi& ep = *this;
    float s0 = 0.0f;
    const int64_t ldn = t.nn;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      if constexpr (MODE == EPI_RESID || MODE == EPI_TRIAL) {
        const __amdgpu_buffer_rsrc_t xrs = t.rsrc(ep.X, ep.ldx);
        float x[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) x[nj][rg] = t.ld32(xrs, t.off(mi, nj, rg, ep.ldx));
        __amdgpu_buffer_rsrc_t ors = xrs;
        if constexpr (MODE == EPI_RESID) ors = t.rsrc(ep.Out, ldn);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const float r = __fsub_rn(acc[mi][nj][rg], x[nj][rg]);
            if (t.inside(o[nj][rg])) s0 += __fmul_rn(r, r);
            if constexpr (MODE == EPI_RESID) t.st32(r, ors, o[nj][rg]);
          }
      } else if constexpr (MODE == EPI_PGRAD) {
        const __amdgpu_buffer_rsrc_t zrs = t.rsrc(ep.Z, ldn), ors = t.rsrc(ep.Out, ldn);
        float z[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) z[nj][rg] = t.ld32(zrs, o[nj][rg]);
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
            if (t.inside(o[nj][rg])) s0 += fabsf(zz);
            t.st32(-pg, ors, o[nj][rg]);
          }
      } else {                                   // EPI_DIR
        const __amdgpu_buffer_rsrc_t vrs = t.rsrc(ep.V, ldn), ors = t.rsrc(ep.Out, ldn);
        float v[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) v[nj][rg] = t.ld32(vrs, o[nj][rg]);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg)
            t.st32(keep_sign(acc[mi][nj][rg], v[nj][rg] > 0.0f, v[nj][rg] < 0.0f), ors, o[nj][rg]);
      }
    }
    if constexpr (MODE != EPI_DIR) {
      double s[1] = {(double)s0};
      float nomax[1] = {0.0f};
      block_fold<1, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(ep.part));
    }
  }
};

template <int MODE>
hipError_t launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const Epi& ep, int side,
                       int rungs, hipStream_t st) {
  return solver::launch_gemm(A, lda, B, ldb, m, nn, kk, EpiM<MODE>{ep}, side, rungs, st);
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

struct Space {
  float *Wt, *Hinv, *Z, *V, *D, *R, *Zc;
  double *part_r, *part_p, *part_t;
  Ctl* ctl;
  HinvStage hinv;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4;
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
  w.hinv = carve_hinv(a, d, k);
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

  // ---- Hinv = (W^T W + 1e-4 I)^-1 (hinv_f64.hpp), the pivots' verdict read at once ----
  int32_t info = 0;
  const int rs = build_hinv(w, ldw, d, k, 1.0, kShift, ws.hinv, ws.Hinv, &info, st);
  res->cholesky_info = info;
  if (rs == LASSO_ERR_BAD_ARG && info != 0)
    return fail(LASSO_ERR_BAD_ARG, "W^T W + 1e-4 I is not positive definite (pivot %d)", (int)info);
  if (rs) return rs;
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

  hipLaunchKernelGGL(init_packed_kernel<>, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, n, k);
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
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, ws.Z, zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace own
}  // namespace lasso
