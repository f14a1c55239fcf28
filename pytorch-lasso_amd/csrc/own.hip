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
// The epilogues, trial_kernel, decide_kernel and accept_kernel are orthant_common.hpp's, shared with owlqn.hip.
#include "hinv_f64.hpp"
#include "brent_host.hpp"
#include "orthant_common.hpp"

namespace lasso {
namespace own {
namespace {

using namespace solver;
using namespace orthant;

constexpr double kShift = 1e-4;       // the reference's hess.diagonal().add_(1e-4)

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
                       backtrack ? 1 : 0, 0.5, alpha, (float)o.ls_tol, ws.ctl);
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
