// GPSR-Basic (Figueiredo, Nowak, Wright 2007; the reference's lasso/linear/solvers/gpsr.py) on the fp32 MFMA GEMM:
// gradient projection on the split z = u - v, u, v >= 0 of  min 0.5 |y - A z|^2 + tau |z|_1  over the whole batch.
//
// This header is the solver without its operator: GPSR's epilogues, the element-wise and one-workgroup decision
// kernels, the control block, and the host loop solve_with<Op>() (at the end of the file).  The loop's only contact
// with the operator A / AT is the Op it is instantiated with: gpsr.hip instantiates it for the dictionary
// (A z = z W^T), conv_gpsr.hip for the convolution (A z = conv_transpose2d(z, W)).  Everything here sits in an
// unnamed namespace: each of the two translation units carries its own copy of the kernels.
//
// Every [n,k] x [k,d]-class product is solver_common.hpp's gemm_kernel (the main loop of gemm.hip) with an epilogue, so
// no [n,k] / [n,d] intermediate makes a trip through HBM that an epilogue can absorb:
//   EPI_GRAD   t = rb W - Ay on the accumulators; reads u, v, writes t (gu = t + tau, gv = tau - t: one array gives both)
//              and c = cu - cv, block partials of <gu,cu>, <gv,cv> and the four infinity norms of the LCP criterion
//   EPI_SUMSQ  |c W^T|^2: block partials only, the [n,d] product never reaches memory
//   EPI_RESID  rb+ = z+ W^T stored, block partials of |y - rb+|^2; blockIdx.z = rung of the step-size ladder
//   EPI_MASK_R / EPI_MASK_AP: the two products of the debias CG with the support mask
//   EPI_STORE / EPI_RESID0: Ay and the debias residual -- solver_common.hpp's StoreEpi and Resid0Epi
// All sums are block partials that ONE workgroup folds in a fixed order (solver_common.hpp).  The scalars that steer the
// iteration (lambda, the sufficient-decrease test, the stop criterion) are computed by those one-workgroup kernels with
// the reference's fp32 operation order and land in a control block that the host reads ONCE per outer iteration: the
// first trial, its decision, the accept step and the criterion are all enqueued behind the gradient; only a rejected
// first trial costs another wait, for a ladder of kLadder further step sizes evaluated in one batch.
#pragma once
#include "solver_common.hpp"

namespace lasso {
namespace gpsr {
namespace {

using namespace solver;

constexpr int kLadder = 4;            // step sizes per batch behind a rejected first trial
constexpr int kMaxReductions = 100;   // the line search gives up after this many reductions of lambda

enum { EPI_STORE = 0, EPI_GRAD, EPI_SUMSQ, EPI_RESID, EPI_RESID0, EPI_MASK_R, EPI_MASK_AP };

// control block (device; copied to the host once per outer iteration)
struct Ctl {
  float f, f_prev, lam0, lam_acc;
  float crit3, crit, ssdx, ssz;
  int accept, bad, nz, dnz;
  float fnew[kLadder], bound[kLadder];
  float absmax, rr, l1, f0;
  // debias CG
  float rtr, thresh, alpha_cg, beta_cg;
  float f_db, rr_db, conv_db; int nz_db;
  int nz0; float rr_rb; int pad[2];
};

struct Epi {
  const float* Ay; const float* U; const float* V;   // GRAD
  float* T; float* Cc;                               // GRAD out (ld = nn)
  const float* Y; int64_t ldy;                       // RESID / RESID0: the data x [m][nn]
  float* Out; int64_t ldo; int64_t out_stride;       // STORE / RESID / RESID0 / MASK_*: the product (RESID per rung: + z * out_stride)
  const float* Mask;                                 // MASK_*: 1 where the code is off the support
  float* P;                                          // MASK_R: -r out; MASK_AP: p in
  int64_t a_stride;                                  // per rung offset of the A operand
  double* part;                                      // [rungs][blocks][kPart]
  float tau;
};

// the epilogue of mode MODE (GRAD, SUMSQ, RESID, MASK_R, MASK_AP) for solver_common.hpp's gemm_kernel
template <int MODE>
struct EpiM : Epi {
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const Epi& ep = *this;
    double s[2] = {0.0, 0.0};
    float mx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float s0 = 0.0f, s1 = 0.0f;
    const int64_t ldn = t.nn;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      if constexpr (MODE == EPI_GRAD) {
        const __amdgpu_buffer_rsrc_t ars = t.rsrc(ep.Ay, ldn), urs = t.rsrc(ep.U, ldn), vrs = t.rsrc(ep.V, ldn);
        const __amdgpu_buffer_rsrc_t trs = t.rsrc(ep.T, ldn), crs = t.rsrc(ep.Cc, ldn);
        unsigned o[NJ][4];
        t.offs(mi, ldn, o);
        float ay[NJ][4], u[NJ][4], v[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            ay[nj][rg] = t.ld32(ars, o[nj][rg]);
            u[nj][rg] = t.ld32(urs, o[nj][rg]);
            v[nj][rg] = t.ld32(vrs, o[nj][rg]);
          }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const float tt = __fsub_rn(acc[mi][nj][rg], ay[nj][rg]);
            const float gu = __fadd_rn(tt, ep.tau), gv = __fadd_rn(-tt, ep.tau);
            const float uu = u[nj][rg], vv = v[nj][rg];
            const float cu = (uu <= 0.0f && gu >= 0.0f) ? 0.0f : gu;
            const float cv = (vv <= 0.0f && gv >= 0.0f) ? 0.0f : gv;
            if (t.inside(o[nj][rg])) {
              s0 += __fmul_rn(gu, cu);
              s1 += __fmul_rn(gv, cv);
              mx[0] = fmaxf(mx[0], fabsf(fminf(gu, uu)));
              mx[1] = fmaxf(mx[1], fabsf(fminf(gv, vv)));
              mx[2] = fmaxf(mx[2], fabsf(uu));
              mx[3] = fmaxf(mx[3], fabsf(vv));
            }
            t.st32(tt, trs, o[nj][rg]);
            t.st32(__fsub_rn(cu, cv), crs, o[nj][rg]);
          }
      } else if constexpr (MODE == EPI_SUMSQ) {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg)
            if (t.inside(t.off(mi, nj, rg, ldn))) s0 += __fmul_rn(acc[mi][nj][rg], acc[mi][nj][rg]);
      } else if constexpr (MODE == EPI_RESID) {            // store rb+, sum (y - rb+)^2
        const __amdgpu_buffer_rsrc_t yrs = t.rsrc(ep.Y, ep.ldy);
        const __amdgpu_buffer_rsrc_t ors = t.rsrc(ep.Out + (int64_t)blockIdx.z * ep.out_stride, ep.ldo);
        float y[NJ][4];
        unsigned oo[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            y[nj][rg] = t.ld32(yrs, t.off(mi, nj, rg, ep.ldy));
            oo[nj][rg] = t.off(mi, nj, rg, ep.ldo);
          }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const float r = __fsub_rn(y[nj][rg], acc[mi][nj][rg]);
            if (t.inside(oo[nj][rg])) s0 += __fmul_rn(r, r);
            t.st32(acc[mi][nj][rg], ors, oo[nj][rg]);
          }
      } else {                                   // EPI_MASK_R, EPI_MASK_AP
        static_assert(MODE == EPI_MASK_R || MODE == EPI_MASK_AP, "STORE and RESID0 are solver_common.hpp's");
        const __amdgpu_buffer_rsrc_t mrs = t.rsrc(ep.Mask, ldn), ors = t.rsrc(ep.Out, ldn), prs = t.rsrc(ep.P, ldn);
        unsigned o[NJ][4];
        t.offs(mi, ldn, o);
        float mk[NJ][4], p[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            mk[nj][rg] = t.ld32(mrs, o[nj][rg]);
            p[nj][rg] = MODE == EPI_MASK_AP ? t.ld32(prs, o[nj][rg]) : 0.0f;
          }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const float val = mk[nj][rg] != 0.0f ? 0.0f : acc[mi][nj][rg];
            t.st32(val, ors, o[nj][rg]);
            const bool in = t.inside(o[nj][rg]);
            if constexpr (MODE == EPI_MASK_R) {
              t.st32(-val, prs, o[nj][rg]);
              if (in) s0 += __fmul_rn(val, val);
            } else {
              if (in) s0 += __fmul_rn(p[nj][rg], val);
            }
          }
      }
    }
    s[0] = (double)s0;
    s[1] = (double)s1;
    block_fold<2, 4>(s, mx, reinterpret_cast<double*>(smem), t.partial(ep.part));
  }
};

// start of a solve / continuation step: f = 0.5 |y - rb|^2 + tau (sum u + sum v); nz of the start
__global__ __launch_bounds__(256) void start_kernel(const double* __restrict__ part_r, int nb_r, const double* __restrict__ part_uv,
                                                    int nb_uv, float tau, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], b[kPart];
  fold_partials(part_r, nb_r, 1, 0, red, a);
  fold_partials(part_uv, nb_uv, 3, 0, red, b);
  if (threadIdx.x == 0) {
    const float f = __fadd_rn(__fmul_rn(0.5f, (float)a[0]), __fmul_rn(tau, __fadd_rn((float)b[0], (float)b[1])));
    ctl->f = f;
    ctl->f_prev = f;
    ctl->f0 = f;
    ctl->nz0 = (int)b[2];
    ctl->bad = 0;
  }
}

// lambda0 = (<gu,cu> + <gv,cv>) / (|c W^T|^2 + 1e-7); the LCP criterion of this iterate
__global__ __launch_bounds__(256) void lambda_kernel(const double* __restrict__ part_g, int nb_g, const double* __restrict__ part_q,
                                                     int nb_q, Ctl* __restrict__ ctl) {
  __shared__ double red[256], g[kPart], qq[kPart];
  fold_partials(part_g, nb_g, 2, 4, red, g);
  fold_partials(part_q, nb_q, 1, 0, red, qq);
  if (threadIdx.x == 0) {
    const float num = __fadd_rn((float)g[0], (float)g[1]);
    const float den = __fadd_rn((float)qq[0], 1e-7f);
    ctl->lam0 = __fdiv_rn(num, den);
    const float numer = fmaxf((float)g[2], (float)g[3]);
    const float denom = fmaxf(fmaxf((float)g[4], (float)g[5]), 1e-6f);
    ctl->crit3 = __fdiv_rn(numer, denom);
    ctl->accept = -1;
  }
}

__device__ __forceinline__ float rung_lambda(float lam0, float beta, int rung) {
  float lam = lam0;
  for (int j = 0; j < rung; ++j) lam = __fmul_rn(lam, beta);     // the reference's lambd = lambd * lambda_backtrack
  return lam;
}

struct Step { float du, dv, un, vn; };
__device__ __forceinline__ Step take_step(float u, float v, float t, float tau, float lam) {
  const float gu = __fadd_rn(t, tau), gv = __fadd_rn(-t, tau);
  Step s;
  s.du = __fsub_rn(fmaxf(__fsub_rn(u, __fmul_rn(lam, gu)), 0.0f), u);
  s.dv = __fsub_rn(fmaxf(__fsub_rn(v, __fmul_rn(lam, gv)), 0.0f), v);
  s.un = __fadd_rn(u, s.du);
  s.vn = __fadd_rn(v, s.dv);
  return s;
}

// candidates of rungs first + blockIdx.y: z+ = z + (du - dv); partials {sum u+, sum v+, <gu,du>, <gv,dv>}
__global__ __launch_bounds__(256) void trial_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                    const float* __restrict__ T, const float* __restrict__ Z,
                                                    float* __restrict__ Zc, int64_t total, float tau, float beta, int first,
                                                    const Ctl* __restrict__ ctl, double* __restrict__ part) {
  __shared__ double red[32];
  if (first > 0 && ctl->accept >= 0) return;
  const float lam = rung_lambda(ctl->lam0, beta, first + blockIdx.y);
  float* const zc = Zc + (int64_t)blockIdx.y * total;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float u = U[i], v = V[i], t = T[i];
    const Step st = take_step(u, v, t, tau, lam);
    zc[i] = __fadd_rn(Z[i], __fsub_rn(st.du, st.dv));
    s[0] += (double)st.un;
    s[1] += (double)st.vn;
    s[2] += (double)__fmul_rn(__fadd_rn(t, tau), st.du);
    s[3] += (double)__fmul_rn(__fadd_rn(-t, tau), st.dv);
  }
  block_fold<4, 0>(s, nomax, red, part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kPart);
}

// the sufficient-decrease test of `count` rungs in the reference's order: the first with f+ <= f + mu g is accepted
__global__ __launch_bounds__(256) void decide_kernel(const double* __restrict__ part_t, int nb_t, const double* __restrict__ part_r,
                                                     int nb_r, int first, int count, float tau, float mu, float beta,
                                                     Ctl* __restrict__ ctl) {
  __shared__ double red[256], t[kPart], r[kPart];
  if (first > 0 && ctl->accept >= 0) return;
  for (int j = 0; j < count; ++j) {
    fold_partials(part_t + (int64_t)j * nb_t * kPart, nb_t, 4, 0, red, t);
    fold_partials(part_r + (int64_t)j * nb_r * kPart, nb_r, 1, 0, red, r);
    if (threadIdx.x == 0 && ctl->accept < 0 && !ctl->bad) {
      const float fnew = __fadd_rn(__fmul_rn(0.5f, (float)r[0]), __fmul_rn(tau, __fadd_rn((float)t[0], (float)t[1])));
      const float bound = __fadd_rn(ctl->f, __fmul_rn(mu, __fadd_rn((float)t[2], (float)t[3])));
      ctl->fnew[j] = fnew;
      ctl->bound[j] = bound;
      if (fnew <= bound) {
        ctl->accept = first + j;
        ctl->lam_acc = rung_lambda(ctl->lam0, beta, first + j);
        ctl->f_prev = ctl->f;
        ctl->f = fnew;
      } else if (!isfinite(fnew)) {
        ctl->bad = 1;
      }
    }
    __syncthreads();
  }
}

// accept step: u, v without their common part, z = u - v; partials {nz, changed pattern, |dz|^2, |z|^2}
__global__ __launch_bounds__(256) void finish_kernel(float* __restrict__ U, float* __restrict__ V, const float* __restrict__ T,
                                                     float* __restrict__ Z, int64_t total, float tau,
                                                     const Ctl* __restrict__ ctl, double* __restrict__ part) {
  __shared__ double red[32];
  if (ctl->accept < 0) return;
  const float lam = ctl->lam_acc;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const Step st = take_step(U[i], V[i], T[i], tau, lam);
    const float mn = fminf(st.un, st.vn);
    const float u = __fsub_rn(st.un, mn), v = __fsub_rn(st.vn, mn);
    const float zn = __fsub_rn(u, v), dz = __fsub_rn(st.du, st.dv);
    const bool was = Z[i] != 0.0f, is = zn != 0.0f;
    s[0] += is ? 1.0 : 0.0;
    s[1] += was != is ? 1.0 : 0.0;
    s[2] += (double)__fmul_rn(dz, dz);
    s[3] += (double)__fmul_rn(zn, zn);
    U[i] = u;
    V[i] = v;
    Z[i] = zn;
  }
  block_fold<4, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// the iteration's stop criterion (gpsr.py:85-117)
__global__ __launch_bounds__(256) void criterion_kernel(const double* __restrict__ part, int nb, int crit_id, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  if (ctl->accept < 0) return;
  fold_partials(part, nb, 4, 0, red, a);
  if (threadIdx.x == 0) {
    ctl->nz = (int)a[0];
    ctl->dnz = (int)a[1];
    ctl->ssdx = (float)a[2];
    ctl->ssz = (float)a[3];
    float c;
    if (crit_id == 0) c = a[0] >= 1.0 ? (float)a[1] : -INFINITY;
    else if (crit_id == 1) c = __fdiv_rn(fabsf(__fsub_rn(ctl->f, ctl->f_prev)), ctl->f_prev);
    else if (crit_id == 2) c = __fdiv_rn(__fsqrt_rn((float)a[2]), __fsqrt_rn((float)a[3]));
    else if (crit_id == 3) c = ctl->crit3;
    else c = ctl->f;
    ctl->crit = c;
  }
}

// z = start (z0, Ay or zeros) unless keep_z; u = relu(start), v = relu(-start); partials {sum u, sum v, nz of z}
__global__ __launch_bounds__(256) void init_kernel(const float* __restrict__ S, int64_t lds_, float* __restrict__ Z,
                                                   float* __restrict__ U, float* __restrict__ V, int n, int k, int keep_z,
                                                   double* __restrict__ part) {
  __shared__ double red[32];
  double s[3] = {0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float x = S ? S[(i / k) * lds_ + (i % k)] : 0.0f;
    const float u = fmaxf(x, 0.0f), v = fmaxf(-x, 0.0f);
    U[i] = u;
    V[i] = v;
    if (!keep_z) Z[i] = x;
    s[0] += (double)u;
    s[1] += (double)v;
    s[2] += (keep_z ? Z[i] : x) != 0.0f ? 1.0 : 0.0;
  }
  block_fold<3, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// max |a|, sum |a|, nonzeros of a [total]; (mask != null) mask = 1 where a == 0
__global__ __launch_bounds__(256) void absstat_kernel(const float* __restrict__ a, int64_t total, float* __restrict__ mask,
                                                      double* __restrict__ part) {
  __shared__ double red[32];
  double s[2] = {0.0, 0.0};
  float mx[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float v = fabsf(a[i]);
    s[0] += (double)v;
    s[1] += v != 0.0f ? 1.0 : 0.0;
    mx[0] = fmaxf(mx[0], v);
    if (mask) mask[i] = v == 0.0f ? 1.0f : 0.0f;
  }
  block_fold<2, 1>(s, mx, red, part + (int64_t)blockIdx.x * kPart);
}

// ctl->l1 / nz_db / absmax from absstat partials; (part_r) ctl->rr = the sum of squares a product's epilogue left
__global__ __launch_bounds__(256) void stat_kernel(const double* __restrict__ part, int nb, const double* __restrict__ part_r, int nb_r,
                                                   Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], r[kPart];
  fold_partials(part, nb, 2, 1, red, a);
  if (part_r) fold_partials(part_r, nb_r, 1, 0, red, r);
  if (threadIdx.x == 0) {
    ctl->l1 = (float)a[0];
    ctl->nz_db = (int)a[1];
    ctl->absmax = (float)a[2];
    if (part_r) ctl->rr = (float)r[0];
  }
}

// |x - rb|^2 of the rb the iteration carries (in a continuation step it is not z W^T: the reference keeps the code
// u - v of the stale pair beside the residual of z + dz, gpsr.py:53,69 -- its summary prints this one)
__global__ __launch_bounds__(256) void rb_sumsq_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ RB, int n,
                                                       int d, double* __restrict__ part) {
  __shared__ double red[32];
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  const int64_t total = (int64_t)n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float r = __fsub_rn(X[(i / d) * ldx + (i % d)], RB[i]);
    s[0] += (double)__fmul_rn(r, r);
  }
  block_fold<1, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

__global__ __launch_bounds__(256) void rb_stat_kernel(const double* __restrict__ part, int nb, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) ctl->rr_rb = (float)a[0];
}

// debias: rTr of the first masked gradient and the CG threshold tol * rTr
__global__ __launch_bounds__(256) void cg_start_kernel(const double* __restrict__ part, int nb, float tol, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) {
    ctl->rtr = (float)a[0];
    ctl->thresh = __fmul_rn(tol, (float)a[0]);
  }
}

__global__ __launch_bounds__(256) void cg_alpha_kernel(const double* __restrict__ part, int nb, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) ctl->alpha_cg = __fdiv_rn(ctl->rtr, (float)a[0]);
}

// z += a p, r += a Ap over [nk]; resid += a Wp over [nd]; partials {r.r, sum |z|, resid.resid}
__global__ __launch_bounds__(256) void cg_axpy_kernel(float* __restrict__ Z, float* __restrict__ R, const float* __restrict__ P,
                                                      const float* __restrict__ AP, int64_t nk, float* __restrict__ RES,
                                                      const float* __restrict__ WP, int64_t nd, const Ctl* __restrict__ ctl,
                                                      double* __restrict__ part) {
  __shared__ double red[32];
  const float a = ctl->alpha_cg;
  double s[3] = {0.0, 0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk + nd; i += (int64_t)gridDim.x * 256) {
    if (i < nk) {
      const float z = __fadd_rn(Z[i], __fmul_rn(a, P[i]));
      const float r = __fadd_rn(R[i], __fmul_rn(a, AP[i]));
      Z[i] = z;
      R[i] = r;
      s[0] += (double)__fmul_rn(r, r);
      s[1] += (double)fabsf(z);
    } else {
      const float e = __fadd_rn(RES[i - nk], __fmul_rn(a, WP[i - nk]));
      RES[i - nk] = e;
      s[2] += (double)__fmul_rn(e, e);
    }
  }
  block_fold<3, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// end of a CG step: beta = rTr+ / rTr, the objective and the figures of the verbose line
__global__ __launch_bounds__(256) void cg_beta_kernel(const double* __restrict__ part, int nb, float tau, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 3, 0, red, a);
  if (threadIdx.x == 0) {
    const float rtr_new = (float)a[0];
    ctl->beta_cg = __fdiv_rn(rtr_new, ctl->rtr);
    ctl->rtr = rtr_new;
    ctl->rr_db = (float)a[2];
    ctl->f_db = __fadd_rn(__fmul_rn(0.5f, (float)a[2]), __fmul_rn(tau, (float)a[1]));
    ctl->conv_db = __fdiv_rn(rtr_new, ctl->thresh);
  }
}

__global__ __launch_bounds__(256) void cg_dir_kernel(float* __restrict__ P, const float* __restrict__ R, int64_t nk,
                                                     const Ctl* __restrict__ ctl) {
  const float b = ctl->beta_cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk; i += (int64_t)gridDim.x * 256)
    P[i] = __fadd_rn(-R[i], __fmul_rn(b, P[i]));
}

// ---- launchers -------------------------------------------------------------------------------------------------------
// the product with the epilogue of mode MODE: `rungs` of them in one launch, ep.a_stride apart
template <int MODE>
hipError_t launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, int m, int nn, int kk, const Epi& ep, int side,
                       int rungs, hipStream_t st) {
  if constexpr (MODE == EPI_STORE)
    return solver::launch_gemm(A, lda, B, ldb, m, nn, kk, StoreEpi{ep.Out, ep.ldo, ep.a_stride}, side, rungs, st);
  else if constexpr (MODE == EPI_RESID0)
    return solver::launch_gemm(A, lda, B, ldb, m, nn, kk, Resid0Epi{ep.Y, ep.ldy, ep.Out, ep.ldo, ep.part, ep.a_stride}, side,
                               rungs, st);
  else
    return solver::launch_gemm(A, lda, B, ldb, m, nn, kk, EpiM<MODE>{ep}, side, rungs, st);
}

// ---- the operator-independent workspace -------------------------------------------------------------------------------
// nk = elements of the code, nd = elements of the data; pk / pd = the most block partials a code-shaped / data-shaped
// product of the operator leaves (per rung)
struct Space {
  float *Ay, *U, *V, *Z, *T, *C, *Zc, *RB;
  double *part_g, *part_q, *part_t, *part_r, *part_e;
  Ctl* ctl;
};

inline Space carve_common(Arena& a, int64_t nk64, int64_t nd64, int pk_cap, int pd_cap) {
  Space w;
  const size_t nk = (size_t)nk64 * 4, nd = (size_t)nd64 * 4;
  w.Ay = a.take(nk);
  w.U = a.take(nk);
  w.V = a.take(nk);
  w.Z = a.take(nk);
  w.T = a.take(nk);
  w.C = a.take(nk);
  w.Zc = a.take(nk * kLadder);
  w.RB = a.take(nd * (kLadder + 1));
  const size_t pk = (size_t)pk_cap * kPart * 8, pd = (size_t)pd_cap * kPart * 8;
  w.part_g = a.take<double>(pk);
  w.part_q = a.take<double>(pd);
  w.part_r = a.take<double>(pd * kLadder);
  w.part_t = a.take<double>((size_t)kEwBlocks * kPart * 8 * kLadder);
  w.part_e = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.ctl = a.take<Ctl>(sizeof(Ctl));
  return w;
}

// ---- the host loop ----------------------------------------------------------------------------------------------------
// Op is the operator.  The code is a matrix [rows][cols] (nk elements), the data nd elements that rb_sumsq reads as
// y [y_rows][y_cols] with pitch ldy.  What the loop asks of Op:
//   at<MODE>(img, ep, st)          AT(img) with a code-shaped epilogue: EPI_STORE (AT(y)), EPI_GRAD, EPI_MASK_R, EPI_MASK_AP;
//                                  leaves pk block partials in ep.part
//   a<MODE>(code, ep, rungs, st)   A(code) with a data-shaped epilogue: EPI_SUMSQ (|A c|^2), EPI_RESID (A z+ of `rungs`
//                                  candidates ep.a_stride apart, stored ep.out_stride apart, |y - A z+|^2), EPI_RESID0,
//                                  EPI_STORE (the debias CG); leaves pd block partials per rung in ep.part
//   start / ld_start               the start z0 as a matrix (null: zeros), given Ay for init = 2
//   write_out(Z, zero, st)         the result to the caller's tensor
template <class Op>
int solve_with(Op& op, const Space& ws, double alpha, const lasso_gpsr_options& o, lasso_gpsr_result* res, hipStream_t st) {
  const int n = op.rows, k = op.cols;
  const int64_t nk = (int64_t)n * k, nd = op.nd;
  const int pk = op.pk, pd = op.pd;
  const int gk = ew_grid(nk);
  Ctl h;
  memset(&h, 0, sizeof(h));
  auto fetch = [&]() -> hipError_t {
    if (hipError_t e = hipMemcpyAsync(&h, ws.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st); e != hipSuccess) return e;
    return hipStreamSynchronize(st);
  };
  res->flags = 0;
  res->n_iter = 0;
  res->db_iters = 0;
  res->steps = 0;
  res->objective = 0.0;

  // ---- set-up: the operator's packed weights, Ay = AT(y), max |Ay| ----
  LASSO_HIP_TRY(hipMemsetAsync(ws.ctl, 0, sizeof(Ctl), st));
  LASSO_HIP_TRY(op.prepare(st));
  Epi e0 = {};
  e0.Out = ws.Ay; e0.ldo = k;
  LASSO_HIP_TRY(op.template at<EPI_STORE>(op.y, e0, st));
  hipLaunchKernelGGL(absstat_kernel, dim3(gk), dim3(256), 0, st, ws.Ay, nk, (float*)nullptr, ws.part_e);
  hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gk, (const double*)nullptr, 0, ws.ctl);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(fetch());
  const double max_tau = (double)h.absmax;
  if (alpha >= max_tau) {                                   // gpsr.py:276-279: the solution is the zero vector
    res->flags |= LASSO_GPSR_ZERO_SOLUTION;
    LASSO_HIP_TRY(op.write_out(ws.Z, 1, st));
    return LASSO_OK;
  }
  // ---- continuation factors (gpsr.py:282-295) ----
  std::vector<double> factors(1, 1.0);
  int steps = 1;
  if (o.continuation) {
    steps = o.cont_steps;
    double first = o.first_tau_factor;
    if (!(first > 0.0) || first * alpha >= max_tau) {
      res->flags |= LASSO_GPSR_TAU_FACTOR_CHANGED;
      first = (double)((0.8f * h.absmax) / (float)alpha);
    }
    factors.assign(steps, 1.0);
    const double a = log10(first);
    for (int i = 0; i < steps; ++i) {                       // 10 ** numpy.linspace(a, 0, steps)
      const double stepv = steps > 1 ? (0.0 - a) / (steps - 1) : 0.0;
      const double e = (i == steps - 1 && steps > 1) ? 0.0 : a + i * stepv;
      factors[i] = pow(10.0, e);
    }
  }
  const float* start = op.start ? op.start : (o.init == 2 ? ws.Ay : nullptr);
  const int64_t ld_start = op.start ? op.ld_start : k;
  const float mu = (float)o.mu, beta = (float)o.lambda_backtrack;
  float* rb = ws.RB;                                        // the buffer that holds rb = A z
  int rb_slot = 0;
  int n_iter = 0;
  bool failed = false;
  lasso_gpsr_trace* const tr = res->trace;
  for (int step = 0; step < steps && !failed; ++step) {
    const double tau_d = alpha * factors[step];
    const float tau = (float)tau_d;
    const bool last = step + 1 == steps;
    const float tol = (float)(last ? o.tol : 1e-3);
    const int crit_id = last ? o.stop_criterion : 3;
    // u, v of the START (the reference hands every continuation step the pair formed before the loop), rb, f
    hipLaunchKernelGGL(init_kernel, dim3(gk), dim3(256), 0, st, start, ld_start, ws.Z, ws.U, ws.V, n, k, step > 0 ? 1 : 0,
                       ws.part_e);
    LASSO_HIP_TRY(hipGetLastError());
    Epi er = {};
    er.Out = rb; er.part = ws.part_r;
    LASSO_HIP_TRY(op.template a<EPI_RESID>(ws.Z, er, 1, st));
    hipLaunchKernelGGL(start_kernel, dim3(1), dim3(256), 0, st, ws.part_r, pd, ws.part_e, gk, tau, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    bool have_start = false;
    while (true) {
      // gradient, curvature, lambda0
      Epi eg = {};
      eg.Ay = ws.Ay; eg.U = ws.U; eg.V = ws.V; eg.T = ws.T; eg.Cc = ws.C; eg.part = ws.part_g; eg.tau = tau;
      LASSO_HIP_TRY(op.template at<EPI_GRAD>(rb, eg, st));
      Epi eq = {};
      eq.part = ws.part_q;
      LASSO_HIP_TRY(op.template a<EPI_SUMSQ>(ws.C, eq, 1, st));
      hipLaunchKernelGGL(lambda_kernel, dim3(1), dim3(256), 0, st, ws.part_g, pk, ws.part_q, pd, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      // trials: rung 0 alone, then ladders of kLadder; the accept step and the criterion ride behind every batch
      int first = 0, accepted = -1;
      int slots[kLadder];
      while (true) {
        const int count = first == 0 ? 1 : std::min(kLadder, kMaxReductions + 1 - first);
        for (int j = 0, s = 0; j < count; ++j, ++s) {       // rb+ of the rungs: the slots the current rb does not use
          if (s == rb_slot) ++s;
          slots[j] = s;
        }
        hipLaunchKernelGGL(trial_kernel, dim3(gk, count), dim3(256), 0, st, ws.U, ws.V, ws.T, ws.Z, ws.Zc, nk, tau, beta, first,
                           ws.ctl, ws.part_t);
        LASSO_HIP_TRY(hipGetLastError());
        // (the rungs' slots are consecutive except around rb_slot: one launch per run of consecutive slots)
        for (int j = 0; j < count;) {
          int run = 1;
          while (j + run < count && slots[j + run] == slots[j] + run) ++run;
          Epi et = {};
          et.Out = ws.RB + (int64_t)slots[j] * nd; et.out_stride = nd;
          et.a_stride = nk; et.part = ws.part_r + (int64_t)j * pd * kPart;
          LASSO_HIP_TRY(op.template a<EPI_RESID>(ws.Zc + (int64_t)j * nk, et, run, st));
          j += run;
        }
        hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(256), 0, st, ws.part_t, gk, ws.part_r, pd, first, count, tau, mu, beta,
                           ws.ctl);
        hipLaunchKernelGGL(finish_kernel, dim3(gk), dim3(256), 0, st, ws.U, ws.V, ws.T, ws.Z, nk, tau, ws.ctl, ws.part_e);
        hipLaunchKernelGGL(criterion_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gk, crit_id, ws.ctl);
        LASSO_HIP_TRY(hipGetLastError());
        LASSO_HIP_TRY(fetch());                                  // the one host wait of an iteration whose first trial holds
        if (!have_start && tr && step < tr->step_capacity) {
          tr->step_f0[step] = h.f0;
          tr->step_nz0[step] = h.nz0;
        }
        have_start = true;
        if (h.accept >= 0) { accepted = h.accept; break; }
        first += count;
        if (h.bad || first > kMaxReductions) break;
      }
      if (accepted < 0) {                                   // the documented extension: end the solve, keep the last accepted z
        res->flags |= LASSO_GPSR_LINESEARCH_FAILED;
        failed = true;
        break;
      }
      rb_slot = slots[accepted - first];                    // rb = rb+ of the accepted rung
      rb = ws.RB + (int64_t)rb_slot * nd;
      ++n_iter;
      if (tr && n_iter <= tr->capacity) {
        tr->lambda[n_iter - 1] = h.lam_acc;
        tr->lambda0[n_iter - 1] = h.lam0;
        tr->trials[n_iter - 1] = accepted + 1;
        tr->objective[n_iter - 1] = h.f;
        tr->criterion[n_iter - 1] = h.crit;
        tr->nz[n_iter - 1] = h.nz;
      }
      res->objective = (double)h.f;
      if ((n_iter > o.miniter && h.crit <= tol) || n_iter >= o.maxiter) break;
    }
    if (tr && step < tr->step_capacity) {
      tr->step_tau[step] = tau_d;
      tr->step_end[step] = n_iter;
    }
    res->steps = step + 1;
  }
  res->n_iter = n_iter;
  // ---- final figures of the main phase: |y - rb|^2 (carried and recomputed from z), |z|_1, nonzeros ----
  {
    Epi er = {};
    er.Out = ws.RB + (int64_t)(rb_slot == 0 ? 1 : 0) * nd; er.part = ws.part_r;
    // (after a failed search rb may belong to a rejected candidate: recompute from z)
    LASSO_HIP_TRY(op.template a<EPI_RESID0>(ws.Z, er, 1, st));
    hipLaunchKernelGGL(absstat_kernel, dim3(gk), dim3(256), 0, st, ws.Z, nk, ws.U /* mask */, ws.part_e);
    hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gk, ws.part_r, pd, ws.ctl);
    const int gd = ew_grid(nd);
    hipLaunchKernelGGL(rb_sumsq_kernel, dim3(gd), dim3(256), 0, st, op.y, op.ldy, rb, op.y_rows, op.y_cols, ws.part_t);
    hipLaunchKernelGGL(rb_stat_kernel, dim3(1), dim3(256), 0, st, ws.part_t, gd, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(fetch());
    res->main_rr = failed ? h.rr : h.rr_rb;
    res->main_l1 = h.l1;
    res->main_nz = h.nz_db;
    res->main_objective = res->objective;
    if (failed) res->objective = 0.5 * (double)h.rr + alpha * (double)h.l1;
  }
  // ---- debias: CG on the support of z (gpsr.py:132-206) ----
  if (o.debias && !failed) {
    float* const RES = ws.RB + (int64_t)(rb_slot == 0 ? 1 : 0) * nd;     // A z - y, from above
    float* const WP = ws.RB + (int64_t)(rb_slot <= 1 ? 2 : 1) * nd;
    float* const R = ws.T; float* const P = ws.C; float* const AP = ws.Zc; float* const MASK = ws.U;
    const float tau = (float)alpha;
    if ((int64_t)h.nz_db > nd || h.nz_db == 0) {
      res->flags |= h.nz_db == 0 ? LASSO_GPSR_DEBIAS_NO_NONZEROS : LASSO_GPSR_DEBIAS_TOO_MANY;
      res->objective = (double)(0.5f * h.rr + tau * h.l1);
    } else {
      Epi em = {};
      em.Mask = MASK; em.Out = R; em.P = P; em.part = ws.part_g;
      LASSO_HIP_TRY(op.template at<EPI_MASK_R>(RES, em, st));
      hipLaunchKernelGGL(cg_start_kernel, dim3(1), dim3(256), 0, st, ws.part_g, pk, (float)o.tol_debias, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      int it = 0;
      const int ge = ew_grid(nk + nd);
      while (true) {
        Epi ew = {};
        ew.Out = WP;
        LASSO_HIP_TRY(op.template a<EPI_STORE>(P, ew, 1, st));
        Epi ea = {};
        ea.Mask = MASK; ea.Out = AP; ea.P = P; ea.part = ws.part_g;
        LASSO_HIP_TRY(op.template at<EPI_MASK_AP>(WP, ea, st));
        hipLaunchKernelGGL(cg_alpha_kernel, dim3(1), dim3(256), 0, st, ws.part_g, pk, ws.ctl);
        hipLaunchKernelGGL(cg_axpy_kernel, dim3(ge), dim3(256), 0, st, ws.Z, R, P, AP, nk, RES, WP, nd, ws.ctl, ws.part_e);
        hipLaunchKernelGGL(cg_beta_kernel, dim3(1), dim3(256), 0, st, ws.part_e, ge, tau, ws.ctl);
        hipLaunchKernelGGL(cg_dir_kernel, dim3(gk), dim3(256), 0, st, P, R, nk, ws.ctl);
        LASSO_HIP_TRY(hipGetLastError());
        LASSO_HIP_TRY(fetch());
        ++it;
        if (tr && it <= tr->db_capacity) {
          tr->db_rr[it - 1] = h.rr_db;
          tr->db_conv[it - 1] = h.conv_db;
        }
        res->objective = (double)h.f_db;
        const bool go = it <= o.miniter_debias || (h.rtr > h.thresh && it <= o.maxiter_debias);
        if (!go) break;
      }
      res->db_iters = it;
      res->n_iter = n_iter + it;
      hipLaunchKernelGGL(absstat_kernel, dim3(gk), dim3(256), 0, st, ws.Z, nk, (float*)nullptr, ws.part_e);
      hipLaunchKernelGGL(stat_kernel, dim3(1), dim3(256), 0, st, ws.part_e, gk, (const double*)nullptr, 0, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      LASSO_HIP_TRY(fetch());
      res->db_rr = h.rr_db;
      res->db_l1 = h.l1;
      res->db_nz = h.nz_db;
    }
  }
  LASSO_HIP_TRY(op.write_out(ws.Z, 0, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace
}  // namespace gpsr
}  // namespace lasso
