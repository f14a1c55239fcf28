// What the two orthant-wise solvers (own.hip: explicit Hessian; owlqn.hip: L-BFGS) share: the projection, the residual,
// pseudo-gradient and trial epilogues of solver_common.hpp's gemm_kernel, and the line-search machinery around them --
// trial_kernel (candidates of a ladder of step sizes), decide_kernel (ONE workgroup folds their partials in a fixed order
// and takes the backtracking verdicts in the reference's fp32 operation order) and accept_kernel (the accepted candidate
// becomes z).  Like solver_common.hpp, everything sits in an unnamed namespace: each translation unit carries its own copy.
#pragma once
#include "solver_common.hpp"

namespace lasso {
namespace orthant {
namespace {

using namespace solver;

constexpr int kRungs = 8;             // step sizes of a backtracking ladder per host read

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

// the objective of `count` rungs (product != 0: part_r holds the candidates' loss sums -- |z_t W^T - x|^2 with scale 0.5,
// a generalised-linear loss with scale 1, which multiplies exactly) and, for a backtracking, the sufficient-decrease test in the reference's order (orthant_wise_newton.py:23): the first rung with
// f+ <= f - tol <v, z+ - z> is accepted.  product == 0: the one candidate is the step the search chose -- accepted.
__global__ __launch_bounds__(256) void decide_kernel(const double* __restrict__ part_t, int nb_t, const double* __restrict__ part_r,
                                                     int nb_r, int count, int product, int backtrack, double scale, double alpha,
                                                     float tol, Ctl* __restrict__ ctl) {
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
        ctl->ft[j] = scale * r[0] + alpha * t[0];
        if (backtrack) {
          const float fnew = __fadd_rn(__fmul_rn((float)scale, (float)r[0]), __fmul_rn((float)alpha, (float)t[0]));
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

}  // namespace
}  // namespace orthant
}  // namespace lasso
