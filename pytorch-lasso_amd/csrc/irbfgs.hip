// BFGS iterated ridge (the reference's lasso/nonlinear/iterative_ridge_bfgs.py with f(z) = 0.5 |z W^T - x|^2): the driver
// behind lasso_irbfgs_solve and lasso_irbfgs_update.  Every batch row keeps its own BFGS Hessian estimate B [k][k]; an
// iteration solves, per row, the masked and diagonally loaded system
//   (mask(B) + diag(alpha / |z| + tikhonov)) d = g + alpha sign(z),   masked where |z| < eps,
// takes ONE step size for the whole batch (bounded Brent on (0, 10), or fixed), stops on |z+ - z|_2 <= xtol, and
// otherwise updates every B by the rank-2 BFGS formula.
//
// row_kernel is the new work: one workgroup per row (grid-strided), ONE launch per iteration.  For its row it forms
// s = z - z_prev, y = g - g_prev, the dots y.s and y.y (double, rounded once), Bs = B s (row sums in double), s^T B s,
// the first update's scaling B *= rho (y.y), the update  B_ij <- (B_ij + rho (y_i y_j)) - (Bs_i Bs_j) / (s^T B s)  in
// place, and -- in the same pass, because the new z is known -- the next iteration's masked system (lower triangle, the
// [k][k] layout batch_solve::chol reads) with its right-hand side, and the new z_prev / g_prev.  Every term of the update
// is a symmetric function of (i, j) evaluated with commutative operations, so B stays bitwise symmetric without a
// mirroring store and every access of B is a full coalesced row.  Traffic per row: B read twice (B s, then the update;
// the second read follows the first through the same workgroup), written once, half a matrix written for the system.
// A row whose |y.s| <= 1e-10 keeps its B: one read of B for the system, no write.  Iteration 1 (B = I) writes B and the
// system without reading anything k x k.
//
// The solve is batch_solve::chol on the emitted systems; when it reports a bad system the upper triangles are filled
// by mirror_kernel and batch_solve::lu solves the whole batch, as the reference does.  The line search evaluates
//   f(t) = 0.5 (|r|^2 - 2 t <r,q> + t^2 |q|^2) + alpha sum |z - t d|,   q = d W^T,
// from three sums taken once per iteration: a Brent evaluation is one pass over [n,k] (the kernels are iter_ridge.hip's
// few lines written again for the step z - t d).  The residual and gradient of the new z are fresh products.
// Every sum is folded in double in a fixed order: no float atomics, two solves of the same arguments are bitwise equal.
// Host reads: the one batch_solve::chol makes (and lu's, on that route), one per Brent evaluation, one per iteration.
#include "solver_common.hpp"
#include "brent_host.hpp"

namespace lasso {
namespace irbfgs {
namespace {

using namespace solver;

constexpr int kMaxK = 1024;                   // batch_solve's general tier (float)
constexpr float kCurvMin = 1e-10f;            // BFGS.update: valid = |y.s| > 1e-10
constexpr int kRowGrid = 4096;                // workgroups of row_kernel at most

// control record (device; the host reads it once per iteration / Brent evaluation)
struct Ctl {
  double rr, l1, g1, dx2, f;                  // |z W^T - x|^2, |z|_1, |g|_1, |z+ - z|^2, objective
  double rq, qq, ft;                          // line search: <r,q>, |q|^2, the last trial's objective
  int invalid, pad;                           // rows whose last update had |y.s| <= 1e-10
};

struct RowArgs {
  float* B;                                   // [n][k][k] in/out
  const float* X; const float* G;             // [n][k] the new iterate and its gradient
  float* Xp; float* Gp;                       // [n][k] in: the previous pair; out: X, G
  float* SYS;                                 // out [n][k][k], lower triangles
  float* RHS;                                 // out [n][k]
  int* valid;                                 // out [n]
  int n, k;
  float alpha, tikhonov, eps;
  int mode;                                   // 0: B = I (no update), 1: update, 2: B as it is (system only)
  int first;                                  // mode 1: the first update's scaling
};

// sum over the 256 threads in a fixed order, the same bits in every thread; red [4]
__device__ __forceinline__ double block_sum(double a, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  __syncthreads();                            // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per row.  VEC: k % 4 == 0, every row of B is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void row_kernel(RowArgs a) {
  __shared__ __attribute__((aligned(16))) float sS[kMaxK], sY[kMaxK], sBs[kMaxK], sM[kMaxK], sD[kMaxK];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int k = a.k, kk = k * k;
  for (int row = blockIdx.x; row < a.n; row += gridDim.x) {
    float* const Br = a.B + (int64_t)row * kk;
    float* const Sr = a.SYS + (int64_t)row * kk;
    const int64_t vo = (int64_t)row * k;
    // ---- the vectors: s, y, their dots; mask, diagonal load and right-hand side of the new z ----
    double ys = 0.0, yy = 0.0;
    for (int j = tid; j < k; j += 256) {
      const float x = a.X[vo + j], g = a.G[vo + j];
      if (a.mode == 1) {
        const float s = __fsub_rn(x, a.Xp[vo + j]), y = __fsub_rn(g, a.Gp[vo + j]);
        sS[j] = s;
        sY[j] = y;
        ys = fma((double)y, (double)s, ys);
        yy = fma((double)y, (double)y, yy);
      }
      const float mag = fabsf(x);
      const bool zero = mag < a.eps;          // (a NaN is not masked: its diagonal is NaN)
      // (alpha / |x| in torch is reciprocal(|x|) * alpha: two roundings, kept)
      const float dg = zero ? 0.0f : __fmul_rn(__fdiv_rn(1.0f, mag), a.alpha);
      a.RHS[vo + j] = zero ? 0.0f : __fadd_rn(g, __fmul_rn(dg, x));
      sM[j] = zero ? 0.0f : 1.0f;
      sD[j] = __fadd_rn(dg, a.tikhonov);
      a.Xp[vo + j] = x;
      a.Gp[vo + j] = g;
    }
    bool valid = true;
    float rho = 0.0f, scale = 1.0f, sbs = 1.0f;
    bool scaled = false;
    if (a.mode == 1) {
      const float ysf = (float)block_sum(ys, red);
      const float yyf = (float)block_sum(yy, red);
      valid = fabsf(ysf) > kCurvMin;          // (a NaN is invalid)
      rho = valid ? __fdiv_rn(1.0f, ysf) : 1000.0f;
      scaled = a.first != 0;
      if (scaled) scale = __fmul_rn(rho, yyf);
    } else {
      __syncthreads();
    }
    if (tid == 0) a.valid[row] = valid ? 1 : 0;
    const bool update = a.mode == 1 && valid;
    if (update) {
      // ---- Bs = B s: a wave per row of B, four rows in flight; sums in double, rounded once ----
      for (int i0 = w; i0 < k; i0 += 16) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (VEC) {
          for (int j = 4 * lane; j < k; j += 256) {
            const float4 sv = *reinterpret_cast<const float4*>(&sS[j]);
            float4 b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int i = i0 + 4 * u;
              b[u] = i < k ? *reinterpret_cast<const float4*>(Br + i * k + j) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (scaled) {
                b[u].x = __fmul_rn(scale, b[u].x); b[u].y = __fmul_rn(scale, b[u].y);
                b[u].z = __fmul_rn(scale, b[u].z); b[u].w = __fmul_rn(scale, b[u].w);
              }
              acc[u] = fma((double)b[u].x, (double)sv.x, acc[u]);
              acc[u] = fma((double)b[u].y, (double)sv.y, acc[u]);
              acc[u] = fma((double)b[u].z, (double)sv.z, acc[u]);
              acc[u] = fma((double)b[u].w, (double)sv.w, acc[u]);
            }
          }
        } else {
          for (int j = lane; j < k; j += 64) {
            const float sv = sS[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int i = i0 + 4 * u;
              float b = i < k ? Br[i * k + j] : 0.0f;
              if (scaled) b = __fmul_rn(scale, b);
              acc[u] = fma((double)b, (double)sv, acc[u]);
            }
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] += __shfl_xor(acc[u], off);
        if (lane == 0)
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (i0 + 4 * u < k) sBs[i0 + 4 * u] = (float)acc[u];
      }
      __syncthreads();
      double q = 0.0;
      for (int j = tid; j < k; j += 256) q = fma((double)sS[j], (double)sBs[j], q);
      sbs = (float)block_sum(q, red);
    }
    // ---- one pass: the update of B in place and the masked, loaded lower triangle of the system ----
    // element (i, j): every term is symmetric in (i, j), so both triangles of B get the same bits
    auto element = [&](float b, int i, int j) -> float {
      if (scaled) b = __fmul_rn(scale, b);
      if (update) {
        const float up = __fadd_rn(b, __fmul_rn(rho, __fmul_rn(sY[i], sY[j])));
        b = __fsub_rn(up, __fdiv_rn(__fmul_rn(sBs[i], sBs[j]), sbs));
      }
      return b;
    };
    auto system = [&](float b, int i, int j) -> float {
      float v = (sM[i] != 0.0f && sM[j] != 0.0f) ? b : 0.0f;
      if (i == j) v = __fadd_rn(v, sD[i]);
      return v;
    };
    const bool readB = a.mode != 0, writeB = a.mode == 0 || update || (a.mode == 1 && scaled);
    if constexpr (VEC) {
      for (int e = 4 * tid; e < kk; e += 1024) {
        const int i = e / k, j = e - i * k;
        float4 b = make_float4(i == j ? 1.0f : 0.0f, i == j + 1 ? 1.0f : 0.0f, i == j + 2 ? 1.0f : 0.0f, i == j + 3 ? 1.0f : 0.0f);
        if (readB) {
          b = *reinterpret_cast<const float4*>(Br + e);
          b.x = element(b.x, i, j); b.y = element(b.y, i, j + 1); b.z = element(b.z, i, j + 2); b.w = element(b.w, i, j + 3);
        }
        if (writeB) *reinterpret_cast<float4*>(Br + e) = b;
        if (j <= i)                           // (the entries right of the diagonal in this vector are the true values)
          *reinterpret_cast<float4*>(Sr + e) =
              make_float4(system(b.x, i, j), system(b.y, i, j + 1), system(b.z, i, j + 2), system(b.w, i, j + 3));
      }
    } else {
      for (int e = tid; e < kk; e += 256) {
        const int i = e / k, j = e - i * k;
        float b = i == j ? 1.0f : 0.0f;
        if (readB) b = element(Br[e], i, j);
        if (writeB) Br[e] = b;
        if (j <= i) Sr[e] = system(b, i, j);
      }
    }
    __syncthreads();                          // (the LDS vectors are rewritten by the next row)
  }
}

// the strict upper triangles of the systems from their lower ones (the LU route reads full matrices)
__global__ __launch_bounds__(256) void mirror_kernel(float* __restrict__ SYS, int64_t total, int k) {
  const int kk = k * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / kk;
    const int r = (int)(e - m * kk), i = r / k, j = r - i * k;
    if (j > i) SYS[e] = SYS[m * kk + (int64_t)j * k + i];
  }
}

// partials {sum |a|, sum |b|} over [total]
__global__ __launch_bounds__(256) void norms_kernel(const float* __restrict__ A, const float* __restrict__ Bv, int64_t total,
                                                    double* __restrict__ part) {
  __shared__ double red[32];
  double s[2] = {0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    s[0] += (double)fabsf(A[i]);
    s[1] += (double)fabsf(Bv[i]);
  }
  block_fold<2, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
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

// partial {sum |z - t d|} over [n,k]
__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ Z, const float* __restrict__ D, int64_t total, float t,
                                                 double* __restrict__ part) {
  __shared__ double red[32];
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    s[0] += (double)fabsf(__fmaf_rn(-t, D[i], Z[i]));
  block_fold<1, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// f(t) = 0.5 (|r|^2 - 2 t <r,q> + t^2 |q|^2) + alpha sum |z - t d|
__global__ __launch_bounds__(256) void trial_fold_kernel(const double* __restrict__ part, int nb, double t, double alpha,
                                                         Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart];
  fold_partials(part, nb, 1, 0, red, a);
  if (threadIdx.x == 0) ctl->ft = 0.5 * (ctl->rr - 2.0 * t * ctl->rq + t * t * ctl->qq) + alpha * a[0];
}

// z+ = where(|z| < eps, z, z - t d) in place; partials {|z+ - z|^2, |z+|_1}
__global__ __launch_bounds__(256) void accept_kernel(float* __restrict__ Z, const float* __restrict__ D, int64_t total, float eps,
                                                     float t, double* __restrict__ part) {
  __shared__ double red[32];
  double s[2] = {0.0, 0.0};
  float nomax[1] = {0.0f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float z = Z[i];
    const float zn = fabsf(z) < eps ? z : __fmaf_rn(-t, D[i], z);
    const double dz = (double)__fsub_rn(zn, z);
    s[0] += dz * dz;
    s[1] += (double)fabsf(zn);
    Z[i] = zn;
  }
  block_fold<2, 0>(s, nomax, red, part + (int64_t)blockIdx.x * kPart);
}

// the objective of the start: {|z|_1, |g|_1} from part_a, |r|^2 from part_r
__global__ __launch_bounds__(256) void start_fold_kernel(const double* __restrict__ part_a, int nb_a, const double* __restrict__ part_r,
                                                         int nb_r, double alpha, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], r[kPart];
  fold_partials(part_a, nb_a, 2, 0, red, a);
  fold_partials(part_r, nb_r, 1, 0, red, r);
  if (threadIdx.x == 0) {
    ctl->l1 = a[0];
    ctl->g1 = a[1];
    ctl->rr = r[0];
    ctl->dx2 = 0.0;
    ctl->f = 0.5 * r[0] + alpha * a[0];
    ctl->invalid = 0;
  }
}

// an iteration's end: {|dz|^2, |z+|_1} from the accept step, |r|^2 of the new z
__global__ __launch_bounds__(256) void iter_fold_kernel(const double* __restrict__ part_a, int nb_a, const double* __restrict__ part_r,
                                                        int nb_r, double alpha, Ctl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], r[kPart];
  fold_partials(part_a, nb_a, 2, 0, red, a);
  fold_partials(part_r, nb_r, 1, 0, red, r);
  if (threadIdx.x == 0) {
    ctl->dx2 = a[0];
    ctl->l1 = a[1];
    ctl->rr = r[0];
    ctl->f = 0.5 * r[0] + alpha * a[1];
  }
}

// rows whose update was invalid
__global__ __launch_bounds__(256) void invalid_kernel(const int* __restrict__ valid, int n, Ctl* __restrict__ ctl) {
  __shared__ int cnt[256];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) c += valid[i] ? 0 : 1;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) ctl->invalid = cnt[0];
}

hipError_t launch_row(const RowArgs& a, int max_wgs, hipStream_t st) {
  const int cap = max_wgs > 0 ? max_wgs : kRowGrid;
  const int grid = std::max(1, std::min(a.n, cap));
  if (a.k % 4 == 0 && (((uintptr_t)a.B | (uintptr_t)a.SYS) & 15) == 0)
    hipLaunchKernelGGL(row_kernel<true>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(row_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

// bytes one launch of row_kernel moves for its k x k matrices (the budget of DESIGN.md 3.19)
double row_bytes(int64_t n, int64_t k, int mode, int64_t invalid) {
  const double kk = (double)k * (double)k * 4.0, half = kk * 0.5;
  if (mode == 0) return (double)n * (kk + half);
  return (double)(n - invalid) * (3.0 * kk + half) + (double)invalid * (kk + half);
}

struct RowTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false, pending = false;
  explicit RowTimer(bool enabled) { on = enabled && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
  ~RowTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void begin(hipStream_t st) { if (on) (void)hipEventRecord(a, st); }
  void end(hipStream_t st) { if (on) pending = hipEventRecord(b, st) == hipSuccess; }
  double collect() {                          // after a synchronisation of the stream
    float ms = 0.0f;
    if (!pending || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = 0.0f;
    pending = false;
    return ms;
  }
};

struct Space {
  float *Wt, *Z, *G, *Zp, *Gp, *RHS, *D, *R, *Q, *B, *SYS;
  int* valid;
  double *part_r, *part_a, *part_e;
  Ctl* ctl;
  char* solve_ws;
  size_t bytes;
};

Space carve(void* base, int64_t n, int64_t d, int64_t k) {
  Space w;
  Arena a(base);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4, nkk = (size_t)n * k * k * 4;
  w.Wt = a.take((size_t)k * d * 4);
  w.Z = a.take(nk);
  w.G = a.take(nk);
  w.Zp = a.take(nk);
  w.Gp = a.take(nk);
  w.RHS = a.take(nk);
  w.D = a.take(nk);
  w.R = a.take(nd);
  w.Q = a.take(nd);
  w.B = a.take(nkk);
  w.SYS = a.take(nkk);
  w.valid = a.take<int>((size_t)n * 4);
  w.part_r = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8);
  w.part_a = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.part_e = a.take<double>((size_t)kEwBlocks * kPart * 8);
  w.ctl = a.take<Ctl>(sizeof(Ctl));
  w.solve_ws = a.take<char>(n > 0 ? batch_solve::workspace_bytes(n, k, LASSO_F32) : 0);
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int update(float* B, const float* x, const float* g, float* x_prev, float* g_prev, float* sys, float* rhs, int32_t* valid,
           int64_t n, int64_t k, double alpha, double tikhonov, double eps, int mode, int first, int max_workgroups,
           hipStream_t st) {
  RowArgs a = {};
  a.B = B; a.X = x; a.G = g; a.Xp = x_prev; a.Gp = g_prev; a.SYS = sys; a.RHS = rhs; a.valid = valid;
  a.n = (int)n; a.k = (int)k;
  a.alpha = (float)alpha; a.tikhonov = (float)tikhonov; a.eps = (float)eps;
  a.mode = mode; a.first = first;
  LASSO_HIP_TRY(launch_row(a, max_workgroups, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha, const lasso_irbfgs_options& o, lasso_irbfgs_result* res,
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
  const int gk = ew_grid(nk), gd = ew_grid(nd);
  const float eps = (float)o.eps;
  lasso_irbfgs_trace* const tr = res->trace;
  RowTimer timer((o.reserved & 2) != 0), solve_timer((o.reserved & 2) != 0);

  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));
  Ctl h;
  memset(&h, 0, sizeof(h));
  int pending = -1;                           // the iteration whose update's count of invalid rows has not been read yet
  auto fetch = [&]() -> int {
    if (int s = read_back(&h, ws.ctl, sizeof(Ctl), st)) return s;
    if (pending >= 0) {
      if (tr && pending < tr->capacity) tr->invalid_rows[pending] = h.invalid;
      if (timer.on) {
        res->row_ms += timer.collect();
        res->row_bytes += row_bytes(n, k, 1, h.invalid);
      }
      pending = -1;
    }
    return LASSO_OK;
  };
  // r = z W^T - x (with the block partials of |r|^2), g = r W
  auto evaluate = [&]() -> hipError_t {
    if (hipError_t e = launch_gemm(ws.Z, k, w, ldw, n, d, k, Resid0Epi{x, ldx, ws.R, d, ws.part_r, 0}, side_d, 1, st); e != hipSuccess)
      return e;
    return launch_gemm(ws.R, d, ws.Wt, d, n, k, d, StoreEpi{ws.G, k, 0}, side_k, 1, st);
  };
  auto rows = [&](int mode, int first) -> hipError_t {
    RowArgs a = {};
    a.B = ws.B; a.X = ws.Z; a.G = ws.G; a.Xp = ws.Zp; a.Gp = ws.Gp; a.SYS = ws.SYS; a.RHS = ws.RHS; a.valid = ws.valid;
    a.n = n; a.k = k;
    a.alpha = (float)alpha; a.tikhonov = (float)o.tikhonov; a.eps = eps;
    a.mode = mode; a.first = first;
    return launch_row(a, 0, st);
  };

  hipLaunchKernelGGL(init_packed_kernel<>, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Z, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(evaluate());
  hipLaunchKernelGGL(norms_kernel, dim3(gk), dim3(256), 0, st, (const float*)ws.Z, (const float*)ws.G, nk, ws.part_a);
  hipLaunchKernelGGL(start_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.part_a, gk, (const double*)ws.part_r, pd, alpha,
                     ws.ctl);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(rows(0, 0));                  // B = I, the first system, z_prev = z, g_prev = g
  if (int s = fetch()) return s;
  res->f0 = res->f_final = h.f;
  // t = clamp(lr / |grad|_1, max=lr), a float32 in the reference (iterative_ridge_bfgs.py:94)
  const float lr32 = (float)o.lr;
  double t_next = (double)fminf(lr32 / (float)h.g1, lr32);
  int n_iter = 0, updates = 0;
  while (n_iter < o.maxiter) {
    // ---- d: Cholesky of every row's system, LU of the whole batch if one fails ----
    lasso_batch_solve_result br = {};
    solve_timer.begin(st);
    if (int s = batch_solve::chol(ws.SYS, (int64_t)k * k, k, ws.RHS, k, ws.D, k, n, k, LASSO_F32, &br, ws.solve_ws, st)) return s;
    bool lu = false;
    if (br.bad_system >= 0) {
      lu = true;
      ++res->lu_count;
      hipLaunchKernelGGL(mirror_kernel, dim3(ew_grid(nk * k)), dim3(256), 0, st, ws.SYS, nk * k, k);
      LASSO_HIP_TRY(hipGetLastError());
      if (int s = batch_solve::lu(ws.SYS, (int64_t)k * k, k, ws.RHS, k, ws.D, k, n, k, LASSO_F32, &br, ws.solve_ws, st)) return s;
      // a zero pivot: the system is singular (the reference raises) -- unless a NaN of the operands reached it (the search
      // for a pivot passes over NaN entries; the reference returns that row as NaN): the row's solution tells
      bool finite = br.bad_system >= 0;
      if (br.bad_system >= 0) {
        std::vector<float> row((size_t)k);
        if (int s = read_back(row.data(), ws.D + br.bad_system * k, (size_t)k * 4, st)) return s;
        for (int j = 0; j < k; ++j) finite = finite && isfinite(row[j]);
      }
      if (finite) {
        res->n_iter = n_iter;
        res->bad_row = br.bad_system;
        return fail(LASSO_ERR_BAD_ARG, "iterative_ridge_bfgs: the system of row %lld is singular", (long long)br.bad_system);
      }
    }
    solve_timer.end(st);
    double t = t_next;
    int ls_iters = 0;
    if (o.line_search) {
      LASSO_HIP_TRY(launch_gemm(ws.D, k, w, ldw, n, d, k, StoreEpi{ws.Q, d, 0}, side_d, 1, st));
      hipLaunchKernelGGL(quad_kernel, dim3(gd), dim3(256), 0, st, (const float*)ws.R, (const float*)ws.Q, nd, ws.part_e);
      hipLaunchKernelGGL(quad_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.part_e, gd, ws.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      BoundedMin search(0.0, 10.0, 1e-5, 500);
      while (!search.finished()) {
        const double tt = search.next();
        const float tf = (float)tt;
        hipLaunchKernelGGL(l1_kernel, dim3(gk), dim3(256), 0, st, (const float*)ws.Z, (const float*)ws.D, nk, tf, ws.part_e);
        hipLaunchKernelGGL(trial_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.part_e, gk, (double)tf, alpha, ws.ctl);
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
      ls_iters = search.evaluations();
    }
    hipLaunchKernelGGL(accept_kernel, dim3(gk), dim3(256), 0, st, ws.Z, (const float*)ws.D, nk, eps, (float)t, ws.part_a);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(evaluate());
    hipLaunchKernelGGL(iter_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.part_a, gk, (const double*)ws.part_r, pd, alpha,
                       ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    if (int s = fetch()) return s;
    res->solve_ms += solve_timer.collect();
    ++n_iter;
    const double delta = sqrt(h.dx2);
    res->f_final = h.f;
    if (tr && n_iter <= tr->capacity) {
      tr->t[n_iter - 1] = t;
      tr->ls_iters[n_iter - 1] = ls_iters;
      tr->f[n_iter - 1] = h.f;
      tr->delta_x[n_iter - 1] = delta;
      tr->invalid_rows[n_iter - 1] = -1;      // (no update followed this iteration -- unless the next read says otherwise)
      tr->lu[n_iter - 1] = lu ? 1 : 0;
    }
    if (!isfinite(h.f)) {
      res->flags |= LASSO_IRBFGS_NONFINITE;
      break;
    }
    if ((float)delta <= (float)o.xtol) {      // the reference compares float32 values
      res->flags |= LASSO_IRBFGS_CONVERGED;
      break;
    }
    if (n_iter == o.maxiter) break;           // (the reference's update behind the last iteration is never used)
    // ---- BFGS.update of every row, and the next iteration's systems ----
    timer.begin(st);
    LASSO_HIP_TRY(rows(1, updates == 0 ? 1 : 0));
    timer.end(st);
    hipLaunchKernelGGL(invalid_kernel, dim3(1), dim3(256), 0, st, (const int*)ws.valid, n, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    ++updates;
    pending = n_iter - 1;
    t_next = o.lr;
  }
  res->n_iter = n_iter;
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, (const float*)ws.Z, zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace irbfgs
}  // namespace lasso
