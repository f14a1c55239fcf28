// Conjugate gradients for a whole batch of right-hand sides (the reference's lasso/conjgrad.py: cg, batch_cg,
// batch_cg_conv2d): the drivers behind lasso_cg_solve and lasso_conv_cg_solve.  conjgrad() of conjgrad.py:13-57 line for
// line: x = 0, r = -b, p = b; alpha = rs_old / curv and rs_new / rs_old are one number PER GROUP (a row of b, or an
// image of it), the five exits test sums over the whole batch.
//
// The state is G groups of L contiguous elements: rows [n][k] of the dense form; for the convolutional form the code
// as the matrix [M = N Hz Wz][K] of conv.hip, whose image n is the contiguous run of L = Hz Wz K elements.
// One iteration `it`:
//   product   Ap = Adot(p) and curv_g = sum p Ap of every group
//     dense fp32   solver_common.hpp's gemm_kernel with CurvEpi: stores Ap and, per row and column block, the partial
//                  sum of p Ap over the block's columns (one slot each), then curv_fold_kernel: a row's slots folded in
//                  a fixed order
//     dense fp64   gemm_f64.hip's product (it gives -p A^T), then dot_kernel: the sign, and curv_g
//     conv fp32    launch_conv_residual (A = conv_transpose2d; the implicit synthesis kernels where they cover the
//                  geometry) and launch_conv_gradient (AT = conv2d: patches + GEMM), then dot_kernel: + tik p, curv_g
//   judge2    ONE workgroup: curv_sum = sum of the curv_g from the block partials of whoever took them, exits 2 and 3
//             (:39-45)
//   rowpass   x += alpha p, r += alpha Ap, rs_new = sum r^2, p = -r + (rs_new / rs_old) p; block partials of sum rs_new
//             and sum |r|.  A wave owns whole groups (L <= 2048: one launch); a longer group is cut into segments, a
//             workgroup each, so that a few large images still fill the device (two launches: the step with the
//             segments' partials of rs_new, then the fold of those and the move of p).  After exit 3 at it = 0 the step
//             takes the steepest-descent fallback x = -(rs_old / curv) b instead (:42-44)
//   judge1    ONE workgroup, for iteration it + 1: exit 0 on sqrt(sum rs_new) (:50; p has moved already, which no
//             result shows), exit 4 at maxiter, exit 1 on sum |r| (:34)
// The judges write a control record {stop, status, iteration}; every launch reads the flag first and does nothing once
// it is set (the two library products of the fp64 and convolutional forms run on, into a buffer nothing reads any
// more): x stays exactly what the reference returns, nothing is replayed.  The host reads the record once per chunk of
// iterations (conjgrad_host.hpp's next_chunk).  All sums: per thread in double, wave butterfly, the four waves, block
// partial, then one workgroup folds the partials in a fixed order -- no float atomics, two solves of the same
// arguments are bitwise equal.  The exit arithmetic itself is conjgrad_host.hpp's, in the tensors' dtype.
#include "solver_common.hpp"
#include "conjgrad_host.hpp"

namespace lasso {
namespace conjgrad {
namespace {

using namespace solver;

constexpr int kLog = 1024;            // iterations whose sums the device keeps between two host reads (a ring)
constexpr int kRowBlocks = 2048;      // most workgroups of a pass over the groups
constexpr int kWaveLen = 2048;        // groups up to this length are owned by a wave; longer ones are cut into segments
constexpr int kSegMin = 1024;         // shortest segment of a long group
constexpr int kSegTarget = 1024;      // segments of all groups together that a pass aims at (workgroups to fill the device)

struct Ctl { int32_t stop, status, iter, pad_; double termcond; };
struct Log { double r_abs, curv_sum, rs; };    // as the dtype holds them

__device__ __forceinline__ float abs_t(float v) { return fabsf(v); }
__device__ __forceinline__ double abs_t(double v) { return fabs(v); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the sum of v over the workgroup, in a fixed order, to every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();                                    // (the last sum's readers have left red)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the dense fp32 product's epilogue ---------------------------------------------------------------------------------
// AP [m][nn] (packed) = C, and slots[blockIdx.x][row] = sum over the block's columns of P C (double)
struct CurvEpi {
  const float* P;                     // [m][nn], the A operand itself
  float* AP;
  double* slots;                      // [column blocks][m]
  const Ctl* ctl;
  int rows;                           // m
  int64_t a_stride;
  __device__ __forceinline__ bool skip() const { return ctl->stop != 0; }
  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t prs = t.rsrc(P, ldn), ars = t.rsrc(AP, ldn);
    double* const rowsum = reinterpret_cast<double*>(smem);        // [2][BM]: the two column halves of the block
    __syncthreads();                                               // (every wave has left the main loop's tiles)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float p[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) p[nj][rg] = t.ld32(prs, o[nj][rg]);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        double s = 0.0;
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
          if (t.inside(o[nj][rg])) s += (double)__fmul_rn(p[nj][rg], acc[mi][nj][rg]);
          t.st32(acc[mi][nj][rg], ars, o[nj][rg]);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);      // the 16 lanes that share the row
        if (t.l15 == 0) rowsum[t.wc * BM + (BM / 2) * t.wr + 16 * mi + 4 * t.q + rg] = s;
      }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < t.rows_valid; r += 256)
      slots[(int64_t)blockIdx.x * rows + (t.i0 + r)] = rowsum[r] + rowsum[BM + r];
  }
};

// ---- passes over short groups (L <= kWaveLen): a wave owns whole groups, four waves to a workgroup -------------------
// the four waves' sums a, b in a fixed order -> part[blockIdx.x] (the workgroup's block partial)
__device__ __forceinline__ void waves_to_partial(double a, double b, double (*wsum)[2], double* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { wsum[w][0] = a; wsum[w][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(int64_t)blockIdx.x * kPart] = (wsum[0][0] + wsum[1][0]) + (wsum[2][0] + wsum[3][0]);
    part[(int64_t)blockIdx.x * kPart + 1] = (wsum[0][1] + wsum[1][1]) + (wsum[2][1] + wsum[3][1]);
  }
}

// x = 0, r = -b, p = b (b: pitch ldb, may be P itself); rs_g = sum b^2; block partials {sum rs_g, sum |b|}
template <class T>
__global__ __launch_bounds__(256) void init_kernel(const T* B, int64_t ldb, T* X, T* R, T* P, T* __restrict__ rs, int G, int64_t L,
                                                   double* __restrict__ part) {
  __shared__ double wsum[4][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double tot_rs = 0.0, tot_abs = 0.0;
  for (int g = blockIdx.x * 4 + w; g < G; g += gridDim.x * 4) {
    const T* const b = B + (int64_t)g * ldb;
    const int64_t base = (int64_t)g * L;
    double s_rs = 0.0, s_abs = 0.0;
    for (int64_t j = lane; j < L; j += 64) {
      const T v = b[j];
      X[base + j] = T(0);
      R[base + j] = -v;
      P[base + j] = v;
      s_rs += (double)(v * v);
      s_abs += (double)abs_t(v);
    }
    const T rs0 = (T)wave_sum(s_rs);
    if (lane == 0) rs[g] = rs0;
    tot_rs += (double)rs0;
    tot_abs += wave_sum(s_abs);
  }
  waves_to_partial(tot_rs, tot_abs, wsum, part);
}

// the products that leave curv to a pass of its own: AP = (negate ? -AP : AP) + (tik > 0 ? tik p : nothing),
// curv_g = sum p AP rounded once; block partials {sum curv_g}
template <class T>
__global__ __launch_bounds__(256) void dot_kernel(const T* __restrict__ P, T* __restrict__ AP, T* __restrict__ curv, int G, int64_t L,
                                                  T tik, int negate, double* __restrict__ cpart, const Ctl* __restrict__ ctl) {
  __shared__ double wsum[4][2];
  if (ctl->stop != 0) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool rewrite = negate != 0 || tik > T(0);
  double tot = 0.0;
  for (int g = blockIdx.x * 4 + w; g < G; g += gridDim.x * 4) {
    const int64_t base = (int64_t)g * L;
    double s = 0.0;
    for (int64_t j = lane; j < L; j += 64) {
      const T p = P[base + j];
      T a = AP[base + j];
      if (negate) a = -a;
      if (tik > T(0)) a = a + tik * p;                               // conjgrad.py:101-102
      if (rewrite) AP[base + j] = a;
      s += (double)(p * a);
    }
    const T c = (T)wave_sum(s);
    if (lane == 0) curv[g] = c;
    tot += (double)c;                                                // curv.sum(): of the rounded values
  }
  waves_to_partial(tot, 0.0, wsum, cpart);
}

// :46-52 on the groups this wave owns; rs_in / rs_out: rs_old read, rs_new written; block partials {sum rs_new, sum |r|}
template <class T>
__global__ __launch_bounds__(256) void rowpass_kernel(T* __restrict__ X, T* __restrict__ R, T* __restrict__ P, const T* __restrict__ AP,
                                                      const T* __restrict__ rs_in, T* __restrict__ rs_out, const T* __restrict__ curv,
                                                      int G, int64_t L, double* __restrict__ part, const Ctl* __restrict__ ctl, int it) {
  __shared__ double wsum[4][2];
  const bool stopped = ctl->stop != 0;
  // :42-44, the one launch that still has work behind a set flag
  const bool fallback = stopped && it == 0 && ctl->status == cg::kCurvNegative && ctl->iter == 0;
  if (stopped && !fallback) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double tot_rs = 0.0, tot_abs = 0.0;
  for (int g = blockIdx.x * 4 + w; g < G; g += gridDim.x * 4) {
    const int64_t base = (int64_t)g * L;
    const T rs_old = rs_in[g], cv = curv[g];
    if (fallback) {
      const T f = (-rs_old) / cv;                                    // x = - rs_old / curv * b, and p is still b
      for (int64_t j = lane; j < L; j += 64) X[base + j] = f * P[base + j];
      continue;
    }
    const T alpha = rs_old / cv;
    double s_rs = 0.0, s_abs = 0.0;
    for (int64_t j = lane; j < L; j += 64) {
      X[base + j] = X[base + j] + alpha * P[base + j];
      const T rn = R[base + j] + alpha * AP[base + j];
      R[base + j] = rn;
      s_rs += (double)(rn * rn);
      s_abs += (double)abs_t(rn);
    }
    const T rs_new = (T)wave_sum(s_rs);
    const T beta = rs_new / rs_old;
    for (int64_t j = lane; j < L; j += 64) P[base + j] = (-R[base + j]) + beta * P[base + j];    // (its own r: no barrier)
    if (lane == 0) rs_out[g] = rs_new;
    tot_rs += (double)rs_new;                                        // rs_new.sum(): of the rounded values
    tot_abs += wave_sum(s_abs);
  }
  if (fallback) return;
  waves_to_partial(tot_rs, tot_abs, wsum, part);
}

// ---- passes over long groups: a group is cut into nseg segments of seglen elements, a workgroup takes one segment
// (item = g nseg + seg) at a time, so that few long groups -- a handful of large images -- still fill the device.  A sum
// over a group is the segments' partials (double) folded in segment order by whoever needs it.
struct Segs { int nseg; int64_t seglen; };

// x = 0, r = -b, p = b on the segment; segpart[item] = {sum b^2, sum |b|}
template <class T>
__global__ __launch_bounds__(256) void seg_init_kernel(const T* B, int64_t ldb, T* X, T* R, T* P, double* __restrict__ segpart, int G,
                                                       int64_t L, Segs sg) {
  __shared__ double red[4];
  const int64_t items = (int64_t)G * sg.nseg;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / sg.nseg), seg = (int)(item % sg.nseg);
    const int64_t lo = seg * sg.seglen, hi = min(L, lo + sg.seglen), base = (int64_t)g * L;
    const T* const b = B + (int64_t)g * ldb;
    double s_rs = 0.0, s_abs = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
      const T v = b[j];
      X[base + j] = T(0);
      R[base + j] = -v;
      P[base + j] = v;
      s_rs += (double)(v * v);
      s_abs += (double)abs_t(v);
    }
    s_rs = block_sum(s_rs, red);
    s_abs = block_sum(s_abs, red);
    if (threadIdx.x == 0) { segpart[item * 2] = s_rs; segpart[item * 2 + 1] = s_abs; }
  }
}

// dot_kernel on a segment: slots[seg][g] = the segment's sum of p AP (curv_fold_kernel folds them)
template <class T>
__global__ __launch_bounds__(256) void seg_dot_kernel(const T* __restrict__ P, T* __restrict__ AP, double* __restrict__ slots, int G,
                                                      int64_t L, Segs sg, T tik, int negate, const Ctl* __restrict__ ctl) {
  __shared__ double red[4];
  if (ctl->stop != 0) return;
  const bool rewrite = negate != 0 || tik > T(0);
  const int64_t items = (int64_t)G * sg.nseg;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / sg.nseg), seg = (int)(item % sg.nseg);
    const int64_t lo = seg * sg.seglen, hi = min(L, lo + sg.seglen), base = (int64_t)g * L;
    double s = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
      const T p = P[base + j];
      T a = AP[base + j];
      if (negate) a = -a;
      if (tik > T(0)) a = a + tik * p;
      if (rewrite) AP[base + j] = a;
      s += (double)(p * a);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) slots[(int64_t)seg * G + g] = s;
  }
}

// x += alpha p, r += alpha Ap on the segment; segpart[item] = {sum r^2, sum |r|} (or the fallback of :42-44)
template <class T>
__global__ __launch_bounds__(256) void seg_step_kernel(T* __restrict__ X, T* __restrict__ R, const T* __restrict__ P,
                                                       const T* __restrict__ AP, const T* __restrict__ rs_in, const T* __restrict__ curv,
                                                       double* __restrict__ segpart, int G, int64_t L, Segs sg,
                                                       const Ctl* __restrict__ ctl, int it) {
  __shared__ double red[4];
  const bool stopped = ctl->stop != 0;
  const bool fallback = stopped && it == 0 && ctl->status == cg::kCurvNegative && ctl->iter == 0;
  if (stopped && !fallback) return;
  const int64_t items = (int64_t)G * sg.nseg;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / sg.nseg), seg = (int)(item % sg.nseg);
    const int64_t lo = seg * sg.seglen, hi = min(L, lo + sg.seglen), base = (int64_t)g * L;
    const T rs_old = rs_in[g], cv = curv[g];
    if (fallback) {
      const T f = (-rs_old) / cv;
      for (int64_t j = lo + threadIdx.x; j < hi; j += 256) X[base + j] = f * P[base + j];
      continue;
    }
    const T alpha = rs_old / cv;
    double s_rs = 0.0, s_abs = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
      X[base + j] = X[base + j] + alpha * P[base + j];
      const T rn = R[base + j] + alpha * AP[base + j];
      R[base + j] = rn;
      s_rs += (double)(rn * rn);
      s_abs += (double)abs_t(rn);
    }
    s_rs = block_sum(s_rs, red);
    s_abs = block_sum(s_abs, red);
    if (threadIdx.x == 0) { segpart[item * 2] = s_rs; segpart[item * 2 + 1] = s_abs; }
  }
}

// rs_new of the group from its segments' partials, p = -r + (rs_new / rs_old) p on the segment (start: not at the set-up),
// and by the group's first segment rs_out[g] and part[g] = {rs_new, sum |r|}
template <class T>
__global__ __launch_bounds__(256) void seg_finish_kernel(const T* __restrict__ R, T* __restrict__ P, const double* __restrict__ segpart,
                                                         const T* __restrict__ rs_in, T* __restrict__ rs_out, double* __restrict__ part,
                                                         int G, int64_t L, Segs sg, const Ctl* __restrict__ ctl, int start) {
  if (!start && ctl->stop != 0) return;
  const int64_t items = (int64_t)G * sg.nseg;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / sg.nseg), seg = (int)(item % sg.nseg);
    const int64_t lo = seg * sg.seglen, hi = min(L, lo + sg.seglen), base = (int64_t)g * L;
    double s_rs = 0.0, s_abs = 0.0;
    for (int q = 0; q < sg.nseg; ++q) {                               // (every workgroup of the group: the same order)
      s_rs += segpart[((int64_t)g * sg.nseg + q) * 2];
      s_abs += segpart[((int64_t)g * sg.nseg + q) * 2 + 1];
    }
    const T rs_new = (T)s_rs;
    if (!start) {
      const T beta = rs_new / rs_in[g];
      for (int64_t j = lo + threadIdx.x; j < hi; j += 256) P[base + j] = (-R[base + j]) + beta * P[base + j];
    }
    if (seg == 0 && threadIdx.x == 0) {
      rs_out[g] = rs_new;
      part[(int64_t)g * kPart] = (double)rs_new;
      part[(int64_t)g * kPart + 1] = s_abs;
    }
  }
}

// curv_g = the fold of a group's slots [nslots][G] in slot order, rounded once; block partials {sum curv_g}
template <class T>
__global__ __launch_bounds__(256) void curv_fold_kernel(const double* __restrict__ slots, int nslots, T* __restrict__ curv, int G,
                                                        double* __restrict__ cpart, const Ctl* __restrict__ ctl) {
  __shared__ double red[4];
  if (ctl->stop != 0) return;
  double tot = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int q = 0; q < nslots; ++q) s += slots[(int64_t)q * G + g];
    const T c = (T)s;
    curv[g] = c;
    tot += (double)c;
  }
  tot = block_sum(tot, red);
  if (threadIdx.x == 0) cpart[(int64_t)blockIdx.x * kPart] = tot;
}

// out (pitch ldo) = X, packed [n][k]
template <class T>
__global__ __launch_bounds__(256) void store_kernel(const T* __restrict__ X, T* __restrict__ out, int64_t ldo, int n, int k) {
  const int64_t total = (int64_t)n * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    out[(i / k) * ldo + (i % k)] = X[i];
}

// ---- the judges: one workgroup each -----------------------------------------------------------------------------------
__device__ __forceinline__ void stop_with(Ctl* ctl, int status, int it) {
  ctl->status = status;
  ctl->iter = it;
  ctl->stop = 1;
}

// in front of iteration `it`: exit 0 of iteration it - 1, exit 4, exit 1 -- in the reference's order
template <class T>
__global__ __launch_bounds__(256) void judge1_kernel(const double* __restrict__ part, int nb, Ctl* ctl, Log* __restrict__ log, int it,
                                                     int maxiter, double rtol, double tol) {
  __shared__ double red[256], out[kPart];
  if (ctl->stop != 0) return;
  fold_partials(part, nb, 2, 0, red, out);
  if (threadIdx.x != 0) return;
  if (it > 0) {
    T rs;
    const int st = cg::exit_after_step<T>(out[0], tol, &rs);
    log[(it - 1) % kLog].rs = (double)rs;
    if (st != cg::kRunning) return stop_with(ctl, st, it - 1);
  }
  if (it == maxiter) return stop_with(ctl, cg::kMaxiter, maxiter);
  if (it == 0) ctl->termcond = (double)cg::termcond<T>(rtol, out[1]);
  log[it % kLog].r_abs = (double)(T)out[1];
  if (cg::exit_before_product<T>(out[1], (T)ctl->termcond) != cg::kRunning) stop_with(ctl, cg::kRelTol, it);
}

// behind the product of iteration `it`: curv_sum from the block partials of whoever took curv, exits 2 and 3
template <class T>
__global__ __launch_bounds__(256) void judge2_kernel(const double* __restrict__ cpart, int nb, Ctl* ctl, Log* __restrict__ log, int it) {
  __shared__ double red[256], out[kPart];
  if (ctl->stop != 0) return;
  fold_partials(cpart, nb, 1, 0, red, out);
  if (threadIdx.x != 0) return;
  log[it % kLog].curv_sum = (double)(T)out[0];
  const int st = cg::exit_after_product<T>(out[0]);
  if (st != cg::kRunning) stop_with(ctl, st, it);
}

// ---- the host loop -------------------------------------------------------------------------------------------------------
template <class T>
struct State {
  T *X, *R, *P, *AP, *rs[2], *curv;
  double *slots, *segpart, *part, *cpart;
  Ctl* ctl;
  Log* log;
};

// how the passes cut a group of L elements: one wave per group (nseg = 0), or nseg >= 1 segments of seglen
Segs segments(int64_t G, int64_t L) {
  if (L <= kWaveLen) return {0, L};
  const int64_t want = std::min<int64_t>((kSegTarget + G - 1) / G, (L + kSegMin - 1) / kSegMin);
  const int64_t seglen = (L + want - 1) / want;
  return {(int)((L + seglen - 1) / seglen), seglen};
}

template <class T>
void carve_state(Arena& a, State<T>& s, int64_t G, int64_t L, int64_t product_slots) {
  const size_t gl = (size_t)G * L * sizeof(T);
  const int64_t nseg = std::max(1, segments(G, L).nseg);
  s.X = a.take<T>(gl);
  s.R = a.take<T>(gl);
  s.P = a.take<T>(gl);
  s.AP = a.take<T>(gl);
  s.rs[0] = a.take<T>((size_t)G * sizeof(T));
  s.rs[1] = a.take<T>((size_t)G * sizeof(T));
  s.curv = a.take<T>((size_t)G * sizeof(T));
  s.slots = a.take<double>((size_t)G * std::max(product_slots, nseg) * 8);
  s.segpart = a.take<double>((size_t)G * nseg * 2 * 8);
  s.part = a.take<double>((size_t)std::max<int64_t>(kRowBlocks, G) * kPart * 8);
  s.cpart = a.take<double>((size_t)kRowBlocks * kPart * 8);
  s.ctl = a.take<Ctl>(sizeof(Ctl));
  s.log = a.take<Log>(sizeof(Log) * kLog);
}

// the passes of one solve: their launch shapes, and which of the two families of kernels they are
template <class T>
struct Passes {
  State<T> s;
  int G; int64_t L;
  Segs sg;
  int grid;                           // workgroups of a pass
  int nb;                             // block partials a pass leaves in part
  hipStream_t st;
  Passes(const State<T>& s_, int G_, int64_t L_, hipStream_t st_) : s(s_), G(G_), L(L_), sg(segments(G_, L_)), st(st_) {
    grid = (int)std::min<int64_t>(kRowBlocks, sg.nseg ? (int64_t)G * sg.nseg : ((int64_t)G + 3) / 4);
    nb = sg.nseg ? G : grid;
  }
  int fold_grid() const { return (int)std::min<int64_t>(kRowBlocks, ((int64_t)G + 255) / 256); }

  int init(const T* b, int64_t ldb) const {
    if (sg.nseg) {
      hipLaunchKernelGGL(seg_init_kernel<T>, dim3(grid), dim3(256), 0, st, b, ldb, s.X, s.R, s.P, s.segpart, G, L, sg);
      hipLaunchKernelGGL(seg_finish_kernel<T>, dim3(grid), dim3(256), 0, st, s.R, s.P, s.segpart, s.rs[0], s.rs[0], s.part, G, L, sg,
                         s.ctl, 1);
    } else {
      hipLaunchKernelGGL(init_kernel<T>, dim3(grid), dim3(256), 0, st, b, ldb, s.X, s.R, s.P, s.rs[0], G, L, s.part);
    }
    LASSO_HIP_TRY(hipGetLastError());
    return LASSO_OK;
  }
  // curv and its block partials from AP as a library product left it; *nc = the partials' count
  int dot(T tik, int negate, int* nc) const {
    if (sg.nseg) {
      hipLaunchKernelGGL(seg_dot_kernel<T>, dim3(grid), dim3(256), 0, st, s.P, s.AP, s.slots, G, L, sg, tik, negate, s.ctl);
      LASSO_HIP_TRY(hipGetLastError());
      return fold(sg.nseg, nc);
    }
    hipLaunchKernelGGL(dot_kernel<T>, dim3(grid), dim3(256), 0, st, s.P, s.AP, s.curv, G, L, tik, negate, s.cpart, s.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    *nc = grid;
    return LASSO_OK;
  }
  // ... from nslots slots per group
  int fold(int nslots, int* nc) const {
    *nc = fold_grid();
    hipLaunchKernelGGL(curv_fold_kernel<T>, dim3(*nc), dim3(256), 0, st, s.slots, nslots, s.curv, G, s.cpart, s.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    return LASSO_OK;
  }
  int step(int it) const {
    const T* const rs_in = s.rs[it & 1];
    T* const rs_out = s.rs[(it + 1) & 1];
    if (sg.nseg) {
      hipLaunchKernelGGL(seg_step_kernel<T>, dim3(grid), dim3(256), 0, st, s.X, s.R, s.P, s.AP, rs_in, s.curv, s.segpart, G, L, sg,
                         s.ctl, it);
      hipLaunchKernelGGL(seg_finish_kernel<T>, dim3(grid), dim3(256), 0, st, s.R, s.P, s.segpart, rs_in, rs_out, s.part, G, L, sg,
                         s.ctl, 0);
    } else {
      hipLaunchKernelGGL(rowpass_kernel<T>, dim3(grid), dim3(256), 0, st, s.X, s.R, s.P, s.AP, rs_in, rs_out, s.curv, G, L, s.part,
                         s.ctl, it);
    }
    LASSO_HIP_TRY(hipGetLastError());
    return LASSO_OK;
  }
};

// product(nc): a lasso_status; leaves AP, curv and *nc block partials of sum curv in cpart.  chunk_cap: the most
// iterations between two host reads where a stop may fire.
template <class T, class Product>
int iterate(const Passes<T>& ps, const T* b, int64_t ldb, int chunk_cap, const lasso_cg_options& o, lasso_cg_result* res,
            Product product) {
  const State<T>& s = ps.s;
  hipStream_t st = ps.st;
  lasso_cg_trace* const tr = (res->trace && res->trace->capacity > 0) ? res->trace : nullptr;
  LASSO_HIP_TRY(hipMemsetAsync(s.ctl, 0, sizeof(Ctl), st));
  LASSO_HIP_TRY(hipMemsetAsync(s.log, 0, sizeof(Log) * kLog, st));
  if (int status = ps.init(b, ldb)) return status;
  hipLaunchKernelGGL(judge1_kernel<T>, dim3(1), dim3(256), 0, st, s.part, ps.nb, s.ctl, s.log, 0, o.maxiter, o.rtol, o.tol);
  LASSO_HIP_TRY(hipGetLastError());
  // rtol = 0 and tol = 0: only exits 2 and 3 and an exact zero are left -- nothing to read until the end (the trace's
  // ring is the one reason left to)
  const bool never = o.rtol == 0.0 && o.tol == 0.0;
  const int cap = never ? (tr ? kLog - 1 : INT32_MAX) : std::min(chunk_cap, kLog - 1);
  std::vector<Log> host(tr ? kLog : 0);
  Ctl h = {};
  int it = 0, prev = 0, fetched = 0, reads = 0;
  for (;;) {
    const int c = it < o.maxiter ? cg::next_chunk(it, o.maxiter, prev, never, cap) : 0;
    for (int j = 0; j < c; ++j, ++it) {
      int nc = 0;
      if (int status = product(&nc)) return status;
      hipLaunchKernelGGL(judge2_kernel<T>, dim3(1), dim3(256), 0, st, s.cpart, nc, s.ctl, s.log, it);
      LASSO_HIP_TRY(hipGetLastError());
      if (int status = ps.step(it)) return status;
      hipLaunchKernelGGL(judge1_kernel<T>, dim3(1), dim3(256), 0, st, s.part, ps.nb, s.ctl, s.log, it + 1, o.maxiter, o.rtol, o.tol);
      LASSO_HIP_TRY(hipGetLastError());
    }
    // the one host read of a chunk: the control record and, for a trace, the ring's entries [fetched, it]
    LASSO_HIP_TRY(hipMemcpyAsync(&h, s.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
    if (tr)
      for (int e = fetched; e <= it;) {
        const int slot = e % kLog, run = std::min(it + 1 - e, kLog - slot);
        LASSO_HIP_TRY(hipMemcpyAsync(host.data() + slot, s.log + slot, sizeof(Log) * run, hipMemcpyDeviceToHost, st));
        e += run;
      }
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    ++reads;
    if (tr) {
      for (int e = fetched; e <= it && e < tr->capacity; ++e) {
        const Log& l = host[e % kLog];
        if (tr->r_abs) tr->r_abs[e] = l.r_abs;
        if (tr->curv_sum) tr->curv_sum[e] = l.curv_sum;
        if (tr->rs) tr->rs[e] = l.rs;
      }
      fetched = it;                    // (entry `it` has only its r_abs so far: it is read again)
    }
    if (h.stop) break;
    prev = c;
  }
  res->n_iter = h.iter;
  res->status = h.status;
  res->termcond = h.termcond;
  res->host_reads = reads;
  return LASSO_OK;
}

template <class T>
struct DenseSpace {
  State<T> s;
  size_t bytes;
};

template <class T>
DenseSpace<T> carve_dense(void* base, int64_t n, int64_t k) {
  DenseSpace<T> w;
  Arena a(base);
  carve_state(a, w.s, n, k, sizeof(T) == 4 ? (k + 63) / 64 : 1);      // 64 x 64 blocks give the most slots
  w.bytes = a.bytes();
  return w;
}

struct ConvSpace {
  float *Wt, *Wp, *RC, *COLSt, *IMG;
  State<float> s;
  size_t bytes;
};

ConvSpace carve_conv(void* base, const ConvGeom& g) {
  ConvSpace w;
  Arena a(base);
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ckk = (int64_t)g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4;
  w.Wt = a.take((size_t)ckk * g.K * 4);
  w.Wp = a.take((size_t)g.K * ldr * 4);
  w.RC = a.take((size_t)M * ldr * 4);
  w.COLSt = a.take((size_t)ckk * M * 4);
  w.IMG = a.take((size_t)g.N * g.C * g.H * g.W * 4);
  carve_state(a, w.s, g.N, (int64_t)g.Hz * g.Wz * g.K, 1);
  w.bytes = a.bytes();
  return w;
}

// do the implicit synthesis kernels of the ISTA path cover the geometry?  Asked of the launchers themselves (dry runs)
bool synth_covered(const ConvGeom& g, int cus) {
  static const float kAligned[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  bool synth = false, few = false;
  (void)launch_conv_synth(kAligned, kAligned, kAligned, nullptr, g, cus, &synth, nullptr, 1);
  if (!synth) (void)launch_conv_synth_few(kAligned, kAligned, kAligned, nullptr, g, cus, &few, nullptr, 1);
  return synth || few;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t k, int dtype) {
  return (dtype == LASSO_F64 ? carve_dense<double>(nullptr, n, k).bytes : carve_dense<float>(nullptr, n, k).bytes) + 256;
}

int solve_f32(const float* A, int64_t lda, const float* b, int64_t ldb, float* xout, int64_t ldx, int64_t n64, int64_t k64,
              const lasso_cg_options& o, lasso_cg_result* res, void* workspace, hipStream_t st) {
  const int n = (int)n64, k = (int)k64;
  const State<float> s = carve_dense<float>(workspace, n, k).s;
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>((int64_t)k, lda);
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  // LASSO_FORCE_BLOCKS_128 (tests): 128 x 128 blocks below the size at which block_side takes them
  const bool force128 = (o.reserved & LASSO_FORCE_BLOCKS_128) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side = force128 ? 128 : block_side(n, k, ldmax, cus);
  const bool fused = !(o.reserved & 1);
  const int ncb = (k + side - 1) / side;
  res->form = fused ? LASSO_CG_FORM_FUSED : LASSO_CG_FORM_UNFUSED;
  const Passes<float> ps(s, n, k, st);
  auto product = [&](int* nc) -> int {
    if (fused) {
      const CurvEpi ep = {s.P, s.AP, s.slots, s.ctl, n, 0};
      LASSO_HIP_TRY(launch_gemm(s.P, k, A, lda, n, k, k, ep, side, 1, st));       // Ap = p A^T (:78)
      return ps.fold(ncb, nc);
    }
    const StoreEpi ep = {s.AP, k, 0};
    LASSO_HIP_TRY(launch_gemm(s.P, k, A, lda, n, k, k, ep, side, 1, st));
    return ps.dot(0.0f, 0, nc);
  };
  if (int status = iterate<float>(ps, b, ldb, fused ? 64 : 8, o, res, product)) return status;
  hipLaunchKernelGGL(store_kernel<float>, dim3(ew_grid((int64_t)n * k)), dim3(256), 0, st, s.X, xout, ldx, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

int solve_f64(const double* A, int64_t lda, const double* b, int64_t ldb, double* xout, int64_t ldx, int64_t n64, int64_t k64,
              const lasso_cg_options& o, lasso_cg_result* res, void* workspace, hipStream_t st) {
  const int n = (int)n64, k = (int)k64;
  const State<double> s = carve_dense<double>(workspace, n, k).s;
  res->form = LASSO_CG_FORM_UNFUSED;
  const Passes<double> ps(s, n, k, st);
  auto product = [&](int* nc) -> int {
    // gemm_f64.hip's product gives 0 - p A^T; the pass that takes curv turns the sign
    LASSO_HIP_TRY(f64::launch_gemm_sub(s.P, k, A, lda, 0, nullptr, 0, s.AP, k, n, k, k, st));
    return ps.dot(0.0, 1, nc);
  };
  if (int status = iterate<double>(ps, b, ldb, 8, o, res, product)) return status;
  hipLaunchKernelGGL(store_kernel<double>, dim3(ew_grid((int64_t)n * k)), dim3(256), 0, st, s.X, xout, ldx, n, k);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

size_t conv_workspace_bytes(const ConvGeom& g) { return carve_conv(nullptr, g).bytes + 256; }

int conv_solve(const float* w, const float* b, float* zout, const ConvGeom& g, const lasso_cg_options& o, lasso_cg_result* res,
               void* workspace, hipStream_t st) {
  const ConvSpace ws = carve_conv(workspace, g);
  const State<float>& s = ws.s;
  const int cus = device_cus();
  const int ckk = g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4, pix = g.Hz * g.Wz;
  const int64_t L = (int64_t)pix * g.K;
  const bool implicit = !(o.reserved & 1) && synth_covered(g, cus);
  res->form = implicit ? LASSO_CG_FORM_CONV_IMPLICIT : LASSO_CG_FORM_CONV_PATCHES;
  const float tik = (float)o.tik;
  const Passes<float> ps(s, g.N, L, st);
  LASSO_HIP_TRY(launch_conv_pack_w(w, ws.Wt, ws.Wp, g.K, ckk, ldr, st));
  LASSO_HIP_TRY(launch_conv_relayout(b, s.P, nullptr, g.N, g.K, pix, 1, st));      // b as rows: p = b is in place already
  auto product = [&](int* nc) -> int {
    // Adot(v) = conv2d(conv_transpose2d(v, W), W) + tik v (:98-103)
    LASSO_HIP_TRY(launch_conv_residual(s.P, ws.Wt, implicit ? w : nullptr, nullptr, ws.COLSt, ws.IMG, g, cus, st));
    LASSO_HIP_TRY(launch_conv_gradient(ws.IMG, ws.Wp, ws.RC, ldr, s.AP, g, st));
    return ps.dot(tik, 0, nc);
  };
  if (int status = iterate<float>(ps, s.P, L, 8, o, res, product)) return status;
  LASSO_HIP_TRY(launch_conv_relayout(s.X, zout, nullptr, g.N, g.K, pix, 0, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace conjgrad
}  // namespace lasso
