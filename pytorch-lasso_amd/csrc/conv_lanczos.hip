// The exact Lipschitz constant of a convolutional dictionary (the reference's lasso/conv2d/lip_const.py:8-31, there by
// ARPACK with a numpy -> torch -> numpy round trip per product): the largest eigenvalue of A = conv_transpose2d o conv2d
// on C x H x W images, or of conv2d o conv_transpose2d on K x Hz x Wz codes -- the nonzero spectra coincide, the driver
// takes the smaller space -- by plain Lanczos with full reorthogonalisation, the driver behind lasso_conv_lip_constant.
//
// State on the device: the basis Q [m + 1][ldq] (ldq = dim rounded up to whole segments, the pad is kept at zero),
// alpha [m], beta [m] in double, and a control record.  One Lanczos step j, q_j = Q[j]:
//   product   w = A q_j: the two convolution launchers the ISTA and CG paths share (fp32: launch_conv_gradient and
//             launch_conv_residual with no image to subtract; fp64: their conv_f64.hip counterparts) on a batch of one
//   dots      c = Q[0..j]^T w.  dim is cut into segments of kSeg elements, a workgroup each; a wave takes every fourth
//             basis vector, a lane 16 elements of the segment; partial dots in double, one slot per (segment, vector)
//   update<0> every workgroup folds the slots in segment order (c, in LDS), w -= Q c on its segment (accumulated in
//             double, rounded once), and takes the second pass's partial dots of the new w against Q[0..j]
//   update<1> folds those, w -= Q c again (classical Gram-Schmidt done twice), and the segment's partial of |w|^2
//   finish    beta_j = |w| (partials folded in a fixed tree), q_{j+1} = w / beta_j into Q; one thread records
//             alpha_j = c_j + c'_j and beta_j and judges the breakdown
// Four launches of this file per step, beside the product's.  A dot over dim needs every segment, so each "dot, then use
// it" is a kernel boundary: c, c' and beta are three of them, and the fourth (dots in front of update<0>) keeps the
// product's output from being read by a kernel that also rewrites it.  What could be fused is: the second pass's dots ride
// on the first update, the norm on the second, alpha on the two folds.
// Breakdown: beta_j <= eps max(alpha_0 .. alpha_j) (a lower bound of theta_j, so never looser than the host's rule), or
// a beta that is not a number, sets the control flag; every kernel of this file reads the flag first and returns once
// it is set (the library's two products run on, into a buffer nothing reads any more).
// The host reads alpha, beta and the record once per chunk of steps (lanczos_host.hpp's next_chunk), judges EVERY prefix
// T_j of the chunk in double and takes the first that stops: the value does not depend on the chunking.
// A basis beyond kMaxBasis vectors or kBasisBytes restarts from the current Ritz vector y = Q s when it is full (the
// update kernel with the coefficients -s on a zero vector), as plain restarted Lanczos.
// All sums: per thread in double, wave butterfly, slots folded in segment order -- the segmentation depends on dim
// alone, never on the device: two calls with the same arguments are bitwise equal, on any launch shape.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"
#include "lanczos_host.hpp"

namespace lasso {
namespace lanczos {
namespace {

constexpr int kSeg = 1024;                            // elements of a segment: 256 threads x one pack of 4
constexpr int64_t kBasisBytes = (int64_t)1 << 30;     // most bytes of basis vectors
constexpr int kMinBasis = 8;

template <class T> struct alignas(sizeof(T) * 4) Pack { T v[4]; };

struct Ctl { int32_t stop, steps; double amax; double cj[2]; };    // steps: Lanczos steps complete when stop was set

template <class T>
struct Dev {
  T* Q; int64_t ldq;                  // [m + 1][ldq]
  T* Wv;                              // [ldq] the product's output, then w
  double* part[2];                    // [nseg][ldp] partial dots of the two passes
  double* npart;                      // [nseg] partial |w|^2
  double* alpha; double* beta;        // [m]
  Ctl* ctl;
  int64_t dim;
  int nseg, ldp;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// partial dots of the segment's w (LDS, kSeg elements) against Q[0..j]: wave w takes the vectors w, w + 4, ...
template <class T>
__device__ __forceinline__ void segment_dots(const Dev<T>& a, const T* wl, int j, int64_t base, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Pack<T> w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = reinterpret_cast<const Pack<T>*>(wl)[lane + 64 * e];
  for (int i = wv; i <= j; i += 4) {
    const Pack<T>* const q = reinterpret_cast<const Pack<T>*>(a.Q + (int64_t)i * a.ldq + base);
    Pack<T> qv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) qv[e] = q[lane + 64 * e];
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < 4; ++c) s += (double)qv[e].v[c] * (double)w[e].v[c];
    s = wave_sum(s);
    if (lane == 0) out[(int64_t)blockIdx.x * a.ldp + i] = s;
  }
}

// Wv = the start vector: element i is a hash of i (murmur3's finaliser) mapped into (-1, 1); npart = the segments' |w|^2
template <class T>
__global__ __launch_bounds__(256) void start_kernel(const Dev<T> a) {
  __shared__ double red[4];
  const int64_t base = (int64_t)blockIdx.x * kSeg + 4 * threadIdx.x;
  Pack<T> w;
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t i = base + c;
    uint32_t h = (uint32_t)i * 0x9E3779B9u + (uint32_t)(i >> 32) + 0x7F4A7C15u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    const T v = i < a.dim ? (T)(((double)(h >> 8) + 0.5) / 8388608.0 - 1.0) : T(0);
    w.v[c] = v;
    s += (double)v * (double)v;
  }
  reinterpret_cast<Pack<T>*>(a.Wv)[(int64_t)blockIdx.x * 256 + threadIdx.x] = w;
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.npart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// first pass: the partial dots of the product's output
template <class T>
__global__ __launch_bounds__(256) void dots_kernel(const Dev<T> a, int j) {
  __shared__ __attribute__((aligned(32))) T wl[kSeg];
  if (a.ctl->stop != 0) return;
  const int64_t base = (int64_t)blockIdx.x * kSeg;
  reinterpret_cast<Pack<T>*>(wl)[threadIdx.x] = reinterpret_cast<const Pack<T>*>(a.Wv + base)[threadIdx.x];
  __syncthreads();
  segment_dots(a, wl, j, base, a.part[0]);
}

// c = the fold of `rows` rows of slots in row order; w -= Q[0..j] c on the segment.  SECOND = 0: then the partial dots of
// the new w into part[1]; SECOND = 1: the segment's |w|^2 into npart.  cj[SECOND] = c_j, for alpha.
// (The restart calls it with SECOND = 1, rows = 1, the coefficients -s in part[1] and Wv zeroed: w = Q s.)
template <class T, int SECOND>
__global__ __launch_bounds__(256) void update_kernel(const Dev<T> a, int j, int rows) {
  __shared__ double cf[kMaxBasis];
  __shared__ __attribute__((aligned(32))) T wl[kSeg];
  __shared__ double red[4];
  if (a.ctl->stop != 0) return;
  const double* const slots = a.part[SECOND];
  for (int i = threadIdx.x; i <= j; i += 256) {
    double s = 0.0;
    for (int sg = 0; sg < rows; ++sg) s += slots[(int64_t)sg * a.ldp + i];
    cf[i] = s;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSeg;
  Pack<T>* const wp = reinterpret_cast<Pack<T>*>(a.Wv + base) + threadIdx.x;
  Pack<T> w = *wp;
  double acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (double)w.v[c];
  const Pack<T>* q = reinterpret_cast<const Pack<T>*>(a.Q + base) + threadIdx.x;
  const int64_t qstep = a.ldq / 4;
  int i = 0;
  for (; i + 4 <= j + 1; i += 4) {                    // four loads in flight
    Pack<T> qv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) qv[u] = q[(int64_t)(i + u) * qstep];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double cu = cf[i + u];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] -= cu * (double)qv[u].v[c];
    }
  }
  for (; i <= j; ++i) {
    const Pack<T> qv = q[(int64_t)i * qstep];
    const double cu = cf[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] -= cu * (double)qv.v[c];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) w.v[c] = (T)acc[c];
  *wp = w;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->cj[SECOND] = cf[j];
  if constexpr (SECOND == 0) {
    reinterpret_cast<Pack<T>*>(wl)[threadIdx.x] = w;
    __syncthreads();
    segment_dots(a, wl, j, base, a.part[1]);
  } else {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) s += (double)w.v[c] * (double)w.v[c];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.npart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// beta = |w| from the segments' partials, Q[j + 1] = w / beta on the segment (zeros in the pad); j = -1: the start
// vector, nothing to record.  Thread 0 of workgroup 0 records alpha_j, beta_j and judges the breakdown.
template <class T>
__global__ __launch_bounds__(256) void finish_kernel(const Dev<T> a, int j, double eps) {
  __shared__ double red[256];
  if (a.ctl->stop != 0) return;
  double s = 0.0;
  for (int sg = threadIdx.x; sg < a.nseg; sg += 256) s += a.npart[sg];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const double beta = sqrt(red[0]);
  const T bt = (T)beta;
  const int64_t base = (int64_t)blockIdx.x * kSeg + 4 * threadIdx.x;
  Pack<T> w = reinterpret_cast<const Pack<T>*>(a.Wv)[(int64_t)blockIdx.x * 256 + threadIdx.x];
#pragma unroll
  for (int c = 0; c < 4; ++c) w.v[c] = base + c < a.dim ? w.v[c] / bt : T(0);
  reinterpret_cast<Pack<T>*>(a.Q + (int64_t)(j + 1) * a.ldq)[(int64_t)blockIdx.x * 256 + threadIdx.x] = w;
  if (blockIdx.x == 0 && threadIdx.x == 0 && j >= 0) {
    const double alpha = a.ctl->cj[0] + a.ctl->cj[1];
    a.alpha[j] = alpha;
    a.beta[j] = beta;
    const double amax = j == 0 ? alpha : fmax(a.ctl->amax, alpha);
    a.ctl->amax = amax;
    if (!(beta > eps * amax)) {       // (a NaN stops it too: nothing after it is a number)
      a.ctl->steps = j + 1;
      a.ctl->stop = 1;
    }
  }
}

// ---- the host side -------------------------------------------------------------------------------------------------
struct Plan {
  int64_t dim, ldq;
  int nseg, ldp, m;                   // m: basis vectors of a cycle
};

Plan make_plan(const ConvGeom& g, int code_space, int maxiter, int dtype) {
  Plan p;
  p.dim = code_space ? (int64_t)g.K * g.Hz * g.Wz : (int64_t)g.C * g.H * g.W;
  p.nseg = (int)((p.dim + kSeg - 1) / kSeg);
  p.ldq = (int64_t)p.nseg * kSeg;
  p.m = basis_size(p.dim, maxiter, dtype);
  p.ldp = (p.m + 7) / 8 * 8;
  return p;
}

// the workspace of the two products (fp32: as conjgrad.hip's convolutional form; fp64: the patch columns and an image)
struct ProductSpace {
  float *Wt, *Wp, *RC, *COLSt;        // fp32
  double* COLS;                       // fp64
  void* other;                        // the vector of the other space between the two products
};

template <class T>
struct Space {
  ProductSpace ps;
  Dev<T> d;
  size_t bytes;
};

template <class T>
Space<T> carve(void* base, const ConvGeom& g, int code_space, const Plan& p) {
  Space<T> w = {};
  Arena a(base);
  const int64_t M = (int64_t)g.Hz * g.Wz, ckk = (int64_t)g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4;
  const int64_t other = code_space ? (int64_t)g.C * g.H * g.W : M * g.K;
  if (sizeof(T) == 4) {
    w.ps.Wt = a.take((size_t)ckk * g.K * 4);
    w.ps.Wp = a.take((size_t)g.K * ldr * 4);
    w.ps.RC = a.take((size_t)M * ldr * 4);
    w.ps.COLSt = a.take((size_t)ckk * M * 4);
  } else {
    w.ps.COLS = a.take<double>((size_t)M * ckk * 8);
  }
  w.ps.other = a.take<T>((size_t)other * sizeof(T));
  w.d.ldq = p.ldq;
  w.d.dim = p.dim;
  w.d.nseg = p.nseg;
  w.d.ldp = p.ldp;
  w.d.Wv = a.take<T>((size_t)p.ldq * sizeof(T));
  w.d.part[0] = a.take<double>((size_t)p.nseg * p.ldp * 8);
  w.d.part[1] = a.take<double>((size_t)p.nseg * p.ldp * 8);
  w.d.npart = a.take<double>((size_t)p.nseg * 8);
  w.d.alpha = a.take<double>((size_t)p.m * 8);
  w.d.beta = a.take<double>((size_t)p.m * 8);
  w.d.ctl = a.take<Ctl>(sizeof(Ctl));
  w.d.Q = a.take<T>((size_t)(p.m + 1) * p.ldq * sizeof(T));
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

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    cus = 1;
  return cus;
}

// out = A in: both products, through the vector of the other space
struct ProductF32 {
  const float* w; ProductSpace ps; ConvGeom g; int code_space, cus; bool implicit;
  int operator()(const float* in, float* out, hipStream_t st) const {
    const int ldr = (g.C * g.kh * g.kw + 3) / 4 * 4;
    float* const other = static_cast<float*>(ps.other);
    if (code_space) {                 // conv2d(conv_transpose2d(v))
      LASSO_HIP_TRY(launch_conv_residual(in, ps.Wt, implicit ? w : nullptr, nullptr, ps.COLSt, other, g, cus, st));
      LASSO_HIP_TRY(launch_conv_gradient(other, ps.Wp, ps.RC, ldr, out, g, st));
    } else {                          // conv_transpose2d(conv2d(v))
      LASSO_HIP_TRY(launch_conv_gradient(in, ps.Wp, ps.RC, ldr, other, g, st));
      LASSO_HIP_TRY(launch_conv_residual(other, ps.Wt, implicit ? w : nullptr, nullptr, ps.COLSt, out, g, cus, st));
    }
    return LASSO_OK;
  }
};

struct ProductF64 {
  const double* w; ProductSpace ps; ConvGeom g; int code_space;
  int operator()(const double* in, double* out, hipStream_t st) const {
    double* const other = static_cast<double*>(ps.other);
    if (code_space) {
      if (int s = f64::launch_conv_synthesis(in, w, ps.COLS, other, g, st)) return s;
      return f64::launch_conv_gradient(other, w, out, g, st);
    }
    if (int s = f64::launch_conv_gradient(in, w, other, g, st)) return s;
    return f64::launch_conv_synthesis(other, w, ps.COLS, out, g, st);
  }
};

template <class T, class Product>
int iterate(const Dev<T>& d, const Plan& p, const lasso_conv_lip_options& o, lasso_conv_lip_result* res, const Product& product,
            hipStream_t st) {
  const double eps = (double)std::numeric_limits<T>::epsilon();
  const dim3 grid(p.nseg), block(256);
  LASSO_HIP_TRY(hipMemsetAsync(d.ctl, 0, sizeof(Ctl), st));
  LASSO_HIP_TRY(hipMemsetAsync(d.Wv, 0, (size_t)p.ldq * sizeof(T), st));
  hipLaunchKernelGGL(start_kernel<T>, grid, block, 0, st, d);
  hipLaunchKernelGGL(finish_kernel<T>, grid, block, 0, st, d, -1, eps);
  LASSO_HIP_TRY(hipGetLastError());
  std::vector<double> alpha(p.m), beta(p.m), vec(p.m);
  Ctl h = {};
  int total = 0, reads = 0, matvecs = 0, restarts = 0, status = kRunning;
  Verdict last = {kRunning, NAN, NAN};
  while (status == kRunning) {
    // one cycle: up to m steps on a fresh T
    int j = 0, judged = 0, prev = 0;
    const int cycle = std::min(p.m, o.maxiter - total);
    while (status == kRunning && j < cycle) {
      const int c = next_chunk(prev, cycle - j);
      for (int s = 0; s < c; ++s, ++j, ++matvecs) {
        if (int e = product(d.Q + (int64_t)j * p.ldq, d.Wv, st)) return e;
        hipLaunchKernelGGL(dots_kernel<T>, grid, block, 0, st, d, j);
        hipLaunchKernelGGL((update_kernel<T, 0>), grid, block, 0, st, d, j, p.nseg);
        hipLaunchKernelGGL((update_kernel<T, 1>), grid, block, 0, st, d, j, p.nseg);
        hipLaunchKernelGGL(finish_kernel<T>, grid, block, 0, st, d, j, eps);
        LASSO_HIP_TRY(hipGetLastError());
      }
      // the one host read of a chunk
      LASSO_HIP_TRY(hipMemcpyAsync(alpha.data() + judged, d.alpha + judged, sizeof(double) * (j - judged), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipMemcpyAsync(beta.data() + judged, d.beta + judged, sizeof(double) * (j - judged), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipMemcpyAsync(&h, d.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
      ++reads;
      const int valid = h.stop ? h.steps : j;          // (entries behind a set flag were never written)
      for (int n = judged + 1; n <= valid && status == kRunning; ++n) {
        const Verdict v = judge(alpha.data(), beta.data(), n, o.tol, eps, restarts ? INT64_MAX : p.dim);
        if (v.status != kNonFinite) last = v;
        ++total;
        if (res->history && total <= res->history_capacity) res->history[total - 1] = v.theta;
        status = v.status;
      }
      if (status == kRunning && h.stop)
        return fail(LASSO_ERR_HIP, "lanczos: the device stopped at step %d and the host found no reason to", h.steps);
      judged = valid;
      prev = c;
    }
    if (status != kRunning) break;
    if (total >= o.maxiter) { status = kMaxiter; break; }
    // the basis is full: go on from the Ritz vector y = Q s (plain restart)
    (void)top_ritz(alpha.data(), beta.data(), cycle, vec.data());
    for (int i = 0; i < cycle; ++i) vec[i] = -vec[i];
    LASSO_HIP_TRY(hipMemsetAsync(d.Wv, 0, (size_t)p.ldq * sizeof(T), st));
    LASSO_HIP_TRY(hipMemcpyAsync(d.part[1], vec.data(), sizeof(double) * cycle, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((update_kernel<T, 1>), grid, block, 0, st, d, cycle - 1, 1);
    hipLaunchKernelGGL(finish_kernel<T>, grid, block, 0, st, d, -1, eps);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(hipStreamSynchronize(st));            // (vec is reused by the next cycle)
    ++restarts;
  }
  res->status = status == kConverged ? LASSO_LIP_CONVERGED : status == kBreakdown ? LASSO_LIP_BREAKDOWN
              : status == kMaxiter ? LASSO_LIP_MAXITER : LASSO_LIP_NONFINITE;
  res->theta = status == kNonFinite ? NAN : last.theta;
  res->residual = status == kNonFinite ? NAN : last.residual;
  res->steps = total;
  res->matvecs = matvecs;
  res->host_reads = reads;
  res->restarts = restarts;
  return LASSO_OK;
}

}  // namespace

int basis_size(int64_t dim, int maxiter, int dtype) {
  const int64_t ldq = (dim + kSeg - 1) / kSeg * kSeg, item = dtype == LASSO_F64 ? 8 : 4;
  const int64_t by_bytes = std::max<int64_t>(kMinBasis, kBasisBytes / (ldq * item) - 1);
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)maxiter, dim, (int64_t)kMaxBasis, by_bytes}));
}

size_t workspace_bytes(const ConvGeom& g, int code_space, int maxiter, int dtype) {
  const Plan p = make_plan(g, code_space, maxiter, dtype);
  return (dtype == LASSO_F64 ? carve<double>(nullptr, g, code_space, p).bytes : carve<float>(nullptr, g, code_space, p).bytes) + 256;
}

int run(const void* w, const ConvGeom& g, int code_space, int dtype, const lasso_conv_lip_options& o, lasso_conv_lip_result* res,
        void* workspace, hipStream_t st) {
  const Plan p = make_plan(g, code_space, o.maxiter, dtype);
  res->dim = p.dim;
  res->space = code_space ? LASSO_LIP_SPACE_CODE : LASSO_LIP_SPACE_IMAGE;
  if (dtype == LASSO_F64) {
    const Space<double> ws = carve<double>(workspace, g, code_space, p);
    const ProductF64 product = {static_cast<const double*>(w), ws.ps, g, code_space};
    return iterate<double>(ws.d, p, o, res, product, st);
  }
  const Space<float> ws = carve<float>(workspace, g, code_space, p);
  const int cus = device_cus(), ckk = g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4;
  const ProductF32 product = {static_cast<const float*>(w), ws.ps, g, code_space, cus, synth_covered(g, cus)};
  LASSO_HIP_TRY(launch_conv_pack_w(product.w, ws.ps.Wt, ws.ps.Wp, g.K, ckk, ldr, st));
  return iterate<float>(ws.d, p, o, res, product, st);
}

}  // namespace lanczos
}  // namespace lasso
