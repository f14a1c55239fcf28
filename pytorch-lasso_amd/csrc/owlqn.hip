// OWL-QN (the reference's lasso/nonlinear/owlqn.py with fun(z) = 0.5 |z W^T - x|^2) on the fp32 MFMA GEMM: the driver
// behind lasso_owlqn_solve.  min 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch with the L-BFGS operator of the
// last `history` pairs (s, y) = (z - z_prev, g - g_prev) in place of a Hessian: no k x k matrix, no cap on k.
// The same driver is behind lasso_owlqn_glm_solve, where fun(z) = sum softplus(u) - x u with u = z W^T (the Bernoulli
// family): LinkEpi<true> / LinkEpi<false> stand in for EPI_RESID / EPI_TRIAL, the buffer of resid holds
// r = sigmoid(u) - x, the objective's scale is 1 instead of 0.5, and everything else below is shared.
//
// Products (solver_common.hpp's gemm_kernel with an epilogue):
//   EPI_RESID  resid = z W^T - x stored, block partials of |resid|^2                                 (orthant_common.hpp)
//   GradEpi    g = resid W on the accumulators; reads z (and z_prev, g_prev); stores g, v = -pseudo-gradient and the
//              candidate pair s = z - z_prev, y = g - g_prev into the next ring slot; block partials of sum |z|,
//              sum |pg|, y.s and y.y
//   EPI_TRIAL  |z_t W^T - x|^2 of the candidates z_t (blockIdx.z = rung): block partials only     (orthant_common.hpp)
// The line search is orthant_common.hpp's trial_kernel / decide_kernel / accept_kernel, as in own.hip.
//
// The direction d = project(H v, v) is the two-loop recursion in its vector-free form: with the held pairs i = 0 (oldest)
// .. m-1, H v = gamma v + sum_i c_i s_i + sum_i e_i y_i, and c, e, gamma follow from the small arrays S^T Y, Y^T Y, S^T v,
// Y^T v alone:
//   first loop   a_i = (s_i.v - sum_{j>i} a_j s_i.y_j) / s_i.y_i                        i = m-1 .. 0
//   second loop  b_i = (gamma (y_i.v - sum_j a_j y_i.y_j) + sum_{j<i} c_j s_j.y_i) / s_i.y_i,  c_i = a_i - b_i   i = 0 .. m-1
//   e_i = -gamma a_i,  gamma = s.y / y.y of the newest pair (1 without pairs)
//   dots_kernel    pass A: the state [n k] in fixed segments of kSeg elements, one workgroup each: v's (and a newly held
//                  pair's) segment stays in registers, every held s_i, y_i streams by once; partial dots in double, one slot
//                  per (segment, dot, pair)
//   coef_kernel    ONE workgroup: folds the slots in segment order, writes the new pair's row and column of S^T Y and
//                  Y^T Y (double, indexed by physical ring slot: a pair that leaves needs no shifting), runs both loops
//   combine_kernel pass B: d = project(gamma v + S c + Y e, v), accumulated in double, rounded once
// Two passes over the history (about 4m vector reads) and three launches per iteration, against the 2m dependent dot / axpy
// pairs (about 8m vector reads) of the recursion launched vector by vector.
//
// The host reads ONE control record at the end of an iteration: f, |dz|^2 and the pair's verdict y.s > 1e-10.  Ring head,
// count and which buffer is z_prev / g_prev are host state (lbfgs_ring_host.hpp).  No float atomics; segmentation depends
// on n k alone: two solves of the same arguments are bitwise equal.
#include "brent_host.hpp"
#include "lbfgs_ring_host.hpp"
#include "orthant_common.hpp"

namespace lasso {
namespace owlqn {
namespace {

using namespace solver;
using namespace orthant;

constexpr int kSeg = 4096;            // elements of a segment of the state: 256 threads x 4 float4
constexpr int kSegVec = kSeg / 1024;  // float4 per thread and vector
constexpr int kDots = 5;              // v.s_j, v.y_j, s_new.y_j, y_new.s_j, y_new.y_j
constexpr int kCoefThreads = 1024;
constexpr float kCurvMin = 1e-10f;    // L_BFGS.update: the pair is dropped when y.s <= 1e-10

// control record (device; the host reads it once per decision): the line search's block, then what an iteration's end adds
struct QnCtl {
  Ctl c;
  double pgl1;                        // |pseudo-gradient|_1 of the current z
  double ys, yy;                      // y.s and y.y of the candidate pair
  int keep, pad;                      // y.s > 1e-10
};

// what coef_kernel leaves for combine_kernel: gamma, then c and e by physical slot
struct CoefView {
  double* gamma;
  double* c;
  double* e;
};

// g = resid W: stores g, v and the candidate pair; partials {sum |z|, sum |pg|, y.s, y.y}
struct GradEpi {
  const float* Z;                     // the code z (ld nn)
  const float* Zp;                    // pair != 0: z_prev, g_prev
  const float* Gp;
  float* G;                           // g
  float* V;                           // v = -pseudo-gradient
  float* S;                           // pair != 0: the ring slot of the candidate (nullable: partials only)
  float* Y;
  int64_t a_stride;
  double* part;                       // [blocks][kPart]
  float alpha;
  int pair;

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const bool store_pair = pair && S != nullptr;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const __amdgpu_buffer_rsrc_t zrs = t.rsrc(Z, ldn), grs = t.rsrc(G, ldn), vrs = t.rsrc(V, ldn);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o[NJ][4];
      t.offs(mi, ldn, o);
      float z[NJ][4];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) z[nj][rg] = t.ld32(zrs, o[nj][rg]);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          // pseudo_grad(), owlqn.py:58-65: the right derivative if it is negative, the left if it is positive, else 0
          const float zz = z[nj][rg], g = acc[mi][nj][rg];
          const float sg = zz > 0.0f ? alpha : (zz < 0.0f ? -alpha : 0.0f);      // alpha * sign(z)
          const float right = __fadd_rn(g, zz == 0.0f ? alpha : sg);
          const float left = __fadd_rn(g, zz == 0.0f ? -alpha : sg);
          float pg = 0.0f;
          if (right < 0.0f) pg = right;
          if (left > 0.0f) pg = left;
          if (t.inside(o[nj][rg])) {
            s[0] += (double)fabsf(zz);
            s[1] += (double)fabsf(pg);
          }
          t.st32(g, grs, o[nj][rg]);
          t.st32(-pg, vrs, o[nj][rg]);
        }
      if (pair) {
        const __amdgpu_buffer_rsrc_t zprs = t.rsrc(Zp, ldn), gprs = t.rsrc(Gp, ldn);
        float sv[NJ][4], yv[NJ][4];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            sv[nj][rg] = t.ld32(zprs, o[nj][rg]);
            yv[nj][rg] = t.ld32(gprs, o[nj][rg]);
          }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            sv[nj][rg] = __fsub_rn(z[nj][rg], sv[nj][rg]);
            yv[nj][rg] = __fsub_rn(acc[mi][nj][rg], yv[nj][rg]);
            if (t.inside(o[nj][rg])) {
              s[2] = fma((double)yv[nj][rg], (double)sv[nj][rg], s[2]);
              s[3] = fma((double)yv[nj][rg], (double)yv[nj][rg], s[3]);
            }
          }
        if (store_pair) {
          const __amdgpu_buffer_rsrc_t srs = t.rsrc(S, ldn), yrs = t.rsrc(Y, ldn);
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              t.st32(sv[nj][rg], srs, o[nj][rg]);
              t.st32(yv[nj][rg], yrs, o[nj][rg]);
            }
        }
      }
    }
    float nomax[1] = {0.0f};
    block_fold<4, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(part));
  }
};

// The Bernoulli family's link on the accumulators u = z W^T against the targets x (the counterparts of EPI_RESID and
// EPI_TRIAL): loss = softplus(u) - x u, r = d loss / d u = sigmoid(u) - x, both from e = exp(-|u|) <= 1 alone -- no
// exp(+|u|), so |u| > 88.7 stays finite (loss -> max(u, 0) - x u, r -> {0, 1} - x).  STORE: r goes to Out (ld nn);
// block partials {sum of the float32 losses, added in double}.  A lane outside the tile holds u = 0, worth log 2: it is
// left out of the sum, and its r = 0.5 - x is dropped by the buffer bounds like every store outside the operand.
template <bool STORE>
struct LinkEpi {
  const float* X; int64_t ldx;        // the targets x [m][nn]
  float* Out;                         // STORE: r (ld nn)
  int64_t a_stride;                   // !STORE: per rung offset of the A operand
  double* part;                       // [rungs][blocks][kPart]

  template <int BM, int BN>
  __device__ __forceinline__ void run(const Tile<BM, BN>& t, f32x4 (&acc)[BM / 32][BN / 32], char* smem) const {
    constexpr int MI = BM / 32, NJ = BN / 32;
    const int64_t ldn = t.nn;
    const __amdgpu_buffer_rsrc_t xrs = t.rsrc(X, ldx);
    __amdgpu_buffer_rsrc_t ors = xrs;
    if constexpr (STORE) ors = t.rsrc(Out, ldn);
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
          const float u = acc[mi][nj][rg], xx = x[nj][rg];
          const float e = expf(-fabsf(u));
          const float loss = __fadd_rn(__fsub_rn(fmaxf(u, 0.0f), __fmul_rn(xx, u)), log1pf(e));
          if (t.inside(o[nj][rg])) s[0] += (double)loss;
          if constexpr (STORE) {
            const float r = __fsub_rn(__fdiv_rn(u >= 0.0f ? 1.0f : e, __fadd_rn(1.0f, e)), xx);
            t.st32(r, ors, o[nj][rg]);
          }
        }
    }
    float nomax[1] = {0.0f};
    block_fold<1, 0>(s, nomax, reinterpret_cast<double*>(smem), t.partial(part));
  }
};

// f = scale * (the loss sum RESID or the link left: 0.5 |resid|^2, or 1 x the Bernoulli loss) + alpha |z|_1 of the
// current z, |pg|_1, and the candidate pair's y.s, y.y and verdict, from the partials of the two products
__global__ __launch_bounds__(256) void eval_kernel(const double* __restrict__ part_r, int nb_r, const double* __restrict__ part_g,
                                                   int nb_g, double scale, double alpha, QnCtl* __restrict__ ctl) {
  __shared__ double red[256], a[kPart], b[kPart];
  fold_partials(part_r, nb_r, 1, 0, red, a);
  fold_partials(part_g, nb_g, 4, 0, red, b);
  if (threadIdx.x == 0) {
    ctl->c.rr = a[0];
    ctl->c.l1 = b[0];
    ctl->c.f = scale * a[0] + alpha * b[0];
    ctl->c.f32 = __fadd_rn(__fmul_rn((float)scale, (float)a[0]), __fmul_rn((float)alpha, (float)b[0]));
    ctl->pgl1 = b[1];
    ctl->ys = b[2];
    ctl->yy = b[3];
    ctl->keep = (float)b[2] > kCurvMin ? 1 : 0;      // (a NaN is dropped)
  }
}

// the held pairs of the ring, as the kernels see them
struct RingView {
  const float* S;                     // [slots][stride]
  const float* Y;
  int64_t stride;
  int head, count, slots;
  int fresh;                          // physical slot of a pair held since the last direction, -1: none
  __device__ __forceinline__ int slot(int i) const { return (head + i) % slots; }
};

struct Frag { float4 q[kSegVec]; };

// this thread's kSegVec float4 of the segment of p: element first + 1024 c + 4 tid .. + 3; zeros beyond total
__device__ __forceinline__ void load_frag(const float* __restrict__ p, int64_t first, int64_t total, Frag& f) {
#pragma unroll
  for (int c = 0; c < kSegVec; ++c) {
    const int64_t i = first + c * 1024 + 4 * (int)threadIdx.x;
    if (i + 3 < total) {
      f.q[c] = *reinterpret_cast<const float4*>(p + i);
    } else {
      f.q[c].x = i < total ? p[i] : 0.0f;
      f.q[c].y = i + 1 < total ? p[i + 1] : 0.0f;
      f.q[c].z = i + 2 < total ? p[i + 2] : 0.0f;
      f.q[c].w = 0.0f;
    }
  }
}

__device__ __forceinline__ double dot_frag(const Frag& a, const Frag& b) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < kSegVec; ++c) {
    s = fma((double)a.q[c].x, (double)b.q[c].x, s);
    s = fma((double)a.q[c].y, (double)b.q[c].y, s);
    s = fma((double)a.q[c].z, (double)b.q[c].z, s);
    s = fma((double)a.q[c].w, (double)b.q[c].w, s);
  }
  return s;
}

// pass A: segment blockIdx.x.  out [segments][kDots][slots]: the partial dots against the held pair in physical slot j
template <bool FRESH>
__global__ __launch_bounds__(256) void dots_kernel(const float* __restrict__ V, RingView r, int64_t total,
                                                   double* __restrict__ out) {
  constexpr int ND = FRESH ? kDots : 2;
  __shared__ double red[2][4][kDots];
  const int64_t first = (int64_t)blockIdx.x * kSeg;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Frag v, sn, yn;
  load_frag(V, first, total, v);
  if constexpr (FRESH) {
    load_frag(r.S + (int64_t)r.fresh * r.stride, first, total, sn);
    load_frag(r.Y + (int64_t)r.fresh * r.stride, first, total, yn);
  }
  double* const mine = out + (int64_t)blockIdx.x * kDots * r.slots;
  for (int i = 0; i < r.count; ++i) {
    const int j = r.slot(i);
    Frag s, y;
    load_frag(r.S + (int64_t)j * r.stride, first, total, s);
    load_frag(r.Y + (int64_t)j * r.stride, first, total, y);
    double p[ND];
    p[0] = dot_frag(v, s);
    p[1] = dot_frag(v, y);
    if constexpr (FRESH) {
      p[2] = dot_frag(sn, y);
      p[3] = dot_frag(yn, s);
      p[4] = dot_frag(yn, y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int q = 0; q < ND; ++q) p[q] += __shfl_xor(p[q], off);
    double (&rd)[4][kDots] = red[i & 1];
    if (lane == 0)
#pragma unroll
      for (int q = 0; q < ND; ++q) rd[w][q] = p[q];
    __syncthreads();                  // (two buffers: the slot written two pairs ago has been read)
    if ((int)threadIdx.x < ND) {
      const int q = threadIdx.x;
      mine[q * r.slots + j] = (rd[0][q] + rd[1][q]) + (rd[2][q] + rd[3][q]);
    }
  }
}

// sum over the lanes of a wave, the same bits in every lane
__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  return a;
}

// ONE workgroup: folds pass A's slots in segment order, brings S^T Y (SY [slots][slots], SY[i][j] = s_i.y_j) and
// Y^T Y up to date, and runs the two loops on the small vectors (wave 0).  Dynamic LDS: 4 x slots doubles.
__global__ __launch_bounds__(kCoefThreads) void coef_kernel(const double* __restrict__ part, int nseg, RingView r,
                                                            double* __restrict__ SY, double* __restrict__ YY, CoefView out) {
  extern __shared__ double lds[];
  double* const sv = lds;                          // s_j.v by physical slot
  double* const yv = lds + r.slots;                // y_j.v
  double* const al = lds + 2 * r.slots;            // a_i by age
  double* const cf = lds + 3 * r.slots;            // c_i by age
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nd = r.fresh >= 0 ? kDots : 2;
  for (int idx = w; idx < nd * r.count; idx += kCoefThreads / 64) {
    const int q = idx / r.count, j = r.slot(idx % r.count);
    double a = 0.0;
    for (int sgm = lane; sgm < nseg; sgm += 64) a += part[((int64_t)sgm * kDots + q) * r.slots + j];
    a = wave_sum(a);
    if (lane == 0) {
      if (q == 0) sv[j] = a;
      else if (q == 1) yv[j] = a;
      else if (q == 2) SY[(int64_t)r.fresh * r.slots + j] = a;
      else if (q == 3) { if (j != r.fresh) SY[(int64_t)j * r.slots + r.fresh] = a; }
      else { YY[(int64_t)r.fresh * r.slots + j] = a; YY[(int64_t)j * r.slots + r.fresh] = a; }
    }
  }
  __syncthreads();
  if (w != 0) return;
  const int m = r.count;
  double gamma = 1.0;
  if (m > 0) {
    const int64_t jn = r.slot(m - 1);
    gamma = SY[jn * r.slots + jn] / YY[jn * r.slots + jn];
  }
  // every lane stores the (identical) value it computed: a lane's later loads follow its own store in program order
  for (int i = m - 1; i >= 0; --i) {
    const int64_t j = r.slot(i);
    double a = 0.0;
    for (int i2 = i + 1 + lane; i2 < m; i2 += 64) a = fma(al[i2], SY[j * r.slots + r.slot(i2)], a);
    a = wave_sum(a);
    al[i] = (sv[j] - a) / SY[j * r.slots + j];
    __builtin_amdgcn_wave_barrier();
  }
  for (int i = 0; i < m; ++i) {
    const int64_t j = r.slot(i);
    double a = 0.0, b = 0.0;
    for (int i2 = lane; i2 < m; i2 += 64) a = fma(al[i2], YY[j * r.slots + r.slot(i2)], a);
    for (int i2 = lane; i2 < i; i2 += 64) b = fma(cf[i2], SY[(int64_t)r.slot(i2) * r.slots + j], b);
    a = wave_sum(a);
    b = wave_sum(b);
    const double beta = (gamma * (yv[j] - a) + b) / SY[j * r.slots + j];
    cf[i] = al[i] - beta;
    __builtin_amdgcn_wave_barrier();
  }
  for (int i = lane; i < m; i += 64) {
    out.c[r.slot(i)] = cf[i];
    out.e[r.slot(i)] = -gamma * al[i];
  }
  if (lane == 0) out.gamma[0] = gamma;
}

// pass B: D = project(gamma v + sum_i c_i s_i + sum_i e_i y_i, v), oldest pair first, in double, rounded once
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ V, RingView r,
                                                      const double* __restrict__ gamma_p, const double* __restrict__ cs,
                                                      const double* __restrict__ es, int64_t total, float* __restrict__ D) {
  const double gamma = gamma_p[0];
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 1024) {
    const bool whole = i + 3 < total;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (whole) {
      const float4 q = *reinterpret_cast<const float4*>(V + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (int u = 0; u < 4; ++u)
        if (i + u < total) v[u] = V[i + u];
    }
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = gamma * (double)v[u];
#pragma unroll 4
    for (int h = 0; h < r.count; ++h) {
      const int j = r.slot(h);
      const double c = cs[j], e = es[j];
      const float* const sp = r.S + (int64_t)j * r.stride + i;
      const float* const yp = r.Y + (int64_t)j * r.stride + i;
      float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (whole) {
        const float4 qs = *reinterpret_cast<const float4*>(sp), qy = *reinterpret_cast<const float4*>(yp);
        s[0] = qs.x; s[1] = qs.y; s[2] = qs.z; s[3] = qs.w;
        y[0] = qy.x; y[1] = qy.y; y[2] = qy.z; y[3] = qy.w;
      } else {
        for (int u = 0; u < 4; ++u)
          if (i + u < total) { s[u] = sp[u]; y[u] = yp[u]; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = fma(e, (double)y[u], fma(c, (double)s[u], a[u]));
    }
    float d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = keep_sign((float)a[u], v[u] > 0.0f, v[u] < 0.0f);
    if (whole) {
      *reinterpret_cast<float4*>(D + i) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
      for (int u = 0; u < 4; ++u)
        if (i + u < total) D[i + u] = d[u];
    }
  }
}

struct Space {
  float *Wt, *Zb[2], *Gb[2], *V, *D, *R, *Zc, *S, *Y;
  double *part_r, *part_g, *part_t, *dots, *SY, *YY, *coef;
  QnCtl* ctl;
  int64_t stride;                     // elements between ring slots
  int nseg;
  size_t bytes;
};

// the pair of events around the direction's launches (bit 1 of options.reserved)
struct DirectionTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false, pending = false;
  explicit DirectionTimer(bool enabled) { on = enabled && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
  ~DirectionTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void begin(hipStream_t st) { if (on) (void)hipEventRecord(a, st); }
  void end(hipStream_t st) { if (on) pending = hipEventRecord(b, st) == hipSuccess; }
  // after a synchronisation of the stream: the time between the two events, once
  double collect() {
    float ms = 0.0f;
    if (!pending || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = 0.0f;
    pending = false;
    return ms;
  }
};

Space carve(void* base, int64_t n, int64_t d, int64_t k, int64_t pairs) {
  Space w;
  Arena a(base);
  const int64_t total = n * k, slots = pairs + 1;
  const size_t nk = (size_t)total * 4, nd = (size_t)n * d * 4;
  w.stride = (total + 63) / 64 * 64;
  w.nseg = (int)((total + kSeg - 1) / kSeg);
  w.Wt = a.take((size_t)k * d * 4);
  for (int b = 0; b < 2; ++b) w.Zb[b] = a.take(nk);
  for (int b = 0; b < 2; ++b) w.Gb[b] = a.take(nk);
  w.V = a.take(nk);
  w.D = a.take(nk);
  w.R = a.take(nd);
  w.Zc = a.take(nk * kRungs);
  w.S = a.take((size_t)w.stride * 4 * slots);
  w.Y = a.take((size_t)w.stride * 4 * slots);
  // block partials: 64 x 64 blocks give the most
  w.part_r = a.take<double>((size_t)gemm_parts((int)n, (int)d, 64) * kPart * 8 * kRungs);
  w.part_g = a.take<double>((size_t)gemm_parts((int)n, (int)k, 64) * kPart * 8);
  w.part_t = a.take<double>((size_t)kEwBlocks * kPart * 8 * kRungs);
  w.dots = a.take<double>((size_t)std::max(w.nseg, 1) * kDots * slots * 8);
  w.SY = a.take<double>((size_t)slots * slots * 8);
  w.YY = a.take<double>((size_t)slots * slots * 8);
  w.coef = a.take<double>((size_t)(2 * slots + 1) * 8);
  w.ctl = a.take<QnCtl>(sizeof(QnCtl));
  w.bytes = a.bytes();
  return w;
}

}  // namespace

// pairs the solve can hold at most: the update behind the last iteration is never used
int pairs_needed(const lasso_owlqn_options& o) { return std::max(0, std::min(o.history_size, o.maxiter - 1)); }

size_t workspace_bytes(int64_t n, int64_t d, int64_t k, int64_t pairs) { return carve(nullptr, n, d, k, pairs).bytes + 256; }

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha, int family, const lasso_owlqn_options& o,
          lasso_owlqn_result* res, void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  if (family != kFamilyRss && family != LASSO_GLM_BERNOULLI) return fail(LASSO_ERR_UNSUPPORTED, "OWL-QN: family %d", family);
  const bool glm = family != kFamilyRss;
  const double scale = glm ? 1.0 : 0.5;                     // f = scale * (the loss sum of the first product) + alpha |z|_1
  PairRing ring(pairs_needed(o));
  const Space ws = carve(workspace, n, d, k, ring.capacity());
  const int cus = device_cus();
  const int64_t ldmax = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw});
  if (ldmax * 64 * 4 >= ((int64_t)1 << 31)) return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  const bool force128 = (o.reserved & 1) && ldmax * 128 * 4 < ((int64_t)1 << 31);
  const int side_k = force128 ? 128 : block_side(n, k, ldmax, cus);      // products [n,k]
  const int side_d = force128 ? 128 : block_side(n, d, ldmax, cus);      // products [n,d]
  const int pk = gemm_parts(n, k, side_k), pd = gemm_parts(n, d, side_d);
  const int64_t nk = (int64_t)n * k;
  const int gk = ew_grid(nk);
  const int gb = (int)std::max<int64_t>(1, std::min<int64_t>(65536, (nk + 1023) / 1024));
  const size_t coef_lds = (size_t)4 * ring.slots() * sizeof(double);
  lasso_owlqn_trace* const tr = res->trace;
  if (tr) tr->eval_count = 0;
  const CoefView coef = {ws.coef, ws.coef + 1, ws.coef + 1 + ring.slots()};
  static_assert((size_t)4 * (kMaxPairs + 1) * sizeof(double) <= 48 * 1024, "coef_kernel's LDS");

  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, d, k, ws.Wt, d, k, d, st));

  TwoBuffers zb;                                            // z / z_prev
  int gprev = 0;                                            // g_prev is Gb[gprev]; a new g goes to the other buffer
  int held = 0;                                             // pairs the reference's memory would hold
  QnCtl h;
  memset(&h, 0, sizeof(h));
  auto fetch = [&]() -> int { return read_back(&h, ws.ctl, sizeof(QnCtl), st); };
  auto ring_view = [&](int fresh) -> RingView {
    return RingView{ws.S, ws.Y, ws.stride, ring.head(), ring.count(), ring.slots(), fresh};
  };
  // resid, g, v, f of the z in its buffer -- and (pair) the candidate pair against z_prev / g_prev in the ring's next slot
  auto evaluate = [&](bool pair) -> int {
    const float* const Z = ws.Zb[zb.cur()];
    if (glm) {
      LinkEpi<true> el = {};
      el.X = x; el.ldx = ldx; el.Out = ws.R; el.part = ws.part_r;
      LASSO_HIP_TRY(solver::launch_gemm(Z, k, w, ldw, n, d, k, el, side_d, 1, st));
    } else {
      Epi er = {};
      er.X = x; er.ldx = ldx; er.Out = ws.R; er.part = ws.part_r;
      LASSO_HIP_TRY(launch_gemm<EPI_RESID>(Z, k, w, ldw, n, d, k, er, side_d, 1, st));
    }
    GradEpi eg = {};
    eg.Z = Z; eg.V = ws.V; eg.part = ws.part_g; eg.alpha = (float)alpha; eg.pair = pair ? 1 : 0;
    // g goes where g_prev is not; without a pair it IS the first g_prev
    eg.G = ws.Gb[pair ? 1 - gprev : gprev];
    if (pair) {
      eg.Zp = ws.Zb[zb.prev()];
      eg.Gp = ws.Gb[gprev];
      eg.S = ws.S + (int64_t)ring.candidate() * ws.stride;
      eg.Y = ws.Y + (int64_t)ring.candidate() * ws.stride;
    }
    LASSO_HIP_TRY(solver::launch_gemm(ws.R, d, ws.Wt, d, n, k, d, eg, side_k, 1, st));
    hipLaunchKernelGGL(eval_kernel, dim3(1), dim3(256), 0, st, ws.part_r, pd, ws.part_g, pk, scale, alpha, ws.ctl);
    LASSO_HIP_TRY(hipGetLastError());
    return fetch();
  };
  DirectionTimer timer((o.reserved & 2) != 0);
  // d = project(H v, v): pass A, the coefficients, pass B
  auto direction = [&](int fresh) -> int {
    const RingView rv = ring_view(fresh);
    // pass A reads v and every held pair (a fresh one twice), pass B reads the same and writes d
    if (timer.on) res->direction_bytes += (double)nk * 4.0 * (4.0 * rv.count + (rv.count && fresh >= 0 ? 2.0 : 0.0) + 3.0);
    timer.begin(st);
    if (rv.count > 0) {
      if (fresh >= 0)
        hipLaunchKernelGGL(dots_kernel<true>, dim3(ws.nseg), dim3(256), 0, st, ws.V, rv, nk, ws.dots);
      else
        hipLaunchKernelGGL(dots_kernel<false>, dim3(ws.nseg), dim3(256), 0, st, ws.V, rv, nk, ws.dots);
      LASSO_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(coef_kernel, dim3(1), dim3(kCoefThreads), coef_lds, st, ws.dots, ws.nseg, rv, ws.SY, ws.YY, coef);
    LASSO_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(combine_kernel, dim3(gb), dim3(256), 0, st, ws.V, rv, coef.gamma, coef.c, coef.e, nk, ws.D);
    LASSO_HIP_TRY(hipGetLastError());
    timer.end(st);
    return LASSO_OK;
  };
  // candidates z_t of `count` step sizes, and (product) their objectives / verdicts; without a product the one candidate
  // is accepted.  The accepted candidate goes to the buffer that is not z_prev.
  auto trial = [&](const Steps& steps, int count, bool product, bool backtrack) -> int {
    hipLaunchKernelGGL(trial_kernel, dim3(gk, count), dim3(256), 0, st, ws.Zb[zb.cur()], ws.V, ws.D, ws.Zc, nk, steps, ws.part_t);
    LASSO_HIP_TRY(hipGetLastError());
    if (product && glm) {
      LinkEpi<false> et = {};
      et.X = x; et.ldx = ldx; et.a_stride = nk; et.part = ws.part_r;
      LASSO_HIP_TRY(solver::launch_gemm(ws.Zc, k, w, ldw, n, d, k, et, side_d, count, st));
    } else if (product) {
      Epi et = {};
      et.X = x; et.ldx = ldx; et.a_stride = nk; et.part = ws.part_r;
      LASSO_HIP_TRY(launch_gemm<EPI_TRIAL>(ws.Zc, k, w, ldw, n, d, k, et, side_d, count, st));
    }
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(256), 0, st, ws.part_t, gk, ws.part_r, pd, count, product ? 1 : 0,
                       backtrack ? 1 : 0, scale, alpha, (float)o.ls_tol, &ws.ctl->c);
    LASSO_HIP_TRY(hipGetLastError());
    if (!product || backtrack) {
      hipLaunchKernelGGL(accept_kernel, dim3(gk), dim3(256), 0, st, ws.Zc, ws.Zb[zb.target()], nk, &ws.ctl->c);
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

  hipLaunchKernelGGL(init_packed_kernel<>, dim3(gk), dim3(256), 0, st, z0, ldz0, ws.Zb[0], n, k);
  LASSO_HIP_TRY(hipGetLastError());
  if (int s = evaluate(false)) return s;
  res->f0 = res->f_final = h.c.f;
  bool stop = false;
  if (!isfinite(h.c.f)) {
    res->flags |= LASSO_OWN_NONFINITE;
    stop = true;
  }
  // t = clamp(lr / |pg|_1, max=lr), a float32 in the reference (owlqn.py:133): the first iteration's steps are float32
  const float lr32 = (float)o.lr;
  double t_next = (double)fminf(lr32 / (float)h.pgl1, lr32);
  bool t_is_f32 = true;
  double h_diag = 1.0;
  int fresh = -1, n_iter = 0;
  while (!stop && n_iter < o.maxiter) {
    if (int s = direction(fresh)) return s;
    fresh = -1;
    double t = t_next;
    int ls_iters = 0;
    bool applied = false;
    Steps steps = {};
    if (o.line_search == 0) {                               // bounded Brent on t -> f(project(z + t d, eta))
      BoundedMin search(0.0, 10.0, 1e-5, 500);
      while (!search.finished()) {
        const double tt = search.next();
        steps.t[0] = (float)tt;
        if (int s = trial(steps, 1, true, false)) return s;
        note_eval(n_iter + 1, tt, h.c.ft[0]);
        if (!isfinite(h.c.ft[0])) { stop = true; break; }
        search.tell(h.c.ft[0]);
      }
      t = search.best_x();
      ls_iters = search.evaluations();
    } else if (o.line_search == 1) {                        // t, t decay, ...: kRungs per host read
      bool accepted = false;
      for (int first = 0; first < o.ls_maxiter && !accepted && !stop; ) {
        const int count = std::min(kRungs, o.ls_maxiter - first);
        double tv[kRungs];
        for (int j = 0; j < count; ++j) {
          tv[j] = t;
          steps.t[j] = (float)t;
          // the reference's t = t * decay: on a float32 tensor in the first iteration, on a Python float afterwards
          t = t_is_f32 ? (double)((float)t * (float)o.ls_decay) : t * o.ls_decay;
        }
        if (int s = trial(steps, count, true, true)) return s;
        const int seen = h.c.accept >= 0 ? h.c.accept + 1 : count;
        for (int j = 0; j < seen; ++j) note_eval(n_iter + 1, tv[j], h.c.ft[j]);
        if (h.c.accept >= 0) {
          accepted = true;
          t = tv[h.c.accept];
          ls_iters = first + h.c.accept + 1;
        } else if (h.c.bad) {
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
    zb.stepped();
    if (int s = evaluate(true)) return s;                   // (reads dz2 of the accepted step and the pair's verdict with f)
    res->direction_ms += timer.collect();
    ++n_iter;
    const double delta = sqrt(h.c.dz2);
    res->f_final = h.c.f;
    const bool nonfinite = !isfinite(h.c.f);
    const bool converged = !nonfinite && (float)delta <= (float)o.xtol;      // the reference compares float32 values
    // L_BFGS.update (owlqn.py:34-51) -- not after the iteration that stops (:188-192)
    bool skipped = false;
    if (!nonfinite && !converged) {
      const bool keep = h.keep != 0;
      skipped = !keep;
      const int taken = ring.update(keep);
      if (taken >= 0) fresh = taken;
      zb.update(keep);
      if (keep) {
        gprev = 1 - gprev;                                  // g went where g_prev was not: now it is g_prev
        held = std::min(held + 1, (int)o.history_size);
        h_diag = h.ys / h.yy;
      }
    }
    if (tr && n_iter <= tr->capacity) {
      tr->t[n_iter - 1] = t;
      tr->ls_iters[n_iter - 1] = ls_iters;
      tr->f[n_iter - 1] = h.c.f;
      tr->delta_x[n_iter - 1] = delta;
      tr->pairs[n_iter - 1] = held;
      tr->skipped[n_iter - 1] = skipped ? 1 : 0;
      tr->h_diag[n_iter - 1] = h_diag;
    }
    if (nonfinite) {
      res->flags |= LASSO_OWN_NONFINITE;
      break;
    }
    if (converged) break;
    t_next = o.lr;
    t_is_f32 = false;
  }
  res->n_iter = n_iter;
  hipLaunchKernelGGL(copy_out_kernel<>, dim3(gk), dim3(256), 0, st, ws.Zb[zb.cur()], zout, ldz, n, k, 0);
  LASSO_HIP_TRY(hipGetLastError());
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return LASSO_OK;
}

}  // namespace owlqn
}  // namespace lasso
