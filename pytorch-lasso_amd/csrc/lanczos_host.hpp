// The tridiagonal arithmetic of the Lanczos iteration behind lasso_conv_lip_constant (conv_lanczos.hip), in double and
// HIP-free: tests/c_host/lanczos_host_main.cpp builds it with the host compiler alone.
//   T_n = tridiag(beta[0..n-2]; alpha[0..n-1]; beta[0..n-2])   (beta[n-1], the coupling to the next vector, is not in T_n)
//   top_ritz   theta = the largest eigenvalue of T_n: bisection on the Sturm count between max alpha (the largest
//              eigenvalue of a symmetric matrix is at least its largest diagonal entry) and the Gershgorin bound, down to
//              neighbouring doubles; theta is the UPPER end of the last bracket, so T_n - theta I has no positive pivot.
//              The eigenvector by the twisted factorisation of T_n - theta I (Parlett & Dhillon 1997): the pivots d_k of
//              the elimination from the top and e_k from the bottom, the twist at the index r where
//              |d_r + e_r - (alpha_r - theta)| is smallest, z_r = 1 and the two two-term recurrences away from r.  Unlike
//              the three-term recurrence from the top it keeps its accuracy where the last component has decayed to
//              nothing, which is exactly where the stop rule reads it.
//   judge      the stop rule of one prefix: residual = beta[n-1] |s_n| (some eigenvalue of a symmetric operator lies
//              within it of theta), breakdown beta[n-1] <= eps theta, convergence residual <= tol theta
//   next_chunk Lanczos steps between two host reads: 8, 16, 32, 32, ...
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace lasso {
namespace lanczos {

enum { kRunning = -1, kConverged = 0, kBreakdown = 1, kMaxiter = 2, kNonFinite = 3 };
constexpr int kMaxBasis = 512;        // most basis vectors of one cycle (the device folds their coefficients in LDS)

struct Ritz {
  double theta;                       // largest eigenvalue of T_n (NaN: a non-finite entry)
  double last;                        // |last component| of its unit eigenvector
};

// number of eigenvalues of T_n below x (negative pivots of T_n - x I); a zero pivot counts as negative, which puts an
// eigenvalue AT x below it: the bisection then ends on the upper side
inline int sturm_below(const double* alpha, const double* beta, int n, double x) {
  int count = 0;
  double d = 1.0;
  for (int k = 0; k < n; ++k) {
    const double b2 = k > 0 ? beta[k - 1] * beta[k - 1] : 0.0;
    d = (alpha[k] - x) - (k > 0 ? b2 / d : 0.0);
    if (d == 0.0) d = -2.2250738585072014e-308;
    if (d < 0.0) ++count;
  }
  return count;
}

// vec (nullable, n doubles): the unit eigenvector itself
inline Ritz top_ritz(const double* alpha, const double* beta, int n, double* vec = nullptr) {
  Ritz out = {NAN, NAN};
  if (n < 1) return out;
  double lo = alpha[0], hi = alpha[0];
  for (int k = 0; k < n; ++k) {
    const double bl = k > 0 ? fabs(beta[k - 1]) : 0.0, br = k + 1 < n ? fabs(beta[k]) : 0.0;
    if (!isfinite(alpha[k]) || !isfinite(bl) || !isfinite(br)) return out;
    lo = fmax(lo, alpha[k]);
    hi = fmax(hi, alpha[k] + bl + br);
  }
  // invariant: sturm_below(hi') == n for every hi' > hi_true >= theta, sturm_below(lo) < n or lo == theta
  if (sturm_below(alpha, beta, n, lo) == n) {
    hi = lo;                          // theta == max alpha (a diagonal T, or the 1 x 1 case)
  } else {
    hi = nextafter(hi, INFINITY);
    for (int it = 0; it < 4096; ++it) {
      const double mid = lo + 0.5 * (hi - lo);
      if (!(mid > lo && mid < hi)) break;
      if (sturm_below(alpha, beta, n, mid) == n) hi = mid; else lo = mid;
    }
  }
  out.theta = hi;
  if (n == 1) {
    out.last = 1.0;
    if (vec) vec[0] = 1.0;
    return out;
  }
  // twisted factorisation: the pivots from the top (d) and from the bottom (e); a zero pivot becomes the smallest
  // negative number (theta is an upper end: no pivot is positive)
  const double tiny = -2.2250738585072014e-308;
  double dbuf[kMaxBasis], ebuf[kMaxBasis];
  if (n > kMaxBasis) return out;      // (last stays NaN: no cycle is longer)
  dbuf[0] = alpha[0] - hi;
  if (dbuf[0] == 0.0) dbuf[0] = tiny;
  for (int k = 1; k < n; ++k) {
    dbuf[k] = (alpha[k] - hi) - beta[k - 1] * beta[k - 1] / dbuf[k - 1];
    if (dbuf[k] == 0.0) dbuf[k] = tiny;
  }
  ebuf[n - 1] = alpha[n - 1] - hi;
  if (ebuf[n - 1] == 0.0) ebuf[n - 1] = tiny;
  for (int k = n - 2; k >= 0; --k) {
    ebuf[k] = (alpha[k] - hi) - beta[k] * beta[k] / ebuf[k + 1];
    if (ebuf[k] == 0.0) ebuf[k] = tiny;
  }
  int r = 0;
  double best = INFINITY;
  for (int k = 0; k < n; ++k) {
    const double gamma = fabs(dbuf[k] + ebuf[k] - (alpha[k] - hi));
    if (gamma < best) { best = gamma; r = k; }
  }
  // z_r = 1; upwards z_k = -beta_k z_{k+1} / d_k, downwards z_{k+1} = -beta_k z_k / e_{k+1}, then the unit vector
  double zlast = 1.0, sum = 1.0;
  double* z = vec;
  if (z) z[r] = 1.0;
  double cur = 1.0;
  for (int k = r - 1; k >= 0; --k) {
    cur = -beta[k] * cur / dbuf[k];
    if (z) z[k] = cur;
    sum += cur * cur;
  }
  cur = 1.0;
  for (int k = r; k + 1 < n; ++k) {
    cur = -beta[k] * cur / ebuf[k + 1];
    if (z) z[k + 1] = cur;
    sum += cur * cur;
  }
  zlast = (r == n - 1) ? 1.0 : cur;
  const double nrm = sqrt(sum);
  out.last = fabs(zlast) / nrm;
  if (z)
    for (int k = 0; k < n; ++k) z[k] /= nrm;
  return out;
}

struct Verdict {
  int status;                         // kRunning, kConverged, kBreakdown or kNonFinite
  double theta, residual;
};

// the stop rule on the prefix T_n with its coupling beta[n-1]; eps: of the dtype the vectors are held in; dim: of the
// space (n == dim: the basis spans it, theta is exact)
inline Verdict judge(const double* alpha, const double* beta, int n, double tol, double eps, int64_t dim, double* vec = nullptr) {
  Verdict v = {kRunning, NAN, NAN};
  if (!isfinite(alpha[n - 1]) || !isfinite(beta[n - 1])) { v.status = kNonFinite; return v; }
  const Ritz r = top_ritz(alpha, beta, n, vec);
  if (!isfinite(r.theta)) { v.status = kNonFinite; return v; }
  v.theta = r.theta;
  v.residual = beta[n - 1] * r.last;
  if (beta[n - 1] <= eps * fabs(r.theta) || (int64_t)n >= dim) v.status = kBreakdown;
  else if (v.residual <= tol * fabs(r.theta)) v.status = kConverged;
  return v;
}

// steps of the next chunk: 8, 16, 32, 32, ... cut at `left`.  Only speed depends on it: a launch behind a set stop flag
// does nothing and the host judges every prefix, so the value returned is that of the first prefix that stops.
inline int next_chunk(int prev, int left) {
  int c = prev <= 0 ? 8 : (prev >= 16 ? 32 : 2 * prev);
  if (c > left) c = left;
  return c < 1 ? 1 : c;
}

}  // namespace lanczos
}  // namespace lasso
