// The exit arithmetic of conjugate gradients (the reference's lasso/conjgrad.py:13-57): the formula for termcond and the
// mapping from the three batch-wide sums of an iteration to a status.  HIP-free: tests/c_host/conjgrad_host_main.cpp
// builds it with the host compiler alone.  The one-workgroup kernels of conjgrad.hip that judge the exits on the device
// call these very functions (LASSO_CG_HD is __host__ __device__ under hipcc and nothing elsewhere): one text, no twin to
// keep in step.  Built with -ffp-contract=off; T = float or double is the tensors' dtype, and every expression is the
// sequence of IEEE operations of that dtype that the reference's tensors go through.  The sums arrive folded in double
// (solver_common.hpp's fixed-order folds) and are rounded ONCE to T before anything is compared.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LASSO_CG_HD __host__ __device__ inline
#else
#define LASSO_CG_HD inline
#endif

namespace lasso {
namespace cg {

// conjgrad.py:4-10, the keys of _status_messages
enum { kAbsTol = 0, kRelTol = 1, kCurvConverged = 2, kCurvNegative = 3, kMaxiter = 4, kRunning = -1 };

template <class T> struct Eps;
template <> struct Eps<float> { static constexpr float value = 1.1920928955078125e-07f; };       // 2^-23
template <> struct Eps<double> { static constexpr double value = 2.220446049250313e-16; };       // 2^-52

LASSO_CG_HD float root(float v) { return sqrtf(v); }
LASSO_CG_HD double root(double v) { return sqrt(v); }

// :18  termcond = rtol * b_abs * b_abs.sqrt().clamp(0, 0.5); the Python scalar rtol enters as a T, clamp keeps a NaN
template <class T>
LASSO_CG_HD T termcond(double rtol, double b_abs_sum) {
  const T b_abs = (T)b_abs_sum;
  T c = root(b_abs);
  if (c < T(0)) c = T(0);
  if (c > T(0.5)) c = T(0.5);
  return ((T)rtol * b_abs) * c;
}

// :34  exit 1, tested before the product
template <class T>
LASSO_CG_HD int exit_before_product(double r_abs_sum, T termcond_) {
  return (T)r_abs_sum <= termcond_ ? (int)kRelTol : (int)kRunning;
}

// :39-45  exits 2 and 3, tested behind the product and before x moves.  A NaN sum takes neither.
template <class T>
LASSO_CG_HD int exit_after_product(double curv_sum) {
  const T c = (T)curv_sum;
  if (T(0) <= c && c <= T(3) * Eps<T>::value) return kCurvConverged;
  if (c < T(0)) return kCurvNegative;
  return kRunning;
}

// :50  exit 0, tested after x and r moved and before p does; the Python scalar tol enters as a T.  *rs = the sqrt.
template <class T>
LASSO_CG_HD int exit_after_step(double rs_sum, double tol, T* rs) {
  *rs = root((T)rs_sum);
  return *rs < (T)tol ? (int)kAbsTol : (int)kRunning;
}

// Iterations of the next chunk between two host reads of the control record, `done` of them behind us.  Only speed
// depends on it: a launch behind a set stop flag does nothing, so a stop inside a chunk costs the rest's empty
// launches and never a replay.  never = true (rtol = 0 and tol = 0: no exit can fire except on an exact zero): the
// whole rest in one chunk.  Otherwise 4, 8, 16 ... up to cap, the reference's runs being 2 to 20 iterations long.
inline int next_chunk(int done, int maxiter, int prev, bool never, int cap) {
  const int left = maxiter - done;
  int c = never ? left : (prev <= 0 ? 4 : 2 * prev);
  if (c > cap) c = cap;
  if (c > left) c = left;
  return c < 1 ? 1 : c;
}

}  // namespace cg
}  // namespace lasso
