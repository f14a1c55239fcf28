// csrc/conjgrad_host.hpp against hand-computed cases: termcond, the mapping from the three batch-wide sums to a status,
// and the chunk sizer.  Host compiler only; tests/test_conjgrad_cpu.py builds and runs it, a second time under
// -fsanitize=address,undefined.  Prints one line per check that fails and "ok N" at the end; exit status 1 on a failure.
#include <math.h>
#include <stdio.h>

#include <limits>

#include "conjgrad_host.hpp"

using namespace lasso::cg;

static int failures = 0, checks = 0;

#define CHECK(cond)                                              \
  do {                                                           \
    ++checks;                                                    \
    if (!(cond)) {                                               \
      ++failures;                                                \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
    }                                                            \
  } while (0)

template <class T>
static void dtype_cases() {
  const T eps = std::numeric_limits<T>::epsilon();
  const double nan = NAN, inf = INFINITY;
  CHECK(Eps<T>::value == eps);
  // termcond = rtol * b_abs * min(sqrt(b_abs), 0.5)
  CHECK(termcond<T>(1.0, 4.0) == T(2));                          // sqrt(4) = 2 -> clamped to 0.5
  CHECK(termcond<T>(0.1, 4.0) == (T(0.1) * T(4)) * T(0.5));      // rtol enters as a T, the products left to right
  CHECK(termcond<T>(1.0, 0.0625) == T(0.0625) * T(0.25));        // sqrt(1/16) = 1/4 < 0.5: not clamped
  CHECK(termcond<T>(1.0, 0.25) == T(0.125));                     // sqrt = 0.5 exactly
  CHECK(termcond<T>(0.0, 100.0) == T(0));
  CHECK(termcond<T>(1.0, 0.0) == T(0));
  CHECK(isnan(termcond<T>(1.0, nan)));                           // clamp keeps a NaN
  CHECK(isinf(termcond<T>(1.0, inf)));
  // exit 1: sum|r| <= termcond, both as T
  CHECK(exit_before_product<T>(1.0, T(1)) == kRelTol);
  CHECK(exit_before_product<T>(0.0, T(0)) == kRelTol);           // b = 0
  CHECK(exit_before_product<T>(1.0 + 4.0 * (double)eps, T(1)) == kRunning);
  CHECK(exit_before_product<T>(1.0 + (double)eps / 4.0, T(1)) == kRelTol);       // rounds to 1 in T before the test
  CHECK(exit_before_product<T>(nan, T(1)) == kRunning);
  CHECK(exit_before_product<T>(1.0, (T)nan) == kRunning);
  // exits 2 and 3: 0 <= curv_sum <= 3 eps; curv_sum < 0
  CHECK(exit_after_product<T>(0.0) == kCurvConverged);
  CHECK(exit_after_product<T>(-0.0) == kCurvConverged);
  CHECK(exit_after_product<T>(3.0 * (double)eps) == kCurvConverged);
  CHECK(exit_after_product<T>(3.0 * (double)eps * (1.0 + 4.0 * (double)eps)) == kRunning);
  CHECK(exit_after_product<T>(1.0) == kRunning);
  CHECK(exit_after_product<T>(-1e-30) == kCurvNegative);
  CHECK(exit_after_product<T>(-1.0) == kCurvNegative);
  CHECK(exit_after_product<T>(-inf) == kCurvNegative);
  CHECK(exit_after_product<T>(inf) == kRunning);
  CHECK(exit_after_product<T>(nan) == kRunning);
  // exit 0: sqrt(sum rs) < tol, both as T
  T rs = T(-1);
  CHECK(exit_after_step<T>(4.0, 1.0, &rs) == kRunning && rs == T(2));
  CHECK(exit_after_step<T>(4.0, 2.0, &rs) == kRunning);          // strictly below
  CHECK(exit_after_step<T>(4.0, 2.5, &rs) == kAbsTol && rs == T(2));
  CHECK(exit_after_step<T>(0.0, 0.0, &rs) == kRunning && rs == T(0));            // tol = 0 never fires
  CHECK(exit_after_step<T>(0.0, 1e-10, &rs) == kAbsTol);
  CHECK(exit_after_step<T>(nan, 1.0, &rs) == kRunning && isnan(rs));
  CHECK(exit_after_step<T>(inf, 1.0, &rs) == kRunning);
}

int main() {
  dtype_cases<float>();
  dtype_cases<double>();
  // the Python scalar tol enters as a T: 1e-10 rounded to float is above 1e-10
  float rsf;
  double rsd;
  CHECK((float)1e-10 > 1e-10);
  CHECK(exit_after_step<float>(0.98e-20, 1e-10, &rsf) == kAbsTol && exit_after_step<double>(0.98e-20, 1e-10, &rsd) == kAbsTol);
  CHECK(exit_after_step<float>(1.02e-20, 1e-10, &rsf) == kRunning && exit_after_step<double>(1.02e-20, 1e-10, &rsd) == kRunning);
  CHECK(exit_after_step<double>(1.0000000001e-20, 1e-10, &rsd) == kRunning);
  // chunks: 4, 8, 16 ... cap, never beyond what is left; never = true: the whole rest
  CHECK(next_chunk(0, 100, 0, false, 64) == 4);
  CHECK(next_chunk(4, 100, 4, false, 64) == 8);
  CHECK(next_chunk(60, 1000, 32, false, 64) == 64);
  CHECK(next_chunk(124, 1000, 64, false, 64) == 64);
  CHECK(next_chunk(98, 100, 8, false, 64) == 2);
  CHECK(next_chunk(0, 2, 0, false, 64) == 2);
  CHECK(next_chunk(0, 8, 0, true, 1 << 30) == 8);
  CHECK(next_chunk(0, 5000, 0, true, 1023) == 1023);
  CHECK(next_chunk(0, 100, 0, false, 8) == 4 && next_chunk(12, 100, 8, false, 8) == 8);
  printf("%s %d\n", failures ? "failed" : "ok", checks);
  return failures ? 1 : 0;
}
