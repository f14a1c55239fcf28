// csrc/lanczos_host.hpp against closed forms: the largest eigenvalue of a symmetric tridiagonal matrix, the last
// component of its eigenvector, the stop rule of a prefix and the chunk sizer.  Host compiler only;
// tests/test_conv_lip_cpu.py builds and runs it, a second time under -fsanitize=address,undefined.  Prints one line per
// check that fails and "ok N" at the end; exit status 1 on a failure.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "lanczos_host.hpp"

using namespace lasso::lanczos;

static int failures = 0, checks = 0;

#define CHECK(cond)                                              \
  do {                                                           \
    ++checks;                                                    \
    if (!(cond)) {                                               \
      ++failures;                                                \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
    }                                                            \
  } while (0)

static bool close(double a, double b, double rel) { return fabs(a - b) <= rel * fmax(fabs(a), fabs(b)) || a == b; }

// |T z - theta z| and |z| - 1 of a returned eigenvector
static double eig_residual(const std::vector<double>& a, const std::vector<double>& b, const std::vector<double>& z, double theta) {
  const int n = (int)a.size();
  double worst = 0.0;
  for (int k = 0; k < n; ++k) {
    double t = a[k] * z[k] - theta * z[k];
    if (k > 0) t += b[k - 1] * z[k - 1];
    if (k + 1 < n) t += b[k] * z[k + 1];
    worst = fmax(worst, fabs(t));
  }
  return worst;
}

int main() {
  const double pi = 3.14159265358979323846;
  // 1 x 1: theta is the entry, the vector is (1)
  {
    const double a[1] = {2.75}, b[1] = {0.5};
    double z[1] = {0.0};
    const Ritz r = top_ritz(a, b, 1, z);
    CHECK(r.theta == 2.75);
    CHECK(r.last == 1.0 && z[0] == 1.0);
    const double an[1] = {-3.0};
    CHECK(top_ritz(an, b, 1).theta == -3.0);
    const double az[1] = {0.0};
    CHECK(top_ritz(az, b, 1).theta == 0.0);
  }
  // diagonal T: every beta is 0; theta = max alpha exactly, the vector is the unit vector of its position
  {
    const std::vector<double> a = {1.0, 4.0, 2.5, 3.0}, b = {0.0, 0.0, 0.0, 0.0};
    std::vector<double> z(4, -1.0);
    const Ritz r = top_ritz(a.data(), b.data(), 4, z.data());
    CHECK(r.theta == 4.0);
    CHECK(r.last == 0.0);
    CHECK(z[0] == 0.0 && fabs(z[1]) == 1.0 && z[2] == 0.0 && z[3] == 0.0);
    const std::vector<double> a2 = {1.0, 2.0, 7.0};
    const Ritz r2 = top_ritz(a2.data(), b.data(), 3);
    CHECK(r2.theta == 7.0 && r2.last == 1.0);
    // prefixes of one array: T_2 of a2 is diag(1, 2)
    const Ritz r3 = top_ritz(a2.data(), b.data(), 2);
    CHECK(r3.theta == 2.0 && r3.last == 1.0);
  }
  // the 1-D Laplacian tridiag(-1, 2, -1): eigenvalues 2 - 2 cos(k pi / (n + 1)), the top vector's last component is
  // sqrt(2 / (n + 1)) sin(n pi / (n + 1)) in magnitude
  for (int n : {2, 3, 10, 64, 257, 512}) {
    const std::vector<double> a(n, 2.0), b(n, -1.0);
    std::vector<double> z(n, 0.0);
    const Ritz r = top_ritz(a.data(), b.data(), n, z.data());
    const double want = 2.0 - 2.0 * cos(n * pi / (n + 1));
    CHECK(close(r.theta, want, 1e-14));
    CHECK(r.theta >= want * (1.0 - 1e-15));
    const double last = sqrt(2.0 / (n + 1)) * sin(n * pi / (n + 1));
    CHECK(close(r.last, fabs(last), 1e-9));
    CHECK(eig_residual(a, b, z, r.theta) <= 1e-13 * n);
    double nrm = 0.0;
    for (double v : z) nrm += v * v;
    CHECK(fabs(nrm - 1.0) <= 1e-13);
    // the same matrix with positive couplings has the same spectrum
    const std::vector<double> bp(n, 1.0);
    CHECK(close(top_ritz(a.data(), bp.data(), n).theta, want, 1e-14));
  }
  // a shifted and scaled Laplacian: theta scales with it
  {
    const int n = 40;
    const std::vector<double> a(n, 3.0e-7 * 2.0 + 5.0e-7), b(n, 3.0e-7);
    const Ritz r = top_ritz(a.data(), b.data(), n);
    CHECK(close(r.theta, 5.0e-7 + 3.0e-7 * (2.0 + 2.0 * cos(pi / (n + 1))), 1e-14));
  }
  // a decayed last component: a converged Lanczos run looks like this (strong top entry, weak couplings)
  {
    const int n = 30;
    std::vector<double> a(n, 1.0), b(n, 1e-3), z(n, 0.0);
    a[0] = 10.0;
    const Ritz r = top_ritz(a.data(), b.data(), n, z.data());
    CHECK(r.theta > 10.0 && r.theta < 10.0 + 1e-6);
    CHECK(r.last < 1e-80 && r.last >= 0.0);          // about (1e-3 / 9)^29: far below what a three-term recurrence keeps
    CHECK(eig_residual(a, b, z, r.theta) <= 1e-14);
  }
  // clustered top eigenvalues: two blocks coupled by 1e-9, both with the top value 3 -> theta within the coupling of 3
  {
    const std::vector<double> a = {2.0, 2.0, 2.0, 2.0}, b = {1.0, 1e-9, 1.0, 0.0};
    std::vector<double> z(4, 0.0);
    const Ritz r = top_ritz(a.data(), b.data(), 4, z.data());
    CHECK(fabs(r.theta - 3.0) <= 2e-9 && r.theta >= 3.0);
    CHECK(r.last >= 0.0 && r.last <= 1.0);
    CHECK(eig_residual(a, b, z, r.theta) <= 1e-12);
    // an exactly repeated top value (the coupling is 0)
    const std::vector<double> b0 = {1.0, 0.0, 1.0, 0.0};
    const Ritz r0 = top_ritz(a.data(), b0.data(), 4, z.data());
    CHECK(close(r0.theta, 3.0, 1e-15));
    CHECK(isfinite(r0.last) && r0.last >= 0.0 && r0.last <= 1.0);
    CHECK(eig_residual(a, b0, z, r0.theta) <= 1e-14);
  }
  // a NaN or Inf entry: NaN comes back, and the bisection ends
  {
    std::vector<double> a = {1.0, NAN, 2.0}, b = {0.5, 0.5, 0.5};
    CHECK(isnan(top_ritz(a.data(), b.data(), 3).theta));
    CHECK(isnan(top_ritz(a.data(), b.data(), 3).last));
    CHECK(top_ritz(a.data(), b.data(), 1).theta == 1.0);           // the prefix in front of it is untouched
    a[1] = 1.0;
    b[0] = NAN;
    CHECK(isnan(top_ritz(a.data(), b.data(), 3).theta));
    b[0] = INFINITY;
    CHECK(isnan(top_ritz(a.data(), b.data(), 2).theta));
    b[0] = 0.5;
    b[2] = NAN;                                                     // the coupling behind T_3 is not part of T_3
    CHECK(isfinite(top_ritz(a.data(), b.data(), 3).theta));
    CHECK(judge(a.data(), b.data(), 3, 1e-5, 1e-7, 100).status == kNonFinite);
    CHECK(isnan(top_ritz(a.data(), b.data(), 0).theta));
  }
  // the stop rule
  {
    const double eps = 1.1920928955078125e-07;
    const double a1[1] = {1.0}, b1[1] = {0.0};
    Verdict v = judge(a1, b1, 1, 1e-5, eps, 9);                     // the identity: beta = 0 at the first step
    CHECK(v.status == kBreakdown && v.theta == 1.0 && v.residual == 0.0);
    const double a0[1] = {0.0};
    v = judge(a0, b1, 1, 1e-5, eps, 9);                             // the zero operator
    CHECK(v.status == kBreakdown && v.theta == 0.0);
    const double b2[1] = {0.25};
    v = judge(a1, b2, 1, 1e-5, eps, 9);
    CHECK(v.status == kRunning && v.theta == 1.0 && v.residual == 0.25);
    v = judge(a1, b2, 1, 0.25, eps, 9);                             // residual <= tol theta, with equality
    CHECK(v.status == kConverged);
    v = judge(a1, b2, 1, 0.0, eps, 9);                              // tol = 0 never converges ...
    CHECK(v.status == kRunning);
    v = judge(a1, b2, 1, 0.0, eps, 1);                              // ... but the basis may span the space
    CHECK(v.status == kBreakdown);
    const double b3[1] = {eps};                                     // beta <= eps theta, with equality
    CHECK(judge(a1, b3, 1, 0.0, eps, 9).status == kBreakdown);
    const double b4[1] = {1.5 * eps};
    CHECK(judge(a1, b4, 1, 0.0, eps, 9).status == kRunning);
    // a decayed last component converges although beta is large
    std::vector<double> a(30, 1.0), b(30, 1e-3);
    a[0] = 10.0;
    CHECK(judge(a.data(), b.data(), 30, 1e-10, eps, 1000).status == kConverged);
    CHECK(judge(a.data(), b.data(), 2, 1e-10, eps, 1000).status == kRunning);
    const double an[2] = {1.0, NAN};
    CHECK(judge(an, b.data(), 2, 1e-5, eps, 9).status == kNonFinite);
    CHECK(judge(an, b.data(), 1, 1e-5, eps, 9).status == kRunning);
  }
  // the chunk sizer: 8, 16, 32, 32, ... cut at what is left, never 0
  CHECK(next_chunk(0, 512) == 8);
  CHECK(next_chunk(8, 504) == 16);
  CHECK(next_chunk(16, 488) == 32);
  CHECK(next_chunk(32, 456) == 32);
  CHECK(next_chunk(0, 5) == 5);
  CHECK(next_chunk(8, 5) == 5);
  CHECK(next_chunk(32, 1) == 1);
  CHECK(next_chunk(0, 0) == 1);
  if (failures) {
    printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  printf("ok %d\n", checks);
  return 0;
}
