// Host-side arithmetic of the line-search drivers (lasso_hip.hip, gemm_f64.hip): FISTA's momentum recurrence, the step
// ladder of a search and the F <= Q verdict of a trial.  Host only, HIP-free (tests/test_linesearch_host_cpu.py builds it
// alone).  Built with -ffp-contract=off: every expression is the sequence of IEEE operations it spells, in ista.py's order.
#pragma once
#include <cmath>
#include <cstdint>

namespace lasso {

constexpr int kBtMultiMax = 8;      // several trials of one outer iteration in one launch: their steps, by value
struct BtSteps { float lr[kBtMultiMax]; float lam[kBtMultiMax]; float hol[kBtMultiMax]; };   // step, alpha * step, 0.5 / step

// ista.py:78,98-100: t_0 = 1 (python int 1; same arithmetic in double), t_{i+1} = (1 + sqrt(1 + 4 t_i^2)) / 2,
// coef_i = (t_i - 1) / t_{i+1}, 0 without momentum (ISTA: y == z).  Coef = float: the python float cast to the tensor
// dtype (Momentum); Coef = double: float64 tensors (Momentum64).
template <class Coef>
struct MomentumT {
  double t = 1.0;
  Coef next(bool fast) {       // the coefficient of this iteration; t moves on to the next
    const double t0 = t;
    skip(1);                                                                        // :98
    return fast ? (Coef)((t0 - 1.0) / t) : (Coef)0;                                 // :99
  }
  void skip(int m) {           // m iterations further, no coefficients (a window that ran on the device; lasso_fista_run's it0)
    for (int i = 0; i < m; ++i) t = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
  }
};
using Momentum = MomentumT<float>;
using Momentum64 = MomentumT<double>;

// The steps of one search: lr0, lr0 / eta, (lr0 / eta) / eta, ... (ista.py:47), in double; a trial takes the step, the
// shrinkage threshold alpha * step (product in double, :90) and 0.5 / step as floats.
struct StepLadder {
  double lr, eta, alpha;
  void descend() { lr = lr / eta; }                                                 // :47
  void fill(BtSteps& s, int nb) {      // the next nb rungs into s[0 .. nb); the ladder is left behind them
    for (int b = 0; b < nb; ++b, descend()) { s.lr[b] = (float)lr; s.lam[b] = (float)(alpha * lr); s.hol[b] = (float)(0.5 / lr); }
  }
};

// The decision of one trial (ista.py:23,28,32-35,45) from its five sums {sum r0^2, sum r1^2, sum |z1|, sum dz g, sum dz^2}.
// T = float rounds the sums and alpha to float first and decides in float, as the device does; T = double is the float64
// solver.  Device twins that must stay in step, operation for operation: bt_decide_kernel (backtrack.hip) and
// bt_iter_decide_kernel (bt_iter.hip), which spell the same order with __f*_rn.
template <class T>
struct LineSearchVerdict { T F, Q; bool accepted; };
template <class T>
inline LineSearchVerdict<T> line_search_verdict(const double* sums, double alpha, double lr_t, bool force) {
  const T rss0 = (T)sums[0], rss1 = (T)sums[1], l1 = (T)sums[2], dzg = (T)sums[3], dz2 = (T)sums[4];
  const T f0 = (T)0.5 * rss0, al1 = (T)alpha * l1;                                  // :23
  const T F = (T)0.5 * rss1 + al1;                                                  // :28
  const T Q = ((f0 + dzg) + (T)(0.5 / lr_t) * dz2) + al1;                           // :32-35
  return {F, Q, force || F <= Q};                                                   // :45
}

}  // namespace lasso
