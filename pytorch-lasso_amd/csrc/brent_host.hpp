// Bounded scalar minimisation on the host: the golden-section / successive-parabola method of Forsythe, Malcolm and
// Moler's fmin (Computer Methods for Mathematical Computations, 1977, ch. 8; Brent 1973, ch. 5), with the constants of
// scipy.optimize.minimize_scalar(method='bounded') -- eps = sqrt(2.2e-16), tolerance |x| eps + xatol / 3 -- so that a
// caller who evaluates the same function sees the same abscissae.  A RESUMABLE state machine: the objective lives on the
// GPU, so the driver (own.hip) asks next() for an abscissa, evaluates there, and hands the value to tell().
//
//   BoundedMin m(0.0, 10.0);
//   while (!m.finished()) m.tell(f(m.next()));
//   m.best_x(), m.best_f(), m.evaluations()
//
// Host compiler only, IEEE doubles, + - * / sqrt and comparisons (build with -ffp-contract=off: a fused multiply-add
// moves the abscissae).  tests/test_brent_host_cpu.py compares every abscissa with scipy bit for bit.
#pragma once
#include <math.h>

namespace lasso {

class BoundedMin {
 public:
  BoundedMin(double lo, double hi, double xatol = 1e-5, int maxiter = 500)
      : lo_(lo), hi_(hi), xatol_(xatol), maxiter_(maxiter) {
    ratio_ = 0.5 * (3.0 - sqrt(5.0));
    eps_ = sqrt(2.2e-16);
    best_ = second_ = third_ = lo_ + ratio_ * (hi_ - lo_);
    probe_ = best_;
  }

  bool finished() const { return done_; }
  double next() const { return probe_; }         // the abscissa whose value tell() expects
  double best_x() const { return best_; }
  double best_f() const { return f_best_; }
  int evaluations() const { return count_; }
  bool hit_maxiter() const { return capped_; }

  void tell(double f) {
    if (done_) return;
    ++count_;
    if (count_ == 1) {
      f_best_ = f_second_ = f_third_ = f;
    } else {
      absorb(probe_, f);
      if (count_ >= maxiter_) {
        refresh();
        capped_ = done_ = true;
        return;
      }
    }
    refresh();
    if (!(fabs(best_ - mid_) > (tol2_ - 0.5 * (hi_ - lo_)))) {
      done_ = true;
      return;
    }
    propose();
  }

 private:
  static double unit(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 1.0); }   // sign(v), with sign(0) = +1

  void refresh() {
    mid_ = 0.5 * (lo_ + hi_);
    tol1_ = eps_ * fabs(best_) + xatol_ / 3.0;
    tol2_ = 2.0 * tol1_;
  }

  // the bracket [lo, hi] and the three best points after the value f at u
  void absorb(double u, double f) {
    if (f <= f_best_) {
      if (u >= best_) lo_ = best_; else hi_ = best_;
      third_ = second_; f_third_ = f_second_;
      second_ = best_; f_second_ = f_best_;
      best_ = u; f_best_ = f;
    } else {
      if (u < best_) lo_ = u; else hi_ = u;
      if (f <= f_second_ || second_ == best_) {
        third_ = second_; f_third_ = f_second_;
        second_ = u; f_second_ = f;
      } else if (f <= f_third_ || third_ == best_ || third_ == second_) {
        third_ = u; f_third_ = f;
      }
    }
  }

  // the next abscissa: the vertex of the parabola through the three best points when it falls inside the bracket and
  // moves less than half the step before last, a golden section of the larger part otherwise
  void propose() {
    bool golden = true;
    if (fabs(prev_) > tol1_) {
      golden = false;
      double r = (best_ - second_) * (f_best_ - f_third_);
      double q = (best_ - third_) * (f_best_ - f_second_);
      double p = (best_ - third_) * q - (best_ - second_) * r;
      q = 2.0 * (q - r);
      if (q > 0.0) p = -p;
      q = fabs(q);
      r = prev_;
      prev_ = step_;
      if (fabs(p) < fabs(0.5 * q * r) && p > q * (lo_ - best_) && p < q * (hi_ - best_)) {
        step_ = (p + 0.0) / q;
        const double u = best_ + step_;
        if ((u - lo_) < tol2_ || (hi_ - u) < tol2_) step_ = tol1_ * unit(mid_ - best_);   // not too close to an end
      } else {
        golden = true;
      }
    }
    if (golden) {
      prev_ = best_ >= mid_ ? lo_ - best_ : hi_ - best_;
      step_ = ratio_ * prev_;
    }
    probe_ = best_ + unit(step_) * fmax(fabs(step_), tol1_);     // never closer than tol1 to the best point
  }

  double lo_, hi_, xatol_;
  int maxiter_;
  double ratio_, eps_;
  double best_, second_, third_;                  // abscissae of the lowest value, the next lowest, the one before
  double f_best_ = 0.0, f_second_ = 0.0, f_third_ = 0.0;
  double step_ = 0.0, prev_ = 0.0;                // the last step and the one before it
  double probe_, mid_ = 0.0, tol1_ = 0.0, tol2_ = 0.0;
  int count_ = 0;
  bool done_ = false, capped_ = false;
};

}  // namespace lasso
