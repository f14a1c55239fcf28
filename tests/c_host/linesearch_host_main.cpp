// Stand-alone driver of csrc/linesearch_host.hpp for tests/test_linesearch_host_cpu.py (host compiler only, no HIP).
// Reads commands from stdin, prints bit patterns:
//   coef                                   -> 64 lines "coef <i> <fast f32> <not fast f32> <fast f64>"
//   ladder <lr0> <eta> <alpha>             -> 8 lines "ladder <rung> <lr f32> <lam f32> <hol f32>" + "ladder_lr <lr f64>"
//   verdict <f|d> <5 sums> <alpha> <lr_t> <force> -> "verdict <F> <Q> <accepted>"
// Numbers are read with strtod (hexadecimal floats are exact).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "linesearch_host.hpp"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "coef")) {
      lasso::Momentum fast, slow, skipped;
      lasso::Momentum64 fast64;
      for (int i = 0; i < 64; ++i) {
        // skip(i) from the start must land where i calls of next() did
        lasso::Momentum s;
        s.skip(i);
        if (bits(s.t) != bits(fast.t)) { printf("skip(%d) differs from %d x next()\n", i, i); return 1; }
        printf("coef %d %08" PRIx32 " %08" PRIx32 " %016" PRIx64 "\n", i, bits(fast.next(true)), bits(slow.next(false)),
               bits(fast64.next(true)));
      }
    } else if (!strcmp(cmd, "ladder")) {
      char a[64], b[64], c[64];
      if (scanf("%63s %63s %63s", a, b, c) != 3) return 2;
      lasso::StepLadder ladder{strtod(a, nullptr), strtod(b, nullptr), strtod(c, nullptr)};
      lasso::BtSteps head, rest;           // 5 rungs, then the 3 behind them: the ladder stays positioned
      ladder.fill(head, 5);
      ladder.fill(rest, 3);
      for (int r = 0; r < 8; ++r) {
        const lasso::BtSteps& s = r < 5 ? head : rest;
        const int j = r < 5 ? r : r - 5;
        printf("ladder %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", r, bits(s.lr[j]), bits(s.lam[j]), bits(s.hol[j]));
      }
      printf("ladder_lr %016" PRIx64 "\n", bits(ladder.lr));
    } else if (!strcmp(cmd, "verdict")) {
      char type[8], tok[8][64];
      if (scanf("%7s", type) != 1) return 2;
      for (int i = 0; i < 8; ++i)
        if (scanf("%63s", tok[i]) != 1) return 2;
      double sums[5];
      for (int i = 0; i < 5; ++i) sums[i] = strtod(tok[i], nullptr);
      const double alpha = strtod(tok[5], nullptr), lr_t = strtod(tok[6], nullptr);
      const bool force = atoi(tok[7]) != 0;
      if (type[0] == 'f') {
        const lasso::LineSearchVerdict<float> v = lasso::line_search_verdict<float>(sums, alpha, lr_t, force);
        printf("verdict %08" PRIx32 " %08" PRIx32 " %d\n", bits(v.F), bits(v.Q), v.accepted ? 1 : 0);
      } else {
        const lasso::LineSearchVerdict<double> v = lasso::line_search_verdict<double>(sums, alpha, lr_t, force);
        printf("verdict %016" PRIx64 " %016" PRIx64 " %d\n", bits(v.F), bits(v.Q), v.accepted ? 1 : 0);
      }
    } else {
      return 3;
    }
  }
  return 0;
}
