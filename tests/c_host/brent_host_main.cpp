// Drives csrc/brent_host.hpp over a script of functions (stdin) and prints every abscissa it asks for and its result as
// the bit patterns of the doubles; tests/test_brent_host_cpu.py compares them with scipy's bounded minimiser.
// One line per function:  <mode> a b k1 p1 k2 p2 c level   (numbers as C99 hex floats)
//   g(t) = a (t - b)^2 + k1 |t - p1| + k2 |t - p2| + c
//   mode 0: g;  mode 1: g rounded through float on every call;  mode 2: max(g, level) -- a plateau
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#include "brent_host.hpp"

static unsigned long long bits(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return (unsigned long long)u;
}

int main() {
  char line[1024];
  int index = 0;
  while (fgets(line, sizeof line, stdin)) {
    int mode = 0;
    double p[8];
    char* cur = line;
    mode = (int)strtol(cur, &cur, 10);
    for (int i = 0; i < 8; ++i) p[i] = strtod(cur, &cur);
    lasso::BoundedMin search(0.0, 10.0, 1e-5, 500);
    while (!search.finished()) {
      const double t = search.next();
      const double u = t - p[1];
      double f = p[0] * u * u + p[2] * fabs(t - p[3]) + p[4] * fabs(t - p[5]) + p[6];
      if (mode == 1) f = (double)(float)f;
      if (mode == 2) f = fmax(f, p[7]);
      printf("%d x %016llx %016llx\n", index, bits(t), bits(f));
      search.tell(f);
    }
    printf("%d result %016llx %016llx %d\n", index, bits(search.best_x()), bits(search.best_f()), search.evaluations());
    ++index;
  }
  return 0;
}
