// Stand-alone driver of csrc/stoprule_host.hpp for tests/test_stoprule_host_cpu.py (host compiler only, no HIP).
// Reads commands from stdin, prints integers and bit patterns:
//   budget <rows> <k> <tol>                                -> "budget <f32 bits> <f64 bits>"
//   tile <budget> <c> <c sums>                             -> "tile <next chunk>"          (next_tile_chunk, chunk_max 64)
//   chunk <f|d> <first> <last> <budget> <c> <it>           -> "chunk <next chunk>"         (next_stop_chunk, chunk_max 64)
//   first <f|d> <budget> <c> <c sums>                      -> "first <index or -1>"        (first_stop)
//   spec <f|d> <maxiter> <budget> <count> <count sums>     -> the event log of speculate_stop_rule, then "spec <it> <last bits>"
//   words <w0> <w1> <w2> <w3>                              -> "words <iterations> <last delta bits> <redo> <warned>"
// `spec` scripts a solve: iteration i (from 0) has the sum sums[i]; the state of the solve is the number of the next
// iteration, which `save` / `restore` checkpoint like the real solvers checkpoint z and y.
// Numbers are read with strtod (hexadecimal floats are exact; "nan", "inf" and "-inf" are what they say).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "linesearch_host.hpp"
#include "stoprule_host.hpp"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static void print_bits(float v) { printf("%08" PRIx32, bits(v)); }
static void print_bits(double v) { printf("%016" PRIx64, bits(v)); }

static bool number(double* v) {
  char tok[64];
  if (scanf("%63s", tok) != 1) return false;
  *v = strtod(tok, nullptr);
  return true;
}

template <class T>
static int chunk_cmd() {
  double first, last, budget, c, it;
  if (!number(&first) || !number(&last) || !number(&budget) || !number(&c) || !number(&it)) return 2;
  printf("chunk %d\n", lasso::next_stop_chunk<T>((T)first, (T)last, (T)budget, (int)c, (int)it, 64));
  return 0;
}

template <class T>
static int first_cmd() {
  double budget, c;
  if (!number(&budget) || !number(&c) || c < 1 || c > 64) return 2;
  T sums[64];
  for (int i = 0; i < (int)c; ++i) {
    double v;
    if (!number(&v)) return 2;
    sums[i] = (T)v;
  }
  printf("first %d\n", lasso::first_stop<T>(sums, (int)c, (T)budget));
  return 0;
}

template <class T>
static int spec_cmd() {
  double maxiter, budget, count;
  if (!number(&maxiter) || !number(&budget) || !number(&count)) return 2;
  std::vector<T> sums((size_t)count);
  for (T& s : sums) {
    double v;
    if (!number(&v)) return 2;
    s = (T)v;
  }
  T slots[64];                       // stands for the device's 64 sums
  for (T& s : slots) s = (T)-1;
  size_t pos = 0, saved = 0;         // the solve's state and its checkpoint
  lasso::MomentumT<T> mom;
  auto iterate = [&](T* slot) -> int {
    if (pos >= sums.size()) return 4;                      // the script ran dry: the loop iterated past maxiter
    printf("iterate %d %zu ", slot ? (int)(slot - slots) : -1, pos);
    print_bits(mom.t);
    printf("\n");
    mom.next(true);
    if (slot) *slot = sums[pos];
    ++pos;
    return 0;
  };
  auto save = [&]() -> int { saved = pos; printf("save\n"); return 0; };
  auto restore = [&]() -> int { pos = saved; printf("restore\n"); return 0; };
  auto flush = [&]() -> int { printf("flush\n"); return 0; };
  auto read = [&](T* host, int c) -> int {
    printf("read %d\n", c);
    memcpy(host, slots, sizeof(T) * (size_t)c);
    return 0;
  };
  int it = -1;
  T last = (T)0;
  const int s = lasso::speculate_stop_rule<T>((int)maxiter, (T)budget, slots, &mom.t, iterate, save, restore, flush, read,
                                              &it, &last, "stoprule_host_main");
  if (s) return s;
  printf("spec %d ", it);
  print_bits(last);
  printf(" %zu ", pos);              // where the state ended: the iteration after the one the solve stopped in
  print_bits(mom.t);
  printf("\n");
  return 0;
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "budget")) {
      double rows, k, tol;
      if (!number(&rows) || !number(&k) || !number(&tol)) return 2;
      printf("budget %08" PRIx32 " %016" PRIx64 "\n", bits(lasso::stop_budget<float>((int64_t)rows, (int64_t)k, tol)),
             bits(lasso::stop_budget<double>((int64_t)rows, (int64_t)k, tol)));
    } else if (!strcmp(cmd, "tile")) {
      double budget, c;
      if (!number(&budget) || !number(&c) || c < 1 || c > 64) return 2;
      float sums[64];
      for (int i = 0; i < (int)c; ++i) {
        double v;
        if (!number(&v)) return 2;
        sums[i] = (float)v;
      }
      printf("tile %d\n", lasso::next_tile_chunk(sums, (int)c, (float)budget, 64));
    } else if (!strcmp(cmd, "chunk") || !strcmp(cmd, "spec") || !strcmp(cmd, "first")) {
      char type[8];
      if (scanf("%7s", type) != 1) return 2;
      const bool f = type[0] == 'f';
      const int s = !strcmp(cmd, "chunk") ? (f ? chunk_cmd<float>() : chunk_cmd<double>())
                    : !strcmp(cmd, "first") ? (f ? first_cmd<float>() : first_cmd<double>())
                                            : (f ? spec_cmd<float>() : spec_cmd<double>());
      if (s) return s;
    } else if (!strcmp(cmd, "words")) {
      lasso::StopWords words;
      for (int32_t& w : words.w) {
        double v;
        if (!number(&v)) return 2;
        w = (int32_t)(int64_t)v;
      }
      printf("words %d %08" PRIx32 " %d %d\n", words.iterations(), bits(words.last_delta()), words.redo() ? 1 : 0,
             words.warned() ? 1 : 0);
    } else {
      return 3;
    }
  }
  return 0;
}
