// Drives csrc/lbfgs_ring_host.hpp from a script on stdin (tests/test_lbfgs_ring_host_cpu.py) and lets the ring and the
// two buffers move REAL data, so that a wrong slot shows as a wrong pair and a wrong index shows under the sanitizers:
//
//   ring <history>          a new PairRing, TwoBuffers and fresh storage of history + 1 slots
//   step <value> <keep>     one iteration: x becomes <value> (written to the buffer target() names), the candidate pair
//                           (value - x_prev) goes into the candidate slot, then update(keep)
//
// After every step it prints: the held pairs oldest first (as the values their slots hold), x_prev, the newest slot.
#include <stdio.h>
#include <string.h>
#include <vector>

#include "lbfgs_ring_host.hpp"

int main() {
  char word[16];
  lasso::PairRing* ring = nullptr;
  lasso::TwoBuffers zb;
  std::vector<long> slots;
  long x[2] = {0, 0};
  while (scanf("%15s", word) == 1) {
    if (!strcmp(word, "ring")) {
      int history = 0;
      if (scanf("%d", &history) != 1) return 2;
      delete ring;
      ring = new lasso::PairRing(history);
      zb = lasso::TwoBuffers();
      slots.assign(ring->slots(), -1);
      x[0] = x[1] = 0;
      printf("ring %d slots %d\n", ring->capacity(), ring->slots());
    } else if (!strcmp(word, "step")) {
      long value = 0;
      int keep = 0;
      if (!ring || scanf("%ld %d", &value, &keep) != 2) return 2;
      x[zb.target()] = value;
      zb.stepped();
      if (zb.cur() == zb.prev()) return 3;                       // x must never land on x_prev
      slots.at(ring->candidate()) = x[zb.cur()] - x[zb.prev()];
      const int taken = ring->update(keep != 0);
      zb.update(keep != 0);
      printf("held");
      for (int i = 0; i < ring->count(); ++i) printf(" %ld", slots.at(ring->slot(i)));
      printf(" | prev %ld | newest %d taken %d\n", x[zb.prev()], ring->newest(), taken);
    } else {
      return 2;
    }
  }
  delete ring;
  return 0;
}
