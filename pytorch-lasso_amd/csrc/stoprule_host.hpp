// Host-side arithmetic of the stop rule (ista.py:64,93 / conv2d/ista.py:44-46) that the drivers in lasso_hip.hip and
// gemm_f64.hip share: the budget, the first iteration of a chunk that meets it, the two chunk sizers, the
// speculate-and-replay loop of DESIGN 3.2 and the four result words of the kernels that judge the rule themselves.  Host
// only, HIP-free (tests/test_stoprule_host_cpu.py builds it alone).  Built with -ffp-contract=off: every expression is
// the sequence of IEEE operations it spells.  Device twins that must stay in step with first_stop and StopWords:
// chunk_verdict_kernel and reduce_verdict_kernel (lasso_hip.hip), the in-kernel rule of fista_tile_sp_kernel.hpp and
// fista_splitk.hip, and bt16_persist_kernel (bt16_persist.hip).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace lasso {

// ista.py:64: z0.numel() * tol.  T = float: the double product rounded once, compared in fp32 like the reference's
// tensors; T = double: float64 tensors.
template <class T>
inline T stop_budget(int64_t rows, int64_t k, double tol) { return (T)((double)rows * (double)k * tol); }

// ista.py:93 over the sums of a chunk: the index of the first one <= budget, -1 without one.
template <class T>
inline int first_stop(const T* sums, int c, T budget) {
  for (int j = 0; j < c; ++j)
    if (sums[j] <= budget) return j;
  return -1;
}

// Size of the next chunk of speculated iterations of speculate_stop_rule after a chunk of `c` iterations without a
// stop whose first / last sums were `first` / `last`, `it` iterations done.  Only speed depends on it; a stop inside a
// chunk costs one chunk (the speculated rest plus the replay).  Within a factor 2 of the budget: one iteration at a time
// (the reference's own cadence: the sums of a momentum run are not monotone, and an iteration speculated past the stop
// costs more than the wait it saves).  Further away: the iterations the rule is still away at the chunk's average decay
// -- that many when it is near (so that it fires at the chunk's END: nothing to replay), half as many when it is far;
// without a decaying chunk behind us, as many iterations as the solve has done; at most half the iterations done, and
// never fewer than the sums would need if they halved every iteration.
template <class T>
inline int next_stop_chunk(T first, T last, T budget, int c, int it, int chunk_max) {
  int next = 1;
  if (last > T(2) * budget) {
    next = std::min(chunk_max, std::max(2, it));
    if (c > 1 && first > T(0) && last < first && budget > T(0)) {
      const double rate = log((double)first / (double)last) / (double)(c - 1);
      const double away = log((double)last / (double)budget) / rate;
      next = away <= 8.0 ? std::max(1, (int)ceil(away)) : (int)std::min((double)chunk_max, away / 2.0);
    }
    const int lg = budget > T(0) ? (int)std::min((double)chunk_max, log2((double)last / (double)budget)) : chunk_max;
    next = std::max(lg, std::min(next, std::max(2, it / 2)));
  }
  return next;
}

// Size of the next chunk of the fused fp32 solve's chunked form (solve_chunked in lasso_hip.hip; its twin for row shards
// is parallel._next_tile_chunk) -- purely a scheduling heuristic, the stop decision itself stays exact: estimate the
// iterations left until a sum <= budget from the geometric decay over the chunk's `c` sums and approach the predicted
// stop with short chunks so that little work is wasted or replayed.  A chunk that holds a NaN sum predicts no stop
// (NaN <= budget is false, and a NaN code stays NaN): the full chunk.  The maxima keep a NaN for that -- std::max,
// like Python's max(), keeps or drops one depending on where it stands.
inline int next_tile_chunk(const float* sums, int c, float budget, int chunk_max) {
  int next_chunk = chunk_max;
  if (c >= 8 && budget > 0.0f) {
    const int h = c / 2;
    float hi = 0.0f, lo = 0.0f;
    for (int i = 0; i < h; ++i) hi = (sums[i] > hi || sums[i] != sums[i]) ? sums[i] : hi;
    for (int i = h; i < c; ++i) lo = (sums[i] > lo || sums[i] != sums[i]) ? sums[i] : lo;
    if (hi != hi || lo != lo) return chunk_max;
    if (lo > budget && hi > lo) {
      const double rate = log((double)hi / lo) / h;              // per-iteration log decay
      const double left = log((double)lo / budget) / rate;       // iterations still needed
      if (left < 2.0 * chunk_max) {
        const int guess = (int)left - 6;
        next_chunk = guess >= chunk_max ? chunk_max : std::max(8, std::min(guess, chunk_max));
      }
    } else if (lo <= budget * 4.0f) {
      next_chunk = 8;
    }
  }
  return next_chunk;
}

// The stop rule of the multi-launch solvers (the first iteration whose sum |z - z_next| over ALL elements is <= budget
// ends the solve with that iteration's z) without a host round trip per iteration -- the speculate-and-replay scheme of
// DESIGN 3.2 at launch granularity: a chunk of <= 64 iterations is enqueued with every iteration's sum kept on the
// device (`iterate(slot)` leaves it in *slot, a place in `delta_dev`), the host reads the chunk's sums ONCE
// (`read(host, c)`: copy delta_dev[0 .. c) and wait); if iteration j of the chunk met the rule and was not the chunk's
// last, the state goes back to the chunk's head (`save` / `restore`, the momentum scalar *t_mom with it) and exactly
// j + 1 iterations are replayed -- every kernel of these paths sums in a fixed order, so the replay is bitwise the state
// the reference stops in.  `flush` puts iterations that `iterate` only queued on the stream (the convolutional solver's
// many-iterations-per-launch kernel); solvers that launch in `iterate` pass a no-op.  The callables return a
// lasso_status; the first that is not 0 (LASSO_OK) ends the loop.  T = float: the fp32 solvers; T = double: float64.
//   save (only if c > 1), c x iterate(slot), flush, read, verdict, [restore, *t_mom back, (hit + 1) x iterate(nullptr), flush]
template <class T, class Iterate, class Save, class Restore, class Flush, class Read>
int speculate_stop_rule(int maxiter, T budget, T* delta_dev, double* t_mom, Iterate iterate, Save save, Restore restore,
                        Flush flush, Read read, int* it_out, T* last_out, const char* who) {
  constexpr int kChunkMax = 64;                    // delta_dev holds 64 sums
  static const bool trace_chunks = getenv("LASSO_STOP_TRACE") != nullptr;        // the chunks and their verdicts on stderr
  T deltas[kChunkMax];
  T last = (T)NAN;
  int it = 0, chunk = 1;
  while (it < maxiter) {
    const int c = std::min(chunk, maxiter - it);
    const double t_head = *t_mom;
    if (c > 1)
      if (int s = save()) return s;
    for (int j = 0; j < c; ++j)
      if (int s = iterate(delta_dev + j)) return s;
    if (int s = flush()) return s;
    if (int s = read(deltas, c)) return s;
    const int hit = first_stop<T>(deltas, c, budget);                              // (compared in T like the reference)
    if (trace_chunks)
      fprintf(stderr, "%s: iterations %d..%d sums %g .. %g budget %g -> %s %d\n", who, it, it + c - 1, (double)deltas[0],
              (double)deltas[c - 1], (double)budget, hit < 0 ? "no stop" : "stop at", hit < 0 ? 0 : it + hit + 1);
    if (hit < 0) {
      it += c;
      last = deltas[c - 1];
      chunk = next_stop_chunk<T>(deltas[0], last, budget, c, it, kChunkMax);
      continue;
    }
    last = deltas[hit];
    if (hit < c - 1) {
      if (int s = restore()) return s;
      *t_mom = t_head;
      for (int j = 0; j <= hit; ++j)
        if (int s = iterate(nullptr)) return s;
      if (int s = flush()) return s;
    }
    it += hit + 1;
    break;
  }
  *it_out = it;
  *last_out = last;
  return 0;
}

// The four int32 words a kernel that judges the stop rule itself leaves behind.
struct StopWords {
  int32_t w[4] = {0, 0, 0, 0};
  int iterations() const { return w[0]; }
  float last_delta() const { float f; memcpy(&f, &w[1], sizeof(float)); return f; }    // (word 1 holds its bits)
  bool redo() const { return w[2] != 0; }      // nothing usable: a workgroup was not resident, or the rule fired inside a chunk
  bool warned() const { return w[3] != 0; }    // a line search ran out of trials
};

}  // namespace lasso
