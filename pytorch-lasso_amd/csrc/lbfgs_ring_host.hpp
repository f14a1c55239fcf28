// The L-BFGS memory of the OWL-QN driver (owlqn.hip) as the host sees it: which physical slots of the pair ring are
// held, where the next candidate pair goes, and which of two buffers holds x_prev / g_prev.  The vectors live on the GPU;
// the host only moves these few integers, driven by the verdict `keep` (y.s > 1e-10) that each iteration's control record
// carries -- the reference's L_BFGS.update (lasso/nonlinear/owlqn.py:34-51).
//
//   PairRing ring(history);                 history + 1 physical slots: the spare one takes the candidate, so a dropped
//   ring.candidate()                        pair never costs a held one
//   ring.update(keep)                       keep: the candidate is held; the oldest pair leaves once `history` are held
//   ring.slot(i)                            physical slot of the i-th oldest held pair, i < ring.count()
//
//   TwoBuffers zb;                          x lives in buffer cur(), x_prev in buffer prev()
//   zb.target()                             where the next x may be written without touching x_prev
//   zb.stepped(); zb.update(keep);          x moved to target(); keep: x_prev = x
//
// Host compiler only, integers only.  tests/test_lbfgs_ring_host_cpu.py drives it against a list-based restatement of
// the reference, plain and under AddressSanitizer + UBSan (tests/c_host/lbfgs_ring_host_main.cpp).
#pragma once

namespace lasso {

class PairRing {
 public:
  explicit PairRing(int history) : cap_(history < 0 ? 0 : history), slots_(cap_ + 1) {}
  int capacity() const { return cap_; }
  int slots() const { return slots_; }
  int head() const { return head_; }
  int count() const { return count_; }
  int slot(int i) const { return (head_ + i) % slots_; }
  int candidate() const { return (head_ + count_) % slots_; }
  int newest() const { return count_ > 0 ? slot(count_ - 1) : -1; }
  // -> the physical slot that became the newest held pair, or -1 (dropped, or a memory of no pairs)
  int update(bool keep) {
    if (!keep || cap_ == 0) return -1;
    const int taken = candidate();
    if (count_ == cap_)
      head_ = (head_ + 1) % slots_;
    else
      ++count_;
    return taken;
  }

 private:
  int cap_, slots_, head_ = 0, count_ = 0;
};

class TwoBuffers {
 public:
  int cur() const { return cur_; }
  int prev() const { return prev_; }
  int target() const { return prev_ == cur_ ? 1 - cur_ : cur_; }
  void stepped() { cur_ = target(); }
  void update(bool keep) {
    if (keep) prev_ = cur_;
  }

 private:
  int cur_ = 0, prev_ = 0;
};

}  // namespace lasso
