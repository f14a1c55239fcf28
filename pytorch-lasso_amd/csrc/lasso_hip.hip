// C-ABI layer of the MI355X FISTA engine (include/lasso_hip.h) plus the small
// support kernels (W packing, momentum table, per-iteration delta reduction).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../include/lasso_hip.h"
#include "lasso_kernels.h"
#include "host_util.hpp"
#include "stoprule_host.hpp"

namespace lasso {

static thread_local char g_err[512] = "";

int fail(int status, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return status;
}

namespace {

int pad_k(int64_t k) {
  if (k <= 256) return 256;
  if (k <= 512) return 512;
  if (k <= 1024) return 1024;
  return -1;
}

// Padded feature count of the fused FISTA kernel: tiles are M x D with M*D = 4096, and the
// y tile (M x Kp fp32) must fit 64 KiB of LDS, so small dictionaries get taller tiles.
int pad_d(int64_t d, int kp);

// ---------------------------------------------------------------------------
// workspace layout
// ---------------------------------------------------------------------------
constexpr int kChunkMax = 64;     // iterations per launch when deltas are recorded

constexpr int kSplitMaxParts = kSplitkMaxParts;

struct Workspace {
  float* wp;        // [256][Kp]
  float* wtp;       // [Kp][256]
  float* coef;      // [coef_cap]  FISTA momentum coefficients
  float* zeros;     // [coef_cap]  ISTA "coefficients"
  float* partials;  // [kChunkMax][ntiles * members]
  float* delta;     // [kChunkMax]
  unsigned long long* gran;  // [kStopRing][max(ntiles, 256)] in-kernel stop-rule granules
  int* stop_out;    // [4]
  float* xch;       // split-k kernel: [2][256][16 KiB] partial-residual exchange
  unsigned* xflags; // split-k kernel: [256][waves] epoch tags
  float* state[4];  // zA, yA, zB, yB  [n][k]   (stop rule only)
  size_t bytes;
};

Workspace carve(void* base, int64_t n, int64_t k, int kp, int coef_cap, bool with_state) {
  Workspace w;
  Arena a(base);
  const int64_t ntiles = (n + kTileM - 1) / kTileM;
  w.wp = a.take((size_t)kFistaD * kp * 4);
  w.wtp = a.take((size_t)kp * kFistaD * 4);
  w.coef = a.take((size_t)std::max(coef_cap, 1) * 4);
  w.zeros = a.take((size_t)std::max(coef_cap, 1) * 4);
  const int members = kp / 128;                       // split-k: members per group
  // [kChunkMax][ntiles] of the tile kernel, then the split-k kernel's rows: one partial per
  // workgroup and round, rounds * groups * members <= (ntiles + 256) * members
  w.partials = a.take((size_t)kChunkMax * ntiles * 4 + (size_t)kChunkMax * (ntiles + kSplitMaxParts) * members * 4);
  w.delta = a.take((size_t)kChunkMax * 4);
  w.gran = a.take<unsigned long long>((size_t)kStopRing * std::max<int64_t>(ntiles, kSplitMaxParts) * 8);
  w.stop_out = a.take<int>(256);
  // exchange payload of the split-k kernel: up to 256 workgroups x T tiles at once, T by batch size
  {
    const int64_t slots = (ntiles * members + kSplitMaxParts - 1) / kSplitMaxParts;   // tiles per group if all 256 CUs take part
    const int tmax = slots <= 1 ? 1 : slots <= 2 ? 2 : kSplitkMaxTiles;
    w.xch = a.take(fista_splitk_exchange_bytes(kp, kSplitMaxParts / members, tmax));
  }
  w.xflags = a.take<unsigned>(kSplitkFlagBytes);
  for (int i = 0; i < 4; ++i) w.state[i] = with_state ? a.take((size_t)n * k * 4) : nullptr;
  w.bytes = a.bytes();
  return w;
}

// ---------------------------------------------------------------------------
// support kernels
// ---------------------------------------------------------------------------
// Wp[r][c] = W[r][c] (zero padded to [256][Kp]); Wtp[c][r] = W[r][c].
__global__ void pack_w_kernel(const float* __restrict__ W, int64_t ldw, int d, int k, int kp,
                              float* __restrict__ wp, float* __restrict__ wtp, int dpad = kFistaD) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;   // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    const float v = (r < d && c < k) ? W[(int64_t)r * ldw + c] : 0.0f;
    tile[i][tx] = v;
    wp[(size_t)r * kp + c] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    wtp[(size_t)c * dpad + r] = tile[tx][i];
  }
}

// Momentum table (ista.py:78,98-100): t_0 = 1, t_{i+1} = (1+sqrt(1+4 t_i^2))/2,
// coef_i = (float)((t_i - 1)/t_{i+1}).  Evaluated in IEEE double without
// contraction so it reproduces the reference's python-float arithmetic.
__global__ void momentum_table_kernel(float* __restrict__ coef, float* __restrict__ zeros, int count) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = 1.0;
  for (int i = 0; i < count; ++i) {
    const double tt = __dmul_rn(t, t);
    const double s = __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(4.0, tt)));
    const double tn = __ddiv_rn(__dadd_rn(1.0, s), 2.0);
    coef[i] = (float)__ddiv_rn(__dsub_rn(t, 1.0), tn);
    zeros[i] = 0.0f;
    t = tn;
  }
}

// Everything a solve needs before its persistent launch, in ONE launch (the EM step is made of
// ~10 such 5-us launches otherwise): pack W (pack_w_kernel), the momentum table
// (momentum_table_kernel, by the last block), zero the stop rule's granule ring and result words,
// and -- lr = LASSO_LR_AUTO -- turn lambda_max into {lr, alpha*lr} (step_from_lipschitz_kernel).
// (PrepareExtras, CoefHead, PrepareJob and the launch's device code: lasso_kernels.h -- the Lipschitz launch of an
// lr = LASSO_LR_AUTO solve carries the same blocks, csrc/lipschitz.hip)
static const CoefHead& coef_head() {
  static const CoefHead head = [] {
    CoefHead h;
    Momentum mom;
    for (int i = 0; i < kCoefHead; ++i) h.v[i] = mom.next(true);
    h.t_next = mom.t;
    return h;
  }();
  return head;
}
__global__ void prepare_solve_kernel(const PrepareJob j) {
  __shared__ float tile[32][33];
  prepare_block(j, blockIdx.x, blockIdx.y, threadIdx.y * 32 + threadIdx.x, tile);
}

// delta[i] = sum_t partials[i][t], fixed summation order (deterministic).  `alt` (nullable):
// the rows of the stand-by launch, taken instead when *alt_if != 0 (the split-k kernel gave up).
// `base` (nullable): rows that are always added in front -- a ragged batch whose full rounds ran on the tile kernel
// and whose tail ran on the split-k kernel (PartialSets below).
struct PartialSets {
  const float* src; int n, stride;            // the launch's own partial sums, row i at src + i * stride
  const float* alt; int alt_n, alt_stride;    // stand-by rows, nullable
  const int* alt_if;
  const float* base; int base_n, base_stride; // nullable
};
struct DeferredVerdict { void* workspace; PartialSets ps; float* delta; int iters; float budget; int* out; bool armed; };
// the arguments of the verdict launch an asynchronous solve of THIS thread left out (one slot: the EM loop's E-step)
static thread_local DeferredVerdict t_deferred_verdict = {nullptr, {}, nullptr, 0, 0.0f, nullptr, false};
__global__ void reduce_partial_sets_kernel(const PartialSets ps, float* __restrict__ delta) {
  __shared__ float sh[256];
  const float* partials = ps.src;
  int ntiles = ps.n, stride = ps.stride;
  if (ps.alt && *ps.alt_if != 0) { partials = ps.alt; ntiles = ps.alt_n; stride = ps.alt_stride; }
  float acc = 0.0f;
  if (ps.base) {
    const float* brow = ps.base + (size_t)blockIdx.x * ps.base_stride;
    for (int t = threadIdx.x; t < ps.base_n; t += 256) acc += brow[t];
  }
  const float* row = partials + (size_t)blockIdx.x * stride;
  for (int t = threadIdx.x; t < ntiles; t += 256) acc += row[t];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) delta[blockIdx.x] = sh[0];
}

// the plain form: delta[i] = sum of row i of a dense [rows][ntiles] array (line search, unfused path)
// dst[0 .. n) = src[0 .. n) (both 16-byte aligned): the checkpoints of lasso_conv_ista_solve.  A kernel of our own
// rather than hipMemcpyAsync: with the runtime's device-to-device copies, 2 of 7 timed runs of a 10 / 20-iteration solve
// on 134 MB codes came out 2-5 ms per solve slow (profiles/r04/ab_conv_stop_rule.txt: none in 4 runs with this kernel;
// the cause inside the runtime was not established -- a copy engine instead of a blit kernel would fit the figure).
__global__ __launch_bounds__(256) void copy_words_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride)
    ((v4*)dst)[i] = __builtin_nontemporal_load((const v4*)src + i);
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

__global__ void reduce_partials_kernel(const float* __restrict__ partials, int ntiles, float* __restrict__ delta) {
  __shared__ float sh[256];
  const float* row = partials + (size_t)blockIdx.x * ntiles;
  float acc = 0.0f;
  for (int t = threadIdx.x; t < ntiles; t += 256) acc += row[t];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) delta[blockIdx.x] = sh[0];
}

// reduce_partial_sets_kernel for `iters` rows and chunk_verdict_kernel behind it in ONE workgroup (the asynchronous
// E-step of an EM loop: one launch less on the step's dependent chain).  Every delta[i] is the same sum in the
// same order as reduce_partials_kernel's.
// defer (nullable): do not launch reduce_verdict_kernel -- leave its arguments there (LASSO_SOLVE_DEFER_VERDICT: the caller
// launches it on another stream, lasso_fista_solve_verdict_deferred)
struct DeferredVerdict;
struct ChunkVerdict { float budget; int* out; int* mirror; DeferredVerdict* defer = nullptr; };
// the verdict's four words a second time, into a device-writable HOST buffer (pinned, mapped; LASSO_SOLVE_STATUS_MAPPED):
// the caller's one host read per EM step then needs no copy launch behind the verdict
__device__ __forceinline__ void mirror_status(int* mirror, int w0, int w1, int w2) {
  if (!mirror) return;
  __hip_atomic_store(mirror + 0, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(mirror + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(mirror + 2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // word 3 = "valid", written last and released: a host that has zeroed it before the call may POLL it instead of
  // recording an event behind the launch (an event record costs the stream ~5 us between two kernels)
  __hip_atomic_store(mirror + 3, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// gate (nullable; the deferred launch on another stream): the word that stream's wait polled -- if it does not hold
// gate_value the wait ran into its bound and the solve's kernels may still be running: the verdict is then "repeat the
// solve" (out[2] = 1), never a judgement of unfinished sums.
__global__ __launch_bounds__(1024) void reduce_verdict_kernel(const PartialSets ps, float* __restrict__ delta, int iters,
                                                              float budget, int* __restrict__ out, int* mirror,
                                                              const int* gate = nullptr, int gate_value = 0) {
  if (gate && __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gate_value) {     // (words count up)
    if (threadIdx.x == 0) {
      out[0] = 0; out[1] = __float_as_int(NAN); out[2] = 1; out[3] = 0;
      mirror_status(mirror, out[0], out[1], out[2]);
    }
    return;
  }
  // One WAVE per row, rows w, w + 16, ... (16 waves: the 10 rows of an EM step's chunk in one pass): lane l plays reduce_partials_kernel's threads l, l + 64, l + 128, l + 192
  // (their strided sums), the first two levels of its tree are then this lane's (a0 + a2) + (a1 + a3), the last six
  // the shuffles below -- no barrier per row.
  __shared__ float sd[64];
  const float* partials = ps.src;
  int ntiles = ps.n, stride = ps.stride;
  if (ps.alt && *ps.alt_if != 0) { partials = ps.alt; ntiles = ps.alt_n; stride = ps.alt_stride; }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = w; i < iters; i += 16) {
    const float* row = partials + (size_t)i * stride;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (ps.base) {
      const float* brow = ps.base + (size_t)i * ps.base_stride;
#pragma unroll
      for (int h = 0; h < 4; ++h)
        for (int t = lane + 64 * h; t < ps.base_n; t += 256) a[h] += brow[t];
    }
#pragma unroll
    for (int h = 0; h < 4; ++h)
      for (int t = lane + 64 * h; t < ntiles; t += 256) a[h] += row[t];
    float v = (a[0] + a[2]) + (a[1] + a[3]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    if (lane == 0) { delta[i] = v; sd[i] = v; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int hit = -1;
    float last = sd[iters - 1];
    for (int i = 0; i < iters; ++i)
      if (sd[i] <= budget) { hit = i; last = sd[i]; break; }
    out[0] = hit >= 0 ? hit + 1 : iters;
    out[1] = __float_as_int(last);
    out[2] = (hit >= 0 && hit + 1 < iters) ? 1 : 0;
    out[3] = 0;
    mirror_status(mirror, out[0], out[1], out[2]);
  }
}

// the stop rule over one chunk's per-iteration deltas (ista.py:93-95): out = {iterations, last delta, redo, 0};
// redo = the rule fired before the chunk's last iteration
__global__ void chunk_verdict_kernel(const float* __restrict__ delta, int c, float budget, int* __restrict__ out,
                                     int* mirror) {
  int hit = -1;
  float last = delta[c - 1];
  for (int i = 0; i < c; ++i)
    if (delta[i] <= budget) { hit = i; last = delta[i]; break; }
  out[0] = hit >= 0 ? hit + 1 : c;
  out[1] = __float_as_int(last);
  out[2] = (hit >= 0 && hit + 1 < c) ? 1 : 0;
  out[3] = 0;
  mirror_status(mirror, out[0], out[1], out[2]);
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}

bool fused_shape(int64_t d, int64_t k) { return d <= kFistaD && k <= kFistaMaxK; }

// workgroups of the fused kernel that can be resident at once (occupancy query x CUs)
int fista_resident_workgroups(int kp, int dpad, int waves = kFistaWaves) {
  int per_cu = 0;
  if (fista_tile_sp_occupancy(kp, dpad, &per_cu, waves) != hipSuccess) return 0;
  return per_cu * device_cus();
}

// Tile geometry of the one-workgroup-per-tile kernel for a batch of n rows: 8-wave workgroups on
// tiles of 4096 / dpad rows, or -- short rows (dpad <= 128) whose tiles would not give every CU
// its share -- 4-wave workgroups on half-height tiles, two per CU (the same waves per CU on twice
// as many tiles; per CU the longest queue of rows is what counts).
struct TilePlan { int waves, rows, ntiles; };
TilePlan plan_tiles(int64_t n, int dpad, int kp = 0) {
  TilePlan t = {kFistaWaves, 4096 / dpad, 0};
  if (kp > 512 && dpad == 128) {       // 128 columns with more than 512 atoms: the 32-row y tile does not fit -- 4 waves on 16 rows
    t.waves = 4; t.rows = 16;
    t.ntiles = (int)((n + 15) / 16);
    return t;
  }
  t.ntiles = (int)((n + t.rows - 1) / t.rows);
  if (dpad >= kFistaD || n <= 0) return t;
  const int cus = std::max(device_cus(), 1);
  const int64_t full_rows = (int64_t)((t.ntiles + cus - 1) / cus) * t.rows;       // rows queued on the busiest CU
  const int half = t.rows / 2, nh = (int)((n + half - 1) / half);
  const int64_t half_rows = (int64_t)((nh + cus - 1) / cus) * half;
  if (half_rows * 10 <= full_rows * 9) { t.waves = 4; t.rows = half; t.ntiles = nh; }
  return t;
}

// (lasso_fista_solve may narrow the tile for the extent of one call: d <= 128 with more than 512 atoms on a batch that
// fills the chip runs 4-wave workgroups on 16 x 128 tiles -- `NarrowTiles` below; thread-local like the error text)
static thread_local int g_dpad_override = 0;
int pad_d(int64_t d, int kp) {
  if (g_dpad_override) return g_dpad_override;
  if (d <= 64 && kp <= 256) return 64;
  if (d <= 128 && kp <= 512) return 128;
  return kFistaD;
}
struct NarrowTiles {
  explicit NarrowTiles(bool on) : on_(on) { if (on_) g_dpad_override = 128; }
  ~NarrowTiles() { if (on_) g_dpad_override = 0; }
  bool on_;
};

int check_common(int64_t n, int64_t d, int64_t k, int dtype, bool allow_large = false) {
  if (dtype != LASSO_F32)
    return fail(LASSO_ERR_UNSUPPORTED, "dtype %d: only LASSO_F32 is implemented", dtype);
  if (n < 0 || d <= 0 || k <= 0) return fail(LASSO_ERR_BAD_ARG, "bad shape n=%lld d=%lld k=%lld",
                                              (long long)n, (long long)d, (long long)k);
  if (!allow_large && !fused_shape(d, k))
    return fail(LASSO_ERR_UNSUPPORTED,
                "shape d=%lld k=%lld exceeds the fused kernel (d<=%d, k<=%d)", (long long)d,
                (long long)k, kFistaD, kFistaMaxK);
  if (n > (int64_t)INT32_MAX - kTileM) return fail(LASSO_ERR_UNSUPPORTED, "n too large");
  return LASSO_OK;
}

// Which fused kernel runs a batch: the split-k kernel (a 16-row tile shared by Kp/128
// workgroups, fista_splitk.hip) when the one-workgroup-per-tile kernel would leave most of the
// chip idle.  `lockstep`: the in-kernel stop rule needs every tile to own a resident group.
// Cost model of the two kernels in microseconds per iteration and round on MI355X
// (tools/bench_small.py): the tile kernel runs ceil(ntiles / #CUs) rounds of tile_us; the
// split-k kernel with T tiles per group runs ceil(ntiles / (groups * T)) rounds of split_us[T].
struct KernelCost { double tile_us, split_us[3]; };   // split_us: T = 1, 2, 4
KernelCost kernel_cost(int kp) {
  if (kp >= 1024) return {31.0, {5.9, 10.4, 18.9}};      // T >= 2: the reduce-scatter form (fista_splitk_rs_kernel)
  if (kp >= 768) return {23.6, {1e9, 1e9, 1e9}};        // (768 atoms: tile kernel only -- 6 members do not split)
  if (kp >= 512) return {15.9, {5.45, 9.9, 19.4}};
  return {8.3, {5.2, 9.6, 18.9}};
}
struct KernelPlan { bool split; int groups, tiles; double us; };   // us: the model's microseconds per iteration

int splitk_max_groups(int kp) {
  int per_cu = 0;
  if (fista_splitk_occupancy(kp, &per_cu) != hipSuccess) return 0;
  const int resident = std::min(per_cu * device_cus(), kSplitMaxParts);
  const int members = fista_splitk_members(kp);
  return resident / (8 * members) * 8;                // whole rows of 8 groups (one per XCD)
}

KernelPlan plan_kernel(int kp, int dpad, int ntiles, bool lockstep, int hint_bits) {
  KernelPlan plan = {false, 0, 1, 0.0};
  const int hint = hint_bits & 0x300;
  const int cus = std::max(device_cus(), 1);
  const KernelCost cost = kernel_cost(kp);
  plan.us = cost.tile_us * ((ntiles + cus - 1) / cus);
  if (dpad != kFistaD || hint == LASSO_KERNEL_TILE || ntiles <= 0) return plan;
  const int gmax = splitk_max_groups(kp);
  if (gmax <= 0) return plan;
  // (5 % in favour of the tile kernel: it has no cross-workgroup dependencies)
  double best = hint == LASSO_KERNEL_SPLITK ? 1e30 : 0.95 * cost.tile_us * ((ntiles + cus - 1) / cus);
  const int forced = (hint_bits >> 12) & 3;           // LASSO_KERNEL_SPLITK_TILES(T): 1, 2, 3 -> T = 1, 2, 4
  for (int ti = 0; ti < 3; ++ti) {
    if (forced && ti != forced - 1) continue;
    const int T = 1 << ti;
    const int groups = std::min(gmax, (ntiles + T - 1) / T);
    const int rounds = (ntiles + groups * T - 1) / (groups * T);
    if (lockstep && rounds > 1) continue;             // the in-kernel stop rule needs every tile in a resident slot
    // the kernel's cost is linear in the tile slots a group works on, and the last round may fill fewer of them
    const int last_tiles = ntiles - (rounds - 1) * groups * T, last_slots = (last_tiles + groups - 1) / groups;
    const double slot_us[5] = {0.0, cost.split_us[0], cost.split_us[1], 0.5 * (cost.split_us[1] + cost.split_us[2]),
                               cost.split_us[2]};
    const double us = cost.split_us[ti] * (rounds - 1) + slot_us[std::min(last_slots, 4)];
    if (us < best) { best = us; plan.split = true; plan.groups = groups; plan.tiles = T; plan.us = us; }
  }
  return plan;
}

// Tiles of a ragged batch's last, partly filled round that go to the split-k kernel (0: none); see run_impl.
// `whole`: what plan_kernel() chose for the whole batch (tile kernel alone, or split-k alone); the hybrid must beat it.
int ragged_tail(int kp, int dpad, int ntiles, int waves, int hint, const KernelPlan& whole, KernelPlan* tail_plan) {
  const int cus = std::max(device_cus(), 1);
  const int rounds = (ntiles + cus - 1) / cus;
  if (rounds < 2 || dpad != kFistaD || waves != kFistaWaves || (hint & 0x300) != LASSO_KERNEL_AUTO) return 0;
  const int t = ntiles - (rounds - 1) * cus;
  if (t >= cus) return 0;
  const KernelPlan sp = plan_kernel(kp, dpad, t, false, LASSO_KERNEL_SPLITK);
  const double tile_us = kernel_cost(kp).tile_us;
  if (!sp.split) return 0;
  const double hybrid_us = (rounds - 1) * tile_us + sp.us;
  if (hybrid_us >= 0.95 * rounds * tile_us || (whole.split && hybrid_us >= whole.us)) return 0;
  if (tail_plan) *tail_plan = sp;
  return t;
}

// Geometry of a fixed-step fp32 solve on the fused shapes: padded dictionary size and tile width.
//   * 256 < k <= 384 with d <= 128: the 384-atom instantiations of the d <= 128 tile kernels;
//   * 512 < k <= 768: the 768-atom instantiation of the tile kernel (a quarter less work than padding to 1024) where it
//     beats what the cost model picks at 1024 (small batches run the split-k kernel there, which needs a power of two
//     of 128-atom slices);
//   * d <= 128 with more than 512 atoms: NARROW tiles -- 4-wave workgroups on 16 x 128 tiles instead of 8 waves on
//     16 x 256 -- half the padded work per tile at nearly the same rate per wave (d=64, k=1024: 34 -> 60 TFLOP/s useful;
//     d=128: 68 -> 119), again only where that beats the split-k kernel of a small batch.
// Costs in microseconds per iteration and round of 256 tiles, measured on MI355X (round 3).  Every choice gives bitwise
// the same code for a row (canonical 128-atom slices, exact-zero padding).  A function of the shape alone: the second
// halves of an asynchronous solve carve the same workspace layout.
struct SolveGeom { int kp; bool narrow; };
SolveGeom solve_geometry(int64_t n, int64_t d, int64_t k) {
  const int kp0 = pad_k(k);
  if (kp0 == 512 && k <= 384 && d <= 128 && n > 0) return {384, false};
  if (kp0 != 1024 || n <= 0) return {kp0, false};
  const int ntiles = (int)((n + kTileM - 1) / kTileM);
  const int cus = std::max(device_cus(), 1);
  const int rounds = (ntiles + cus - 1) / cus;
  SolveGeom best = {1024, false};
  const KernelPlan whole = plan_kernel(1024, kFistaD, ntiles, false, LASSO_KERNEL_AUTO);
  double best_us = whole.us;
  {   // a ragged batch at 1024 atoms: full rounds on the tile kernel + the tail on the split-k kernel (run_impl)
    KernelPlan tp = {false, 0, 1, 0.0};
    if (ragged_tail(1024, kFistaD, ntiles, kFistaWaves, LASSO_KERNEL_AUTO, whole, &tp))
      best_us = (rounds - 1) * kernel_cost(1024).tile_us + tp.us;
  }
  auto consider = [&](int kp, bool narrow, double us_per_round) {
    if (us_per_round * rounds < best_us) { best_us = us_per_round * rounds; best = {kp, narrow}; }
  };
  if (k <= 768) consider(768, false, kernel_cost(768).tile_us);
  if (d <= 128) {
    consider(1024, true, 18.0);
    if (k <= 768) consider(768, true, 13.7);
  }
  return best;
}
int pad_k_solve(int64_t n, int64_t d, int64_t k) { return solve_geometry(n, d, k).kp; }
bool narrow_tiles(int64_t n, int64_t d, int64_t k, int kp, int hint_bits) {
  if (d > 128 || kp <= 512 || n <= 0) return false;
  if ((hint_bits & 0x800) && (hint_bits & 0x300) == LASSO_KERNEL_AUTO) return true;   // A/B knob "narrow": 0x800 ALONE
  if ((hint_bits & 0x300) == LASSO_KERNEL_SPLITK) return false;   // (with LASSO_KERNEL_SPLITK 0x800 is the exchange variant)
  return solve_geometry(n, d, k).narrow;
}

int run_impl(const Workspace& ws, int kp, const float* x, int64_t ldx, const float* z_in,
             int64_t ldz_in, const float* y_in, int64_t ldy_in, float* z_out, int64_t ldz_out,
             float* y_out, int64_t ldy_out, int64_t n, int64_t d, int64_t k, double alpha, double lr,
             int fast, int it0, int iters, float* delta, hipStream_t stream, float stop_budget = -1.0f,
             int hint = LASSO_KERNEL_AUTO, bool* used_split = nullptr, const float* lr_dev = nullptr,
             const ChunkVerdict* verdict = nullptr) {
  if (used_split) *used_split = false;
  if (n == 0) return LASSO_OK;
  const int dpad = pad_d(d, kp);
  const TilePlan tp = plan_tiles(n, dpad, kp);
  const int ntiles = tp.ntiles;
  FistaTileParams p;
  p.X = x; p.ldx = ldx;
  p.Wp = ws.wp; p.Wtp = ws.wtp;
  p.z_in = z_in; p.ldz_in = ldz_in;
  p.y_in = y_in; p.ldy_in = ldy_in;
  p.z_out = z_out; p.ldz_out = ldz_out;
  p.y_out = y_out; p.ldy_out = ldy_out;
  p.coef = (fast ? ws.coef : ws.zeros) + it0;
  p.partials = delta ? ws.partials : nullptr;
  p.n = (int)n; p.d = (int)d; p.k = (int)k;
  p.ntiles = ntiles; p.iters = iters;
  p.lr = (float)lr;                 // ATen casts the python scalar to the tensor dtype
  p.lam = (float)(alpha * lr);      // softshrink(lambd = alpha*lr), product in double (ista.py:90)
  p.lr_dev = lr_dev;                // LASSO_LR_AUTO: {lr, lam} read from device memory instead
  p.stop_on = stop_budget >= 0.0f;
  p.stop_budget = stop_budget;
  p.stop_gran = ws.gran;
  p.stop_out = ws.stop_out;
  p.xch = nullptr; p.xflags = nullptr; p.groups = 0;
  p.run_if = nullptr; p.part_stride = ntiles;
  // A/B knobs of the split-k kernel (only together with LASSO_KERNEL_SPLITK; 0x800 alone is the "narrow tiles" knob)
  p.variant = (hint & 0x300) != LASSO_KERNEL_SPLITK ? 0 : (hint & 0x400) ? 1 : (hint & 0x800) ? 2 : 0;
  const int cus = device_cus();
  if (cus <= 0) return fail(LASSO_ERR_HIP, "no HIP device");
  // in-place launches keep the tile kernel: a split-k launch that gives up is redone from its
  // inputs, which must still be there
  const bool in_place = (z_in && z_in == z_out) || (y_in && y_in == y_out) || (y_in && y_in == z_out) ||
                        (z_in && y_out && z_in == y_out);
  // (the split-k kernel reads a tile's 16 rows of x / z / y through 32-bit buffer offsets: a row pitch of 2^31 / 64 floats
  // or more keeps the tile kernel, whose loads are 64-bit addressed -- ADVICE r05: the descriptor clamped silently)
  const bool wide_pitch = std::max(std::max(ldx, ldz_in), std::max(ldy_in, std::max(ldz_out, ldy_out))) * 64 >= ((int64_t)1 << 31);
  KernelPlan plan = plan_kernel(kp, dpad, ntiles, p.stop_on != 0, (in_place || wide_pitch) ? LASSO_KERNEL_TILE : hint);
  float* const split_rows = ws.partials + (size_t)kChunkMax * ntiles;    // behind the tile kernel's rows
  // ---- ragged batches (round 4): the tile kernel runs ceil(ntiles / #CUs) rounds, so 257 tiles cost what 512 do.
  // The LAST, partly filled round goes to the split-k kernel instead when the cost model says so: the full rounds on
  // the tile kernel (rows [0, n_main)), then the tail's tiles on the split-k kernel (its own launch on the same
  // stream; rows are independent and a row's code is bitwise the same from either kernel).  n = 5000 at k = 1024:
  // 63 -> 42 us per iteration.
  KernelPlan tplan = {false, 0, 1, 0.0};
  const int tail = (in_place || wide_pitch || p.stop_on) ? 0 : ragged_tail(kp, dpad, ntiles, tp.waves, hint, plan, &tplan);
  if (tail) plan.split = false;                  // (the hybrid beats the split-k kernel on the whole batch as well)
  // the split-k kernel on the tiles of `q` (+ its stand-by): returns the partial sums per row of that launch
  auto launch_split = [&](FistaTileParams q, const KernelPlan& pl, float* standby_partials, int* nparts_out) -> int {
    // cross-workgroup hand-offs: epoch tags and the abort flag start from zero in every launch
    q.xch = ws.xch; q.xflags = ws.xflags; q.groups = pl.groups;
    const int members = fista_splitk_members(kp);
    const int rounds = (q.ntiles + pl.groups * pl.tiles - 1) / (pl.groups * pl.tiles);
    const int np = rounds * pl.groups * members;      // one partial per workgroup and round
    *nparts_out = np;
    q.part_stride = np;
    if (q.partials) q.partials = split_rows;
    LASSO_HIP_TRY(hipMemsetAsync(ws.xflags, 0, kSplitkFlagBytes, stream));
    if (!q.stop_on) LASSO_HIP_TRY(hipMemsetAsync(ws.stop_out, 0, 16, stream));   // (the stop-rule caller zeroed it)
    LASSO_HIP_TRY(launch_fista_splitk(q, kp, pl.tiles, stream));
    if (used_split) *used_split = true;
    if (!q.stop_on) {
      // No host synchronisation on this path, so the stand-by is enqueued right behind: the tile
      // kernel, which returns at once unless the split-k kernel raised its abort flag (a peer
      // workgroup was not resident) -- then it redoes the launch from the untouched inputs.
      // (With the stop rule on, the caller reads the flag at its synchronisation instead.)
      FistaTileParams f = q;
      f.run_if = ws.stop_out + 2;
      f.part_stride = ntiles;
      if (f.partials) f.partials = standby_partials;
      LASSO_HIP_TRY(launch_fista_tile_sp(f, kp, dpad, std::min(q.ntiles, cus), stream, tp.waves));
    }
    return LASSO_OK;
  };
  int nparts = ntiles;
  const int main_tiles = ntiles - tail;
  if (plan.split) {
    if (int st = launch_split(p, plan, ws.partials, &nparts)) return st;
  } else {
    // persistent over tiles: one 8-wave workgroup per CU (LDS bound), or two 4-wave ones
    FistaTileParams pm = p;
    if (tail) { pm.n = main_tiles * kTileM; pm.ntiles = main_tiles; }
    const int grid = std::min(main_tiles, cus * ((tp.waves == 4 && kp <= 512) ? 2 : 1));   // (4 waves, > 512 atoms: 104 KiB of LDS, one per CU)
    LASSO_HIP_TRY(launch_fista_tile_sp(pm, kp, dpad, grid, stream, tp.waves));
    if (tail) {
      const int64_t r0 = (int64_t)main_tiles * kTileM;
      FistaTileParams q = p;
      q.X = p.X + r0 * p.ldx;
      if (p.z_in) q.z_in = p.z_in + r0 * p.ldz_in;
      if (p.y_in) q.y_in = p.y_in + r0 * p.ldy_in;
      q.z_out = p.z_out + r0 * p.ldz_out;
      if (p.y_out) q.y_out = p.y_out + r0 * p.ldy_out;
      q.n = (int)(n - r0); q.ntiles = tail;
      if (int st = launch_split(q, tplan, ws.partials + main_tiles, &nparts)) return st;
    }
  }
  if (delta && iters > 0) {
    PartialSets ps = {ws.partials, ntiles, ntiles, nullptr, 0, 0, nullptr, nullptr, 0, 0};
    if (plan.split) ps = {split_rows, nparts, nparts, ws.partials, ntiles, ntiles, ws.stop_out + 2, nullptr, 0, 0};
    else if (tail) ps = {split_rows, nparts, nparts, ws.partials + main_tiles, tail, ntiles, ws.stop_out + 2,
                         ws.partials, main_tiles, ntiles};
    if (verdict && iters <= 64 && verdict->defer) {     // the caller enqueues that launch itself, on another stream
      DeferredVerdict& dv = *verdict->defer;
      dv.ps = ps; dv.delta = delta; dv.iters = iters; dv.budget = verdict->budget; dv.out = verdict->out; dv.armed = true;
    } else if (verdict && iters <= 64)
      hipLaunchKernelGGL(reduce_verdict_kernel, dim3(1), dim3(1024), 0, stream, ps, delta, iters, verdict->budget, verdict->out,
                         verdict->mirror);
    else
      hipLaunchKernelGGL(reduce_partial_sets_kernel, dim3(iters), dim3(256), 0, stream, ps, delta);
    LASSO_HIP_TRY(hipGetLastError());
  }
  return LASSO_OK;
}

// The four result words a kernel that judges the stop rule itself left at `dev` (StopWords, stoprule_host.hpp)
int read_stop_words(const int* dev, hipStream_t stream, StopWords* words) { return read_back(words->w, dev, 16, stream); }

static PrepareJob prepare_job(const Workspace& ws, int kp, const float* w, int64_t ldw, int64_t d, int64_t k, int coef_cap,
                              const PrepareExtras* extras) {
  PrepareJob j;
  j.W = w; j.ldw = ldw; j.d = (int)d; j.k = (int)k; j.kp = kp;
  j.wp = ws.wp; j.wtp = ws.wtp; j.dpad = pad_d(d, kp); j.coef = ws.coef; j.zeros = ws.zeros;
  j.count = std::max(coef_cap, 1);
  j.x = PrepareExtras{nullptr, 0, nullptr, 0, nullptr, 0.0, nullptr};
  if (extras) j.x = *extras;
  j.head = coef_head();
  j.gx = kp / 32; j.gy = j.dpad / 32;
  return j;
}

int prepare_impl(const Workspace& ws, int kp, const float* w, int64_t ldw, int64_t d, int64_t k,
                 int coef_cap, hipStream_t stream, const PrepareExtras* extras = nullptr) {
  const PrepareJob j = prepare_job(ws, kp, w, ldw, d, k, coef_cap, extras);
  hipLaunchKernelGGL(prepare_solve_kernel, dim3(j.gx, j.gy), dim3(32, 8), 0, stream, j);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

// lr = LASSO_LR_AUTO on the fused shapes: the Lipschitz launches and the prepare launch of the solve as ONE sequence --
// the prepare blocks ride in the Gram launch of the Lipschitz computation (both read only W), and the launch that
// finishes lambda_max leaves {lr, alpha lr} itself: one launch less on an EM step's dependent chain (round 6)
int prepare_with_lipschitz(const Workspace& ws, int kp, const float* w, int64_t ldw, int64_t d, int64_t k, int coef_cap,
                           hipStream_t stream, const PrepareExtras& extras, void* lip_ws) {
  PrepareExtras x = extras;
  const LipLr lr{x.lr_slot, x.alpha};
  x.lip = nullptr; x.lr_slot = nullptr;               // (the step size is the Lipschitz launches' business now)
  const PrepareJob j = prepare_job(ws, kp, w, ldw, d, k, coef_cap, &x);
  bool fused = false;
  LASSO_HIP_TRY(launch_lipschitz(w, ldw, d, k, lip_ws, 20, stream, &j, &fused, lr));
  if (!fused) {
    hipLaunchKernelGGL(prepare_solve_kernel, dim3(j.gx, j.gy), dim3(32, 8), 0, stream, j);
    LASSO_HIP_TRY(hipGetLastError());
  }
  return LASSO_OK;
}


// ---------------------------------------------------------------------------
// backtracking driver (ista.py:17-54 + the outer loop :79-102)
// ---------------------------------------------------------------------------
constexpr int kBtFinishGrid = 1024;
constexpr int kBtBatch = 8;          // trials enqueued per host round trip
constexpr int kBtMaxTrials = 1000;   // ista.py:17 (maxiter=1000)

struct BtWorkspace {
  float* wp; float* wtp; float* partials; float* dpart; float* delta; int* flags; float* fvals;
  float* partsM;   // [kBtMultiMax][4][ntiles] tile sums of the trials of a multi-trial launch (fp32 tensors)
  float* dtile;    // [ntiles] sum |z - z_next| per tile of bt_iter_kernel's accept step
  double* sums;    // [kBtMaxTrials][5] per-trial sums of a row-sharded solve
  float* G; float* C; float* Y;
  float* Zf;       // bf16 tensors: fp32 working copy of z
  // persistent bf16 solve (bt16_persist.hip)
  void* pG;        // [ntiles64 * 64][kp] bf16 gradient
  void* pZ0;       // [n][k] bf16 copy of z0 when it aliases z_out (a fall-back needs it intact)
  float* pcoef;    // [maxiter] momentum coefficients (+ [maxiter] zeros)
  void* pgran;     // trial granules + |dz| granules
  int* pout;       // [4]
  int* ptrials; float* plrs; float* pfvals;   // [maxiter] each
  int* rtrials; float* rlrs; float* rfs;      // [maxiter] each: record of a multi-launch solve enqueued without host waits
  int* ctl;                                   // its control words (bt_iter_end_kernel)
  float* rrec;                                // [maxiter][4] the same record, one 16-byte entry per iteration (bt_iter_decide_kernel)
  size_t bytes;
};

BtWorkspace carve_bt(void* base, int64_t n, int64_t k, int kp, bool half = false, int maxiter = 0) {
  BtWorkspace w;
  Arena a(base);
  const int64_t ntiles = (n + kTileM - 1) / kTileM;
  w.wp = a.take((size_t)kFistaD * kp * 4);
  w.wtp = a.take((size_t)kp * kFistaD * 4);
  w.partials = a.take((size_t)5 * std::max<int64_t>(ntiles, 1) * 4);
  w.partsM = a.take((size_t)kBtMultiMax * 4 * std::max<int64_t>(ntiles, 1) * 4);
  w.dpart = a.take((size_t)kBtFinishGrid * 4);
  w.dtile = a.take((size_t)std::max<int64_t>(ntiles, 1) * 4);
  w.delta = a.take(256);
  w.flags = a.take<int>(256);
  w.fvals = a.take(256);
  w.sums = a.take<double>((size_t)kBtMaxTrials * 5 * sizeof(double));
  w.G = a.take((size_t)n * k * 4);
  w.C = a.take((size_t)n * k * 4);
  w.Y = a.take((size_t)n * k * 4);
  w.Zf = half ? a.take((size_t)n * k * 4) : nullptr;      // (wp / wtp hold the two bf16 packs then)
  w.pG = w.pZ0 = w.pgran = nullptr; w.pcoef = nullptr; w.pout = nullptr; w.ptrials = nullptr; w.plrs = w.pfvals = nullptr;
  if (half) {
    const int64_t nt64 = (n + 63) / 64;
    const int cap = std::max(maxiter, 1);
    w.pG = a.take((size_t)nt64 * 64 * kp * 2);
    w.pZ0 = a.take((size_t)n * k * 2);
    w.pcoef = a.take((size_t)cap * 4 * 2);
    w.pgran = a.take(bt16_persist_granule_bytes((int)std::max<int64_t>(nt64, 1)));
    w.pout = a.take<int>(256);
    w.ptrials = a.take<int>((size_t)cap * 4);
    w.plrs = a.take((size_t)cap * 4);
    w.pfvals = a.take((size_t)cap * 4);
  }
  {   // line search enqueued without host waits: the per-iteration record and the control words
    const int cap = std::max(maxiter, 1);
    w.rtrials = a.take<int>((size_t)cap * 4);
    w.rlrs = a.take((size_t)cap * 4);
    w.rfs = a.take((size_t)cap * 4);
    w.ctl = a.take<int>(256);
    w.rrec = a.take((size_t)cap * 16);
  }
  w.bytes = a.bytes();
  return w;
}

// Persistent single-launch solve on bf16 tensors (bt16_persist.hip), fixed step or line search.
// Returns LASSO_OK / LASSO_WARN_LINESEARCH when it ran; `*ran` false when it does not apply (more
// tiles than resident workgroups) or the kernel gave up (a workgroup was not resident): the caller
// then takes the multi-launch path.
int solve_bf16_persistent(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                          int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int kp,
                          double alpha, double lr, int fast, int maxiter, double tol, int backtrack, double eta,
                          int32_t* iters_out, float* last_delta_out, int32_t* trials_out, float* accepted_lr_out,
                          float* accepted_f_out, void* workspace, size_t ws_bytes, hipStream_t st, bool* ran,
                          const void** z0_for_fallback) {
  *ran = false;
  *z0_for_fallback = z0_dev;
  BtWorkspace ws = carve_bt(workspace, n, k, kp, true, maxiter);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  const int ntiles = (int)((n + 63) / 64);
  int per_cu = 0;
  if (bt16_persist_occupancy(kp, &per_cu) != hipSuccess) return LASSO_OK;
  if (ntiles > per_cu * device_cus()) return LASSO_OK;            // not all tiles resident: multi-launch path
  LASSO_HIP_TRY(launch_pack_w_bf16(w_dev, ldw, (int)d, (int)k, kp, 1, ws.wp, ws.wtp, st));
  hipLaunchKernelGGL(momentum_table_kernel, dim3(1), dim3(64), 0, st, ws.pcoef, ws.pcoef + std::max(maxiter, 1),
                     std::max(maxiter, 1));
  LASSO_HIP_TRY(hipGetLastError());
  const void* z0 = z0_dev;
  if (z0_dev && z0_dev == z_out_dev) {      // in place: keep the start for a fall-back run
    LASSO_HIP_TRY(hipMemcpy2DAsync(ws.pZ0, k * 2, z0_dev, ldz0 * 2, k * 2, n, hipMemcpyDeviceToDevice, st));
    *z0_for_fallback = ws.pZ0;
  }
  LASSO_HIP_TRY(hipMemsetAsync(ws.pgran, 0, bt16_persist_granule_bytes(ntiles), st));
  LASSO_HIP_TRY(hipMemsetAsync(ws.pout, 0, 16, st));
  Bt16PersistParams p;
  p.X = x_dev; p.ldx = ldx; p.Wq1 = ws.wp; p.Wq2 = ws.wtp;
  p.Z0 = z0; p.ldz0 = ldz0; p.Z = z_out_dev; p.ldz = ldz; p.G = ws.pG;
  p.n = (int)n; p.d = (int)d; p.k = (int)k; p.ntiles = ntiles;
  p.maxiter = maxiter; p.fast = fast; p.backtrack = backtrack;
  p.alpha = alpha; p.lr0 = lr; p.eta = eta;
  p.budget = tol > 0.0 ? stop_budget<float>(n, k, tol) : -1.0f;
  p.coef = ws.pcoef;
  p.gran = ws.pgran;
  p.dgran = reinterpret_cast<unsigned long long*>((char*)ws.pgran + (size_t)8 * ntiles * 32);
  p.out = ws.pout;
  p.trials = ws.ptrials; p.lrs = ws.plrs; p.fvals = ws.pfvals;
  LASSO_HIP_TRY(launch_bt16_persist(p, kp, st));
  StopWords words;
  if (int s = read_stop_words(ws.pout, st, &words)) return s;
  if (words.redo()) {                              // some workgroup was not resident: nothing usable was produced
    if (z0_dev && z0_dev == z_out_dev) {
      // z_out was updated in place by the iterations that did complete: restore the start
      LASSO_HIP_TRY(hipMemcpy2DAsync(z_out_dev, ldz * 2, ws.pZ0, k * 2, k * 2, n, hipMemcpyDeviceToDevice, st));
    }
    return LASSO_OK;
  }
  *ran = true;
  const int its = words.iterations();
  if (iters_out) *iters_out = its;
  if (last_delta_out) *last_delta_out = words.last_delta();
  if (backtrack && its > 0 && (trials_out || accepted_lr_out || accepted_f_out)) {
    if (accepted_f_out) LASSO_HIP_TRY(hipMemcpy(accepted_f_out, ws.pfvals, (size_t)its * 4, hipMemcpyDeviceToHost));
    if (trials_out) LASSO_HIP_TRY(hipMemcpy(trials_out, ws.ptrials, (size_t)its * 4, hipMemcpyDeviceToHost));
    if (accepted_lr_out) LASSO_HIP_TRY(hipMemcpy(accepted_lr_out, ws.plrs, (size_t)its * 4, hipMemcpyDeviceToHost));
  }
  return words.warned() ? fail(LASSO_WARN_LINESEARCH, "backtracking line search failed; reverted to lr0") : LASSO_OK;
}

// The start of a solve (ista.py:76-78): z = z0 in zout -- left alone where z0 IS zout, zeros without a z0 -- and then
// y = z in Y (nullable: the caller has no y, or fills it from elsewhere).
int seed_state(const float* z0, int64_t ldz0, float* zout, int64_t ldz, float* Y, int64_t n, int64_t k, hipStream_t st) {
  if (!z0) LASSO_HIP_TRY(hipMemset2DAsync(zout, ldz * 4, 0, k * 4, n, st));
  else if (z0 != zout) LASSO_HIP_TRY(hipMemcpy2DAsync(zout, ldz * 4, z0, ldz0 * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
  if (Y) LASSO_HIP_TRY(hipMemcpy2DAsync(Y, k * 4, zout, ldz * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
  return LASSO_OK;
}

struct BtTrace {             // the caller's per-iteration trace of a line search (each array nullable)
  int32_t* trials; float* lr; float* f;
  void record(int it, int ntrials, float lr_acc, float f_acc) const {
    if (trials) trials[it] = ntrials;      // trials evaluated up to the accepted one
    if (lr) lr[it] = lr_acc;               // the step the iteration used (ista.py:40,52)
    if (f) f[it] = f_acc;                  // F(z_next) of the accepted trial (:28)
  }
};
// The words bt_decide_kernel leaves in flags / fvals, decided on the host instead: a row shard, whose sums the caller's
// callback has added over the ranks -- same float arithmetic (line_search_verdict<float>), same outcome on every rank.
struct HostDecision {
  int flags[4] = {0, 0, 0, 0}; float fvals[4] = {0.f, 0.f, 0.f, 0.f};
  void take(const double* sums, double alpha, double lr_t, int idx, bool force) {
    const LineSearchVerdict<float> v = line_search_verdict<float>(sums, alpha, lr_t, force);
    fvals[0] = v.F; fvals[1] = v.Q; flags[1] = idx + 1;
    if (v.accepted) { flags[0] = 1; flags[2] = idx; fvals[2] = (float)lr_t; fvals[3] = (float)(alpha * lr_t); }
  }
  int upload(int* flags_dev, float* fvals_dev, hipStream_t st) const {
    LASSO_HIP_TRY(hipMemcpyAsync(flags_dev, flags, sizeof(flags), hipMemcpyHostToDevice, st));
    LASSO_HIP_TRY(hipMemcpyAsync(fvals_dev, fvals, sizeof(fvals), hipMemcpyHostToDevice, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));     // (the words live on the caller's stack frame)
    return LASSO_OK;
  }
};

// The three ways solve_backtracking runs a solve:
//   Fused        fp32 tensors, one process, flat 16-byte-aligned state: one bt_iter launch per iteration, in windows;
//   MultiLaunch  one process, flat state otherwise (bf16 tensors, k no multiple of 4, the A/B knobs bt_hint & 1: one trial
//                per launch, bt_hint & 2: round 4's form): gradient, trials and accept as separate launches, in windows;
//   Sync         a row shard (the decisions need the other ranks' sums) or a strided z_out: iteration by iteration, the
//                host reads every decision.  Also the one iteration of a window whose search ran out of trials.
enum class BtForm { Fused, MultiLaunch, Sync };
enum class BtWindowEnd { RanThrough = 0, StopRule = 1, OutOfTrials = 2 };   // ctl[0] of the kernels that close an iteration
constexpr int kBtWindow = 16;
constexpr int kBtFirst = 5;          // trials of the first multi-trial launch of an iteration

struct BtSolve {
  // geometry and constants of the solve
  BtWorkspace ws;
  BtParams p;                // P / ldp: the point, y (fast) or z itself
  bool half;                 // bf16 tensors: bt_bf16.hip kernels, 64-row tiles, state in ws.Zf
  bool multi_trials;         // MultiLaunch: the trials of a batch as bt_trials_kernel launches (fp32, flat aligned state)
  bool recompute;            // candidates stay on chip, the finish kernel recomputes the accepted one
  bool zero_in_kernel;       // Fused with an all-zero start: the first launch writes the zeros of z and y itself
  int kp, grid, fast, maxiter;
  float* zout; int64_t ldz, nk;
  double alpha, lr0, eta;
  float stop_budget;         // n k tol (ista.py:64, over all ranks), -1 without the stop rule: no sum |dz| >= 0 is below it
  BtTrace trace; lasso_allreduce_fn reduce; void* reduce_ctx; hipStream_t st;
  // running state
  int it = 0, prev_trials = kBtBatch - 1;
  Momentum mom;              // ista.py:78
  float last = NAN; bool warned = false;
};

// One trial of a search at step lr_t (bf16 tensors: the trial and its decision are two launches).
int launch_trial(const BtSolve& c, const BtParams& p, double lr_t, int idx, int force, double* sums_dev) {
  if (c.half) LASSO_HIP_TRY(launch_bt16_trial(p, c.kp, c.grid, (float)lr_t, (float)(c.alpha * lr_t), force, c.st));
  LASSO_HIP_TRY(c.half ? launch_bt_decide(p, c.alpha, lr_t, idx, force, c.st, sums_dev)
                       : launch_bt_trial(p, c.kp, c.grid, c.alpha, lr_t, idx, force, c.st, sums_dev));
  return LASSO_OK;
}

// The end of a window: its control words -- and, `hrec` given, the fused form's per-iteration records, a second small
// copy -- with ONE wait.  Says how the window ended and moves c.it (StopRule: the iteration the rule fired at, :93-95),
// c.last and c.mom over the iterations it completed.
int window_wait(BtSolve& c, int win0, int wlen, float* hrec, BtWindowEnd* end) {
  int hctl[4] = {0, 0, 0, 0};
  LASSO_HIP_TRY(hipMemcpyAsync(hctl, c.ws.ctl, sizeof(hctl), hipMemcpyDeviceToHost, c.st));
  if (hrec) LASSO_HIP_TRY(hipMemcpyAsync(hrec, c.ws.rrec + 4 * (size_t)win0, (size_t)wlen * 16, hipMemcpyDeviceToHost, c.st));
  LASSO_HIP_TRY(hipStreamSynchronize(c.st));
  *end = (BtWindowEnd)hctl[0];
  c.it = hctl[1] > 0 ? hctl[1] : win0;      // (ctl[1] = iterations completed, absolute; 0: none in this window)
  if (c.it > win0) memcpy(&c.last, &hctl[2], sizeof(float));
  c.mom.skip(c.it - win0);
  return LASSO_OK;
}

// The whole solve is enqueued WITHOUT a host wait, in WINDOWS of kBtWindow outer iterations (all `maxiter`
// iterations at once meant ~19 launches per remaining iteration of empty work after the rule fired -- maxiter = 1000
// stopping at 20: ~19k no-op launches): once the stop rule fired on the device -- or a search needed more trials than
// were enqueued -- the window's remaining launches are no-ops (*skip != 0).  The control words are read between windows;
// a search that ran out of trials takes ONE iteration_sync from the untouched state of the iteration that needed them.
// Round 5, fp32 tensors: ONE launch per outer iteration (bt_iter.hip: the accept step of the previous iteration, the
// gradient and the first `n_first` trials per tile) + ONE decision launch that also closes the previous iteration;
// decisions live in per-iteration slots of ws.flags / ws.fvals (kBtWindow slots of 4 words).  The trials beyond
// n_first (old kernel, p and g re-read) are enqueued only after a search of THIS solve has run out of trials once
// (`safety`); until then such a search costs one synchronous iteration.
int window_fused(BtSolve& c, int& n_first_next, bool& safety, BtWindowEnd* end) {
  const BtWorkspace& ws = c.ws; hipStream_t st = c.st;
  const int win0 = c.it, wlen = std::min(kBtWindow, c.maxiter - c.it), n_first = n_first_next, ntiles = c.p.ntiles;
  LASSO_HIP_TRY(hipMemsetAsync(ws.flags, 0, (size_t)kBtWindow * 4 * sizeof(int), st));
  LASSO_HIP_TRY(hipMemsetAsync(ws.ctl, 0, 4 * sizeof(int), st));
  BtIterParams q;
  q.X = c.p.X; q.ldx = c.p.ldx; q.Wp = ws.wp; q.Wtp = ws.wtp; q.Z = c.zout; q.Y = ws.Y; q.G = ws.G;
  q.partials = ws.partials; q.partsM = ws.partsM; q.dpart = ws.dtile; q.skip = ws.ctl;
  q.n = c.p.n; q.d = c.p.d; q.k = c.p.k; q.ntiles = ntiles; q.fast = c.fast ? 1 : 0;
  q.zero_start = (c.zero_in_kernel && c.it == 0) ? 1 : 0;
  const float stop_budget = c.stop_budget;
  Momentum mom = c.mom;
  float coef_prev = 0.0f;
  BtSteps steps;
  for (int i = win0; i < win0 + wlen; ++i) {
    const float coef = mom.next(c.fast);                                             // :98-99
    const int slot = i - win0;
    int* const cur_flags = ws.flags + 4 * slot;
    float* const cur_fvals = ws.fvals + 4 * slot;
    const int* const prev_flags = slot > 0 ? ws.flags + 4 * (slot - 1) : nullptr;
    const float* const prev_fvals = slot > 0 ? ws.fvals + 4 * (slot - 1) : nullptr;
    StepLadder ladder{c.lr0, c.eta, c.alpha};
    ladder.fill(steps, n_first);                                                     // :47
    q.acc_flags = prev_flags; q.acc_fvals = prev_fvals; q.coef = coef_prev; q.tail = 0; q.ntrials = n_first;
    LASSO_HIP_TRY(launch_bt_iter(q, steps, c.kp, c.grid, st));
    const bool more = safety && n_first < kBtBatch;
    LASSO_HIP_TRY(launch_bt_iter_decide(ws.partials, ws.partsM, ntiles, c.alpha, steps, n_first, 0, more ? 0 : 1, cur_flags,
                                        cur_fvals, prev_flags, prev_fvals, ws.dtile, i - 1, stop_budget, ws.ctl,
                                        ws.rrec, st));
    if (more) {
      BtSteps rest;
      const int nb = kBtBatch - n_first;
      ladder.fill(rest, nb);
      BtParams pb = c.p;
      pb.flags = cur_flags; pb.fvals = cur_fvals; pb.skip = ws.ctl;
      LASSO_HIP_TRY(launch_bt_trials_only(pb, c.kp, c.grid, rest, nb, ws.partsM, st));
      LASSO_HIP_TRY(launch_bt_iter_decide(ws.partials, ws.partsM, ntiles, c.alpha, rest, nb, n_first, 1, cur_flags,
                                          cur_fvals, nullptr, nullptr, nullptr, 0, -1.0f, ws.ctl, ws.rrec, st));
    }
    coef_prev = coef;
  }
  {   // the accept step of the window's last iteration, and its record
    const int slot = wlen - 1;
    q.acc_flags = ws.flags + 4 * slot; q.acc_fvals = ws.fvals + 4 * slot; q.coef = coef_prev; q.tail = 1; q.ntrials = 0;
    LASSO_HIP_TRY(launch_bt_iter(q, steps, c.kp, c.grid, st));
    LASSO_HIP_TRY(launch_bt_iter_decide(ws.partials, ws.partsM, ntiles, c.alpha, steps, 0, 0, 0, nullptr, nullptr,
                                        ws.flags + 4 * slot, ws.fvals + 4 * slot, ws.dtile, win0 + wlen - 1,
                                        stop_budget, ws.ctl, ws.rrec, st));
  }
  float hrec[kBtWindow * 4];
  if (int s = window_wait(c, win0, wlen, hrec, end)) return s;
  if (c.it > win0) {
    int most = 1;
    for (int i = 0; i < c.it - win0; ++i) {
      int tr;
      memcpy(&tr, &hrec[4 * i], sizeof(int));
      c.trace.record(win0 + i, tr, hrec[4 * i + 1], hrec[4 * i + 2]);
      most = std::max(most, tr);
      c.prev_trials = tr;
    }
    // the next window computes as many trials per tile as this one's longest search took (every computed trial costs
    // its GEMM whether it is needed or not; a search that outgrows the guess costs one synchronous iteration)
    n_first_next = std::min(kBtBatch, std::max(2, most));
    // a whole window without a search beyond its first batch: the second trial batch and its decision leave the
    // windows again (two launches per iteration that did nothing; ADVICE r05: `safety` was never cleared)
    if (*end != BtWindowEnd::OutOfTrials && most <= n_first) safety = false;
  }
  if (*end == BtWindowEnd::OutOfTrials) safety = true;
  return LASSO_OK;
}

// A window of the multi-launch form (see window_fused for the windows): every outer iteration is the gradient,
// kBtBatch trial launches with the step sequence lr0 / eta^t (a trial behind the accepted one returns at once), the
// accept step and a one-block kernel that keeps the iteration's record and evaluates the stop rule on the device.
int window_multi_launch(BtSolve& c, BtWindowEnd* end) {
  const BtWorkspace& ws = c.ws; hipStream_t st = c.st;
  const int win0 = c.it, wlen = std::min(kBtWindow, c.maxiter - c.it);
  LASSO_HIP_TRY(hipMemsetAsync(ws.flags, 0, 4 * sizeof(int), st));
  LASSO_HIP_TRY(hipMemsetAsync(ws.ctl, 0, 4 * sizeof(int), st));
  BtParams p = c.p;
  p.skip = ws.ctl;
  Momentum mom = c.mom;
  for (int i = win0; i < win0 + wlen; ++i) {
    const float coef = mom.next(c.fast);                                             // :98-99
    LASSO_HIP_TRY(c.half ? launch_bt16_grad(p, c.kp, c.grid, st) : launch_bt_grad(p, c.kp, c.grid, st));
    StepLadder ladder{c.lr0, c.eta, c.alpha};
    if (c.multi_trials) {
      // fp32 tensors: the kBtBatch pre-enqueued trials as TWO launches -- trials 0 .. kBtFirst-1 (p and g of a tile
      // read once, in registers for all of them) and the rest (a no-op once a trial of the first launch passed)
      for (int b0 = 0; b0 < kBtBatch; b0 += kBtFirst) {
        BtSteps steps;
        const int nb = std::min(kBtFirst, kBtBatch - b0);
        ladder.fill(steps, nb);                                                      // :47
        LASSO_HIP_TRY(launch_bt_trials(p, c.kp, c.grid, c.alpha, steps, nb, b0, ws.partsM, st));
      }
    } else {
      for (int b = 0; b < kBtBatch; ++b, ladder.descend())                           // :47
        if (int s = launch_trial(c, p, ladder.lr, b, 0, nullptr)) return s;
    }
    LASSO_HIP_TRY(launch_bt_finish_recompute(c.zout, ws.Y, p.P, ws.G, c.nk, coef, ws.flags, ws.fvals, ws.dpart,
                                             kBtFinishGrid, st, ws.ctl));
    LASSO_HIP_TRY(launch_bt_iter_end(ws.dpart, kBtFinishGrid, ws.flags, ws.fvals, ws.ctl, i, c.stop_budget, ws.rtrials,
                                     ws.rlrs, ws.rfs, st));
  }
  if (int s = window_wait(c, win0, wlen, nullptr, end)) return s;
  if (c.it > win0) {
    const int cnt = c.it - win0;
    std::vector<int> ht(cnt);
    std::vector<float> hl(cnt), hf(cnt);
    LASSO_HIP_TRY(hipMemcpy(ht.data(), ws.rtrials + win0, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    LASSO_HIP_TRY(hipMemcpy(hl.data(), ws.rlrs + win0, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    LASSO_HIP_TRY(hipMemcpy(hf.data(), ws.rfs + win0, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < cnt; ++i) c.trace.record(win0 + i, ht[i], hl[i], hf[i]);
    c.prev_trials = ht[cnt - 1];
  }
  return LASSO_OK;
}

// One outer iteration with the host in the loop: the trials are enqueued in batches and the host reads the decision
// behind each batch.  On a row shard (c.reduce) the sums behind the two global decisions of an iteration -- F <= Q of
// every trial (ista.py:23,28,32-35) and sum |z_next - z| <= n k tol (:93) -- are added over the ranks by the caller's
// callback; every rank then takes the same decision from the same numbers.  *stop: the stop rule fired (:93-95).
int iteration_sync(BtSolve& c, bool* stop) {
  const BtWorkspace& ws = c.ws; const BtParams& p = c.p; hipStream_t st = c.st;
  const float coef = c.mom.next(c.fast);                                             // :98-99
  LASSO_HIP_TRY(hipMemsetAsync(ws.flags, 0, 4 * sizeof(int), st));
  LASSO_HIP_TRY(c.half ? launch_bt16_grad(p, c.kp, c.grid, st) : launch_bt_grad(p, c.kp, c.grid, st));
  StepLadder ladder{c.lr0, c.eta, c.alpha};
  struct { int flags[4]; float fvals[4]; float delta; } host = {{0, 0, 0, 0}, {0.f, 0.f, 0.f, 0.f}, 0.f};
  int t = 0; bool accepted = false;
  while (!accepted) {
    const bool give_up = t >= kBtMaxTrials;
    // the first batch of an iteration is sized from the previous iteration's trial count
    // (trials enqueued after the accepted one only cost their launch, but that adds up)
    const int want = t == 0 ? std::min(kBtBatch, std::max(2, c.prev_trials + 1)) : kBtBatch / 2;
    const int batch = give_up ? 1 : std::min(want, kBtMaxTrials - t), force = give_up ? 1 : 0;
    double lr_batch[kBtBatch];
    for (int b = 0; b < batch; ++b) {
      const double lr_t = give_up ? c.lr0 : ladder.lr;      // ista.py:48-52: warn and revert to the initial step size
      lr_batch[b] = lr_t;
      if (int s = launch_trial(c, p, lr_t, t + b, force, c.reduce ? ws.sums + 5 * b : nullptr)) return s;
      if (give_up) c.warned = true;
      else ladder.descend();                                                         // :47
    }
    if (c.reduce) {
      // the batch's sums: all ranks add theirs, then the decision of bt_decide_kernel on the host, trial by trial in order
      double hsums[kBtBatch * 5];
      LASSO_HIP_TRY(hipMemcpyAsync(hsums, ws.sums, (size_t)batch * 5 * sizeof(double), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
      if (c.reduce(c.reduce_ctx, hsums, batch * 5) != 0) return fail(LASSO_ERR_HIP, "all-reduce callback failed");
      HostDecision dec;
      for (int b = 0; b < batch && !dec.flags[0]; ++b) dec.take(hsums + 5 * b, c.alpha, lr_batch[b], t + b, give_up);
      if (int s = dec.upload(ws.flags, ws.fvals, st)) return s;
    }
    t += batch;
    if (c.recompute)   // P is Y (fast) or Z itself: element-wise in place is safe either way
      LASSO_HIP_TRY(launch_bt_finish_recompute(c.zout, ws.Y, p.P, ws.G, c.nk, coef, ws.flags, ws.fvals, ws.dpart,
                                               kBtFinishGrid, st));
    else
      LASSO_HIP_TRY(launch_bt_finish(c.zout, c.ldz, ws.Y, ws.C, p.n, p.k, coef, ws.flags, ws.dpart, kBtFinishGrid, st));
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, kBtFinishGrid, ws.delta);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(hipMemcpyAsync(host.flags, ws.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipMemcpyAsync(&host.delta, ws.delta, sizeof(float), hipMemcpyDeviceToHost, st));
    if (c.trace.lr || c.trace.f)
      LASSO_HIP_TRY(hipMemcpyAsync(host.fvals, ws.fvals, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    accepted = host.flags[0] != 0;
  }
  if (c.reduce) {                                    // sum |z_next - z| over all ranks (:93)
    double dsum = (double)host.delta;
    if (c.reduce(c.reduce_ctx, &dsum, 1) != 0) return fail(LASSO_ERR_HIP, "all-reduce callback failed");
    host.delta = (float)dsum;
  }
  // (the forced step at lr0 behind kBtMaxTrials rejected trials is no trial: the reference counts 1000, ista.py:17,48-52)
  const int trials = std::min(host.flags[2] + 1, kBtMaxTrials);
  c.prev_trials = trials;
  c.trace.record(c.it, trials, host.fvals[2], host.fvals[0]);
  c.last = host.delta;
  ++c.it;
  *stop = host.delta <= c.stop_budget;                                               // :93-95
  return LASSO_OK;
}

int solve_backtracking(const void* x_any, int64_t ldx, const void* w_any, int64_t ldw, const void* z0_any,
                       int64_t ldz0, void* zout_any, int64_t ldz_any, int64_t n, int64_t d, int64_t k, int kp,
                       int dtype, double alpha, double lr0, int fast, int maxiter, double tol, double eta,
                       int32_t* iters_out, float* last_delta_out, int32_t* trials_out, float* accepted_lr_out,
                       float* accepted_f_out, void* workspace, size_t ws_bytes, hipStream_t st,
                       lasso_allreduce_fn reduce = nullptr, void* reduce_ctx = nullptr, int64_t n_global = 0,
                       int bt_hint = 0 /* 1: single-trial launches also for fp32 tensors (A/B); 2: the multi-launch form */) {
  // ---- validate and carve.  reduce != nullptr: this process holds a row shard (iteration_sync)
  BtSolve c;
  const bool half = dtype == LASSO_BF16;      // bf16 tensors: bt_bf16.hip kernels, 64-row tiles
  c.ws = carve_bt(workspace, n, k, kp, half, maxiter);
  const BtWorkspace& ws = c.ws;
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  const int cus = device_cus();
  if (cus <= 0) return fail(LASSO_ERR_HIP, "no HIP device");
  const int tile_rows = half ? 64 : kTileM, ntiles = (int)((n + tile_rows - 1) / tile_rows);
  float* zout = half ? ws.Zf : (float*)zout_any;
  const int64_t ldz = half ? k : ldz_any;
  const bool recompute = half || ldz == k;     // a flat [n][k] state: always for bf16 tensors; fp32: unless z_out is strided
  // ---- the form, chosen once (BtForm).  The multi-trial and one-launch-per-iteration kernels take fp32 tensors with a flat
  // 16-byte-aligned point and gradient (flat: ldz == k, so a row pitch that is no multiple of 4 floats never reaches them)
  const bool flat16 = !half && recompute && (k & 3) == 0 && k >= 4 && (((uintptr_t)zout) & 15) == 0 &&
                      (((uintptr_t)ws.Y) & 15) == 0 && (((uintptr_t)ws.G) & 15) == 0;
  const BtForm form = (reduce || !recompute) ? BtForm::Sync : (flat16 && !(bt_hint & 3)) ? BtForm::Fused : BtForm::MultiLaunch;
  c.half = half; c.recompute = recompute; c.multi_trials = flat16 && !(bt_hint & 1);
  c.zero_in_kernel = form == BtForm::Fused && !z0_any && maxiter > 0;
  // (refused before the first launch: z_out is not touched)
  if (reduce && !recompute) return fail(LASSO_ERR_UNSUPPORTED, "row-sharded line search needs ldz == k");
  // ---- pack W and seed the state: z lives in zout, y in the workspace (y0 = z0, ista.py:76-78)
  if (half) {
    LASSO_HIP_TRY(launch_pack_w_bf16(w_any, ldw, (int)d, (int)k, kp, 1, ws.wp, ws.wtp, st));
    if (z0_any) LASSO_HIP_TRY(launch_cvt_bf16(z0_any, ldz0, zout, k, (int)n, (int)k, 1, st));
    else LASSO_HIP_TRY(hipMemsetAsync(zout, 0, (size_t)n * k * 4, st));
    LASSO_HIP_TRY(hipMemcpy2DAsync(ws.Y, k * 4, zout, ldz * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
  } else {
    hipLaunchKernelGGL(pack_w_kernel, dim3(kp / 32, kFistaD / 32), dim3(32, 8), 0, st, (const float*)w_any, ldw,
                       (int)d, (int)k, kp, ws.wp, ws.wtp);
    LASSO_HIP_TRY(hipGetLastError());
    if (!c.zero_in_kernel)
      if (int s = seed_state((const float*)z0_any, ldz0, zout, ldz, ws.Y, n, k, st)) return s;
  }
  BtParams& p = c.p;
  p.X = (const float*)x_any; p.ldx = ldx; p.Wp = ws.wp; p.Wtp = ws.wtp;
  p.Xh = x_any; p.Wq1 = ws.wp; p.Wq2 = ws.wtp;
  p.P = fast ? ws.Y : zout; p.ldp = fast ? k : ldz;
  p.G = ws.G; p.C = recompute ? nullptr : ws.C; p.partials = ws.partials; p.flags = ws.flags; p.fvals = ws.fvals;
  p.n = (int)n; p.d = (int)d; p.k = (int)k; p.ntiles = ntiles; p.skip = nullptr;
  c.kp = kp; c.grid = std::min(ntiles, cus); c.fast = fast; c.maxiter = maxiter; c.zout = zout; c.ldz = ldz; c.nk = n * k;
  c.alpha = alpha; c.lr0 = lr0; c.eta = eta; c.reduce = reduce; c.reduce_ctx = reduce_ctx; c.st = st;
  c.stop_budget = tol > 0.0 ? stop_budget<float>(reduce ? n_global : n, k, tol) : -1.0f;
  c.trace = {trials_out, accepted_lr_out, accepted_f_out};
  // ---- run a window; one whose search ran out of trials is followed by that one iteration on the synchronous path
  int n_first = kBtFirst; bool safety = false;
  while (c.it < maxiter) {
    if (form != BtForm::Sync) {
      BtWindowEnd end;
      if (int s = form == BtForm::Fused ? window_fused(c, n_first, safety, &end) : window_multi_launch(c, &end)) return s;
      if (end == BtWindowEnd::StopRule) break;
      if (end != BtWindowEnd::OutOfTrials) continue;
    }
    bool stop = false;
    if (int s = iteration_sync(c, &stop)) return s;
    if (stop) break;
  }
  if (half) LASSO_HIP_TRY(launch_cvt_bf16(zout, k, zout_any, ldz_any, (int)n, (int)k, 0, st));
  if (iters_out) *iters_out = c.it;
  if (last_delta_out) *last_delta_out = c.last;
  return c.warned ? fail(LASSO_WARN_LINESEARCH, "backtracking line search failed; reverted to lr0") : LASSO_OK;
}


// ---------------------------------------------------------------------------
// Fixed-step solve on bf16 tensors: the bf16-MFMA gradient kernel of the line search
// (bt_bf16.hip: g = (y W^T - x) W, bf16 operands, fp32 accumulation) + the fp32
// prox/momentum pass, state in fp32 -- no up-converted copies of x and W, and at large n
// faster than the fp32 fused kernel fed such copies.  The stop rule is evaluated on the host
// once per iteration like the reference does (ista.py:93).
// ---------------------------------------------------------------------------
int solve_fixed_bf16(const void* x_any, int64_t ldx, const void* w_any, int64_t ldw, const void* z0_any,
                     int64_t ldz0, void* zout_any, int64_t ldz_any, int64_t n, int64_t d, int64_t k, int kp,
                     double alpha, double lr, int fast, int maxiter, double tol, int32_t* iters_out,
                     float* last_delta_out, void* workspace, size_t ws_bytes, hipStream_t st) {
  BtWorkspace ws = carve_bt(workspace, n, k, kp, true);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  const int cus = device_cus();
  if (cus <= 0) return fail(LASSO_ERR_HIP, "no HIP device");
  const int ntiles = (int)((n + 63) / 64);
  float* Z = ws.Zf;
  LASSO_HIP_TRY(launch_pack_w_bf16(w_any, ldw, (int)d, (int)k, kp, 1, ws.wp, ws.wtp, st));
  if (z0_any) LASSO_HIP_TRY(launch_cvt_bf16(z0_any, ldz0, Z, k, (int)n, (int)k, 1, st));
  else LASSO_HIP_TRY(hipMemsetAsync(Z, 0, (size_t)n * k * 4, st));
  LASSO_HIP_TRY(hipMemcpyAsync(ws.Y, Z, (size_t)n * k * 4, hipMemcpyDeviceToDevice, st));
  BtParams p;
  p.X = nullptr; p.ldx = ldx; p.Wp = ws.wp; p.Wtp = ws.wtp;
  p.skip = nullptr;
  p.Xh = x_any; p.Wq1 = ws.wp; p.Wq2 = ws.wtp;
  p.G = ws.G; p.C = nullptr; p.partials = ws.partials; p.flags = ws.flags; p.fvals = ws.fvals;
  p.n = (int)n; p.d = (int)d; p.k = (int)k; p.ntiles = ntiles;
  const float budget = stop_budget<float>(n, k, tol);
  const float lr_f = (float)lr, lam = (float)(alpha * lr);
  Momentum mom;
  float last = NAN;
  int it = 0;
  for (; it < maxiter; ++it) {
    const float coef = mom.next(fast);
    p.P = ws.Y; p.ldp = k;                    // ISTA: coef = 0 keeps y == z
    LASSO_HIP_TRY(launch_bt16_grad(p, kp, std::min(ntiles, cus), st));
    LASSO_HIP_TRY(launch_generic_prox(Z, k, ws.Y, ws.G, (int)n, (int)k, lr_f, lam, coef, ws.dpart, kBtFinishGrid, st));
    if (tol > 0.0) {
      hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, kBtFinishGrid, ws.delta);
      LASSO_HIP_TRY(hipGetLastError());
      LASSO_HIP_TRY(hipMemcpyAsync(&last, ws.delta, sizeof(float), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
      if (last <= budget) { ++it; break; }
    }
  }
  LASSO_HIP_TRY(launch_cvt_bf16(Z, k, zout_any, ldz_any, (int)n, (int)k, 0, st));
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return LASSO_OK;
}

// ---------------------------------------------------------------------------
// Unfused path for shapes beyond the fused kernel (d > 256 or k > 1024): two MFMA GEMM
// launches + one elementwise launch per iteration, state in HBM.  Same arithmetic
// (ista.py:72-73,90,93,98-102); the stop rule is evaluated on the host every iteration
// like the reference does.  Correctness path, not tuned.
// ---------------------------------------------------------------------------
constexpr int kGenGrid = 1024;
struct GenWorkspace { float* Wt; float* Y; float* NR; float* G; float* dpart; float* delta;
                      float* C; float* part; int* flags; float* fvals;      // line search only
                      double* sums;                                         // (its five sums of a trial: row shards)
                      float* Wc;                                            // [d][k] copy of W (lasso_fista_prepare / _run)
                      float* Yc;                                            // y at the head of a speculated chunk (stop rule; z's copy lives in G)
                      size_t bytes; };

// with_state: room for y's checkpoint at the head of a speculated chunk -- only solves with a live stop rule take it
// (fixed-iteration solves paid n k words for a buffer they never touch)
GenWorkspace carve_generic(void* base, int64_t n, int64_t d, int64_t k, bool backtrack = false, bool with_state = true) {
  GenWorkspace w;
  Arena a(base);
  w.Wt = a.take((size_t)k * d * 4);
  w.Wc = a.take((size_t)d * k * 4);             // (both dictionary copies first: their place does not depend on n)
  w.Y = a.take((size_t)n * k * 4);
  w.NR = a.take((size_t)n * d * 4);
  w.G = a.take((size_t)n * k * 4);
  // per-block sums of |z - z_next|: the fused GEMM-2 + prox launch writes one per 64 x 64 (or larger) block
  w.dpart = a.take(std::max<size_t>((size_t)kGenGrid, (size_t)((n + 63) / 64) * (size_t)((k + 63) / 64)) * 4);
  w.delta = a.take(256);
  w.C = w.part = w.fvals = nullptr; w.flags = nullptr; w.sums = nullptr;
  if (backtrack) {
    w.C = a.take((size_t)n * k * 4);
    w.part = a.take((size_t)5 * kGenGrid * 4);
    w.flags = a.take<int>(256);
    w.fvals = a.take(256);
    w.sums = a.take<double>(256);
  }
  w.Yc = with_state ? a.take((size_t)n * k * 4) : nullptr;
  w.bytes = a.bytes();
  return w;
}

int solve_generic(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0,
                  float* zout, int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha, double lr,
                  int fast, int maxiter, double tol, int32_t* iters_out, float* last_delta_out,
                  void* workspace, size_t ws_bytes, hipStream_t st) {
  GenWorkspace ws = carve_generic(workspace, n, d, k, false, tol > 0.0 && maxiter > 0);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, (int)d, (int)k, ws.Wt, d, (int)k, (int)d, st));
  if (int s = seed_state(z0, ldz0, zout, ldz, ws.Y, n, k, st)) return s;
  const float budget = stop_budget<float>(n, k, tol);
  const float lr_f = (float)lr, lam = (float)(alpha * lr);
  Momentum mom;
  float last = NAN;
  int it = 0;
  const int parts = gemm_nt_prox_parts((int)n, (int)k);
  auto iterate = [&](float* delta_slot) -> int {
    const float coef = mom.next(fast);
    // NR = x - y W^T  (= -r);   G = 0 - NR Wt^T = r W
    // the gradient block g = r W never goes to memory: the proximal step runs in GEMM-2's epilogue
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.Y, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));
    LASSO_HIP_TRY(launch_gemm_nt_prox(ws.NR, d, ws.Wt, d, zout, ldz, ws.Y, k, (int)n, (int)k, (int)d, lr_f, lam, coef,
                                      ws.dpart, st));
    if (delta_slot) {
      hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, parts, delta_slot);
      LASSO_HIP_TRY(hipGetLastError());
    }
    return LASSO_OK;
  };
  if (!(tol > 0.0)) {
    for (; it < maxiter; ++it)
      if (int s = iterate(nullptr)) return s;
  } else {
    // the stop rule once per chunk of speculated iterations (speculate_stop_rule, stoprule_host.hpp; round 3: a host round trip
    // per iteration): z's checkpoint lives in G (unused since the proximal step moved into GEMM-2's epilogue), y's in Yc
    const int64_t words = n * k;
    const bool compact = ldz == k && ((uintptr_t)zout & 15) == 0;      // (else the runtime's strided copy)
    const int copy_grid = (int)std::min<int64_t>((words / 4 + 255) / 256 + 1, (int64_t)std::max(device_cus(), 1) * 16);
    auto save = [&]() -> int {
      if (compact) hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, zout, ws.G, words);
      else LASSO_HIP_TRY(hipMemcpy2DAsync(ws.G, k * 4, zout, ldz * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Y, ws.Yc, words);
      LASSO_HIP_TRY(hipGetLastError());
      return LASSO_OK;
    };
    auto restore = [&]() -> int {
      if (compact) hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.G, zout, words);
      else LASSO_HIP_TRY(hipMemcpy2DAsync(zout, ldz * 4, ws.G, k * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Yc, ws.Y, words);
      LASSO_HIP_TRY(hipGetLastError());
      return LASSO_OK;
    };
    auto read = [&](float* host, int c) -> int { return read_back(host, ws.delta, sizeof(float) * c, st); };
    if (int s = speculate_stop_rule<float>(maxiter, budget, ws.delta, &mom.t, iterate, save, restore,
                                           [] { return (int)LASSO_OK; }, read, &it, &last, "lasso_fista_solve (unfused)"))
      return s;
  }
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return LASSO_OK;
}

// `iters` iterations it0 .. of the unfused solve from a given (z, y) state: the resumable form behind
// lasso_fista_run for shapes beyond the fused kernels (traced forward pass of the autograd path,
// verbose mode).  Wt must have been prepared in the workspace (lasso_fista_prepare).
int run_generic(const float* x, int64_t ldx, const float* z_in, int64_t ldz_in,
                const float* y_in, int64_t ldy_in, float* z_out, int64_t ldz_out, float* y_out, int64_t ldy_out,
                int64_t n, int64_t d, int64_t k, double alpha, double lr, int fast, int it0, int iters, float* delta_dev,
                void* workspace, size_t ws_bytes, hipStream_t st) {
  GenWorkspace ws = carve_generic(workspace, n, d, k, false, false);   // (no stop-rule checkpoint here)
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (n == 0) return LASSO_OK;
  if (int s = seed_state(z_in, ldz_in, z_out, ldz_out, y_in ? nullptr : ws.Y, n, k, st)) return s;
  if (y_in) LASSO_HIP_TRY(hipMemcpy2DAsync(ws.Y, k * 4, y_in, ldy_in * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
  const float lr_f = (float)lr, lam = (float)(alpha * lr);
  Momentum mom;
  mom.skip(it0);
  for (int i = 0; i < iters; ++i) {
    const float coef = mom.next(fast);
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.Y, k, ws.Wc, k, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));
    LASSO_HIP_TRY(launch_gemm_nt_prox(ws.NR, d, ws.Wt, d, z_out, ldz_out, ws.Y, k, (int)n, (int)k, (int)d, lr_f, lam,
                                      coef, ws.dpart, st));
    if (delta_dev) {
      hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, gemm_nt_prox_parts((int)n, (int)k),
                         delta_dev + i);
      LASSO_HIP_TRY(hipGetLastError());
    }
  }
  if (y_out)
    LASSO_HIP_TRY(hipMemcpy2DAsync(y_out, ldy_out * 4, ws.Y, k * 4, k * 4, n, hipMemcpyDeviceToDevice, st));
  return LASSO_OK;
}

// The line search of ista.py:17-54 for shapes beyond the fused kernels: per outer iteration two
// launches of the general GEMM for the gradient at p, then per trial one element-wise launch
// (candidate + three of the sums), one GEMM (its residual), the sum of squares and the decision
// kernel of backtrack.hip, one host synchronisation per trial -- the reference's own structure on
// HIP kernels.  Correctness path, not tuned.
int solve_generic_backtracking(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0,
                               int64_t ldz0, float* zout, int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha,
                               double lr0, int fast, int maxiter, double tol, double eta, int32_t* iters_out,
                               float* last_delta_out, int32_t* trials_out, float* accepted_lr_out,
                               float* accepted_f_out, void* workspace, size_t ws_bytes, hipStream_t st,
                               lasso_allreduce_fn reduce = nullptr, void* reduce_ctx = nullptr, int64_t n_global = 0) {
  // reduce != nullptr: a row shard -- the five sums of every trial and sum|z - z+| are added over the ranks and the
  // decision of bt_decide_kernel is taken on the host, as in solve_backtracking
  GenWorkspace ws = carve_generic(workspace, n, d, k, true, false);
  if (ws_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, ws.bytes);
  if (n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  LASSO_HIP_TRY(launch_transpose_pad(w, ldw, (int)d, (int)k, ws.Wt, d, (int)k, (int)d, st));
  if (int s = seed_state(z0, ldz0, zout, ldz, ws.Y, n, k, st)) return s;
  BtParams bp;                                             // only what bt_decide_kernel reads
  bp.skip = nullptr;
  bp.partials = ws.part; bp.ntiles = kGenGrid; bp.flags = ws.flags; bp.fvals = ws.fvals;
  const float budget = stop_budget<float>(reduce ? n_global : n, k, tol);
  const BtTrace trace = {trials_out, accepted_lr_out, accepted_f_out};
  bool warned = false;
  Momentum mom;
  float last = NAN;
  int it = 0;
  for (; it < maxiter; ++it) {
    const float coef = mom.next(fast);                                                // :98-99 (ISTA: y == z)
    LASSO_HIP_TRY(hipMemsetAsync(ws.flags, 0, 4 * sizeof(int), st));
    // NR = x - p W^T (= -r0, :22);  G = r0 W (:24);  partials[0] = sum r0^2 (:23)
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.Y, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.NR, d, ws.Wt, d, nullptr, 0, ws.G, k, (int)n, (int)k, (int)d, st));
    LASSO_HIP_TRY(launch_sumsq_partials(ws.NR, n * d, ws.part, kGenGrid, st));
    StepLadder ladder{lr0, eta, alpha};
    int t = 0, accepted_at = -1;
    HostDecision host;
    for (;;) {
      const bool give_up = t >= kBtMaxTrials;
      const double lr_t = give_up ? lr0 : ladder.lr;                                    // :48-52
      LASSO_HIP_TRY(launch_generic_trial(ws.Y, ws.G, ws.C, n * k, (float)lr_t, (float)(alpha * lr_t), ws.part,
                                         kGenGrid, st));                                // :40, :31-35
      LASSO_HIP_TRY(launch_gemm_nt_sub(ws.C, k, w, ldw, x, ldx, ws.NR, d, (int)n, (int)d, (int)k, st));   // :27
      LASSO_HIP_TRY(launch_sumsq_partials(ws.NR, n * d, ws.part + kGenGrid, kGenGrid, st));
      LASSO_HIP_TRY(launch_bt_decide(bp, alpha, lr_t, t, give_up ? 1 : 0, st, reduce ? ws.sums : nullptr));   // :28, :32-35, :45
      if (reduce) {
        double hs[5];
        LASSO_HIP_TRY(hipMemcpyAsync(hs, ws.sums, sizeof(hs), hipMemcpyDeviceToHost, st));
        LASSO_HIP_TRY(hipStreamSynchronize(st));
        if (reduce(reduce_ctx, hs, 5) != 0) return fail(LASSO_ERR_HIP, "all-reduce callback failed");
        host = HostDecision();
        host.take(hs, alpha, lr_t, t, give_up);                                         // ista.py:23, :28, :32-35, :45
        if (int s = host.upload(ws.flags, ws.fvals, st)) return s;
      } else {
        LASSO_HIP_TRY(hipMemcpyAsync(host.flags, ws.flags, sizeof(host.flags), hipMemcpyDeviceToHost, st));
        LASSO_HIP_TRY(hipMemcpyAsync(host.fvals, ws.fvals, sizeof(host.fvals), hipMemcpyDeviceToHost, st));
        LASSO_HIP_TRY(hipStreamSynchronize(st));
      }
      if (give_up) warned = true;
      if (host.flags[0]) { accepted_at = t; break; }
      ladder.descend();                                                                 // :47
      ++t;
    }
    LASSO_HIP_TRY(launch_bt_finish(zout, ldz, ws.Y, ws.C, (int)n, (int)k, coef, ws.flags, ws.dpart, kGenGrid, st));
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, kGenGrid, ws.delta);
    LASSO_HIP_TRY(hipGetLastError());
    LASSO_HIP_TRY(hipMemcpyAsync(&last, ws.delta, sizeof(float), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    if (reduce) {                                    // sum |z_next - z| over all ranks (:93)
      double dsum = (double)last;
      if (reduce(reduce_ctx, &dsum, 1) != 0) return fail(LASSO_ERR_HIP, "all-reduce callback failed");
      last = (float)dsum;
    }
    trace.record(it, accepted_at + 1, host.fvals[2], host.fvals[0]);
    if (tol > 0.0 && last <= budget) { ++it; break; }                                   // :93-95
  }
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return warned ? fail(LASSO_WARN_LINESEARCH, "backtracking line search failed; reverted to lr0") : LASSO_OK;
}

// ---------------------------------------------------------------------------
// greedy coordinate descent (cd.hip): workspace = persistent per-row state
// ---------------------------------------------------------------------------
int pad_k_cd(int64_t k) {
  for (int kp = 256; kp <= 4096; kp *= 2)
    if (k <= kp) return kp;
  return -1;
}
struct CdWorkspace { float* S; float* Wt; float* B; float* Zt; int* active; int* row_steps; int* counter; int* info; size_t bytes; };

CdWorkspace carve_cd(void* base, int64_t n, int64_t d, int kp) {
  CdWorkspace w;
  Arena a(base);
  w.S = a.take((size_t)kp * kp * 4);
  w.Wt = a.take((size_t)kp * d * 4);
  w.B = a.take((size_t)n * kp * 4);
  w.Zt = a.take((size_t)n * kp * 4);
  w.active = a.take<int>((size_t)n * 4);
  w.row_steps = a.take<int>((size_t)n * 4);
  w.counter = a.take<int>(256);
  w.info = a.take<int>(256);
  w.bytes = a.bytes();
  return w;
}

int check_cd(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d: only LASSO_F32 is implemented", dtype);
  if (n < 0 || d <= 0 || k <= 0) return fail(LASSO_ERR_BAD_ARG, "bad shape n=%lld d=%lld k=%lld",
                                              (long long)n, (long long)d, (long long)k);
  if (pad_k_cd(k) < 0) return fail(LASSO_ERR_UNSUPPORTED, "coordinate descent: k=%lld > 4096", (long long)k);
  if (n > INT32_MAX / 2 || d > INT32_MAX / 2) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  return LASSO_OK;
}
// the arguments of lasso_cd_run / lasso_cd_finish beyond the shape: one copy, also for lasso_cd_solve, which asks before
// lasso_cd_prepare enqueues anything
int check_cd_run_args(int iters, double alpha) {
  if (iters < 0 || !(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "iters=%d alpha=%g", iters, alpha);
  return LASSO_OK;
}
int check_cd_finish_args(const void* z_out_dev, int64_t ldz, const void* z_track_out_dev, int64_t ldzt, int64_t k) {
  if ((z_out_dev && ldz < k) || (z_track_out_dev && ldzt < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  return LASSO_OK;
}

// ---------------------------------------------------------------------------
// convolutional ISTA (conv.hip)
// ---------------------------------------------------------------------------
// (kConvDpart, lasso_kernels.h: partial sums |z - z+|: 64 iterations per launch x up to 1024 workgroups, conv_fused.hip)
struct ConvWorkspace { float* Wt; float* Wp; void* Wf; float* Zm; float* Ym; float* G; float* PT; float* R; float* dpart; float* delta; double* sums;
                       float* Zc; float* Yc;      // (z, y) at the head of a speculated chunk of iterations (stop rule, below)
                       size_t bytes; };

ConvWorkspace carve_conv(void* base, const ConvGeom& g) {
  ConvWorkspace w;
  Arena a(base, 4);
  const size_t ckk = (size_t)g.C * g.kh * g.kw, M = (size_t)g.N * g.Hz * g.Wz;
  const size_t ldr = (ckk + 3) / 4 * 4;       // row stride of the pixel-major patch matrix
  w.Wt = a.take(ckk * g.K * 4);
  w.Wp = a.take(ldr * g.K * 4);
  w.Wf = a.take(conv_fused_table_bytes());
  w.Zm = a.take(M * g.K * 4);
  w.Ym = a.take(M * g.K * 4);
  w.G = a.take(M * g.K * 4);
  w.PT = a.take(ldr * M * 4);
  w.R = a.take((size_t)g.N * g.C * g.H * g.W * 4);
  w.dpart = a.take((size_t)kConvDpart * 4);
  w.delta = a.take(256);
  w.sums = a.take<double>(256);
  w.Zc = a.take(M * g.K * 4);
  w.Yc = a.take(M * g.K * 4);
  w.bytes = a.bytes();
  return w;
}

int check_conv(const ConvGeom& g, int dtype) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64)
    return fail(LASSO_ERR_UNSUPPORTED, "dtype %d: LASSO_F32 and LASSO_F64 are implemented", dtype);
  if (g.N < 0 || g.C <= 0 || g.K <= 0 || g.H <= 0 || g.W <= 0 || g.Hz <= 0 || g.Wz <= 0 || g.kh <= 0 ||
      g.kw <= 0 || g.sh <= 0 || g.sw <= 0 || g.ph < 0 || g.pw < 0)
    return fail(LASSO_ERR_BAD_ARG, "bad convolution geometry");
  // x must have exactly the size conv_transpose2d gives the code (ista.py:19: x_hat - x)
  if ((int64_t)(g.Hz - 1) * g.sh - 2 * g.ph + g.kh != g.H || (int64_t)(g.Wz - 1) * g.sw - 2 * g.pw + g.kw != g.W)
    return fail(LASSO_ERR_BAD_ARG, "image %dx%d does not match code %dx%d under kernel %dx%d stride %d,%d padding %d,%d",
                g.H, g.W, g.Hz, g.Wz, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw);
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ckk = (int64_t)g.C * g.kh * g.kw;
  if (M > INT32_MAX / 2 || ckk > INT32_MAX / 2 || (int64_t)g.N * g.C * g.H * g.W > ((int64_t)1 << 40))
    return fail(LASSO_ERR_UNSUPPORTED, "convolution problem too large");
  return LASSO_OK;
}

ConvGeom make_geom(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw,
                   int sh, int sw, int ph, int pw) {
  ConvGeom g;
  g.N = (int)N; g.C = (int)C; g.H = (int)H; g.W = (int)W; g.K = (int)K; g.Hz = (int)Hz; g.Wz = (int)Wz;
  g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
  return g;
}

// One iteration of the two-kernel form on (ws.Zm, ws.Ym) (ista.py:19-20,29,42,44): the synthesis residual, then the
// fused implicit-GEMM gradient + prox when the geometry fits, else patches + GEMM + prox.  *dcount = the number of
// partial sums |z - z+| left in ws.dpart.
int conv_two_kernel_step(const ConvWorkspace& ws, const ConvGeom& g, const float* x, const float* w, float lr, float lam,
                         float coef, int cus, int* dcount, hipStream_t st) {
  const int ldr = (g.C * g.kh * g.kw + 3) / 4 * 4;
  *dcount = 0;
  LASSO_HIP_TRY(launch_conv_residual(ws.Ym, ws.Wt, w, x, ws.PT, ws.R, g, cus, st));                   // :19
  LASSO_HIP_TRY(launch_conv_grad_prox(ws.R, ws.Wp, ldr, ws.Zm, ws.Ym, lr, lam, coef, ws.dpart, kGenGrid, g, cus,
                                      dcount, st));                                                   // :20,:29,:42,:44
  if (*dcount == 0) {
    LASSO_HIP_TRY(launch_conv_gradient(ws.R, ws.Wp, ws.PT, ldr, ws.G, g, st));                         // :20
    LASSO_HIP_TRY(launch_generic_prox(ws.Zm, g.K, ws.Ym, ws.G, (int)((int64_t)g.N * g.Hz * g.Wz), g.K, lr, lam, coef,
                                      ws.dpart, kGenGrid, st));                                       // :29,:42,:44
    *dcount = kGenGrid;
  }
  return LASSO_OK;
}

// momentum coefficients c_i = (t_i - 1) / t_{i+1} of iterations 0 .. iterations-1 (ista.py:41-42; 0 without momentum)
std::vector<float> fista_coefs(int iterations, int fast) {
  std::vector<float> coef((size_t)std::max(iterations, 1), 0.0f);
  Momentum mom;
  for (int i = 0; i < iterations; ++i) coef[i] = mom.next(fast);
  return coef;
}

}  // namespace
}  // namespace lasso

namespace lasso {
hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes) {
  // (kernel, device) -> the largest size set so far: kernels whose LDS size depends on the geometry (the convolutional
  // kernels) raise the attribute again when a later call needs more (the cache ignored the byte count)
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({kernel, dev});
  if (it != done.end() && it->second >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done[{kernel, dev}] = bytes;
  return e;
}
}  // namespace lasso

using namespace lasso;

extern "C" {

int lasso_hip_abi_version(void) { return LASSO_HIP_ABI_VERSION; }

const char* lasso_hip_status_string(int status) {
  switch (status) {
    case LASSO_OK: return "ok";
    case LASSO_ERR_BAD_ARG: return "bad argument";
    case LASSO_ERR_UNSUPPORTED: return "unsupported shape or dtype";
    case LASSO_ERR_WORKSPACE: return "workspace too small";
    case LASSO_ERR_HIP: return "HIP runtime error";
    case LASSO_WARN_LINESEARCH: return "backtracking line search failed; reverted to initial step";
    default: return "unknown status";
  }
}

const char* lasso_hip_last_error(void) { return g_err; }

int lasso_debug_force_standby(int on) {
  const int prev = lasso::g_force_standby;
  lasso::g_force_standby = on ? 1 : 0;
  return prev;
}

int lasso_hip_device_cus(int* cus_out) {
  const int c = device_cus();
  if (cus_out) *cus_out = c;
  return c > 0 ? LASSO_OK : fail(LASSO_ERR_HIP, "no HIP device visible");
}

// bytes of the solver's own workspace (the objective_out region follows it)
static size_t solver_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                                     int stop_mode, int backtrack) {
  stop_mode &= 0xFF;                                   // kernel hint / LASSO_SOLVE_ASYNC bits ride above
  const bool with_state = tol > 0.0 && stop_mode != LASSO_STOP_NONE && maxiter > 0;
  if (!fused_shape(d, k)) return carve_generic(nullptr, n, d, k, backtrack != 0, with_state).bytes;
  const int kp = pad_k(k);
  if (kp < 0) return 0;
  if (backtrack || dtype == LASSO_BF16) return carve_bt(nullptr, n, k, kp, dtype == LASSO_BF16, maxiter).bytes;
  // Every padded dictionary size solve_geometry() / the kernel hints can pick for this shape: a SMALLER kp means more
  // split-k groups, i.e. a LARGER exchange region (carve(384) needs ~2.2 MiB more than carve(512)), so the size is the
  // maximum over the candidates, not the size at pad_k(k) (an exactly-sized workspace failed at
  // d=64, k=300 and for most n at d <= 32).
  size_t bytes = carve(nullptr, n, k, kp, maxiter, with_state).bytes;
  if (kp == 512 && k <= 384 && d <= 128) bytes = std::max(bytes, carve(nullptr, n, k, 384, maxiter, with_state).bytes);
  if (kp == 1024 && k <= 768) bytes = std::max(bytes, carve(nullptr, n, k, 768, maxiter, with_state).bytes);
  // (LASSO_KERNEL_UNFUSED / the cost model may send a fused shape down the general-GEMM path: room for either)
  return std::max(bytes, carve_generic(nullptr, n, d, k, false, with_state).bytes);
}

// {lr, alpha*lr} in fp32 from L (double) with the roundings of the host path: lr = 1/L in
// double (ista.py:72-73), then the casts of run_impl()
__global__ void step_from_lipschitz_kernel(const double* __restrict__ L, double alpha, float* __restrict__ out) {
  const double lr = 1.0 / L[0];
  out[0] = (float)lr;
  out[1] = (float)(alpha * lr);
}

// One solve's workspace, any dtype: solver | objective | lipschitz.
//  objective (objective_out): a 256-byte slot for the device scalar of the loss, the objective's own workspace, and --
//    bf16 tensors -- fp32 copies of x, W and z
//  lipschitz (lr = LASSO_LR_AUTO; absent for bf16 tensors and when min(d, k) > 2048): the Lipschitz workspace, whose first
//    double is lambda_max, and -- fp32 tensors -- a 256-byte slot for {lr, alpha*lr} as floats
// fp32 / bf16 shapes without a solver (solver == 0) have no workspace: total == 0.
struct SolveRegions { size_t solver, objective, lipschitz, total; };
static SolveRegions solve_regions(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol, int stop_mode,
                                  int backtrack) {
  const bool dbl = dtype == LASSO_F64;
  SolveRegions r;
  r.solver = align_up(dbl ? f64::solve_workspace_bytes(n, d, k, maxiter, tol, stop_mode, backtrack)
                          : solver_workspace_bytes(n, d, k, dtype, maxiter, tol, stop_mode, backtrack));
  r.objective = align_up(dbl ? f64::objective_workspace_bytes(n, d, k) : lasso_objective_workspace_bytes(n, d, k)) + 256;
  if (dtype == LASSO_BF16)
    r.objective += align_up((size_t)n * d * 4) + align_up((size_t)d * k * 4) + align_up((size_t)n * k * 4);
  r.lipschitz = (dtype == LASSO_BF16 || std::min(d, k) > 2048) ? 0 : align_up(lipschitz_workspace_bytes(d, k)) + (dbl ? 0 : 256);
  r.total = (r.solver == 0 && !dbl) ? 0 : r.solver + r.objective + r.lipschitz;
  return r;
}

const char* lasso_fista_kernel_name(int64_t n, int64_t d, int64_t k, int dtype, int backtrack) {
  if (n <= 0 || d <= 0 || k <= 0) return "";
  if (dtype == LASSO_F64) return f64::solve_kernel_name(backtrack);
  if (!fused_shape(d, k)) return "lasso::gemm_nt_kernel + lasso::gemm_nt_kernel<.., prox epilogue> (unfused)";
  if (dtype == LASSO_BF16) {
    int per_cu = 0;
    const int kpb = pad_k(k);
    if (bt16_persist_occupancy(kpb, &per_cu) == hipSuccess && (n + 63) / 64 <= (int64_t)per_cu * device_cus())
      return kpb == 1024 ? "lasso::bt16_persist_kernel<1024>" : kpb == 512 ? "lasso::bt16_persist_kernel<512>"
                                                                            : "lasso::bt16_persist_kernel<256>";
    return backtrack ? "lasso::bt16_grad_kernel / bt16_trial_kernel" : "lasso::bt16_grad_kernel + lasso::generic_prox_kernel";
  }
  if (backtrack) {
    // what run_bt() dispatches for fp32 tensors in one process (row pitch == k, 16-byte-aligned state as torch and
    // hipMalloc hand it out): ONE bt_iter_kernel launch per outer iteration (accept + gradient + the first trials per
    // tile; the first launch of a solve is the <K, false> instantiation: nothing to accept) + ONE bt_iter_decide_kernel;
    // k not a multiple of 4 takes the multi-launch kernels of backtrack.hip
    const int kpb = pad_k(k);
    if ((k & 3) == 0 && k >= 4) {
      static thread_local char bname[160];
      snprintf(bname, sizeof(bname), "lasso::bt_iter_kernel<%d, true> / bt_iter_kernel<%d, false> + lasso::bt_iter_decide_kernel",
               kpb, kpb);
      return bname;
    }
    return "lasso::bt_grad_kernel / bt_trial_kernel";
  }
  const SolveGeom geom = solve_geometry(n, d, k);
  const NarrowTiles narrow(geom.narrow);
  const int kp = geom.kp, dpad = pad_d(d, kp);
  const KernelPlan plan = plan_kernel(kp, dpad, (int)((n + kTileM - 1) / kTileM), false, LASSO_KERNEL_AUTO);
  const TilePlan tp = plan_tiles(n, dpad, kp);
  KernelPlan tplan = {false, 0, 1, 0.0};
  const int tail = ragged_tail(kp, dpad, tp.ntiles, tp.waves, LASSO_KERNEL_AUTO, plan, &tplan);
  if (plan.split && !tail) {
    static thread_local char name[96];
    if (kp == 1024 && plan.tiles >= 2) snprintf(name, sizeof(name), "lasso::splitk::fista_splitk_rs_kernel<%d>", plan.tiles);
    else snprintf(name, sizeof(name), "lasso::splitk::fista_splitk_kernel<%d, %d, false>", kp, plan.tiles);
    return name;
  }
  static thread_local char tname[160];
  if (tail)
    snprintf(tname, sizeof(tname), "lasso::sp::fista_tile_sp_kernel<%d, %d, false, %d> + the last %d tiles on the split-k kernel (T = %d)",
             kp, tp.rows, tp.waves, tail, tplan.tiles);
  else
  snprintf(tname, sizeof(tname), "lasso::sp::fista_tile_sp_kernel<%d, %d, false, %d>", kp, tp.rows, tp.waves);
  return tname;
}

size_t lasso_fista_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int maxiter,
                                   double tol, int stop_mode, int backtrack) {
  if (n < 0 || d <= 0 || k <= 0) return 0;
  return solve_regions(n, d, k, dtype, maxiter, tol, stop_mode, backtrack).total;
}

int lasso_fista_prepare(const void* w_dev, int64_t ldw, int64_t d, int64_t k, int dtype, int maxiter,
                        void* workspace_dev, size_t workspace_bytes, void* stream) {
  // packs W and builds the momentum table for iterations 0 .. maxiter-1 (the workspace must
  // come from lasso_fista_workspace_bytes with the same maxiter)
  if (int s = check_common(0, d, k, dtype, /*allow_large=*/true)) return s;
  if (!w_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldw < k || maxiter < 0) return fail(LASSO_ERR_BAD_ARG, "ldw < k or maxiter < 0");
  if (!fused_shape(d, k)) {          // unfused path: W^T for the second GEMM (the workspace of solve_generic)
    if (d > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
    GenWorkspace gw = carve_generic(workspace_dev, 0, d, k, false, false);
    if (workspace_bytes < gw.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", gw.bytes);
    LASSO_HIP_TRY(launch_transpose_pad((const float*)w_dev, ldw, (int)d, (int)k, gw.Wt, d, (int)k, (int)d,
                                       (hipStream_t)stream));
    LASSO_HIP_TRY(hipMemcpy2DAsync(gw.Wc, k * 4, w_dev, ldw * 4, k * 4, d, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LASSO_OK;
  }
  const int kp = pad_k(k);
  Workspace ws = carve(workspace_dev, 0, k, kp, maxiter, false);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", ws.bytes);
  return prepare_impl(ws, kp, (const float*)w_dev, ldw, d, k, maxiter, (hipStream_t)stream);
}

int lasso_fista_run(const void* x_dev, int64_t ldx, const void* z_in_dev, int64_t ldz_in,
                    const void* y_in_dev, int64_t ldy_in, void* z_out_dev, int64_t ldz_out,
                    void* y_out_dev, int64_t ldy_out, int64_t n, int64_t d, int64_t k, int dtype,
                    double alpha, double lr, int fast, int it0, int iters, int maxiter, int kernel_hint,
                    float* delta_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (int s = check_common(n, d, k, dtype, /*allow_large=*/true)) return s;
  if (!x_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (it0 < 0 || iters < 0) return fail(LASSO_ERR_BAD_ARG, "negative iteration range");
  if (!fused_shape(d, k)) {
    if (it0 + iters > maxiter) return fail(LASSO_ERR_BAD_ARG, "it0 + iters = %d > maxiter = %d", it0 + iters, maxiter);
    if (ldx < d || ldz_out < k || (z_in_dev && ldz_in < k) || (y_in_dev && ldy_in < k) || (y_out_dev && ldy_out < k))
      return fail(LASSO_ERR_BAD_ARG, "leading dimension smaller than the row length");
    return run_generic((const float*)x_dev, ldx, (const float*)z_in_dev, ldz_in,
                       (const float*)y_in_dev, ldy_in, (float*)z_out_dev, ldz_out, (float*)y_out_dev, ldy_out, n, d, k,
                       alpha, lr, fast, it0, iters, delta_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
  }
  if (delta_dev && iters > kChunkMax)
    return fail(LASSO_ERR_BAD_ARG, "iters=%d > %d with delta recording", iters, kChunkMax);
  if (ldx < d || ldz_out < k || (z_in_dev && ldz_in < k) || (y_in_dev && ldy_in < k) ||
      (y_out_dev && ldy_out < k))
    return fail(LASSO_ERR_BAD_ARG, "leading dimension smaller than the row length");
  const int kp = pad_k(k);
  if (it0 + iters > maxiter) return fail(LASSO_ERR_BAD_ARG, "it0 + iters = %d > maxiter = %d", it0 + iters, maxiter);
  if ((kernel_hint & ~LASSO_KERNEL_MASK) || ((kernel_hint & 0x300) != LASSO_KERNEL_AUTO &&
      (kernel_hint & 0x300) != LASSO_KERNEL_TILE && (kernel_hint & 0x300) != LASSO_KERNEL_SPLITK))
    return fail(LASSO_ERR_BAD_ARG, "kernel hint 0x%x", kernel_hint);
  // same carve as lasso_fista_prepare(maxiter): the momentum table it built is read here
  Workspace ws = carve(workspace_dev, n, k, kp, maxiter, false);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", ws.bytes);
  hipStream_t st = (hipStream_t)stream;
  return run_impl(ws, kp, (const float*)x_dev, ldx, (const float*)z_in_dev, ldz_in,
                  (const float*)y_in_dev, ldy_in, (float*)z_out_dev, ldz_out, (float*)y_out_dev,
                  ldy_out, n, d, k, alpha, lr, fast, it0, iters, delta_dev, st, -1.0f, kernel_hint);
}

// What lasso_fista_solve decodes, once, from the LASSO_SOLVE_* bits of stop_mode (status_mapped: LASSO_SOLVE_STATUS_MAPPED,
// the device-writable host words) and from lr = LASSO_LR_AUTO on the fp32 fixed-step path: {lr, alpha*lr} as floats in
// device memory, lambda_max they are made from, and the Lipschitz workspace whose launches carry the prepare blocks.
struct SolveAsync { bool async, sharded, one_chunk, defer_verdict; int32_t* status_mapped; };
struct AutoStep { const float* lr_dev; const double* lip_dev; void* lip_ws; };

// bf16 fixed step without the stop rule: rows are independent, so a batch beyond the persistent kernel's capacity (one
// resident workgroup per 64-row tile: `cap` = 16384 rows) is a sequence of launches over row blocks of that size instead
// of the multi-launch kernels (2.7x slower per row).  *ran = false: a block gave up (busy GPU), the caller redoes everything.
static int solve_bf16_row_blocks(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                                 int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int kp,
                                 int64_t cap, double alpha, double lr, int fast, int maxiter, double eta_backtrack,
                                 int32_t* iters_out, void* workspace_dev, size_t workspace_bytes, hipStream_t st,
                                 bool* ran) {
  const char* xb = (const char*)x_dev; const char* zb = (const char*)z0_dev; char* ob = (char*)z_out_dev;
  *ran = true;
  int64_t r0 = 0;
  for (; r0 < n; r0 += cap) {
    const int64_t nb = std::min(cap, n - r0);
    bool ran_b = false;
    const void* fb = nullptr;
    const int sb = solve_bf16_persistent(xb + r0 * ldx * 2, ldx, w_dev, ldw, zb ? zb + r0 * ldz0 * 2 : nullptr, ldz0,
                                         ob + r0 * ldz * 2, ldz, nb, d, k, kp, alpha, lr, fast, maxiter, 0.0, 0,
                                         eta_backtrack, nullptr, nullptr, nullptr, nullptr, nullptr, workspace_dev,
                                         workspace_bytes, st, &ran_b, &fb);
    if (sb != LASSO_OK) return sb;
    if (!ran_b) { *ran = false; break; }
  }
  if (*ran && iters_out) *iters_out = maxiter;
  if (!*ran && z0_dev && z0_dev == z_out_dev && r0 > 0)
    return fail(LASSO_ERR_HIP, "in-place bf16 solve interrupted after %lld rows", (long long)r0);
  return LASSO_OK;
}

// The fp32 fixed-step solve on the fused shapes: solve_fixed_f32 carves and prepares, then runs ONE of the four forms of
// the stop rule below -- or, after the in-kernel rule gave up, a second one.
struct FixedSolve {
  const float* x; int64_t ldx; const float* w; int64_t ldw; const float* z0; int64_t ldz0; float* zout; int64_t ldz;
  int64_t n, d, k;
  double alpha, lr; int fast, maxiter, hint;
  int32_t* iters_out; float* last_delta_out; void* workspace_dev; hipStream_t st;
  const SolveAsync& req; const AutoStep& step;
  // set by solve_fixed_f32
  Workspace ws; int kps;
  float budget;                               // n k tol (ista.py:64), compared in fp32
  const float* start; int64_t ld_start;       // z0 -- its copy in ws.state[2] where z0 IS zout: intact for a replay / a second attempt
};

// `iters` iterations from iteration it0 in one run_impl call, with the hint the form runs under
static int run_fixed(const FixedSolve& c, int hint, const float* z_in, int64_t ldz_in, const float* y_in, int64_t ldy_in,
                     float* z_out, int64_t ldz_out, float* y_out, int64_t ldy_out, int it0, int iters, float* delta_dev,
                     float in_kernel_budget, const ChunkVerdict* cv) {
  return run_impl(c.ws, c.kps, c.x, c.ldx, z_in, ldz_in, y_in, ldy_in, z_out, ldz_out, y_out, ldy_out, c.n, c.d, c.k,
                  c.alpha, c.lr, c.fast, it0, iters, delta_dev, c.st, in_kernel_budget, hint, nullptr, c.step.lr_dev, cv);
}

// LASSO_SOLVE_SHARDED: this batch is a row shard -- the rule needs the other ranks' sums.  One chunk, its per-iteration
// sums left in ws.delta for the caller's all-reduce; lasso_fista_solve_verdict judges them.
static int solve_sharded_one_chunk(const FixedSolve& c, int stop_mode) {
  if (!c.req.async || stop_mode != LASSO_STOP_GLOBAL)
    return fail(LASSO_ERR_BAD_ARG, "LASSO_SOLVE_SHARDED needs LASSO_SOLVE_ASYNC | LASSO_STOP_GLOBAL");
  if (c.maxiter > kChunkMax)
    return fail(LASSO_ERR_UNSUPPORTED, "LASSO_SOLVE_SHARDED: maxiter=%d > %d", c.maxiter, kChunkMax);
  // (y_out = NULL: the one chunk is the whole solve -- a verdict of "redo" repeats it from its start, nothing
  // continues from its momentum point; round 6: the kernel no longer writes the n x k tile of y nobody reads)
  if (int s = run_fixed(c, c.hint, c.start, c.ld_start, nullptr, 0, c.zout, c.ldz, nullptr, 0, 0, c.maxiter, c.ws.delta,
                        -1.0f, nullptr))
    return s;
  return LASSO_PENDING;
}

// The exact global rule in-kernel (every tile has its own resident workgroup; one-iteration lag): a single
// launch runs to the stopping iteration -- one host sync, at the end (asynchronous: none, the caller collects the words
// later).  CUs held by OTHER work are invisible to the occupancy query that admitted the grid: then the handshake times
// out and the kernel aborts as a whole without touching z_out.  *aborted says so: another form repeats the solve.
static int solve_in_kernel(const FixedSolve& c, bool* aborted) {
  *aborted = false;
  // (granule ring and stop_out were zeroed by the prepare launch)
  if (int s = run_fixed(c, c.hint, c.start, c.ld_start, nullptr, 0, c.zout, c.ldz, nullptr, 0, 0, c.maxiter, nullptr,
                        c.budget, nullptr))
    return s;
  if (c.req.async) return LASSO_PENDING;
  StopWords words;
  if (int s = read_stop_words(c.ws.stop_out, c.st, &words)) return s;
  if ((*aborted = words.redo())) return LASSO_OK;          // some workgroup was not resident
  if (c.iters_out) *c.iters_out = words.iterations();
  if (c.last_delta_out) *c.last_delta_out = words.last_delta();
  return LASSO_OK;
}

// LASSO_SOLVE_ASYNC beyond the in-kernel rule (more tiles than resident workgroups) when maxiter fits one chunk: the
// chunk is enqueued, a one-thread kernel turns its per-iteration deltas into the words the collect call copies --
// {iterations, last delta, redo} -- and the call returns without waiting.  "redo" is set when the rule fired BEFORE the
// last iteration (z_out is then a later iterate): the caller repeats the solve synchronously, as after an aborted
// handshake.  The E-step of an EM loop (maxiter = 10) practically never stops early, and no longer waits for the host.
static int solve_async_one_chunk(const FixedSolve& c, int hint) {
  // LASSO_SOLVE_DEFER_VERDICT: the verdict launch is left to lasso_fista_solve_verdict_deferred (another stream)
  const bool defer = c.req.defer_verdict && c.req.status_mapped && c.maxiter <= 64 && c.n > 0;
  t_deferred_verdict.armed = false;
  t_deferred_verdict.workspace = c.workspace_dev;
  const ChunkVerdict cv{c.budget, c.ws.stop_out, c.req.status_mapped, defer ? &t_deferred_verdict : nullptr};
  if (int s = run_fixed(c, hint, c.start, c.ld_start, nullptr, 0, c.zout, c.ldz, nullptr, 0, 0, c.maxiter, c.ws.delta,
                        -1.0f, &cv))
    return s;
  if (c.maxiter > 64 || c.n == 0) {
    hipLaunchKernelGGL(chunk_verdict_kernel, dim3(1), dim3(1), 0, c.st, c.ws.delta, c.maxiter, c.budget, c.ws.stop_out,
                       c.req.status_mapped);
    LASSO_HIP_TRY(hipGetLastError());
  }
  if (defer && t_deferred_verdict.armed) return LASSO_PENDING_DEFERRED;
  return c.req.status_mapped ? LASSO_PENDING_MAPPED : LASSO_PENDING;
}

// The exact global rule, chunked: speculate a chunk, read its per-iteration deltas, replay the chunk up to the stopping
// iteration if one fired.  The state ping-pongs between two pairs of workspace buffers, so a chunk's
// input stays intact for its replay without a copy (run_impl takes in / out state pointers: speculate_stop_rule's save /
// restore would add launches here).
static int solve_chunked(const FixedSolve& c, int hint) {
  const float* cur_z = c.start, * cur_y = nullptr;
  int64_t cur_ldz = c.ld_start, cur_ldy = 0;
  int done = 0, flip = 0, next_chunk = kChunkMax;
  float hdelta[kChunkMax], last = NAN;
  while (done < c.maxiter) {
    const int cn = std::min(next_chunk, c.maxiter - done);
    const bool final_chunk = (done + cn == c.maxiter);
    float* nz = final_chunk ? c.zout : c.ws.state[2 * flip];
    const int64_t nldz = final_chunk ? c.ldz : c.k;
    float* ny = c.ws.state[2 * flip + 1];
    // the aliasing copy used state[2]; first chunk writes state[0]/[1] (flip = 0)
    if (int s = run_fixed(c, hint, cur_z, cur_ldz, cur_y, cur_ldy, nz, nldz, ny, c.k, done, cn, c.ws.delta, -1.0f, nullptr))
      return s;
    if (int s = read_back(hdelta, c.ws.delta, cn * sizeof(float), c.st)) return s;
    const int hit = first_stop<float>(hdelta, cn, c.budget);
    if (hit >= 0) {
      if (hit + 1 < cn) {   // replay the chunk from its (intact) input state
        if (int s = run_fixed(c, hint, cur_z, cur_ldz, cur_y, cur_ldy, c.zout, c.ldz, nullptr, 0, done, hit + 1, nullptr,
                              -1.0f, nullptr))
          return s;
      } else if (!final_chunk) {
        LASSO_HIP_TRY(hipMemcpy2DAsync(c.zout, c.ldz * 4, nz, nldz * 4, c.k * 4, c.n, hipMemcpyDeviceToDevice, c.st));
      }
      done += hit + 1;
      last = hdelta[hit];
      break;
    }
    done += cn;
    last = hdelta[cn - 1];
    cur_z = nz; cur_ldz = nldz; cur_y = ny; cur_ldy = c.k;
    flip ^= 1;
    next_chunk = next_tile_chunk(hdelta, cn, c.budget, kChunkMax);       // (scheduling only: stoprule_host.hpp)
  }
  if (c.iters_out) *c.iters_out = done;
  if (c.last_delta_out) *c.last_delta_out = last;
  return LASSO_OK;
}

static int solve_fixed_f32(FixedSolve& c, double tol, int stop_mode, bool stop_rule, size_t workspace_bytes) {
  const int64_t n = c.n, d = c.d, k = c.k;
  const int kps = c.kps = pad_k_solve(n, d, k);          // (768 atoms have their own tile kernel)
  // (a thread-local that pad_d reads: alive across every run_impl, plan_tiles and pad_d call of the solve)
  const NarrowTiles narrow(narrow_tiles(n, d, k, kps, c.hint));
  c.ws = carve(c.workspace_dev, n, k, kps, c.maxiter, stop_rule);
  const Workspace& ws = c.ws;
  if (workspace_bytes < ws.bytes)
    return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  // one launch: pack W, momentum table, {lr, alpha*lr} from lambda_max, the zeroing of the in-kernel rule's ring and words
  PrepareExtras px = {nullptr, 0, nullptr, 0, c.step.lip_dev, c.alpha, const_cast<float*>(c.step.lr_dev)};
  const TilePlan tp = plan_tiles(n, pad_d(d, kps), kps);
  if (stop_rule && stop_mode == LASSO_STOP_GLOBAL) {
    px.zero_a = ws.gran; px.words_a = kStopRing * std::max(tp.ntiles, kSplitMaxParts);
    px.zero_b = reinterpret_cast<unsigned long long*>(ws.stop_out); px.words_b = 2;
  }
  // (lr = LASSO_LR_AUTO: the Lipschitz launches were left to this point -- their Gram launch carries the prepare blocks)
  if (c.step.lip_ws) {
    if (int s = prepare_with_lipschitz(ws, kps, c.w, c.ldw, d, k, c.maxiter, c.st, px, c.step.lip_ws)) return s;
  } else if (int s = prepare_impl(ws, kps, c.w, c.ldw, d, k, c.maxiter, c.st, &px)) return s;

  if (!stop_rule) {
    if (int s = run_fixed(c, c.hint, c.z0, c.ldz0, nullptr, 0, c.zout, c.ldz, nullptr, 0, 0, c.maxiter, nullptr, -1.0f, nullptr))
      return s;
    if (c.iters_out) *c.iters_out = c.maxiter;
    return LASSO_OK;
  }

  c.budget = stop_budget<float>(n, k, tol);
  const bool aliased = c.z0 && c.z0 == c.zout;
  c.start = c.z0; c.ld_start = c.ldz0;
  if (aliased) {              // keep the initial state intact for a replay / a second attempt
    LASSO_HIP_TRY(hipMemcpy2DAsync(ws.state[2], k * 4, c.z0, c.ldz0 * 4, k * 4, n, hipMemcpyDeviceToDevice, c.st));
    c.start = ws.state[2]; c.ld_start = k;
  }
  if (c.req.sharded) return solve_sharded_one_chunk(c, stop_mode);
  // an asynchronous solve whose maxiter fits one chunk can leave the verdict to the device
  const bool fits_one_chunk = c.req.async && stop_mode == LASSO_STOP_GLOBAL && c.maxiter <= kChunkMax && !aliased;
  int hint = c.hint;
  // (LASSO_SOLVE_ONE_CHUNK: all `maxiter` iterations are expected to run -- the plain kernels + the device verdict are
  // cheaper per iteration than the in-kernel rule's exchange, whose granule fetch covers 256 tiles: four per lane of a wave)
  if (stop_mode == LASSO_STOP_GLOBAL && !(c.req.one_chunk && fits_one_chunk) &&
      tp.ntiles <= std::min(fista_resident_workgroups(kps, pad_d(d, kps), tp.waves), 256)) {
    bool aborted = false;
    const int s = solve_in_kernel(c, &aborted);
    if (!aborted) return s;
    hint = LASSO_KERNEL_TILE;      // no cross-workgroup traffic from here on
  }
  if (fits_one_chunk) return solve_async_one_chunk(c, hint);
  return solve_chunked(c, hint);
}

static int solve_impl(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                      const void* z0_dev, int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n,
                      int64_t d, int64_t k, int dtype, double alpha, double lr, int fast,
                      int maxiter, double tol, int stop_mode, int backtrack, double eta_backtrack,
                      int32_t* iters_out, float* last_delta_out, int32_t* trials_out,
                      float* accepted_lr_out, float* accepted_f_out, void* workspace_dev,
                      size_t workspace_bytes, void* stream, const SolveAsync& req, const AutoStep& step) {
  // LASSO_BF16 (x, W, z0, z_out all bf16) is native on the fused shapes
  const bool half_any = dtype == LASSO_BF16 && fused_shape(d, k) && maxiter > 0 && n > 0;
  const bool half_bt = half_any && backtrack;
  if (int s = check_common(n, d, k, half_any ? LASSO_F32 : dtype, /*allow_large=*/true)) return s;
  if (!x_dev || !w_dev || !z_out_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (maxiter < 0) return fail(LASSO_ERR_BAD_ARG, "maxiter < 0");
  if (!fused_shape(d, k) && backtrack && dtype != LASSO_F32)
    return fail(LASSO_ERR_UNSUPPORTED, "backtrack=1 beyond d<=%d, k<=%d needs fp32 tensors", kFistaD, kFistaMaxK);
  if (ldx < d || ldw < k || ldz < k || (z0_dev && ldz0 < k))
    return fail(LASSO_ERR_BAD_ARG, "leading dimension smaller than the row length");
  if (!(lr > 0.0) || !(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "need lr > 0 and alpha >= 0");
  if (backtrack && !(eta_backtrack > 1.0)) return fail(LASSO_ERR_BAD_ARG, "eta must be > 1.");
  hipStream_t st = (hipStream_t)stream;
  if (iters_out) *iters_out = 0;
  if (last_delta_out) *last_delta_out = NAN;
  const float* x = (const float*)x_dev;
  const float* z0 = (const float*)z0_dev;
  float* zout = (float*)z_out_dev;

  if (maxiter == 0 || n == 0) {   // ista.py:76,104: returns z0 itself
    return n > 0 ? seed_state(z0, ldz0, zout, ldz, nullptr, n, k, st) : LASSO_OK;
  }

  int hint = stop_mode & LASSO_KERNEL_MASK;            // kernel-selection hint rides in stop_mode
  stop_mode &= ~LASSO_KERNEL_MASK;
  if (stop_mode != LASSO_STOP_GLOBAL && stop_mode != LASSO_STOP_NONE && stop_mode != LASSO_STOP_GLOBAL_CHUNKED)
    return fail(LASSO_ERR_BAD_ARG, "stop_mode %d", stop_mode);
  // defined hints: AUTO (optionally | 0x800 = narrow tiles), TILE, UNFUSED, SPLITK with its T / exchange knobs
  if (((hint & 0x300) != LASSO_KERNEL_SPLITK && (hint & 0x3400)) ||
      ((hint & 0x300) != LASSO_KERNEL_SPLITK && (hint & 0x300) != LASSO_KERNEL_AUTO && (hint & 0x800)) ||
      ((hint & 0x400) && (hint & 0x800)))
    return fail(LASSO_ERR_BAD_ARG, "kernel hint 0x%x", hint);
  const bool want_unfused = (hint & 0x300) == LASSO_KERNEL_UNFUSED;
  const bool stop_rule = tol > 0.0 && stop_mode != LASSO_STOP_NONE;
  if (!workspace_dev) return fail(LASSO_ERR_WORKSPACE, "workspace is null");
  if (!fused_shape(d, k) && backtrack)
    return solve_generic_backtracking(x, ldx, (const float*)w_dev, ldw, z0, ldz0, zout, ldz, n, d, k, alpha, lr, fast,
                                      maxiter, stop_rule ? tol : 0.0, eta_backtrack, iters_out, last_delta_out,
                                      trials_out, accepted_lr_out, accepted_f_out, workspace_dev, workspace_bytes, st);
  if (!fused_shape(d, k) || (want_unfused && !backtrack && dtype == LASSO_F32 && !step.lr_dev && !req.async))
    return solve_generic(x, ldx, (const float*)w_dev, ldw, z0, ldz0, zout, ldz, n, d, k, alpha, lr, fast,
                         maxiter, stop_rule ? tol : 0.0, iters_out, last_delta_out, workspace_dev,
                         workspace_bytes, st);
  const int kp = pad_k(k);
  if (half_any && (hint & 0x300) != LASSO_KERNEL_TILE) {
    // bf16 tensors: the persistent single-launch kernel when every 64-row tile has its own
    // resident workgroup (LASSO_KERNEL_TILE asks for the multi-launch kernels instead)
    bool ran = false;
    const void* z0_fb = z0_dev;
    int per_cu = 0;
    const int64_t cap = bt16_persist_occupancy(kp, &per_cu) == hipSuccess ? (int64_t)per_cu * device_cus() * 64 : 0;
    if (!backtrack && !stop_rule && cap > 0 && n > cap) {
      // (with the stop rule or the line search the decisions need sums over ALL rows at once: the multi-launch path)
      bool all = false;
      if (int sb = solve_bf16_row_blocks(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, kp, cap, alpha, lr,
                                         fast, maxiter, eta_backtrack, iters_out, workspace_dev, workspace_bytes, st, &all))
        return sb;
      if (all) return LASSO_OK;
    } else {
    const int s = solve_bf16_persistent(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, kp, alpha, lr,
                                        fast, maxiter, stop_rule ? tol : 0.0, backtrack, eta_backtrack, iters_out,
                                        last_delta_out, trials_out, accepted_lr_out, accepted_f_out, workspace_dev,
                                        workspace_bytes, st, &ran, &z0_fb);
    if (ran || (s != LASSO_OK && s != LASSO_WARN_LINESEARCH)) return s;
    z0_dev = z0_fb;
    if (z0_fb != z0) ldz0 = k;
    }
  }
  if (half_any && !backtrack)
    return solve_fixed_bf16(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, kp, alpha, lr, fast,
                            maxiter, stop_rule ? tol : 0.0, iters_out, last_delta_out, workspace_dev,
                            workspace_bytes, st);
  if (backtrack)
    return solve_backtracking(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, kp,
                              half_bt ? LASSO_BF16 : LASSO_F32, alpha, lr, fast, maxiter,
                              stop_rule ? tol : 0.0, eta_backtrack,
                              iters_out, last_delta_out, trials_out, accepted_lr_out, accepted_f_out, workspace_dev,
                              workspace_bytes, st, nullptr, nullptr, 0,
                              // A/B knobs of the fp32 line search: TILE = one trial per launch, SPLITK = round 4's
                              // multi-launch form (gradient / trials / accept as separate launches)
                              (hint & 0x300) == LASSO_KERNEL_TILE ? 1 : (hint & 0x300) == LASSO_KERNEL_SPLITK ? 2 : 0);
  // fp32 fixed step from here on
  FixedSolve c{x, ldx, (const float*)w_dev, ldw, z0, ldz0, zout, ldz, n, d, k, alpha, lr, fast, maxiter, hint, iters_out,
               last_delta_out, workspace_dev, st, req, step};
  return solve_fixed_f32(c, tol, stop_mode, stop_rule, workspace_bytes);
}

// float64 tensors: see lasso_fista_solve_f64 in include/lasso_hip.h
int lasso_fista_solve_f64(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                          int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha,
                          double lr, int fast, int maxiter, double tol, int stop_mode, int backtrack,
                          double eta_backtrack, int32_t* iters_out, double* last_delta_out, int32_t* trials_out,
                          double* accepted_lr_out, double* accepted_f_out, double* objective_out, void* workspace_dev,
                          size_t workspace_bytes, void* stream) {
  if (objective_out) *objective_out = NAN;
  if (stop_mode & ~0xFF & ~LASSO_KERNEL_MASK)
    return fail(LASSO_ERR_UNSUPPORTED, "LASSO_F64: asynchronous and sharded solves are fp32 only");
  if ((stop_mode & 0x300) == LASSO_KERNEL_TILE || (stop_mode & 0x300) == LASSO_KERNEL_SPLITK)
    return fail(LASSO_ERR_UNSUPPORTED, "LASSO_F64: the fused tile / split-k kernels are fp32 only");
  stop_mode &= 0xFF;
  if (n < 0 || d <= 0 || k <= 0) return fail(LASSO_ERR_BAD_ARG, "bad shape n=%lld d=%lld k=%lld", (long long)n,
                                              (long long)d, (long long)k);
  if (!w_dev || !workspace_dev || (n > 0 && (!x_dev || !z_out_dev))) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || (z0_dev && ldz0 < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (maxiter < 0) return fail(LASSO_ERR_BAD_ARG, "maxiter < 0");
  if (backtrack && !(eta_backtrack > 1.0)) return fail(LASSO_ERR_BAD_ARG, "eta must be > 1.");     // ista.py:18-19
  if (stop_mode == LASSO_STOP_NONE) tol = 0.0;
  const SolveRegions reg = solve_regions(n, d, k, LASSO_F64, maxiter, tol, stop_mode, backtrack);
  hipStream_t st = (hipStream_t)stream;
  if (lr == LASSO_LR_AUTO) {                            // lr = 1 / lambda_max(W^T W) (ista.py:59-63), one host round trip
    if (reg.lipschitz == 0) return fail(LASSO_ERR_UNSUPPORTED, "lr = LASSO_LR_AUTO: min(d,k) > 2048");
    if (workspace_bytes < reg.total) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, reg.total);
    char* const lip_ws = (char*)workspace_dev + reg.solver + reg.objective;
    LASSO_HIP_TRY(launch_lipschitz_f64((const double*)w_dev, ldw, d, k, lip_ws, 20, st));
    double L = 0.0;
    LASSO_HIP_TRY(hipMemcpyAsync(&L, lip_ws, sizeof(double), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    lr = 1.0 / L;
  }
  if (n == 0) {                                         // nothing to solve (the reference's loop stops at once: 0 <= 0)
    if (iters_out) *iters_out = maxiter > 0 ? 1 : 0;
    if (last_delta_out) *last_delta_out = maxiter > 0 ? 0.0 : NAN;
    return LASSO_OK;
  }
  int status;
  if (backtrack)
    status = f64::solve_backtracking((const double*)x_dev, ldx, (const double*)w_dev, ldw, (const double*)z0_dev, ldz0,
                                     (double*)z_out_dev, ldz, n, d, k, alpha, lr, fast, maxiter, tol, eta_backtrack,
                                     iters_out, last_delta_out, trials_out, accepted_lr_out, accepted_f_out,
                                     workspace_dev, std::min(workspace_bytes, reg.solver), st);
  else
    status = f64::solve((const double*)x_dev, ldx, (const double*)w_dev, ldw, (const double*)z0_dev, ldz0,
                        (double*)z_out_dev, ldz, n, d, k, alpha, lr, fast, maxiter, tol, iters_out, last_delta_out,
                        workspace_dev, std::min(workspace_bytes, reg.solver), st);
  if ((status != LASSO_OK && status != LASSO_WARN_LINESEARCH) || !objective_out) return status;
  // objective_out: the mean objective of the RETURNED code, in double (ista.py:66-69)
  if (workspace_bytes < reg.solver + reg.objective)
    return fail(LASSO_ERR_WORKSPACE, "objective_out: workspace %zu < %zu bytes", workspace_bytes, reg.solver + reg.objective);
  double* const loss_dev = (double*)((char*)workspace_dev + reg.solver);
  if (int s2 = f64::objective((const double*)x_dev, ldx, (const double*)w_dev, ldw, (const double*)z_out_dev, ldz, n, d,
                              k, alpha, loss_dev, nullptr, nullptr, (char*)loss_dev + 256, reg.objective - 256, st))
    return s2;
  LASSO_HIP_TRY(hipMemcpyAsync(objective_out, loss_dev, sizeof(double), hipMemcpyDeviceToHost, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  return status;
}

int lasso_fista_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                      const void* z0_dev, int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n,
                      int64_t d, int64_t k, int dtype, double alpha, double lr, int fast,
                      int maxiter, double tol, int stop_mode, int backtrack, double eta_backtrack,
                      int32_t* iters_out, float* last_delta_out, int32_t* trials_out,
                      float* accepted_lr_out, float* accepted_f_out, float* objective_out, void* workspace_dev,
                      size_t workspace_bytes, void* stream) {
  if (dtype == LASSO_F64) {
    // the same solve; the float slots receive the doubles rounded once (lasso_fista_solve_f64 keeps them)
    const int cap = std::max(maxiter, 1);
    std::vector<double> lr64(accepted_lr_out ? cap : 0), f64v(accepted_f_out ? cap : 0);
    double last64 = NAN, obj64 = NAN;
    int32_t iters = 0;
    const int status = lasso_fista_solve_f64(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, alpha, lr, fast,
                                             maxiter, tol, stop_mode, backtrack, eta_backtrack, &iters, &last64, trials_out,
                                             accepted_lr_out ? lr64.data() : nullptr, accepted_f_out ? f64v.data() : nullptr,
                                             objective_out ? &obj64 : nullptr, workspace_dev, workspace_bytes, stream);
    if (status != LASSO_OK && status != LASSO_WARN_LINESEARCH) return status;
    if (iters_out) *iters_out = iters;
    if (last_delta_out) *last_delta_out = (float)last64;
    if (objective_out) *objective_out = (float)obj64;
    if (backtrack)
      for (int i = 0; i < iters && i < cap; ++i) {
        if (accepted_lr_out) accepted_lr_out[i] = (float)lr64[i];
        if (accepted_f_out) accepted_f_out[i] = (float)f64v[i];
      }
    return status;
  }
  if (objective_out) *objective_out = NAN;
  SolveAsync req = {(stop_mode & LASSO_SOLVE_ASYNC) != 0, (stop_mode & LASSO_SOLVE_SHARDED) != 0,
                    (stop_mode & LASSO_SOLVE_ONE_CHUNK) != 0, (stop_mode & LASSO_SOLVE_DEFER_VERDICT) != 0, nullptr};
  if (stop_mode & LASSO_SOLVE_STATUS_MAPPED) {      // iters_out is a device-writable host buffer of four words
    if (!req.async || !iters_out) return fail(LASSO_ERR_BAD_ARG, "LASSO_SOLVE_STATUS_MAPPED needs LASSO_SOLVE_ASYNC and iters_out");
    req.status_mapped = iters_out;
    iters_out = nullptr; last_delta_out = nullptr;
  }
  if (req.defer_verdict && (!(req.status_mapped && req.one_chunk) || req.sharded))
    return fail(LASSO_ERR_BAD_ARG, "LASSO_SOLVE_DEFER_VERDICT needs LASSO_SOLVE_STATUS_MAPPED and LASSO_SOLVE_ONE_CHUNK, without LASSO_SOLVE_SHARDED");
  stop_mode &= ~(LASSO_SOLVE_ASYNC | LASSO_SOLVE_SHARDED | LASSO_SOLVE_ONE_CHUNK | LASSO_SOLVE_STATUS_MAPPED |
                 LASSO_SOLVE_DEFER_VERDICT);
  if (req.sharded && !(req.async && tol > 0.0 && maxiter > 0 && n > 0 && fused_shape(d, k)))
    return fail(LASSO_ERR_UNSUPPORTED, "LASSO_SOLVE_SHARDED: asynchronous fp32 solves with tol > 0 on the fused shapes only");
  if (req.async && (objective_out || backtrack || dtype != LASSO_F32))
    return fail(LASSO_ERR_BAD_ARG, "LASSO_SOLVE_ASYNC: fp32 fixed-step solves without objective_out only");
  AutoStep step = {nullptr, nullptr, nullptr};
  if (lr == LASSO_LR_AUTO) {
    // lr = 1/L, L = lambda_max(W^T W) (ista.py:72-73, :8-14) computed here on the stream.  The fp32
    // fixed-step kernels read {lr, alpha*lr} from device memory -- no host round trip; the other
    // paths need the step size on the host (line-search bookkeeping, the unfused driver).
    if (dtype != LASSO_F32) return fail(LASSO_ERR_BAD_ARG, "lr = LASSO_LR_AUTO needs fp32 tensors (ista.py:12)");
    if (!x_dev || !w_dev || d <= 0 || k <= 0 || n < 0 || ldw < k) return fail(LASSO_ERR_BAD_ARG, "bad argument");
    const SolveRegions reg = solve_regions(n, d, k, dtype, maxiter, tol, stop_mode, backtrack);
    if (reg.lipschitz == 0) return fail(LASSO_ERR_UNSUPPORTED, "lr = LASSO_LR_AUTO: min(d,k) > 2048");
    const size_t before = reg.solver + reg.objective;
    if (!workspace_dev || workspace_bytes < before + reg.lipschitz)
      return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, before + reg.lipschitz);
    hipStream_t st = (hipStream_t)stream;
    char* const lip_ws = (char*)workspace_dev + before;
    if (fused_shape(d, k) && !backtrack && maxiter > 0 && n > 0) {
      float* const slot = (float*)(lip_ws + reg.lipschitz - 256);
      // solve_fixed_f32 enqueues the Lipschitz launches with its prepare blocks; the launch that finishes lambda_max
      // fills the slot
      step = {slot, (const double*)lip_ws, lip_ws};
      lr = 1.0;                                        // placeholder, never used by the kernels
    } else {
      LASSO_HIP_TRY(launch_lipschitz((const float*)w_dev, ldw, d, k, lip_ws, 20, st));
      double L = 0.0;
      LASSO_HIP_TRY(hipMemcpyAsync(&L, lip_ws, sizeof(double), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
      lr = 1.0 / L;
    }
  }
  const int status = solve_impl(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, dtype, alpha, lr,
                                fast, maxiter, tol, stop_mode, backtrack, eta_backtrack, iters_out,
                                last_delta_out, trials_out, accepted_lr_out, accepted_f_out, workspace_dev,
                                workspace_bytes, stream, req, step);
  if ((status != LASSO_OK && status != LASSO_WARN_LINESEARCH) || !objective_out || n <= 0) return status;
  // objective_out: (0.5*||x - z W^T||^2 + alpha*||z||_1)/n of the RETURNED code, evaluated in fp32
  // (the verbose print of ista.py:66-69,80-81 for the final iterate; dict_learning.py:10-13)
  char saved[sizeof(g_err)];
  memcpy(saved, g_err, sizeof(saved));          // keep the line-search warning text
  const SolveRegions reg = solve_regions(n, d, k, dtype, maxiter, tol, stop_mode, backtrack);
  if (!workspace_dev || workspace_bytes < reg.solver + reg.objective)
    return fail(LASSO_ERR_WORKSPACE, "objective_out: workspace %zu < %zu bytes", workspace_bytes,
                reg.solver + reg.objective);
  hipStream_t st = (hipStream_t)stream;
  Arena a((char*)workspace_dev + reg.solver);
  float* loss_dev = a.take(256);
  const size_t obj_bytes = align_up(lasso_objective_workspace_bytes(n, d, k));
  char* obj_ws = a.take<char>(obj_bytes);
  const void* xo = x_dev; const void* wo = w_dev; const void* zo = z_out_dev;
  int64_t ldxo = ldx, ldwo = ldw, ldzo = ldz;
  if (dtype == LASSO_BF16) {
    float* xf = a.take((size_t)n * d * 4), * wf = a.take((size_t)d * k * 4), * zf = a.take((size_t)n * k * 4);
    LASSO_HIP_TRY(launch_cvt_bf16(x_dev, ldx, xf, d, (int)n, (int)d, 1, st));
    LASSO_HIP_TRY(launch_cvt_bf16(w_dev, ldw, wf, k, (int)d, (int)k, 1, st));
    LASSO_HIP_TRY(launch_cvt_bf16(z_out_dev, ldz, zf, k, (int)n, (int)k, 1, st));
    xo = xf; wo = wf; zo = zf; ldxo = d; ldwo = k; ldzo = k;
  }
  if (int s2 = lasso_objective(xo, ldxo, wo, ldwo, zo, ldzo, n, d, k, LASSO_F32, alpha, loss_dev, nullptr, obj_ws,
                               obj_bytes, stream))
    return s2;
  LASSO_HIP_TRY(hipMemcpyAsync(objective_out, loss_dev, sizeof(float), hipMemcpyDeviceToHost, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));
  memcpy(g_err, saved, sizeof(saved));
  return status;
}

// Line-search solve on a ROW SHARD of the batch: see include/lasso_hip.h
int lasso_fista_solve_sharded(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                              int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t n_global, int64_t d,
                              int64_t k, int dtype, double alpha, double lr, int fast, int maxiter, double tol,
                              double eta_backtrack, lasso_allreduce_fn reduce, void* reduce_ctx, int32_t* iters_out,
                              float* last_delta_out, int32_t* trials_out, float* accepted_lr_out,
                              float* accepted_f_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 && dtype != LASSO_BF16) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!reduce) return fail(LASSO_ERR_BAD_ARG, "reduce callback is null");
  if (n <= 0 || n_global < n || d <= 0 || k <= 0 || maxiter <= 0) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (!x_dev || !w_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || (z0_dev && ldz0 < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (!(lr > 0.0) || !(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "need lr > 0 and alpha >= 0");
  if (!(eta_backtrack > 1.0)) return fail(LASSO_ERR_BAD_ARG, "eta must be > 1.");
  if (!fused_shape(d, k)) {                     // beyond the fused shapes: the unfused line search (fp32 tensors)
    if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "bf16 line search needs d<=%d, k<=%d", kFistaD, kFistaMaxK);
    if (iters_out) *iters_out = 0;
    if (last_delta_out) *last_delta_out = NAN;
    return solve_generic_backtracking((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0,
                                      (float*)z_out_dev, ldz, n, d, k, alpha, lr, fast, maxiter, tol, eta_backtrack,
                                      iters_out, last_delta_out, trials_out, accepted_lr_out, accepted_f_out,
                                      workspace_dev, workspace_bytes, (hipStream_t)stream, reduce, reduce_ctx, n_global);
  }
  if (n > (int64_t)INT32_MAX - kTileM) return fail(LASSO_ERR_UNSUPPORTED, "n too large");
  if (iters_out) *iters_out = 0;
  if (last_delta_out) *last_delta_out = NAN;
  return solve_backtracking(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, pad_k(k), dtype, alpha, lr,
                            fast, maxiter, tol, eta_backtrack, iters_out, last_delta_out, trials_out, accepted_lr_out,
                            accepted_f_out, workspace_dev, workspace_bytes, (hipStream_t)stream, reduce, reduce_ctx,
                            n_global);
}

// LASSO_SOLVE_ASYNC solve that returned LASSO_PENDING: enqueue the copy of what the persistent
// kernel leaves behind -- no synchronisation
int lasso_fista_solve_collect(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                              int32_t* out4_host, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 || !fused_shape(d, k) || n <= 0 || maxiter <= 0 || !(tol > 0.0) || !out4_host)
    return fail(LASSO_ERR_BAD_ARG, "no pending solve of this shape");
  const int kp = pad_k_solve(n, d, k);
  Workspace ws = carve(workspace_dev, n, k, kp, maxiter, true);
  if (!workspace_dev || workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", ws.bytes);
  LASSO_HIP_TRY(hipMemcpyAsync(out4_host, ws.stop_out, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return LASSO_OK;
}

float* lasso_fista_solve_deltas(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                                void* workspace_dev, size_t workspace_bytes) {
  if (dtype != LASSO_F32 || !fused_shape(d, k) || n <= 0 || maxiter <= 0 || maxiter > kChunkMax || !(tol > 0.0) ||
      !workspace_dev)
    return nullptr;
  Workspace ws = carve(workspace_dev, n, k, pad_k_solve(n, d, k), maxiter, true);
  return workspace_bytes < ws.bytes ? nullptr : ws.delta;
}

static int solve_verdict_impl(int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                              const float* sums_dev, int32_t* status_mapped, void* workspace_dev, size_t workspace_bytes,
                              void* stream) {
  if (dtype != LASSO_F32 || !fused_shape(d, k) || n <= 0 || n_global < n || maxiter <= 0 || maxiter > kChunkMax ||
      !(tol > 0.0))
    return fail(LASSO_ERR_BAD_ARG, "no pending sharded solve of this shape");
  Workspace ws = carve(workspace_dev, n, k, pad_k_solve(n, d, k), maxiter, true);
  if (!workspace_dev || workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", ws.bytes);
  const float budget = stop_budget<float>(n_global, k, tol);   // ista.py:64 on the whole batch
  hipLaunchKernelGGL(chunk_verdict_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sums_dev ? sums_dev : ws.delta,
                     maxiter, budget, ws.stop_out, status_mapped);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

int lasso_fista_solve_verdict(int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                              const float* sums_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return solve_verdict_impl(n, n_global, d, k, dtype, maxiter, tol, sums_dev, nullptr, workspace_dev, workspace_bytes, stream);
}

// The verdict launch an asynchronous LASSO_SOLVE_DEFER_VERDICT solve of this thread left out (it returned
// LASSO_PENDING_DEFERRED), on `stream` -- which the caller has ordered behind the solve's kernels (the EM loop: its side
// stream, behind a wave that polls a word the next launch of the solve's stream raises): the stop rule's launch is then
// off the step's dependent chain.  Same kernel, same sums, same words in `status_mapped` as the solve would have left.
int lasso_fista_solve_verdict_deferred(void* workspace_dev, int32_t* status_mapped, const int32_t* gate_word,
                                       int32_t gate_value, void* stream) {
  DeferredVerdict& dv = t_deferred_verdict;
  if (!status_mapped) return fail(LASSO_ERR_BAD_ARG, "status_mapped is NULL");
  if (!dv.armed || dv.workspace != workspace_dev)
    return fail(LASSO_ERR_BAD_ARG, "no deferred verdict for this workspace (LASSO_SOLVE_DEFER_VERDICT, same thread, one at a time)");
  dv.armed = false;
  hipLaunchKernelGGL(reduce_verdict_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dv.ps, dv.delta, dv.iters, dv.budget,
                     dv.out, status_mapped, gate_word, gate_value);
  LASSO_HIP_TRY(hipGetLastError());
  return LASSO_OK;
}

// the same verdict, its four words ALSO written to `status_mapped` (device-writable host memory): no collect call
int lasso_fista_solve_verdict_mapped(int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                                     const float* sums_dev, int32_t* status_mapped, void* workspace_dev,
                                     size_t workspace_bytes, void* stream) {
  if (!status_mapped) return fail(LASSO_ERR_BAD_ARG, "status_mapped is NULL");
  return solve_verdict_impl(n, n_global, d, k, dtype, maxiter, tol, sums_dev, status_mapped, workspace_dev, workspace_bytes,
                            stream);
}

// the synchronous form: collect, wait, decode
int lasso_fista_solve_finish(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                             int32_t* iters_out, float* last_delta_out, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 || !fused_shape(d, k) || n <= 0 || maxiter <= 0 || !(tol > 0.0))
    return fail(LASSO_ERR_BAD_ARG, "no pending solve of this shape");
  const int kp = pad_k_solve(n, d, k);
  Workspace ws = carve(workspace_dev, n, k, kp, maxiter, true);
  if (!workspace_dev || workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", ws.bytes);
  StopWords words;
  if (int s = read_stop_words(ws.stop_out, (hipStream_t)stream, &words)) return s;
  if (words.redo()) {
    if (iters_out) *iters_out = 0;
    if (last_delta_out) *last_delta_out = NAN;
    snprintf(g_err, sizeof(g_err), "asynchronous solve must be repeated (handshake gave up, or the rule fired before the end of the chunk)");
    return LASSO_WARN_ABORTED;
  }
  if (iters_out) *iters_out = words.iterations();
  if (last_delta_out) *last_delta_out = words.last_delta();
  return LASSO_OK;
}

// ---------------------------------------------------------------------------
size_t lasso_lipschitz_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0) return 0;
  return lipschitz_workspace_bytes(d, k);
}

int lasso_lipschitz(const void* w_dev, int64_t ldw, int64_t d, int64_t k, int dtype, double* l_out,
                    void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!w_dev || !workspace_dev || d <= 0 || k <= 0 || ldw < k)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (std::min(d, k) > 2048) return fail(LASSO_ERR_UNSUPPORTED, "min(d,k) > 2048");
  if (workspace_bytes < lipschitz_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lipschitz_workspace_bytes(d, k));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LASSO_F64) LASSO_HIP_TRY(launch_lipschitz_f64((const double*)w_dev, ldw, d, k, workspace_dev, 20, st));
  else LASSO_HIP_TRY(launch_lipschitz((const float*)w_dev, ldw, d, k, workspace_dev, 20, st));
  if (l_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(l_out, workspace_dev, sizeof(double), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
  }
  return LASSO_OK;
}

// ---------------------------------------------------------------------------
constexpr int kObjGenGrid = 1024;
// The tile kernel pads d to 256 columns of residual: at d <= 64 (8 x 8 patches) three quarters of its MFMAs multiply
// zeros, and the general GEMM + one reduction pass is the faster route (d=64, k=256, n=65536: 0.10 -> 0.07 ms).
static bool objective_unfused(int64_t d, int64_t k) { return !fused_shape(d, k) || d <= 64; }

size_t lasso_objective_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (n < 0 || d <= 0 || k <= 0) return 0;
  if (objective_unfused(d, k))     // unfused: residual [n][d] + partial pairs
    return align_up((size_t)std::max<int64_t>(n, 1) * d * 4) + align_up((size_t)kObjGenGrid * 2 * 4) + 256;
  const int kp = pad_k(k);
  const int64_t ntiles = (n + kTileM - 1) / kTileM;
  return align_up((size_t)kFistaD * kp * 4) + align_up((size_t)kp * kFistaD * 4) +
         align_up((size_t)std::max<int64_t>(ntiles, 1) * 2 * 4) + 256;
}

size_t lasso_objective_f64_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (n < 0 || d <= 0 || k <= 0) return 0;
  return f64::objective_workspace_bytes(n, d, k);
}

// float64 tensors: the loss as a device double (loss_dev) and / or rounded to a device float (loss32_dev)
static int objective_f64_impl(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z_dev,
                              int64_t ldz, int64_t n, int64_t d, int64_t k, double alpha, double* loss_dev,
                              float* loss32_dev, double* sums_dev, void* workspace_dev, size_t workspace_bytes,
                              void* stream) {
  if (n < 0 || d <= 0 || k <= 0) return fail(LASSO_ERR_BAD_ARG, "bad shape n=%lld d=%lld k=%lld", (long long)n,
                                              (long long)d, (long long)k);
  if (!x_dev || !w_dev || !z_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  return f64::objective((const double*)x_dev, ldx, (const double*)w_dev, ldw, (const double*)z_dev, ldz, n, d, k, alpha,
                        loss_dev, loss32_dev, sums_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int lasso_objective_f64(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z_dev, int64_t ldz,
                        int64_t n, int64_t d, int64_t k, double alpha, double* loss_dev, double* sums_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream) {
  return objective_f64_impl(x_dev, ldx, w_dev, ldw, z_dev, ldz, n, d, k, alpha, loss_dev, nullptr, sums_dev, workspace_dev,
                            workspace_bytes, stream);
}

static int objective_impl(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z_dev,
                          int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                          float* loss_dev, double* sums_dev, int max_workgroups, void* workspace_dev,
                          size_t workspace_bytes, void* stream) {
  if (dtype == LASSO_F64)      // (workspace: lasso_objective_f64_workspace_bytes; max_workgroups does not apply)
    return objective_f64_impl(x_dev, ldx, w_dev, ldw, z_dev, ldz, n, d, k, alpha, nullptr, loss_dev, sums_dev, workspace_dev,
                              workspace_bytes, stream);
  if (int s = check_common(n, d, k, dtype, /*allow_large=*/true)) return s;
  if (!x_dev || !w_dev || !z_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_objective_workspace_bytes(n, d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_objective_workspace_bytes(n, d, k));
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace_dev;
  if (objective_unfused(d, k)) {
    if (d > INT32_MAX / 2 || k > INT32_MAX / 2) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
    float* R = (float*)base;
    float* partials = (float*)(base + align_up((size_t)std::max<int64_t>(n, 1) * d * 4));
    double* sums = (double*)((char*)partials + align_up((size_t)kObjGenGrid * 2 * 4));
    if (n > 0)
      LASSO_HIP_TRY(launch_objective_generic((const float*)x_dev, ldx, (const float*)w_dev, ldw,
                                             (const float*)z_dev, ldz, (int)n, (int)d, (int)k, R, partials,
                                             kObjGenGrid, alpha, (double)n, sums_dev ? sums_dev : sums,
                                             loss_dev, st));
    return LASSO_OK;
  }
  const int kp = pad_k(k);
  const int ntiles = (int)((n + kTileM - 1) / kTileM);
  float* wp = (float*)base;
  float* wtp = (float*)(base + align_up((size_t)kFistaD * kp * 4));
  float* partials = (float*)((char*)wtp + align_up((size_t)kp * kFistaD * 4));
  double* sums = (double*)((char*)partials + align_up((size_t)std::max(ntiles, 1) * 2 * 4));
  hipLaunchKernelGGL(pack_w_kernel, dim3(kp / 32, kFistaD / 32), dim3(32, 8), 0, st,
                     (const float*)w_dev, ldw, (int)d, (int)k, kp, wp, wtp);
  LASSO_HIP_TRY(hipGetLastError());
  ObjectiveParams p;
  p.X = (const float*)x_dev; p.ldx = ldx; p.Wp = wp;
  p.Z = (const float*)z_dev; p.ldz = ldz; p.partials = partials;
  p.n = (int)n; p.d = (int)d; p.k = (int)k; p.ntiles = ntiles;
  const int cus = device_cus();
  if (cus <= 0) return fail(LASSO_ERR_HIP, "no HIP device");
  if (n > 0) {
    int grid = std::min(ntiles, cus);
    if (max_workgroups > 0) grid = std::max(1, std::min(grid, max_workgroups));
    LASSO_HIP_TRY(launch_objective(p, kp, grid, alpha, (double)n,
                                   sums_dev ? sums_dev : sums, loss_dev, st));
  }
  return LASSO_OK;
}

int lasso_objective(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z_dev,
                    int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                    float* loss_dev, double* sums_dev, void* workspace_dev, size_t workspace_bytes,
                    void* stream) {
  return objective_impl(x_dev, ldx, w_dev, ldw, z_dev, ldz, n, d, k, dtype, alpha, loss_dev, sums_dev, 0, workspace_dev,
                        workspace_bytes, stream);
}

// the same on at most `max_workgroups` workgroups of the fused kernel (0: as many as there are CUs): for a caller that
// runs the objective BESIDE latency-bound work on another stream (the EM loop's atom sweep) -- a quarter of the chip
// takes four times as long and disturbs its neighbour's memory round trips less (round 6: 8 us less on the sweep)
int lasso_objective_throttled(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z_dev,
                              int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                              float* loss_dev, double* sums_dev, int max_workgroups, void* workspace_dev,
                              size_t workspace_bytes, void* stream) {
  if (max_workgroups < 0) return fail(LASSO_ERR_BAD_ARG, "max_workgroups < 0");
  return objective_impl(x_dev, ldx, w_dev, ldw, z_dev, ldz, n, d, k, dtype, alpha, loss_dev, sums_dev, max_workgroups,
                        workspace_dev, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
static int gram_max_splits(int64_t d, int64_t k) {
  const int64_t one = k * std::max(k, d) * 4;
  return (int)std::min<int64_t>(128, std::max<int64_t>(16, ((int64_t)64 << 20) / std::max<int64_t>(one, 1)));
}

size_t lasso_gram_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (n < 0 || d <= 0 || k <= 0) return 0;
  // sample splits of the larger product: 16, more for small dictionaries (few output blocks: the splits are what
  // fills the chip -- k = 256, d = 64 ran on 48 workgroups with 16) up to 64 MB; the fused [A | B] kernel sizes its own
  return std::max((size_t)gram_max_splits(d, k) * (size_t)k * (size_t)std::max(k, d) * 4, gram_ab_scratch_bytes(d, k)) + 256;
}

static int gram_accumulate_impl(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n,
                                int64_t d, int64_t k, int dtype, float* a_dev, float* b_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream, int32_t* started_word,
                                int32_t started_value);
int lasso_gram_accumulate(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n,
                          int64_t d, int64_t k, int dtype, float* a_dev, float* b_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
  return gram_accumulate_impl(z_dev, ldz, x_dev, ldx, n, d, k, dtype, a_dev, b_dev, workspace_dev, workspace_bytes, stream,
                              nullptr, 0);
}
// the same products; the first launch raises *started_word = started_value when it STARTS (device memory): "everything
// enqueued on this stream before the call has completed", for a wave of another stream that polls the word
// (lasso_stream_wait_word) -- a start signal without an event record on this stream (~5 us between two kernels)
int lasso_gram_accumulate_signal(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n,
                                 int64_t d, int64_t k, int dtype, float* a_dev, float* b_dev,
                                 void* workspace_dev, size_t workspace_bytes, int32_t* started_word, int32_t started_value,
                                 void* stream) {
  if (!started_word) return fail(LASSO_ERR_BAD_ARG, "started_word is NULL");
  return gram_accumulate_impl(z_dev, ldz, x_dev, ldx, n, d, k, dtype, a_dev, b_dev, workspace_dev, workspace_bytes, stream,
                              started_word, started_value);
}
static int gram_accumulate_impl(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n,
                                int64_t d, int64_t k, int dtype, float* a_dev, float* b_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream, int32_t* started_word,
                                int32_t started_value) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!z_dev || !x_dev || !a_dev || !b_dev || n < 0 || d <= 0 || k <= 0 || ldz < k || ldx < d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (n > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "n too large");
  hipStream_t st = (hipStream_t)stream;
  const float* Z = (const float*)z_dev;
  // optional scratch for the split-n partial products (NULL = single pass)
  float* scratch = (workspace_dev && workspace_bytes >= lasso_gram_workspace_bytes(n, d, k))
                       ? (float*)workspace_dev : nullptr;
  const int cus = device_cus();
  if (scratch) {
    hipError_t e = hipSuccess;
    if (launch_gram_ab(Z, ldz, (int)k, (const float*)x_dev, ldx, (int)d, (int)n, a_dev, b_dev, scratch,
                       workspace_bytes - 256, cus, st, &e, started_word, started_value)) {
      LASSO_HIP_TRY(e);
      return LASSO_OK;
    }
  }
  if (scratch && !getenv("LASSO_GRAM_TWO_LAUNCHES")) {      // small dictionaries: one product launch, one fold (A/B: the env switch)
    hipError_t e = hipSuccess;
    if (launch_gram_ab128(Z, ldz, (int)k, (const float*)x_dev, ldx, (int)d, (int)n, a_dev, b_dev, scratch,
                          workspace_bytes - 256, cus, gram_max_splits(d, k), st, &e, started_word, started_value)) {
      LASSO_HIP_TRY(e);
      return LASSO_OK;
    }
  }
  // (the other product kernels do not carry the signal: a launch of its own in front of them)
  if (started_word) LASSO_HIP_TRY(launch_set_flag(started_word, started_value, st));
  const int smax = scratch ? gram_max_splits(d, k) : 1;
  const int sa = gram_splits((int)k, (int)k, (int)n, 1, cus, smax), sb = gram_splits((int)k, (int)d, (int)n, 0, cus, smax);
  LASSO_HIP_TRY(launch_gram_tn(Z, ldz, (int)k, Z, ldz, (int)k, (int)n, a_dev, k, 1, scratch, sa, st));
  LASSO_HIP_TRY(launch_gram_tn(Z, ldz, (int)k, (const float*)x_dev, ldx, (int)d, (int)n, b_dev, d, 0,
                               scratch, sb, st));
  return LASSO_OK;
}

size_t lasso_dict_sweep_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0 || d > kSweepMaxD || k > kSweepMaxK) return 0;
  const size_t dp = (size_t)(d + 255) / 256 * 256;
  return align_up((size_t)k * dp * 4) * 2 + align_up((size_t)kSweepBlock * dp * 4) + 256 +
         (dp == 256 ? align_up(sweep_persist_extra_bytes((int)k)) : 0);
}

// d_out_dev (pitch ldo): where the new dictionary goes -- d_dev itself (in place), or another buffer: d_dev is then only
// read (lasso_dict_sweep_async_to)
static int dict_sweep_impl(const float* a_dev, const float* b_dev, void* d_dev, int64_t ldd, int64_t d,
                           int64_t k, int dtype, double eps, int positive, const float* pool_dev,
                           int64_t pool_rows, int64_t pool_ld, uint64_t seed, int32_t* degenerate_dev,
                           int32_t* ndeg_out, int32_t* ndeg_mapped, void* workspace_dev, size_t workspace_bytes,
                           void* stream, void* d_out_dev = nullptr, int64_t ldo = 0, int32_t* started_word = nullptr,
                           int32_t started_value = 0) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!a_dev || !b_dev || !d_dev || !degenerate_dev || !workspace_dev || d <= 0 || k <= 0 || ldd < k)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (!d_out_dev) { d_out_dev = d_dev; ldo = ldd; }
  if (ldo < k) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (d_out_dev != d_dev) {         // two buffers: they must not overlap (the old atoms are read while the new ones land)
    const char* a0 = (const char*)d_dev, * a1 = a0 + ((size_t)(d - 1) * ldd + k) * 4;
    const char* b0 = (const char*)d_out_dev, * b1 = b0 + ((size_t)(d - 1) * ldo + k) * 4;
    if (a0 < b1 && b0 < a1) return fail(LASSO_ERR_BAD_ARG, "d_out_dev overlaps d_dev");
  }
  if (d > kSweepMaxD || k > kSweepMaxK)
    return fail(LASSO_ERR_UNSUPPORTED, "atom sweep: d=%lld k=%lld (d <= %d, k <= %d)", (long long)d,
                (long long)k, kSweepMaxD, kSweepMaxK);
  if (pool_dev && (pool_rows <= 0 || pool_ld < d)) return fail(LASSO_ERR_BAD_ARG, "bad pool");
  if (workspace_bytes < lasso_dict_sweep_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_dict_sweep_workspace_bytes(d, k));
  hipStream_t st = (hipStream_t)stream;
  const int dp = (int)((d + 255) / 256 * 256);     // row stride of U / Dt / dD: whole 256-feature panels
  char* base = (char*)workspace_dev;
  float* U = (float*)base;
  float* Dt = (float*)(base + align_up((size_t)k * dp * 4));
  float* dD = (float*)((char*)Dt + align_up((size_t)k * dp * 4));
  int* ndeg = (int*)((char*)dD + align_up((size_t)kSweepBlock * dp * 4));
  float* D = (float*)d_dev;
  float* Dnew = (float*)d_out_dev;
  // (ndeg is written by degenerate_fixup_kernel on every path: no clearing launch in front)
  // U[j][dd] = B[j][dd] - sum_i A[j][i] D[dd][i]          (k x d, zero padded to dp columns)
  // The single-launch sweep (dp == 256) reads its old atoms from D itself, never reads the padding of U, and its
  // last launch writes the new dictionary: no transposed copies, no clearing of U (four launches off the chain).
  const bool direct = dp == 256 && k % 4 == 0 && ldd % 4 == 0 && ((uintptr_t)D & 15) == 0 && ldo % 4 == 0 &&
                      ((uintptr_t)Dnew & 15) == 0;
  if (dp != d && !direct) LASSO_HIP_TRY(hipMemsetAsync(U, 0, (size_t)k * dp * 4, st));   // (d == dp: the product writes every column)
  void* const extra = dp == 256 ? (void*)((char*)ndeg + 256) : nullptr;
  // (the product's first workgroup also clears the single-launch sweep's flag words: no fill launch between them)
  int* const flag_words = extra ? sweep_persist_flags(extra, (int)k) : nullptr;
  LASSO_HIP_TRY(launch_gemm_nt_sub(a_dev, k, D, ldd, b_dev, d, U, dp, (int)k, (int)d, (int)k, st, 0, flag_words,
                                   flag_words ? 1024 : 0));
  // Dt[j][dd] = D[dd][j]  (zero padded to dp features)
  if (!direct) LASSO_HIP_TRY(launch_transpose_pad(D, ldd, (int)d, (int)k, Dt, dp, (int)k, dp, st));
  // "the sweep starts now": a word another stream's wave polls (work that should run BESIDE the sweep, which leaves most
  // of the chip idle -- the EM loop's objective on large batches); one 4-us launch on this stream
  if (started_word) LASSO_HIP_TRY(launch_set_flag(started_word, started_value, st));
  SweepParams p;
  p.flags_cleared = flag_words != nullptr;
  p.Dsrc = direct ? D : nullptr; p.ldd = ldd;
  p.Dout = direct ? Dnew : nullptr; p.ldo = ldo;
  p.A = a_dev; p.lda = k; p.U = U; p.ldu = dp; p.Dt = Dt; p.dD = dD; p.dp = dp;
  p.pool = pool_dev; p.pool_rows = (int)pool_rows; p.pool_ld = pool_ld; p.seed = seed;
  p.degenerate = degenerate_dev; p.ndeg_in_out = ndeg; p.ndeg_mirror = ndeg_mapped;
  p.wait_word = nullptr; p.wait_value = 0;
  p.k = (int)k; p.d = (int)d; p.eps = (float)eps; p.positive = positive;
  float* dt_new = Dt;
  LASSO_HIP_TRY(launch_dict_sweep(p, st, extra, &dt_new));
  // D[dd][j] = Dt[j][dd]
  if (!direct) LASSO_HIP_TRY(launch_transpose_pad(dt_new, dp, (int)k, (int)d, Dnew, ldo, (int)d, (int)k, st));
  if (ndeg_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(ndeg_out, ndeg, sizeof(int), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
  }
  return LASSO_OK;
}

int lasso_dict_sweep(const float* a_dev, const float* b_dev, void* d_dev, int64_t ldd, int64_t d,
                     int64_t k, int dtype, double eps, int positive, const float* pool_dev,
                     int64_t pool_rows, int64_t pool_ld, uint64_t seed, int32_t* degenerate_dev,
                     int32_t* ndeg_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return dict_sweep_impl(a_dev, b_dev, d_dev, ldd, d, k, dtype, eps, positive, pool_dev, pool_rows, pool_ld, seed,
                         degenerate_dev, ndeg_out, nullptr, workspace_dev, workspace_bytes, stream);
}

// the same sweep without a host wait: the count of degenerate atoms goes to `ndeg_mapped`, a device-writable HOST word
// (pinned, mapped), written by the sweep's last kernel -- valid once an event recorded behind this call has completed
int lasso_dict_sweep_async(const float* a_dev, const float* b_dev, void* d_dev, int64_t ldd, int64_t d,
                           int64_t k, int dtype, double eps, int positive, const float* pool_dev,
                           int64_t pool_rows, int64_t pool_ld, uint64_t seed, int32_t* degenerate_dev,
                           int32_t* ndeg_mapped, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!ndeg_mapped) return fail(LASSO_ERR_BAD_ARG, "ndeg_mapped is NULL");
  return dict_sweep_impl(a_dev, b_dev, d_dev, ldd, d, k, dtype, eps, positive, pool_dev, pool_rows, pool_ld, seed,
                         degenerate_dev, nullptr, ndeg_mapped, workspace_dev, workspace_bytes, stream);
}

// lasso_dict_sweep_async with the new dictionary written to ANOTHER buffer: d_dev is only read, so the call may be
// enqueued before the host knows whether the step it belongs to stands (an EM loop's E-step verdict, the previous sweep's
// count of degenerate atoms: a step that has to be repeated simply keeps d_dev), and work on another stream may go on
// reading the old dictionary beside it (the objective of dict_learning.py:39) -- DESIGN.md 3.3h
int lasso_dict_sweep_async_to(const float* a_dev, const float* b_dev, const void* d_dev, int64_t ldd, void* d_out_dev,
                              int64_t ldo, int64_t d, int64_t k, int dtype, double eps, int positive,
                              const float* pool_dev, int64_t pool_rows, int64_t pool_ld, uint64_t seed,
                              int32_t* degenerate_dev, int32_t* ndeg_mapped, int32_t* started_word,
                              int32_t started_value, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!ndeg_mapped) return fail(LASSO_ERR_BAD_ARG, "ndeg_mapped is NULL");
  if (!d_out_dev || d_out_dev == d_dev) return fail(LASSO_ERR_BAD_ARG, "d_out_dev must be another buffer");
  return dict_sweep_impl(a_dev, b_dev, const_cast<void*>(d_dev), ldd, d, k, dtype, eps, positive, pool_dev, pool_rows, pool_ld,
                         seed, degenerate_dev, nullptr, ndeg_mapped, workspace_dev, workspace_bytes, stream, d_out_dev, ldo,
                         started_word, started_value);
}

// ---- pipelined constrained M-step (ABI 7) -------------------------------------------------------
// workspace = [the sweep's workspace (lasso_dict_sweep_workspace_bytes) | the Gram partial sums of every block row]
namespace {
struct PipeWs { SweepParams p; void* extra; float* gram; MstepPipePlan plan; size_t bytes; };
// the SweepParams of every call of one pipelined M-step (the same carve of the same workspace each time)
bool pipe_carve(int64_t n, int64_t d, int64_t k, void* workspace_dev, PipeWs* w) {
  const int cus = device_cus();
  w->plan = mstep_pipe_plan(n, d, k, cus);
  if (w->plan.nstages == 0) return false;
  const size_t sweep = align_up(lasso_dict_sweep_workspace_bytes(d, k));
  w->bytes = sweep + w->plan.scratch_bytes + 256;
  const int dp = 256;
  char* base = (char*)workspace_dev;
  float* U = (float*)base;
  float* Dt = (float*)(base + align_up((size_t)k * dp * 4));
  float* dD = (float*)((char*)Dt + align_up((size_t)k * dp * 4));
  int* ndeg = (int*)((char*)dD + align_up((size_t)kSweepBlock * dp * 4));
  w->extra = (void*)((char*)ndeg + 256);
  w->gram = (float*)(base + sweep);
  SweepParams& p = w->p;
  p.flags_cleared = 1;
  p.U = U; p.ldu = dp; p.Dt = Dt; p.dD = dD; p.dp = dp;
  p.pool = nullptr; p.pool_rows = 0; p.pool_ld = 0; p.seed = 0;
  p.ndeg_in_out = ndeg; p.ndeg_mirror = nullptr;
  p.wait_word = nullptr; p.wait_value = 0;
  p.k = (int)k; p.d = (int)d;
  return true;
}
}  // namespace

int lasso_mstep_pipe_stages(int64_t n, int64_t d, int64_t k) {
  if (n <= 0 || d <= 0 || k <= 0) return 0;
  return mstep_pipe_plan(n, d, k, device_cus()).nstages;
}

int lasso_mstep_pipe_stage_rows(int64_t n, int64_t d, int64_t k, int stage, int64_t* row_lo, int64_t* row_hi) {
  if (n <= 0 || d <= 0 || k <= 0 || !row_lo || !row_hi) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  const MstepPipePlan pl = mstep_pipe_plan(n, d, k, device_cus());
  if (stage < 0 || stage >= pl.nstages) return fail(LASSO_ERR_BAD_ARG, "stage %d of %d", stage, pl.nstages);
  *row_lo = 256 * (int64_t)pl.lo[stage];
  *row_hi = 256 * (int64_t)pl.hi[stage];
  return LASSO_OK;
}

size_t lasso_mstep_pipe_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  PipeWs w;
  if (n <= 0 || d <= 0 || k <= 0 || !pipe_carve(n, d, k, nullptr, &w)) return 0;
  return w.bytes;
}

int lasso_mstep_pipe_gram(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n, int64_t d,
                          int64_t k, int dtype, float* ab_dev, int64_t ldab, int stage, void* workspace_dev,
                          size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  PipeWs w;
  if (!ab_dev || !workspace_dev || n < 0 || (n > 0 && (!z_dev || !x_dev || ldz < k || ldx < d)) || ldab < k + d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  // (the layout rules of include/lasso_hip.h come first: they hold for every shape and need no device)
  if ((ldab & 3) || ((uintptr_t)ab_dev & 15)) return fail(LASSO_ERR_BAD_ARG, "[A | B] must be 16-byte aligned, pitch a multiple of 4");
  if (n > 0 && ((ldz & 3) || (ldx & 3) || ((uintptr_t)z_dev & 15) || ((uintptr_t)x_dev & 15)))
    return fail(LASSO_ERR_BAD_ARG, "Z and X must be 16-byte aligned, pitches multiples of 4");
  if (!pipe_carve(std::max<int64_t>(n, 1), d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for n=%lld d=%lld k=%lld",
                                                           (long long)n, (long long)d, (long long)k);
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  if (stage < 0 || stage >= w.plan.nstages) return fail(LASSO_ERR_BAD_ARG, "stage %d of %d", stage, w.plan.nstages);
  // the head's launch also clears the sweep's flag words: it sits in front of every launch that sets or reads them
  int* const flags = stage == 0 ? sweep_persist_flags(w.extra, (int)k) : nullptr;
  if (n == 0) {
    // a rank without rows (it still runs the identical sweep on the all-reduced [A | B]): zero contributions, and the
    // flag words cleared all the same -- stale "rows complete" words would let the gated sweep run ahead of its rows
    const int lo = w.plan.lo[stage], hi = w.plan.hi[stage];
    LASSO_HIP_TRY(hipMemset2DAsync(ab_dev + (int64_t)256 * lo * ldab, ldab * 4, 0, (size_t)(k + d) * 4, (size_t)256 * (hi - lo),
                                   (hipStream_t)stream));
    if (flags) LASSO_HIP_TRY(hipMemsetAsync(flags, 0, 4096, (hipStream_t)stream));
    return LASSO_OK;
  }
  LASSO_HIP_TRY(launch_gram_rows((const float*)z_dev, ldz, (int)k, (const float*)x_dev, ldx, (int)d, (int)n, ab_dev, ldab,
                                 stage, w.plan, w.gram, flags, flags ? 1024 : 0, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_stream_wait_word(const int32_t* word, int32_t value, int host_memory, void* stream) {
  if (!word) return fail(LASSO_ERR_BAD_ARG, "word is NULL");
  LASSO_HIP_TRY(launch_wait_word(word, value, host_memory, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_mstep_pipe_wait(int64_t n, int64_t d, int64_t k, int seq, void* workspace_dev, size_t workspace_bytes,
                          void* stream) {
  PipeWs w;
  if (!workspace_dev) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (!pipe_carve(n, d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for this shape");
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  LASSO_HIP_TRY(launch_wait_word(sweep_pipe_words(w.extra, (int)k) + 1, seq, 0, (hipStream_t)stream));
  return LASSO_OK;
}

// the word lasso_mstep_pipe_wait polls (device memory inside the workspace; NULL: no pipelined M-step for the shape) --
// for launches behind the wait that must re-check it themselves (lasso_fista_solve_verdict_deferred's gate)
const int32_t* lasso_mstep_pipe_head_word(int64_t n, int64_t d, int64_t k, void* workspace_dev, size_t workspace_bytes) {
  PipeWs w;
  if (!workspace_dev || !pipe_carve(n, d, k, workspace_dev, &w) || workspace_bytes < w.bytes) return nullptr;
  return sweep_pipe_words(w.extra, (int)k) + 1;
}

int lasso_mstep_pipe_rows(const float* ab_dev, int64_t ldab, const void* d_dev, int64_t ldd, int64_t n, int64_t d,
                          int64_t k, int dtype, int stage, int seq, void* workspace_dev, size_t workspace_bytes,
                          void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  PipeWs w;
  if (!ab_dev || !d_dev || !workspace_dev || ldd < k || ldab < k + d) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if ((ldab & 3) || (ldd & 3) || ((uintptr_t)ab_dev & 15) || ((uintptr_t)d_dev & 15))
    return fail(LASSO_ERR_BAD_ARG, "[A | B] and the dictionary must be 16-byte aligned, pitches multiples of 4");
  if (!pipe_carve(n, d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for this shape");
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  if (stage < 0 || stage >= w.plan.nstages) return fail(LASSO_ERR_BAD_ARG, "stage %d of %d", stage, w.plan.nstages);
  hipStream_t st = (hipStream_t)stream;
  const int lo = w.plan.lo[stage], hi = w.plan.hi[stage];
  const int64_t r0 = 256 * (int64_t)lo;
  // U[j] = B[j] - sum_i A[j][i] D[:, i]   for the rows j of the block (dict_learning.py:82 in Gram form)
  // (uprod_rows_kernel: bitwise launch_gemm_nt_sub's product; its last workgroup raises the block row's flag)
  // (the head: `seq` into the word lasso_mstep_pipe_wait watches -- the head of the chain is through; the other
  // stages: the flags of their block rows for the running sweep)
  int* const words = sweep_pipe_words(w.extra, (int)k);
  int* const flag = stage > 0 ? sweep_persist_flags(w.extra, (int)k) + kSweepRowFlag + lo : words + 1;
  LASSO_HIP_TRY(launch_uprod_rows(ab_dev + r0 * ldab, ldab, (const float*)d_dev, ldd, ab_dev + r0 * ldab + k, ldab,
                                  w.p.U + r0 * 256, 256, 256 * (hi - lo), (int)k, words + 8 + stage, flag,
                                  stage > 0 ? hi - lo : 1, stage > 0 ? 1 : seq, st));
  return LASSO_OK;
}

int lasso_mstep_pipe_sweep(const float* ab_dev, int64_t ldab, const void* d_dev, int64_t ldd, int64_t n, int64_t d,
                           int64_t k, int dtype, double eps, int positive, int32_t* degenerate_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  PipeWs w;
  if (!ab_dev || !d_dev || !degenerate_dev || !workspace_dev || ldd < k || ldab < k + d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if ((k & 3) || (ldd & 3) || ((uintptr_t)d_dev & 15)) return fail(LASSO_ERR_BAD_ARG, "the dictionary must be 16-byte aligned, pitch a multiple of 4");
  if (!pipe_carve(n, d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for this shape");
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  SweepParams& p = w.p;
  p.A = ab_dev; p.lda = ldab;
  p.Dsrc = (const float*)d_dev; p.ldd = ldd;
  p.Dout = (float*)const_cast<void*>(d_dev); p.ldo = ldd;      // (only launch_sweep_fixup writes it: lasso_mstep_pipe_finish)
  p.degenerate = degenerate_dev; p.eps = (float)eps; p.positive = positive;
  float* dt_new = nullptr;
  LASSO_HIP_TRY(launch_sweep_gated(p, w.extra, 256 / kSweepBlock, w.plan.hi[0], &dt_new, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_mstep_pipe_signal(int64_t n, int64_t d, int64_t k, int seq, void* workspace_dev, size_t workspace_bytes,
                            void* stream) {
  PipeWs w;
  if (!workspace_dev) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (!pipe_carve(n, d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for this shape");
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  LASSO_HIP_TRY(launch_set_flag(sweep_pipe_words(w.extra, (int)k) + 2, seq, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_mstep_pipe_finish(void* d_dev, int64_t ldd, int64_t n, int64_t d, int64_t k, int dtype, double eps, int positive,
                            int32_t* degenerate_dev, int32_t* ndeg_mapped, int wait_seq, void* workspace_dev,
                            size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  PipeWs w;
  if (!d_dev || !degenerate_dev || !workspace_dev || ldd < k) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (!pipe_carve(n, d, k, workspace_dev, &w)) return fail(LASSO_ERR_UNSUPPORTED, "no pipelined M-step for this shape");
  if (workspace_bytes < w.bytes) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", w.bytes);
  SweepParams& p = w.p;
  p.A = nullptr; p.lda = 0;
  p.Dsrc = (const float*)d_dev; p.ldd = ldd;
  p.Dout = (float*)d_dev; p.ldo = ldd;
  p.degenerate = degenerate_dev; p.eps = (float)eps; p.positive = positive;
  p.ndeg_mirror = ndeg_mapped;
  if (wait_seq != 0) { p.wait_word = sweep_pipe_words(w.extra, (int)k) + 2; p.wait_value = wait_seq; }
  p.Dt = (float*)w.extra;                      // the single-launch sweep's new atoms (SweepPersist::DtN)
  LASSO_HIP_TRY(launch_sweep_fixup(p, (hipStream_t)stream));
  return LASSO_OK;
}

// Device address of the sweep's count of degenerate atoms inside `workspace_dev` (valid once the sweep enqueued
// with this workspace has run): a caller that does not want lasso_dict_sweep's host wait (ndeg_out = NULL) copies
// these 4 bytes at its own synchronisation instead of reducing the k flags.
int32_t* lasso_dict_sweep_count(int64_t d, int64_t k, void* workspace_dev, size_t workspace_bytes) {
  if (!workspace_dev || d <= 0 || k <= 0 || d > kSweepMaxD || k > kSweepMaxK ||
      workspace_bytes < lasso_dict_sweep_workspace_bytes(d, k))
    return nullptr;
  const int dp = (int)((d + 255) / 256 * 256);
  char* base = (char*)workspace_dev;
  return (int32_t*)(base + 2 * align_up((size_t)k * dp * 4) + align_up((size_t)kSweepBlock * dp * 4));
}

// ---- init='transpose': z0 = x W, sparse_encode.py:24-25 --------------------------------------
size_t lasso_init_transpose_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0) return 0;
  return (size_t)k * (size_t)d * sizeof(float) + 256;
}

int lasso_init_transpose(int64_t n, int64_t d, int64_t k, int dtype, const void* x_dev, int64_t ldx,
                         const void* w_dev, int64_t ldw, void* z0_dev, int64_t ldz, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (!w_dev || !workspace_dev || (n > 0 && (!x_dev || !z0_dev))) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_init_transpose_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_init_transpose_workspace_bytes(d, k));
  if (n == 0) return LASSO_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == LASSO_F64)                                   // reads W as it is: the workspace is not used
    return f64::init_transpose((const double*)x_dev, ldx, (const double*)w_dev, ldw, (double*)z0_dev, ldz, n, d, k, st);
  float* const Wt = (float*)workspace_dev;                  // [k][d]: z0 = x Wt^T on the NT GEMM
  LASSO_HIP_TRY(launch_transpose_pad((const float*)w_dev, ldw, (int)d, (int)k, Wt, d, (int)k, (int)d, st));
  LASSO_HIP_TRY(launch_gemm_nt_sub((const float*)x_dev, ldx, Wt, d, nullptr, 0, (float*)z0_dev, ldz, (int)n, (int)k,
                                   (int)d, st, /*add=*/1));
  return LASSO_OK;
}

// ---- GPSR-Basic: gpsr_basic, gpsr.py:209-365 (csrc/gpsr.hip) ------------------------------------
size_t lasso_gpsr_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return 0;
  return gpsr::workspace_bytes(n, d, k);
}

// the option, trace and result checks the two GPSR entry points share; clears the result
static int check_gpsr_request(const lasso_gpsr_options* o, lasso_gpsr_result* res, bool has_z0, int defined_bits) {
  if (o->reserved & ~defined_bits) return fail(LASSO_ERR_BAD_ARG, "GPSR: an undefined bit of reserved");
  if (o->stop_criterion < 0 || o->stop_criterion > 4) return fail(LASSO_ERR_BAD_ARG, "Unknown stopping criterion");
  if (!has_z0 && o->init == 1) return fail(LASSO_ERR_UNSUPPORTED, "GPSR: init=1 (random start) is passed as z0");
  if (!has_z0 && o->init != 0 && o->init != 2) return fail(LASSO_ERR_BAD_ARG, "Unknown initialization option");
  if (o->continuation && o->cont_steps < 1) return fail(LASSO_ERR_BAD_ARG, "cont_steps < 1");
  if (!(o->lambda_backtrack > 0.0 && o->lambda_backtrack < 1.0)) return fail(LASSO_ERR_BAD_ARG, "lambda_backtrack outside (0, 1)");
  if (const lasso_gpsr_trace* t = res->trace) {
    if ((t->capacity > 0 && (!t->lambda || !t->lambda0 || !t->trials || !t->objective || !t->criterion || !t->nz)) ||
        (t->step_capacity > 0 && (!t->step_tau || !t->step_f0 || !t->step_nz0 || !t->step_end)) ||
        (t->db_capacity > 0 && (!t->db_rr || !t->db_conv)) || t->capacity < 0 || t->step_capacity < 0 || t->db_capacity < 0)
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  res->n_iter = res->flags = res->steps = res->db_iters = 0;
  res->objective = res->main_objective = 0.0;
  res->main_rr = res->main_l1 = res->db_rr = res->db_l1 = 0.0f;
  res->main_nz = res->db_nz = 0;
  return LASSO_OK;
}

int lasso_gpsr_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                     void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                     const lasso_gpsr_options* o, lasso_gpsr_result* res, void* workspace_dev, size_t workspace_bytes,
                     void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "GPSR: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (int s = check_gpsr_request(o, res, z0_dev != nullptr, LASSO_FORCE_BLOCKS_128)) return s;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || (z0_dev && ldz0 < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_gpsr_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_gpsr_workspace_bytes(n, d, k, dtype));
  return gpsr::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev,
                     ldz, n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

// ---- orthant-wise Newton: orthant_wise_newton.py:33-160 (csrc/own.hip) ----------------------
size_t lasso_own_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || k > 4096 || n > INT32_MAX || d > INT32_MAX) return 0;
  return own::workspace_bytes(n, d, k);
}

int lasso_own_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                    void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                    const lasso_own_options* o, lasso_own_result* res, void* workspace_dev, size_t workspace_bytes,
                    void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "orthant-wise Newton: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (k > 4096) return fail(LASSO_ERR_UNSUPPORTED, "orthant-wise Newton: k=%lld > 4096", (long long)k);
  if (!(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha < 0");
  if (o->line_search < 0 || o->line_search > 2)
    return fail(LASSO_ERR_BAD_ARG, "line_search must be one of 0 (brent), 1 (backtrack), 2 (none)");
  if (o->maxiter < 0 || (o->line_search == 1 && o->ls_maxiter < 1)) return fail(LASSO_ERR_BAD_ARG, "maxiter < 0 or ls_maxiter < 1");
  if (const lasso_own_trace* t = res->trace) {
    if (t->capacity < 0 || t->eval_capacity < 0 || (t->capacity > 0 && (!t->t || !t->ls_iters || !t->f || !t->delta_z)) ||
        (t->eval_capacity > 0 && (!t->eval_iter || !t->eval_t || !t->eval_f)))
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  res->n_iter = res->flags = res->cholesky_info = res->ls_failures = 0;
  res->f0 = res->f_final = 0.0;
  if (res->trace) res->trace->eval_count = 0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_own_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_own_workspace_bytes(n, d, k, dtype));
  return own::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev, ldz,
                    n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

// ---- OWL-QN: lasso/nonlinear/owlqn.py:80-199 with fun = 0.5 |z W^T - x|^2 (csrc/owlqn.hip) ----
size_t lasso_owlqn_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int64_t pairs) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX || pairs < 0 ||
      pairs > owlqn::kMaxPairs)
    return 0;
  return owlqn::workspace_bytes(n, d, k, pairs);
}

// both OWL-QN entry points: the refusals, then the driver on the objective's family
static int owlqn_entry(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                       void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha, int family,
                       const lasso_owlqn_options* o, lasso_owlqn_result* res, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "OWL-QN: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (!(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha < 0");
  if (o->line_search < 0 || o->line_search > 2)
    return fail(LASSO_ERR_BAD_ARG, "line_search must be one of 0 (brent), 1 (backtrack), 2 (none)");
  if (o->maxiter < 0 || o->history_size < 1 || (o->line_search == 1 && o->ls_maxiter < 1))
    return fail(LASSO_ERR_BAD_ARG, "maxiter < 0, history_size < 1 or ls_maxiter < 1");
  if (const lasso_owlqn_trace* t = res->trace) {
    if (t->capacity < 0 || t->eval_capacity < 0 ||
        (t->capacity > 0 && (!t->t || !t->ls_iters || !t->f || !t->delta_x || !t->pairs || !t->skipped || !t->h_diag)) ||
        (t->eval_capacity > 0 && (!t->eval_iter || !t->eval_t || !t->eval_f)))
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  const int pairs = owlqn::pairs_needed(*o);
  if (pairs > owlqn::kMaxPairs)
    return fail(LASSO_ERR_UNSUPPORTED, "OWL-QN: min(history_size, maxiter - 1) = %d > %d pairs", pairs, owlqn::kMaxPairs);
  res->n_iter = res->flags = res->ls_failures = res->reserved = 0;
  res->f0 = res->f_final = res->direction_ms = res->direction_bytes = 0.0;
  if (res->trace) res->trace->eval_count = 0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_owlqn_workspace_bytes(n, d, k, dtype, pairs))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_owlqn_workspace_bytes(n, d, k, dtype, pairs));
  return owlqn::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev, ldz,
                      n, d, k, alpha, family, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

int lasso_owlqn_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                      void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                      const lasso_owlqn_options* o, lasso_owlqn_result* res, void* workspace_dev, size_t workspace_bytes,
                      void* stream) {
  return owlqn_entry(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, dtype, alpha, owlqn::kFamilyRss, o, res,
                     workspace_dev, workspace_bytes, stream);
}

// ---- OWL-QN on a generalised-linear objective: fun = sum loss(z W^T, x) (csrc/owlqn.hip's link epilogues) ----
int lasso_owlqn_glm_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                          void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha, int family,
                          const lasso_owlqn_options* o, lasso_owlqn_result* res, void* workspace_dev, size_t workspace_bytes,
                          void* stream) {
  if (family != LASSO_GLM_BERNOULLI)
    return fail(LASSO_ERR_UNSUPPORTED, "OWL-QN: family %d (LASSO_GLM_BERNOULLI = %d only)", family, LASSO_GLM_BERNOULLI);
  return owlqn_entry(x_dev, ldx, w_dev, ldw, z0_dev, ldz0, z_out_dev, ldz, n, d, k, dtype, alpha, family, o, res, workspace_dev,
                     workspace_bytes, stream);
}

// ---- BFGS iterated ridge: lasso/nonlinear/iterative_ridge_bfgs.py:45-140 with f = 0.5 |z W^T - x|^2 (csrc/irbfgs.hip) ----
size_t lasso_irbfgs_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX ||
      k > batch_solve::tier_cap(LASSO_F32, LASSO_BATCH_TIER_GENERAL))
    return 0;
  return irbfgs::workspace_bytes(n, d, k);
}

int lasso_irbfgs_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                       void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                       const lasso_irbfgs_options* o, lasso_irbfgs_result* res, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "iterative_ridge_bfgs: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  const int cap = batch_solve::tier_cap(LASSO_F32, LASSO_BATCH_TIER_GENERAL);
  if (k > cap) return fail(LASSO_ERR_UNSUPPORTED, "iterative_ridge_bfgs: k=%lld > %d", (long long)k, cap);
  if (!(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha < 0");
  if ((o->reserved & ~(int64_t)(2 | LASSO_FORCE_BLOCKS_128)) != 0)
    return fail(LASSO_ERR_BAD_ARG, "iterative_ridge_bfgs: unknown bit of reserved");
  if (o->maxiter < 0 || o->line_search < 0 || o->line_search > 1 || !(o->lr >= 0.0) || !(o->xtol >= 0.0) ||
      !(o->tikhonov >= 0.0) || !(o->eps >= 0.0))
    return fail(LASSO_ERR_BAD_ARG, "maxiter, lr, xtol, tikhonov, eps >= 0 and line_search 0 / 1 are required");
  if (const lasso_irbfgs_trace* t = res->trace) {
    if (t->capacity < 0 || t->eval_capacity < 0 ||
        (t->capacity > 0 && (!t->t || !t->ls_iters || !t->f || !t->delta_x || !t->invalid_rows || !t->lu)) ||
        (t->eval_capacity > 0 && (!t->eval_iter || !t->eval_t || !t->eval_f)))
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  res->n_iter = res->flags = res->lu_count = res->reserved = 0;
  res->f0 = res->f_final = res->row_ms = res->row_bytes = res->solve_ms = 0.0;
  res->bad_row = -1;
  if (res->trace) res->trace->eval_count = 0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_irbfgs_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_irbfgs_workspace_bytes(n, d, k, dtype));
  return irbfgs::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev, ldz,
                       n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

int lasso_irbfgs_update(void* b_dev, const void* x_dev, const void* g_dev, void* x_prev_dev, void* g_prev_dev,
                        void* system_dev, void* rhs_dev, int32_t* valid_dev, int64_t n, int64_t k, int dtype, double alpha,
                        double tikhonov, double eps, int mode, int first, int max_workgroups, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "iterative_ridge_bfgs: dtype %d (fp32 tensors only)", dtype);
  if (n < 0 || k <= 0 || n > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  const int cap = batch_solve::tier_cap(LASSO_F32, LASSO_BATCH_TIER_GENERAL);
  if (k > cap) return fail(LASSO_ERR_UNSUPPORTED, "iterative_ridge_bfgs: k=%lld > %d", (long long)k, cap);
  if (!(alpha >= 0.0) || !(tikhonov >= 0.0) || !(eps >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha, tikhonov, eps >= 0 are required");
  if (mode < 0 || mode > 2 || max_workgroups < 0) return fail(LASSO_ERR_BAD_ARG, "mode must be 0, 1 or 2 and max_workgroups >= 0");
  if (n == 0) return LASSO_OK;
  if (!b_dev || !x_dev || !g_dev || !x_prev_dev || !g_prev_dev || !system_dev || !rhs_dev || !valid_dev)
    return fail(LASSO_ERR_BAD_ARG, "null pointer");
  return irbfgs::update((float*)b_dev, (const float*)x_dev, (const float*)g_dev, (float*)x_prev_dev, (float*)g_prev_dev,
                        (float*)system_dev, (float*)rhs_dev, valid_dev, n, k, alpha, tikhonov, eps, mode, first, max_workgroups,
                        static_cast<hipStream_t>(stream));
}

// ---- iterated ridge: iterative_ridge.py:11-141 (csrc/iter_ridge.hip) -------------------------
size_t lasso_iter_ridge_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || k > 1024 || n > INT32_MAX || d > INT32_MAX) return 0;
  return iter_ridge::workspace_bytes(n, d, k);
}

int lasso_iter_ridge_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                           void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                           const lasso_iter_ridge_options* o, lasso_iter_ridge_result* res, void* workspace_dev,
                           size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "iterated ridge: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (k > 1024) return fail(LASSO_ERR_UNSUPPORTED, "iterated ridge: k=%lld > 1024", (long long)k);
  if (!(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha < 0");
  if ((o->reserved & ~(int64_t)LASSO_FORCE_BLOCKS_128) != 0)
    return fail(LASSO_ERR_BAD_ARG, "iterated ridge: only bit 3 of reserved is defined");
  if (o->maxiter < 0 || o->line_search < 0 || o->line_search > 1 || !(o->tol >= 0.0) || !(o->tikhonov >= 0.0) || !(o->eps >= 0.0))
    return fail(LASSO_ERR_BAD_ARG, "maxiter, tol, tikhonov, eps >= 0 and line_search 0 / 1 are required");
  if (const lasso_iter_ridge_trace* t = res->trace) {
    if (t->capacity < 0 || t->eval_capacity < 0 ||
        (t->capacity > 0 && (!t->f || !t->update || !t->t || !t->ls_evals || !t->support_max || !t->support_mean)) ||
        (t->eval_capacity > 0 && (!t->eval_iter || !t->eval_t || !t->eval_f)))
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  res->n_iter = 0;
  res->status = LASSO_ITER_RIDGE_MAXITER;
  res->f0 = res->f_final = 0.0;
  res->bad_row = -1;
  res->bad_minor = res->pad_ = 0;
  if (res->trace) res->trace->eval_count = 0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_iter_ridge_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_iter_ridge_workspace_bytes(n, d, k, dtype));
  return iter_ridge::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev,
                           ldz, n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

int lasso_iter_ridge_rows(const void* g_dev, int64_t ldg, const void* rhs_dev, int64_t ldr, const void* z_dev, int64_t ldz,
                          void* z_sol_dev, int64_t ldzs, int64_t n, int64_t k, int dtype, double alpha, double tikhonov,
                          double eps, int64_t* bad_row_out, int32_t* bad_minor_out, int32_t* support_max_out,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "iterated ridge: dtype %d (fp32 tensors only)", dtype);
  if (!bad_row_out || !bad_minor_out) return fail(LASSO_ERR_BAD_ARG, "null result");
  if (n < 0 || k <= 0 || n > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (k > 1024) return fail(LASSO_ERR_UNSUPPORTED, "iterated ridge: k=%lld > 1024", (long long)k);
  if (!(alpha >= 0.0) || !(tikhonov >= 0.0) || !(eps >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha, tikhonov, eps >= 0 are required");
  *bad_row_out = -1;
  *bad_minor_out = 0;
  if (support_max_out) *support_max_out = 0;
  if (n == 0) return LASSO_OK;
  if (!g_dev || !rhs_dev || !z_dev || !z_sol_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldg < k || ldr < k || ldz < k || ldzs < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_iter_ridge_workspace_bytes(n, 1, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_iter_ridge_workspace_bytes(n, 1, k, dtype));
  return iter_ridge::rows((const float*)g_dev, ldg, (const float*)rhs_dev, ldr, (const float*)z_dev, ldz, (float*)z_sol_dev,
                          ldzs, n, k, alpha, tikhonov, eps, bad_row_out, bad_minor_out, support_max_out, workspace_dev,
                          static_cast<hipStream_t>(stream));
}

// ---- Split Bregman: split_bregman.py:5-86 (csrc/split_bregman.hip) ---------------------------
size_t lasso_split_bregman_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || k > 4096 || n > INT32_MAX || d > INT32_MAX) return 0;
  return split_bregman::workspace_bytes(n, d, k);
}

int lasso_split_bregman_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* x0_dev, int64_t ldx0,
                              void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                              const lasso_split_bregman_options* o, lasso_split_bregman_result* res, void* workspace_dev,
                              size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "Split Bregman: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (k > 4096) return fail(LASSO_ERR_UNSUPPORTED, "Split Bregman: k=%lld > 4096", (long long)k);
  if (!(alpha > 0.0) || !(o->lambd > 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha > 0 and lambd > 0 are required");
  if (o->tol != o->tol || o->tau != o->tau) return fail(LASSO_ERR_BAD_ARG, "tol or tau is not a number");
  if (o->maxiter < 1 || o->niter_inner < 1) return fail(LASSO_ERR_BAD_ARG, "maxiter >= 1 and niter_inner >= 1 are required");
  if (o->reserved & ~1) return fail(LASSO_ERR_BAD_ARG, "Split Bregman: only bit 0 of reserved is defined");
  if (const lasso_split_bregman_trace* t = res->trace) {
    if (t->capacity < 0) return fail(LASSO_ERR_BAD_ARG, "trace with a negative capacity");
  }
  res->n_iter = res->itn = res->stopped = res->cholesky_info = 0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || (x0_dev && ldx0 < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_split_bregman_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_split_bregman_workspace_bytes(n, d, k, dtype));
  return split_bregman::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)x0_dev, ldx0,
                              (float*)z_out_dev, ldz, n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

// ---- interior point: interior_point.py:93-225 (csrc/interior_point.hip) ----------------------
size_t lasso_interior_point_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  if (dtype != LASSO_F32 || n < 0 || d <= 0 || k <= 0 || d > 256 || k > 4096 || n > INT32_MAX) return 0;
  return interior_point::workspace_bytes(n, d, k);
}

int lasso_interior_point_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                               void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                               const lasso_interior_point_options* o, lasso_interior_point_result* res, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "interior point: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX)
    return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (d > 256) return fail(LASSO_ERR_UNSUPPORTED, "interior point: d=%lld > 256", (long long)d);
  if (k > 4096) return fail(LASSO_ERR_UNSUPPORTED, "interior point: k=%lld > 4096", (long long)k);
  if (!(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "alpha < 0");
  if ((o->reserved & ~(int64_t)LASSO_FORCE_BLOCKS_128) != 0)
    return fail(LASSO_ERR_BAD_ARG, "interior point: only bit 3 of reserved is defined");
  if (o->maxiter < 0 || !(o->eps >= 0.0) || o->tol != o->tol || o->barrier_init != o->barrier_init)
    return fail(LASSO_ERR_BAD_ARG, "maxiter >= 0, eps >= 0 and numbers for tol and barrier_init are required");
  if (const lasso_interior_point_trace* t = res->trace) {
    if (t->capacity < 0 || (t->capacity > 0 && (!t->obj || !t->prim_feas || !t->dual_feas || !t->gap)))
      return fail(LASSO_ERR_BAD_ARG, "trace with a null array");
  }
  res->n_iter = 0;
  res->status = LASSO_INTERIOR_POINT_MAXITER;
  res->obj0 = 0.0;
  if (n == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z0_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k || ldz0 < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_interior_point_workspace_bytes(n, d, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_interior_point_workspace_bytes(n, d, k, dtype));
  return interior_point::solve((const float*)x_dev, ldx, (const float*)w_dev, ldw, (const float*)z0_dev, ldz0, (float*)z_out_dev,
                               ldz, n, d, k, alpha, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

int lasso_interior_point_rows(const void* w_dev, int64_t ldw, const void* c_dev, int64_t ldc, const void* b_dev, int64_t ldb,
                              void* y_dev, int64_t ldy, int64_t n, int64_t d, int64_t k, int dtype, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "interior point: dtype %d (fp32 tensors only)", dtype);
  if (n < 0 || d <= 0 || k <= 0 || n > INT32_MAX || d > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (d > 256) return fail(LASSO_ERR_UNSUPPORTED, "interior point: d=%lld > 256", (long long)d);
  if (k > 4096) return fail(LASSO_ERR_UNSUPPORTED, "interior point: k=%lld > 4096", (long long)k);
  if (n == 0) return LASSO_OK;
  if (!w_dev || !c_dev || !b_dev || !y_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldw < k || ldc < k || ldb < d || ldy < d) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  return interior_point::rows((const float*)w_dev, ldw, (const float*)c_dev, ldc, (const float*)b_dev, ldb, (float*)y_dev, ldy,
                              n, d, k, static_cast<hipStream_t>(stream));
}

// ---- the block side of the solvers' GEMM shell (csrc/solver_common.hpp) ----------------------
int lasso_solver_block_side(int64_t m, int64_t nn, int64_t ldmax) {
  if (m < 0 || nn < 0 || m > INT32_MAX || nn > INT32_MAX) return 0;
  return gpsr::block_side_here((int)m, (int)nn, ldmax);
}

// ---- one dense system per batch entry: utils.py:43-58 (csrc/batch_solve.hip) -----------------
int lasso_batch_solve_tier_cap(int dtype, int tier) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64) return 0;
  return batch_solve::tier_cap(dtype, tier);
}

static bool batch_solve_shape_ok(int64_t nbatch, int64_t d, int dtype) {
  return (dtype == LASSO_F32 || dtype == LASSO_F64) && nbatch >= 1 && nbatch <= INT32_MAX && d >= 1 &&
         d <= batch_solve::tier_cap(dtype, LASSO_BATCH_TIER_GENERAL);
}

int lasso_batch_solve_workgroups(int64_t nbatch, int64_t d, int dtype) {
  return batch_solve_shape_ok(nbatch, d, dtype) ? batch_solve::general_workgroups(nbatch, d, dtype) : 0;
}

size_t lasso_batch_solve_workspace_bytes(int64_t nbatch, int64_t d, int dtype) {
  return batch_solve_shape_ok(nbatch, d, dtype) ? batch_solve::workspace_bytes(nbatch, d, dtype) : 0;
}

static int check_batch_solve(const void* a_dev, int64_t batch_stride, int64_t lda, const void* b_dev, int64_t ldb,
                             const void* x_dev, int64_t ldx, int64_t nbatch, int64_t d, int dtype,
                             lasso_batch_solve_result* res, const void* workspace_dev, size_t workspace_bytes) {
  if (!a_dev || !b_dev || !x_dev || !res || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "batch solve: null pointer");
  if (nbatch < 1 || d < 1 || nbatch > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "batch solve: bad shape");
  if (batch_stride < 0 || lda < d || ldb < d || ldx < d)
    return fail(LASSO_ERR_BAD_ARG, "batch solve: a negative batch stride or a leading dimension below d");
  if (dtype != LASSO_F32 && dtype != LASSO_F64)
    return fail(LASSO_ERR_UNSUPPORTED, "batch solve: dtype %d (LASSO_F32 and LASSO_F64 are implemented)", dtype);
  if (d > batch_solve::tier_cap(dtype, LASSO_BATCH_TIER_GENERAL))
    return fail(LASSO_ERR_UNSUPPORTED, "batch solve: d = %lld is beyond the cap of %d for this dtype", (long long)d,
                batch_solve::tier_cap(dtype, LASSO_BATCH_TIER_GENERAL));
  if (workspace_bytes < lasso_batch_solve_workspace_bytes(nbatch, d, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_batch_solve_workspace_bytes(nbatch, d, dtype));
  res->bad_system = -1;
  res->bad_minor = 0;
  res->tier = 0;
  return LASSO_OK;
}

int lasso_batch_chol_solve(const void* a_dev, int64_t batch_stride, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev,
                           int64_t ldx, int64_t nbatch, int64_t d, int dtype, lasso_batch_solve_result* res,
                           void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (int s = check_batch_solve(a_dev, batch_stride, lda, b_dev, ldb, x_dev, ldx, nbatch, d, dtype, res, workspace_dev,
                                workspace_bytes))
    return s;
  return batch_solve::chol(a_dev, batch_stride, lda, b_dev, ldb, x_dev, ldx, nbatch, d, dtype, res, workspace_dev,
                           static_cast<hipStream_t>(stream));
}

int lasso_batch_lu_solve(const void* a_dev, int64_t batch_stride, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev,
                         int64_t ldx, int64_t nbatch, int64_t d, int dtype, lasso_batch_solve_result* res,
                         void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (int s = check_batch_solve(a_dev, batch_stride, lda, b_dev, ldb, x_dev, ldx, nbatch, d, dtype, res, workspace_dev,
                                workspace_bytes))
    return s;
  return batch_solve::lu(a_dev, batch_stride, lda, b_dev, ldb, x_dev, ldx, nbatch, d, dtype, res, workspace_dev,
                         static_cast<hipStream_t>(stream));
}

// ---- conjugate gradients: conjgrad.py:13-107 (csrc/conjgrad.hip) -----------------------------
static int check_cg_request(const lasso_cg_options* o, lasso_cg_result* res, bool dense) {
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  if (o->maxiter < 0 || !(o->tol >= 0.0) || !(o->rtol >= 0.0) || !(o->tik >= 0.0))
    return fail(LASSO_ERR_BAD_ARG, "conjugate gradients: maxiter, tol, rtol, tik >= 0 are required");
  if (dense && o->tik != 0.0) return fail(LASSO_ERR_BAD_ARG, "conjugate gradients: the dense form takes tik = 0");
  if (o->reserved & ~(dense ? 1 | LASSO_FORCE_BLOCKS_128 : 1))
    return fail(LASSO_ERR_BAD_ARG, "conjugate gradients: an undefined bit of reserved");
  if (const lasso_cg_trace* t = res->trace)
    if (t->capacity < 0) return fail(LASSO_ERR_BAD_ARG, "trace with a negative capacity");
  res->n_iter = 0;
  res->status = LASSO_CG_MAXITER;
  res->host_reads = 0;
  res->form = 0;
  res->termcond = 0.0;
  return LASSO_OK;
}

size_t lasso_cg_workspace_bytes(int64_t n, int64_t k, int dtype) {
  if ((dtype != LASSO_F32 && dtype != LASSO_F64) || n < 0 || k <= 0 || n > INT32_MAX || k > INT32_MAX) return 0;
  return conjgrad::workspace_bytes(n, k, dtype);
}

int lasso_cg_solve(const void* a_dev, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev, int64_t ldx, int64_t n,
                   int64_t k, int dtype, const lasso_cg_options* o, lasso_cg_result* res, void* workspace_dev,
                   size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64)
    return fail(LASSO_ERR_UNSUPPORTED, "conjugate gradients: dtype %d (LASSO_F32 and LASSO_F64 are implemented)", dtype);
  if (n < 0 || k <= 0 || n > INT32_MAX || k > INT32_MAX) return fail(LASSO_ERR_BAD_ARG, "bad shape");
  if (int s = check_cg_request(o, res, true)) return s;
  if (n == 0) return LASSO_OK;
  if (!a_dev || !b_dev || !x_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (lda < k || ldb < k || ldx < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (workspace_bytes < lasso_cg_workspace_bytes(n, k, dtype))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_cg_workspace_bytes(n, k, dtype));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == LASSO_F64)
    return conjgrad::solve_f64((const double*)a_dev, lda, (const double*)b_dev, ldb, (double*)x_dev, ldx, n, k, *o, res,
                               workspace_dev, st);
  return conjgrad::solve_f32((const float*)a_dev, lda, (const float*)b_dev, ldb, (float*)x_dev, ldx, n, k, *o, res,
                             workspace_dev, st);
}

// what the convolutional form cannot address: the limits of the two GEMMs around the patch matrices (as convolutional GPSR)
static bool conv_cg_too_large(const ConvGeom& g) {
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ldr = ((int64_t)g.C * g.kh * g.kw + 3) / 4 * 4;
  return (int64_t)g.C * g.H * g.W > INT32_MAX || std::max<int64_t>({M, (int64_t)g.K, ldr}) * 64 * 4 >= ((int64_t)1 << 31);
}

size_t lasso_conv_cg_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh,
                                     int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F32) || conv_cg_too_large(g)) return 0;
  return conjgrad::conv_workspace_bytes(g);
}

int lasso_conv_cg_solve(const void* w_dev, const void* b_dev, void* z_out_dev, int64_t N, int64_t C, int64_t H, int64_t W,
                        int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                        const lasso_cg_options* o, lasso_cg_result* res, void* workspace_dev, size_t workspace_bytes,
                        void* stream) {
  if (dtype != LASSO_F32)
    return fail(LASSO_ERR_UNSUPPORTED, "convolutional conjugate gradients: dtype %d (fp32 tensors only)", dtype);
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (conv_cg_too_large(g))
    return fail(LASSO_ERR_UNSUPPORTED, "convolutional conjugate gradients: %lld code pixels / %lld image elements are beyond 32-bit block offsets",
                (long long)(N * Hz * Wz), (long long)(C * H * W));
  if (int s = check_cg_request(o, res, false)) return s;
  if (N == 0) return LASSO_OK;
  if (!w_dev || !b_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  const size_t need = conjgrad::conv_workspace_bytes(g);
  if (workspace_bytes < need) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", need);
  return conjgrad::conv_solve((const float*)w_dev, (const float*)b_dev, (float*)z_out_dev, g, *o, res, workspace_dev,
                              static_cast<hipStream_t>(stream));
}

// ---- exact Lipschitz constant of a convolutional dictionary: lip_const.py:8-31 (csrc/conv_lanczos.hip) -------
// The geometry of a batch of one from the reference's imsize: the image's size (transpose == 0, it must round-trip) or
// the code's.  false: no such geometry.
static bool conv_lip_geom(int64_t K, int64_t C, int kh, int kw, int64_t H, int64_t W, int sh, int sw, int ph, int pw,
                          int transpose, ConvGeom* g) {
  if (K <= 0 || C <= 0 || kh <= 0 || kw <= 0 || H <= 0 || W <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0 ||
      K > INT32_MAX || C > INT32_MAX || H > INT32_MAX / 2 || W > INT32_MAX / 2)
    return false;
  int64_t Hi, Wi, Hz, Wz;
  if (transpose) {
    Hz = H; Wz = W;
    Hi = (Hz - 1) * sh - 2 * (int64_t)ph + kh;
    Wi = (Wz - 1) * sw - 2 * (int64_t)pw + kw;
  } else {
    Hi = H; Wi = W;
    const int64_t eh = Hi + 2 * (int64_t)ph - kh, ew = Wi + 2 * (int64_t)pw - kw;
    if (eh < 0 || ew < 0 || eh % sh != 0 || ew % sw != 0) return false;
    Hz = eh / sh + 1; Wz = ew / sw + 1;
  }
  if (Hi <= 0 || Wi <= 0 || Hi > INT32_MAX / 2 || Wi > INT32_MAX / 2) return false;
  *g = make_geom(1, C, Hi, Wi, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  return true;
}

static int conv_lip_code_space(const ConvGeom& g) {       // the smaller space; a tie goes to the images
  return (int64_t)g.K * g.Hz * g.Wz < (int64_t)g.C * g.H * g.W;
}

size_t lasso_conv_lip_constant_workspace_bytes(int64_t K, int64_t C, int kh, int kw, int64_t H, int64_t W, int sh, int sw,
                                               int ph, int pw, int transpose, int dtype, int maxiter) {
  ConvGeom g;
  if ((dtype != LASSO_F32 && dtype != LASSO_F64) || maxiter < 1) return 0;
  if (!conv_lip_geom(K, C, kh, kw, H, W, sh, sw, ph, pw, transpose, &g)) return 0;
  if (check_conv(g, dtype) || conv_cg_too_large(g)) return 0;
  return lanczos::workspace_bytes(g, conv_lip_code_space(g), maxiter, dtype);
}

int lasso_conv_lip_constant(const void* w_dev, int64_t K, int64_t C, int kh, int kw, int64_t H, int64_t W, int sh, int sw,
                            int ph, int pw, int transpose, int dtype, const lasso_conv_lip_options* o,
                            lasso_conv_lip_result* res, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32 && dtype != LASSO_F64)
    return fail(LASSO_ERR_UNSUPPORTED, "lip_constant: dtype %d (LASSO_F32 and LASSO_F64 are implemented)", dtype);
  if (!o || !res || !w_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (o->maxiter < 1 || !(o->tol >= 0.0) || o->reserved != 0)
    return fail(LASSO_ERR_BAD_ARG, "lip_constant: maxiter >= 1, tol >= 0 and reserved == 0 are required");
  if (res->history && res->history_capacity < 0) return fail(LASSO_ERR_BAD_ARG, "history with a negative capacity");
  ConvGeom g;
  if (!conv_lip_geom(K, C, kh, kw, H, W, sh, sw, ph, pw, transpose, &g))
    return fail(LASSO_ERR_BAD_ARG, "lip_constant: no convolution of a %lldx%lld %s by a %dx%d kernel, stride %d,%d padding %d,%d%s",
                (long long)H, (long long)W, transpose ? "code" : "image", kh, kw, sh, sw, ph, pw,
                transpose ? "" : " (the image size must round-trip)");
  if (int s = check_conv(g, dtype)) return s;
  if (conv_cg_too_large(g))
    return fail(LASSO_ERR_UNSUPPORTED, "lip_constant: %lld code pixels / %lld image elements are beyond 32-bit block offsets",
                (long long)g.Hz * g.Wz, (long long)C * g.H * g.W);
  res->theta = res->residual = NAN;
  res->steps = res->matvecs = res->host_reads = res->restarts = 0;
  res->status = LASSO_LIP_MAXITER;
  const int code_space = conv_lip_code_space(g);
  const size_t need = lanczos::workspace_bytes(g, code_space, o->maxiter, dtype);
  if (workspace_bytes < need) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", need);
  return lanczos::run(w_dev, g, code_space, dtype, *o, res, workspace_dev, static_cast<hipStream_t>(stream));
}

// ---- unconstrained M-step: update_dict_ridge, dict_learning.py:106-123 ---------------------
size_t lasso_ridge_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0 || k > 4096) return 0;
  return ridge_workspace_bytes(d, k) + 256;
}

int lasso_ridge_solve(const float* a_dev, const float* b_dev, void* v_dev, int64_t ldv, int64_t d, int64_t k,
                      int dtype, double lambda_n, int32_t* info_out, void* workspace_dev, size_t workspace_bytes,
                      void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!a_dev || !b_dev || !v_dev || !workspace_dev || d <= 0 || k <= 0 || ldv < k)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (k > 4096) return fail(LASSO_ERR_UNSUPPORTED, "ridge solve: k=%lld > 4096", (long long)k);
  if (workspace_bytes < lasso_ridge_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_ridge_workspace_bytes(d, k));
  hipStream_t st = (hipStream_t)stream;
  int* const info_dev = (int*)((char*)workspace_dev + ridge_workspace_bytes(d, k));
  LASSO_HIP_TRY(launch_ridge_solve(a_dev, b_dev, (float*)v_dev, ldv, (int)d, (int)k, (float)lambda_n, workspace_dev,
                                   info_dev, st));
  if (info_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(info_out, info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    if (*info_out != 0)
      return fail(LASSO_ERR_BAD_ARG, "Z^T Z + lambd*n*I is not positive definite (pivot %d)", *info_out);
  }
  return LASSO_OK;
}

int lasso_dict_fill_degenerate(void* d_dev, int64_t ldd, int64_t d, int64_t k, int dtype,
                               const int32_t* degenerate_dev, const float* pool_dev, int64_t pool_rows,
                               int64_t pool_ld, int positive, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!d_dev || !degenerate_dev || !pool_dev || d <= 0 || k <= 0 || ldd < k || pool_rows <= 0 || pool_ld < d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  LASSO_HIP_TRY(launch_fill_degenerate((float*)d_dev, ldd, (int)d, (int)k, degenerate_dev, pool_dev, (int)pool_rows,
                                       pool_ld, positive, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_zero_columns(void* z_dev, int64_t ldz, int64_t n, int64_t k, int dtype,
                       const int32_t* degenerate_dev, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (!z_dev || !degenerate_dev || n < 0 || k <= 0 || ldz < k) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  LASSO_HIP_TRY(launch_zero_columns((float*)z_dev, ldz, (int)n, (int)k, degenerate_dev, (hipStream_t)stream));
  return LASSO_OK;
}

// ---- float64 M-step (mstep_f64.hip): the entry points above with double matrices; see include/lasso_hip.h ----------
size_t lasso_gram_f64_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (n <= 0 || d <= 0 || k <= 0) return 0;
  return f64::gram_workspace_bytes(n, d, k) + 256;
}

int lasso_gram_accumulate_f64(const double* z_dev, int64_t ldz, const double* x_dev, int64_t ldx, int64_t n, int64_t d,
                              int64_t k, double* a_dev, double* b_dev, void* workspace_dev, size_t workspace_bytes,
                              void* stream) {
  if (!z_dev || !x_dev || !a_dev || !b_dev || n <= 0 || d <= 0 || k <= 0 || ldz < k || ldx < d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (n > INT32_MAX - 64 || (k + 63) / 64 > 65535 || (d + 63) / 64 > 65535) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  // optional scratch for the row slabs' partial products (NULL or too small: one pass)
  double* scratch = (workspace_dev && workspace_bytes >= lasso_gram_f64_workspace_bytes(n, d, k)) ? (double*)workspace_dev
                                                                                                  : nullptr;
  const int splits = scratch ? f64::gram_splits(n, d, k, device_cus()) : 1;
  LASSO_HIP_TRY(f64::launch_gram(z_dev, ldz, x_dev, ldx, (int)n, (int)d, (int)k, a_dev, b_dev, scratch, splits,
                                 (hipStream_t)stream));
  return LASSO_OK;
}

size_t lasso_dict_sweep_f64_workspace_bytes(int64_t d, int64_t k) {
  if (d <= 0 || k <= 0 || d > kSweepMaxD || k > kSweepMaxK) return 0;
  return f64::sweep_workspace_bytes(d, k);
}

int lasso_dict_sweep_f64(const double* a_dev, const double* b_dev, double* d_dev, int64_t ldd, int64_t d, int64_t k,
                         double eps, int positive, int32_t* degenerate_dev, int32_t* ndeg_out, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
  if (!a_dev || !b_dev || !d_dev || !degenerate_dev || !workspace_dev || d <= 0 || k <= 0 || ldd < k)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (d > kSweepMaxD || k > kSweepMaxK)
    return fail(LASSO_ERR_UNSUPPORTED, "atom sweep: d=%lld k=%lld (d <= %d, k <= %d)", (long long)d, (long long)k,
                kSweepMaxD, kSweepMaxK);
  if (workspace_bytes < lasso_dict_sweep_f64_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_dict_sweep_f64_workspace_bytes(d, k));
  hipStream_t st = (hipStream_t)stream;
  LASSO_HIP_TRY(f64::launch_sweep(a_dev, b_dev, d_dev, ldd, (int)d, (int)k, eps, positive, degenerate_dev, workspace_dev, st));
  if (ndeg_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(ndeg_out, (char*)workspace_dev + f64::sweep_count_offset(d, k), sizeof(int),
                                 hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
  }
  return LASSO_OK;
}

int lasso_dict_fill_degenerate_f64(double* d_dev, int64_t ldd, int64_t d, int64_t k, const int32_t* degenerate_dev,
                                   const double* pool_dev, int64_t pool_rows, int64_t pool_ld, int positive,
                                   void* stream) {
  if (!d_dev || !degenerate_dev || !pool_dev || d <= 0 || k <= 0 || ldd < k || pool_rows <= 0 || pool_ld < d)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (d > INT32_MAX || k > INT32_MAX || pool_rows > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  LASSO_HIP_TRY(f64::launch_fill_degenerate(d_dev, ldd, (int)d, (int)k, degenerate_dev, pool_dev, (int)pool_rows, pool_ld,
                                            positive, (hipStream_t)stream));
  return LASSO_OK;
}

int lasso_zero_columns_f64(double* z_dev, int64_t ldz, int64_t n, int64_t k, const int32_t* degenerate_dev, void* stream) {
  if (!z_dev || !degenerate_dev || n <= 0 || k <= 0 || ldz < k) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (k > INT32_MAX) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  LASSO_HIP_TRY(f64::launch_zero_columns(z_dev, ldz, n, (int)k, degenerate_dev, (hipStream_t)stream));
  return LASSO_OK;
}

size_t lasso_ridge_f64_workspace_bytes(int64_t d, int64_t k) {
  const size_t s = f64::ridge_workspace_bytes(d, k);
  return s ? s + 256 : 0;
}

int lasso_ridge_solve_f64(const double* a_dev, const double* b_dev, double* v_dev, int64_t ldv, int64_t d, int64_t k,
                          double lambda_n, int32_t* info_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!a_dev || !b_dev || !v_dev || !workspace_dev || d <= 0 || k <= 0 || ldv < k)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (k > 4096 || d > INT32_MAX - 4096) return fail(LASSO_ERR_UNSUPPORTED, "ridge solve: k=%lld > 4096", (long long)k);
  if (workspace_bytes < lasso_ridge_f64_workspace_bytes(d, k))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_ridge_f64_workspace_bytes(d, k));
  hipStream_t st = (hipStream_t)stream;
  int* const info_dev = (int*)((char*)workspace_dev + f64::ridge_workspace_bytes(d, k));
  LASSO_HIP_TRY(f64::launch_ridge_solve(a_dev, b_dev, v_dev, ldv, (int)d, (int)k, lambda_n, workspace_dev, info_dev, st));
  if (info_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(info_out, info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
    if (*info_out != 0)
      return fail(LASSO_ERR_BAD_ARG, "Z^T Z + lambd*n*I is not positive definite (pivot %d)", *info_out);
  }
  return LASSO_OK;
}

// ---- greedy coordinate descent: coordinate_descent.py:5-54 -------------------------
size_t lasso_cd_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  (void)dtype;
  const int kp = pad_k_cd(k);
  if (kp < 0 || n < 0 || d <= 0) return 0;
  return carve_cd(nullptr, n, d, kp).bytes;
}

int lasso_cd_prepare(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                     int64_t ldz0, int64_t n, int64_t d, int64_t k, int dtype, void* workspace_dev,
                     size_t workspace_bytes, void* stream) {
  if (int s = check_cd(n, d, k, dtype)) return s;
  if (!w_dev || (n > 0 && !x_dev) || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || (z0_dev && ldz0 < k)) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  const int kp = pad_k_cd(k);
  CdWorkspace ws = carve_cd(workspace_dev, n, d, kp);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // Wt [kp][d] (zero rows past k);  S = -Wt Wt^T (:22), +1 on the first k diagonal entries
  // (:23);  b = x Wt^T (:19).  Padded columns of b and S are exact zeros.
  LASSO_HIP_TRY(launch_transpose_pad((const float*)w_dev, ldw, (int)d, (int)k, ws.Wt, d, kp, (int)d, st));
  LASSO_HIP_TRY(launch_gemm_nt_sub(ws.Wt, d, ws.Wt, d, nullptr, 0, ws.S, kp, kp, kp, (int)d, st));
  LASSO_HIP_TRY(launch_cd_init((const float*)z0_dev, ldz0, ws.Zt, kp, (int)n, (int)k, ws.active,
                               ws.row_steps, ws.S, st));
  if (n > 0)
    LASSO_HIP_TRY(launch_gemm_nt_sub((const float*)x_dev, ldx, ws.Wt, d, nullptr, 0, ws.B, kp, (int)n, kp,
                                     (int)d, st, /*add=*/1));
  return LASSO_OK;
}

int lasso_cd_run(int64_t n, int64_t d, int64_t k, double alpha, double tol_abs, int iters,
                 int32_t* n_active_out, int32_t* max_steps_out, void* workspace_dev,
                 size_t workspace_bytes, void* stream) {
  if (int s = check_cd(n, d, k, LASSO_F32)) return s;
  if (!workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null workspace");
  if (int s = check_cd_run_args(iters, alpha)) return s;
  const int kp = pad_k_cd(k);
  CdWorkspace ws = carve_cd(workspace_dev, n, d, kp);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool want_info = n_active_out || max_steps_out;
  int info[2] = {0, 0};
  if (n > 0) {
    CdParams p;
    p.B = ws.B; p.Zt = ws.Zt; p.S = ws.S; p.active = ws.active; p.row_steps = ws.row_steps;
    p.counter = ws.counter; p.n = (int)n; p.iters = iters;
    p.alpha = (float)alpha; p.tol = (float)tol_abs;
    LASSO_HIP_TRY(launch_cd_rows(p, kp, device_cus(), want_info ? ws.info : nullptr, st));
    if (want_info) {
      LASSO_HIP_TRY(hipMemcpyAsync(info, ws.info, sizeof(info), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
    }
  }
  if (n_active_out) *n_active_out = info[0];
  if (max_steps_out) *max_steps_out = info[1];
  return LASSO_OK;
}

int lasso_cd_finish(void* z_out_dev, int64_t ldz, void* z_track_out_dev, int64_t ldzt, int64_t n,
                    int64_t d, int64_t k, double alpha, void* workspace_dev, size_t workspace_bytes,
                    void* stream) {
  if (int s = check_cd(n, d, k, LASSO_F32)) return s;
  if (!workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null workspace");
  if (int s = check_cd_finish_args(z_out_dev, ldz, z_track_out_dev, ldzt, k)) return s;
  const int kp = pad_k_cd(k);
  CdWorkspace ws = carve_cd(workspace_dev, n, d, kp);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  LASSO_HIP_TRY(launch_cd_finish(ws.B, ws.Zt, kp, (float*)z_out_dev, ldz, (float*)z_track_out_dev, ldzt,
                                 (int)n, (int)k, (float)alpha, static_cast<hipStream_t>(stream)));
  return LASSO_OK;
}

int lasso_cd_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, void* z0_inout_dev,
                   int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                   double alpha, int maxiter, double tol, int32_t* n_active_out, int32_t* max_steps_out,
                   void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (int s = check_cd(n, d, k, dtype)) return s;
  if (!z_out_dev && n > 0) return fail(LASSO_ERR_BAD_ARG, "null z_out");
  // (what lasso_cd_run / _finish would refuse, before lasso_cd_prepare enqueues anything)
  if (int s = check_cd_run_args(maxiter, alpha)) return s;
  if (int s = check_cd_finish_args(z_out_dev, ldz, z0_inout_dev, ldz0, k)) return s;
  if (int s = lasso_cd_prepare(x_dev, ldx, w_dev, ldw, z0_inout_dev, ldz0, n, d, k, dtype, workspace_dev,
                               workspace_bytes, stream))
    return s;
  // :9  tol = tol * code_dim
  if (int s = lasso_cd_run(n, d, k, alpha, tol * (double)k, maxiter, n_active_out, max_steps_out,
                           workspace_dev, workspace_bytes, stream))
    return s;
  return lasso_cd_finish(z_out_dev, ldz, z0_inout_dev, ldz0, n, d, k, alpha, workspace_dev,
                         workspace_bytes, stream);
}

// ---- cyclic coordinate descent with a duality-gap stop: coordinate_descent.py:57-139 ----
namespace {
struct CdModWorkspace { float* G; float* Wt; float* B0; int* row_sweeps; int* row_conv; unsigned long long* row_commits;
                        long long* info; size_t bytes; };

CdModWorkspace carve_cd_mod(void* base, int64_t n, int64_t d, int kp) {
  CdModWorkspace w;
  Arena a(base);
  w.G = a.take((size_t)kp * kp * 4);
  w.Wt = a.take((size_t)kp * d * 4);
  w.B0 = a.take((size_t)n * kp * 4);
  w.row_sweeps = a.take<int>((size_t)n * 4);
  w.row_conv = a.take<int>((size_t)n * 4);
  w.row_commits = a.take<unsigned long long>((size_t)n * 8);
  w.info = a.take<long long>(256);
  w.bytes = a.bytes();
  return w;
}
}  // namespace

size_t lasso_cd_mod_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype) {
  const int kp = pad_k_cd(k);
  if (dtype != LASSO_F32 || kp < 0 || n < 0 || d <= 0) return 0;
  return carve_cd_mod(nullptr, n, d, kp).bytes;
}

int lasso_cd_mod_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, void* z_inout_dev, int64_t ldz,
                       int z_has_start, float* gap_out_dev, int32_t* sweeps_out_dev, uint8_t* converged_out_dev,
                       int64_t n, int64_t d, int64_t k, int dtype, double alpha, int max_iter, double tol,
                       int32_t* n_unconverged_out, int64_t* committed_out, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
  if (int s = check_cd(n, d, k, dtype)) return s;
  if (!w_dev || !workspace_dev || (n > 0 && (!x_dev || !z_inout_dev || !gap_out_dev)))
    return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || ldz < k) return fail(LASSO_ERR_BAD_ARG, "leading dimension too small");
  if (max_iter < 0 || !(alpha >= 0.0) || tol != tol)
    return fail(LASSO_ERR_BAD_ARG, "max_iter=%d alpha=%g tol=%g", max_iter, alpha, tol);
  const int kp = pad_k_cd(k);
  CdModWorkspace ws = carve_cd_mod(workspace_dev, n, d, kp);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  long long info[2] = {0, 0};
  if (n > 0) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    // Wt [kp][d] (zero rows past k);  G = Wt Wt^T, whose diagonal holds the atoms' squared norms (:84);
    // b0 = x Wt^T.  Padded columns of b0 and G are exact zeros, and so are the row and column of an all-zero atom.
    LASSO_HIP_TRY(launch_transpose_pad((const float*)w_dev, ldw, (int)d, (int)k, ws.Wt, d, kp, (int)d, st));
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.Wt, d, ws.Wt, d, nullptr, 0, ws.G, kp, kp, kp, (int)d, st, /*add=*/1));
    LASSO_HIP_TRY(launch_gemm_nt_sub((const float*)x_dev, ldx, ws.Wt, d, nullptr, 0, ws.B0, kp, (int)n, kp, (int)d, st,
                                     /*add=*/1));
    CdModParams p;
    p.x = (const float*)x_dev; p.ldx = ldx; p.B0 = ws.B0; p.G = ws.G;
    p.z = (float*)z_inout_dev; p.ldz = ldz; p.has_start = z_has_start ? 1 : 0;
    p.gap = gap_out_dev; p.sweeps_out = sweeps_out_dev; p.conv_out = converged_out_dev;
    p.row_sweeps = ws.row_sweeps; p.row_conv = ws.row_conv; p.row_commits = ws.row_commits;
    p.n = (int)n; p.d = (int)d; p.k = (int)k; p.max_iter = max_iter;
    p.alpha = (float)alpha; p.tol = (float)tol; p.gap0 = (float)(tol + 1.0);     // :78
    LASSO_HIP_TRY(launch_cd_mod_rows(p, kp, device_cus(), st));
    if (n_unconverged_out || committed_out) {
      LASSO_HIP_TRY(launch_cd_mod_info(ws.row_conv, ws.row_commits, (int)n, ws.info, st));
      LASSO_HIP_TRY(hipMemcpyAsync(info, ws.info, sizeof(info), hipMemcpyDeviceToHost, st));
      LASSO_HIP_TRY(hipStreamSynchronize(st));
    }
  }
  if (n_unconverged_out) *n_unconverged_out = (int32_t)info[0];
  if (committed_out) *committed_out = (int64_t)info[1];
  return LASSO_OK;
}

// ---- convolutional ISTA/FISTA: lasso/conv2d/ista.py:7-49, lip_const.py:96-135 ----------
size_t lasso_conv_ista_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz,
                                       int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F32)) return 0;
  return carve_conv(nullptr, g).bytes;
}

const char* lasso_conv_ista_kernel_name(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                                        int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (N <= 0 || check_conv(g, LASSO_F32)) return "";
  const int cus = std::max(device_cus(), 1);
  if (const char* fused = conv_fused_kernel_name(g, cus)) return fused;
  // the two-kernel form: what the launchers themselves say about this geometry (their dry runs: no duplicate of the
  // eligibility rules here -- VERDICT r05 / tests/test_bench_gpu.py: a name must occur in its own dispatch)
  static const float kAligned[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  bool synth = false, few = false;
  int gp = 0;
  (void)launch_conv_synth(kAligned, kAligned, kAligned, nullptr, g, cus, &synth, nullptr, 1);
  if (!synth) (void)launch_conv_synth_few(kAligned, kAligned, kAligned, nullptr, g, cus, &few, nullptr, 1);
  (void)launch_conv_grad_prox(nullptr, nullptr, 0, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, kGenGrid, g, cus, &gp, nullptr, 1);
  static thread_local char cname[192];
  snprintf(cname, sizeof(cname), "%s + %s",
           synth ? "lasso::conv_synth_kernel" : few ? "lasso::conv_synth_few_kernel"
                                                    : "lasso::gemm_nt_kernel + lasso::conv_residual_kernel",
           gp > 0 ? "lasso::conv_grad_prox_kernel"
                  : "lasso::conv_patches_kernel + lasso::gemm_nt_kernel + lasso::generic_prox_kernel");
  return cname;
}

// ---- convolutional GPSR-Basic: gpsr_basic with A = conv_transpose2d, AT = conv2d (csrc/conv_gpsr.hip) ----
// what the solve cannot address: an image row beyond int, or a pitch (the tap-major matrix has pitch M) beyond the
// 32-bit offsets of a 64-row GEMM block
static bool conv_gpsr_too_large(const ConvGeom& g) {
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ldr = ((int64_t)g.C * g.kh * g.kw + 3) / 4 * 4;
  return (int64_t)g.C * g.H * g.W > INT32_MAX || std::max<int64_t>({M, (int64_t)g.K, ldr}) * 64 * 4 >= ((int64_t)1 << 31);
}
size_t lasso_conv_gpsr_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                                       int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F32) || conv_gpsr_too_large(g)) return 0;
  return gpsr::conv_workspace_bytes(g);
}

const char* lasso_conv_gpsr_form(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh,
                                 int kw, int sh, int sw, int ph, int pw, int reserved) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F32) || conv_gpsr_too_large(g)) return "";
  return gpsr::conv_form(g, reserved & 1);
}

int lasso_conv_gpsr_solve(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev, int64_t N,
                          int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh,
                          int sw, int ph, int pw, int dtype, double tau, const lasso_gpsr_options* o,
                          lasso_gpsr_result* res, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype != LASSO_F32) return fail(LASSO_ERR_UNSUPPORTED, "convolutional GPSR: dtype %d (fp32 tensors only)", dtype);
  if (!o || !res) return fail(LASSO_ERR_BAD_ARG, "null options / result");
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (conv_gpsr_too_large(g))
    return fail(LASSO_ERR_UNSUPPORTED, "convolutional GPSR: %lld code pixels / %lld image elements are beyond 32-bit block offsets",
                (long long)(N * Hz * Wz), (long long)(C * H * W));
  if (int s = check_gpsr_request(o, res, z0_dev != nullptr, 1 | LASSO_FORCE_BLOCKS_128)) return s;
  if (N == 0) return LASSO_OK;
  if (!x_dev || !w_dev || !z_out_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  const size_t need = gpsr::conv_workspace_bytes(g);
  if (workspace_bytes < need) return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", need);
  return gpsr::conv_solve((const float*)x_dev, (const float*)w_dev, (const float*)z0_dev, (float*)z_out_dev, g, tau, *o, res,
                          workspace_dev, static_cast<hipStream_t>(stream));
}

int lasso_conv_ista_solve(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev, int64_t N,
                          int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw,
                          int sh, int sw, int ph, int pw, int dtype, double alpha, double lr, int fast,
                          int maxiter, double tol, int32_t* iters_out, float* last_delta_out,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (dtype == LASSO_F64) {
    // the same solve; the float slot receives the double rounded once (lasso_conv_ista_solve_f64 keeps it)
    double last64 = NAN;
    const int status = lasso_conv_ista_solve_f64(x_dev, w_dev, z0_dev, z_out_dev, N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph,
                                                 pw, alpha, lr, fast, maxiter, tol, iters_out, &last64, workspace_dev,
                                                 workspace_bytes, stream);
    if (status == LASSO_OK && last_delta_out) *last_delta_out = (float)last64;
    return status;
  }
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (!w_dev || !workspace_dev || (N > 0 && (!x_dev || !z_out_dev))) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (maxiter < 0 || !(lr > 0.0) || !(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "maxiter=%d lr=%g alpha=%g", maxiter, lr, alpha);
  ConvWorkspace ws = carve_conv(workspace_dev, g);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (iters_out) *iters_out = 0;
  if (last_delta_out) *last_delta_out = NAN;
  if (N == 0) return LASSO_OK;
  const int ckk = g.C * g.kh * g.kw, P = g.Hz * g.Wz;
  const int64_t M = (int64_t)g.N * P;
  const int ldr = (ckk + 3) / 4 * 4;
  const int cus = std::max(device_cus(), 1);
  const float* const conv_w = (const float*)w_dev;
  bool fused = false;                     // conv_fused.hip: whole iterations in one launch, a workgroup per image
  LASSO_HIP_TRY(launch_conv_fused_pack(conv_w, ws.Wf, g, cus, &fused, st));
  if (!fused) LASSO_HIP_TRY(launch_conv_pack_w(conv_w, ws.Wt, ws.Wp, g.K, ckk, ldr, st));
  if (z0_dev) {
    LASSO_HIP_TRY(launch_conv_relayout((const float*)z0_dev, ws.Zm, ws.Ym, g.N, g.K, P, 1, st));     // y0 = z0 in the same pass
  } else {
    LASSO_HIP_TRY(hipMemsetAsync(ws.Zm, 0, (size_t)M * g.K * 4, st));
    LASSO_HIP_TRY(hipMemsetAsync(ws.Ym, 0, (size_t)M * g.K * 4, st));
  }
  const float budget = stop_budget<float>(M, g.K, tol);            // ista.py:16, compared in fp32
  const float lr_f = (float)lr, lam = (float)(alpha * lr);
  Momentum mom;
  float last = NAN;
  int it = 0;
  // conv_fused.hip takes up to 64 iterations per launch: `iterate` only queues them (momentum factor + where the sum
  // goes; a chunk's slots are consecutive), `flush` launches what is queued
  float q_coef[64];
  int queued = 0;
  float* q_slot0 = nullptr;
  const int q_max = fused ? std::min(64, conv_fused_max_iters(g, cus)) : 0;
  const bool two_y = fused && conv_fused_two_y_buffers(g, cus);     // bands: y ping-pongs between Ym and G
  auto flush = [&]() -> int {
    if (queued == 0) return LASSO_OK;
    LASSO_HIP_TRY(launch_conv_fused(ws.Wf, (const float*)x_dev, ws.Zm, ws.Ym, two_y ? ws.G : ws.Ym, lr_f, lam, q_coef,
                                    queued, ws.dpart, kConvDpart, q_slot0, g, cus, st));            // :19-20,:29,:42,:44
    if (two_y) std::swap(ws.Ym, ws.G);           // (save / restore below copy whatever ws.Ym is at the time)
    queued = 0;
    q_slot0 = nullptr;
    return LASSO_OK;
  };
  // one iteration on the stream; the sum |z - z_next| of the iteration (ista.py:44) goes to *delta_slot when given
  auto iterate = [&](float* delta_slot) -> int {
    const float coef = mom.next(fast);                                              // :41-42
    if (fused) {
      const bool fits = queued < q_max &&
                        (delta_slot ? (q_slot0 && delta_slot == q_slot0 + queued) : q_slot0 == nullptr);
      if (queued > 0 && !fits)
        if (int s = flush()) return s;
      if (queued == 0) q_slot0 = delta_slot;
      q_coef[queued++] = coef;
      return LASSO_OK;
    }
    int dcount = 0;
    if (int s = conv_two_kernel_step(ws, g, (const float*)x_dev, conv_w, lr_f, lam, coef, cus, &dcount, st)) return s;
    if (delta_slot) {
      hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, ws.dpart, dcount, delta_slot);
      LASSO_HIP_TRY(hipGetLastError());
    }
    return LASSO_OK;
  };
  if (!(tol > 0.0)) {
    for (; it < maxiter; ++it)
      if (int s = iterate(nullptr)) return s;
    if (int s = flush()) return s;
  } else {
    const int64_t code_words = M * g.K;
    const int copy_grid = (int)std::min<int64_t>((code_words / 4 + 255) / 256 + 1, (int64_t)cus * 16);
    auto save = [&]() -> int {
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Zm, ws.Zc, code_words);
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Ym, ws.Yc, code_words);
      LASSO_HIP_TRY(hipGetLastError());
      return LASSO_OK;
    };
    auto restore = [&]() -> int {
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Zc, ws.Zm, code_words);
      hipLaunchKernelGGL(copy_words_kernel, dim3(copy_grid), dim3(256), 0, st, ws.Yc, ws.Ym, code_words);
      LASSO_HIP_TRY(hipGetLastError());
      return LASSO_OK;
    };
    auto read = [&](float* host, int c) -> int { return read_back(host, ws.delta, sizeof(float) * c, st); };
    if (int s = speculate_stop_rule<float>(maxiter, budget, ws.delta, &mom.t, iterate, save, restore, flush, read, &it,
                                           &last, "lasso_conv_ista_solve"))
      return s;
  }
  LASSO_HIP_TRY(launch_conv_relayout(ws.Zm, (float*)z_out_dev, nullptr, g.N, g.K, P, 0, st));
  if (iters_out) *iters_out = it;
  if (last_delta_out) *last_delta_out = last;
  return LASSO_OK;
}

// (0.5*||x - conv_transpose2d(z)||^2 + alpha*||z||_1) / N   (ista.py:23-26) -> loss_dev
int lasso_conv_objective(const void* x_dev, const void* w_dev, const void* z_dev, int64_t N, int64_t C, int64_t H,
                         int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph,
                         int pw, int dtype, double alpha, float* loss_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (!x_dev || !w_dev || !z_dev || !loss_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (N == 0) return fail(LASSO_ERR_BAD_ARG, "empty batch");
  if (dtype == LASSO_F64)       // the double loss rounded once into the float slot (lasso_conv_objective_f64 keeps it)
    return f64::conv_objective((const double*)x_dev, (const double*)w_dev, (const double*)z_dev, g, alpha, nullptr,
                               loss_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream));
  ConvWorkspace ws = carve_conv(workspace_dev, g);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ckk = g.C * g.kh * g.kw, P = g.Hz * g.Wz;
  const int64_t M = (int64_t)g.N * P;
  LASSO_HIP_TRY(launch_conv_pack_w((const float*)w_dev, ws.Wt, ws.Wp, g.K, ckk, (ckk + 3) / 4 * 4, st));
  LASSO_HIP_TRY(launch_conv_relayout((const float*)z_dev, ws.Zm, nullptr, g.N, g.K, P, 1, st));
  LASSO_HIP_TRY(launch_conv_residual(ws.Zm, ws.Wt, (const float*)w_dev, (const float*)x_dev, ws.PT, ws.R, g,
                                     std::max(device_cus(), 1), st));
  LASSO_HIP_TRY(launch_objective_reduce(ws.R, (int64_t)g.N * g.C * g.H * g.W, ws.Zm, g.K, (int)M, g.K, ws.dpart,
                                        kGenGrid, alpha, (double)g.N, ws.sums, loss_dev, st));
  return LASSO_OK;
}

// ---- reverse pass of the convolutional solve (conv_autograd.hip) ------------
size_t lasso_conv_ista_trace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                                   int kh, int kw, int sh, int sw, int ph, int pw, int iterations) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (iterations < 0 || check_conv(g, LASSO_F32)) return 0;
  return (size_t)(iterations + 1) * (size_t)N * Hz * Wz * K * 4;
}

int lasso_conv_ista_run_traced(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev, int64_t N,
                               int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw,
                               int sh, int sw, int ph, int pw, int dtype, double alpha, double lr, int fast,
                               int iterations, void* trace_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (!w_dev || !workspace_dev || (N > 0 && (!x_dev || !z0_dev || !z_out_dev || !trace_dev)))
    return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (iterations < 0 || !(lr > 0.0) || !(alpha >= 0.0))
    return fail(LASSO_ERR_BAD_ARG, "iterations=%d lr=%g alpha=%g", iterations, lr, alpha);
  if (dtype == LASSO_F64)       // trace_dev: lasso_conv_ista_trace_bytes_f64 bytes, doubles
    return f64::conv_solve((const double*)x_dev, (const double*)w_dev, (const double*)z0_dev, (double*)z_out_dev, g, alpha,
                           lr, fast, iterations, 0.0, (double*)trace_dev, nullptr, nullptr, workspace_dev, workspace_bytes,
                           static_cast<hipStream_t>(stream));
  ConvWorkspace ws = carve_conv(workspace_dev, g);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  if (N == 0) return LASSO_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ckk = g.C * g.kh * g.kw, P = g.Hz * g.Wz;
  const int64_t mk = (int64_t)g.N * P * g.K;
  const int cus = std::max(device_cus(), 1);
  const float* const conv_w = (const float*)w_dev;
  float* const trace = (float*)trace_dev;
  LASSO_HIP_TRY(launch_conv_pack_w(conv_w, ws.Wt, ws.Wp, g.K, ckk, (ckk + 3) / 4 * 4, st));
  LASSO_HIP_TRY(launch_conv_relayout((const float*)z0_dev, ws.Zm, ws.Ym, g.N, g.K, P, 1, st));
  LASSO_HIP_TRY(hipMemcpyAsync(trace, ws.Zm, (size_t)mk * 4, hipMemcpyDeviceToDevice, st));
  // the two-kernel form for every geometry: conv_fused.hip computes the same iterates bitwise
  // (tests/test_conv_gpu.py::test_many_iterations_per_launch_kernel)
  const std::vector<float> coef = fista_coefs(iterations, fast);
  const float lr_f = (float)lr, lam = (float)(alpha * lr);
  for (int it = 0; it < iterations; ++it) {
    int dcount = 0;
    if (int s = conv_two_kernel_step(ws, g, (const float*)x_dev, conv_w, lr_f, lam, coef[it], cus, &dcount, st)) return s;
    LASSO_HIP_TRY(hipMemcpyAsync(trace + (it + 1) * mk, ws.Zm, (size_t)mk * 4, hipMemcpyDeviceToDevice, st));
  }
  LASSO_HIP_TRY(launch_conv_relayout(ws.Zm, (float*)z_out_dev, nullptr, g.N, g.K, P, 0, st));
  return LASSO_OK;
}

namespace {
struct ConvBwWorkspace {
  float* Wt; float* Wp;                                    // the weight as the forward's kernels take it
  float* zbA; float* zbB; float* yb; float* ub; float* gb; float* y;     // [M][K]
  float* R; float* RB;                                     // r_i, rb [N][C][H][W]
  float* PT;                                               // patches / COLSt of the explicit paths
  float* T1; float* T2; float* scratch;                    // conv_patches + gram_tn form of dW
  float* part; int splits;                                 // conv_wgrad_kernel's partial tiles
  size_t bytes;
};
ConvBwWorkspace carve_conv_bw(void* base, const ConvGeom& g, int cus) {
  ConvBwWorkspace w;
  Arena a(base, 4);
  const size_t ckk = (size_t)g.C * g.kh * g.kw, M = (size_t)g.N * g.Hz * g.Wz, ldr = (ckk + 3) / 4 * 4;
  const size_t mk = M * g.K * 4, img = (size_t)g.N * g.C * g.H * g.W * 4, kc = ckk * g.K * 4;
  w.Wt = a.take(kc); w.Wp = a.take(ldr * g.K * 4);
  w.zbA = a.take(mk); w.zbB = a.take(mk); w.yb = a.take(mk); w.ub = a.take(mk); w.gb = a.take(mk); w.y = a.take(mk);
  w.R = a.take(img); w.RB = a.take(img);
  w.PT = a.take(ldr * M * 4);
  w.T1 = a.take(kc); w.T2 = a.take(kc); w.scratch = a.take(16 * kc);
  w.splits = std::max(conv_wgrad_splits(g, cus), 1);
  w.part = a.take((size_t)w.splits * kc);
  w.bytes = a.bytes();
  return w;
}
}  // namespace

size_t lasso_conv_ista_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz,
                                                int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F32)) return 0;
  return carve_conv_bw(nullptr, g, std::max(device_cus(), 1)).bytes;
}

int lasso_conv_ista_backward(const void* x_dev, const void* w_dev, const void* trace_dev, const void* grad_z_dev,
                             int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh,
                             int kw, int sh, int sw, int ph, int pw, int dtype, double lr, int fast, int iterations,
                             void* grad_x_dev, void* grad_w_dev, void* grad_z0_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, dtype)) return s;
  if (!w_dev || !workspace_dev || (N > 0 && (!x_dev || !trace_dev || !grad_z_dev)))
    return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (iterations < 0 || !(lr > 0.0)) return fail(LASSO_ERR_BAD_ARG, "iterations=%d lr=%g", iterations, lr);
  if (dtype == LASSO_F64)       // trace and gradients in double; workspace: lasso_conv_ista_backward_workspace_bytes_f64
    return f64::conv_backward((const double*)x_dev, (const double*)w_dev, (const double*)trace_dev,
                              (const double*)grad_z_dev, g, lr, fast, iterations, (double*)grad_x_dev, (double*)grad_w_dev,
                              (double*)grad_z0_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream));
  const int cus = std::max(device_cus(), 1);
  ConvBwWorkspace ws = carve_conv_bw(workspace_dev, g, cus);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ckk = g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4, P = g.Hz * g.Wz;
  const int64_t M = (int64_t)g.N * P, mk = M * g.K, img = (int64_t)g.N * g.C * g.H * g.W, kc = (int64_t)g.K * ckk;
  const float* const X = (const float*)x_dev;
  const float* const conv_w = (const float*)w_dev;
  const float* const trace = (const float*)trace_dev;
  float* const gx = (float*)grad_x_dev;
  float* const gw = (float*)grad_w_dev;
  float* const gz0 = (float*)grad_z0_dev;
  // dW: conv_wgrad_kernel (conv_autograd.hip), or the composition conv_patches + gram_tn where it does not cover the
  // geometry -- or where LASSO_CONV_WGRAD=gram asks for it (the A/B of tools/bench_conv_backward.py)
  const char* form = getenv("LASSO_CONV_WGRAD");
  const int splits = (form && strcmp(form, "gram") == 0) ? 0 : std::min(conv_wgrad_splits(g, cus), ws.splits);
  if (gx && img > 0) LASSO_HIP_TRY(hipMemsetAsync(gx, 0, (size_t)img * 4, st));
  if (gw && (splits == 0 || iterations == 0 || N == 0)) LASSO_HIP_TRY(hipMemsetAsync(gw, 0, (size_t)kc * 4, st));
  if (N == 0) return LASSO_OK;
  if (iterations == 0) {                       // z_T = z_0
    if (gz0) LASSO_HIP_TRY(hipMemcpyAsync(gz0, grad_z_dev, (size_t)mk * 4, hipMemcpyDeviceToDevice, st));
    return LASSO_OK;
  }
  const std::vector<float> coef = fista_coefs(iterations, fast);
  const float lr_f = (float)lr;
  LASSO_HIP_TRY(launch_conv_pack_w(conv_w, ws.Wt, ws.Wp, g.K, ckk, ldr, st));
  float* zb_next = ws.zbA;
  float* zb_cur = ws.zbB;
  LASSO_HIP_TRY(launch_conv_relayout((const float*)grad_z_dev, zb_next, nullptr, g.N, g.K, P, 1, st));
  LASSO_HIP_TRY(hipMemsetAsync(ws.yb, 0, (size_t)mk * 4, st));
  const int gsplits = gram_splits(g.K, ckk, (int)M, 0, cus);
  for (int i = iterations - 1; i >= 0; --i) {
    const float* z_next = trace + (int64_t)(i + 1) * mk;
    const float* z_i = trace + (int64_t)i * mk;
    // zb_{i+1} += (1+c_i) yb_{i+1} ; zb_i = -c_i yb_{i+1} ; ub = [z_{i+1} != 0] zb_{i+1} ; gb = -lr ub
    LASSO_HIP_TRY(launch_bw_prox(zb_next, zb_cur, ws.yb, z_next, ws.ub, ws.gb, mk, coef[i], lr_f, st));
    // rb = conv_transpose2d(gb, W) (no x) ; yb_i = ub + conv2d(rb, W)
    LASSO_HIP_TRY(launch_conv_residual(ws.gb, ws.Wt, conv_w, nullptr, ws.PT, ws.RB, g, cus, st));
    LASSO_HIP_TRY(launch_conv_gradient(ws.RB, ws.Wp, ws.PT, ldr, ws.yb, g, st, ws.ub));
    if (gw) {
      // the point of iteration i, y_i = z_i + c_{i-1} (z_i - z_{i-1}) (y_0 = z_0), and its residual r_i
      LASSO_HIP_TRY(launch_bw_point(z_i, (i > 0 && fast) ? trace + (int64_t)(i - 1) * mk : nullptr, ws.y, mk,
                                    i > 0 ? coef[i - 1] : 0.0f, st));
      if (splits == 0)                         // (PT holds P(rb) until the residual below reuses it)
        LASSO_HIP_TRY(launch_gram_tn(ws.y, g.K, g.K, ws.PT, ldr, ckk, (int)M, ws.T2, ckk, 0, ws.scratch, gsplits, st));
      LASSO_HIP_TRY(launch_conv_residual(ws.y, ws.Wt, conv_w, X, ws.PT, ws.R, g, cus, st));
      // dW += gb^T P(r_i) + y_i^T P(rb)
      if (splits > 0) {
        LASSO_HIP_TRY(launch_conv_wgrad(ws.gb, ws.R, ws.y, ws.RB, ws.part, splits, i != iterations - 1, g, st));
      } else {
        LASSO_HIP_TRY(launch_conv_patches(ws.R, ws.PT, ldr, g, st));
        LASSO_HIP_TRY(launch_gram_tn(ws.gb, g.K, g.K, ws.PT, ldr, ckk, (int)M, ws.T1, ckk, 0, ws.scratch, gsplits, st));
        LASSO_HIP_TRY(launch_bw_axpy(gw, ws.T1, 1.0f, ws.T2, 1.0f, kc, st));
      }
    }
    if (gx) LASSO_HIP_TRY(launch_bw_axpy(gx, ws.RB, -1.0f, nullptr, 0.0f, img, st));    // xb -= rb
    std::swap(zb_next, zb_cur);
  }
  if (gw && splits > 0) LASSO_HIP_TRY(launch_conv_wgrad_sum(ws.part, splits, g, gw, st));
  if (gz0) {
    // z0b = zb_0 + yb_0 (y_0 = z_0), back to [N][K][Hz][Wz]
    LASSO_HIP_TRY(launch_bw_axpy(zb_next, ws.yb, 1.0f, nullptr, 0.0f, mk, st));
    LASSO_HIP_TRY(launch_conv_relayout(zb_next, gz0, nullptr, g.N, g.K, P, 0, st));
  }
  return LASSO_OK;
}

size_t lasso_conv_lip_workspace_bytes(int64_t K, int64_t C, int ksize, int sample) {
  (void)ksize;
  if (K <= 0 || C <= 0 || sample <= 0) return 0;
  return align_up((size_t)sample * 4) + align_up((size_t)std::min(K, C) * 4) + 256;
}

int lasso_conv_lip_bound(const void* w_dev, int64_t K, int64_t C, int ksize, int padding, int sample,
                         int take_sqrt, double* l_out, void* workspace_dev, size_t workspace_bytes,
                         void* stream) {
  if (!w_dev || !workspace_dev || K <= 0 || C <= 0 || ksize <= 0 || sample < 2)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (ksize % 2 != 1) return fail(LASSO_ERR_BAD_ARG, "The dimension of the kernel must be odd.");   // :101-102
  if (workspace_bytes < lasso_conv_lip_workspace_bytes(K, C, ksize, sample))
    return fail(LASSO_ERR_WORKSPACE, "need %zu bytes", lasso_conv_lip_workspace_bytes(K, C, ksize, sample));
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = (char*)workspace_dev;
  float* freq = (float*)base;
  float* maxes = (float*)(base + align_up((size_t)sample * 4));
  double* out = (double*)((char*)maxes + align_up((size_t)std::min(K, C) * 4));
  // torch.linspace(0, 2*pi, sample) in fp32 (:110): start + i*step below the midpoint,
  // end - (sample-1-i)*step above it
  std::vector<float> f(sample);
  const float lo = 0.0f, hi = (float)(2.0 * M_PI);
  const float step = (hi - lo) / (float)(sample - 1);
  for (int i = 0; i < sample; ++i) f[i] = i < sample / 2 ? lo + step * (float)i : hi - step * (float)(sample - 1 - i);
  LASSO_HIP_TRY(hipMemcpyAsync(freq, f.data(), (size_t)sample * 4, hipMemcpyHostToDevice, st));
  LASSO_HIP_TRY(hipStreamSynchronize(st));            // f is a stack-lifetime staging buffer
  const int T = ksize * ksize;
  // the smaller channel dimension is summed last (:106-107)
  const bool swap = K > C;
  const int O = (int)(swap ? C : K), I = (int)(swap ? K : C);
  const int64_t so = swap ? T : (int64_t)C * T, si = swap ? (int64_t)C * T : T;
  if ((size_t)I * T * 4 > 64 * 1024) return fail(LASSO_ERR_UNSUPPORTED, "kernel too large for the bound kernel");
  LASSO_HIP_TRY(launch_conv_lip((const float*)w_dev, O, I, so, si, ksize, padding, freq, sample, take_sqrt, maxes,
                                out, st));
  if (l_out) {
    LASSO_HIP_TRY(hipMemcpyAsync(l_out, out, sizeof(double), hipMemcpyDeviceToHost, st));
    LASSO_HIP_TRY(hipStreamSynchronize(st));
  }
  return LASSO_OK;
}

// ---- float64 forms of the convolutional entry points (conv_f64.hip) ------------------------
size_t lasso_conv_ista_workspace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz,
                                           int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F64)) return 0;
  return f64::conv_workspace_bytes(g);
}

size_t lasso_conv_ista_trace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                                       int kh, int kw, int sh, int sw, int ph, int pw, int iterations) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (iterations < 0 || check_conv(g, LASSO_F64)) return 0;
  return (size_t)(iterations + 1) * (size_t)N * Hz * Wz * K * 8;
}

size_t lasso_conv_ista_backward_workspace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz,
                                                    int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (check_conv(g, LASSO_F64)) return 0;
  return f64::conv_backward_workspace_bytes(g);
}

int lasso_conv_ista_solve_f64(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev, int64_t N,
                              int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh,
                              int sw, int ph, int pw, double alpha, double lr, int fast, int maxiter, double tol,
                              int32_t* iters_out, double* last_delta_out, void* workspace_dev, size_t workspace_bytes,
                              void* stream) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, LASSO_F64)) return s;
  if (!w_dev || !workspace_dev || (N > 0 && (!x_dev || !z_out_dev))) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (maxiter < 0 || !(lr > 0.0) || !(alpha >= 0.0)) return fail(LASSO_ERR_BAD_ARG, "maxiter=%d lr=%g alpha=%g", maxiter, lr, alpha);
  return f64::conv_solve((const double*)x_dev, (const double*)w_dev, (const double*)z0_dev, (double*)z_out_dev, g, alpha,
                         lr, fast, maxiter, tol, nullptr, iters_out, last_delta_out, workspace_dev, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

int lasso_conv_objective_f64(const void* x_dev, const void* w_dev, const void* z_dev, int64_t N, int64_t C, int64_t H,
                             int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw,
                             double alpha, double* loss_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const ConvGeom g = make_geom(N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw);
  if (int s = check_conv(g, LASSO_F64)) return s;
  if (!x_dev || !w_dev || !z_dev || !loss_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (N == 0) return fail(LASSO_ERR_BAD_ARG, "empty batch");
  return f64::conv_objective((const double*)x_dev, (const double*)w_dev, (const double*)z_dev, g, alpha, loss_dev, nullptr,
                             workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t lasso_conv_lip_workspace_bytes_f64(int64_t K, int64_t C, int ksize, int sample) {
  (void)ksize;
  if (K <= 0 || C <= 0 || sample <= 0) return 0;
  return f64::conv_lip_workspace_bytes(K, C, sample);
}

int lasso_conv_lip_bound_f64(const void* w_dev, int64_t K, int64_t C, int ksize, int padding, int sample, int take_sqrt,
                             double* l_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!w_dev || !workspace_dev || K <= 0 || C <= 0 || ksize <= 0 || sample < 2)
    return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (ksize % 2 != 1) return fail(LASSO_ERR_BAD_ARG, "The dimension of the kernel must be odd.");   // :101-102
  return f64::conv_lip_bound((const double*)w_dev, K, C, ksize, padding, sample, take_sqrt, l_out, workspace_dev,
                             workspace_bytes, static_cast<hipStream_t>(stream));
}

// ---- reverse-mode derivative of the unrolled fixed-step solve (autograd.hip) --------------
namespace {
struct BwWorkspace { float* Wt; float* zbA; float* zbB; float* yb; float* ub; float* gb; float* y; float* nr; float* rb; float* T1; float* T2; float* scratch; size_t bytes; };
BwWorkspace carve_bw(void* base, int64_t n, int64_t d, int64_t k) {
  BwWorkspace w;
  Arena a(base, 4);
  const size_t nk = (size_t)n * k * 4, nd = (size_t)n * d * 4, dk = (size_t)d * k * 4;
  w.Wt = a.take(dk);
  w.zbA = a.take(nk); w.zbB = a.take(nk); w.yb = a.take(nk); w.ub = a.take(nk); w.gb = a.take(nk); w.y = a.take(nk);
  w.nr = a.take(nd); w.rb = a.take(nd);
  w.T1 = a.take(dk); w.T2 = a.take(dk);
  w.scratch = a.take(16 * dk);
  w.bytes = a.bytes();
  return w;
}
}  // namespace

size_t lasso_fista_backward_workspace_bytes(int64_t n, int64_t d, int64_t k) {
  if (n < 0 || d <= 0 || k <= 0) return 0;
  return carve_bw(nullptr, n, d, k).bytes;
}

int lasso_fista_backward(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* trace_dev,
                         const void* grad_z_dev, int64_t n, int64_t d, int64_t k, int dtype, double lr, int fast,
                         int iterations, void* grad_x_dev, void* grad_w_dev, void* grad_z0_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream) {
  return lasso_fista_backward_steps(x_dev, ldx, w_dev, ldw, trace_dev, grad_z_dev, n, d, k, dtype, lr, nullptr, fast,
                                    iterations, grad_x_dev, grad_w_dev, grad_z0_dev, workspace_dev, workspace_bytes,
                                    stream);
}

int lasso_fista_backward_steps(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* trace_dev,
                               const void* grad_z_dev, int64_t n, int64_t d, int64_t k, int dtype, double lr,
                               const float* lr_steps_host, int fast, int iterations, void* grad_x_dev,
                               void* grad_w_dev, void* grad_z0_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream) {
  if (int s = check_common(n, d, k, dtype, /*allow_large=*/true)) return s;
  if (!x_dev || !w_dev || !trace_dev || !grad_z_dev || !workspace_dev) return fail(LASSO_ERR_BAD_ARG, "null pointer");
  if (ldx < d || ldw < k || iterations < 0) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  if (d > INT32_MAX / 2 || k > INT32_MAX / 2) return fail(LASSO_ERR_UNSUPPORTED, "shape too large");
  BwWorkspace ws = carve_bw(workspace_dev, n, d, k);
  if (workspace_bytes < ws.bytes) return fail(LASSO_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* X = (const float*)x_dev;
  const float* W = (const float*)w_dev;
  const float* trace = (const float*)trace_dev;
  const int64_t nk = n * k;
  float* gx = (float*)grad_x_dev;
  float* gw = (float*)grad_w_dev;
  float* gz0 = (float*)grad_z0_dev;
  if (gx && n > 0) LASSO_HIP_TRY(hipMemsetAsync(gx, 0, (size_t)n * d * 4, st));
  if (gw) LASSO_HIP_TRY(hipMemsetAsync(gw, 0, (size_t)d * k * 4, st));
  if (n == 0) return LASSO_OK;
  const int cus = device_cus();
  // momentum coefficients c_i = (t_i - 1)/t_{i+1}  (ista.py:98-99)
  const std::vector<float> coef = fista_coefs(iterations, fast);
  LASSO_HIP_TRY(launch_transpose_pad(W, ldw, (int)d, (int)k, ws.Wt, d, (int)k, (int)d, st));
  float* zb_next = ws.zbA;
  float* zb_cur = ws.zbB;
  LASSO_HIP_TRY(hipMemcpyAsync(zb_next, grad_z_dev, (size_t)nk * 4, hipMemcpyDeviceToDevice, st));
  LASSO_HIP_TRY(hipMemsetAsync(ws.yb, 0, (size_t)nk * 4, st));
  const int splits = gram_splits((int)d, (int)k, (int)n, 0, cus);
  for (int i = iterations - 1; i >= 0; --i) {
    const float* z_next = trace + (int64_t)(i + 1) * nk;
    const float* z_i = trace + (int64_t)i * nk;
    // c_i formed y_{i+1}; for the last iteration y_{i+1} was never used (yb == 0)
    LASSO_HIP_TRY(launch_bw_prox(zb_next, zb_cur, ws.yb, z_next, ws.ub, ws.gb, nk, coef[i],
                                 lr_steps_host ? lr_steps_host[i] : (float)lr, st));
    // the point of iteration i:  y_i = z_i + c_{i-1} (z_i - z_{i-1}),  y_0 = z_0
    LASSO_HIP_TRY(launch_bw_point(z_i, (i > 0 && fast) ? trace + (int64_t)(i - 1) * nk : nullptr, ws.y, nk,
                                  i > 0 ? coef[i - 1] : 0.0f, st));
    // nr = x - y W^T (= -r_i);  rb = gb W^T;  yb_i = ub + rb W
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.y, k, W, ldw, X, ldx, ws.nr, d, (int)n, (int)d, (int)k, st, 0));
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.gb, k, W, ldw, nullptr, 0, ws.rb, d, (int)n, (int)d, (int)k, st, 1));
    LASSO_HIP_TRY(launch_gemm_nt_sub(ws.rb, d, ws.Wt, d, ws.ub, k, ws.yb, k, (int)n, (int)k, (int)d, st, 1));
    if (gw) {
      // Wb += r_i^T gb + rb^T y_i = -(nr^T gb) + rb^T y_i
      LASSO_HIP_TRY(launch_gram_tn(ws.nr, d, (int)d, ws.gb, k, (int)k, (int)n, ws.T1, k, 0, ws.scratch, splits, st));
      LASSO_HIP_TRY(launch_gram_tn(ws.rb, d, (int)d, ws.y, k, (int)k, (int)n, ws.T2, k, 0, ws.scratch, splits, st));
      LASSO_HIP_TRY(launch_bw_axpy(gw, ws.T2, 1.0f, ws.T1, -1.0f, d * k, st));
    }
    if (gx) LASSO_HIP_TRY(launch_bw_axpy(gx, ws.rb, -1.0f, nullptr, 0.0f, n * d, st));
    std::swap(zb_next, zb_cur);       // zb_cur (adjoint of z_i so far) becomes the next "zb_{i+1}"
  }
  if (gz0) {
    // z0b = zb_0 + yb_0  (y_0 = z_0)
    LASSO_HIP_TRY(hipMemcpyAsync(gz0, zb_next, (size_t)nk * 4, hipMemcpyDeviceToDevice, st));
    LASSO_HIP_TRY(launch_bw_axpy(gz0, ws.yb, 1.0f, nullptr, 0.0f, nk, st));
  }
  return LASSO_OK;
}

// ---- patch front end (conv.hip) --------------------------------------------------------
namespace {
int patch_geom(ConvGeom& g, int64_t N, int64_t C, int64_t H, int64_t W, int ph, int pw, int sh, int sw) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || ph <= 0 || pw <= 0 || sh <= 0 || sw <= 0 || ph > H || pw > W)
    return fail(LASSO_ERR_BAD_ARG, "bad patch geometry");
  g = make_geom(N, C, H, W, 1, (H - ph) / sh + 1, (W - pw) / sw + 1, ph, pw, sh, sw, 0, 0);
  if ((int64_t)g.N * g.Hz * g.Wz > INT32_MAX / 2) return fail(LASSO_ERR_UNSUPPORTED, "too many patches");
  return LASSO_OK;
}
}  // namespace

int lasso_patches_extract(const void* img_dev, void* patches_dev, int64_t ld, float* means_dev, int64_t N,
                          int64_t C, int64_t H, int64_t W, int ph, int pw, int sh, int sw, int center,
                          void* stream) {
  ConvGeom g;
  if (int s = patch_geom(g, N, C, H, W, ph, pw, sh, sw)) return s;
  if ((N > 0 && (!img_dev || !patches_dev)) || ld < (int64_t)C * ph * pw) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  LASSO_HIP_TRY(launch_patches_extract((const float*)img_dev, (float*)patches_dev, ld, means_dev, g, center,
                                       static_cast<hipStream_t>(stream)));
  return LASSO_OK;
}

int lasso_patches_reconstruct(const void* patches_dev, int64_t ld, const float* means_dev, void* img_out_dev,
                              int64_t N, int64_t C, int64_t H, int64_t W, int ph, int pw, int sh, int sw,
                              void* stream) {
  ConvGeom g;
  if (int s = patch_geom(g, N, C, H, W, ph, pw, sh, sw)) return s;
  if ((N > 0 && (!img_out_dev || !patches_dev)) || ld < (int64_t)C * ph * pw) return fail(LASSO_ERR_BAD_ARG, "bad argument");
  LASSO_HIP_TRY(launch_patches_reconstruct((const float*)patches_dev, ld, means_dev, (float*)img_out_dev, g,
                                           static_cast<hipStream_t>(stream)));
  return LASSO_OK;
}

}  // extern "C"
