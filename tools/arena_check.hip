// Host-only check of the workspace carving (csrc/host_util.hpp: Arena) and of the solve's region layout
// (lasso_hip.hip: solve_regions) under AddressSanitizer / UBSan.  No kernel is launched and no device is needed.
//
// Every carve function is run twice at three shapes: with a null base (all pointers must be null: the size queries) and
// with a malloc'ed base of exactly bytes(); then the first and the last byte of every region are written.  An offset or
// a size that left the block would be a heap-buffer-overflow report.
//
// The carve functions live in anonymous namespaces, so this program includes the three translation units that hold
// them and links the objects of the ordinary build for the rest (mstep.hip among them: its plan is checked by value):
//
//   cd pytorch-lasso_amd/csrc && make
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -c ../../tools/arena_check.hip -o /tmp/arena_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/arena_check.o \
//       $(ls build/*.o | grep -v -e /lasso_hip.o -e /gemm_f64.o -e /gpsr.o -e /conv_gpsr.o) -o /tmp/arena_check && /tmp/arena_check
//
// Run it on the build machine, never on a machine whose GPU others share.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

struct Seen { char* p; size_t bytes; };
static std::vector<Seen> g_seen;
#define LASSO_ARENA_OBSERVER(ptr, bytes) g_seen.push_back(Seen{ptr, bytes})

#include "../pytorch-lasso_amd/csrc/lasso_hip.hip"
#include "../pytorch-lasso_amd/csrc/gemm_f64.hip"
#include "../pytorch-lasso_amd/csrc/gpsr.hip"
#include "../pytorch-lasso_amd/csrc/conv_gpsr.hip"

static int g_checked = 0, g_regions = 0;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// carve_fn(base) -> bytes of the workspace
template <class F>
static void check(const char* what, F carve_fn) {
  g_seen.clear();
  const size_t bytes = carve_fn(nullptr);
  for (const Seen& s : g_seen) REQUIRE(s.p == nullptr);
  const size_t count = g_seen.size();
  char* base = static_cast<char*>(malloc(bytes ? bytes : 1));
  REQUIRE(base != nullptr);
  g_seen.clear();
  REQUIRE(carve_fn(base) == bytes);
  REQUIRE(g_seen.size() == count);
  char* expect = base;
  for (const Seen& s : g_seen) {
    REQUIRE(s.p == expect);                                   // regions follow each other, 256-byte aligned
    REQUIRE((size_t)(s.p - base) % 256 == 0);
    REQUIRE((size_t)(s.p - base) + s.bytes <= bytes);
    if (s.bytes) { s.p[0] = 1; s.p[s.bytes - 1] = 2; }
    expect = s.p + align_up(s.bytes);
    ++g_regions;
  }
  REQUIRE(expect == base + bytes);
  free(base);
  ++g_checked;
  printf("%-28s %12zu bytes, %2zu regions\n", what, bytes, count);
}

int main() {
  struct Shape { int64_t n, d, k; };
  const Shape shapes[] = {{37, 8, 12}, {4096, 64, 300}, {37, 300, 520}};
  for (const Shape& s : shapes) {
    const int64_t n = s.n, d = s.d, k = s.k;
    printf("n=%lld d=%lld k=%lld\n", (long long)n, (long long)d, (long long)k);
    if (fused_shape(d, k)) {
      const int kp = pad_k(k);
      check("carve", [&](void* b) { return carve(b, n, k, kp, 100, true).bytes; });
      check("carve (no state)", [&](void* b) { return carve(b, n, k, kp, 0, false).bytes; });
      check("carve_bt", [&](void* b) { return carve_bt(b, n, k, kp, false, 10).bytes; });
      check("carve_bt (bf16)", [&](void* b) { return carve_bt(b, n, k, kp, true, 10).bytes; });
    }
    check("carve_generic", [&](void* b) { return carve_generic(b, n, d, k, false, true).bytes; });
    check("carve_generic (line search)", [&](void* b) { return carve_generic(b, n, d, k, true, false).bytes; });
    check("carve_cd", [&](void* b) { return carve_cd(b, n, d, pad_k_cd(k)).bytes; });
    check("carve_bw", [&](void* b) { return carve_bw(b, n, d, k).bytes; });
    check("f64::carve", [&](void* b) { return lasso::f64::carve(b, n, d, k, false, true).bytes; });
    check("f64::carve (line search)", [&](void* b) { return lasso::f64::carve(b, n, d, k, true, false).bytes; });
    check("gpsr::carve", [&](void* b) { return lasso::gpsr::carve(b, n, d, k).bytes; });
    // the solve's regions, every dtype: solver | objective | lipschitz fill lasso_fista_workspace_bytes exactly
    for (int dtype : {LASSO_F32, LASSO_BF16, LASSO_F64})
      for (int backtrack : {0, 1}) {
        const SolveRegions r = solve_regions(n, d, k, dtype, 10, 1e-5, LASSO_STOP_GLOBAL, backtrack);
        REQUIRE(r.total == lasso_fista_workspace_bytes(n, d, k, dtype, 10, 1e-5, LASSO_STOP_GLOBAL, backtrack));
        if (r.total == 0) continue;
        REQUIRE(r.total == r.solver + r.objective + r.lipschitz);
        char* base = static_cast<char*>(malloc(r.total));
        REQUIRE(base != nullptr);
        Arena a(base);
        const size_t sizes[] = {r.solver, r.objective, r.lipschitz};
        for (size_t bytes : sizes) {
          REQUIRE(bytes % 256 == 0);
          char* p = a.take<char>(bytes);
          if (bytes) { p[0] = 1; p[bytes - 1] = 2; }
        }
        REQUIRE(a.bytes() == r.total);
        free(base);
        ++g_checked;
      }
  }
  // the convolution workspaces (every region at least 4 bytes) and the pipelined M-step's scratch offsets
  const ConvGeom geoms[] = {make_geom(1, 1, 6, 6, 2, 4, 4, 3, 3, 1, 1, 0, 0), make_geom(64, 3, 64, 64, 128, 64, 64, 5, 5, 1, 1, 2, 2),
                            make_geom(0, 1, 6, 6, 2, 4, 4, 3, 3, 1, 1, 0, 0)};
  for (const ConvGeom& g : geoms) {
    check("carve_conv", [&](void* b) { return carve_conv(b, g).bytes; });
    check("carve_conv_bw", [&](void* b) { return carve_conv_bw(b, g, 256).bytes; });
    check("gpsr::carve (conv)", [&](void* b) { return lasso::gpsr::carve(b, g).bytes; });
  }
  for (int64_t k : {512, 1024, 4096}) {      // (mstep.hip comes from the ordinary build: offsets only, nothing observed)
    const MstepPipePlan pl = mstep_pipe_plan(70000, 256, k, 256);
    REQUIRE(pl.nstages > 0 && pl.scratch_off[0] == 0);
    for (int s = 0; s < pl.nstages; ++s) {
      const size_t end = s + 1 < pl.nstages ? pl.scratch_off[s + 1] : pl.scratch_bytes;
      const size_t need = (size_t)pl.splits[s] * (pl.hi[s] - pl.lo[s]) * 256 * (size_t)(k + 256) * 4;
      REQUIRE(pl.scratch_off[s] % 256 == 0 && end == pl.scratch_off[s] + align_up(need));
    }
    ++g_checked;
  }
  printf("arena_check: %d layouts, %d regions touched: ok\n", g_checked, g_regions);
  return 0;
}
