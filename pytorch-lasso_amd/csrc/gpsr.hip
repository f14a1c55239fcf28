// GPSR-Basic on the dictionary (the reference's lasso/linear/solvers/gpsr.py with A z = z W^T, AT r = r W): the operator
// that gpsr_driver.hpp's host loop is instantiated with for lasso_gpsr_solve.  Every [n,k] x [k,d]-class product is ONE
// launch of solver_common.hpp's GEMM with the epilogue the loop asks for; the epilogues, the decision kernels, the control
// block and the loop itself are in the driver's header and serve the convolutional operator of conv_gpsr.hip as well.
#include "gpsr_driver.hpp"

namespace lasso {
namespace gpsr {
namespace {

// y = x [n][d] (pitch ldx), the code [n][k], the dictionary w [d][k] (pitch ldw) and its transpose Wt [k][d]
struct LinearOp {
  // what the loop reads
  int rows, cols;
  int64_t nd;
  int pk, pd;
  const float* y; int64_t ldy; int y_rows, y_cols;
  const float* start; int64_t ld_start;
  // the operator's own
  const float* w; int64_t ldw;
  float* Wt;
  float* zout; int64_t ldz;
  int d, side_k, side_d;

  hipError_t prepare(hipStream_t st) const { return launch_transpose_pad(w, ldw, d, cols, Wt, d, cols, d, st); }

  // AT(img) = img W: [n,d] x [d,k]; the data itself has the caller's pitch, every other image is packed
  template <int MODE>
  hipError_t at(const float* img, const Epi& ep, hipStream_t st) const {
    return launch_gemm<MODE>(img, img == y ? ldy : (int64_t)d, Wt, d, rows, cols, d, ep, side_k, 1, st);
  }

  // A(code) = code W^T: [n,k] x [k,d]
  template <int MODE>
  hipError_t a(const float* code, Epi ep, int rungs, hipStream_t st) const {
    ep.Y = y; ep.ldy = ldy; ep.ldo = d;
    return launch_gemm<MODE>(code, cols, w, ldw, rows, d, cols, ep, side_d, rungs, st);
  }

  hipError_t write_out(const float* Z, int zero, hipStream_t st) const {
    hipLaunchKernelGGL(copy_out_kernel<>, dim3(ew_grid((int64_t)rows * cols)), dim3(256), 0, st, Z, zout, ldz, rows, cols, zero);
    return hipGetLastError();
  }
};

struct LinearSpace {
  float* Wt;
  Space common;
  size_t bytes;
};

LinearSpace carve(void* base, int64_t n, int64_t d, int64_t k) {
  LinearSpace w;
  Arena a(base);
  w.Wt = a.take((size_t)k * d * 4);
  // block partials: 64 x 64 blocks give the most
  w.common = carve_common(a, n * k, n * d, gemm_parts((int)n, (int)k, 64), gemm_parts((int)n, (int)d, 64));
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t workspace_bytes(int64_t n, int64_t d, int64_t k) { return carve(nullptr, n, d, k).bytes + 256; }

int block_side_here(int m, int nn, int64_t ldmax) { return block_side(m, nn, ldmax, solver::device_cus()); }

int solve(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* z0, int64_t ldz0, float* zout, int64_t ldz,
          int64_t n64, int64_t d64, int64_t k64, double alpha, const lasso_gpsr_options& o, lasso_gpsr_result* res,
          void* workspace, hipStream_t st) {
  const int n = (int)n64, d = (int)d64, k = (int)k64;
  const LinearSpace ws = carve(workspace, n, d, k);
  const int cus = solver::device_cus();
  if (std::max<int64_t>({(int64_t)d, (int64_t)k, ldx, ldw}) * 64 * 4 >= ((int64_t)1 << 31)) {
    return fail(LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block");
  }
  LinearOp op;
  op.rows = n; op.cols = k; op.nd = (int64_t)n * d;
  const int64_t ldmax_k = std::max<int64_t>({(int64_t)d, (int64_t)k, ldx}), ldmax_d = std::max<int64_t>(ldmax_k, ldw);
  // LASSO_FORCE_BLOCKS_128 (tests): 128 x 128 blocks below the size at which block_side takes them
  const bool force128 = (o.reserved & LASSO_FORCE_BLOCKS_128) && ldmax_d * 128 * 4 < ((int64_t)1 << 31);
  op.side_k = force128 ? 128 : block_side(n, k, ldmax_k, cus);           // products [n,k]
  op.side_d = force128 ? 128 : block_side(n, d, ldmax_d, cus);           // products [n,d]
  op.pk = gemm_parts(n, k, op.side_k);
  op.pd = gemm_parts(n, d, op.side_d);
  op.y = x; op.ldy = ldx; op.y_rows = n; op.y_cols = d;
  op.start = z0; op.ld_start = ldz0;
  op.w = w; op.ldw = ldw; op.Wt = ws.Wt; op.zout = zout; op.ldz = ldz; op.d = d;
  return solve_with(op, ws.common, alpha, o, res, st);
}

}  // namespace gpsr
}  // namespace lasso
