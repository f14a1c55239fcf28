// Convolutional GPSR-Basic: gpsr_driver.hpp's host loop on the operator
//   A z  = conv_transpose2d(z, W)      AT r = conv2d(r, W)
// (the two closures a user of the reference's gpsr_basic(y, A, tau, AT, ...) passes for a convolutional dictionary).
//
// Layout, as in conv.hip: the code stays a MATRIX Zm [M = N*Hz*Wz][K] for the whole solve -- relaid out once on the way
// in (z0) and once on the way out -- so u, v, t, c and the rung candidates are [M][K] matrices and every decision kernel
// of the driver works on them unchanged; rb and y are NCHW images.
//   AT(img):  RC [M][ldr] = pixel-major patches of img (conv_patches_kernel), then the driver's GEMM RC Wp^T with the
//             epilogue the loop asks for (EPI_STORE / EPI_GRAD / EPI_MASK_*), contraction over the C kh kw taps
//   A(code):  COLSt [C kh kw][M] = Wt code^T through the same GEMM (EPI_STORE), then conv_gpsr_overlap_add_kernel: the
//             gather of conv_residual_kernel (no atomics) with the data-shaped epilogue -- |A c|^2 only, store rb+ with
//             the block partials of |y - rb+|^2 (blockIdx.z = rung), store A z - y, or the plain store of the debias CG
// That is the general form ("patches": any C, K, kernel size, stride, padding).  The implicit form ("implicit") takes the
// geometries the implicit-GEMM kernels of the ISTA path cover -- the coverage rule of lasso_conv_ista_kernel_name: stride
// 1, few channels, 3/5/7 kernels, K a multiple of 4 -- and removes both round trips from the hot products:
//   AT(rb) GRAD:  conv_grad_prox_kernel<.., GPSR = true> (conv.hip): the same implicit GEMM with GPSR's GRAD epilogue
//   A(code):      conv_synth_kernel / conv_synth_few_kernel as they are (x = null: A z; x = y: A z - y), then
//                 conv_gpsr_image_epi_kernel over the IMAGE for the block partials -- the image is C H W / (K Hz Wz) of
//                 the code's bytes (1.5 - 6 % at the benchmark geometries), so the synthesis kernels stay untouched and
//                 their ISTA use is bitwise what it was by construction
// AT(y) once per solve and the two masked products of the debias CG stay on the general form.
// options.reserved bit 0 forces the general form.
// Reductions as everywhere in the driver: per thread, wave butterfly, block partial in double, one workgroup folds the
// partials in a fixed order; two solves of the same arguments are bitwise equal.
// Bound of the general form: the patch matrix and COLSt make one round trip through HBM per product (M C kh kw floats each
// way); the implicit form has neither.
#include "gpsr_driver.hpp"

namespace lasso {
namespace gpsr {
namespace {

// image[n][c][i][j] = sum_{a,b} COLSt[(c,a,b)][(n,u,v)], u = (i + ph - a)/sh, v = (j + pw - b)/sw where they are integers
// inside the code grid; blockIdx.z = rung (COLSt cols_stride apart, images out_stride apart).  MODE:
//   EPI_SUMSQ   sum image^2, nothing stored        EPI_RESID   store image, sum (y - image)^2
//   EPI_RESID0  store image - y, sum of its squares  EPI_STORE   store image
template <int MODE>
__global__ __launch_bounds__(256) void conv_gpsr_overlap_add_kernel(const float* __restrict__ colst, int64_t cols_stride,
                                                                    const float* __restrict__ y, float* __restrict__ out,
                                                                    int64_t out_stride, const ConvGeom g,
                                                                    double* __restrict__ part) {
  __shared__ double red[32];
  const int64_t total = (int64_t)g.N * g.C * g.H * g.W;
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz;
  colst += (int64_t)blockIdx.z * cols_stride;
  if (MODE != EPI_SUMSQ) out += (int64_t)blockIdx.z * out_stride;
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % g.W);
    const int i = (int)((e / g.W) % g.H);
    const int c = (int)((e / ((int64_t)g.W * g.H)) % g.C);
    const int n = (int)(e / ((int64_t)g.W * g.H * g.C));
    float acc = 0.0f;
    if (g.sh == 1 && g.sw == 1) {               // the usual case: no divisions in the tap loops
      const int a_lo = max(0, i + g.ph - (g.Hz - 1)), a_hi = min(g.kh - 1, i + g.ph);
      const int b_lo = max(0, j + g.pw - (g.Wz - 1)), b_hi = min(g.kw - 1, j + g.pw);
      for (int a = a_lo; a <= a_hi; ++a) {
        const int u = i + g.ph - a;
        const float* row = colst + ((int64_t)n * g.Hz + u) * g.Wz + (j + g.pw);
        const int64_t tb = ((int64_t)c * g.kh + a) * g.kw;
        for (int b = b_lo; b <= b_hi; ++b) acc = __fadd_rn(acc, row[(tb + b) * M - b]);
      }
    } else {
      for (int a = 0; a < g.kh; ++a) {
        const int ii = i + g.ph - a;
        if (ii < 0 || ii % g.sh != 0) continue;
        const int u = ii / g.sh;
        if (u >= g.Hz) continue;
        for (int b = 0; b < g.kw; ++b) {
          const int jj = j + g.pw - b;
          if (jj < 0 || jj % g.sw != 0) continue;
          const int v = jj / g.sw;
          if (v >= g.Wz) continue;
          const int64_t t = ((int64_t)c * g.kh + a) * g.kw + b;
          acc = __fadd_rn(acc, colst[t * M + ((int64_t)n * g.Hz + u) * g.Wz + v]);
        }
      }
    }
    if constexpr (MODE == EPI_SUMSQ) {
      s[0] += (double)__fmul_rn(acc, acc);
    } else if constexpr (MODE == EPI_RESID) {
      const float r = __fsub_rn(y[e], acc);
      s[0] += (double)__fmul_rn(r, r);
      out[e] = acc;
    } else if constexpr (MODE == EPI_RESID0) {
      const float r = __fsub_rn(acc, y[e]);
      s[0] += (double)__fmul_rn(r, r);
      out[e] = r;
    } else {
      out[e] = acc;
    }
  }
  if constexpr (MODE != EPI_STORE) block_fold<1, 0>(s, nomax, red, part + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * kPart);
}

// block partials of an image the synthesis kernels stored (blockIdx.z = rung, images img_stride apart):
//   EPI_RESID: sum (y - img)^2 (img = A z+)      EPI_RESID0 / EPI_SUMSQ: sum img^2 (img = A z - y / A c)
template <int MODE>
__global__ __launch_bounds__(256) void conv_gpsr_image_epi_kernel(const float* __restrict__ img, int64_t img_stride,
                                                                  const float* __restrict__ y, int64_t total,
                                                                  double* __restrict__ part) {
  __shared__ double red[32];
  img += (int64_t)blockIdx.z * img_stride;
  double s[1] = {0.0};
  float nomax[1] = {0.0f};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const float r = MODE == EPI_RESID ? __fsub_rn(y[e], img[e]) : img[e];
    s[0] += (double)__fmul_rn(r, r);
  }
  block_fold<1, 0>(s, nomax, red, part + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * kPart);
}

// x [N][C][H][W], the code rows [M][K], the weight w [K][C][kh][kw] packed as Wt [C kh kw][K] and Wp [K][ldr]
struct ConvOp {
  // what the loop reads
  int rows, cols;
  int64_t nd;
  int pk, pd;
  const float* y; int64_t ldy; int y_rows, y_cols;
  const float* start; int64_t ld_start;
  // the operator's own
  ConvGeom g;
  const float* w; const float* z0;
  float *Wt, *Wp, *RC, *COLSt, *Z0m, *IMG;
  float* zout;
  int ckk, ldr, side_k, side_c;
  bool implicit; int cus, pk_cap, pk_gemm;

  hipError_t prepare(hipStream_t st) const {
    if (hipError_t e = launch_conv_pack_w(w, Wt, Wp, g.K, ckk, ldr, st); e != hipSuccess) return e;
    if (z0) return launch_conv_relayout(z0, Z0m, nullptr, g.N, g.K, g.Hz * g.Wz, 1, st);
    return hipSuccess;
  }

  // AT(img) = conv2d(img, W) in row layout: patches, then RC Wp^T with the loop's epilogue
  template <int MODE>
  hipError_t at(const float* img, const Epi& ep, hipStream_t st) const {
    if (implicit) {
      // (the two forms leave different numbers of block partials: the folds read pk of them, the rest are zeros)
      if (MODE != EPI_STORE && pk > 0)
        if (hipError_t e = hipMemsetAsync(ep.part, 0, (size_t)pk * kPart * 8, st); e != hipSuccess) return e;
      if constexpr (MODE == EPI_GRAD) {
        ConvGradGpsr ge = {ep.Ay, ep.U, ep.V, ep.T, ep.Cc, ep.part, ep.tau};
        int count = 0;
        if (hipError_t e = launch_conv_grad_prox(img, Wp, ldr, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, pk_cap, g, cus, &count,
                                                 st, 0, &ge);
            e != hipSuccess)
          return e;
        return count > 0 && count <= pk ? hipSuccess : hipErrorInvalidValue;     // (covered: the dry run at set-up said so)
      }
    }
    if (hipError_t e = launch_conv_patches(img, RC, ldr, g, st); e != hipSuccess) return e;
    return launch_gemm<MODE>(RC, ldr, Wp, ldr, rows, cols, ldr, ep, side_k, 1, st);
  }

  // A(code) = conv_transpose2d(code, W): COLSt = Wt code^T per rung, then one overlap-add launch over the rungs
  template <int MODE>
  hipError_t a(const float* code, const Epi& ep, int rungs, hipStream_t st) const {
    if (implicit) {
      float* const dst = MODE == EPI_SUMSQ ? IMG : ep.Out;
      const int64_t dstride = MODE == EPI_SUMSQ ? 0 : ep.out_stride;
      for (int r = 0; r < rungs; ++r) {
        bool done = false;
        const float* const zr = code + r * ep.a_stride;
        const float* const sub = MODE == EPI_RESID0 ? y : nullptr;
        if (hipError_t e = launch_conv_synth(zr, w, sub, dst + r * dstride, g, cus, &done, st); e != hipSuccess) return e;
        if (!done)
          if (hipError_t e = launch_conv_synth_few(zr, w, sub, dst + r * dstride, g, cus, &done, st); e != hipSuccess) return e;
        if (!done) return hipErrorInvalidValue;                                    // (covered: the dry run at set-up said so)
      }
      if constexpr (MODE != EPI_STORE) {
        hipLaunchKernelGGL(conv_gpsr_image_epi_kernel<MODE>, dim3(pd, 1, rungs), dim3(256), 0, st, dst, dstride, y, nd, ep.part);
        return hipGetLastError();
      }
      return hipSuccess;
    }
    const int64_t cm = (int64_t)ckk * rows;
    for (int r = 0; r < rungs; ++r) {
      Epi ec = {};
      ec.Out = COLSt + r * cm; ec.ldo = rows;
      if (hipError_t e = launch_gemm<EPI_STORE>(Wt, cols, code + r * ep.a_stride, cols, ckk, rows, cols, ec, side_c, 1, st);
          e != hipSuccess)
        return e;
    }
    hipLaunchKernelGGL(conv_gpsr_overlap_add_kernel<MODE>, dim3(pd, 1, rungs), dim3(256), 0, st, COLSt, cm, y, ep.Out,
                       ep.out_stride, g, ep.part);
    return hipGetLastError();
  }

  hipError_t write_out(const float* Z, int zero, hipStream_t st) const {
    if (zero) return hipMemsetAsync(zout, 0, (size_t)rows * cols * 4, st);
    return launch_conv_relayout(Z, zout, nullptr, g.N, g.K, g.Hz * g.Wz, 0, st);
  }
};

struct ConvSpace {
  float *Wt, *Wp, *RC, *COLSt, *Z0m, *IMG;
  Space common;
  size_t bytes;
};

ConvSpace carve(void* base, const ConvGeom& g) {
  ConvSpace w;
  Arena a(base);
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ckk = (int64_t)g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4;
  const int64_t nk = M * g.K, nd = (int64_t)g.N * g.C * g.H * g.W;
  w.Wt = a.take((size_t)ckk * g.K * 4);
  w.Wp = a.take((size_t)g.K * ldr * 4);
  w.RC = a.take((size_t)M * ldr * 4);
  w.COLSt = a.take((size_t)ckk * M * 4 * kLadder);
  w.Z0m = a.take((size_t)nk * 4);
  w.IMG = a.take((size_t)nd * 4);
  w.common = carve_common(a, nk, nd, gemm_parts((int)M, g.K, 64), kEwBlocks);
  w.bytes = a.bytes();
  return w;
}

}  // namespace

size_t conv_workspace_bytes(const ConvGeom& g) { return carve(nullptr, g).bytes + 256; }

// the coverage rule of lasso_conv_ista_kernel_name, asked of the launchers themselves (their dry runs): the synthesis
// side by conv_synth / conv_synth_few AND the gradient side by conv_grad_prox; *count = the gradient kernel's partials
static bool implicit_covered(const ConvGeom& g, int cus, int cap, int* count) {
  static const float kAligned[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  bool synth = false, few = false;
  *count = 0;
  (void)launch_conv_synth(kAligned, kAligned, kAligned, nullptr, g, cus, &synth, nullptr, 1);
  if (!synth) (void)launch_conv_synth_few(kAligned, kAligned, kAligned, nullptr, g, cus, &few, nullptr, 1);
  if (!synth && !few) return false;
  (void)launch_conv_grad_prox(nullptr, nullptr, 0, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, cap, g, cus, count, nullptr, 1);
  return *count > 0;
}

const char* conv_form(const ConvGeom& g, int forced_general) {
  int count = 0;
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz;
  if (forced_general || g.N <= 0) return "patches";
  return implicit_covered(g, solver::device_cus(), gemm_parts((int)M, g.K, 64), &count) ? "implicit" : "patches";
}

int conv_solve(const float* x, const float* w, const float* z0, float* zout, const ConvGeom& g, double tau,
               const lasso_gpsr_options& o, lasso_gpsr_result* res, void* workspace, hipStream_t st) {
  const ConvSpace ws = carve(workspace, g);
  const int cus = solver::device_cus();
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz;
  const int ckk = g.C * g.kh * g.kw, ldr = (ckk + 3) / 4 * 4;
  // (the GEMM's epilogue addresses a 64-row block with 32-bit offsets: COLSt has pitch M)
  if (std::max<int64_t>({M, (int64_t)g.K, (int64_t)ldr}) * 64 * 4 >= ((int64_t)1 << 31))
    return fail(LASSO_ERR_UNSUPPORTED, "convolutional GPSR: %lld code pixels are beyond the 32-bit offsets of a 64-row block",
                (long long)M);
  ConvOp op;
  op.rows = (int)M; op.cols = g.K; op.nd = (int64_t)g.N * g.C * g.H * g.W;
  // LASSO_FORCE_BLOCKS_128 (tests): 128 x 128 blocks below the size at which block_side takes them
  const bool force128 = (o.reserved & LASSO_FORCE_BLOCKS_128) &&
                        std::max<int64_t>({M, (int64_t)g.K, (int64_t)ldr}) * 128 * 4 < ((int64_t)1 << 31);
  op.side_k = force128 ? 128 : block_side((int)M, g.K, std::max<int64_t>(ldr, g.K), cus);          // products [M,K]
  op.side_c = force128 ? 128 : block_side(ckk, (int)M, std::max<int64_t>(M, g.K), cus);            // COLSt [C kh kw, M]
  op.pk_gemm = gemm_parts((int)M, g.K, op.side_k);
  op.pk_cap = gemm_parts((int)M, g.K, 64);
  op.cus = cus;
  int count = 0;
  op.implicit = !(o.reserved & 1) && implicit_covered(g, cus, op.pk_cap, &count);
  op.pk = op.implicit ? std::max(op.pk_gemm, count) : op.pk_gemm;
  op.pd = ew_grid(op.nd);
  op.y = x; op.ldy = (int64_t)g.C * g.H * g.W; op.y_rows = g.N; op.y_cols = g.C * g.H * g.W;
  op.start = z0 ? ws.Z0m : nullptr; op.ld_start = g.K;
  op.g = g; op.w = w; op.z0 = z0;
  op.Wt = ws.Wt; op.Wp = ws.Wp; op.RC = ws.RC; op.COLSt = ws.COLSt; op.Z0m = ws.Z0m; op.IMG = ws.IMG; op.zout = zout;
  op.ckk = ckk; op.ldr = ldr;
  return solve_with(op, ws.common, tau, o, res, st);
}

}  // namespace gpsr
}  // namespace lasso
