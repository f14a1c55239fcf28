// Weight gradient of the unrolled convolutional ISTA/FISTA solve (SURVEY.md 8f rows f3 + f4: the
// reference's ista_conv2d, lasso/conv2d/ista.py:7-49, is plain torch code that torch.autograd
// differentiates with respect to x, weight and z0).
//
// Reverse pass of iteration i (codes held as matrices [M = N Hz Wz][K], P(img) = the
// patch matrix [M][C kh kw] of an NCHW image under the conv's stride and padding):
//     ub = [z_{i+1} != 0] zb_{i+1} ;  gb = -lr ub ;  rb = conv_transpose2d(gb, W)
//     yb_i = ub + conv2d(rb, W) ;  xb -= rb
//     dW[k][(c,a,b)] += sum_m ( gb[m][k] P(r_i)[m][(c,a,b)] + y_i[m][k] P(rb)[m][(c,a,b)] )
// The dW line is ONE reduction over 2M rows -- the pairs (gb, P(r_i)) followed by (y_i, P(rb)) -- and
// this file runs it as an implicit GEMM on v_mfma_f32_16x16x4_f32: the patches are gathered from the
// NCHW images straight into LDS (no M x C kh kw patch matrix in HBM), the code rows are staged beside
// them, both terms accumulate in the same registers.  M is split over the whole chip; each split keeps
// its partial tile in a slot of its own and adds every iteration of the reverse pass into it (a plain
// read-modify-write: no atomics), and one small kernel sums the slots in split order at the end --
// bitwise reproducible from run to run.  The rest of the reverse pass is the forward's own kernels
// (conv.hip / conv_synth*.hip) and autograd.hip's elementwise glue; lasso_hip.hip drives it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "lasso_kernels.h"

namespace lasso {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgT = 64;              // output tile: 64 atoms x 64 taps, four 16 x 16 MFMA blocks each way
constexpr int kWgRows = 64;           // code pixels (rows of the reduction) staged per step
constexpr int kWgLd = kWgT + 16;      // LDS row pitch: the rows 4 s + q of one MFMA operand read fall on disjoint banks
constexpr int kWgOcc = 4;             // workgroups per CU: 128 registers, 4 x 40 KiB of LDS (gfx950: 160 KiB)

struct ConvWgrad {
  const float* A0; const float* A1;   // [M][K]: gb, y_i
  const float* I0; const float* I1;   // [N][C][H][W]: r_i, rb
  float* part;                        // [splits][K][C kh kw]
  ConvGeom g;
  int64_t M;
  int ckk, tiles_t, nch, splits, accumulate;
};

// Workgroup = 4 waves = one 64 x 64 tile of dW over a contiguous range of 64-row chunks of the 2M rows.  A chunk is
// staged as As [64 rows][64 atoms] and Bs [64 rows][64 taps]; wave w multiplies the MFMA steps (4 rows each)
// w, w + 4, w + 8, w + 12 of it into its own 4 x 4 blocks, and the four waves' sums meet in LDS in wave order at the
// end.  The global loads of the next chunk are issued before the MFMAs of the current one.
__global__ __launch_bounds__(256, kWgOcc) void conv_wgrad_kernel(const ConvWgrad p) {
  __shared__ __attribute__((aligned(16))) float sm[2 * kWgRows * kWgLd];
  float* const As = sm;
  float* const Bs = sm + kWgRows * kWgLd;
  const ConvGeom& g = p.g;
  // (w through readfirstlane: the compiler then knows the rows of a wave -- and their decode in fetch below -- to be
  // wave-uniform and keeps that arithmetic on the scalar unit; per lane it was ten times the MFMA phase's instructions)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15,
            q = lane >> 4;
  const int K = g.K, ckk = p.ckk, P = g.Hz * g.Wz;
  const int k0 = kWgT * (int)(blockIdx.y / p.tiles_t), t0 = kWgT * (int)(blockIdx.y % p.tiles_t);
  // this thread stages column `lane` (atom k0 + lane of A, tap t0 + lane of B) of the rows 16 w .. 16 w + 15
  const int ka = k0 + lane, t = t0 + lane, row0 = 16 * w;
  const bool kok = ka < K, tok = t < ckk;
  int ta = 0, tb = 0, toff = 0;
  if (tok) {
    tb = t % g.kw;
    ta = (t / g.kw) % g.kh;
    toff = ((t / (g.kw * g.kh)) * g.H + ta) * g.W + tb;
  }
  const int chw = g.C * g.H * g.W, M = (int)p.M;      // (32-bit: conv_wgrad_splits keeps the operands below 2 GiB)
  const int total = 2 * p.nch;
  const int c_begin = (int)((int64_t)blockIdx.x * total / p.splits);
  const int c_end = (int)((int64_t)(blockIdx.x + 1) * total / p.splits);
  const unsigned abytes = (unsigned)(M * K * 4), ibytes = (unsigned)(g.N * chw * 4);
  float av[16], bv[16];
  // Loads through buffer descriptors of the whole operand: the offset of a zero (outside the image, beyond M / K /
  // C kh kw) is out of range and reads 0, so every lane issues all 32 loads and nothing sits under a branch
  auto fetch = [&](int ch) {
    const int term = ch >= p.nch ? 1 : 0;
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(term ? p.A1 : p.A0), 0,
                                                                         (int)abytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(term ? p.I1 : p.I0), 0,
                                                                         (int)ibytes, 0x00020000);
    const int m0 = (ch - term * p.nch) * kWgRows + row0;
    int n = m0 / P;
    const int rem = m0 - n * P;
    int u = rem / g.Wz, v = rem - (rem / g.Wz) * g.Wz;
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      const int m = m0 + h;
      const bool mok = m < M;
      unsigned oa = (mok && kok) ? (unsigned)(m * K + ka) * 4u : 0xfffffff0u;
      const int i0 = u * g.sh - g.ph, j0 = v * g.sw - g.pw;
      const bool bok = mok && tok && (unsigned)(i0 + ta) < (unsigned)g.H && (unsigned)(j0 + tb) < (unsigned)g.W;
      unsigned ob = bok ? (unsigned)(n * chw + i0 * g.W + j0 + toff) * 4u : 0xfffffff0u;
      asm volatile("" : "+v"(oa), "+v"(ob));
      av[h] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ars, oa, 0, 0));
      bv[h] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(irs, ob, 0, 0));
      if (++v == g.Wz) { v = 0; if (++u == g.Hz) { u = 0; ++n; } }
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      As[(row0 + h) * kWgLd + lane] = av[h];
      Bs[(row0 + h) * kWgLd + lane] = bv[h];
    }
  };
  f32x4 acc[4][4] = {};
  bool mt_ok[4], nt_ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mt_ok[j] = k0 + 16 * j < K;
    nt_ok[j] = t0 + 16 * j < ckk;
  }
  if (c_begin < c_end) fetch(c_begin);
  for (int ch = c_begin; ch < c_end; ++ch) {
    put();
    __syncthreads();
    if (ch + 1 < c_end) fetch(ch + 1);           // the next chunk's loads run under this chunk's MFMAs
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      const int r = 4 * (w + 4 * ss) + q;
      float a[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = As[r * kWgLd + 16 * j + l15];
        b[j] = Bs[r * kWgLd + 16 * j + l15];
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          if (mt_ok[mt] && nt_ok[nt])            // (uniform: tiles at the edge of K / C kh kw)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    __syncthreads();
  }
  // the four waves' sums meet in LDS in wave order (acc[mt][nt][rg] = dW[k0 + 16 mt + 4 q + rg][t0 + 16 nt + l15])
  float* const red = sm;
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int e = (16 * mt + 4 * q + rg) * kWgT + 16 * nt + l15;
            red[e] = ww == 0 ? acc[mt][nt][rg] : red[e] + acc[mt][nt][rg];
          }
    }
    __syncthreads();
  }
  float* const part = p.part + (int64_t)blockIdx.x * K * ckk;
  for (int e = tid; e < kWgT * kWgT; e += 256) {
    const int k = k0 + e / kWgT, tt = t0 + e % kWgT;
    if (k < K && tt < ckk) {
      float* const o = part + (int64_t)k * ckk + tt;
      *o = p.accumulate ? *o + red[e] : red[e];
    }
  }
}

// gw[e] = sum over the splits, in split order, of part[s][e]
__global__ __launch_bounds__(256) void conv_wgrad_sum_kernel(const float* __restrict__ part, int splits, int64_t words,
                                                             float* __restrict__ gw) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < words; e += (int64_t)gridDim.x * 256) {
    float s = 0.0f;
    for (int sp = 0; sp < splits; ++sp) s += part[sp * words + e];
    gw[e] = s;
  }
}

}  // namespace

// Splits of the 2M rows (one per workgroup column of the grid): one round of kWgOcc workgroups per CU over all tiles.
// 0: the geometry is not covered (32-bit offsets inside an image, grid limits) -- the caller takes conv_patches +
// gram_tn.
int conv_wgrad_splits(const ConvGeom& g, int cus) {
  const int64_t M = (int64_t)g.N * g.Hz * g.Wz, ckk = (int64_t)g.C * g.kh * g.kw;
  const int64_t tiles = ((g.K + kWgT - 1) / kWgT) * ((ckk + kWgT - 1) / kWgT);
  // (32-bit buffer offsets: the codes and the images below 2 GiB)
  if (M <= 0 || tiles > 65535 || M * g.K * 4 >= INT32_MAX || (int64_t)g.N * g.C * g.H * g.W * 4 >= INT32_MAX) return 0;
  const int64_t nch = (M + kWgRows - 1) / kWgRows;
  const int64_t s = (kWgOcc * (int64_t)std::max(cus, 1) + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>({s, 2 * nch, 1024}));
}

// part [splits][K][C kh kw] (+)= the splits' sums of gb^T P(r) + y^T P(rb); accumulate = 0 on the first iteration
hipError_t launch_conv_wgrad(const float* gb, const float* r, const float* y, const float* rb, float* part, int splits,
                             int accumulate, const ConvGeom& g, hipStream_t stream) {
  ConvWgrad p;
  p.A0 = gb; p.A1 = y; p.I0 = r; p.I1 = rb; p.part = part; p.g = g;
  p.M = (int64_t)g.N * g.Hz * g.Wz;
  p.ckk = g.C * g.kh * g.kw;
  p.tiles_t = (p.ckk + kWgT - 1) / kWgT;
  p.nch = (int)((p.M + kWgRows - 1) / kWgRows);
  p.splits = splits;
  p.accumulate = accumulate;
  const int tiles = ((g.K + kWgT - 1) / kWgT) * p.tiles_t;
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(splits, tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_conv_wgrad_sum(const float* part, int splits, const ConvGeom& g, float* gw, hipStream_t stream) {
  const int64_t words = (int64_t)g.K * g.C * g.kh * g.kw;
  hipLaunchKernelGGL(conv_wgrad_sum_kernel, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 4096)), dim3(256), 0,
                     stream, part, splits, words, gw);
  return hipGetLastError();
}

}  // namespace lasso
