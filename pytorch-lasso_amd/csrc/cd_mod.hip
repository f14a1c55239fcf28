// Cyclic coordinate descent with a duality-gap stop (reference
// lasso/linear/solvers/coordinate_descent.py:57-139, `coord_descent_mod`, after sklearn's
// enet_coordinate_descent).
//
// Per sample row the reference sweeps the atoms in order (:110-129): put the coordinate's share back into the
// residual R, z_i <- S_alpha(R . w_i) / ||w_i||^2, take the new share out again.  After a sweep the row is checked
// (:132) when nothing is left, when the largest change is below tol relative to the largest coordinate, or on the last
// sweep; a checked row gets its duality gap (:87-99) and is frozen once gap < tol * ||x||^2.  Rows never interact.
//
// Kernel: ONE WAVE PER ROW, ONE LAUNCH FOR THE WHOLE SOLVE, the row's state in VGPRs as in cd.hip (K/64 floats per lane
// and quantity, lane l owns columns 256c + 4l .. +3).  The state is the COVARIANCE form: z and q = W^T x - G z with
// G = W^T W, so that R . w_i + ||w_i||^2 z_i = q_i + G_ii z_i needs no d-long reduction and a change of coordinate i is
// q -= change * G[i, :], one coalesced row of G from L2 (G is bitwise symmetric: row i is column i).
//
// A coordinate whose new value equals its old one bit for bit leaves q untouched; for a zero coordinate that is
// |q_i| <= alpha.  So a sweep does not visit the atoms one by one: all K coordinates are tested at once (zero-norm atoms
// and the padding are masked out for the whole solve), the wave jumps to the first coordinate >= the cursor that is
// nonzero or would become nonzero, updates it, and tests again from there.  That is the sequential sweep in this form
// bit for bit, at one dependent step per coordinate that can change instead of one per atom.  A sweep that changed
// nothing leaves a state that no later sweep changes (but for the rounding of a rebuild of q, below): the row is then
// finished at once with the outcome the remaining sweeps would have had.
//
// q is rebuilt from b0, G and the current z every 4 sweeps (see rebuild_q): the running update alone drifts.
//
// The gap comes from resident data plus b0 = W^T x and ||x||^2: XtA = q, R . x = ||x||^2 - z . b0,
// ||R||^2 = ||x||^2 - z . b0 - z . q; the dot products, ||x||^2 and the gap's own arithmetic are double.
//
// No LDS, no barriers, no atomics: two calls give the same bits.  Bound by the dependent chain per updated coordinate
// (test -> wave minimum -> row of G from L2 -> K fused multiply-adds).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "lasso_kernels.h"
#include "static_for.hpp"

namespace lasso {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int N> using fvec = float __attribute__((ext_vector_type(N)));

constexpr unsigned kNone = 0x7fffffffu;
constexpr int kRefresh = 4;      // sweeps between two rebuilds of q from b0, G and z

__device__ __forceinline__ float shrink(float v, float lam) {
  return v - __builtin_amdgcn_fmed3f(v, -lam, lam);    // == softshrink bit for bit (lam >= 0)
}

// wave max / min of unsigned keys (as in cd.hip): DPP row_shr 1,2,4,8 leaves each 16-lane row's result in its last
// lane; the four row results are folded on the scalar unit.  Result is wave-uniform.
__device__ __forceinline__ unsigned wave_max_u32(unsigned x) {
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true));
  const unsigned r0 = __builtin_amdgcn_readlane((int)x, 15), r1 = __builtin_amdgcn_readlane((int)x, 31);
  const unsigned r2 = __builtin_amdgcn_readlane((int)x, 47), r3 = __builtin_amdgcn_readlane((int)x, 63);
  return max(max(r0, r1), max(r2, r3));
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned x) {
  constexpr int kBig = (int)kNone;
  x = min(x, (unsigned)__builtin_amdgcn_update_dpp(kBig, (int)x, 0x111, 0xf, 0xf, false));
  x = min(x, (unsigned)__builtin_amdgcn_update_dpp(kBig, (int)x, 0x112, 0xf, 0xf, false));
  x = min(x, (unsigned)__builtin_amdgcn_update_dpp(kBig, (int)x, 0x114, 0xf, 0xf, false));
  x = min(x, (unsigned)__builtin_amdgcn_update_dpp(kBig, (int)x, 0x118, 0xf, 0xf, false));
  const unsigned r0 = __builtin_amdgcn_readlane((int)x, 15), r1 = __builtin_amdgcn_readlane((int)x, 31);
  const unsigned r2 = __builtin_amdgcn_readlane((int)x, 47), r3 = __builtin_amdgcn_readlane((int)x, 63);
  return min(min(r0, r1), min(r2, r3));
}
// wave sum of doubles in a fixed order (butterfly); only at the start of a row and per gap evaluation
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int NC>
__global__ __launch_bounds__(256) void cd_mod_rows_kernel(const CdModParams p) {
  constexpr int KP = 256 * NC;
  constexpr int H = NC > 8 ? NC / 8 : 1;       // register tuples per quantity
  constexpr int HN = 4 * NC / H;               // floats per tuple (<= 32)
  typedef fvec<HN> vec;
  const int lane = threadIdx.x & 63;
  const float alpha = p.alpha, tol = p.tol;
  // rows are dealt out statically, wave w takes rows w, w + #waves, ...: every branch in this kernel is wave-uniform
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nwaves = (int)gridDim.x * 4;

  // bit I of `live`: the lane's element I is an atom (column < k) of nonzero norm (:111); everything else never moves
  unsigned long long live = 0;
  static_for<4 * NC>([&](auto i) {
    constexpr int I = decltype(i)::value;
    const int col = 256 * (I / 4) + (I % 4) + 4 * lane;
    if (col < p.k && p.G[(int64_t)col * KP + col] != 0.0f) live |= 1ull << I;
  });

  // element `slot` of a quantity in lane `owner`, wave-uniform
  auto pick = [&](const vec (&v)[H], int slot, int owner) -> float {
    float t;
    if constexpr (H == 1) t = v[0][slot];
    else t = slot < HN ? v[0][slot] : v[1][slot - HN];
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), owner));
  };

  for (int row = wave; row < p.n; row += nwaves) {
    // ||x||^2 in double (:81); the reference's threshold is tol * that, in float
    double xx = 0.0;
    const float* const xr = p.x + (int64_t)row * p.ldx;
    for (int c = lane; c < p.d; c += 64) { const double v = (double)xr[c]; xx += v * v; }
    xx = wave_sum_f64(xx);
    const float tol_row = tol * (float)xx;

    const float* const bp = p.B0 + (int64_t)row * KP + 4 * lane;
    float* const zrow = p.z + (int64_t)row * p.ldz;
    vec q[H], z[H];
    // a zero-norm atom is never visited (:111): its start value stays in the caller's memory, out of the register
    // state (its q is an exact zero for the whole solve), and only its share of ||z||_1 is carried along
    double l1_dead = 0.0;
    static_for<NC>([&](auto c) {
      constexpr int C = decltype(c)::value;
      const f32x4 tb = *(const f32x4*)(bp + 256 * C);
      static_for<4>([&](auto e_) {
        constexpr int E = decltype(e_)::value;
        constexpr int I = 4 * C + E;
        const int col = 256 * C + 4 * lane + E;
        q[I / HN][I % HN] = tb[E];
        float zi = (p.has_start && col < p.k) ? zrow[col] : 0.0f;               // the pitch is the caller's: by element
        if (!((live >> I) & 1)) { l1_dead += (double)__builtin_fabsf(zi); zi = 0.0f; }
        z[I / HN][I % HN] = zi;
      });
    });

    // the smallest column >= cursor among the lane elements flagged in `want`, or kNone
    auto first_from = [&](unsigned cursor, auto want) -> unsigned {
      unsigned best = kNone;
      static_for<4 * NC>([&](auto i) {
        constexpr int I = decltype(i)::value;
        const unsigned col = 256 * (I / 4) + (I % 4) + 4 * lane;
        if (want(i) && col >= cursor) best = min(best, col);
      });
      return wave_min_u32(best);
    };
    // q -= c * G[j, :]
    auto take_out = [&](unsigned j, float c) {
      const float* const gp = p.G + (int64_t)j * KP + 4 * lane;
      f32x4 s[NC];
      static_for<NC>([&](auto cc) { s[cc] = *(const f32x4*)(gp + 256 * cc); });
      static_for<4 * NC>([&](auto i) {
        constexpr int I = decltype(i)::value;
        q[I / HN][I % HN] = __builtin_fmaf(-c, s[I / 4][I % 4], q[I / HN][I % HN]);
      });
    };

    // q = b0 - G z from scratch: one row of G per nonzero coordinate, in coordinate order.  At the start (:102), and
    // again every kRefresh sweeps: q -= change * G[i, :] rounds once per update, and over some tens of sweeps that
    // drift moved z by 9-12 x the float32-float64 spread of the reference's own residual form (measured);
    // rebuilt every 4 sweeps it measures 0.7-3.3 x.  The rows are independent loads, not the sweep's dependent chain.
    auto rebuild_q = [&](bool reload) {
      if (reload)
        static_for<NC>([&](auto c) {
          constexpr int C = decltype(c)::value;
          const f32x4 tb = *(const f32x4*)(bp + 256 * C);
          static_for<4>([&](auto e_) {
            constexpr int I = 4 * C + decltype(e_)::value;
            q[I / HN][I % HN] = tb[decltype(e_)::value];
          });
        });
      unsigned cursor = 0;
      for (;;) {
        const unsigned j = first_from(cursor, [&](auto i) {
          constexpr int I = decltype(i)::value;
          return z[I / HN][I % HN] != 0.0f;
        });
        if (j == kNone) break;
        const int owner = (j & 255) >> 2, slot = ((j >> 8) << 2) | (j & 3);
        take_out(j, pick(z, slot, owner));
        cursor = j + 1;
      }
    };
    if (p.has_start) rebuild_q(false);

    int sweeps = 0, conv = 0;
    float gap = p.gap0;
    unsigned long long commits = 0;
    while (sweeps < p.max_iter) {
      if (sweeps > 0 && sweeps % kRefresh == 0) rebuild_q(true);
      float dzmax = 0.0f;
      bool moved = false;
      unsigned cursor = 0;
      for (;;) {
        // :116-125 leave every coordinate with z_i == 0 and |q_i| <= alpha as it is: the jump to the next other one
        const unsigned j = first_from(cursor, [&](auto i) {
          constexpr int I = decltype(i)::value;
          const float zi = z[I / HN][I % HN], qi = q[I / HN][I % HN];
          return zi != 0.0f || !(__builtin_fabsf(qi) <= alpha);      // (a NaN q is visited: S(NaN) is NaN, :118-121)
        });
        if (j == kNone) break;
        const int owner = (j & 255) >> 2, slot = ((j >> 8) << 2) | (j & 3);
        const float qj = pick(q, slot, owner), zj = pick(z, slot, owner);
        const float gjj = p.G[(int64_t)j * KP + j];                           // :84 ||w_j||^2
        const float zn = shrink(__builtin_fmaf(gjj, zj, qj), alpha) / gjj;   // :118-121
        const float dz = zn - zj;
        dzmax = __builtin_fmaxf(dzmax, __builtin_fabsf(dz));                  // :128
        if (dz != 0.0f) {
          if constexpr (H == 1) {                                             // (owner lane only)
            z[0][slot] = lane == owner ? zn : z[0][slot];
          } else {
            if (slot < HN) z[0][slot] = lane == owner ? zn : z[0][slot];
            else z[1][slot - HN] = lane == owner ? zn : z[1][slot - HN];
          }
          take_out(j, dz);                                                    // :118,125
          ++commits;
          moved = true;
        }
        cursor = j + 1;
      }
      ++sweeps;
      // :129  largest coordinate over the atoms the sweep visits
      float zm = 0.0f;
      static_for<4 * NC>([&](auto i) {
        constexpr int I = decltype(i)::value;
        zm = __builtin_fmaxf(zm, __builtin_fabsf(z[I / HN][I % HN]));
      });
      const float zmax = __uint_as_float(wave_max_u32(__float_as_uint(zm)));
      const bool check = zmax == 0.0f || dzmax / zmax < tol || sweeps == p.max_iter;   // :132
      if (check || !moved) {
        // :87-99 with XtA = q
        float qm = 0.0f;
        double l1 = l1_dead, zb = 0.0, zq = 0.0;
        static_for<NC>([&](auto c) {
          constexpr int C = decltype(c)::value;
          const f32x4 tb = *(const f32x4*)(bp + 256 * C);
          static_for<4>([&](auto e_) {
            constexpr int E = decltype(e_)::value;
            constexpr int I = 4 * C + E;
            const float zi = z[I / HN][I % HN], qi = q[I / HN][I % HN];
            qm = __builtin_fmaxf(qm, __builtin_fabsf(qi));
            l1 += (double)__builtin_fabsf(zi);
            zb += (double)zi * (double)tb[E];
            zq += (double)zi * (double)qi;
          });
        });
        const float dual = __uint_as_float(wave_max_u32(__float_as_uint(qm)));
        l1 = wave_sum_f64(l1); zb = wave_sum_f64(zb); zq = wave_sum_f64(zq);
        const double rx = xx - zb, rn2 = rx - zq;
        const bool small = dual <= alpha;
        const double cst = small ? 1.0 : (double)(alpha / dual);
        const double g = (small ? rn2 : 0.5 * rn2 * (1.0 + cst * cst)) + (double)alpha * l1 - cst * rx;
        gap = (float)g;
        conv = gap < tol_row;                                                  // :97
        if (check && conv) break;
        // nothing moved: every further sweep repeats this one, and the last one is always checked
        if (!moved) { sweeps = p.max_iter; break; }
      }
    }

    static_for<4 * NC>([&](auto i) {
      constexpr int I = decltype(i)::value;
      const int col = 256 * (I / 4) + (I % 4) + 4 * lane;
      if (col < p.k && (((live >> I) & 1) || !p.has_start)) zrow[col] = z[I / HN][I % HN];
    });
    // every lane writes the same values to the same words: no divergent tail
    p.gap[row] = gap;
    if (p.sweeps_out) p.sweeps_out[row] = sweeps;
    if (p.conv_out) p.conv_out[row] = (unsigned char)conv;
    p.row_sweeps[row] = sweeps;
    p.row_conv[row] = conv;
    p.row_commits[row] = commits;
  }
}

__global__ __launch_bounds__(256) void cd_mod_info_kernel(const int* __restrict__ row_conv,
                                                          const unsigned long long* __restrict__ row_commits, int n,
                                                          long long* __restrict__ info) {
  __shared__ long long su[256], sc[256];
  long long u = 0, c = 0;
  for (int i = threadIdx.x; i < n; i += 256) { u += row_conv[i] ? 0 : 1; c += (long long)row_commits[i]; }
  su[threadIdx.x] = u; sc[threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { su[threadIdx.x] += su[threadIdx.x + s]; sc[threadIdx.x] += sc[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { info[0] = su[0]; info[1] = sc[0]; }
}

}  // namespace

hipError_t launch_cd_mod_rows(const CdModParams& p, int kp, int cus, hipStream_t stream) {
  if (p.n <= 0) return hipSuccess;
  // 4 rows (waves) per workgroup; enough workgroups to fill every SIMD at the kernel's occupancy
  const int wgs = std::max(1, std::min((p.n + 3) / 4, cus * 8));
  switch (kp) {
    case 256: hipLaunchKernelGGL(cd_mod_rows_kernel<1>, dim3(wgs), dim3(256), 0, stream, p); break;
    case 512: hipLaunchKernelGGL(cd_mod_rows_kernel<2>, dim3(wgs), dim3(256), 0, stream, p); break;
    case 1024: hipLaunchKernelGGL(cd_mod_rows_kernel<4>, dim3(wgs), dim3(256), 0, stream, p); break;
    case 2048: hipLaunchKernelGGL(cd_mod_rows_kernel<8>, dim3(wgs), dim3(256), 0, stream, p); break;
    case 4096: hipLaunchKernelGGL(cd_mod_rows_kernel<16>, dim3(wgs), dim3(256), 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_cd_mod_info(const int* row_conv, const unsigned long long* row_commits, int n, long long* info,
                              hipStream_t stream) {
  hipLaunchKernelGGL(cd_mod_info_kernel, dim3(1), dim3(256), 0, stream, row_conv, row_commits, n, info);
  return hipGetLastError();
}

}  // namespace lasso
