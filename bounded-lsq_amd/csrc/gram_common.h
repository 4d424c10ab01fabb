// Shared by gram_kernels.hip (the Gram kernels), chol_reg.hip (N <= 80: Cholesky and fused Newton rounds),
// chol_rl.hip (N > 80: Cholesky) and cert_kernels.hip (certificate): launch geometry, the
// explicit LDS read helpers with counted waits and the column scales of the Cholesky kernels.
#pragma once
#include <stdlib.h>
#include <type_traits>

#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"

namespace blsq {

static constexpr int GR_NT = 512;
static constexpr int GR_NW = GR_NT / WAVE;
static constexpr int GR_RC = 32;          // rows per staged chunk (8 MFMA k-steps)
static constexpr int REG_NW = 4;          // one-wave-per-problem kernels (N <= 80): problems (waves) per workgroup —
static constexpr int REG_NT = REG_NW * WAVE;   // 1024 problems spread over 256 workgroups instead of 128
// Problem of wave `wv` of workgroup `w` in the one-wave-per-problem kernels.  Workgroups are dealt round-robin over
// the eight XCDs and the Gram kernel that has just written the problem's matrix ran as workgroup b (one per problem):
// b and the workgroup that reads it back agree mod 8, so the read finds the matrix in the L2 it was written through.
__device__ __forceinline__ int reg_problem(int w, int wv) { return (((w >> 3) * REG_NW + wv) << 3) | (w & 7); }
static inline unsigned reg_grid(int B) { return (unsigned)(((B + 8 * REG_NW - 1) / (8 * REG_NW)) * 8); }
static constexpr double GRAM_SMIN = GRAM_SMIN_PROVEN;   // early reject: a pivot of R' below what the certificate could accept

// An explicit 8-byte LDS read (byte address: lds_addr, blsq_device.h) whose completion the CALLER waits for
// (counted s_waitcnt lgkmcnt)
__device__ __forceinline__ void lds_read64(double& dst, unsigned byte_addr) {
  asm volatile("ds_read_b64 %0, %1" : "=v"(dst) : "v"(byte_addr));
}

__host__ __device__ inline int gram_ldx(int NT) { return NT * 16 + ((NT & 1) ? 0 : 16); }

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
template <int OFF>
__device__ __forceinline__ void lds_read64_off(double& dst, unsigned byte_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field is 16 bits");
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(byte_addr), "n"(OFF));
}

// Column j of the equilibration of H = D G D + diag(e^2) (+ alpha I) on the first n of its N = n + 1 columns, from the
// source Gram's diagonal entry of index sj = src(j) (j < N), into the LDS vectors of the factor kernels:
//   dl_j = 1 / sqrt(h_jj) (v_rsq and two Newton steps),  sq_j = sqrt(h_jj),  sc_j = colscale_j dl_j (the scale of the
//   source entries),  td_j = (e_j^2 + alpha) dl_j^2 - tau (added to the diagonal of C; tau: the shift of certificate
//   stage 3, on the first n columns).
// bad = 1 if h_jj of a variable (j < n) is not positive and finite.  Returns dl_j; sj the source index.
template <class Src>
__device__ __forceinline__ double col_scale(const double* Gs, int NPAD, int j, int n, Src&& src, const double* csv,
                                            const double* edv, double sa, double tau, double* dl, double* sq,
                                            double* sc, double* td, int& bad, int& sj) {
  const int N = n + 1;
  const double cs = (csv && j < n) ? csv[j] : 1.0;
  const double ej = (edv && j < n) ? edv[j] : 0.0;
  const double add = (j < n) ? fma(ej, ej, sa * sa) : 0.0;
  sj = (j < N) ? src(j) : j;
  const double g = (j < N) ? fma(Gs[(long)sj * NPAD + sj] * cs, cs, add) : 0.0;
  const bool okc = (g > 0.0) && is_finite(g);
  if (j < n && !okc) bad = 1;
  double d = 1.0, s = 1.0;
  if (j < N && okc) {
    d = __builtin_amdgcn_rsq(g);
    d = d * fma(-0.5 * g * d, d, 1.5);
    d = d * fma(-0.5 * g * d, d, 1.5);
    s = g * d;
  }
  dl[j] = d; sq[j] = s; sc[j] = cs * d; td[j] = add * d * d - ((j < n) ? tau : 0.0);
  return d;
}

// Diagnostic build only (-DBLSQ_CHOL_STAMPS): wall-clock stamps (100 MHz) of the phases of the Cholesky and certificate
// kernels, taken by lane 0 of chosen waves of ONE problem.  chol_reg.hip, chol_rl.hip and cert_kernels.hip each keep
// their own g_chol_st[4][20][8]; chol_debug_stamps (chol_rl.hip) puts the copies together.  Never enabled in the product.
#ifdef BLSQ_CHOL_STAMPS
#define CST(cond, p, kb, i) do { if ((cond) && lane == 0) g_chol_st[p][kb][i] = (long long)wall_clock64(); } while (0)
#else
#define CST(cond, p, kb, i) do { } while (0)
#endif

}  // namespace blsq
