// Matrix-vector products of ONE workgroup of NT threads with an n x n matrix in global memory (row-major, stride ld):
// one wave per row, lanes stride the columns, RB rows per wave pass.  Vectors live in LDS (or global memory).
// Used by the n-space step kernels (trf_kernels.hip, dogbox_kernels.hip: compiled with -ffp-contract=off) and by the
// SVD-free path (lm_kernels.hip, lm_body.h: contracting), so the file follows the contraction rule of blsq_device.h:
// every multiply-add below is an fma() call.
//
// Per row the chain is  acc = fma(m_ij, s_j, acc)  over j = j0 + lane + 64 k, k ascending, from acc = 0, and the 64
// lane sums go through the tree of wave_sum (wave_sum16 is that tree for sixteen values at once): a row's bits depend
// on neither NT nor RB.  R does not fit any cache for a whole batch, so the RB loads of a pass are unconditional
// (clamped) and in flight together — a row at a time pays a full memory round trip per row.
#pragma once
#include "blsq_device.h"

namespace blsq {

// u = R diag(dvec) s  (R upper triangular; dvec == nullptr: u = R s).  (R[i][j] * d[j]) * s[j]: the roundings of a
// materialised R D.  RB == 8: the eight row totals by one transposed butterfly; any other RB: wave_sum per row.
template <int NT, int RB>
__device__ void tri_matvec(const double* R, const double* dvec, int n, int ld, const double* svec, double* u) {
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i0 = w; i0 < n; i0 += NW * RB) {
    double acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0;
    for (int jj = 0; i0 + jj < n; jj += WAVE) {             // (wave-uniform: the longest row, i0)
      double rv[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        const int ic = (i < n) ? i : n - 1;
        const int j = ic + lane + jj;
        rv[r] = R[(long)ic * ld + ((j < n) ? j : n - 1)];
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        const int j = i + lane + jj;
        if (i < n && j < n) acc[r] = fma(dvec ? rv[r] * dvec[j] : rv[r], svec[j], acc[r]);
      }
    }
    if constexpr (RB == 8) {
      double v[16];
#pragma unroll
      for (int r = 0; r < RB; ++r) { v[r] = acc[r]; v[8 + r] = 0.0; }
      wave_sum16(v);
      const int idx = wave_sum16_index(lane), ri = i0 + (idx & 7) * NW;
      if (lane < 16 && idx < 8 && ri < n) u[ri] = v[0];
    } else {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        const double t = wave_sum(acc[r]);
        if (lane == 0 && i < n) u[i] = t;
      }
    }
  }
  __syncthreads();
}

// u = M s for a DENSE n x n block: the Jacobi rows s_i v_i^T of a problem whose factor went through the SVD
template <int NT, int RB>
__device__ void full_matvec(const double* M, int n, int ld, const double* svec, double* u) {
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i0 = w; i0 < n; i0 += NW * RB) {
    double acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0;
    for (int jj = lane; jj < n; jj += WAVE) {
      double rv[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        rv[r] = M[(long)((i < n) ? i : n - 1) * ld + jj];
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) acc[r] = fma(rv[r], svec[jj], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int i = i0 + r * NW;
      const double t = wave_sum(acc[r]);
      if (lane == 0 && i < n) u[i] = t;
    }
  }
  __syncthreads();
}

// Three products with ONE pass over the matrix (the reflective branch of the TRF step needs J_h p_h, J_h r_h and
// J_h (-g_h); the matrix — half a megabyte per problem at n = 256 — does not stay in any cache between separate
// passes):  u1 = M s1,  u2 = M s2 (s2 == nullptr: skipped),  u3 = M (-g3).
// Per row and product exactly the operations of tri_matvec<NT, 8> / full_matvec<NT, 4>, in the same order.
template <int NT>
__device__ void tri_matvec3(const double* R, const double* dvec, int n, int ld, const double* s1,
                            double* u1, const double* s2, double* u2, const double* g3, double* u3) {
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int RB = 8;
  for (int i0 = w; i0 < n; i0 += NW * RB) {
    double a1[RB], a2[RB], a3[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) { a1[r] = 0.0; a2[r] = 0.0; a3[r] = 0.0; }
    for (int jj = 0; i0 + jj < n; jj += WAVE) {             // (wave-uniform: the longest row, i0)
      double rv[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        const int ic = (i < n) ? i : n - 1;
        const int j = ic + lane + jj;
        rv[r] = R[(long)ic * ld + ((j < n) ? j : n - 1)];
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        const int j = i + lane + jj;
        if (i < n && j < n) {
          const double rd = dvec ? rv[r] * dvec[j] : rv[r];
          a1[r] = fma(rd, s1[j], a1[r]);
          if (s2) a2[r] = fma(rd, s2[j], a2[r]);
          a3[r] = fma(rd, -g3[j], a3[r]);
        }
      }
    }
    // The 24 row totals by two transposed butterflies (wave_sum16: the same tree as wave_sum for every one of them — xor 1,
    // 2, 4, 8 inside the 16-lane rows, then (r0 + r16) + (r32 + r48) — in 15 exchanges per sixteen totals instead of 64).
    static_assert(RB == 8, "two sixteen-value reductions");
    double v[16];
    const int idx = wave_sum16_index(lane), ri = i0 + (idx & 7) * NW;
#pragma unroll
    for (int r = 0; r < RB; ++r) { v[r] = a1[r]; v[8 + r] = s2 ? a2[r] : 0.0; }
    wave_sum16(v);
    if (lane < 16 && ri < n) {
      if (idx < 8) u1[ri] = v[0];
      else if (s2) u2[ri] = v[0];
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) { v[r] = a3[r]; v[8 + r] = 0.0; }
    wave_sum16(v);
    if (lane < 16 && idx < 8 && ri < n) u3[ri] = v[0];
  }
  __syncthreads();
}
template <int NT>
__device__ void full_matvec3(const double* M, int n, int ld, const double* s1, double* u1,
                             const double* s2, double* u2, const double* g3, double* u3) {
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int RB = 4;
  for (int i0 = w; i0 < n; i0 += NW * RB) {
    double a1[RB], a2[RB], a3[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) { a1[r] = 0.0; a2[r] = 0.0; a3[r] = 0.0; }
    for (int jj = lane; jj < n; jj += WAVE) {
      double rv[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = i0 + r * NW;
        rv[r] = M[(long)((i < n) ? i : n - 1) * ld + jj];
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        a1[r] = fma(rv[r], s1[jj], a1[r]);
        if (s2) a2[r] = fma(rv[r], s2[jj], a2[r]);
        a3[r] = fma(rv[r], -g3[jj], a3[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int i = i0 + r * NW;
      const double t1 = wave_sum(a1[r]);
      const double t2 = s2 ? wave_sum(a2[r]) : 0.0;
      const double t3 = wave_sum(a3[r]);
      if (lane == 0 && i < n) { u1[i] = t1; if (s2) u2[i] = t2; u3[i] = t3; }
    }
  }
  __syncthreads();
}

// u = R^T s  (R upper triangular; thread per column j: sum_{i<=j} R[i][j] s_i; coalesced across threads)
template <int NT>
__device__ __forceinline__ void tri_mtv(const double* R, int n, int ld, const double* s,
                                        double* u) {
  for (int j = threadIdx.x; j < n; j += NT) {
    double acc = 0.0;
    // 32 rows per pass, unconditional (clamped) loads in flight together: the passes are serialised by
    // their waits, and the longest column has n rows (8 per pass: 32 round trips at n = 256)
    for (int i0 = 0; i0 <= j; i0 += 32) {
      double rv[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) rv[k] = R[(long)((i0 + k <= j) ? i0 + k : j) * ld + j];
#pragma unroll
      for (int k = 0; k < 32; ++k)
        if (i0 + k <= j) acc = fma(rv[k], s[i0 + k], acc);
    }
    u[j] = acc;
  }
  __syncthreads();
}

}  // namespace blsq
