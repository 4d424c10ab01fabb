// Separable fits: variable projection of the linear parameters (blsq_varpro_expand_dev, blsq_varpro_reduce_dev;
// DESIGN.md 7v).  The second stage behind the model-eval entries, which write the raw Jacobian G [B][m][n] of the model
// at unit linear parameters.  With lin the nl linear columns (Phi), non the na = n - nl others, w the weights:
//   Phi_w = w Phi,  A_w = [w G[:, non] | w y],  S = Phi_w^T Phi_w
//   T  = S^-1 Phi_w^T A_w      E  = A_w - Phi_w T
//   T2 = S^-1 Phi_w^T E        E <- E - Phi_w T2,  T <- T + T2       (one correction against Phi_w itself)
//   c  = T[:, last]   f = -E[:, last]   J[:, i] = c[owner[non[i]]] E[:, i]                    (Kaufman's Jacobian)
// models.varpro_reduce of bounded_lsq/_varpro.py is the definition.
//
// varpro_reduce_kernel: one workgroup of four waves per problem, three passes over the rows in blocks of 64.  A block is
// staged into LDS in the WORK layout: columns 0 .. 15 Phi_w padded with zeros, then the na non-linear columns, then w y,
// then zeros up to a multiple of 16: NT = 1 + ceil((na + 1) / 16) <= 5 tiles of 16 columns; the weights are applied and
// the columns gathered while staging (consecutive threads read consecutive doubles of a row of G).  Wave v owns rows
// 16 v .. 16 v + 15 of the block.
//   pass 1  the moments Phi_w^T [Phi_w | A_w] (16 x 16 NT) on v_mfma_f64_16x16x4_f64: Phi_w of the block is the 16-wide
//           operand; k-step g of a wave takes its rows g, 4 + g, 8 + g, 12 + g.  Tile 0 is S.
//   factor  S is scaled to unit diagonal, D S D with D = diag(S)^-1/2, and wave 0 factors it with chol16_blocked3, which
//           also leaves the inverse of the factor: S^-1 = D Ri Ri^T D.  A diagonal entry that is not positive and finite
//           or a pivot of the scaled matrix that is not above VARPRO_PIVOT_TOL eps marks the problem rank deficient:
//           info = 1, every output NaN, and the workgroup leaves.
//   pass 2  E = A_w - Phi_w T of a block as a second MFMA product (the block is the accumulator, -Phi_w the left
//           operand) — in registers, and in the accumulator layout it is at once the right operand of the moments
//           Phi_w^T E.
//   pass 3  E again (the same instructions on the same operands: the same bits), E - Phi_w T2 by one more product, and
//           the outputs.
// A problem of m <= 64 rows is one block: it is staged once and stays in LDS for all three passes.  A longer one
// re-stages its blocks from global memory in every pass (three reads of a problem's G, which the L2 serves for the sizes
// of a fit).  The staged doubles are the same either way, so the switch between m = 64 and m = 65 changes no bit.
//
// Summation order, a function of (m, the work layout) alone: a wave adds its blocks in ascending order into its
// accumulators, and the four waves add theirs into the moments in the order 0, 1, 2, 3.  Nothing depends on B or on the
// batch mates.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"
#include "chol16.h"

namespace blsq {

static constexpr int VP_NT = 256;                // four waves
static constexpr int VP_ROWS = 64;               // rows of a block
static constexpr int VP_MAX_TILES = 5;           // Phi, and up to 64 columns of A_w
static constexpr int VP_PAD = 255, VP_YCOL = 254;
static constexpr double VP_PIVOT_TOL = 64.0 * DBL_EPS;   // VARPRO_PIVOT_TOL of bounded_lsq/_varpro.py

struct VarproArgs {
  static constexpr bool global = false;
  int m, n, nl, na, nt;         // nt: tiles of the work layout
  const double* G;
  const double* y;
  const double* w; long w_stride;
  double* f; double* J; double* c; int* info;
  const int* mask;
  unsigned char col[16 * VP_MAX_TILES];   // work column -> column of G, VP_YCOL (w y) or VP_PAD (zeros)
  signed char own[BLSQ_MODEL_MAX_N];      // non-linear column i -> position in lin of the amplitude it scales with
};

// What a separable global fit adds: workgroup b = g S + s is data set s of group g.  The nv = nsh + S nloc
// solver variables of a group are the shared non-linear parameters, then the window of nloc local ones of data set 0,
// 1, ... (GlobalMap of bounded_lsq/_params.py over the non-linear parameters).
struct VarproGlobalArgs {
  int S, nv, nsh, nloc;
  double* Sinv;                           // [G S][nl][nl] or nullptr
  double* TD;                             // [G S][nl][na] or nullptr
  unsigned char vcol[BLSQ_MODEL_MAX_N];   // non-linear column i -> its variable in data set 0
  unsigned char vloc[BLSQ_MODEL_MAX_N];   // 1: local (data set s: vcol + s nloc), 0: shared

  __device__ __forceinline__ int column(int i, int s) const { return vcol[i] + (vloc[i] ? s * nloc : 0); }
  __device__ __forceinline__ bool owns(int v, int s) const { return v < nsh || (v - nsh) / nloc == s; }
};

struct VarproReduceGlobalArgs : VarproArgs {
  static constexpr bool global = true;
  VarproGlobalArgs q;
};

struct VarproExpandArgs {
  int n, na;
  const double* X;
  double* P;
  signed char src[BLSQ_MODEL_MAX_N];      // parameter j -> solver variable, or -1: a linear slot (1.0)
};

__global__ __launch_bounds__(256) void varpro_expand_kernel(VarproExpandArgs A, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long b = e / A.n;
  const int j = (int)(e - b * A.n);
  const int s = A.src[j];
  A.P[e] = s < 0 ? 1.0 : A.X[b * A.na + s];
}

__global__ __launch_bounds__(256) void varpro_expand_global_kernel(VarproExpandArgs A, VarproGlobalArgs Q, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long b = e / A.n;
  const int j = (int)(e - b * A.n);
  const int i = A.src[j];
  const long g = b / Q.S;
  A.P[e] = i < 0 ? 1.0 : A.X[g * Q.nv + Q.column(i, (int)(b - g * Q.S))];
}

// double-double arithmetic for the one extra correction of TD (7x): error-free sum and product, FMA for the latter
// (no contraction of their own sums and products: the error terms are exact only for the operations as written)
struct dd { double hi, lo; };
__device__ __forceinline__ dd dd_add(dd x, dd y) {
#pragma clang fp contract(off)
  const double s = x.hi + y.hi, bb = s - x.hi;
  const double e = ((x.hi - (s - bb)) + (y.hi - bb)) + (x.lo + y.lo);
  const double hi = s + e;
  return {hi, e - (hi - s)};
}
__device__ __forceinline__ dd dd_mul(dd x, double d) {
#pragma clang fp contract(off)
  const double p = x.hi * d;
  const double e = fma(x.lo, d, fma(x.hi, d, -p));
  const double hi = p + e;
  return {hi, e - (hi - p)};
}
// x - a b
__device__ __forceinline__ dd dd_sub_prod(dd x, double a, double b) {
#pragma clang fp contract(off)
  const double p = -a * b;
  return dd_add(x, dd{p, fma(-a, b, -p)});
}

// rows [i0, i0 + 64) of the problem in the work layout (rows past m: zeros).  Holds two barriers.
__device__ __forceinline__ void varpro_stage(const VarproArgs& A, const double* __restrict__ Gb,
                                             const double* __restrict__ yb, const double* __restrict__ wb, int i0,
                                             double* tile, int nc, int ld) {
  __syncthreads();                                // the block before is done with
  for (int e = threadIdx.x; e < VP_ROWS * nc; e += VP_NT) {
    const int r = e / nc, k = e - r * nc;
    const int i = i0 + r, src = A.col[k];
    double v = 0.0;
    if (i < A.m && src != VP_PAD) {
      v = src == VP_YCOL ? yb[i] : Gb[(long)i * A.n + src];
      if (wb) v = wb[i] * v;
    }
    tile[r * ld + k] = v;
  }
  __syncthreads();
}

// the accumulators of the four waves into Mo (16 x nc), in the order of the waves.  Holds four barriers.
__device__ __forceinline__ void varpro_fold(const v4d (&acc)[VP_MAX_TILES], int t0, int nt, double* Mo, int nc) {
  const int lane = lane_id(), lr = lane >> 4, lc = lane & 15, wv = wave_id();
  for (int q = 0; q < VP_NT / WAVE; ++q) {
    if (wv == q) {
#pragma unroll
      for (int t = 0; t < VP_MAX_TILES; ++t) {
        if (t < t0 || t >= nt) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int at = (lr + 4 * g) * nc + TILE * t + lc;
          Mo[at] = q == 0 ? acc[t][g] : Mo[at] + acc[t][g];
        }
      }
    }
    __syncthreads();
  }
}

// To = S^-1 Mo over the work columns [16 t0, nc): Z = Ri^T D Mo, To = D Ri Z, each sum in ascending order.  Holds two
// barriers; the caller has one before (Mo complete).
__device__ __forceinline__ void varpro_solve(const double* Mo, double* Z, double* To, const double* Ri,
                                             const double* dsc, int t0, int nc) {
  const int k0 = TILE * t0, wide = nc - k0;
  for (int e = threadIdx.x; e < TILE * wide; e += VP_NT) {
    const int q = e / wide, k = k0 + e - q * wide;
    double z = 0.0;
    for (int p = 0; p <= q; ++p) z = fma(Ri[p * TILE + q], dsc[p] * Mo[p * nc + k], z);
    Z[q * nc + k] = z;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TILE * wide; e += VP_NT) {
    const int p = e / wide, k = k0 + e - p * wide;
    double v = 0.0;
    for (int q = p; q < TILE; ++q) v = fma(Ri[p * TILE + q], Z[q * nc + k], v);
    To[p * nc + k] = dsc[p] * v;
  }
  __syncthreads();
}

// E = A_w - Phi_w T for tile t of the wave's 16 rows: E[g] is row r0 + lr + 4 g, work column 16 t + lc
__device__ __forceinline__ v4d varpro_project(const double* tile, int ld, int r0, int t, const double* T, int nc, v4d E) {
  const int lane = lane_id(), lr = lane >> 4, lc = lane & 15;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    E = mfma_f64(-tile[(r0 + lc) * ld + 4 * s + lr], T[(4 * s + lr) * nc + TILE * t + lc], E);
  return E;
}

// Args = VarproReduceGlobalArgs (GLOBAL; blsq_varpro_reduce_global_dev, 7x): problem b is data set s = b % S of group g = b / S.  G, y, w, f, c and
// info are indexed by b as they are without it (y and f [G][S m] are [G S][m]); the mask is per group; J goes into the
// group's layout [g][s m + i][nv], Kaufman's columns at q.column(k, s) and +0.0 in every column of those rows that is
// not one of data set s, so that the workgroups of a group together write every element of its J exactly once; and
// Sinv = D Ri Ri^T D and TD = c[own] (T + T2) leave the LDS they are in after pass 2, TD after one more correction of
// T in double-double arithmetic (below).
template <class Args>
__global__ __launch_bounds__(VP_NT) void varpro_reduce_kernel(Args A) {
  constexpr bool GLOBAL = Args::global;
  extern __shared__ double vp_lds[];
  const long b = blockIdx.x;
  if constexpr (GLOBAL) {
    if (A.mask && A.mask[b / A.q.S] == 0) return; // a masked group: nothing of it is read or written
  } else {
    if (A.mask && A.mask[b] == 0) return;         // a masked problem: nothing of it is read or written
  }
  const int m = A.m, n = A.n, nl = A.nl, na = A.na, nt = A.nt;
  const int nc = TILE * nt, ld = nc + 1;
  double* tile = vp_lds;                          // 64 x ld
  double* Mo = tile + VP_ROWS * ld;               // 16 x nc: moments
  double* Z = Mo + TILE * nc;                     // 16 x nc
  double* T = Z + TILE * nc;                      // 16 x nc
  double* T2 = T + TILE * nc;                     // 16 x nc
  double* Dt = T2 + TILE * nc;                    // 16 x 16: D S D, then its factor
  double* Ri = Dt + TILE * TILE;                  // 16 x 16: the inverse of the factor
  double* dsc = Ri + TILE * TILE;                 // 16: D
  double* cs = dsc + TILE;                        // 16: c
  double* flag = cs + TILE;                       // 2: rank deficient (diagonal, pivot)
  const double* Gb = A.G + b * (long)m * n;
  const double* yb = A.y + b * (long)m;
  const double* wb = A.w ? A.w + b * A.w_stride : nullptr;
  const int tid = threadIdx.x, lane = lane_id(), lr = lane >> 4, lc = lane & 15, wv = wave_id();
  const int r0 = TILE * wv;
  const v4d zero = {0.0, 0.0, 0.0, 0.0};
  v4d acc[VP_MAX_TILES];
  int ds = 0;                                     // GLOBAL: the data set within its group
  if constexpr (GLOBAL) {
    ds = (int)(b % A.q.S);
    if (A.J) {                                    // the columns of the other data sets, in this one's rows
      const int nv = A.q.nv;
      double* Jb = A.J + b * (long)m * nv;
      for (long e = tid; e < (long)m * nv; e += VP_NT)
        if (!A.q.owns((int)(e % nv), ds)) Jb[e] = 0.0;
    }
  }

  // ---- pass 1: Phi_w^T [Phi_w | A_w] ----
#pragma unroll
  for (int t = 0; t < VP_MAX_TILES; ++t) acc[t] = zero;
  for (int i0 = 0; i0 < m; i0 += VP_ROWS) {
    varpro_stage(A, Gb, yb, wb, i0, tile, nc, ld);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const double* row = tile + (r0 + lr + 4 * g) * ld;
      const double a = row[lc];
#pragma unroll
      for (int t = 0; t < VP_MAX_TILES; ++t)
        if (t < nt) acc[t] = mfma_f64(a, row[TILE * t + lc], acc[t]);
    }
  }
  varpro_fold(acc, 0, nt, Mo, nc);

  // ---- factor: D S D = R^T R, Ri = R^-1 ----
  if (tid < TILE) {
    const double d = Mo[tid * nc + tid];
    const bool ok = tid >= nl || (d > 0.0 && is_finite(d));
    dsc[tid] = (tid < nl && ok) ? 1.0 / sqrt(d) : 0.0;
    if (tid == 0) flag[0] = flag[1] = 0.0;
  }
  __syncthreads();
  if (tid < nl && dsc[tid] == 0.0) flag[0] = 1.0;
  Dt[tid] = Mo[(tid >> 4) * nc + (tid & 15)] * dsc[tid >> 4] * dsc[tid & 15];
  __syncthreads();
  if (wv == 0) {
    const double pmin = chol16_blocked3(Dt, Ri, nl, __builtin_huge_val());
    if (lane == 0 && !(pmin > VP_PIVOT_TOL)) flag[1] = 1.0;
  }
  __syncthreads();
  if (flag[0] != 0.0 || flag[1] != 0.0) {         // rank deficient: NaN everywhere (uniform per workgroup)
    const double nan = __builtin_nan("");
    if (A.f) for (int i = tid; i < m; i += VP_NT) A.f[b * (long)m + i] = nan;
    if constexpr (GLOBAL) {
      if (A.J)
        for (long e = tid; e < (long)m * na; e += VP_NT)
          A.J[(b * (long)m + e / na) * A.q.nv + A.q.column((int)(e % na), ds)] = nan;
      if (A.q.Sinv) for (int e = tid; e < nl * nl; e += VP_NT) A.q.Sinv[b * (long)nl * nl + e] = nan;
      if (A.q.TD) for (int e = tid; e < nl * na; e += VP_NT) A.q.TD[b * (long)nl * na + e] = nan;
    } else {
      if (A.J) for (long e = tid; e < (long)m * na; e += VP_NT) A.J[b * (long)m * na + e] = nan;
    }
    if (A.c && tid < nl) A.c[b * (long)nl + tid] = nan;
    if (A.info && tid == 0) A.info[b] = 1;
    return;
  }
  varpro_solve(Mo, Z, T, Ri, dsc, 1, nc);

  // ---- pass 2: Phi_w^T E, E = A_w - Phi_w T ----
  const bool resident = m <= VP_ROWS;             // the one block of pass 1 is still in LDS
#pragma unroll
  for (int t = 0; t < VP_MAX_TILES; ++t) acc[t] = zero;
  for (int i0 = 0; i0 < m; i0 += VP_ROWS) {
    if (!resident) varpro_stage(A, Gb, yb, wb, i0, tile, nc, ld);
#pragma unroll
    for (int t = 1; t < VP_MAX_TILES; ++t) {
      if (t >= nt) continue;
      v4d E;
#pragma unroll
      for (int g = 0; g < 4; ++g) E[g] = tile[(r0 + lr + 4 * g) * ld + TILE * t + lc];
      E = varpro_project(tile, ld, r0, t, T, nc, E);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[t] = mfma_f64(tile[(r0 + lr + 4 * g) * ld + lc], E[g], acc[t]);
    }
  }
  varpro_fold(acc, 1, nt, Mo, nc);
  varpro_solve(Mo, Z, T2, Ri, dsc, 1, nc);
  if (tid < TILE) cs[tid] = T[tid * nc + TILE + na] + T2[tid * nc + TILE + na];
  __syncthreads();
  if (A.c && tid < nl) A.c[b * (long)nl + tid] = cs[tid];
  if (A.info && tid == 0) A.info[b] = 0;
  if constexpr (GLOBAL) {
    if (A.q.Sinv)                                  // (Ri Ri^T)[p][q] = sum over k >= max(p, q), ascending; mirrored
      for (int e = tid; e < nl * nl; e += VP_NT) {
        const int p = e / nl, q = e - p * nl, lo = p < q ? p : q, hi = p < q ? q : p;
        double v = 0.0;
        for (int k = hi; k < nl; ++k) v = fma(Ri[lo * TILE + k], Ri[hi * TILE + k], v);
        A.q.Sinv[b * (long)nl * nl + e] = dsc[lo] * dsc[hi] * v;
      }
    if (A.q.TD) {
      // TD = c[own] T needs T beyond the kappa eps |T| of the scheme: a column of T is the least-squares solution for
      // a column of G, whose residual is as large as the column, and |T| reaches |G_i| / sigma_min(Phi_w).  One more
      // correction, T3 = (T + T2) + S^-1 Phi_w^T (A_w - Phi_w (T + T2)), with the residual and its moments in
      // double-double arithmetic on the unrounded w G (read from global memory, not from the staged block): the
      // solve through the factor contracts the error by kappa^2 eps per step, so one step leaves the rounding of the
      // sum.  Column na (w y) gives the c that multiplies; the outputs c, f and J are not touched.
      for (int e = tid; e < TILE * nc; e += VP_NT) Mo[e] = 0.0;
      __syncthreads();
      const int wide = na + 1;
      for (int e = tid; e < nl * wide; e += VP_NT) {
        const int p = e / wide, k = e - p * wide;
        const int src = A.col[TILE + k], cp = A.col[p];
        dd acc = {0.0, 0.0};
        for (int i = 0; i < m; ++i) {
          const double* row = Gb + (long)i * n;
          dd r = {src == VP_YCOL ? yb[i] : row[src], 0.0};
          for (int q = 0; q < nl; ++q)
            r = dd_sub_prod(r, row[A.col[q]], T[q * nc + TILE + k] + T2[q * nc + TILE + k]);
          if (wb) r = dd_mul(dd_mul(r, wb[i]), wb[i]);
          acc = dd_add(acc, dd_mul(r, row[cp]));
        }
        Mo[p * nc + TILE + k] = acc.hi + acc.lo;
      }
      __syncthreads();
      varpro_solve(Mo, Z, Mo, Ri, dsc, 1, nc);      // (in place: the second half reads Z alone)
      for (int e = tid; e < nl * na; e += VP_NT) {
        const int p = e / na, i = e - p * na, o = A.own[i];
        const double c3 = (T[o * nc + TILE + na] + T2[o * nc + TILE + na]) + Mo[o * nc + TILE + na];
        A.q.TD[b * (long)nl * na + e] = c3 * ((T[p * nc + TILE + i] + T2[p * nc + TILE + i]) + Mo[p * nc + TILE + i]);
      }
      __syncthreads();
    }
  }
  if (!A.f && !A.J) return;

  // ---- pass 3: E - Phi_w T2 and the outputs ----
  for (int i0 = 0; i0 < m; i0 += VP_ROWS) {
    if (!resident) varpro_stage(A, Gb, yb, wb, i0, tile, nc, ld);
#pragma unroll
    for (int t = 1; t < VP_MAX_TILES; ++t) {
      if (t >= nt) continue;
      v4d E;
#pragma unroll
      for (int g = 0; g < 4; ++g) E[g] = tile[(r0 + lr + 4 * g) * ld + TILE * t + lc];
      E = varpro_project(tile, ld, r0, t, T, nc, E);
      E = varpro_project(tile, ld, r0, t, T2, nc, E);
      const int k = TILE * (t - 1) + lc;          // column of A_w
      const double scale = k < na ? cs[A.own[k]] : -1.0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long i = (long)i0 + r0 + lr + 4 * g;
        if constexpr (GLOBAL) {
          if (i < m && k < na && A.J) A.J[(b * (long)m + i) * A.q.nv + A.q.column(k, ds)] = scale * E[g];
        } else {
          if (i < m && k < na && A.J) A.J[(b * (long)m + i) * na + k] = scale * E[g];
        }
        if (i < m && k == na && A.f) A.f[b * (long)m + i] = -E[g];
      }
    }
  }
}

// The per-data-set blocks of the covariance of a separable global fit (blsq_varpro_cov_blocks_dev, 7x): one workgroup
// per data set b = g S + s.  C_s, the rows and columns of the group's reduced covariance C [nv][nv] that belong to data
// set s (read from the upper triangle, so C_s is symmetric), TD_s, W = TD_s C_s and Sinv_s stay in LDS:
//   alpha-alpha = C_s    c-alpha = -W    c-c = Sinv_s + W TD_s^T
// every sum in ascending order; element (j, k) and (k, j) are computed from the same operands in the same order, so the
// block is exactly symmetric.  NaN for a data set with info = 1 or a group with status != 0.
struct VarproCovArgs {
  int n, nl, na;
  const double* C; const double* Sinv; const double* TD; const double* scale;
  const int* info; const int* status;
  double* cov;
  signed char src[BLSQ_MODEL_MAX_N];      // parameter j -> its position in non, or -1
  signed char pos[BLSQ_MODEL_MAX_N];      // parameter j -> its position in lin, or -1
};

__global__ __launch_bounds__(256) void varpro_cov_blocks_kernel(VarproCovArgs A, VarproGlobalArgs Q) {
  extern __shared__ double vc_lds[];
  const long b = blockIdx.x;
  const long g = b / Q.S;
  const int s = (int)(b - g * Q.S);
  const int n = A.n, nl = A.nl, na = A.na, nv = Q.nv, tid = threadIdx.x;
  double* out = A.cov + b * (long)n * n;
  if ((A.info && A.info[b] != 0) || (A.status && A.status[g] != 0)) {
    const double nan = __builtin_nan("");
    for (int e = tid; e < n * n; e += 256) out[e] = nan;
    return;
  }
  double* Cs = vc_lds;                            // na x na
  double* Td = Cs + na * na;                      // nl x na
  double* W = Td + nl * na;                       // nl x na
  double* Si = W + nl * na;                       // nl x nl
  const double* Cg = A.C + g * (long)nv * nv;
  for (int e = tid; e < na * na; e += 256) {
    const int a = e / na, c = e - a * na;
    const int va = Q.column(a, s), vb = Q.column(c, s);
    Cs[e] = Cg[(long)(va < vb ? va : vb) * nv + (va < vb ? vb : va)];
  }
  for (int e = tid; e < nl * na; e += 256) Td[e] = A.TD[b * (long)nl * na + e];
  for (int e = tid; e < nl * nl; e += 256) {
    const int p = e / nl, q = e - p * nl;
    Si[e] = A.Sinv[b * (long)nl * nl + (p < q ? p * nl + q : q * nl + p)];
  }
  __syncthreads();
  for (int e = tid; e < nl * na; e += 256) {
    const int p = e / na, a = e - p * na;
    double v = 0.0;
    for (int i = 0; i < na; ++i) v = fma(Td[p * na + i], Cs[i * na + a], v);
    W[e] = v;
  }
  __syncthreads();
  const double sc = A.scale ? A.scale[g] : 1.0;
  for (int e = tid; e < n * n; e += 256) {
    const int j = e / n, k = e - j * n, lo = j < k ? j : k, hi = j < k ? k : j;
    const int a = A.src[lo], c = A.src[hi], p = A.pos[lo], q = A.pos[hi];
    double v;
    if (a >= 0 && c >= 0) {
      v = Cs[a * na + c];
    } else if (p >= 0 && q >= 0) {
      double t = 0.0;
      for (int i = 0; i < na; ++i) t = fma(W[p * na + i], Td[q * na + i], t);
      v = Si[p * nl + q] + t;
    } else {
      v = -(p >= 0 ? W[p * na + c] : W[q * na + a]);
    }
    out[e] = sc * v;
  }
}

size_t varpro_lds_bytes(int na) {
  const int nt = 1 + (na + 1 + TILE - 1) / TILE, nc = TILE * nt;
  return sizeof(double) * ((size_t)VP_ROWS * (nc + 1) + 4 * (size_t)TILE * nc + 2 * TILE * TILE + 2 * TILE + 2);
}

hipError_t launch_varpro_expand(const VarproExpandCall& c, hipStream_t s) {
  if (c.B < 1 || c.n < 2 || c.n > BLSQ_MODEL_MAX_N || c.nl < 1 || c.nl >= c.n || !c.lin || !c.X || !c.P)
    return hipErrorInvalidValue;
  VarproExpandArgs A;
  A.n = c.n; A.na = c.n - c.nl; A.X = c.X; A.P = c.P;
  int at = 0, v = 0;
  for (int j = 0; j < c.n; ++j) {
    if (at < c.nl && c.lin[at] == j) { A.src[j] = -1; ++at; }
    else A.src[j] = (signed char)v++;
  }
  if (at != c.nl) return hipErrorInvalidValue;    // lin not ascending within 0 .. n - 1
  for (int j = c.n; j < BLSQ_MODEL_MAX_N; ++j) A.src[j] = -1;
  const long total = (long)c.B * c.n;
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(varpro_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A, total);
  return hipGetLastError();
}

// the arguments of the reduce kernel from a call (B problems): false for what launch_varpro_reduce refuses
static bool varpro_reduce_args(const VarproReduceCall& c, long B, VarproArgs& A) {
  if (B < 1 || c.n < 2 || c.n > BLSQ_MODEL_MAX_N || c.nl < 1 || c.nl > BLSQ_VARPRO_MAX_NL || c.nl >= c.n ||
      c.m <= c.nl)
    return false;
  if (!c.lin || !c.owner || !c.G || !c.y) return false;
  A.m = c.m; A.n = c.n; A.nl = c.nl; A.na = c.n - c.nl;
  A.nt = 1 + (A.na + 1 + TILE - 1) / TILE;
  A.G = c.G; A.y = c.y; A.w = c.w; A.w_stride = c.w ? c.w_stride : 0;
  A.f = c.f; A.J = c.J; A.c = c.c; A.info = c.info; A.mask = c.mask;
  for (int k = 0; k < TILE * VP_MAX_TILES; ++k) A.col[k] = VP_PAD;
  for (int i = 0; i < BLSQ_MODEL_MAX_N; ++i) A.own[i] = 0;
  int at = 0, v = 0;
  for (int j = 0; j < c.n; ++j) {
    if (at < c.nl && c.lin[at] == j) {
      if (c.owner[j] != -1) return false;
      A.col[at++] = (unsigned char)j;
    } else {
      if (c.owner[j] < 0 || c.owner[j] >= c.nl) return false;
      A.own[v] = (signed char)c.owner[j];
      A.col[TILE + v++] = (unsigned char)j;
    }
  }
  if (at != c.nl) return false;                   // lin not ascending within 0 .. n - 1
  A.col[TILE + A.na] = VP_YCOL;
  return true;
}

hipError_t launch_varpro_reduce(const VarproReduceCall& c, hipStream_t s) {
  if (!c.f && !c.J && !c.c) return hipErrorInvalidValue;
  if (c.w && c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  VarproArgs A;
  if (!varpro_reduce_args(c, c.B, A)) return hipErrorInvalidValue;
  return launch<varpro_reduce_kernel<VarproArgs>>(dim3((unsigned)c.B), dim3(VP_NT), varpro_lds_bytes(A.na), s, A);
}

// the layout of a group from lin and the 0 / 1 flags shared [n] of the model parameters: false for a flag that is
// neither, a flag set on a linear parameter, or nv above BLSQ_GLOBAL_MAX_NV.  src: parameter -> position in non or -1.
static bool varpro_global_layout(int S, int n, int nl, const int* lin, const int* shared, VarproGlobalArgs& Q,
                                 signed char* src, signed char* pos) {
  if (S < 1 || !lin || !shared) return false;
  Q.S = S; Q.nsh = 0; Q.nloc = 0; Q.Sinv = nullptr; Q.TD = nullptr;
  for (int i = 0; i < BLSQ_MODEL_MAX_N; ++i) { Q.vcol[i] = 0; Q.vloc[i] = 0; src[i] = -1; if (pos) pos[i] = -1; }
  int at = 0, v = 0;
  for (int j = 0; j < n; ++j) {
    if (shared[j] != 0 && shared[j] != 1) return false;
    if (at < nl && lin[at] == j) {
      if (shared[j]) return false;
      if (pos) pos[j] = (signed char)at;
      ++at;
      continue;
    }
    Q.vloc[v] = shared[j] ? 0 : 1;
    Q.vcol[v] = (unsigned char)(shared[j] ? Q.nsh++ : Q.nloc++);
    src[j] = (signed char)v++;
  }
  if (at != nl) return false;
  for (int i = 0; i < v; ++i)
    if (Q.vloc[i]) Q.vcol[i] = (unsigned char)(Q.vcol[i] + Q.nsh);
  const long nv = (long)Q.nsh + (long)S * Q.nloc;
  if (nv > BLSQ_GLOBAL_MAX_NV) return false;
  Q.nv = (int)nv;
  if (Q.nloc == 0) Q.nloc = 1;                    // (the divisor of owns(); nothing is local then)
  return true;
}

int varpro_global_nv(int S, int n, int nl, const int* lin, const int* shared) {
  VarproGlobalArgs Q;
  signed char src[BLSQ_MODEL_MAX_N];
  if (n < 2 || n > BLSQ_MODEL_MAX_N || nl < 1 || nl >= n) return -1;
  return varpro_global_layout(S, n, nl, lin, shared, Q, src, nullptr) ? Q.nv : -1;
}

hipError_t launch_varpro_expand_global(const VarproExpandCall& c, const VarproGlobalCall& q, hipStream_t s) {
  if (c.B < 1 || c.n < 2 || c.n > BLSQ_MODEL_MAX_N || c.nl < 1 || c.nl >= c.n || !c.lin || !c.X || !c.P)
    return hipErrorInvalidValue;
  VarproExpandArgs A;
  VarproGlobalArgs Q;
  if (!varpro_global_layout(q.S, c.n, c.nl, c.lin, q.shared, Q, A.src, nullptr)) return hipErrorInvalidValue;
  A.n = c.n; A.na = c.n - c.nl; A.X = c.X; A.P = c.P;
  const long total = (long)c.B * q.S * c.n;       // c.B: the groups
  const long blocks = (total + 255) / 256;
  if ((long)c.B * q.S > 0x7fffffffL || blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(varpro_expand_global_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A, Q, total);
  return hipGetLastError();
}

hipError_t launch_varpro_reduce_global(const VarproReduceCall& c, const VarproGlobalCall& q, hipStream_t s) {
  // c.B: the groups; c.w_stride: 0 or S m, the stride of a group, which is m per data set
  if (c.B < 1 || q.S < 1 || (long)c.B * q.S > 0x7fffffffL) return hipErrorInvalidValue;
  if (!c.f && !c.J && !c.c && !q.Sinv && !q.TD) return hipErrorInvalidValue;
  if (c.w && c.w_stride != 0 && c.w_stride != (long)q.S * c.m) return hipErrorInvalidValue;
  VarproReduceGlobalArgs A;
  signed char src[BLSQ_MODEL_MAX_N];
  if (!varpro_reduce_args(c, (long)c.B * q.S, A)) return hipErrorInvalidValue;
  if (!varpro_global_layout(q.S, c.n, c.nl, c.lin, q.shared, A.q, src, nullptr)) return hipErrorInvalidValue;
  A.w_stride = (c.w && c.w_stride != 0) ? (long)c.m : 0;
  A.q.Sinv = q.Sinv; A.q.TD = q.TD;
  return launch<varpro_reduce_kernel<VarproReduceGlobalArgs>>(dim3((unsigned)((long)c.B * q.S)), dim3(VP_NT),
                                                              varpro_lds_bytes(A.na), s, A);
}

hipError_t launch_varpro_cov_blocks(const VarproCovCall& c, hipStream_t s) {
  if (c.G < 1 || c.S < 1 || (long)c.G * c.S > 0x7fffffffL || c.n < 2 || c.n > BLSQ_MODEL_MAX_N || c.nl < 1 ||
      c.nl > BLSQ_VARPRO_MAX_NL || c.nl >= c.n || !c.lin || !c.shared || !c.C || !c.Sinv || !c.TD || !c.cov)
    return hipErrorInvalidValue;
  VarproCovArgs A;
  VarproGlobalArgs Q;
  if (!varpro_global_layout(c.S, c.n, c.nl, c.lin, c.shared, Q, A.src, A.pos)) return hipErrorInvalidValue;
  A.n = c.n; A.nl = c.nl; A.na = c.n - c.nl;
  A.C = c.C; A.Sinv = c.Sinv; A.TD = c.TD; A.scale = c.scale; A.info = c.info; A.status = c.status; A.cov = c.cov;
  const size_t lds = sizeof(double) * ((size_t)A.na * A.na + 2 * (size_t)A.nl * A.na + (size_t)A.nl * A.nl);
  return launch<varpro_cov_blocks_kernel>(dim3((unsigned)((long)c.G * c.S)), dim3(256), lds, s, A, Q);
}

}  // namespace blsq
