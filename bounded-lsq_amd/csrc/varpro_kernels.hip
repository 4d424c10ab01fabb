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
  int m, n, nl, na, nt;         // nt: tiles of the work layout
  const double* G;
  const double* y;
  const double* w; long w_stride;
  double* f; double* J; double* c; int* info;
  const int* mask;
  unsigned char col[16 * VP_MAX_TILES];   // work column -> column of G, VP_YCOL (w y) or VP_PAD (zeros)
  signed char own[BLSQ_MODEL_MAX_N];      // non-linear column i -> position in lin of the amplitude it scales with
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

__global__ __launch_bounds__(VP_NT) void varpro_reduce_kernel(VarproArgs A) {
  extern __shared__ double vp_lds[];
  const long b = blockIdx.x;
  if (A.mask && A.mask[b] == 0) return;           // a masked problem: nothing of it is read or written
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
    if (A.J) for (long e = tid; e < (long)m * na; e += VP_NT) A.J[b * (long)m * na + e] = nan;
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
        if (i < m && k < na && A.J) A.J[(b * (long)m + i) * na + k] = scale * E[g];
        if (i < m && k == na && A.f) A.f[b * (long)m + i] = -E[g];
      }
    }
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

hipError_t launch_varpro_reduce(const VarproReduceCall& c, hipStream_t s) {
  if (c.B < 1 || c.n < 2 || c.n > BLSQ_MODEL_MAX_N || c.nl < 1 || c.nl > BLSQ_VARPRO_MAX_NL || c.nl >= c.n ||
      c.m <= c.nl)
    return hipErrorInvalidValue;
  if (!c.lin || !c.owner || !c.G || !c.y || (!c.f && !c.J && !c.c)) return hipErrorInvalidValue;
  if (c.w && c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  VarproArgs A;
  A.m = c.m; A.n = c.n; A.nl = c.nl; A.na = c.n - c.nl;
  A.nt = 1 + (A.na + 1 + TILE - 1) / TILE;
  A.G = c.G; A.y = c.y; A.w = c.w; A.w_stride = c.w ? c.w_stride : 0;
  A.f = c.f; A.J = c.J; A.c = c.c; A.info = c.info; A.mask = c.mask;
  for (int k = 0; k < TILE * VP_MAX_TILES; ++k) A.col[k] = VP_PAD;
  for (int i = 0; i < BLSQ_MODEL_MAX_N; ++i) A.own[i] = 0;
  int at = 0, v = 0;
  for (int j = 0; j < c.n; ++j) {
    if (at < c.nl && c.lin[at] == j) {
      if (c.owner[j] != -1) return hipErrorInvalidValue;
      A.col[at++] = (unsigned char)j;
    } else {
      if (c.owner[j] < 0 || c.owner[j] >= c.nl) return hipErrorInvalidValue;
      A.own[v] = (signed char)c.owner[j];
      A.col[TILE + v++] = (unsigned char)j;
    }
  }
  if (at != c.nl) return hipErrorInvalidValue;    // lin not ascending within 0 .. n - 1
  A.col[TILE + A.na] = VP_YCOL;
  return launch<varpro_reduce_kernel>(dim3((unsigned)c.B), dim3(VP_NT), varpro_lds_bytes(A.na), s, A);
}

}  // namespace blsq
