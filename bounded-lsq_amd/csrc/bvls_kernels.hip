// Bounded-variable least squares by an exact active-set method (blsq_bvls_moments_dev, blsq_bvls_solve_dev):
//   min 1/2 |W (A x - y)|^2,  lb <= x <= ub        as the quadratic programme in  G = A^T W^2 A,  c = A^T W^2 y.
//
// Two kernels:
//   bvls_moments_kernel  out[p][j] = sum_i (w_i L(p, i)) (w_i R(i, j)) on the FP64 MFMA pipe (v_mfma_f64_16x16x4_f64): one
//                        wave owns 16 rows p and ALL columns j (NT tiles of 16), K runs over the rows i of A.
//                          shared A (and w not per problem):  G: L = A^T, R = A (one launch for the batch);
//                                                             c: L = Y (16 PROBLEMS per wave), R = A: a true GEMM;
//                          per-problem A or w:                L = A_b^T, R = [A_b | y_b]: G_b and c_b in one pass.
//                        Summation order, a function of m alone: rows come in blocks of 16; k-step s (0 .. 3) of block r
//                        feeds the MFMA the rows 16 r + 4 q + s, q = 0 .. 3, and the k-steps accumulate into one
//                        accumulator in ascending (r, s); rows past m enter as exact zeros.  An output depends on its
//                        row p of L and its column j of R only, so a problem's c does not depend on its batch mates, and
//                        G is symmetric in every bit (both operands carry w once: (w a')(w a) commutes).
//   bvls_solve_kernel    one problem per workgroup of ONE wave: the clip-in start, the release passes, the drop loops
//                        and (with A) the correction against A and the true residual, gradient and optimality, all in
//                        this launch.  LDS (dynamic, sized by n): the packed lower triangle of the current free
//                        block's Cholesky factor, column by column (lanes over the rows of a column read consecutive
//                        addresses), six n-vectors and three int n-vectors.  The free block is factored from scratch
//                        (left-looking) on every solve; the two substitutions keep the right-hand side in registers
//                        (lane l: entries l and l + 64) and broadcast through v_readlane: no barrier inside them.
//                        Every loop has a structural bound (start: n + 1 solves, passes: max_pass, drop loop: n + 1
//                        rounds, the release choice: asked at most twice), and a pivot <= 0 or not finite, or a value
//                        not finite, ends the problem with status -1: nothing spins.
//
// bvls_solve_kernel<true> (blsq_bvls_solve_eq_dev) is the same iteration under one equality e^T x = d:
// the feasible start in place of the clip-in start, a second right-hand side v = G_FF^-1 e_F per factorisation (both
// substitutions share one walk over the factor), the multiplier lambda, the reduced gradient g + lambda e in the
// release test and the projected correction against A.  LDS: two more n-vectors, e (by variable) and v (by the place
// of the variable in the free set).  bvls_solve_kernel<false> is the kernel described above, instruction for
// instruction: everything the equality adds stands behind `if constexpr (EQ)`.
//
// Compiled with -ffp-contract=off (EXACT_SRCS): every fused operation of this file is spelled fma(), so the stated
// summation orders and the exact bound values do not depend on what the compiler would contract.  The decisions are
// those of bounded_lsq._bvls.bvls_reference wherever no comparison is decided by rounding; the sums themselves are not
// in numpy's order.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"

#include <algorithm>
#include <climits>

namespace blsq {

static constexpr int BV_NT = WAVE;               // one wave per workgroup
static constexpr int BV_MAX_TILES = (BLSQ_BVLS_MAX_N + 1 + TILE - 1) / TILE;   // columns of [A | y]
static_assert(BLSQ_BVLS_MAX_N <= 2 * WAVE, "a lane holds two entries of an n-vector");

// ------------------------------------------------------------------------------------------------------ moments ----
// blockIdx.x = b * tilesP + tile: batch entry b (offsets *_bs), rows p0 .. p0 + 15 of the output.
// L(p, i) = left[p * lp + i * li];  R(i, j) = j < n ? A[i * n + j] : ycol[i] (ncols = n, or n + 1 with ycol);
// out: column j < n into outM[p * n + j], column n into outv[p].
template <int NT>
__global__ __launch_bounds__(BV_NT) void bvls_moments_kernel(int P, int tilesP, int m, int n, int ncols,
                                                             const double* __restrict__ left, long lp, long li,
                                                             long left_bs, const double* __restrict__ A, long A_bs,
                                                             const double* __restrict__ ycol, long y_bs,
                                                             const double* __restrict__ w, long w_bs,
                                                             double* __restrict__ outM, long outM_bs,
                                                             double* __restrict__ outv, long outv_bs) {
  const long b = blockIdx.x / tilesP;
  const int p0 = (int)(blockIdx.x % tilesP) * TILE;
  const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
  left += b * left_bs;
  A += b * A_bs;
  if (ycol) ycol += b * y_bs;
  if (w) w += b * w_bs;
  const int p = p0 + r;
  const bool p_in = p < P;
  v4d acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < m; i0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int i = i0 + 4 * q + s;
      const bool i_in = i < m;
      const double wi = (i_in && w) ? w[i] : 1.0;
      const double a = (i_in && p_in) ? wi * left[(long)p * lp + (long)i * li] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int j = TILE * t + r;
        double bv = 0.0;
        if (i_in && j < ncols) bv = wi * (j < n ? A[(long)i * n + j] : ycol[i]);
        acc[t] = mfma_f64(a, bv, acc[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = TILE * t + r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = p0 + q + 4 * g;
      if (row >= P || j >= ncols) continue;
      if (j < n) outM[b * outM_bs + (long)row * n + j] = acc[t][g];
      else outv[b * outv_bs + row] = acc[t][g];
    }
  }
}

template <int NT>
static hipError_t launch_moments_nt(long grid, hipStream_t s, int P, int tilesP, int m, int n, int ncols,
                                    const double* left, long lp, long li, long left_bs, const double* A, long A_bs,
                                    const double* ycol, long y_bs, const double* w, long w_bs, double* outM,
                                    long outM_bs, double* outv, long outv_bs) {
  return launch<bvls_moments_kernel<NT>>(dim3((unsigned)grid), dim3(BV_NT), 0, s, P, tilesP, m, n, ncols, left, lp, li,
                                         left_bs, A, A_bs, ycol, y_bs, w, w_bs, outM, outM_bs, outv, outv_bs);
}

// `batch` entries of P output rows each
static hipError_t launch_moments_one(hipStream_t s, long batch, int P, int m, int n, int ncols, const double* left,
                                     long lp, long li, long left_bs, const double* A, long A_bs, const double* ycol,
                                     long y_bs, const double* w, long w_bs, double* outM, long outM_bs, double* outv,
                                     long outv_bs) {
  const int tilesP = (P + TILE - 1) / TILE;
  const long grid = batch * tilesP;
  if (grid < 1 || grid > 0x7fffffffL) return hipErrorInvalidValue;
  const int nt = (ncols + TILE - 1) / TILE;
#define BV_CASE(NT_)                                                                                                  \
  case NT_:                                                                                                           \
    return launch_moments_nt<NT_>(grid, s, P, tilesP, m, n, ncols, left, lp, li, left_bs, A, A_bs, ycol, y_bs, w,     \
                                  w_bs, outM, outM_bs, outv, outv_bs)
  switch (nt) {
    BV_CASE(1); BV_CASE(2); BV_CASE(3); BV_CASE(4); BV_CASE(5); BV_CASE(6); BV_CASE(7); BV_CASE(8); BV_CASE(9);
  }
#undef BV_CASE
  static_assert(BV_MAX_TILES == 9, "one case per tile count");
  return hipErrorInvalidValue;
}

hipError_t launch_bvls_moments(const BvlsMomentsCall& c, hipStream_t s) {
  if (c.B < 1 || c.m < 1 || c.n < 1 || c.n > BLSQ_BVLS_MAX_N) return hipErrorInvalidValue;
  const long mn = (long)c.m * c.n, nn = (long)c.n * c.n;
  if (!c.A || !c.y || !c.G || !c.c) return hipErrorInvalidValue;
  if ((c.A_stride != 0 && c.A_stride != mn) || (c.w_stride != 0 && c.w_stride != (long)c.m)) return hipErrorInvalidValue;
  if (c.G_stride != 0 && c.G_stride != nn) return hipErrorInvalidValue;
  const bool per_problem = c.A_stride != 0 || (c.w && c.w_stride != 0);
  if (per_problem && c.G_stride == 0) return hipErrorInvalidValue;
  if (c.G_stride == 0) {
    // one G for the batch, then c as the GEMM Y (B x m) . A (m x n)
    const hipError_t e = launch_moments_one(s, 1, c.n, c.m, c.n, c.n, c.A, 1, c.n, 0, c.A, 0, nullptr, 0, c.w, 0, c.G,
                                            0, nullptr, 0);
    if (e != hipSuccess) return e;
    return launch_moments_one(s, 1, c.B, c.m, c.n, c.n, c.y, c.m, 1, 0, c.A, 0, nullptr, 0, c.w, 0, c.c, 0, nullptr, 0);
  }
  // problem by problem over [A_b | y_b]: G_b and c_b from one pass
  return launch_moments_one(s, c.B, c.n, c.m, c.n, c.n + 1, c.A, 1, c.n, c.A_stride, c.A, c.A_stride, c.y, c.m, c.w,
                            c.w ? c.w_stride : 0, c.G, nn, c.c, c.n);
}

// -------------------------------------------------------------------------------------------------------- solve ----
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, WAVE));
  return v;
}

// The state of one problem in LDS; every member function is called by the whole wave in uniform control flow.
struct BvlsState {
  int n, lane;
  const double* G;        // [n][n] of this problem
  const double* c;        // [n]
  double *Lt, *xs, *zs, *gs, *lbs, *ubs, *ts;
  int *fidx, *on, *barred;

  // the free variables in ascending order into fidx -> their number
  __device__ int build_free() {
    int k = 0;
    for (int base = 0; base < n; base += WAVE) {
      const int j = base + lane;
      const bool fr = j < n && on[j] == 0;
      const unsigned long long mask = __ballot(fr);
      if (fr) fidx[k + __popcll(mask & ((1ull << lane) - 1ull))] = j;
      k += __popcll(mask);
    }
    __syncthreads();
    return k;
  }

  // Cholesky factor of G_FF, left-looking, into Lt: entry (i, t), i >= t, at t k - t (t - 1) / 2 + (i - t).
  // false: a pivot <= 0 or not finite
  __device__ bool factor(int k) {
    for (int j = 0; j < k; ++j) {
      const double* Grow = G + (long)fidx[j] * n;                     // G is symmetric: row f_j, columns f_i
      const int i0 = j + lane, i1 = i0 + WAVE;
      double a0 = i0 < k ? Grow[fidx[i0]] : 1.0;
      double a1 = i1 < k ? Grow[fidx[i1]] : 1.0;
      const int r0 = i0 < k ? i0 : j, r1 = i1 < k ? i1 : j;           // (a lane past the end reads row j: in bounds)
      int o = 0;                                                      // offset of column t, less t
      for (int t = 0; t < j; ++t) {
        const double ljt = Lt[o + j];
        a0 = fma(-Lt[o + r0], ljt, a0);
        a1 = fma(-Lt[o + r1], ljt, a1);
        o += k - t - 1;
      }
      const double d = read_lane(a0, 0);                              // i0 == j on lane 0
      if (!(d > 0.0) || !is_finite(d)) return false;
      const double sd = sqrt(d);
      if (i0 < k) Lt[o + i0] = lane == 0 ? sd : a0 / sd;
      if (i1 < k) Lt[o + i1] = a1 / sd;
      __syncthreads();
    }
    return true;
  }

  // (L L^T)^-1 v for v in registers (v0: entry lane, v1: entry lane + 64; entries >= k are ignored and returned as 0)
  __device__ void tri_solve(int k, double& v0, double& v1) {
    const int i0 = lane, i1 = lane + WAVE;
    if (i0 >= k) v0 = 0.0;
    if (i1 >= k) v1 = 0.0;
    int off = 0;                                                      // offset of column t
    for (int t = 0; t < k; ++t) {
      const double yt = (t < WAVE ? read_lane(v0, t & 63) : read_lane(v1, t & 63)) / Lt[off];
      if (i0 == t) v0 = yt;
      if (i1 == t) v1 = yt;
      if (i0 > t && i0 < k) v0 = fma(-Lt[off + i0 - t], yt, v0);
      if (i1 > t && i1 < k) v1 = fma(-Lt[off + i1 - t], yt, v1);
      off += k - t;
    }
    // L^T z = y: entry (t, i) of L, i < t, at i k - i (i - 1) / 2 + (t - i)
    const int c0 = i0 * k - i0 * (i0 - 1) / 2 - i0, c1 = i1 * k - i1 * (i1 - 1) / 2 - i1;
    for (int t = k - 1; t >= 0; --t) {
      off -= k - t;
      const double zt = (t < WAVE ? read_lane(v0, t & 63) : read_lane(v1, t & 63)) / Lt[off];
      if (i0 == t) v0 = zt;
      if (i1 == t) v1 = zt;
      if (i0 < t) v0 = fma(-Lt[c0 + t], zt, v0);
      if (i1 < t) v1 = fma(-Lt[c1 + t], zt, v1);
    }
  }

  // tri_solve for two right-hand sides in one walk over Lt (the operations on each are those of tri_solve)
  __device__ void tri_solve2(int k, double& v0, double& v1, double& w0, double& w1) {
    const int i0 = lane, i1 = lane + WAVE;
    if (i0 >= k) v0 = w0 = 0.0;
    if (i1 >= k) v1 = w1 = 0.0;
    int off = 0;
    for (int t = 0; t < k; ++t) {
      const double piv = Lt[off];
      const double yt = (t < WAVE ? read_lane(v0, t & 63) : read_lane(v1, t & 63)) / piv;
      const double qt = (t < WAVE ? read_lane(w0, t & 63) : read_lane(w1, t & 63)) / piv;
      if (i0 == t) { v0 = yt; w0 = qt; }
      if (i1 == t) { v1 = yt; w1 = qt; }
      if (i0 > t && i0 < k) {
        const double l = Lt[off + i0 - t];
        v0 = fma(-l, yt, v0);
        w0 = fma(-l, qt, w0);
      }
      if (i1 > t && i1 < k) {
        const double l = Lt[off + i1 - t];
        v1 = fma(-l, yt, v1);
        w1 = fma(-l, qt, w1);
      }
      off += k - t;
    }
    const int c0 = i0 * k - i0 * (i0 - 1) / 2 - i0, c1 = i1 * k - i1 * (i1 - 1) / 2 - i1;
    for (int t = k - 1; t >= 0; --t) {
      off -= k - t;
      const double piv = Lt[off];
      const double zt = (t < WAVE ? read_lane(v0, t & 63) : read_lane(v1, t & 63)) / piv;
      const double qt = (t < WAVE ? read_lane(w0, t & 63) : read_lane(w1, t & 63)) / piv;
      if (i0 == t) { v0 = zt; w0 = qt; }
      if (i1 == t) { v1 = zt; w1 = qt; }
      if (i0 < t) {
        const double l = Lt[c0 + t];
        v0 = fma(-l, zt, v0);
        w0 = fma(-l, qt, w0);
      }
      if (i1 < t) {
        const double l = Lt[c1 + t];
        v1 = fma(-l, zt, v1);
        w1 = fma(-l, qt, w1);
      }
    }
  }

  // zs[f_i] = the solution of G_FF z = c_F - G_FB x_B; false: not positive definite, or a value not finite
  __device__ bool solve(int k) {
    if (!factor(k)) return false;
    double v[2];
    for (int h = 0; h < 2; ++h) {
      const int i = lane + h * WAVE;
      double acc = 0.0;
      if (i < k) {
        const int fi = fidx[i];
        acc = c[fi];
        for (int j = 0; j < n; ++j)
          if (on[j] != 0) acc = fma(-G[(long)j * n + fi], xs[j], acc);
      }
      v[h] = acc;
    }
    tri_solve(k, v[0], v[1]);
    bool bad = false;
    for (int h = 0; h < 2; ++h) {
      const int i = lane + h * WAVE;
      if (i < k) {
        zs[fidx[i]] = v[h];
        bad |= !is_finite(v[h]);
      }
    }
    __syncthreads();
    return !__any(bad);
  }

  // gs = G x - c -> false: an entry is not finite
  __device__ bool gradient() {
    bool bad = false;
    for (int j = lane; j < n; j += WAVE) {
      double acc = -c[j];
      for (int i = 0; i < n; ++i) acc = fma(G[(long)i * n + j], xs[i], acc);
      gs[j] = acc;
      bad |= !is_finite(acc);
    }
    __syncthreads();
    return !__any(bad);
  }

  // max(max over free |g_j|, max over bound g_j on_j, 0) of gs
  __device__ double optimality() {
    double v = 0.0;
    for (int j = lane; j < n; j += WAVE) v = nanmax2(v, on[j] == 0 ? fabs(gs[j]) : gs[j] * (double)on[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax2(v, __shfl_xor(v, o, WAVE));
    return v;
  }
};

// What the equality e^T x = d adds to the state (bvls_solve_kernel<true> only); every member function is called by the
// whole wave in uniform control flow.  Dot products over the free set: lane l forms fma(e_1, a_1, e_0 a_0) of its two
// entries (places l and l + 64), then wave_sum; the sums over all variables that feed a DECISION of the start (the gap
// d - e^T x) run in ascending j on every lane alike.
struct BvlsEq {
  double* es;             // [n] e, by variable
  double* vs;             // [n] v = G_FF^-1 e_F of the last solve, by place in the free set
  double d;
  double lam;             // lambda of the last accepted solve
  double lam_z;           // lambda of the last solve
  double ev;              // e_F^T v of the last solve

  // d - sum over the variables with on != 0 (BOUND_ONLY) or over all of them of e_j x_j, ascending j
  template <bool BOUND_ONLY>
  __device__ double gap(const BvlsState& st) const {
    double acc = d;
    for (int j = 0; j < st.n; ++j)
      if (!BOUND_ONLY || st.on[j] != 0) acc = fma(-es[j], st.xs[j], acc);
    return acc;
  }

  __device__ static double dot2(double e0, double a0, double e1, double a1) { return wave_sum(fma(e1, a1, e0 * a0)); }

  // x = clip(0, lb, ub) (already in xs) and the gap walked off in ascending j -> 2, or -1 / -2 with xs the clipped start
  __device__ int feasible_start(BvlsState& st) {
    const int n = st.n, lane = st.lane;
    bool bad = false;
    for (int j = lane; j < n; j += WAVE) bad |= !is_finite(es[j]) || es[j] == 0.0;
    int ret = (__any(bad) || !is_finite(d)) ? -1 : 2;
    if (ret == 2) {
      double g = gap<false>(st);
      for (int j = 0; j < n; ++j) {                                   // (uniform: every lane holds the same g)
        if (g == 0.0) break;
        const double ej = es[j], step = g / ej;
        if (!is_finite(g) || !is_finite(step)) { ret = -1; break; }
        const double xj = st.xs[j], lo = st.lbs[j], hi = st.ubs[j];
        const double bound = step > 0.0 ? hi : lo, room = bound - xj;
        double nx;
        if (fabs(step) <= fabs(room)) {
          nx = fmin(fmax(xj + step, lo), hi);
          g = 0.0;
        } else {
          nx = bound;
          g = fma(-ej, room, g);
        }
        if (lane == 0) st.xs[j] = nx;                                 // (xs[j] is read at step j only)
        if (g == 0.0) break;
      }
      if (ret == 2 && !is_finite(g)) ret = -1;
      if (ret == 2 && g != 0.0) ret = -2;
    }
    __syncthreads();
    for (int j = lane; j < n; j += WAVE) {
      if (ret != 2) st.xs[j] = fmin(fmax(0.0, st.lbs[j]), st.ubs[j]);
      const double x = st.xs[j];
      st.on[j] = x == st.lbs[j] ? -1 : (x == st.ubs[j] ? 1 : 0);
    }
    __syncthreads();
    return ret;
  }

  // Lt holds the factor of the free block: v into vs and registers, ev = e_F^T v -> false: ev <= 0 or not finite
  __device__ bool project(BvlsState& st, int k, double (&v)[2]) {
    for (int h = 0; h < 2; ++h) {
      const int i = st.lane + h * WAVE;
      v[h] = i < k ? es[st.fidx[i]] : 0.0;
    }
    const double e0 = v[0], e1 = v[1];
    st.tri_solve(k, v[0], v[1]);
    ev = dot2(e0, v[0], e1, v[1]);
    for (int h = 0; h < 2; ++h)
      if (st.lane + h * WAVE < k) vs[st.lane + h * WAVE] = v[h];
    __syncthreads();
    return ev > 0.0 && is_finite(ev);
  }

  // zs[f_i] = z_F = u - lambda v (a free set of one variable j: (d - e_B^T x_B) / e_j clamped into its box); lam_z = lambda
  // false: not positive definite, e_F^T v <= 0, or a value not finite
  __device__ bool solve(BvlsState& st, int k) {
    if (!st.factor(k)) return false;
    const int n = st.n, lane = st.lane;
    double u[2], v[2], e[2];
    for (int h = 0; h < 2; ++h) {
      const int i = lane + h * WAVE;
      double acc = 0.0, ei = 0.0;
      if (i < k) {
        const int fi = st.fidx[i];
        acc = st.c[fi];
        for (int j = 0; j < n; ++j)
          if (st.on[j] != 0) acc = fma(-st.G[(long)j * n + fi], st.xs[j], acc);
        ei = es[fi];
      }
      u[h] = acc;
      v[h] = e[h] = ei;
    }
    st.tri_solve2(k, u[0], u[1], v[0], v[1]);
    const double dF = gap<true>(st);
    const double eu = dot2(e[0], u[0], e[1], u[1]);
    ev = dot2(e[0], v[0], e[1], v[1]);
    if (!(ev > 0.0) || !is_finite(ev)) return false;
    const double l = (eu - dF) / ev;
    bool bad = !is_finite(l);
    for (int h = 0; h < 2; ++h) {
      const int i = lane + h * WAVE;
      if (i < k) {
        const int fi = st.fidx[i];
        double z = fma(-l, v[h], u[h]);
        bad |= !is_finite(z);
        if (k == 1) z = fmin(fmax(dF / e[h], st.lbs[fi]), st.ubs[fi]);
        st.zs[fi] = z;
        vs[i] = v[h];
      }
    }
    __syncthreads();
    lam_z = l;
    return !__any(bad);
  }

  // The first pass: a drop loop with nothing released, so without the bars and the zero-step end of the kernel's own;
  // the ratio test, the clamp and the exact bound values are those.  At most n + 1 rounds.
  __device__ void first_pass(BvlsState& st, int& k, int& nfact, int& status, bool& valid) {
    const int n = st.n, lane = st.lane;
    for (int round = 0; round <= n; ++round) {
      k = st.build_free();
      if (k == 0) return;
      ++nfact;
      if (!solve(st, k)) { status = -1; return; }
      double abest = INFINITY;
      int ibest = INT_MAX;
      for (int j = lane; j < n; j += WAVE) {
        if (st.on[j] != 0) continue;
        const double z = st.zs[j], x = st.xs[j];
        double bound;
        if (z < st.lbs[j]) bound = st.lbs[j];
        else if (z > st.ubs[j]) bound = st.ubs[j];
        else continue;
        const double a = (bound - x) / (z - x);
        if (ibest == INT_MAX || a < abest) { abest = a; ibest = j; }
      }
      if (!__any(ibest != INT_MAX)) {             // accepted
        for (int j = lane; j < n; j += WAVE)
          if (st.on[j] == 0) st.xs[j] = st.zs[j];
        __syncthreads();
        lam = lam_z;
        valid = true;
        return;
      }
      const double amin = wave_min(abest);
      const int id = wave_min_int((ibest != INT_MAX && abest == amin) ? ibest : INT_MAX);
      if (id == INT_MAX) { status = -1; return; }
      const double al = fmin(fmax(amin, 0.0), 1.0);
      for (int j = lane; j < n; j += WAVE) {
        if (st.on[j] != 0) continue;
        const double x = st.xs[j];
        st.xs[j] = fmin(fmax(x + al * (st.zs[j] - x), st.lbs[j]), st.ubs[j]);
      }
      __syncthreads();
      if (lane == 0) {
        const bool low = st.zs[id] < st.lbs[id];
        st.on[id] = low ? -1 : 1;
        st.xs[id] = low ? st.lbs[id] : st.ubs[id];
      }
      __syncthreads();
    }
    status = -1;                                  // (unreachable: every round removes a variable)
  }

  // every variable is on a bound: the interval [lo, hi] of the multipliers no bound variable objects to (from gs)
  __device__ void interval(const BvlsState& st, double& lo, double& hi) const {
    lo = -INFINITY;
    hi = INFINITY;
    for (int j = st.lane; j < st.n; j += WAVE) {
      if (st.on[j] == 0) continue;
      const double q = -st.gs[j] / es[j];
      if ((double)st.on[j] * es[j] > 0.0) hi = fmin(hi, q);
      else lo = fmax(lo, q);
    }
    lo = wave_max(lo);
    hi = wave_min(hi);
  }

  __device__ bool any_free(const BvlsState& st) const {
    bool fr = false;
    for (int j = st.lane; j < st.n; j += WAVE) fr |= st.on[j] == 0;
    return __any(fr);
  }

  // the multiplier reported, from gs: -e_F^T g_F / e_F^T e_F; F empty: the midpoint of the interval, or its finite end
  __device__ double multiplier(const BvlsState& st) const {
    if (any_free(st)) {
      double e[2] = {0.0, 0.0}, g[2] = {0.0, 0.0};
      for (int h = 0; h < 2; ++h) {
        const int j = st.lane + h * WAVE;
        if (j < st.n && st.on[j] == 0) { e[h] = es[j]; g[h] = st.gs[j]; }
      }
      return -dot2(e[0], g[0], e[1], g[1]) / dot2(e[0], e[0], e[1], e[1]);
    }
    double lo, hi;
    interval(st, lo, hi);
    if (is_finite(lo) && is_finite(hi)) return 0.5 * (lo + hi);
    return is_finite(lo) ? lo : (is_finite(hi) ? hi : 0.0);
  }

  // max(max over free |g_j + l e_j|, max over bound (g_j + l e_j) on_j, 0) of gs
  __device__ double optimality(const BvlsState& st, double l) const {
    double v = 0.0;
    for (int j = st.lane; j < st.n; j += WAVE) {
      const double r = fma(l, es[j], st.gs[j]);
      v = nanmax2(v, st.on[j] == 0 ? fabs(r) : r * (double)st.on[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax2(v, __shfl_xor(v, o, WAVE));
    return v;
  }
};

// One pass over the rows of A with x = st.xs:  f_i = w_i (sum_j A_ij x_j - y_i), u_i = (CORRECT ? -w_i : w_i) f_i,
// st.ts[j] = sum_i A_ij u_i; FINAL (not CORRECT) also writes fun (where given) and returns sum f_i^2.  A row belongs to
// a group of Gs = 2^lg lanes (Gs >= min(n, 64)): coalesced along j; lane g of the group runs fma(A_ij, x_j, .) over
// j = g, g + 64 from +0.0 and the butterfly o = Gs / 2 .. 1 adds the partial sums, as linear_f_kernel does.  The
// column sums run over a lane's rows in ascending order, then over the 64 / Gs row groups by the butterfly o = Gs .. 32.
template <bool CORRECT>
__device__ double bvls_a_pass(BvlsState& st, int m, int lg, const double* __restrict__ A, const double* __restrict__ y,
                              const double* __restrict__ w, double* __restrict__ fun) {
  const int n = st.n, lane = st.lane;
  const int Gs = 1 << lg, R = WAVE >> lg, g = lane & (Gs - 1), r = lane >> lg;
  const bool h0 = g < n, h1 = g + WAVE < n;                          // (h1 only with Gs == 64)
  const double x0 = h0 ? st.xs[g] : 0.0, x1 = h1 ? st.xs[g + WAVE] : 0.0;
  double t0 = 0.0, t1 = 0.0, ss = 0.0;
  for (int ib = 0; ib < m; ib += R) {                                // (the same trip count for every lane)
    const int i = ib + r;
    const bool in = i < m;
    const double a0 = (in && h0) ? A[(long)i * n + g] : 0.0;
    const double a1 = (in && h1) ? A[(long)i * n + g + WAVE] : 0.0;
    double acc = fma(a1, x1, fma(a0, x0, 0.0));
    for (int o = Gs >> 1; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, WAVE);
    if (!in) continue;
    const double wi = w ? w[i] : 1.0;
    const double f = wi * (acc - y[i]);
    if (!CORRECT && g == 0) {
      if (fun) fun[i] = f;
      ss = fma(f, f, ss);
    }
    const double u = CORRECT ? -(wi * f) : wi * f;
    t0 = fma(a0, u, t0);
    t1 = fma(a1, u, t1);
  }
  for (int o = Gs; o < WAVE; o <<= 1) {
    t0 = t0 + __shfl_xor(t0, o, WAVE);
    t1 = t1 + __shfl_xor(t1, o, WAVE);
  }
  __syncthreads();
  if (r == 0) {
    if (h0) st.ts[g] = t0;
    if (h1) st.ts[g + WAVE] = t1;
  }
  __syncthreads();
  return CORRECT ? 0.0 : wave_sum(ss);
}

template <bool EQ>
__global__ __launch_bounds__(BV_NT) void bvls_solve_kernel(BvlsSolveCall c, int lg, BvlsEqCall ec) {
  extern __shared__ __attribute__((aligned(16))) char bv_smem[];
  const int n = c.n, lane = threadIdx.x;
  const long b = blockIdx.x;
  const int tri = n * (n + 1) / 2;
  BvlsState st;
  st.n = n;
  st.lane = lane;
  st.G = c.G + b * c.G_stride;
  st.c = c.c + b * n;
  double* d = reinterpret_cast<double*>(bv_smem);
  st.Lt = d; d += tri;
  st.xs = d; d += n;
  st.zs = d; d += n;
  st.gs = d; d += n;
  st.lbs = d; d += n;
  st.ubs = d; d += n;
  st.ts = d; d += n;
  int* q = reinterpret_cast<int*>(d);
  st.fidx = q; q += n;
  st.on = q; q += n;
  st.barred = q;
  BvlsEq eq;
  if constexpr (EQ) {
    double* de = reinterpret_cast<double*>(q + n + (n & 1));          // (8-byte aligned behind the three int vectors)
    eq.es = de;
    eq.vs = de + n;
    eq.d = ec.d[b];
    eq.lam = 0.0;
    eq.ev = 0.0;
    for (int j = lane; j < n; j += WAVE) eq.es[j] = ec.e[b * ec.e_stride + j];
  }

  for (int j = lane; j < n; j += WAVE) {
    const double lo = c.lb[b * n + j], hi = c.ub[b * n + j];
    st.lbs[j] = lo;
    st.ubs[j] = hi;
    st.xs[j] = fmin(fmax(0.0, lo), hi);
    st.zs[j] = 0.0;
    st.on[j] = 0;
    st.barred[j] = 0;
  }
  __syncthreads();

  int status = 2, nit = 0, nfact = 0;             // 2: running
  bool valid = false;                             // Lt holds the factor of the current free block
  int k = 0;

  // (1) clip-in start; under the equality the feasible start, and a first pass that is a drop loop with no release
  if constexpr (EQ) {
    const int ret = eq.feasible_start(st);
    if (ret != 2) status = ret;
    else eq.first_pass(st, k, nfact, status, valid);
  }
  for (int it = 0; !EQ && it <= n; ++it) {
    k = st.build_free();
    if (k == 0) break;
    ++nfact;
    if (!st.solve(k)) { status = -1; break; }
    bool moved = false;
    for (int j = lane; j < n; j += WAVE) {
      if (st.on[j] != 0) continue;
      const double z = st.zs[j];
      if (z < st.lbs[j]) { st.on[j] = -1; st.xs[j] = st.lbs[j]; moved = true; }
      else if (z > st.ubs[j]) { st.on[j] = 1; st.xs[j] = st.ubs[j]; moved = true; }
      else st.xs[j] = z;
    }
    __syncthreads();
    if (!__any(moved)) { valid = true; break; }
  }

  // (2) release passes
  while (status == 2) {
    if (!st.gradient()) { status = -1; break; }
    double lam = 0.0;                             // (EQ) the multiplier the release test reads
    if constexpr (EQ) {
      lam = eq.lam;
      if (!eq.any_free(st)) {
        double lo, hi;
        eq.interval(st, lo, hi);
        if (lo <= hi + c.tol) { status = 1; break; }
        lam = 0.5 * (lo + hi);
      }
    }
    // the variable that wants to leave its bound most, of those not barred; when none of them does, the bars are
    // cleared and the barred ones are asked again: status 1 means that NO variable on a bound wants to leave it
    double vmax = -INFINITY;
    int jr = INT_MAX;
    for (int ask = 0; ask < 2; ++ask) {
      double vbest = -INFINITY;
      int jbest = INT_MAX;
      bool any_barred = false;
      for (int j = lane; j < n; j += WAVE) {
        if (st.on[j] == 0) continue;
        if (st.barred[j]) { any_barred = true; continue; }
        double v;
        if constexpr (EQ) v = fma(lam, eq.es[j], st.gs[j]) * (double)st.on[j];
        else v = st.gs[j] * (double)st.on[j];
        if (jbest == INT_MAX || v > vbest) { vbest = v; jbest = j; }
      }
      vmax = wave_max(vbest);
      jr = wave_min_int((jbest != INT_MAX && vbest == vmax) ? jbest : INT_MAX);
      if ((jr != INT_MAX && vmax > c.tol) || !__any(any_barred)) break;
      __syncthreads();
      for (int j = lane; j < n; j += WAVE) st.barred[j] = 0;
      __syncthreads();
    }
    if (jr == INT_MAX || !(vmax > c.tol)) { status = 1; break; }
    if (nit >= c.max_pass) { status = 0; break; }
    ++nit;
    __syncthreads();
    const int left = st.on[jr];
    __syncthreads();
    if (lane == 0) st.on[jr] = 0;
    __syncthreads();
    valid = false;
    bool first = true, ended = false;
    // (3) drop loop
    for (int round = 0; round <= n && !ended; ++round) {
      k = st.build_free();
      if (k == 0) {
        for (int j = lane; j < n; j += WAVE) st.barred[j] = 0;
        __syncthreads();
        ended = true;
        break;
      }
      ++nfact;
      if constexpr (EQ) {
        if (!eq.solve(st, k)) { status = -1; break; }
      } else {
        if (!st.solve(k)) { status = -1; break; }
      }
      double abest = INFINITY;
      int ibest = INT_MAX;
      for (int j = lane; j < n; j += WAVE) {
        if (st.on[j] != 0) continue;
        const double z = st.zs[j], x = st.xs[j];
        double bound;
        if (z < st.lbs[j]) bound = st.lbs[j];
        else if (z > st.ubs[j]) bound = st.ubs[j];
        else continue;
        const double a = (bound - x) / (z - x);
        if (ibest == INT_MAX || a < abest) { abest = a; ibest = j; }
      }
      if (!__any(ibest != INT_MAX)) {             // accepted
        for (int j = lane; j < n; j += WAVE) {
          if (st.on[j] == 0) st.xs[j] = st.zs[j];
          st.barred[j] = 0;
        }
        __syncthreads();
        if constexpr (EQ) eq.lam = eq.lam_z;
        valid = true;
        ended = true;
        break;
      }
      const double amin = wave_min(abest);
      const int id = wave_min_int((ibest != INT_MAX && abest == amin) ? ibest : INT_MAX);
      if (id == INT_MAX) { status = -1; break; }  // (a ratio that is not a number)
      const double al = fmin(fmax(amin, 0.0), 1.0);
      for (int j = lane; j < n; j += WAVE) {
        if (st.on[j] != 0) continue;
        const double x = st.xs[j];
        st.xs[j] = fmin(fmax(x + al * (st.zs[j] - x), st.lbs[j]), st.ubs[j]);
      }
      __syncthreads();
      if (lane == 0) {
        const bool low = st.zs[id] < st.lbs[id];
        st.on[id] = low ? -1 : 1;
        st.xs[id] = low ? st.lbs[id] : st.ubs[id];
        if (first && id == jr) st.barred[jr] = 1;
      }
      __syncthreads();
      // the released variable dropped first is barred; back on the bound it left with a zero step, x and F are those
      // before the pass, which ends here (a further solve would accept and clear the bar at once)
      if (first && id == jr && al == 0.0 && st.on[jr] == left) ended = true;
      first = false;
    }
    if (status == 2 && !ended) status = -1;       // (unreachable: every round removes a variable)
  }

  double cost = 0.0, opt;
  if (c.A) {
    const double* A = c.A + b * c.A_stride;
    const double* y = c.y + b * (long)c.m;
    const double* w = c.w ? c.w + b * c.w_stride : nullptr;
    // one corrected-semi-normal-equations step on the final free block: x_F += (G_FF)^-1 A_F^T W^2 (y - A x)
    if constexpr (EQ) {
      // under the equality the step is projected: with t = A^T W^2 (y - A x), s = (G_FF)^-1 t_F and the v of this free
      // block, x_F += s - mu v, mu = (e_F^T s - (d - e^T x)) / (e_F^T v): the sum is restored as well
      if (status >= 0) {
        bool ok = valid;
        double v[2];
        if (valid) {
          v[0] = lane < k ? eq.vs[lane] : 0.0;
          v[1] = lane + WAVE < k ? eq.vs[lane + WAVE] : 0.0;
        } else {
          k = st.build_free();
          if (k > 0) {
            ++nfact;
            ok = st.factor(k) && eq.project(st, k, v);
          }
        }
        if (ok && k > 0) {
          bvls_a_pass<true>(st, c.m, lg, A, y, w, nullptr);
          double s0 = lane < k ? st.ts[st.fidx[lane]] : 0.0;
          double s1 = lane + WAVE < k ? st.ts[st.fidx[lane + WAVE]] : 0.0;
          const double e0 = lane < k ? eq.es[st.fidx[lane]] : 0.0;
          const double e1 = lane + WAVE < k ? eq.es[st.fidx[lane + WAVE]] : 0.0;
          st.tri_solve(k, s0, s1);
          const double mu = (BvlsEq::dot2(e0, s0, e1, s1) - eq.template gap<false>(st)) / eq.ev;
          s0 = fma(-mu, v[0], s0);
          s1 = fma(-mu, v[1], s1);
          const bool fin = !__any((lane < k && !is_finite(s0)) || (lane + WAVE < k && !is_finite(s1)));
          if (fin) {                              // (a correction that is not finite is not applied)
            for (int h = 0; h < 2; ++h) {
              const int i = lane + h * WAVE;
              if (i >= k) continue;
              const int j = st.fidx[i];
              st.xs[j] = fmin(fmax(st.xs[j] + (h ? s1 : s0), st.lbs[j]), st.ubs[j]);
            }
          }
          __syncthreads();
        }
      }
    } else if (status != -1) {
      bool ok = valid;
      if (!valid) {
        k = st.build_free();
        if (k > 0) {
          ++nfact;
          ok = st.factor(k);
        }
      }
      if (ok && k > 0) {
        bvls_a_pass<true>(st, c.m, lg, A, y, w, nullptr);
        double v0 = lane < k ? st.ts[st.fidx[lane]] : 0.0;
        double v1 = lane + WAVE < k ? st.ts[st.fidx[lane + WAVE]] : 0.0;
        st.tri_solve(k, v0, v1);
        const bool fin = !__any((lane < k && !is_finite(v0)) || (lane + WAVE < k && !is_finite(v1)));
        if (fin) {                                // (a correction that is not finite is not applied)
          for (int h = 0; h < 2; ++h) {
            const int i = lane + h * WAVE;
            if (i >= k) continue;
            const int j = st.fidx[i];
            st.xs[j] = fmin(fmax(st.xs[j] + (h ? v1 : v0), st.lbs[j]), st.ubs[j]);
          }
        }
        __syncthreads();
      }
    }
    const double ss = bvls_a_pass<false>(st, c.m, lg, A, y, w, c.fun ? c.fun + b * (long)c.m : nullptr);
    cost = 0.5 * ss;
    for (int j = lane; j < n; j += WAVE) st.gs[j] = st.ts[j];
    __syncthreads();
  } else {
    st.gradient();
  }
  double mult = 0.0;
  if constexpr (EQ) {
    mult = eq.multiplier(st);
    opt = eq.optimality(st, mult);
  } else {
    opt = st.optimality();
  }
  for (int j = lane; j < n; j += WAVE) {
    c.x[b * n + j] = st.xs[j];
    c.on_bound[b * n + j] = st.on[j];
    c.grad[b * n + j] = st.gs[j];
  }
  if (lane == 0) {
    c.opt[2 * b] = opt;
    c.opt[2 * b + 1] = cost;
    c.stat[3 * b] = status;
    c.stat[3 * b + 1] = nit;
    c.stat[3 * b + 2] = nfact;
    if constexpr (EQ) ec.multiplier[b] = mult;
  }
}

size_t bvls_solve_lds_bytes(int n, bool eq) {
  const size_t base = sizeof(double) * ((size_t)n * (n + 1) / 2 + 6 * (size_t)n) + sizeof(int) * 3 * (size_t)n;
  return eq ? base + sizeof(int) * (size_t)(n & 1) + sizeof(double) * 2 * (size_t)n : base;
}

static hipError_t checked_solve_call(const BvlsSolveCall& c) {
  if (c.B < 1 || c.n < 1 || c.n > BLSQ_BVLS_MAX_N || c.max_pass < 0) return hipErrorInvalidValue;
  if (!c.G || !c.c || !c.lb || !c.ub || !c.x || !c.on_bound || !c.grad || !c.opt || !c.stat) return hipErrorInvalidValue;
  if (c.G_stride != 0 && c.G_stride != (long)c.n * c.n) return hipErrorInvalidValue;
  if (c.A) {
    if (c.m < 1 || !c.y) return hipErrorInvalidValue;
    if (c.A_stride != 0 && c.A_stride != (long)c.m * c.n) return hipErrorInvalidValue;
    if (c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  } else if (c.fun) {
    return hipErrorInvalidValue;
  }
  return hipSuccess;
}

static int group_log2(int n) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < n) ++lg;
  return lg;
}

hipError_t launch_bvls_solve(const BvlsSolveCall& c, hipStream_t s) {
  const hipError_t e = checked_solve_call(c);
  if (e != hipSuccess) return e;
  return launch<bvls_solve_kernel<false>>(dim3((unsigned)c.B), dim3(BV_NT), bvls_solve_lds_bytes(c.n, false), s, c,
                                          group_log2(c.n), BvlsEqCall{nullptr, 0, nullptr, nullptr});
}

hipError_t launch_bvls_solve_eq(const BvlsSolveCall& c, const BvlsEqCall& q, hipStream_t s) {
  const hipError_t e = checked_solve_call(c);
  if (e != hipSuccess) return e;
  if (!q.e || !q.d || !q.multiplier || (q.e_stride != 0 && q.e_stride != (long)c.n)) return hipErrorInvalidValue;
  return launch<bvls_solve_kernel<true>>(dim3((unsigned)c.B), dim3(BV_NT), bvls_solve_lds_bytes(c.n, true), s, c,
                                         group_log2(c.n), q);
}

}  // namespace blsq
