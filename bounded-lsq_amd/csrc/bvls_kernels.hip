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

__global__ __launch_bounds__(BV_NT) void bvls_solve_kernel(BvlsSolveCall c, int lg) {
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

  // (1) clip-in start
  for (int it = 0; it <= n; ++it) {
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
        const double v = st.gs[j] * (double)st.on[j];
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
      if (!st.solve(k)) { status = -1; break; }
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
    if (status != -1) {
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
  opt = st.optimality();
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
  }
}

size_t bvls_solve_lds_bytes(int n) {
  return sizeof(double) * ((size_t)n * (n + 1) / 2 + 6 * (size_t)n) + sizeof(int) * 3 * (size_t)n;
}

hipError_t launch_bvls_solve(const BvlsSolveCall& c, hipStream_t s) {
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
  int lg = 0;
  while (lg < 6 && (1 << lg) < c.n) ++lg;
  return launch<bvls_solve_kernel>(dim3((unsigned)c.B), dim3(BV_NT), bvls_solve_lds_bytes(c.n), s, c, lg);
}

}  // namespace blsq
