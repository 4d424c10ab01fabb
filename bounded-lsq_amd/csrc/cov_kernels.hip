// Parameter covariance from the final Jacobian (blsq_cov*, blsq_outer_covariance).
//
// C = (J^T J)^-1 = R^-1 R^-T with R the Householder triangle of J (the TSQR tree, qr_panel.hip: a Gram-Cholesky
// triangle squares the conditioning and is not used here).  With a mask of active variables the free columns of J are
// moved to the front first: the leading nfree x nfree block of the triangle of the permuted matrix is the triangle
// of J_F, and C is scattered back through the permutation with zeros in the rows and columns of active variables.
//
//   cov_perm_kernel      perm [B][n] (free columns first, both groups in ascending order) and nfree [B] from the
//                        int64 mask; cov_trf_mask_kernel: the mask of a TRF driver from its x (find_active_constraints)
//   cov_gather_kernel    one streaming pass: Jp[r][c] = J[r][perm[c]].  Row-chunk grid as loss_scale_kernel (one tall
//                        problem fills the chip), 16-byte stores where n is even
//   cov_inverse_kernel   one workgroup per problem: pivot test and ||R||_1, then X = R^-1 by blocked back substitution
//                        over 16 x 16 tiles — all diagonal tiles first (one wave each, a lane per column, registers),
//                        then block column j = 1 .. NT-1:  X_ij = -(sum_{k=i}^{j-1} X_ik R_kj) X_jj, the tiles i < j
//                        dealt over the waves, every product on the FP64 MFMA pipe.  X lives in a plan-owned slot
//                        [NPAD][NPAD] per problem (L2-resident: n = 256 does not fit LDS).  ||X||_1, rcond_1 and the
//                        verdict follow; a singular problem's output is filled with NaN, a masked one's with zeros
//   cov_product_kernel   C_F = X X^T, tile (i, j >= i) = sum_{k >= j} X_ik X_jk^T on the MFMA pipe, written with its
//                        mirror image through perm: exactly symmetric by construction
//
// The pseudo-inverse route (blsq_cov_pinv*) replaces the last two by the one-sided Jacobi SVD of the
// triangle (jacobi_svd.hip: row i of the free block becomes s_i v_i^T) and
//   cov_pinv_weights_kernel  one workgroup per problem: sigma_max, curve_fit's threshold eps max(m, |F|) sigma_max, the
//                        rank, w_i = 1 / s_i^2 (exactly 0.0 for a dropped row), rcond = sigma_min / sigma_max,
//                        kept_rcond, the verdict and the NaN / zero fill of cov
//   cov_pinv_product_kernel  C_F = sum_i (w_i r_i)(w_i r_i)^T = Y^T Y with Y = diag(w) [rows]: tile (i, j >= i) summed
//                        over the rows in ascending order on the MFMA pipe (operands read along the rows, the weight
//                        applied on the load), times an optional per-problem scale, written with its mirror image
//
//
// Row forms through the factor either route leaves behind (blsq_cov_rows*):
//   cov_rows_kernel      out[i] = scale |a_i[F] X|^2 (regular) or scale sum_k (w_k r_k . a_i[F])^2 (pinv) for every row of
//                        an [rows][n] matrix: leverages h_i = (J C J^T)_ii and prediction variances diag(A C A^T)
//                        without forming C.  Row-chunk grid, a wave per 16 rows, the products on the MFMA pipe
//
// cov_product_kernel, cov_pinv_product_kernel, cov_pinv_rowgram_kernel and cov_pinv_rowfactor_kernel are instances of one
// skeleton: the CovTile prologue (cov_tile) and the loop nest cov_tile_product, parameterised by the two operand
// loaders, the start of j and of k and the epilogue; the two *_product kernels share the symmetric scatter through perm
// (cov_scatter_sym).  cov_rows_kernel and the MFMA loops inside cov_inverse_kernel have another nest and their own code.
// Workgroup maxima, minima and the rank count are block_max / block_min / block_sum_int of blsq_device.h.
//
// Every sum has a fixed order and nothing is atomic: a problem's bits depend on its own J, mask, m and n only.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"

namespace blsq {

static constexpr int COV_NT = 512;
static constexpr int COV_NW = COV_NT / WAVE;
static constexpr int COV_PNT = 256;               // product kernel: four waves, one output tile each at a time
static constexpr int COV_PNW = COV_PNT / WAVE;
static constexpr int COV_GNT = 256;
static constexpr int COV_TARGET_ELEMS = 8192;     // J doubles per gather workgroup

// ---- masks and permutations --------------------------------------------------------------------
__global__ __launch_bounds__(256) void cov_perm_kernel(int B, int n, const long long* __restrict__ active, int lda,
                                                       int* __restrict__ perm, int* __restrict__ nfree,
                                                       int* __restrict__ ncols) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long* a = active + (long)b * lda;
  int* p = perm + (long)b * n;
  int k = 0;
  for (int j = 0; j < n; ++j)
    if (a[j] == 0) p[k++] = j;
  nfree[b] = k;
  if (ncols) ncols[b] = k + 1;                       // (the Jacobi kernel's per-problem width: free block + carried column)
  for (int j = 0; j < n; ++j)
    if (a[j] != 0) p[k++] = j;
}

// bounds.py:51-76 (find_active_constraints) with rtol, as the host drivers report it for 'trf'
__global__ __launch_bounds__(256) void cov_trf_mask_kernel(int B, int n, int ld, double rtol,
                                                           const double* __restrict__ x, const double* __restrict__ lb,
                                                           const double* __restrict__ ub, long long* __restrict__ mask) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * n) return;
  const int b = (int)(idx / n), j = (int)(idx - (long)b * n);
  const double xv = x[idx], l = lb[(long)b * ld + j], u = ub[(long)b * ld + j];
  const double dl = xv - l, du = u - xv;
  const bool lower_nearer = dl < du;
  const bool on_l = dl < rtol * fmax(1.0, fabs(l));
  const bool on_u = du < rtol * fmax(1.0, fabs(u));
  long long v = 0;
  if (lower_nearer && on_l) v = -1;
  if (!lower_nearer && on_u) v = 1;
  mask[idx] = v;
}

// ---- gather ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(COV_GNT) void cov_gather_kernel(int m, int n, int rows, int chunks,
                                                             const double* __restrict__ J,
                                                             const int* __restrict__ perm, double* __restrict__ Jp) {
  extern __shared__ int psh[];                       // [n]
  const int b = blockIdx.x / chunks, r0 = (blockIdx.x - b * chunks) * rows, tid = threadIdx.x;
  const int nr = min(rows, m - r0);
  for (int j = tid; j < n; j += COV_GNT) psh[j] = perm[(long)b * n + j];
  __syncthreads();
  const long base = ((long)b * m + r0) * n;
  const double* src = J + base;
  const unsigned un = (unsigned)n;
  if (VEC) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    v2d* dst = reinterpret_cast<v2d*>(Jp + base);
    const int L = (nr * n) >> 1;
    for (int k = tid; k < L; k += COV_GNT) {
      const unsigned e = 2u * (unsigned)k, r = e / un, c = e - r * un;   // (n even: c and c + 1 are in one row)
      v2d v;
      v.x = src[r * un + (unsigned)psh[c]];
      v.y = src[r * un + (unsigned)psh[c + 1]];
      dst[k] = v;
    }
  } else {
    double* dst = Jp + base;
    const int L = nr * n;
    for (int k = tid; k < L; k += COV_GNT) {
      const unsigned r = (unsigned)k / un, c = (unsigned)k - r * un;
      dst[k] = src[r * un + (unsigned)psh[c]];
    }
  }
}

// rows [r0, r0 + c) of J under the triangle of the stack (sequential fold of a plan past the tree's merge capacity)
__global__ __launch_bounds__(COV_GNT) void cov_stack_kernel(int m, int n, int r0, int c, const double* __restrict__ J,
                                                            double* __restrict__ S, int srows, int ld) {
  const int b = blockIdx.y, i = blockIdx.x;          // i < c
  const double* src = J + ((long)b * m + r0 + i) * n;
  double* dst = S + ((long)b * srows + ld + i) * ld;
  for (int j = threadIdx.x; j < n; j += COV_GNT) dst[j] = src[j];
}

// ---- inverse -----------------------------------------------------------------------------------
// column sums of |T| over the leading nf x nf upper triangle (thread per column, rows in ascending order)
__device__ __forceinline__ double cov_norm1_part(const double* T, int ld, int nf, int* bad) {
  double best = 0.0;
  for (int c = threadIdx.x; c < nf; c += COV_NT) {
    double s = 0.0;
    for (int r = 0; r <= c; ++r) s += fabs(T[(long)r * ld + c]);
    if (!is_finite(s)) *bad = 1;
    best = fmax(best, s);
  }
  return best;
}

__device__ __forceinline__ void cov_fill(double* C, long count, double v) {
  for (long k = threadIdx.x; k < count; k += COV_NT) C[k] = v;
}

__global__ __launch_bounds__(COV_NT) void cov_inverse_kernel(int m, int n, int NPAD, const double* __restrict__ Rall,
                                                             double* Xall, const int* __restrict__ nfree,
                                                             double* __restrict__ cov, double* __restrict__ rcond,
                                                             int* __restrict__ status) {
  __shared__ double red[32];
  __shared__ double tsh[COV_NW][256];               // per wave: a staged tile (row-major)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nf = nfree ? nfree[b] : n;
  const int ld = NPAD;
  const double* R = Rall + (long)b * NPAD * NPAD;
  double* X = Xall + (long)b * NPAD * NPAD;
  double* C = cov + (long)b * n * n;
  const long nn = (long)n * n;
  if (nf == 0) {                                     // every variable on a bound: nothing to invert
    cov_fill(C, nn, 0.0);
    if (tid == 0) { rcond[b] = 1.0; status[b] = 0; }
    return;
  }
  // 1. pivots and ||R||_1
  int bad = 0;
  for (int c = tid; c < nf; c += COV_NT) {
    const double p = R[(long)c * ld + c];
    if (!(p != 0.0) || !is_finite(p)) bad = 1;
  }
  const double rpart = cov_norm1_part(R, ld, nf, &bad);
  bad = __syncthreads_or(bad);
  if (bad) {                                         // uniform
    cov_fill(C, nn, __builtin_nan(""));
    if (tid == 0) { rcond[b] = 0.0; status[b] = 1; }
    return;
  }
  const double rnorm = block_max(rpart, red);
  const int NTl = (nf + 15) >> 4;                    // tiles of the free block (NTl * 16 <= NPAD: nf <= n < NPAD)
  // R restricted to the free block and padded with the identity up to the tile edge
  auto ldR = [&](int r, int c) -> double {
    return (r < nf && c < nf) ? R[(long)r * ld + c] : ((r == c) ? 1.0 : 0.0);
  };
  const int lr = lane >> 4, lc = lane & 15;
  double* ts = tsh[w];
  // 2. diagonal tiles: X_jj = R_jj^-1, a wave per tile, lane c < 16 solves R_jj x = e_c in registers
  for (int j = w; j < NTl; j += COV_NW) {
    const int o = 16 * j;
#pragma unroll
    for (int q = 0; q < 4; ++q) ts[(lr + 4 * q) * 16 + lc] = ldR(o + lr + 4 * q, o + lc);
    __builtin_amdgcn_wave_barrier();
    double x[16];
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double s = (i == lc) ? 1.0 : 0.0;
#pragma unroll
      for (int k = i + 1; k < 16; ++k) s = fma(-ts[i * 16 + k], x[k], s);
      x[i] = s / ts[i * 16 + i];
    }
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < 16; ++i) X[(long)(o + i) * ld + o + lc] = (i <= lc) ? x[i] : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __threadfence_block();
  __syncthreads();
  // 3. block columns
  for (int j = 1; j < NTl; ++j) {
    for (int i = w; i < j; i += COV_NW) {
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int k = i; k < j; ++k) {                  // T = sum_k X_ik R_kj
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double a = X[(long)(16 * i + lc) * ld + 16 * k + 4 * q + lr];
          const double bb = ldR(16 * k + 4 * q + lr, 16 * j + lc);
          acc = mfma_f64(a, bb, acc);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) ts[(lr + 4 * g) * 16 + lc] = acc[g];
      __builtin_amdgcn_wave_barrier();
      v4d out = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) {                  // X_ij = -T X_jj
        const double a = ts[lc * 16 + 4 * q + lr];
        const double bb = X[(long)(16 * j + 4 * q + lr) * ld + 16 * j + lc];
        out = mfma_f64(a, bb, out);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) X[(long)(16 * i + lr + 4 * g) * ld + 16 * j + lc] = -out[g];
      __builtin_amdgcn_wave_barrier();
    }
    __threadfence_block();
    __syncthreads();
  }
  // 4. ||X||_1, rcond_1, verdict
  int xbad = 0;
  const double xpart = cov_norm1_part(X, ld, nf, &xbad);
  xbad = __syncthreads_or(xbad);
  const double xnorm = block_max(xpart, red);
  double rc = 0.0;
  if (!xbad) rc = 1.0 / (rnorm * xnorm);
  const double thresh = DBL_EPS * (double)(m > nf ? m : nf);
  const int sing = !(rc >= thresh);
  if (tid == 0) { rcond[b] = rc; status[b] = sing; }
  if (sing) cov_fill(C, nn, __builtin_nan(""));
  else if (nf < n) cov_fill(C, nn, 0.0);
}

// ---- 16 x 16 tile products ------------------------------------------------------------------------
// The covariance tail's four tile-product kernels are one skeleton: workgroup (i, b) owns tile row i of problem b, its
// four waves stride the tile columns j, k runs over tiles, four MFMAs of a k-step go into one accumulator.  A kernel is
// its two operand loaders, the start of j and of k, and what it does with a finished tile.
struct CovTile { int b, i, w, lr, lc, nf, NTl; };
// false: nothing to do, the caller returns (uniform) — the inverse / weights kernel has filled the output of a problem
// whose status is not 0, and tile rows past the free block do not exist
__device__ __forceinline__ bool cov_tile(CovTile& t, int n, const int* __restrict__ nfree,
                                         const int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  t.i = blockIdx.x; t.b = blockIdx.y;
  t.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (status[t.b] != 0) return false;
  t.nf = nfree ? nfree[t.b] : n;
  t.NTl = (t.nf + 15) >> 4;
  if (t.i >= t.NTl) return false;
  t.lr = lane >> 4; t.lc = lane & 15;
  return true;
}
// la(k, q) / lb(j, k, q): this lane's A[lc][4 q + lr] and B[4 q + lr][lc] of k-tile k;  k0(j): the first k-tile of
// column j;  store(j, acc): rows lr + 4 g, column lc of the finished tile (i, j).  Sums run over k, then q, ascending.
template <class LoadA, class LoadB, class K0, class Store>
__device__ __forceinline__ void cov_tile_product(const CovTile& t, int j0, K0 k0, LoadA la, LoadB lb, Store store) {
  for (int j = j0 + t.w; j < t.NTl; j += COV_PNW) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k = k0(j); k < t.NTl; ++k) {
      double a[4], bb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[q] = la(k, q); bb[q] = lb(j, k, q); }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = mfma_f64(a[q], bb[q], acc);
    }
    store(j, acc);
  }
}
// tile (i, j >= i) of the free block and its mirror image into C through perm: exactly symmetric by construction
template <bool SCALED>
__device__ __forceinline__ void cov_scatter_sym(const CovTile& t, int j, v4d acc, double sc, const int* pm, int n,
                                                double* C) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int r = 16 * t.i + t.lr + 4 * g, c = 16 * j + t.lc;
    if (r < t.nf && c < t.nf && r <= c) {            // (i < j: always r < c)
      const int pr = pm ? pm[r] : r, pc = pm ? pm[c] : c;
      double v = acc[g];
      if constexpr (SCALED) v *= sc;
      C[(long)pr * n + pc] = v;
      C[(long)pc * n + pr] = v;
    }
  }
}

// ---- product -----------------------------------------------------------------------------------
__global__ __launch_bounds__(COV_PNT) void cov_product_kernel(int n, int NPAD, const double* __restrict__ Xall,
                                                              const int* __restrict__ nfree,
                                                              const int* __restrict__ perm,
                                                              const int* __restrict__ status,
                                                              double* __restrict__ cov) {
  CovTile t;
  if (!cov_tile(t, n, nfree, status)) return;
  const int ld = NPAD;
  const double* X = Xall + (long)t.b * NPAD * NPAD;
  const int* pm = perm ? perm + (long)t.b * n : nullptr;
  double* C = cov + (long)t.b * n * n;
  cov_tile_product(t, t.i, [](int j) { return j; },
                   [&](int k, int q) { return X[(long)(16 * t.i + t.lc) * ld + t.lr + 16 * k + 4 * q]; },
                   [&](int j, int k, int q) { return X[(long)(16 * j + t.lc) * ld + t.lr + 16 * k + 4 * q]; },
                   [&](int j, v4d acc) { cov_scatter_sym<false>(t, j, acc, 1.0, pm, n, C); });
}

// ---- pseudo-inverse: weights and product ---------------------------------------------------------
// After launch_jacobi row i < nf of the triangle slot is s_i v_i^T and s[b][i] = s_i (unsorted).  The recipe restated
// (scipy 1.15.3 _minpack_py.py, curve_fit: "threshold = np.finfo(float).eps * max(jac.shape) * s[0]; s = s[s >
// threshold]; VT = VT[:s.size]; pcov = np.dot(VT.T / s**2, VT)"): status 0 ok, 1 not finite, 2 Jacobi not converged.
__global__ __launch_bounds__(COV_PNT) void cov_pinv_weights_kernel(int m, int n, int NPAD, const double* __restrict__ Xall,
                                                                   const double* __restrict__ sall,
                                                                   const int* __restrict__ sweeps, int max_sweeps,
                                                                   const int* __restrict__ nfree,
                                                                   double* __restrict__ wall, double* __restrict__ cov,
                                                                   int* __restrict__ rank, double* __restrict__ rcond,
                                                                   double* __restrict__ kept_rcond,
                                                                   int* __restrict__ status) {
  __shared__ double red[32];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nf = nfree ? nfree[b] : n;
  const int ld = NPAD;
  const double* X = Xall + (long)b * NPAD * NPAD;
  const double* s = sall + (long)b * ld;
  double* w = wall + (long)b * ld;
  double* C = cov + (long)b * n * n;
  const long nn = (long)n * n;
  auto fill = [&](double v) { for (long k = tid; k < nn; k += COV_PNT) C[k] = v; };
  if (nf == 0) {                                     // every variable on a bound
    fill(0.0);
    if (tid == 0) { rank[b] = 0; rcond[b] = 1.0; kept_rcond[b] = 1.0; status[b] = 0; }
    return;
  }
  // 1. non-finite singular values or rows (scipy's svd raises on them), a Jacobi run that used all its sweeps
  int bad = 0;
  for (int i = tid; i < nf; i += COV_PNT) if (!is_finite(s[i])) bad = 1;
  for (int k = tid; k < nf * nf; k += COV_PNT) {
    const int r = k / nf, c = k - r * nf;
    if (!is_finite(X[(long)r * ld + c])) bad = 1;
  }
  bad = __syncthreads_or(bad);
  const int stalled = sweeps[b] >= max_sweeps;
  if (bad || stalled) {                              // uniform
    fill(__builtin_nan(""));
    if (tid == 0) { rank[b] = 0; rcond[b] = 0.0; kept_rcond[b] = 0.0; status[b] = bad ? 1 : 2; }
    return;
  }
  // 2. sigma_max, sigma_min
  double mx = 0.0, mn = __builtin_inf();
  for (int i = tid; i < nf; i += COV_PNT) { mx = fmax(mx, s[i]); mn = fmin(mn, s[i]); }
  const double smax = block_max(mx, red);
  const double smin = block_min(mn, red);
  // 3. threshold, rank, weights, smallest kept value
  const double thresh = DBL_EPS * (double)(m > nf ? m : nf) * smax;
  int cnt = 0;
  double kmn = __builtin_inf();
  const int nrow = ((nf + 15) >> 4) << 4;            // (<= NPAD: nf <= n < NPAD)
  for (int i = tid; i < nrow; i += COV_PNT) {
    double wi = 0.0;
    if (i < nf && s[i] > thresh) { wi = 1.0 / (s[i] * s[i]); ++cnt; kmn = fmin(kmn, s[i]); }
    w[i] = wi;
  }
  const double kmin = block_min(kmn, red);
  const int rk = block_sum_int(cnt, red);
  if (tid == 0) {
    rank[b] = rk;
    rcond[b] = smax > 0.0 ? smin / smax : 0.0;
    kept_rcond[b] = rk > 0 ? kmin / smax : 0.0;
    status[b] = 0;
  }
  if (nf < n) fill(0.0);                             // (the product launch writes the whole free block)
}

__global__ __launch_bounds__(COV_PNT) void cov_pinv_product_kernel(int n, int NPAD, const double* __restrict__ Xall,
                                                                   const double* __restrict__ wall,
                                                                   const int* __restrict__ nfree,
                                                                   const int* __restrict__ perm,
                                                                   const int* __restrict__ status,
                                                                   const double* __restrict__ dscale,
                                                                   double* __restrict__ cov) {
  CovTile t;
  if (!cov_tile(t, n, nfree, status)) return;
  const int ld = NPAD;
  const double* X = Xall + (long)t.b * NPAD * NPAD;
  const double* wt = wall + (long)t.b * ld;
  const int* pm = perm ? perm + (long)t.b * n : nullptr;
  double* C = cov + (long)t.b * n * n;
  const double sc = dscale ? dscale[t.b] : 1.0;
  // rows 16 k .. 16 k + 15 of Y = diag(w) [rows], ascending; lanes of one lr: 16 consecutive doubles of a row
  // (rows >= nf of a masked problem belong to its active columns)
  auto ldY = [&](int ct, int k, int q) {
    const int r = 16 * k + 4 * q + t.lr;
    const double v = X[(long)r * ld + 16 * ct + t.lc] * wt[r];
    return (r < t.nf) ? v : 0.0;
  };
  cov_tile_product(t, t.i, [](int) { return 0; },
                   [&](int k, int q) { return ldY(t.i, k, q); },
                   [&](int j, int k, int q) { return ldY(j, k, q); },
                   [&](int j, v4d acc) { cov_scatter_sym<true>(t, j, acc, sc, pm, n, C); });
}

// ---- row forms through the kept factor (7i) ------------------------------------------------------
// out[b][i] = scale[b] sum_k t_ik^2 for every row a_i of A [B][rows][n]:  regular route t_i = a_i[F] X (X upper
// triangular, so output tile j sums the tiles k <= j only), pinv route t_ik = w_k (row k of the rotated triangle) . a_i[F].
// One workgroup per 64 rows of one problem, a wave per 16 rows; A is read through perm (staged in LDS) on the load, the
// factor tile by tile from L2.  A wave accumulates COV_RJB output tiles at a time so that an A operand is loaded once per
// block of tiles; every tile's sum runs over k in ascending order, the squares are added tile by tile in ascending
// order, and one xor tree over the 16 lanes of a row group finishes a row: its bits depend on the row, the factor,
// and nothing else.  Outside the leading nf x nf block the X slot holds the identity padding of the last tile and
// whatever an earlier call with more free variables left, so both operands are masked to r, c < nf.
// The pinv route's factor for the row forms.  The Jacobi SVD stops rotating a pair of rows once their cosine is below
// sqrt(n) eps, so the rows W = (s_k v_k^T) are orthogonal to ~16 eps only, and t = diag(w) W a — exact for orthogonal
// rows — misses  a^T (W^T W)^-1 a = |M^-1 W a|^2, M = W W^T,  by that cosine times the ratio of the components it couples
// (measured: 1.9 x the test bound at 1030 x 272, kappa 1e3 with column scales).  One Newton step on M^-1 from its diagonal
// removes the first order:  Y' = (I - N) Y,  Y = diag(w) W,  N = diag(w) offdiag(M);  t = Y' a.  Two launches per
// covariance call, made by the first row-form call after it; a dropped direction (w_k = 0) keeps an exactly zero row.
//   cov_pinv_rowgram_kernel    M = W W^T over the free block, tile (i, j) summed over the columns in ascending order
//   cov_pinv_rowfactor_kernel  Y' tile (i, j) = Y_ij - sum_k N_ik Y_kj into the plan's (otherwise idle) X slot
__global__ __launch_bounds__(COV_PNT) void cov_pinv_rowgram_kernel(int n, int NPAD, const double* __restrict__ Wall,
                                                                   const int* __restrict__ nfree,
                                                                   const int* __restrict__ status,
                                                                   double* __restrict__ Gall) {
  CovTile t;
  if (!cov_tile(t, n, nfree, status)) return;
  const int ld = NPAD, nf = t.nf;
  const double* W = Wall + (long)t.b * NPAD * NPAD;
  double* G = Gall + (long)t.b * NPAD * NPAD;
  auto ldW = [&](int rt, int k, int q) {             // row 16 rt + lc of W, column 4 q + lr of k-tile k
    const int r = 16 * rt + t.lc, c = 16 * k + 4 * q + t.lr;
    return (r < nf && c < nf) ? W[(long)r * ld + c] : 0.0;
  };
  cov_tile_product(t, 0, [](int) { return 0; },
                   [&](int k, int q) { return ldW(t.i, k, q); },
                   [&](int j, int k, int q) { return ldW(j, k, q); },
                   [&](int j, v4d acc) {
#pragma unroll
                     for (int g = 0; g < 4; ++g) G[(long)(16 * t.i + t.lr + 4 * g) * ld + 16 * j + t.lc] = acc[g];
                   });
}

__global__ __launch_bounds__(COV_PNT) void cov_pinv_rowfactor_kernel(int n, int NPAD, const double* __restrict__ Wall,
                                                                     const double* __restrict__ wall,
                                                                     const double* __restrict__ Gall,
                                                                     const int* __restrict__ nfree,
                                                                     const int* __restrict__ status,
                                                                     double* __restrict__ Yall) {
  CovTile t;
  if (!cov_tile(t, n, nfree, status)) return;
  const int ld = NPAD, nf = t.nf;
  const double* W = Wall + (long)t.b * NPAD * NPAD;
  const double* G = Gall + (long)t.b * NPAD * NPAD;
  const double* wt = wall + (long)t.b * ld;
  double* Y = Yall + (long)t.b * NPAD * NPAD;
  const int ra = 16 * t.i + t.lc;
  const double wa = (ra < nf) ? wt[ra] : 0.0;
  cov_tile_product(t, 0, [](int) { return 0; },
                   [&](int k, int q) {
                     const int c = 16 * k + 4 * q + t.lr;            // column of N = row of Y
                     return (ra < nf && c < nf && c != ra) ? wa * G[(long)ra * ld + c] : 0.0;
                   },
                   [&](int j, int k, int q) {
                     const int c = 16 * k + 4 * q + t.lr, cb = 16 * j + t.lc;
                     return (c < nf && cb < nf) ? wt[c] * W[(long)c * ld + cb] : 0.0;
                   },
                   [&](int j, v4d acc) {
                     const int cb = 16 * j + t.lc;
#pragma unroll
                     for (int g = 0; g < 4; ++g) {
                       const int r = 16 * t.i + t.lr + 4 * g;
                       const double y = (r < nf && cb < nf) ? wt[r] * W[(long)r * ld + cb] : 0.0;
                       Y[(long)r * ld + cb] = (r < nf && cb < nf) ? y - acc[g] : 0.0;
                     }
                   });
}

static constexpr int COV_RNT = 256;               // four waves
static constexpr int COV_RNW = COV_RNT / WAVE;
static constexpr int COV_RROWS = 16 * COV_RNW;    // rows of A per workgroup
static constexpr int COV_RJB = 4;                 // output tiles a wave accumulates at a time

template <bool PINV>
__global__ __launch_bounds__(COV_RNT) void cov_rows_kernel(int rows, int n, int NPAD, int chunks,
                                                           const double* __restrict__ Aall,
                                                           const int* __restrict__ perm,
                                                           const int* __restrict__ nfree,
                                                           const double* __restrict__ Xall,
                                                           const double* __restrict__ wall,
                                                           const int* __restrict__ status,
                                                           const double* __restrict__ dscale,
                                                           double* __restrict__ out) {
  extern __shared__ int psh[];                       // [n] (with a permutation only)
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* o = out + (long)b * rows;
  const int nf = nfree ? nfree[b] : n;
  const int st = status[b];
  if (st != 0 || nf == 0) {                          // uniform: no factor (NaN), or nothing free (0.0)
    const int r = chunk * COV_RROWS + tid;
    if (tid < COV_RROWS && r < rows) o[r] = (st != 0) ? __builtin_nan("") : 0.0;
    return;
  }
  if (perm) {
    for (int j = tid; j < nf; j += COV_RNT) psh[j] = perm[(long)b * n + j];
    __syncthreads();
  }
  const int r0 = chunk * COV_RROWS + 16 * w;         // this wave's 16 rows
  if (r0 >= rows) return;
  const int lr = lane >> 4, lc = lane & 15;
  const int NTl = (nf + 15) >> 4;                    // (16 NTl <= NPAD: nf <= n < NPAD)
  const int ld = NPAD;
  const double* X = Xall + (long)b * NPAD * NPAD;
  const bool arow = r0 + lc < rows;                  // operand A: row lc of the group, column 4 q + lr of the tile
  const double* a = Aall + ((long)b * rows + (arow ? r0 + lc : r0)) * n;
  double ssq[4] = {0.0, 0.0, 0.0, 0.0};              // rows lr + 4 g, the columns = lc (mod 16)
  for (int j0 = 0; j0 < NTl; j0 += COV_RJB) {
    const int jn = min(COV_RJB, NTl - j0);
    const int kend = PINV ? NTl : j0 + jn;
    v4d acc[COV_RJB];
#pragma unroll
    for (int jj = 0; jj < COV_RJB; ++jj) acc[jj] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < kend; ++k) {
      double av[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 16 * k + 4 * q + lr;
        av[q] = (arow && c < nf) ? a[perm ? psh[c] : c] : 0.0;
      }
#pragma unroll
      for (int jj = 0; jj < COV_RJB; ++jj) {
        const int j = j0 + jj;
        if (jj < jn && (PINV || k <= j)) {           // uniform (regular route: the tiles below the diagonal are skipped)
          double bv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int r = PINV ? 16 * j + lc : 16 * k + 4 * q + lr;
            const int c = PINV ? 16 * k + 4 * q + lr : 16 * j + lc;
            bv[q] = (r < nf && c < nf) ? X[(long)r * ld + c] : 0.0;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[jj] = mfma_f64(av[q], bv[q], acc[jj]);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < COV_RJB; ++jj) {
      if (jj < jn) {
        double wt = 1.0;
        if (PINV) {
          const int kk = 16 * (j0 + jj) + lc;
          wt = (kk < nf) ? (wall ? wall[(long)b * ld + kk] : 1.0) : 0.0;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          double t = acc[jj][g];
          if (PINV) t = (wt != 0.0) ? t * wt : 0.0;  // (a dropped direction: exactly nothing)
          ssq[g] = fma(t, t, ssq[g]);
        }
      }
    }
  }
  const double sc = dscale ? dscale[b] : 1.0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    double v = ssq[g];
#pragma unroll
    for (int h = 8; h > 0; h >>= 1) v += __shfl_xor(v, h, 64);
    const int r = r0 + lr + 4 * g;
    if (lc == 0 && r < rows) o[r] = sc * v;
  }
}

// dscale[b] = obj[b] / (m - n): curve_fit's residual variance ("s_sq = cost / (ysize - p0.size)")
__global__ __launch_bounds__(256) void cov_variance_kernel(int B, double dof, const double* __restrict__ obj,
                                                           double* __restrict__ dscale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) dscale[b] = obj[b] / dof;
}

// dscale[b] = obj[b] / (nobs[b] - n), the problem's own degrees of freedom (nan_policy='omit'); +inf
// where nobs[b] <= n: the covariance of such a problem cannot be estimated
__global__ __launch_bounds__(256) void cov_variance_nobs_kernel(int B, int n, const double* __restrict__ obj,
                                                                const int* __restrict__ nobs,
                                                                double* __restrict__ dscale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    const int dof = nobs[b] - n;
    dscale[b] = dof > 0 ? obj[b] / (double)dof : __builtin_huge_val();
  }
}

// ---- launches ----------------------------------------------------------------------------------
hipError_t launch_cov_perm(int B, int n, const long long* active, int lda, int* perm, int* nfree, int* ncols,
                           hipStream_t s) {
  hipLaunchKernelGGL(cov_perm_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, n, active, lda, perm, nfree, ncols);
  return hipGetLastError();
}

hipError_t launch_cov_trf_mask(int B, int n, int ld, double rtol, const double* x, const double* lb, const double* ub,
                               long long* mask, hipStream_t s) {
  const long tot = (long)B * n;
  hipLaunchKernelGGL(cov_trf_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, B, n, ld, rtol, x, lb,
                     ub, mask);
  return hipGetLastError();
}

hipError_t launch_cov_gather(int B, int m, int n, const double* J, const int* perm, double* Jp, hipStream_t s) {
  int rows = COV_TARGET_ELEMS / n;
  rows = rows < 1 ? 1 : rows;
  if (rows > m) rows = m;
  const int chunks = (m + rows - 1) / rows;
  const long grid = (long)B * chunks;
  if (grid > 0x7fffffffL) return hipErrorInvalidValue;
  const size_t lds = sizeof(int) * (size_t)n;
  const bool vec = (n % 2 == 0) && ((reinterpret_cast<uintptr_t>(Jp) & 15) == 0);
  if (vec) return launch<cov_gather_kernel<true>>(dim3((unsigned)grid), dim3(COV_GNT), lds, s, m, n, rows, chunks, J,
                                                  perm, Jp);
  return launch<cov_gather_kernel<false>>(dim3((unsigned)grid), dim3(COV_GNT), lds, s, m, n, rows, chunks, J, perm, Jp);
}

hipError_t launch_cov_stack(int B, int m, int n, int r0, int c, const double* J, double* S, int srows, int ld,
                            hipStream_t s) {
  if (c <= 0 || r0 < 0 || r0 + c > m || ld + c > srows || n > ld || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_stack_kernel, dim3(c, B), dim3(COV_GNT), 0, s, m, n, r0, c, J, S, srows, ld);
  return hipGetLastError();
}

hipError_t launch_cov_inverse(int B, int m, int n, int NPAD, const double* R, double* X, const int* nfree, double* cov,
                              double* rcond, int* status, hipStream_t s) {
  hipLaunchKernelGGL(cov_inverse_kernel, dim3(B), dim3(COV_NT), 0, s, m, n, NPAD, R, X, nfree, cov, rcond, status);
  return hipGetLastError();
}

hipError_t launch_cov_product(int B, int n, int NPAD, const double* X, const int* nfree, const int* perm,
                              const int* status, double* cov, hipStream_t s) {
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_product_kernel, dim3((n + 15) / 16, B), dim3(COV_PNT), 0, s, n, NPAD, X, nfree, perm, status,
                     cov);
  return hipGetLastError();
}

hipError_t launch_cov_pinv_weights(int B, int m, int n, int NPAD, const double* X, const double* s, const int* sweeps,
                                   int max_sweeps, const int* nfree, double* w, double* cov, int* rank, double* rcond,
                                   double* kept_rcond, int* status, hipStream_t st) {
  hipLaunchKernelGGL(cov_pinv_weights_kernel, dim3(B), dim3(COV_PNT), 0, st, m, n, NPAD, X, s, sweeps, max_sweeps,
                     nfree, w, cov, rank, rcond, kept_rcond, status);
  return hipGetLastError();
}

hipError_t launch_cov_pinv_product(int B, int n, int NPAD, const double* X, const double* w, const int* nfree,
                                   const int* perm, const int* status, const double* dscale, double* cov,
                                   hipStream_t st) {
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_pinv_product_kernel, dim3((n + 15) / 16, B), dim3(COV_PNT), 0, st, n, NPAD, X, w, nfree, perm,
                     status, dscale, cov);
  return hipGetLastError();
}

hipError_t launch_cov_variance(int B, int m, int n, const double* obj, double* dscale, hipStream_t st) {
  if (m <= n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_variance_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, (double)(m - n), obj, dscale);
  return hipGetLastError();
}

hipError_t launch_cov_variance_nobs(int B, int n, const double* obj, const int* nobs, double* dscale, hipStream_t st) {
  if (!nobs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_variance_nobs_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, n, obj, nobs, dscale);
  return hipGetLastError();
}

hipError_t launch_cov_rows(int B, int rows, int n, int NPAD, int pinv, const double* A, const int* perm,
                           const int* nfree, const double* X, const double* w, const int* status,
                           const double* dscale, double* out, hipStream_t st) {
  if (rows <= 0 || (perm && !nfree)) return hipErrorInvalidValue;
  const int chunks = (rows + COV_RROWS - 1) / COV_RROWS;
  const long grid = (long)B * chunks;
  if (grid > 0x7fffffffL) return hipErrorInvalidValue;
  const size_t lds = perm ? sizeof(int) * (size_t)n : 0;
  if (pinv) return launch<cov_rows_kernel<true>>(dim3((unsigned)grid), dim3(COV_RNT), lds, st, rows, n, NPAD, chunks, A,
                                                 perm, nfree, X, w, status, dscale, out);
  return launch<cov_rows_kernel<false>>(dim3((unsigned)grid), dim3(COV_RNT), lds, st, rows, n, NPAD, chunks, A, perm,
                                        nfree, X, w, status, dscale, out);
}

hipError_t launch_cov_pinv_rowfactor(int B, int n, int NPAD, const double* W, const double* w, const int* nfree,
                                     const int* status, double* G, double* Y, hipStream_t st) {
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cov_pinv_rowgram_kernel, dim3((n + 15) / 16, B), dim3(COV_PNT), 0, st, n, NPAD, W, nfree, status, G);
  hipLaunchKernelGGL(cov_pinv_rowfactor_kernel, dim3((n + 15) / 16, B), dim3(COV_PNT), 0, st, n, NPAD, W, w, G, nfree,
                     status, Y);
  return hipGetLastError();
}

}  // namespace blsq
