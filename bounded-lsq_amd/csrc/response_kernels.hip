// Instrument response (blsq_response_apply_dev): a model convolved with a measured kernel h before it is
// compared with the data.  The second stage behind the model-eval entries, which write the raw model values g and the
// raw (mapped, nc wide) Jacobian G:
//   mu[q][i]   = sum_{k < L} h[b][k] * g[q][i + origin - k]          q = b * reps + r; a term whose index i + origin - k
//   HG[b][i][j] = sum_{k < L} h[b][k] * G[b][i + origin - k][j]       lies outside [0, m) is dropped
//   f = w (mu - y), J = w HG   |   Poisson: (r, c) = poisson_rc(mu, y), f = r, J = c HG   |   OMIT: 0 where y is NaN
// models.apply_response of bounded_lsq/_models.py is the definition.  J is the product of a banded Toeplitz matrix with
// the (m x nc) matrix G of a problem; f is the same walk over the single column g.
//
// One kernel, response_kernel, launched once for f (src = g, one column, Q = B reps problems) and once for J (src = G,
// nc columns, B problems).  A workgroup owns problem blockIdx.x and walks over blocks of `rows` output rows (a stride
// loop over gridDim.y: m has no limit), inside a block over tiles of ct <= RESP_CT columns, inside a tile over chunks of
// RESP_KC taps.  For a chunk [kc, kend) it stages into LDS the taps and the source rows the block needs for them,
// [i0 + origin - (kend - 1), i0 + nr - 1 + origin - kc] clipped to [0, m): consecutive threads read consecutive
// addresses (a block of rows at ct == nc is one contiguous piece of memory).  Then thread e of the tile, row e / ct and
// column e % ct, runs its taps: consecutive lanes on consecutive LDS doubles (no bank conflict), and the result is
// stored with consecutive lanes on consecutive addresses.  The partial sum of an element crosses a chunk through an LDS
// tile of its own, which exists only where L > RESP_KC.  LDS: (rows + RESP_KC - 1) ct + RESP_KC + rows doubles, and
// rows ct more where L > RESP_KC: at most 50 KB for any nc and L (rows ct <= RESP_ELEMS), so the loops, not a limit on
// nc or L, keep the grant small.
//
// Summation order, a function of (L, origin, i, m) alone: the taps k of row i that are not dropped are
// k_lo = max(0, i + origin - (m - 1)) .. k_hi = min(L - 1, i + origin) (never empty: k = origin is among them); the sum
// starts as the PRODUCT h[k_lo] * src[i + origin - k_lo] and takes the others in ascending k by acc = fma(h[k], src, acc).
// A partial sum parked in LDS between two chunks is the same double.  Nothing depends on B, reps, nc, the strides, the
// tiling or the batch mates; with h = [1.0] the sum is 1.0 * src, src itself in every bit.
//
// The epilogue uses the operations of the model kernel's own (model_kernels.hip), in its order: mu - y first, then
// the weight; the Poisson pair comes from poisson_rc (poisson_rc.h), and for J its c needs mu of the row, so a J launch
// under the Poisson estimator first walks g for the rows of its block (the same sum, hence the same mu as f's) and
// keeps c per row in LDS.  A row whose y is NaN gives +0.0 under OMIT; the model was still evaluated there, because
// its neighbours need it.
//
// Compiled with -ffp-contract=off (EXACT_SRCS): every fused operation of this file is spelled fma().
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"
#include "poisson_rc.h"

#include <algorithm>

namespace blsq {

static constexpr int RESP_NT = 256;
static constexpr int RESP_CT = 32;               // columns of a tile
static constexpr int RESP_KC = 64;               // taps of a chunk
static constexpr int RESP_ELEMS = 2048;          // elements of a tile: rows = RESP_ELEMS / ct

struct RespArgs {
  int m, nc, reps, L, origin;
  int ct, rows;                 // columns of a tile (min(nc, RESP_CT)) and rows of a block
  int poisson, omit, is_J;
  const double* h; long h_stride;
  const double* src;            // g [Q][m] (f launch) or G [Q][m][nc] (J launch)
  const double* g;              // J launch under Poisson: the model values mu is convolved from
  const double* y;
  const double* w; long w_stride;
  double* dst;
  const int* mask;              // J launch alone
};

// The sums of one tile: rows [i0, i0 + nr) and columns [c0, c0 + ncol) of H src for the problem whose source starts at
// `src` (row stride ld).  `tile`, `hs`, `part` are the workgroup's LDS; done(e, r, c, sum) receives every element once.
// All threads of the workgroup call this with the same arguments (it holds barriers).
template <class Done>
__device__ __forceinline__ void response_tile(const RespArgs& A, const double* __restrict__ src, int ld, int c0,
                                              int ncol, int i0, int nr, const double* __restrict__ hq, double* tile,
                                              double* hs, double* part, Done done) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int m = A.m, L = A.L, origin = A.origin;
  const int total = nr * ncol;
  for (int kc = 0; kc < L; kc += RESP_KC) {
    const int kend = min(L, kc + RESP_KC);
    const int jlo = max(0, i0 + origin - (kend - 1)), jhi = min(m - 1, i0 + nr - 1 + origin - kc);
    __syncthreads();                              // the tile and the taps of the chunk (or tile) before are done with
    for (int k = kc + tid; k < kend; k += nt) hs[k - kc] = hq[k];
    const int staged = (jhi - jlo + 1) * ncol;    // (<= 0: no row of the block meets a tap of this chunk)
    if (ncol == ld) {                             // whole rows: one contiguous piece
      const double* s0 = src + (long)jlo * ld;
      for (int e = tid; e < staged; e += nt) tile[e] = s0[e];
    } else {
      for (int e = tid; e < staged; e += nt) {
        const int j = e / ncol, c = e - j * ncol;
        tile[e] = src[(long)(jlo + j) * ld + c0 + c];
      }
    }
    __syncthreads();
    for (int e = tid; e < total; e += nt) {
      const int r = e / ncol, c = e - r * ncol;
      const int i = i0 + r;
      const int k_first = max(0, i + origin - (m - 1));
      int k = max(kc, k_first);
      const int khi = min(kend - 1, i + origin);
      // element (j, c) of the staged rows, j = i + origin - k: one row back per tap
      const double* tp = tile + (long)(i + origin - k - jlo) * ncol + c;
      double acc = 0.0;
      if (kc > 0) acc = part[e];
      if (k <= khi && k == k_first) {
        acc = hs[k - kc] * *tp;
        ++k; tp -= ncol;
      }
      for (; k <= khi; ++k, tp -= ncol) acc = fma(hs[k - kc], *tp, acc);
      if (kend < L) part[e] = acc;
      else done(e, r, c, acc);
    }
  }
}

__global__ __launch_bounds__(RESP_NT) void response_kernel(RespArgs A) {
  extern __shared__ double resp_lds[];
  const long q = blockIdx.x, b = q / A.reps;
  if (A.mask && A.mask[b] == 0) return;           // a masked problem: nothing of it is read (uniform per workgroup)
  const int m = A.m, nc = A.nc, ct = A.ct, rows = A.rows;
  double* tile = resp_lds;                                        // (rows + RESP_KC - 1) * ct
  double* hs = tile + (size_t)(rows + RESP_KC - 1) * ct;          // RESP_KC
  double* cs = hs + RESP_KC;                                      // rows: c of the Poisson transform (J launch)
  double* part = cs + rows;                                       // rows * ct, where L > RESP_KC
  const double* hq = A.h + b * A.h_stride;
  const double* yb = A.y ? A.y + b * (long)m : nullptr;
  const double* wb = (!A.poisson && A.w) ? A.w + b * A.w_stride : nullptr;
  const bool omit = A.omit != 0;
  for (long i0l = (long)blockIdx.y * rows; i0l < m; i0l += (long)gridDim.y * rows) {
    const int i0 = (int)i0l, nr = min(rows, m - i0);
    if (!A.is_J) {
      double* out = A.dst + q * (long)m + i0;
      response_tile(A, A.src + q * (long)m, 1, 0, 1, i0, nr, hq, tile, hs, part, [&](int e, int r, int, double mu) {
        const int i = i0 + r;
        const double yi = yb ? yb[i] : 0.0;
        double v;
        if (omit && yi != yi) {
          v = 0.0;
        } else if (A.poisson) {
          double c;
          poisson_rc(mu, yi, v, c);
        } else {
          const double res = yb ? mu - yi : mu;
          v = wb ? wb[i] * res : res;
        }
        out[e] = v;
      });
      continue;
    }
    if (A.poisson) {                              // c of every row of the block, from mu as the f launch sums it
      response_tile(A, A.g + q * (long)m, 1, 0, 1, i0, nr, hq, tile, hs, part, [&](int, int r, int, double mu) {
        double rr, c;
        poisson_rc(mu, yb[i0 + r], rr, c);
        cs[r] = c;
      });
      __syncthreads();
    }
    const double* Gq = A.src + q * (long)m * nc;
    double* Jq = A.dst + (q * (long)m + i0) * nc;
    for (int c0 = 0; c0 < nc; c0 += ct) {
      const int ncol = min(ct, nc - c0);
      response_tile(A, Gq, nc, c0, ncol, i0, nr, hq, tile, hs, part, [&](int, int r, int c, double s) {
        const int i = i0 + r;
        double v;
        if (omit && yb[i] != yb[i]) v = 0.0;
        else if (A.poisson) v = cs[r] * s;
        else v = wb ? wb[i] * s : s;
        Jq[(long)r * nc + c0 + c] = v;
      });
    }
  }
}

static hipError_t launch_response_one(const ResponseCall& c, bool is_J, hipStream_t s) {
  RespArgs A;
  A.m = c.m; A.nc = is_J ? c.nc : 1; A.reps = is_J ? 1 : c.reps; A.L = c.L; A.origin = c.origin;
  A.ct = std::min(A.nc, RESP_CT);
  A.rows = RESP_ELEMS / A.ct;
  A.poisson = c.est == BLSQ_EST_POISSON; A.omit = c.nan_policy == BLSQ_NAN_OMIT; A.is_J = is_J;
  A.h = c.h; A.h_stride = c.h_stride;
  A.src = is_J ? c.G : c.g; A.g = c.g;
  A.y = c.y; A.w = c.w; A.w_stride = c.w_stride;
  A.dst = is_J ? c.J : c.f;
  A.mask = is_J ? c.mask : nullptr;
  const long Q = (long)c.B * A.reps;
  if (Q > 0x7fffffffL) return hipErrorInvalidValue;
  const long blocks = ((long)c.m + A.rows - 1) / A.rows;
  const size_t lds = sizeof(double) * ((size_t)(A.rows + RESP_KC - 1) * A.ct + RESP_KC + A.rows +
                                       (c.L > RESP_KC ? (size_t)A.rows * A.ct : 0));
  // a workgroup no wider than the elements of its largest tile (whole waves)
  const long elems = (long)std::min(c.m, A.rows) * A.ct;
  const int nt = (int)std::min<long>(RESP_NT, (elems + WAVE - 1) / WAVE * WAVE);
  return launch<response_kernel>(dim3((unsigned)Q, (unsigned)std::min(blocks, 65535L)), dim3(nt), lds, s, A);
}

hipError_t launch_response_apply(const ResponseCall& c, hipStream_t s) {
  const bool poisson = c.est == BLSQ_EST_POISSON, omit = c.nan_policy == BLSQ_NAN_OMIT;
  if ((!poisson && c.est != BLSQ_EST_LSE) || (!omit && c.nan_policy != BLSQ_NAN_PROPAGATE)) return hipErrorInvalidValue;
  if (c.B < 1 || c.reps < 1 || c.m < 1 || c.m > BLSQ_RESPONSE_MAX_M || c.nc < 1) return hipErrorInvalidValue;
  if (c.L < 1 || c.L > BLSQ_RESPONSE_MAX_L || c.origin < 0 || c.origin >= c.L) return hipErrorInvalidValue;
  if (!c.h || (c.h_stride != 0 && c.h_stride != (long)c.L)) return hipErrorInvalidValue;
  if (!c.f && !c.J) return hipErrorInvalidValue;
  if ((c.f || (c.J && poisson)) && !c.g) return hipErrorInvalidValue;
  if (c.J && (!c.G || c.reps != 1)) return hipErrorInvalidValue;
  if (((poisson || omit) && !c.y) || (poisson && c.w)) return hipErrorInvalidValue;
  if (c.w && c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  if (c.f) {
    const hipError_t e = launch_response_one(c, false, s);
    if (e != hipSuccess) return e;
  }
  return c.J ? launch_response_one(c, true, s) : hipSuccess;
}

}  // namespace blsq
