// Built-in fit models evaluated on the device (blsq_model_eval_dev).
//
// For a batch of parameter vectors P [Q][n], Q = B * reps, q = b * reps + r:
//   f[q][i]    = w[b][i] * (model(t[b][.., i]; P[q]) - y[b][i])
//   J[q][i][j] = w[b][i] * d model / d p_j                               (reps == 1)
// Five closed-form families (BLSQ_MODEL_*); the formulas, operation by operation, are those of the numpy functions of
// bounded_lsq/_models.py.  Compiled with -ffp-contract=off, so a value does not depend on what the compiler fuses; the
// only difference from numpy is the last bit of exp().  No checking: a non-finite value passes through as IEEE gives it.
//
// Shape.  One WAVE owns one work item: 64 consecutive rows of one point q; a workgroup is 1, 2 or 4 independent waves
// (as many as the J tiles leave room for in LDS).  A lane owns row i, reads its parameters through wave-uniform (scalar)
// loads and evaluates the K terms once for both f and the J row.  f is stored directly (lane i -> f[q][i]).  The J
// tile of the 64 rows is one contiguous block of 64 n doubles in memory: a lane writes its row into the wave's LDS
// tile (row stride n | 1 doubles: odd, so the 16 lanes of an 8-byte LDS store group fall on 16 different bank pairs), and
// the wave then streams the tile out with consecutive lanes on consecutive addresses.  Store-bound: 8 m n bytes per
// problem; no MFMA, no scratch.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"

namespace blsq {

static constexpr int MODEL_ROWS = 64;                 // rows of one work item: one per lane
static constexpr int MODEL_LDS_BYTES = 48 * 1024;     // J tiles of one workgroup (n = 64: one wave, 33280 B)

struct ModelArgs {
  int m, n, reps, tiles;        // tiles = ceil(m / 64)
  long items;                   // Q * tiles
  const double* t; long t_stride;
  const double* y;
  const double* w; long w_stride;
  const double* P;
  double* f;
  double* J;
  const int* mask;
};

// The terms of one row.  `row` is the lane's slice of the wave's LDS tile (nullptr: f only); returns the model value.
template <int MODEL>
__device__ __forceinline__ double model_row(int n, int m, const double* __restrict__ tb, int i,
                                            const double* __restrict__ p, double wi, double* row) {
  if (MODEL == BLSQ_MODEL_POLY) {
    const double t = tb[i];
    double acc = p[n - 1];
    for (int k = n - 2; k >= 0; --k) acc = acc * t + p[k];            // Horner
    if (row) {
      double pw = 1.0;
      for (int k = 0; k < n; ++k) { row[k] = wi * pw; pw = pw * t; }
    }
    return acc;
  }
  if (MODEL == BLSQ_MODEL_EXP_SUM) {
    const double t = tb[i];
    const int K = (n - 1) / 2;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double a = p[2 * k], r = p[2 * k + 1];
      const double e = exp(-(r * t));
      const double g = a * e;
      acc = (k == 0) ? g : acc + g;
      if (row) { row[2 * k] = wi * e; row[2 * k + 1] = wi * (-(t * g)); }
    }
    if (row) row[n - 1] = wi;
    return acc + p[n - 1];
  }
  if (MODEL == BLSQ_MODEL_GAUSS_SUM || MODEL == BLSQ_MODEL_LORENTZ_SUM) {
    const double t = tb[i];
    const int K = (n - 1) / 3;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double a = p[3 * k], mu = p[3 * k + 1], s = p[3 * k + 2];
      const double z = (t - mu) / s;
      double e, g, dmu;
      if (MODEL == BLSQ_MODEL_GAUSS_SUM) {
        e = exp(-0.5 * (z * z));
        g = a * e;
        dmu = (g * z) / s;
      } else {
        e = 1.0 / (1.0 + z * z);
        g = a * e;
        dmu = (((2.0 * g) * e) * z) / s;
      }
      acc = (k == 0) ? g : acc + g;
      if (row) { row[3 * k] = wi * e; row[3 * k + 1] = wi * dmu; row[3 * k + 2] = wi * (dmu * z); }
    }
    if (row) row[n - 1] = wi;
    return acc + p[n - 1];
  }
  // BLSQ_MODEL_GAUSS2D: t is [2][m]
  const double du = tb[i] - p[1], dv = tb[m + i] - p[2];
  const double a = p[0], s = p[3];
  const double r2 = du * du + dv * dv, s2 = s * s;
  const double e = exp(-0.5 * (r2 / s2));
  const double g = a * e;
  if (row) {
    row[0] = wi * e;
    row[1] = wi * ((g * du) / s2);
    row[2] = wi * ((g * dv) / s2);
    row[3] = wi * ((g * r2) / (s2 * s));
    row[4] = wi;
  }
  return g + p[4];
}

template <int MODEL>
__global__ __launch_bounds__(256) void model_eval_kernel(ModelArgs A) {
  extern __shared__ double model_tiles[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);            // wave-uniform, in a scalar register
  const int wpb = blockDim.x >> 6;
  const long item = (long)blockIdx.x * wpb + wave;
  bool live = item < A.items;
  long q = 0;
  int r0 = 0;
  if (live) {
    q = item / A.tiles;
    r0 = (int)(item - q * A.tiles) * MODEL_ROWS;
  }
  const long b = q / A.reps;
  if (live && A.mask && A.mask[b] == 0) live = false;                           // a masked problem is left untouched
  const int n = A.n, m = A.m;
  const int ld = n | 1;
  const int nr = live ? min(MODEL_ROWS, m - r0) : 0;
  double* tile = A.J ? model_tiles + (size_t)wave * MODEL_ROWS * ld : nullptr;
  if (lane < nr) {
    const int i = r0 + lane;
    const double* tb = A.t + b * A.t_stride;
    const double wi = A.w ? A.w[b * A.w_stride + i] : 1.0;
    const double v = model_row<MODEL>(n, m, tb, i, A.P + q * n, wi, tile ? tile + lane * ld : nullptr);
    if (A.f) {
      const double r = A.y ? v - A.y[b * m + i] : v;
      A.f[q * m + i] = A.w ? wi * r : r;
    }
  }
  if (A.J) {
    __syncthreads();                       // (every wave of the workgroup arrives: no early return above)
    // the wave's rows are the contiguous block J[q][r0 .. r0 + nr)[0 .. n): lane l takes elements l, l + 64, ...
    double* out = A.J + (q * m + r0) * (long)n;
    const int total = nr * n;
    int row = lane / n, col = lane - row * n;
    const int drow = WAVE / n, dcol = WAVE - drow * n;
    for (int e = lane; e < total; e += WAVE) {
      out[e] = tile[row * ld + col];
      row += drow; col += dcol;
      if (col >= n) { col -= n; ++row; }
    }
  }
}

hipError_t launch_model_eval(int model, int B, int reps, int m, int n, const double* t, long t_stride, const double* y,
                             const double* w, long w_stride, const double* P, double* f, double* J, const int* mask,
                             hipStream_t s) {
  ModelArgs A;
  A.m = m; A.n = n; A.reps = reps; A.tiles = (m + MODEL_ROWS - 1) / MODEL_ROWS;
  A.items = (long)B * reps * A.tiles;
  A.t = t; A.t_stride = t_stride; A.y = y; A.w = w; A.w_stride = w_stride; A.P = P; A.f = f; A.J = J; A.mask = mask;
  const size_t tile_bytes = J ? sizeof(double) * MODEL_ROWS * (size_t)(n | 1) : 0;
  int wpb = 4;
  while (wpb > 1 && tile_bytes * wpb > (size_t)MODEL_LDS_BYTES) wpb >>= 1;
  if (tile_bytes * wpb > (size_t)MODEL_LDS_BYTES) return hipErrorInvalidValue;
  const long grid = (A.items + wpb - 1) / wpb;
  if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 g((unsigned)grid), blk(64 * wpb);
  const size_t lds = tile_bytes * wpb;
  switch (model) {
    case BLSQ_MODEL_POLY: hipLaunchKernelGGL(model_eval_kernel<BLSQ_MODEL_POLY>, g, blk, lds, s, A); break;
    case BLSQ_MODEL_EXP_SUM: hipLaunchKernelGGL(model_eval_kernel<BLSQ_MODEL_EXP_SUM>, g, blk, lds, s, A); break;
    case BLSQ_MODEL_GAUSS_SUM: hipLaunchKernelGGL(model_eval_kernel<BLSQ_MODEL_GAUSS_SUM>, g, blk, lds, s, A); break;
    case BLSQ_MODEL_LORENTZ_SUM: hipLaunchKernelGGL(model_eval_kernel<BLSQ_MODEL_LORENTZ_SUM>, g, blk, lds, s, A); break;
    case BLSQ_MODEL_GAUSS2D: hipLaunchKernelGGL(model_eval_kernel<BLSQ_MODEL_GAUSS2D>, g, blk, lds, s, A); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace blsq
