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
//
// Mapped instances (MAPPED = true; blsq_model_eval_map_dev).  The model's n parameters are a function of
// nf <= n solver variables: P_full[q][j] = X[q][pmap[j]], or Pfix[b][j] where pmap[j] == -1.  A wave expands its point's
// vector once (lane j produces P_full[q][j]) into 64 doubles of LDS of its own, and model_row reads p[] from there: every
// lane reads the same address, which LDS broadcasts.  The J row is written through row_put: column j goes to slot
// pmap[j] of a tile of row stride nf | 1: the first column of a slot is stored, later ones are added in ascending j
// (a sequential float64 sum), a column with pmap[j] == -1 is computed and dropped.  f is the residual of the unmapped
// instance at P_full, bit for bit.  The unmapped instances resolve row_put to the plain store and compile to the code
// they had before the flag existed.
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

// The map of a mapped launch, behind the arguments every instance takes.  pm[j]: -1 (held at Pfix), the slot k for the
// first column of slot k (its leader), 64 + k for a later one.
struct ModelMapArgs : ModelArgs {
  int nf;                       // solver variables; P is X [Q][nf]
  const double* Pfix;           // [B][n]; read where pm[j] == -1 only
  signed char pm[MODEL_ROWS];
};
template <bool MAPPED> struct ModelArgsOf { using type = ModelArgs; };
template <> struct ModelArgsOf<true> { using type = ModelMapArgs; };

__device__ __forceinline__ int map_nf(const ModelArgs& A) { return A.n; }
__device__ __forceinline__ int map_nf(const ModelMapArgs& A) { return A.nf; }
__device__ __forceinline__ const signed char* map_pm(const ModelArgs&) { return nullptr; }
__device__ __forceinline__ const signed char* map_pm(const ModelMapArgs& A) { return A.pm; }
__device__ __forceinline__ const double* map_pfix(const ModelArgs&) { return nullptr; }
__device__ __forceinline__ const double* map_pfix(const ModelMapArgs& A) { return A.Pfix; }

// row[k] = v of model_row.  Unmapped: the plain store.  Mapped: into the slot of column k (columns arrive in ascending k).
template <bool MAPPED>
__device__ __forceinline__ void row_put(double* row, const signed char* pm, int k, double v) {
  if (!MAPPED) {
    row[k] = v;
  } else {
    const int c = pm[k];
    if (c >= MODEL_ROWS) row[c - MODEL_ROWS] = row[c - MODEL_ROWS] + v;
    else if (c >= 0) row[c] = v;
  }
}

// The terms of one row.  `row` is the lane's slice of the wave's LDS tile (nullptr: f only); returns the model value.
template <int MODEL, bool MAPPED>
__device__ __forceinline__ double model_row(int n, int m, const double* __restrict__ tb, int i,
                                            const double* __restrict__ p, double wi, double* row,
                                            const signed char* pm) {
#define PUT(k, v) row_put<MAPPED>(row, pm, (k), (v))
  if (MODEL == BLSQ_MODEL_POLY) {
    const double t = tb[i];
    double acc = p[n - 1];
    for (int k = n - 2; k >= 0; --k) acc = acc * t + p[k];            // Horner
    if (row) {
      double pw = 1.0;
      for (int k = 0; k < n; ++k) { PUT(k, wi * pw); pw = pw * t; }
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
      if (row) { PUT(2 * k, wi * e); PUT(2 * k + 1, wi * (-(t * g))); }
    }
    if (row) PUT(n - 1, wi);
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
      if (row) { PUT(3 * k, wi * e); PUT(3 * k + 1, wi * dmu); PUT(3 * k + 2, wi * (dmu * z)); }
    }
    if (row) PUT(n - 1, wi);
    return acc + p[n - 1];
  }
  // BLSQ_MODEL_GAUSS2D: t is [2][m]
  const double du = tb[i] - p[1], dv = tb[m + i] - p[2];
  const double a = p[0], s = p[3];
  const double r2 = du * du + dv * dv, s2 = s * s;
  const double e = exp(-0.5 * (r2 / s2));
  const double g = a * e;
  if (row) {
    PUT(0, wi * e);
    PUT(1, wi * ((g * du) / s2));
    PUT(2, wi * ((g * dv) / s2));
    PUT(3, wi * ((g * r2) / (s2 * s)));
    PUT(4, wi);
  }
  return g + p[4];
#undef PUT
}

template <int MODEL, bool MAPPED>
__global__ __launch_bounds__(256) void model_eval_kernel(typename ModelArgsOf<MAPPED>::type A) {
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
  const int nc = map_nf(A);                                                     // columns of J: n, or nf when mapped
  const int ld = nc | 1;
  const int nr = live ? min(MODEL_ROWS, m - r0) : 0;
  // mapped: the waves' parameter vectors (64 doubles each) lie in front of the tiles
  double* tiles = MAPPED ? model_tiles + (size_t)wpb * MODEL_ROWS : model_tiles;
  double* tile = A.J ? tiles + (size_t)wave * MODEL_ROWS * ld : nullptr;
  const double* p = A.P + q * nc;
  if constexpr (MAPPED) {
    double* pv = model_tiles + (size_t)wave * MODEL_ROWS;
    if (live && lane < n) {
      const int c = map_pm(A)[lane];
      pv[lane] = c < 0 ? map_pfix(A)[b * n + lane] : p[c & (MODEL_ROWS - 1)];
    }
    __syncthreads();                       // (the wave reads only its own vector; every wave arrives)
    p = pv;
  }
  if (lane < nr) {
    const int i = r0 + lane;
    const double* tb = A.t + b * A.t_stride;
    const double wi = A.w ? A.w[b * A.w_stride + i] : 1.0;
    const double v = model_row<MODEL, MAPPED>(n, m, tb, i, p, wi, tile ? tile + lane * ld : nullptr, map_pm(A));
    if (A.f) {
      const double r = A.y ? v - A.y[b * m + i] : v;
      A.f[q * m + i] = A.w ? wi * r : r;
    }
  }
  if (A.J) {
    __syncthreads();                       // (every wave of the workgroup arrives: no early return above)
    // the wave's rows are the contiguous block J[q][r0 .. r0 + nr)[0 .. nc): lane l takes elements l, l + 64, ...
    double* out = A.J + (q * m + r0) * (long)nc;
    const int total = nr * nc;
    int row = lane / nc, col = lane - row * nc;
    const int drow = WAVE / nc, dcol = WAVE - drow * nc;
    for (int e = lane; e < total; e += WAVE) {
      out[e] = tile[row * ld + col];
      row += drow; col += dcol;
      if (col >= nc) { col -= nc; ++row; }
    }
  }
}

// Waves per workgroup (4 / 2 / 1) whose LDS (wave_bytes each) fits the grant, and the launch of instance <.., MAPPED>.
template <bool MAPPED>
static hipError_t launch_model_instance(int model, typename ModelArgsOf<MAPPED>::type& A, size_t wave_bytes,
                                        hipStream_t s) {
  int wpb = 4;
  while (wpb > 1 && wave_bytes * wpb > (size_t)MODEL_LDS_BYTES) wpb >>= 1;
  if (wave_bytes * wpb > (size_t)MODEL_LDS_BYTES) return hipErrorInvalidValue;
  const long grid = (A.items + wpb - 1) / wpb;
  if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 g((unsigned)grid), blk(64 * wpb);
  const size_t lds = wave_bytes * wpb;
  switch (model) {
    case BLSQ_MODEL_POLY: hipLaunchKernelGGL((model_eval_kernel<BLSQ_MODEL_POLY, MAPPED>), g, blk, lds, s, A); break;
    case BLSQ_MODEL_EXP_SUM: hipLaunchKernelGGL((model_eval_kernel<BLSQ_MODEL_EXP_SUM, MAPPED>), g, blk, lds, s, A); break;
    case BLSQ_MODEL_GAUSS_SUM:
      hipLaunchKernelGGL((model_eval_kernel<BLSQ_MODEL_GAUSS_SUM, MAPPED>), g, blk, lds, s, A); break;
    case BLSQ_MODEL_LORENTZ_SUM:
      hipLaunchKernelGGL((model_eval_kernel<BLSQ_MODEL_LORENTZ_SUM, MAPPED>), g, blk, lds, s, A); break;
    case BLSQ_MODEL_GAUSS2D: hipLaunchKernelGGL((model_eval_kernel<BLSQ_MODEL_GAUSS2D, MAPPED>), g, blk, lds, s, A); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static void fill_model_args(ModelArgs& A, int B, int reps, int m, int n, const double* t, long t_stride, const double* y,
                            const double* w, long w_stride, const double* P, double* f, double* J, const int* mask) {
  A.m = m; A.n = n; A.reps = reps; A.tiles = (m + MODEL_ROWS - 1) / MODEL_ROWS;
  A.items = (long)B * reps * A.tiles;
  A.t = t; A.t_stride = t_stride; A.y = y; A.w = w; A.w_stride = w_stride; A.P = P; A.f = f; A.J = J; A.mask = mask;
}

hipError_t launch_model_eval(int model, int B, int reps, int m, int n, const double* t, long t_stride, const double* y,
                             const double* w, long w_stride, const double* P, double* f, double* J, const int* mask,
                             hipStream_t s) {
  ModelArgs A;
  fill_model_args(A, B, reps, m, n, t, t_stride, y, w, w_stride, P, f, J, mask);
  const size_t tile_bytes = J ? sizeof(double) * MODEL_ROWS * (size_t)(n | 1) : 0;
  return launch_model_instance<false>(model, A, tile_bytes, s);
}

hipError_t launch_model_eval_map(int model, int B, int reps, int m, int n, int nf, const int* pmap, const double* t,
                                 long t_stride, const double* y, const double* w, long w_stride, const double* X,
                                 const double* Pfix, double* f, double* J, const int* mask, hipStream_t s) {
  if (n < 1 || n > MODEL_ROWS || nf < 1 || nf > n) return hipErrorInvalidValue;
  ModelMapArgs A;
  fill_model_args(A, B, reps, m, n, t, t_stride, y, w, w_stride, X, f, J, mask);
  A.nf = nf; A.Pfix = Pfix;
  bool seen[MODEL_ROWS] = {};
  for (int j = 0; j < MODEL_ROWS; ++j) {
    int c = -1;
    if (j < n && pmap[j] >= 0) {
      if (pmap[j] >= nf) return hipErrorInvalidValue;
      c = seen[pmap[j]] ? MODEL_ROWS + pmap[j] : pmap[j];
      seen[pmap[j]] = true;
    }
    A.pm[j] = (signed char)c;
  }
  // per wave: the parameter vector, and the tile at nf | 1 when J is wanted
  const size_t wave_bytes = sizeof(double) * MODEL_ROWS * (size_t)(1 + (J ? (nf | 1) : 0));
  return launch_model_instance<true>(model, A, wave_bytes, s);
}

}  // namespace blsq
