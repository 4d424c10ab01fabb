// Robust loss functions for the trf / dogbox drivers (blsq_loss_*_dev, blsq_outer_set_loss).
//
// scipy.optimize.least_squares (1.15.3) grew `loss=` / `f_scale=` on top of the same drivers as the reference.  The
// loss changes only the INPUTS of a step (scipy: _lsq/common.py scale_for_robust_loss_function):
//   z = (f / f_scale)^2,  rho = (rho0, rho1, rho2)(z)  with rho0 *= f_scale^2, rho2 /= f_scale^2,
//   w = sqrt(max(rho1 + 2 rho2 f^2, EPS))   (a value below EPS is raised to EPS; NaN stays NaN)
//   J <- diag(w) J,   f_s = f * (rho1 / w),
// and the objective becomes f_scale^2 * sum rho0(z) (the library's convention: no 1/2, so 'linear' with f_scale = 1
// is ||f||^2, twice scipy's `cost`).  Everything downstream (Gram, certificate, tiers, step kernels) sees only the
// transformed J and f.
//
// Two kernels:
//   loss_cost_kernel   one workgroup per problem, a compensated (Neumaier) sum in a fixed order: a problem's bits
//                      depend on m and its own residuals only, never on B or its batch mates;
//   loss_scale_kernel  a streaming pass over the rows of J (B*m*n doubles read and written): the grid covers ROW
//                      CHUNKS of every problem, so one 250000 x 128 problem fills the chip as 1024 of 512 x 64 do.
//                      Each workgroup first computes w and f_s of its rows (w kept in LDS), then streams its
//                      contiguous J segment, four loads issued before any branch (a request behind a branch makes
//                      the compiler wait for every outstanding load at the join).
//
// Compiled with -ffp-contract=off: the formulas are evaluated operation by operation as written.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"

namespace blsq {

static constexpr int LOSS_NT = 256;
static constexpr int LOSS_MAX_ROWS = 1024;       // rows of one scale workgroup (LDS: 8 KiB of w)
static constexpr int LOSS_TARGET_ELEMS = 8192;   // J doubles per scale workgroup (64 KiB read + 64 KiB written)

// rho0 / rho1 / rho2 at z of the five losses (scipy's IMPLEMENTED_LOSSES, from their definitions):
//   linear  rho(z) = z
//   huber   rho(z) = z for z <= 1, 2 sqrt(z) - 1 otherwise
//   soft_l1 rho(z) = 2 (sqrt(1 + z) - 1)
//   cauchy  rho(z) = log(1 + z)
//   arctan  rho(z) = arctan(z)
__device__ __forceinline__ double loss_rho0(int loss, double z) {
  switch (loss) {
    case BLSQ_LOSS_HUBER: return (z <= 1.0) ? z : 2.0 * sqrt(z) - 1.0;
    case BLSQ_LOSS_SOFT_L1: return 2.0 * (sqrt(1.0 + z) - 1.0);
    case BLSQ_LOSS_CAUCHY: return log1p(z);
    case BLSQ_LOSS_ARCTAN: return atan(z);
    default: return z;
  }
}

__device__ __forceinline__ void loss_rho12(int loss, double z, double& r1, double& r2) {
  switch (loss) {
    case BLSQ_LOSS_HUBER:
      if (z <= 1.0) { r1 = 1.0; r2 = 0.0; }
      else { const double r = 1.0 / sqrt(z); r1 = r; r2 = -0.5 * (r / z); }     // z^-1/2, -z^-3/2 / 2
      break;
    case BLSQ_LOSS_SOFT_L1: {
      const double t = 1.0 + z, r = 1.0 / sqrt(t);
      r1 = r; r2 = -0.5 * (r / t);
      break;
    }
    case BLSQ_LOSS_CAUCHY: {
      const double t = 1.0 + z;
      r1 = 1.0 / t; r2 = -1.0 / (t * t);
      break;
    }
    case BLSQ_LOSS_ARCTAN: {
      const double t = 1.0 + z * z;
      r1 = 1.0 / t; r2 = (-2.0 * z) / (t * t);
      break;
    }
    default: r1 = 1.0; r2 = 0.0;
  }
}

__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// obj[b] = f_scale^2 * sum_i rho0((f_i / f_scale)^2)
__global__ __launch_bounds__(LOSS_NT) void loss_cost_kernel(int m, int loss, const double* __restrict__ fscale,
                                                            const double* __restrict__ f, double* __restrict__ obj,
                                                            const int* __restrict__ mask) {
  __shared__ double rs[LOSS_NT], rc[LOSS_NT];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (mask && mask[b] == 0) return;                 // uniform per workgroup
  const double fs = fscale[b];
  const double* fb = f + (long)b * m;
  double s = 0.0, c = 0.0;
  for (int i = tid; i < m; i += LOSS_NT) {
    const double q = fb[i] / fs;
    double e;
    two_sum(s, loss_rho0(loss, q * q), s, e);
    c += e;
  }
  rs[tid] = s; rc[tid] = c;
  __syncthreads();
  for (int h = LOSS_NT / 2; h > 0; h >>= 1) {       // fixed pairwise tree of (sum, compensation) pairs
    if (tid < h) {
      double t, e;
      two_sum(rs[tid], rs[tid + h], t, e);
      rs[tid] = t;
      rc[tid] = rc[tid] + rc[tid + h] + e;
    }
    __syncthreads();
  }
  if (tid == 0) obj[b] = (fs * fs) * (rs[0] + rc[0]);
}

// J rows of problem b, rows [r0, r0 + nr): J_i <- w_i J_i, fsc_i = f_i * (rho1_i / w_i).  VEC: n even, so a 16-byte
// pair never straddles two rows and every segment starts 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(LOSS_NT) void loss_scale_kernel(int m, int n, int loss, int rows, int chunks,
                                                             const double* __restrict__ fscale,
                                                             const double* __restrict__ f, double* __restrict__ J,
                                                             double* __restrict__ fsc, const int* __restrict__ mask) {
  __shared__ double wsh[LOSS_MAX_ROWS];
  const int b = blockIdx.x / chunks, r0 = (blockIdx.x - b * chunks) * rows, tid = threadIdx.x;
  if (mask && mask[b] == 0) return;                 // uniform per workgroup
  const int nr = min(rows, m - r0);
  const double fs = fscale[b], fs2 = fs * fs;
  const long row0 = (long)b * m + r0;
  for (int r = tid; r < nr; r += LOSS_NT) {
    const double fi = f[row0 + r];
    const double q = fi / fs, z = q * q;
    double r1, r2;
    loss_rho12(loss, z, r1, r2);
    r2 = r2 / fs2;
    double js = r1 + (2.0 * r2) * (fi * fi);
    if (js < DBL_EPS) js = DBL_EPS;
    const double w = sqrt(js);
    fsc[row0 + r] = fi * (r1 / w);
    wsh[r] = w;
  }
  __syncthreads();
  const unsigned un = (unsigned)n;
  if (VEC) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    v2d* seg = reinterpret_cast<v2d*>(J + row0 * n);
    const int L = (nr * n) >> 1;
    int k = tid;
    for (; k + 3 * LOSS_NT < L; k += 4 * LOSS_NT) {
      v2d v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = seg[k + u * LOSS_NT];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double w = wsh[(2u * (unsigned)(k + u * LOSS_NT)) / un];
        v[u].x = v[u].x * w; v[u].y = v[u].y * w;
        seg[k + u * LOSS_NT] = v[u];
      }
    }
    for (; k < L; k += LOSS_NT) {
      v2d v = seg[k];
      const double w = wsh[(2u * (unsigned)k) / un];
      v.x = v.x * w; v.y = v.y * w;
      seg[k] = v;
    }
  } else {
    double* seg = J + row0 * n;
    const int L = nr * n;
    int k = tid;
    for (; k + 3 * LOSS_NT < L; k += 4 * LOSS_NT) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = seg[k + u * LOSS_NT];
#pragma unroll
      for (int u = 0; u < 4; ++u) seg[k + u * LOSS_NT] = v[u] * wsh[(unsigned)(k + u * LOSS_NT) / un];
    }
    for (; k < L; k += LOSS_NT) seg[k] = seg[k] * wsh[(unsigned)k / un];
  }
}

hipError_t launch_loss_cost(int B, int m, int loss, const double* fscale, const double* f, double* obj,
                            const int* mask, hipStream_t s) {
  hipLaunchKernelGGL(loss_cost_kernel, dim3(B), dim3(LOSS_NT), 0, s, m, loss, fscale, f, obj, mask);
  return hipGetLastError();
}

hipError_t launch_loss_scale(int B, int m, int n, int loss, const double* fscale, const double* f, double* J,
                             double* fsc, const int* mask, hipStream_t s) {
  int rows = LOSS_TARGET_ELEMS / n;
  rows = rows < 1 ? 1 : (rows > LOSS_MAX_ROWS ? LOSS_MAX_ROWS : rows);
  if (rows > m) rows = m;
  const int chunks = (m + rows - 1) / rows;
  const long grid = (long)B * chunks;
  if (grid > 0x7fffffffL) return hipErrorInvalidValue;
  const bool vec = (n % 2 == 0) && ((reinterpret_cast<uintptr_t>(J) & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(loss_scale_kernel<true>, dim3((unsigned)grid), dim3(LOSS_NT), 0, s, m, n, loss, rows, chunks,
                       fscale, f, J, fsc, mask);
  else
    hipLaunchKernelGGL(loss_scale_kernel<false>, dim3((unsigned)grid), dim3(LOSS_NT), 0, s, m, n, loss, rows, chunks,
                       fscale, f, J, fsc, mask);
  return hipGetLastError();
}

}  // namespace blsq
