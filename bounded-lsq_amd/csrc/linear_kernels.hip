// Linear residuals for the device outer driver (blsq_linear_eval_dev): the callbacks of
//   min 1/2 |A x - y|^2,  lb <= x <= ub
// evaluated on the GPU, so that a bounded linear least-squares solve stays there like a fit of a built-in model:
//   f[q][i] = w_i (sum_j A[b][i][j] x[q][j] - y[b][i])        q = b * reps + r, r < reps
//   J[b]    = diag(w) A[b]                                     for every b with mask == nullptr or mask[b] != 0
// A is row-major [m][n], the layout of J; A_stride = m n (one matrix per problem) or 0 (ONE matrix for all problems: read
// through the same code with a zero stride, never broadcast on the host).
//
// Two kernels:
//   linear_f_kernel   one workgroup per point q and chunk of rows.  x[q] is staged in LDS once.  A row belongs to a
//                     GROUP of G consecutive lanes, G the smallest power of two >= min(n, 64): the lanes of a wave read
//                     consecutive addresses along j (for n <= 64 the 64 / G rows of a wave pass are contiguous too), so
//                     every load of A is coalesced, and a wave is full for small n as for large.
//                     Summation order, a function of n alone: lane g of the group runs acc = fma(A[i][j], x[j], acc)
//                     over j = g, g + G, g + 2 G, ... in ascending order from +0.0; the G partial sums are then added
//                     by the butterfly t = t + (t of lane ^ o) for o = G / 2, G / 4, ..., 1 (every lane of the group
//                     computes the same tree).  Nothing depends on B, reps, m, the strides or the batch mates: f for
//                     a shared A is, in every bit, f for the same matrix replicated.
//   linear_j_kernel   a streaming copy in 16-byte vectors (m n even and 16-byte aligned pointers; 8-byte otherwise).  A
//                     workgroup holds 1024 vectors of the matrix in registers; with a shared A it loads them ONCE and
//                     stores them into every unmasked problem of its share of the batch, with per-problem matrices
//                     it loads inside that loop.  Without w no arithmetic touches a value: the copy is exact in every
//                     bit.  With w each element is multiplied once by the weight of its row.  A problem with
//                     mask[b] == 0 is neither read nor written.
//
// Compiled with -ffp-contract=off (EXACT_SRCS): every fused operation of this file is spelled fma(), and J with weights
// is held to numpy's single multiply bit for bit, so the compiler must not be free to fuse anything else.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"

#include <algorithm>
#include <type_traits>

namespace blsq {

static constexpr int LIN_NT = 256;
static constexpr int LIN_XMAX = 1024;            // doubles of x a workgroup stages (n <= BLSQ_LINEAR_MAX_N < 1024)
static constexpr int LIN_F_PASSES = 4;           // row passes a residual workgroup is sized for
static constexpr int LIN_J_UNROLL = 4;           // vectors per thread of the copy
static_assert(BLSQ_LINEAR_MAX_N < LIN_XMAX, "x of one point fits the staging buffer");

// lg: log2 of the group size G (0 .. 6)
__global__ __launch_bounds__(LIN_NT) void linear_f_kernel(int m, int n, int reps, int lg, const double* __restrict__ A,
                                                          long A_stride, const double* __restrict__ y,
                                                          const double* __restrict__ w, long w_stride,
                                                          const double* __restrict__ X, double* __restrict__ f) {
  __shared__ double xs[LIN_XMAX];
  const int tid = threadIdx.x;
  const long q = blockIdx.x, b = q / reps;
  for (int j = tid; j < n; j += LIN_NT) xs[j] = X[q * n + j];
  __syncthreads();
  const int G = 1 << lg, R = LIN_NT >> lg;       // lanes per row, rows per pass
  const int g = tid & (G - 1), r = tid >> lg;
  const double* Ab = A + b * A_stride;
  // (the trip count is the same for every thread: all lanes reach the butterfly; the lanes of a group share their row)
  for (long i0 = (long)blockIdx.y * R; i0 < m; i0 += (long)gridDim.y * R) {
    const long i = i0 + r;
    double acc = 0.0;
    if (i < m) {
      const double* row = Ab + i * n;
      for (int j = g; j < n; j += G) acc = fma(row[j], xs[j], acc);
    }
    for (int o = G >> 1; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, WAVE);
    if (i < m && g == 0) {
      const double res = y ? acc - y[b * m + i] : acc;
      f[q * m + i] = w ? w[b * w_stride + i] * res : res;
    }
  }
}

typedef double lin_v2d __attribute__((ext_vector_type(2)));

// L: the vectors of one matrix (m n / 2 with VEC, m n without).  Vector k of the matrix: elements 2 k, 2 k + 1 (VEC) or k.
template <bool VEC, bool SHARED>
__global__ __launch_bounds__(LIN_NT) void linear_j_kernel(int B, long L, int n, const double* __restrict__ A,
                                                          const double* __restrict__ w, long w_stride,
                                                          double* __restrict__ J, const int* __restrict__ mask) {
  using T = typename std::conditional<VEC, lin_v2d, double>::type;
  constexpr int E = VEC ? 2 : 1;
  const long k0 = (long)blockIdx.x * (LIN_NT * LIN_J_UNROLL) + threadIdx.x;
  const long mn = L * E;                         // doubles of one matrix (VEC: m n is even)
  T v[LIN_J_UNROLL];
  long row[LIN_J_UNROLL][E];                     // with w: the row of every element this thread holds
  if (w) {
#pragma unroll
    for (int u = 0; u < LIN_J_UNROLL; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) row[u][e] = ((k0 + (long)u * LIN_NT) * E + e) / n;
  }
  if (SHARED) {
#pragma unroll
    for (int u = 0; u < LIN_J_UNROLL; ++u) {
      const long k = k0 + (long)u * LIN_NT;
      if (k < L) v[u] = reinterpret_cast<const T*>(A)[k];
    }
  }
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    if (mask && mask[b] == 0) continue;          // uniform per workgroup
    if (!SHARED) {
      const T* src = reinterpret_cast<const T*>(A + (long)b * mn);
#pragma unroll
      for (int u = 0; u < LIN_J_UNROLL; ++u) {
        const long k = k0 + (long)u * LIN_NT;
        if (k < L) v[u] = src[k];
      }
    }
    T* dst = reinterpret_cast<T*>(J + (long)b * mn);
    const double* wb = w ? w + (long)b * w_stride : nullptr;
#pragma unroll
    for (int u = 0; u < LIN_J_UNROLL; ++u) {
      const long k = k0 + (long)u * LIN_NT;
      if (k >= L) continue;
      T out = v[u];
      if (wb) {
        if constexpr (VEC) { out.x = wb[row[u][0]] * out.x; out.y = wb[row[u][1]] * out.y; }
        else out = wb[row[u][0]] * out;
      }
      dst[k] = out;
    }
  }
}

template <bool VEC, bool SHARED>
static hipError_t launch_linear_j(const LinearEvalCall& c, hipStream_t s) {
  const long mn = (long)c.m * c.n, L = VEC ? mn / 2 : mn;
  const long gx = (L + LIN_NT * LIN_J_UNROLL - 1) / (LIN_NT * LIN_J_UNROLL);
  if (gx > 0x7fffffffL) return hipErrorInvalidValue;
  // shared A: every workgroup loads its vectors once and walks over its share of the problems; enough workgroups to
  // fill the chip, no more.  Per-problem A: one problem per workgroup until the grid's second dimension is used up
  long gy = SHARED ? std::max(1L, 4096 / gx) : 65535;
  gy = std::min(std::min(gy, (long)c.B), 65535L);
  return launch<linear_j_kernel<VEC, SHARED>>(dim3((unsigned)gx, (unsigned)gy), dim3(LIN_NT), 0, s, c.B, L, c.n, c.A, c.w,
                                              c.w_stride, c.J, c.mask);
}

hipError_t launch_linear_eval(const LinearEvalCall& c, hipStream_t s) {
  if (c.B < 1 || c.reps < 1 || c.m < 1 || c.n < 1 || c.n > BLSQ_LINEAR_MAX_N) return hipErrorInvalidValue;
  const long mn = (long)c.m * c.n;
  if (!c.A || !c.X || (!c.f && !c.J) || (c.A_stride != 0 && c.A_stride != mn)) return hipErrorInvalidValue;
  if (c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  if (c.J && c.reps != 1) return hipErrorInvalidValue;
  if (c.f) {
    int lg = 0;
    while (lg < 6 && (1 << lg) < c.n) ++lg;
    const long Q = (long)c.B * c.reps;
    if (Q > 0x7fffffffL) return hipErrorInvalidValue;
    const int R = LIN_NT >> lg;
    const long chunks = ((long)c.m + R - 1) / R;
    const long gy = std::min((chunks + LIN_F_PASSES - 1) / LIN_F_PASSES, 65535L);
    const hipError_t e = launch<linear_f_kernel>(dim3((unsigned)Q, (unsigned)gy), dim3(LIN_NT), 0, s, c.m, c.n, c.reps,
                                                 lg, c.A, c.A_stride, c.y, c.w, c.w_stride, c.X, c.f);
    if (e != hipSuccess) return e;
  }
  if (c.J) {
    const bool vec = mn % 2 == 0 && ((reinterpret_cast<uintptr_t>(c.A) | reinterpret_cast<uintptr_t>(c.J)) & 15) == 0;
    const bool shared = c.A_stride == 0;
    if (vec) return shared ? launch_linear_j<true, true>(c, s) : launch_linear_j<true, false>(c, s);
    return shared ? launch_linear_j<false, true>(c, s) : launch_linear_j<false, false>(c, s);
  }
  return hipSuccess;
}

}  // namespace blsq
