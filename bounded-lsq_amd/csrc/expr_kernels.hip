// Expression models interpreted on the device (blsq_expr_eval_dev).
//
// The model is a straight-line program of at most 64 ops compiled on the host from the user's formula
// (bounded_lsq/_expr.py, whose numpy interpreter IS the definition; include/blsq.h has the format).  For the points
// X [Q][nf], Q = B * reps, q = b * reps + r:
//   f[q][i]    = w[b][i] * (v - y[b][i])                    v: the value of the program's root for row i
//   J[q][i][k] = w[b][i] * d v / d X[q][k]                  (reps == 1)
// The forward sweep computes val[k] for k ascending; the reverse sweep pushes adjoints for k descending and leaves the
// exact row of J.  Every operation is the definition's, in its order; the file is compiled with -ffp-contract=off
// (EXACT_SRCS) and spells no fma(), so the device differs from numpy in the last bits of exp, log, sin, cos, atan, erf,
// erfc and pow only, and a program without those is numpy bit for bit.
//
// Shape.  One wave per workgroup (no barrier between waves); a work item is 64 consecutive rows of one point q, a lane
// owns row i, as in model_kernels.hip.  The program and its constants travel by value in the kernel arguments (about
// 0.9 KB), as the composite table does: the loop counter is wave-uniform, so the fetch of an op word, the switch on its
// opcode, the decode of its operands and the reads of a VAR (X), a PFIX (Pfix) or a CONST run on scalar loads and scalar
// branches.  A lane loads its at most four coordinates once into registers and selects among them by a compare chain,
// never by an indexed array: no scratch.
// LDS (dynamic, through launch<>): the tape val[op][lane], then (with J) the adjoints adj[slot][lane] of the ops that
// depend on a variable and the wave's J tile at row stride nf | 1: 512 (nops + nact + (nf | 1)) bytes with J, 512 nops
// without.  In [op][lane] order the lanes of a wave fall on consecutive 8-byte addresses: no bank conflict; the tile's
// odd stride is the model kernel's, and so is the stream-out: consecutive lanes on consecutive addresses of the
// contiguous block J[q][r0 .. r0 + nr).  Which ops depend on a variable is derived by the launcher (a 64-bit mask in
// the arguments; the adjoint slot of op k is the number of set bits below k).
// POISSON and OMIT are template flags for the reason given for POISSON in model_kernels.hip: the plain instance does not
// carry the transform's registers or the branch.  An omitted row writes +0.0 into its slots and evaluates nothing.
// Nothing is checked on the device: the launcher refuses every program whose operands could leave the tape, the
// arguments or the tile.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "blsq_launch.h"
#include "poisson_rc.h"

namespace blsq {

static constexpr int EXPR_ROWS = 64;                  // rows of one work item: one per lane
static constexpr double EXPR_TWO_BY_SQRT_PI = 1.1283791670955126;
static_assert(BLSQ_EXPR_MAX_OPS == 64, "the mask of the ops that depend on a variable is one 64-bit word");
static_assert(BLSQ_MODEL_MAX_N <= 255 && BLSQ_EXPR_MAX_OPS <= 256 && BLSQ_EXPR_MAX_CONST <= 256, "an index is a byte");

struct ExprArgs {
  int m, nf, npfix, ncoord, reps, tiles, nops, root;
  long items;                   // Q * tiles
  const double* t; long t_stride;
  const double* y;
  const double* w; long w_stride;
  const double* X;
  const double* Pfix;
  double* f;
  double* J;
  const int* mask;
  unsigned long long active;    // bit k: op k depends on a variable
  unsigned long long ops[BLSQ_EXPR_MAX_OPS];
  double consts[BLSQ_EXPR_MAX_CONST];
};

// What a lane needs to read an operand: everything but `lane` and the coordinates is wave-uniform.
struct ExprLane {
  const double* val;            // the tape, [op][lane]
  const double* x;              // X[q]
  const double* pfix;           // Pfix[b]
  double c0, c1, c2, c3;        // the coordinates of the row
  int lane;
};

__device__ __forceinline__ double expr_fetch(const ExprArgs& A, const ExprLane& L, unsigned o) {
  const unsigned kind = o >> 8, i = o & 0xffu;
  switch (kind) {
    case BLSQ_EXPR_TAPE: return L.val[i * EXPR_ROWS + L.lane];
    case BLSQ_EXPR_VAR: return L.x[i];
    case BLSQ_EXPR_PFIX: return L.pfix[i];
    case BLSQ_EXPR_CONST: return A.consts[i];
    default: return i == 0 ? L.c0 : i == 1 ? L.c1 : i == 2 ? L.c2 : L.c3;
  }
}

__device__ __forceinline__ bool expr_two_operands(unsigned opc) { return opc <= BLSQ_EXPR_DIV || opc == BLSQ_EXPR_POWC; }

// dst = dst + c for a TAPE operand whose op depends on a variable (its adjoint) or a VAR (its column); dropped otherwise
__device__ __forceinline__ bool expr_takes_push(unsigned long long active, unsigned o) {
  const unsigned kind = o >> 8;
  return kind == BLSQ_EXPR_VAR || (kind == BLSQ_EXPR_TAPE && ((active >> (o & 0xffu)) & 1ull));
}
__device__ __forceinline__ void expr_push(unsigned long long active, double* adj, double* row, int lane, unsigned o,
                                          double c) {
  const unsigned i = o & 0xffu;
  if ((o >> 8) == BLSQ_EXPR_VAR) {
    row[i] = row[i] + c;
  } else {
    double* d = adj + __builtin_popcountll(active & ((1ull << i) - 1ull)) * EXPR_ROWS + lane;
    *d = *d + c;
  }
}

template <bool POISSON, bool OMIT>
__global__ __launch_bounds__(EXPR_ROWS) void expr_eval_kernel(ExprArgs A) {
  extern __shared__ double expr_lds[];
  const int lane = threadIdx.x;
  const long item = blockIdx.x;
  const long q = item / A.tiles;
  const int r0 = (int)(item - q * A.tiles) * EXPR_ROWS;
  const long b = q / A.reps;
  if (A.mask && A.mask[b] == 0) return;                 // a masked problem is left untouched (uniform: one wave)
  const int m = A.m, nf = A.nf, nops = A.nops, ld = nf | 1;
  const unsigned long long active = A.active;
  const int nact = __builtin_popcountll(active);
  const int nr = min(EXPR_ROWS, m - r0);
  double* val = expr_lds;
  double* adj = val + nops * EXPR_ROWS;
  double* tile = adj + nact * EXPR_ROWS;                // (neither is touched without J)
  if (lane < nr) {
    const int i = r0 + lane;
    double* row = tile + lane * ld;
    bool omitted = false;
    if constexpr (OMIT) {                  // a NaN in y leaves the row out: zeros, and nothing of the row is read
      const double yi = A.y[b * m + i];
      omitted = yi != yi;
      if (omitted) {
        if (A.J)
          for (int k = 0; k < nf; ++k) row[k] = 0.0;
        if (A.f) A.f[q * m + i] = 0.0;
      }
    }
    if (!omitted) {
      const double* tb = A.t + b * A.t_stride + i;
      ExprLane L;
      L.val = val; L.x = A.X + q * nf; L.pfix = A.Pfix + b * A.npfix; L.lane = lane;
      L.c0 = tb[0];
      L.c1 = A.ncoord > 1 ? tb[m] : 0.0;
      L.c2 = A.ncoord > 2 ? tb[2 * (long)m] : 0.0;
      L.c3 = A.ncoord > 3 ? tb[3 * (long)m] : 0.0;
      for (int k = 0; k < nops; ++k) {
        const unsigned long long op = A.ops[k];
        const unsigned opc = (unsigned)(op & 0xffu);
        const double va = expr_fetch(A, L, (unsigned)(op >> 8) & 0xffffu);
        double vb = 0.0;
        if (expr_two_operands(opc)) vb = expr_fetch(A, L, (unsigned)(op >> 24) & 0xffffu);
        double v;
        switch (opc) {
          case BLSQ_EXPR_ADD: v = va + vb; break;
          case BLSQ_EXPR_SUB: v = va - vb; break;
          case BLSQ_EXPR_MUL: v = va * vb; break;
          case BLSQ_EXPR_DIV: v = va / vb; break;
          case BLSQ_EXPR_NEG: v = -va; break;
          case BLSQ_EXPR_EXP: v = exp(va); break;
          case BLSQ_EXPR_LOG: v = log(va); break;
          case BLSQ_EXPR_SQRT: v = sqrt(va); break;
          case BLSQ_EXPR_SIN: v = sin(va); break;
          case BLSQ_EXPR_COS: v = cos(va); break;
          case BLSQ_EXPR_ATAN: v = atan(va); break;
          case BLSQ_EXPR_ERF: v = erf(va); break;
          case BLSQ_EXPR_ERFC: v = erfc(va); break;
          default: v = pow(va, vb); break;               // POWC
        }
        val[k * EXPR_ROWS + lane] = v;
      }
      const double v = expr_fetch(A, L, (unsigned)A.root);
      if (A.J) {
        for (int s = 0; s < nact; ++s) adj[s * EXPR_ROWS + lane] = 0.0;
        for (int k = 0; k < nf; ++k) row[k] = 0.0;
        if (expr_takes_push(active, (unsigned)A.root)) expr_push(active, adj, row, lane, (unsigned)A.root, 1.0);
        for (int k = nops - 1; k >= 0; --k) {
          if (!((active >> k) & 1ull)) continue;        // depends on no variable: nothing to push, and no adjoint
          const unsigned long long op = A.ops[k];
          const unsigned opc = (unsigned)(op & 0xffu);
          const unsigned oa = (unsigned)(op >> 8) & 0xffffu, ob = (unsigned)(op >> 24) & 0xffffu;
          const bool pa = expr_takes_push(active, oa), pb = expr_two_operands(opc) && expr_takes_push(active, ob);
          const double g = adj[__builtin_popcountll(active & ((1ull << k) - 1ull)) * EXPR_ROWS + lane];
          double ca = 0.0, cb = 0.0;                    // the contributions to a and b
          switch (opc) {
            case BLSQ_EXPR_ADD: ca = g; cb = g; break;
            case BLSQ_EXPR_SUB: ca = g; cb = -g; break;
            case BLSQ_EXPR_MUL:
              if (pa) ca = g * expr_fetch(A, L, ob);
              if (pb) cb = g * expr_fetch(A, L, oa);
              break;
            case BLSQ_EXPR_DIV: {
              const double vb = expr_fetch(A, L, ob);
              if (pa) ca = g / vb;
              if (pb) cb = -((g * val[k * EXPR_ROWS + lane]) / vb);
              break;
            }
            case BLSQ_EXPR_NEG: ca = -g; break;
            case BLSQ_EXPR_EXP: ca = g * val[k * EXPR_ROWS + lane]; break;
            case BLSQ_EXPR_LOG: ca = g / expr_fetch(A, L, oa); break;
            case BLSQ_EXPR_SQRT: ca = (0.5 * g) / val[k * EXPR_ROWS + lane]; break;
            case BLSQ_EXPR_SIN: ca = g * cos(expr_fetch(A, L, oa)); break;
            case BLSQ_EXPR_COS: ca = -(g * sin(expr_fetch(A, L, oa))); break;
            case BLSQ_EXPR_ATAN: {
              const double va = expr_fetch(A, L, oa);
              ca = g / (1.0 + va * va);
              break;
            }
            case BLSQ_EXPR_ERF: {
              const double va = expr_fetch(A, L, oa);
              ca = g * (EXPR_TWO_BY_SQRT_PI * exp(-(va * va)));
              break;
            }
            case BLSQ_EXPR_ERFC: {
              const double va = expr_fetch(A, L, oa);
              ca = -(g * (EXPR_TWO_BY_SQRT_PI * exp(-(va * va))));
              break;
            }
            default: {                                   // POWC: b is the constant exponent and takes no push
              const double va = expr_fetch(A, L, oa), c = expr_fetch(A, L, ob);
              ca = g * (c * pow(va, c - 1.0));
              break;
            }
          }
          if (pa) expr_push(active, adj, row, lane, oa, ca);
          if (pb) expr_push(active, adj, row, lane, ob, cb);
        }
      }
      if constexpr (POISSON) {
        double r, c;
        poisson_rc(v, A.y[b * m + i], r, c);
        if (A.f) A.f[q * m + i] = r;
        if (A.J)
          for (int k = 0; k < nf; ++k) row[k] = c * row[k];
      } else {
        const double wi = A.w ? A.w[b * A.w_stride + i] : 1.0;
        if (A.f) {
          const double r = A.y ? v - A.y[b * m + i] : v;
          A.f[q * m + i] = A.w ? wi * r : r;
        }
        if (A.J && A.w)
          for (int k = 0; k < nf; ++k) row[k] = wi * row[k];
      }
    }
  }
  if (A.J) {
    __syncthreads();                       // (one wave: the lanes' rows are visible to each other)
    // the wave's rows are the contiguous block J[q][r0 .. r0 + nr)[0 .. nf): lane l takes elements l, l + 64, ...
    double* out = A.J + (q * m + r0) * (long)nf;
    const int total = nr * nf;
    int row = lane / nf, col = lane - row * nf;
    const int drow = EXPR_ROWS / nf, dcol = EXPR_ROWS - drow * nf;
    for (int e = lane; e < total; e += EXPR_ROWS) {
      out[e] = tile[row * ld + col];
      row += drow; col += dcol;
      if (col >= nf) { col -= nf; ++row; }
    }
  }
}

// 0, or which argument of a program is the first bad one (EXPR_BAD_*; blsq_kernels.h): the list blsq_expr_check documents.
int expr_program_bad(int nops, const unsigned long long* ops, int root, int nconst, int nf, int npfix, int ncoord) {
  if (nops < 0 || nops > BLSQ_EXPR_MAX_OPS) return EXPR_BAD_NOPS;
  if (nops > 0 && !ops) return EXPR_BAD_OPS;
  if (nconst < 0 || nconst > BLSQ_EXPR_MAX_CONST) return EXPR_BAD_NCONST;
  if (nf < 1 || nf > BLSQ_MODEL_MAX_N) return EXPR_BAD_NF;
  if (npfix < 0 || npfix > BLSQ_MODEL_MAX_N) return EXPR_BAD_NPFIX;
  if (ncoord < 1 || ncoord > BLSQ_EXPR_MAX_COORD) return EXPR_BAD_NCOORD;
  auto operand_ok = [&](unsigned o, int earlier) {
    const int i = (int)(o & 0xffu);
    switch (o >> 8) {
      case BLSQ_EXPR_TAPE: return i < earlier;
      case BLSQ_EXPR_VAR: return i < nf;
      case BLSQ_EXPR_PFIX: return i < npfix;
      case BLSQ_EXPR_CONST: return i < nconst;
      case BLSQ_EXPR_COORD: return i < ncoord;
      default: return false;
    }
  };
  for (int k = 0; k < nops; ++k) {
    const unsigned long long op = ops[k];
    const unsigned opc = (unsigned)(op & 0xffu);
    const unsigned oa = (unsigned)(op >> 8) & 0xffffu, ob = (unsigned)(op >> 24) & 0xffffu;
    if (opc > BLSQ_EXPR_POWC || (op >> 40) != 0) return EXPR_BAD_OPS;
    if (!operand_ok(oa, k)) return EXPR_BAD_OPS;
    if (opc <= BLSQ_EXPR_DIV || opc == BLSQ_EXPR_POWC) {
      if (!operand_ok(ob, k)) return EXPR_BAD_OPS;
      if (opc == BLSQ_EXPR_POWC && (ob >> 8) != BLSQ_EXPR_CONST) return EXPR_BAD_OPS;
    }
  }
  if (root < 0 || root > 0xffff || !operand_ok((unsigned)root, nops)) return EXPR_BAD_ROOT;
  return 0;
}

// whether the program reads Pfix at all (a checked program)
bool expr_reads_pfix(int nops, const unsigned long long* ops, int root) {
  if ((root >> 8) == BLSQ_EXPR_PFIX) return true;
  for (int k = 0; k < nops; ++k) {
    const unsigned opc = (unsigned)(ops[k] & 0xffu);
    if (((ops[k] >> 16) & 0xffu) == BLSQ_EXPR_PFIX) return true;
    if ((opc <= BLSQ_EXPR_DIV || opc == BLSQ_EXPR_POWC) && ((ops[k] >> 32) & 0xffu) == BLSQ_EXPR_PFIX) return true;
  }
  return false;
}

hipError_t launch_expr_eval(const ExprEvalCall& c, hipStream_t s) {
  const bool poisson = c.est == BLSQ_EST_POISSON, omit = c.nan_policy == BLSQ_NAN_OMIT;
  if ((!poisson && c.est != BLSQ_EST_LSE) || (!omit && c.nan_policy != BLSQ_NAN_PROPAGATE)) return hipErrorInvalidValue;
  if (((poisson || omit) && !c.y) || (poisson && c.w)) return hipErrorInvalidValue;   // both read y; Poisson takes no w
  if (c.B < 1 || c.reps < 1 || c.m < 1) return hipErrorInvalidValue;
  if (expr_program_bad(c.nops, c.ops, c.root, c.nconst, c.nf, c.npfix, c.ncoord)) return hipErrorInvalidValue;
  if (c.nconst > 0 && !c.consts) return hipErrorInvalidValue;
  if (!c.t || !c.X || (!c.f && !c.J) || (c.J && c.reps != 1)) return hipErrorInvalidValue;
  if (c.t_stride != 0 && c.t_stride != (long)c.ncoord * c.m) return hipErrorInvalidValue;
  if (c.w && c.w_stride != 0 && c.w_stride != (long)c.m) return hipErrorInvalidValue;
  ExprArgs A;
  A.m = c.m; A.nf = c.nf; A.npfix = c.npfix; A.ncoord = c.ncoord; A.reps = c.reps; A.nops = c.nops; A.root = c.root;
  A.tiles = (c.m + EXPR_ROWS - 1) / EXPR_ROWS;
  A.items = (long)c.B * c.reps * A.tiles;
  A.t = c.t; A.t_stride = c.t_stride; A.y = c.y; A.w = c.w; A.w_stride = c.w ? c.w_stride : 0; A.X = c.X;
  A.Pfix = c.Pfix; A.f = c.f; A.J = c.J; A.mask = c.mask;
  if (!c.Pfix && expr_reads_pfix(c.nops, c.ops, c.root)) return hipErrorInvalidValue;
  A.active = 0;                                      // the ops that depend on a variable
  auto depends = [&](unsigned o) {
    return (o >> 8) == BLSQ_EXPR_VAR || ((o >> 8) == BLSQ_EXPR_TAPE && ((A.active >> (o & 0xffu)) & 1ull));
  };
  for (int k = 0; k < BLSQ_EXPR_MAX_OPS; ++k) {
    A.ops[k] = k < c.nops ? c.ops[k] : 0;
    if (k >= c.nops) continue;
    const unsigned opc = (unsigned)(A.ops[k] & 0xffu);
    bool dep = depends((unsigned)(A.ops[k] >> 8) & 0xffffu);
    if (opc <= BLSQ_EXPR_DIV || opc == BLSQ_EXPR_POWC) dep = depends((unsigned)(A.ops[k] >> 24) & 0xffffu) || dep;
    if (dep) A.active |= 1ull << k;
  }
  for (int k = 0; k < BLSQ_EXPR_MAX_CONST; ++k) A.consts[k] = k < c.nconst ? c.consts[k] : 0.0;
  if (A.items <= 0 || A.items > 0x7fffffffL) return hipErrorInvalidValue;
  const int nact = __builtin_popcountll(A.active);
  const size_t lds = sizeof(double) * EXPR_ROWS * (size_t)(c.nops + (c.J ? nact + (c.nf | 1) : 0));
  const dim3 g((unsigned)A.items), blk(EXPR_ROWS);
  if (poisson) return omit ? launch<expr_eval_kernel<true, true>>(g, blk, lds, s, A)
                           : launch<expr_eval_kernel<true, false>>(g, blk, lds, s, A);
  return omit ? launch<expr_eval_kernel<false, true>>(g, blk, lds, s, A)
              : launch<expr_eval_kernel<false, false>>(g, blk, lds, s, A);
}

}  // namespace blsq
