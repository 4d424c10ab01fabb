// Triangular kernels on the n x n factor R (upper triangular, row-major, stride ld,
// resident in global memory / L2), executed by ONE workgroup of TRI_NT threads.
// Vectors live in LDS.  Used by the SVD-free trust-region path (lm_kernels.hip).
#pragma once
#include <type_traits>

#include "blsq_device.h"
#include "mv_ops.h"             // u = R s, u = R^T s: the matrix-vector family

namespace blsq {

// Sixteen LDS operands requested together and waited for ONCE: written as a plain loop the compiler emitted
// read -> wait -> fma sixteen times in a row (0.9 us per phase of a block step, tools/cert0_stamps.py).
// base: LDS byte address (per lane); element k is at base + 8 * STRIDE * k.
template <int STRIDE>
__device__ __forceinline__ void tri_lds16_issue(double (&v)[16], unsigned base) {
#define BLSQ_TRI_RD(K) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v[K]) : "v"(base), "n"(8 * STRIDE * (K)));
  if constexpr (8 * STRIDE * 15 < 65536) {
    BLSQ_TRI_RD(0) BLSQ_TRI_RD(1) BLSQ_TRI_RD(2) BLSQ_TRI_RD(3) BLSQ_TRI_RD(4) BLSQ_TRI_RD(5) BLSQ_TRI_RD(6) BLSQ_TRI_RD(7)
    BLSQ_TRI_RD(8) BLSQ_TRI_RD(9) BLSQ_TRI_RD(10) BLSQ_TRI_RD(11) BLSQ_TRI_RD(12) BLSQ_TRI_RD(13) BLSQ_TRI_RD(14) BLSQ_TRI_RD(15)
  }
#undef BLSQ_TRI_RD
}
// (run-time element stride, in doubles)
// (the address register is stepped inside the statement: sixteen separate addresses would be computed up front and
//  occupy sixteen registers; stride_bytes must be wave-uniform)
__device__ __forceinline__ void tri_lds16_issue_rt(double (&v)[16], unsigned base, unsigned stride_bytes) {
#pragma unroll
  for (int k = 0; k < 16; ++k)
    asm volatile("ds_read_b64 %0, %1\n\tv_add_u32 %1, %2, %1" : "=&v"(v[k]), "+v"(base) : "s"(stride_bytes));
}
__device__ __forceinline__ void tri_lds16_wait(double (&v)[16]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                 "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
}
__device__ __forceinline__ void tri_lds16_tie(double (&v)[16]) {       // (already waited for: pin behind that wait)
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                    "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
}

static constexpr int TRI_NT = 256;
static constexpr int TRI_NW = TRI_NT / WAVE;
// Every routine is a template on NT, the thread count of the calling workgroup (default TRI_NT): the fused
// Newton-round kernel of chol_reg.hip runs them with its 512 threads.

// invd[i] = 1 / R[i][i]
template <int NT = TRI_NT>
__device__ __forceinline__ void tri_invdiag(const double* R, int n, int ld, double* invd) {
  for (int i = threadIdx.x; i < n; i += NT) invd[i] = 1.0 / R[(long)i * ld + i];
  __syncthreads();
}

// In place: x <- R^{-1} x.  Blocked back substitution, 16-wide blocks: the diagonal
// block is solved by lanes 0..15 of wave 0 (lane i owns row i, x_s broadcast with
// v_readlane), the part above it is updated by all threads (one row each).
template <int NT = TRI_NT>
__device__ __forceinline__ void tri_solve_upper(const double* R, int n, int ld,
                                                const double* invd, double* x) {
  const int tid = threadIdx.x;
  const int nblk = (n + 15) / 16;
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int c0 = kb * 16;
    const int bs = (n - c0 < 16) ? n - c0 : 16;
    if (tid < 64) {                       // wave 0 (all 64 lanes run; lanes >= 16 are idle copies)
      const int i = tid & 15;
      double D[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {        // clamped unconditional loads, select afterwards
        const double val = R[(long)(c0 + ((i < bs) ? i : bs - 1)) * ld + c0 + ((s < bs) ? s : bs - 1)];
        D[s] = (i < bs && s < bs && s > i) ? val : 0.0;
      }
      double r = (i < bs) ? x[c0 + i] : 0.0;
      const double iv = (i < bs) ? invd[c0 + i] : 0.0;
#pragma unroll
      for (int s = 15; s >= 0; --s) {
        const double xs = read_lane(r * iv, s);       // x_s (0 for s >= bs)
        if (i < s) r = fma(-D[s], xs, r);
      }
      if (tid < bs) x[c0 + tid] = r * iv;
    }
    __syncthreads();
    for (int i = tid; i < c0; i += NT) {           // rows above the block
      const double* row = R + (long)i * ld + c0;
      double rv[16], acc = 0.0;             // unconditional (clamped) loads: a guarded load would
#pragma unroll                              // serialise into branch + load + wait per element
      for (int s = 0; s < 16; ++s) rv[s] = row[(s < bs) ? s : bs - 1];
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = fma(rv[s], (s < bs) ? x[c0 + s] : 0.0, acc);
      x[i] -= acc;
    }
    __syncthreads();
  }
}

// In place: y <- R^{-T} y.  Blocked forward substitution.
template <int NT = TRI_NT>
__device__ __forceinline__ void tri_solve_upper_t(const double* R, int n, int ld,
                                                  const double* invd, double* y) {
  const int tid = threadIdx.x;
  const int nblk = (n + 15) / 16;
  for (int kb = 0; kb < nblk; ++kb) {
    const int c0 = kb * 16;
    const int bs = (n - c0 < 16) ? n - c0 : 16;
    if (tid < 64) {
      const int i = tid & 15;               // row i of the lower-triangular block = column i of R's block
      double D[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double val = R[(long)(c0 + ((s < bs) ? s : bs - 1)) * ld + c0 + ((i < bs) ? i : bs - 1)];
        D[s] = (i < bs && s < bs && s < i) ? val : 0.0;
      }
      double r = (i < bs) ? y[c0 + i] : 0.0;
      const double iv = (i < bs) ? invd[c0 + i] : 0.0;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double ys = read_lane(r * iv, s);
        if (i > s) r = fma(-D[s], ys, r);
      }
      if (tid < bs) y[c0 + tid] = r * iv;
    }
    __syncthreads();
    for (int j = c0 + 16 + tid; j < n; j += NT) {   // columns to the right of the block
      double rv[16], acc = 0.0;             // 16 rows = 16 cache lines: all loads in flight together
#pragma unroll
      for (int s = 0; s < 16; ++s) rv[s] = R[(long)(c0 + ((s < bs) ? s : bs - 1)) * ld + j];
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = fma(rv[s], (s < bs) ? y[c0 + s] : 0.0, acc);
      y[j] -= acc;
    }
    __syncthreads();
  }
}

// ---- the same two solves with the operands prefetched by LDS-DMA ---------------------------
// R does not fit any cache level for a whole batch, so each 16-wide block step of the solves
// above pays HBM / MALL round trips for its diagonal block and its panel.  Here the operands of
// block step kb-1 (kb+1) stream global -> LDS (global_load_lds, no VGPR staging) while step kb
// computes from LDS; the barriers inside the loop are LDS-only so the DMA stays in flight.
// buf: 2 * 16 * ld doubles of LDS.  R rows must be 16-byte aligned (ld % 2 == 0).

// rows 0 .. c0+15, columns c0 .. c0+15  ->  dst[row * 16 + col - c0]   (W0: the first W0 waves issue nothing)
template <int NT = TRI_NT, int W0 = 0>
__device__ __forceinline__ void tri_pf_issue_upper(const double* R, int ld, int c0, double* dst, int tid) {
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6) - W0;
  if (W0 > 0 && w < 0) return;
  const int nrow = c0 + 16;                              // multiple of 16: whole 8-row DMA pieces
  // A panel row is 128 bytes: one row per thread, every thread at the same column, is a 32-way bank conflict in the
  // plain row-major image (1.2 us of a block step at 240 rows).  The DMA writes 1 KB of LDS per instruction in lane
  // order, but WHICH 16-byte piece a lane fetches is free: piece (row r, column pair c) of the 8-row block g goes to
  // slot ((r ^ (g & 1)) * 8 + (c ^ r)) of the block — sixteen consecutive rows then hit sixteen different 4-bank
  // groups at every column pair (tri_pf_upper_read16 below undoes it).
  for (int r0 = w * 8; r0 < nrow; r0 += (NT / WAVE - W0) * 8) {
    const int g1 = (r0 >> 3) & 1;
    const int r = (lane >> 3) ^ g1, c = (lane & 7) ^ r;
    glds16(R + c0, (unsigned)((r0 + r) * ld + 2 * c) * 8u, dst + r0 * 16);
  }
}
// the sixteen entries of panel row `row` (staged by tri_pf_issue_upper) as eight 16-byte reads: issue, then
// tri_pf_upper_wait (the registers hold nothing before it), which also unpacks into v
typedef double tri_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void tri_pf_upper_issue(tri_v2d (&t)[8], const double* b, int row) {
  const int r = row & 7, g1 = (row >> 3) & 1;
  const unsigned blk = lds_addr(b) + 8u * (unsigned)((row & ~7) * 16) + 128u * (unsigned)(r ^ g1);
#define BLSQ_TRI_RD2(C) asm volatile("ds_read_b128 %0, %1" : "=v"(t[C]) : "v"(blk + 16u * (unsigned)((C) ^ r)));
  BLSQ_TRI_RD2(0) BLSQ_TRI_RD2(1) BLSQ_TRI_RD2(2) BLSQ_TRI_RD2(3) BLSQ_TRI_RD2(4) BLSQ_TRI_RD2(5) BLSQ_TRI_RD2(6) BLSQ_TRI_RD2(7)
#undef BLSQ_TRI_RD2
}
__device__ __forceinline__ void tri_pf_upper_wait(tri_v2d (&t)[8], double (&v)[16]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
#pragma unroll
  for (int c = 0; c < 8; ++c) { v[2 * c] = t[c][0]; v[2 * c + 1] = t[c][1]; }
}
// rows c0 .. c0+15, columns c0 .. ld-1  ->  dst[s * (ld - c0) + col - c0]
template <int NT = TRI_NT, int W0 = 0>
__device__ __forceinline__ void tri_pf_issue_lower(const double* R, int ld, int c0, double* dst, int tid) {
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6) - W0;
  if (W0 > 0 && w < 0) return;
  const int L = ld - c0;                                 // multiple of 16
  const int half = L >> 1;                               // 16-byte pieces per row
  const int total = 16 * half;                           // multiple of 64
  for (int i0 = w * 64; i0 < total; i0 += (NT / WAVE - W0) * 64) {
    const int idx = i0 + lane;
    const int srow = idx / half, off = idx - srow * half;
    glds16(R + c0, (unsigned)((c0 + srow) * ld + 2 * off) * 8u, dst + i0 * 2);
  }
}

// Per-row hook of the backward solve: a caller that wants something else from the panel while it is in LDS (the row sums
// of the certificate's stage 0, cert_kernels.hip) passes an object with these members; TriNoHook does nothing.
//   block(slot, c0)           request (LDS reads, not waited for) what rows will need for columns c0 .. c0+15; slot 0 | 1:
//                             the look-ahead's wave 0 has two column blocks in hand per step
//   ready()                   the solver has waited for its own LDS reads (s_waitcnt lgkmcnt(0)): pin the requested values
//   row(slot, i, rv, c0, bs)  row i's sixteen entries of columns c0 .. c0+bs-1 (rv as stored: no sign, no mask), once per
//                             column block and row i <= c0 + 15; per row, the blocks in the order of the solve
//   stamp(kb, k)              diagnostic builds: phase k of block step kb
struct TriNoHook {
  static constexpr bool active = false;
  __device__ __forceinline__ void block(int, int) {}
  __device__ __forceinline__ void ready() {}
  __device__ __forceinline__ void row(int, int, const double (&)[16], int, int) {}
  __device__ __forceinline__ void stamp(int, int) {}
};

// Lane i's share of the diagonal block at c0, straight from global memory: row c0+i (128 bytes) / column c0+i (coalesced
// across the lanes).  Address-space-1 pointers: global_load, not flat_load (which would count on lgkmcnt as well).
__device__ __forceinline__ void tri_diag_row(double (&v)[16], const double* R, int ld, int c0, int i) {
  typedef __attribute__((address_space(1))) const char gchar_t;
  typedef __attribute__((address_space(1))) const tri_v2d gv2d_t;
  gchar_t* base = (gchar_t*)(R + (long)c0 * ld + c0);
  const unsigned off = 8u * (unsigned)(i * ld);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const tri_v2d t = *(gv2d_t*)(base + off + 16u * (unsigned)c);
    v[2 * c] = t[0]; v[2 * c + 1] = t[1];
  }
}
__device__ __forceinline__ void tri_diag_col(double (&v)[16], const double* R, int ld, int c0, int i) {
  typedef __attribute__((address_space(1))) const char gchar_t;
  typedef __attribute__((address_space(1))) const double gdbl_t;
  gchar_t* p = (gchar_t*)(R + (long)c0 * ld + c0) + 8u * (unsigned)i;
  const long stride = 8L * ld;                           // (one 64-bit add per row, not a multiplication)
#pragma unroll
  for (int s = 0; s < 16; ++s) { v[s] = *(gdbl_t*)p; p += stride; }
}

// CMP: the COMPARISON matrix M(R) instead of R (diagonal as it is, off-diagonal entries -|r_ij|): for a non-negative
// right-hand side the solution is entrywise >= |R^-1| rhs (Higham, ASNA 8.2) — the certificate's stage 0.
//
// Two schedules of the same arithmetic.  *_pf_ref: per block step wave 0 substitutes, THEN everybody updates the rows
// above — three barriers per step.  *_pf_la (look-ahead): wave 0 updates the sixteen rows of the NEXT diagonal block first
// and substitutes it while the other waves update the rest with the block just solved — one barrier per step.  Every
// entry of x receives the same operations in the same order in both (per block acc = fma(r_s, x_s, acc), s = 0 .. 15,
// from acc = 0, then x -= acc; blocks in kb order; the same substitution chain): bit-identical, tests compare them.
// tri_solve_upper_pf / tri_solve_upper_t_pf choose by `ref` (Options::tri_ref), a workgroup-uniform value.
template <int NT = TRI_NT, bool CMP = false, class Hook = TriNoHook>
__device__ __forceinline__ void tri_solve_upper_pf_ref(const double* R, int n, int ld, const double* invd, double* x,
                                                       double* buf, Hook hook = Hook()) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));                          // (no lane offset of this solve is kept in a register outside it)
  const int nblk = (n + 15) / 16;
  const int bsz = 16 * ld;
  int cur = 0;
  __builtin_amdgcn_s_waitcnt(0x0F70);
  tri_pf_issue_upper<NT>(R, ld, (nblk - 1) * 16, buf, tid);
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int c0 = kb * 16;
    const int bs = (n - c0 < 16) ? n - c0 : 16;
    const double* b = buf + cur * bsz;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();                                       // every wave's pieces have landed
    if (kb > 0) tri_pf_issue_upper<NT>(R, ld, c0 - 16, buf + (cur ^ 1) * bsz, tid);
    if (tid < 64) {                                      // wave 0 (lanes >= 16 are idle copies)
      const int i = tid & 15;
      double D[16], bv[16];
      tri_v2d bt[8];
      tri_pf_upper_issue(bt, b, c0 + i);
      hook.block(0, c0);
      double r = (i < bs) ? x[c0 + i] : 0.0;
      const double iv = (i < bs) ? invd[c0 + i] : 0.0;
      tri_pf_upper_wait(bt, bv);
      hook.ready();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double val = CMP ? -fabs(bv[s]) : bv[s];
        D[s] = (i < bs && s < bs && s > i) ? val : 0.0;
      }
#pragma unroll
      for (int s = 15; s >= 0; --s) {
        const double xs = read_lane(r * iv, s);
        if (i < s) r = fma(-D[s], xs, r);
      }
      if (tid < bs) { x[c0 + tid] = r * iv; hook.row(0, c0 + tid, bv, c0, bs); }
    }
    lds_barrier();
    if (tid < c0) {                                      // rows above the block
      double xv[16];
      tri_lds16_issue<1>(xv, lds_addr(x) + 8u * (unsigned)c0);
      hook.block(0, c0);
      for (int i = tid; i < c0; i += NT) {
        double rv[16];
        tri_v2d rt[8];
        tri_pf_upper_issue(rt, b, i);
        tri_pf_upper_wait(rt, rv);
        tri_lds16_tie(xv);
        hook.ready();
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(rv[s]) : rv[s], (s < bs) ? xv[s] : 0.0, acc);
        x[i] -= acc;
        hook.row(0, i, rv, c0, bs);
      }
    }
    lds_barrier();
    cur ^= 1;
  }
}

template <int NT = TRI_NT, bool CMP = false>
__device__ __forceinline__ void tri_solve_upper_t_pf_ref(const double* R, int n, int ld,
                                                         const double* invd, double* y, double* buf) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));                          // (no lane offset of this solve is kept in a register outside it)
  const int nblk = (n + 15) / 16;
  const int bsz = 16 * ld;
  int cur = 0;
  __builtin_amdgcn_s_waitcnt(0x0F70);
  tri_pf_issue_lower<NT>(R, ld, 0, buf, tid);
  for (int kb = 0; kb < nblk; ++kb) {
    const int c0 = kb * 16;
    const int bs = (n - c0 < 16) ? n - c0 : 16;
    const int L = ld - c0;
    const double* b = buf + cur * bsz;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if (kb + 1 < nblk) tri_pf_issue_lower<NT>(R, ld, c0 + 16, buf + (cur ^ 1) * bsz, tid);
    if (tid < 64) {
      const int i = tid & 15;               // row i of the lower-triangular block = column i of R's block
      double D[16], bv[16];
      tri_lds16_issue_rt(bv, lds_addr(b) + 8u * (unsigned)i, 8u * (unsigned)L);
      double r = (i < bs) ? y[c0 + i] : 0.0;
      const double iv = (i < bs) ? invd[c0 + i] : 0.0;
      tri_lds16_wait(bv);
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double val = CMP ? -fabs(bv[s]) : bv[s];
        D[s] = (i < bs && s < bs && s < i) ? val : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double ys = read_lane(r * iv, s);
        if (i > s) r = fma(-D[s], ys, r);
      }
      if (tid < bs) y[c0 + tid] = r * iv;
    }
    lds_barrier();
    if (c0 + 16 + tid < n) {                             // columns to the right of the block
      double yv[16];
      tri_lds16_issue<1>(yv, lds_addr(y) + 8u * (unsigned)c0);
      for (int j = c0 + 16 + tid; j < n; j += NT) {
        double cv[16];
        tri_lds16_issue_rt(cv, lds_addr(b) + 8u * (unsigned)(j - c0), 8u * (unsigned)L);
        tri_lds16_wait(cv);
        tri_lds16_tie(yv);
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(cv[s]) : cv[s], (s < bs) ? yv[s] : 0.0, acc);
        y[j] -= acc;
      }
    }
    lds_barrier();
    cur ^= 1;
  }
}

// ---- look-ahead schedule --------------------------------------------------------------------------------------------
// Iteration kb finds block kb solved and panel kb landed.  Wave 0 (lanes 0 .. 15; the others are idle copies) applies
// panel kb to the sixteen rows of block kb-1 and substitutes that block; waves 1 .. NT/64-1 apply it to the rows above
// (row -> thread fixed: row i belongs to thread 64 + i % (NT - 64)).  The two touch disjoint entries of x, so the one
// barrier at the top of the next iteration is all the synchronisation: it publishes x_blk(kb-1) and the rows above, and
// frees the other panel buffer for the DMA.  Every wave executes nblk + 1 barriers.
//   The diagonal block wave 0 substitutes belongs to a panel whose DMA has only just been issued, so wave 0 fetches it
// itself, from global memory into registers, one iteration ahead: the loads of block kb-2 are issued in front of the
// substitution chain of block kb-1, into the registers the masked copy of that block has just left, and are first used
// behind the row update of the next iteration.  Wave 0 takes no part in the panel DMA, so its vmcnt counts these loads
// alone and it does not wait at the top of an iteration.
//   x_blk(kb) stays in wave 0's registers: its row update broadcasts it with v_readlane, as the substitution does.
template <int NT = TRI_NT, bool CMP = false, class Hook = TriNoHook>
__device__ __forceinline__ void tri_solve_upper_pf_la(const double* R, int n, int ld, const double* invd, double* x,
                                                      double* buf, Hook hook = Hook()) {
  static_assert(NT >= 128 && NT % WAVE == 0, "look-ahead needs wave 0 and at least one wave for the rows above");
  constexpr int NB = NT - WAVE;                          // threads of the bulk update
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));                          // (... and no lane offset is kept in a register between solves)
  const bool w0 = tid < WAVE;                            // (wave-uniform)
  const int i = tid & 15;
  const int nblk = (n + 15) / 16;
  const int bsz = 16 * ld;
  int cur = 0;
  __builtin_amdgcn_s_waitcnt(0x0F70);
  double Dn[16];                                         // wave 0: row i of the diagonal block substituted next, as stored
  if (w0) tri_diag_row(Dn, R, ld, (nblk - 1) * 16, i);
  tri_pf_issue_upper<NT, 1>(R, ld, (nblk - 1) * 16, buf, tid);
  lds_barrier();                                         // x and invd as the caller's threads left them
  // wave 0: the 16 x 16 block at c0 (bs valid rows; kb its index) from Dn; r: the row's entry of x before it.
  // -> x_{c0+i} (0 for i >= bs)
  auto subst = [&](int kb, int c0, int bs, double r) -> double {
    const double iv = (i < bs) ? invd[c0 + i] : 0.0;
    tri_lds16_tie(Dn);                                   // (all sixteen stay registers of their own until here: the loads land behind the row update)
    if (tid < bs) hook.row(1, c0 + tid, Dn, c0, bs);
    double D[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double val = CMP ? -fabs(Dn[s]) : Dn[s];
      D[s] = (i < bs && s < bs && s > i) ? val : 0.0;
    }
    tri_lds16_tie(D);                                    // (Dn is free from here)
    if (kb >= 1) tri_diag_row(Dn, R, ld, c0 - 16, i);
#pragma unroll
    for (int s = 15; s >= 0; --s) {
      const double xs = read_lane(r * iv, s);
      if (i < s) r = fma(-D[s], xs, r);
    }
    if (tid < bs) x[c0 + tid] = r * iv;
    return r * iv;
  };
  double xk = 0.0;
  if (w0) {
    const int c0 = (nblk - 1) * 16, bs = n - c0;
    hook.block(1, c0);
    const double r = (i < bs) ? x[c0 + i] : 0.0;
    if (Hook::active) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    hook.ready();
    xk = subst(nblk - 1, c0, bs, r);
  }
  // Two loops with the same nblk - 1 barriers: wave 0's carries the diagonal block in registers, the other waves' does not
  // (one loop would keep those registers alive through the bulk update).
  if (w0) {
    for (int kb = nblk - 1; kb >= 1; --kb) {
      const int c0 = kb * 16;
      const int bs = (n - c0 < 16) ? n - c0 : 16;
      const double* b = buf + cur * bsz;
      hook.stamp(kb, 1);
      hook.stamp(kb, 2);
      lds_barrier();                                     // the rows above block kb and panel kb are visible
      hook.stamp(kb, 3);
      hook.stamp(kb, 4);
      // rows c0-16 .. c0-1 (a whole block): their update from panel kb, then their substitution
      double rv[16];
      tri_v2d rt[8];
      tri_pf_upper_issue(rt, b, c0 - 16 + i);
      hook.block(0, c0);
      hook.block(1, c0 - 16);
      double r = x[c0 - 16 + i];
      tri_pf_upper_wait(rt, rv);
      hook.ready();
      double acc = 0.0;
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(rv[s]) : rv[s], read_lane(xk, s), acc);   // (x_s: 0 for s >= bs)
      r -= acc;
      if (tid < 16) hook.row(0, c0 - 16 + tid, rv, c0, bs);
      asm volatile("" : "+v"(r));                        // (the row update is done before the block's registers are touched)
      hook.stamp(kb, 5);
      xk = subst(kb - 1, c0 - 16, 16, r);
      hook.stamp(kb, 6);
      cur ^= 1;
    }
  } else {
    for (int kb = nblk - 1; kb >= 1; --kb) {
      const int c0 = kb * 16;
      const int bs = (n - c0 < 16) ? n - c0 : 16;
      const double* b = buf + cur * bsz;
      hook.stamp(kb, 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of panel kb have landed
      hook.stamp(kb, 2);
      lds_barrier();                                     // x_blk(kb), the rows above it and panel kb are visible
      hook.stamp(kb, 3);
      tri_pf_issue_upper<NT, 1>(R, ld, c0 - 16, buf + (cur ^ 1) * bsz, tid);
      hook.stamp(kb, 4);
      if (tid - WAVE < c0 - 16) {                        // rows above block kb-1
        double xv[16];
        tri_lds16_issue<1>(xv, lds_addr(x) + 8u * (unsigned)c0);
        hook.block(0, c0);
        for (int r_ = tid - WAVE; r_ < c0 - 16; r_ += NB) {
          double rv[16];
          tri_v2d rt[8];
          tri_pf_upper_issue(rt, b, r_);
          tri_pf_upper_wait(rt, rv);
          tri_lds16_tie(xv);
          hook.ready();
          double acc = 0.0;
#pragma unroll
          for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(rv[s]) : rv[s], (s < bs) ? xv[s] : 0.0, acc);
          x[r_] -= acc;
          hook.row(0, r_, rv, c0, bs);
        }
      }
      hook.stamp(kb, 6);
      cur ^= 1;
    }
  }
  lds_barrier();                                         // x is complete for every thread
}

// The mirror image: row panels, kb ascending; wave 0 updates columns c0+16 .. c0+31 and substitutes block kb+1, the
// other waves update the columns to the right of it.  Lane i fetches COLUMN i of the next diagonal block (coalesced).
template <int NT = TRI_NT, bool CMP = false>
__device__ __forceinline__ void tri_solve_upper_t_pf_la(const double* R, int n, int ld, const double* invd, double* y,
                                                        double* buf) {
  static_assert(NT >= 128 && NT % WAVE == 0, "look-ahead needs wave 0 and at least one wave for the columns to the right");
  constexpr int NB = NT - WAVE;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const bool w0 = tid < WAVE;                            // (wave-uniform)
  const int i = tid & 15;               // row i of the lower-triangular block = column i of R's block
  const int nblk = (n + 15) / 16;
  const int bsz = 16 * ld;
  int cur = 0;
  __builtin_amdgcn_s_waitcnt(0x0F70);
  double Dn[16];                                         // wave 0: column i of the diagonal block substituted next
  if (w0) tri_diag_col(Dn, R, ld, 0, i);
  tri_pf_issue_lower<NT, 1>(R, ld, 0, buf, tid);
  lds_barrier();                                         // y and invd as the caller's threads left them
  // wave 0: block kb at c0 (bs valid columns) from Dn -> y_{c0+i} (0 for i >= bs)
  auto subst = [&](int kb, int c0, int bs, double r) -> double {
    const double iv = (i < bs) ? invd[c0 + i] : 0.0;
    tri_lds16_tie(Dn);
    double D[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double val = CMP ? -fabs(Dn[s]) : Dn[s];
      D[s] = (i < bs && s < bs && s < i) ? val : 0.0;
    }
    tri_lds16_tie(D);                                    // (Dn is free from here)
    if (kb + 1 < nblk) tri_diag_col(Dn, R, ld, c0 + 16, i);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double ys = read_lane(r * iv, s);
      if (i > s) r = fma(-D[s], ys, r);
    }
    if (tid < bs) y[c0 + tid] = r * iv;
    return r * iv;
  };
  double yk = 0.0;
  if (w0) {
    const int bs = (n < 16) ? n : 16;
    yk = subst(0, 0, bs, (i < bs) ? y[i] : 0.0);
  }
  if (w0) {                                              // (two loops, nblk - 1 barriers each, as above)
    for (int kb = 0; kb + 1 < nblk; ++kb) {
      const int c0 = kb * 16;                            // (block kb is a whole one: another follows it)
      const int L = ld - c0;
      const double* b = buf + cur * bsz;
      lds_barrier();                                     // the columns to the right of block kb and panel kb are visible
      // columns c0+16 .. c0+31 (block kb+1, bs1 of them inside the matrix): their update from panel kb, their substitution
      const int bs1 = (n - c0 - 16 < 16) ? n - c0 - 16 : 16;
      double cv[16];
      tri_lds16_issue_rt(cv, lds_addr(b) + 8u * (unsigned)(16 + i), 8u * (unsigned)L);
      double r = (i < bs1) ? y[c0 + 16 + i] : 0.0;
      tri_lds16_wait(cv);
      double acc = 0.0;
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(cv[s]) : cv[s], read_lane(yk, s), acc);
      if (i < bs1) r -= acc;
      asm volatile("" : "+v"(r));
      yk = subst(kb + 1, c0 + 16, bs1, r);
      cur ^= 1;
    }
  } else {
    for (int kb = 0; kb + 1 < nblk; ++kb) {
      const int c0 = kb * 16;
      const int L = ld - c0;
      const double* b = buf + cur * bsz;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();                                     // y_blk(kb), the columns to the right and panel kb are visible
      tri_pf_issue_lower<NT, 1>(R, ld, c0 + 16, buf + (cur ^ 1) * bsz, tid);
      if (c0 + 32 + tid - WAVE < n) {                    // columns to the right of block kb+1
        double yv[16];
        tri_lds16_issue<1>(yv, lds_addr(y) + 8u * (unsigned)c0);
        for (int j = c0 + 32 + tid - WAVE; j < n; j += NB) {
          double cv[16];
          tri_lds16_issue_rt(cv, lds_addr(b) + 8u * (unsigned)(j - c0), 8u * (unsigned)L);
          tri_lds16_wait(cv);
          tri_lds16_tie(yv);
          double acc = 0.0;
#pragma unroll
          for (int s = 0; s < 16; ++s) acc = fma(CMP ? -fabs(cv[s]) : cv[s], yv[s], acc);
          y[j] -= acc;
        }
      }
      cur ^= 1;
    }
  }
  lds_barrier();                                         // y is complete for every thread
}

// ref != 0 (workgroup-uniform; Options::tri_ref): the three-barrier schedule
template <int NT = TRI_NT, bool CMP = false, class Hook = TriNoHook>
__device__ __forceinline__ void tri_solve_upper_pf(const double* R, int n, int ld, const double* invd, double* x,
                                                   double* buf, int ref, Hook hook = Hook()) {
  if (ref) tri_solve_upper_pf_ref<NT, CMP, Hook>(R, n, ld, invd, x, buf, hook);
  else tri_solve_upper_pf_la<NT, CMP, Hook>(R, n, ld, invd, x, buf, hook);
}
template <int NT = TRI_NT, bool CMP = false>
__device__ __forceinline__ void tri_solve_upper_t_pf(const double* R, int n, int ld, const double* invd, double* y,
                                                     double* buf, int ref) {
  if (ref) tri_solve_upper_t_pf_ref<NT, CMP>(R, n, ld, invd, y, buf);
  else tri_solve_upper_t_pf_la<NT, CMP>(R, n, ld, invd, y, buf);
}

template <int NT = TRI_NT>
__device__ __forceinline__ double tri_dot(const double* a, const double* b, int n, double* red) {
  double acc = 0.0;
  for (int j = threadIdx.x; j < n; j += NT) acc = fma(a[j], b[j], acc);
  return block_sum(acc, red);
}

}  // namespace blsq
