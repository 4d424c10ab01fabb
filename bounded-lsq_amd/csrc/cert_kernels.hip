// The conditioning certificate of the normal-equations path (the factor kernels are in chol_reg.hip and chol_rl.hip):
//
//   gram_cert0_kernel       stage 0, N > 80: the comparison-matrix bound from the factor kernel's share
//   gram_cond_kernel<NWP>   the norm stage: a PROVEN bound on kappa_2 from the explicit inverse
#include "gram_common.h"
#include "tri_ops.h"

namespace blsq {

#ifdef BLSQ_CHOL_STAMPS
static __device__ long long g_chol_st[4][20][8];       // this file's copy (chol_debug_stamps, chol_rl.hip)
#endif

// Per-row hook of the backward solve (tri_ops.h) for the one-pass form of stage 0: every row adds the panel's share of its
// sum_j |T_ij| dl_j (columns at and right of the diagonal) while the panel is in LDS.  Per row the contributions arrive in
// the order of the solve's blocks.  All LDS operands are requested before the first is used (read -> wait -> fma sixteen
// times in a row cost 0.9 us per phase, tools/cert0_stamps.py).
struct Cert0RowSums {
  static constexpr bool active = true;
  double* rowsB;                         // [NPAD] LDS, zeroed by the caller
  unsigned dl_addr;                      // LDS byte address of dl[0]
  bool stp;                              // diagnostic builds: this workgroup takes the stamps
  double dv[2][16];                      // dl of the column block(s) in hand
  __device__ __forceinline__ void block(int slot, int c0) {
    const unsigned db_ = dl_addr + 8u * (unsigned)c0;
    static_for<0, 16>([&](auto is) { constexpr int s_ = decltype(is)::value; lds_read64_off<8 * s_>(dv[slot][s_], db_); });
  }
  __device__ __forceinline__ void ready() {            // (the solver has waited for lgkmcnt(0))
    tri_lds16_tie(dv[0]);
    tri_lds16_tie(dv[1]);
  }
  __device__ __forceinline__ void row(int slot, int i, const double (&rv)[16], int c0, int bs) {
    double rs = 0.0;
#pragma unroll
    for (int s_ = 0; s_ < 16; ++s_)
      if (s_ < bs && c0 + s_ >= i) rs = fma(fabs(rv[s_]), dv[slot][s_], rs);
    rowsB[i] += rs;
  }
  __device__ __forceinline__ void stamp(int kb, int k) {
#ifdef BLSQ_CHOL_STAMPS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    CST(stp && (w == 0 || w == 2), w == 0 ? 1 : 2, kb, k);
#endif
  }
};

// ---- certificate, stage 0: the comparison-matrix bound (two triangular solves instead of an inverse) ----
// For triangular T, |T^-1| <= M(T)^-1 entrywise, M(T) the comparison matrix (diagonal |t_ii|, off-diagonal
// -|t_ij|; Higham, ASNA 8.2), so  ||R'^-1||_inf <= max_i (M(R')^-1 e)_i  and  ||R'^-1||_1 <= max_j (M(R')^-T e)_j :
// an O(n^2) PROVEN bound on the pair ||Y||_1 ||Y||_inf of the stage below, which needs the O(n^3) explicit
// inverse.  It grows like exp(sum of the off-diagonal mass), so it settles what is well conditioned by a margin
// (Gaussian 4096 x 256: 1600 against the inverse's 430; the bench's bounded problems) and leaves everything else
// to gram_cond_kernel, which then finds the problem flagged (cert_done) and leaves at once.  With R' = T diag(dl):
// M(R') z = e  <=>  M(T) w = e, z = w / dl;   M(R')^T y = e  <=>  M(T)^T y = 1 / dl.  All terms are non-negative
// (no cancellation; the result is inflated by 1e-9 for the rounding of <= 2 n additions per entry).
__global__ __launch_bounds__(TRI_NT, 3) void gram_cert0_kernel(GramCholArgs a) {
  extern __shared__ double sh[];
  __shared__ double red[32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // (GramCholArgs::unsettled: problems this launch does NOT finish — certified here AND through the rank gate's sure
  //  case, as the N <= 80 factor kernel counts them: zero means the rest of the gate has nothing to do)
  auto unsettle = [&]() { if (tid == 0 && a.unsettled) atomicAdd(a.unsettled, 1); };
  if (a.mask && a.mask[b] <= 1) { unsettle(); return; }
  if (a.fb_mask[b] != 0) { unsettle(); return; }        // already failed on a pivot
  const int NPAD = a.NPAD;
  const int n = a.ncols_dev ? a.ncols_dev[b] - 1 : a.n;
  if (n <= 0) { unsettle(); return; }
  const double* T = a.G + (long)b * NPAD * NPAD;
  double* x = sh;                        // [NPAD] M(T)^-1 e
  double* y = x + NPAD;                  // [NPAD] M(T)^-T (1 / dl)
  double* invd = y + NPAD;               // [NPAD]
  double* dl = invd + NPAD;              // [NPAD]
  double* pfbuf = dl + NPAD;             // [2 * 16 * NPAD] DMA staging of the solves
  double* rowsR = pfbuf;                 // [NPAD] row sums (after the solves: two workgroups per CU need <= 80 KB each)
  double* rowsB = pfbuf + 32 * NPAD;     // [NPAD] row sums gathered DURING the backward solve
  for (int j = tid; j < NPAD; j += TRI_NT) dl[j] = a.dsc[(long)b * NPAD + j];
  __syncthreads();
  const bool stp = b == 0; (void)stp;
  CST(stp && w == 0, 0, 18, 0);
  if (a.cert_ym && a.cert_ym[b] > 0.0) {
    // The factor kernel has done the transposed solve and the column sums on its way (GramCholArgs::cert_ym):
    // what is left is ONE pass over the factor — the backward solve M(T) x = e by column panels, each thread adding
    // the panel's share of its row's |T_ij| / ||J_j|| sum while the panel is in LDS.
    const double ym = a.cert_ym[b], r1 = a.cert_r1[b];
    CST(stp && w == 0, 0, 18, 1);
    tri_invdiag(T, n, NPAD, invd);
    for (int i = tid; i < NPAD; i += TRI_NT) { x[i] = 1.0; rowsB[i] = 0.0; }
    __syncthreads();
    CST(stp && w == 0, 0, 18, 2);
    // (the shared backward solve on the comparison matrix; Cert0RowSums adds the row sums while a panel is in LDS)
    tri_solve_upper_pf<TRI_NT, true, Cert0RowSums>(T, n, NPAD, invd, x, pfbuf, a.tri_ref,
                                                   Cert0RowSums{rowsB, lds_addr(dl), stp});
    CST(stp && w == 0, 0, 18, 3);
    double zm = 0.0, rinf = 0.0;
    for (int i = tid; i < n; i += TRI_NT) { zm = nanmax2(zm, x[i] / dl[i]); rinf = fmax(rinf, rowsB[i]); }
    zm = block_max(zm, red);
    rinf = block_max(rinf, red);
    const double kmax = a.k2_max > 0.0 ? a.k2_max : GRAM_K2_MAX;
    const double k2 = (r1 * rinf) * (zm * ym) * (1.0 + 1.0e-9);
    const bool passed = k2 <= kmax;                     // (NaN / inf fail)
    // for a problem left open: Lambda_0 for the third stage, or "hopeless" — lambda_min(C) <= min_j r'_jj^2 and
    // lambda_max(C) >= 1, so kappa_2(C) >= 1 / min_j r'_jj^2 (r'_jj = T_jj / ||J_j||: 1 / (invd_j / dl_j))
    double pinv = 0.0, emax = 0.0;
    if (a.cert_open && !passed) {
      const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
      for (int i = tid; i < n; i += TRI_NT) {
        const double t = invd[i] / dl[i];
        pinv = nanmax2(pinv, t * t);
        if (edv) emax = nanmax2(emax, fabs(edv[i]));
      }
      pinv = block_max(pinv, red);
      emax = block_max(emax, red);
    }
    if (tid == 0) {
      a.cert_done[b] = passed ? 1 : 0;
      if (passed) {
        if (a.k2_out) a.k2_out[b] = k2;
        if (a.lam_out) a.lam_out[b] = fmin(r1 * rinf, (double)n);
      }
      // TRF finish (GramCholArgs::lmfin): the `sure` branch of lm_gate_kernel, same expressions
      bool finished = false;
      if (a.lmfin.fast && passed && a.colinfo && a.lmfin.enable != 0 && a.lmfin.m >= n) {
        const double mn = a.colinfo[2 * (long)b], sm = a.colinfo[2 * (long)b + 1];
        const double smin_lb = GRAM_SMIN_PROVEN * mn, smax_ub = sqrt(sm);
        if (is_finite(sm) && sm > 0.0 && smin_lb > LM_GATE_MARGIN * DBL_EPS * a.lmfin.m * smax_ub) {
          a.lmfin.fast[b] = 1;
          a.lmfin.ncols_jac[b] = 0;
          a.lmfin.sc[(long)b * 16 + SC_SMAX] = smax_ub;
          a.lmfin.sc[(long)b * 16 + SC_SMIN] = smin_lb;
          a.lmfin.st[(long)b * 4 + ST_PHASE] = LM_IDLE;
          finished = true;
        }
      }
      if (!finished && a.unsettled) atomicAdd(a.unsettled, 1);
      CST(stp, 0, 18, 4);
      if (a.cert_open) {
        const double lam0 = fmin(r1 * rinf, (double)n);
        // kappa_2 >= pinv: beyond the gate the problem is hopeless.  Otherwise the note depends on what the system IS:
        // with a Coleman-Li block (E != 0: a variable near a bound in its descent direction) the comparison-matrix
        // bound fails long before the system is ill conditioned, and the norm stage settles such a problem more cheaply
        // than a factorisation (bench, bounded mix: certificate 0.26 against 0.36 ms); a pure Jacobian system (E = 0)
        // that fails it is usually near or beyond the gate, where the norm stage — 3.5 ... 13 of overestimate — cannot
        // decide and the third stage is where the problem ends up anyway (unbounded mix: 0.84 -> 0.56 ms).
        double note = 0.0;
        if (!passed && is_finite(lam0) && lam0 >= 1.0) {
          if (!(pinv <= kmax)) note = -1.0;
          else if (emax == 0.0) note = lam0;
        }
        a.cert_open[b] = note;
      }
    }
    return;
  }
  if (a.cert_open && tid == 0) a.cert_open[b] = 0.0;    // (four-pass form: the norm stage below keeps its own counsel)
  unsettle();                                           // (... and the rank gate's launch finishes what passes here)
  // the two comparison solves FIRST: ||R'||_1 ||R'||_inf >= lambda_max(C) >= 1, so a product of the two maxima
  // beyond the gate already decides "not settled here" and the norm passes are skipped
  tri_invdiag(T, n, NPAD, invd);
  for (int i = tid; i < n; i += TRI_NT) { x[i] = 1.0; y[i] = 1.0 / dl[i]; }
  __syncthreads();
  tri_solve_upper_pf<TRI_NT, true>(T, n, NPAD, invd, x, pfbuf, a.tri_ref);
  tri_solve_upper_t_pf<TRI_NT, true>(T, n, NPAD, invd, y, pfbuf, a.tri_ref);
  double zm = 0.0, ym = 0.0;
  for (int i = tid; i < n; i += TRI_NT) { zm = nanmax2(zm, x[i] / dl[i]); ym = nanmax2(ym, y[i]); }
  zm = block_max(zm, red);
  ym = block_max(ym, red);
  const double kmax = a.k2_max > 0.0 ? a.k2_max : GRAM_K2_MAX;
  if (!(zm * ym <= kmax)) {                             // (uniform; NaN / inf included)
    if (tid == 0) a.cert_done[b] = 0;
    return;
  }
  __syncthreads();                                      // (rowsR aliases the solves' staging)
  // ||R'||_1 (thread per column) and ||R'||_inf (wave per row), as gram_cond_kernel
  double r1 = 0.0;
  for (int j = tid; j < n; j += TRI_NT) {
    double sum = 0.0;
    for (int i0 = 0; i0 <= j; i0 += 32) {
      double rv[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) rv[u] = T[(long)((i0 + u <= j) ? i0 + u : j) * NPAD + j];
#pragma unroll
      for (int u = 0; u < 32; ++u) if (i0 + u <= j) sum += fabs(rv[u]);
    }
    r1 = fmax(r1, sum * dl[j]);
  }
  r1 = block_max(r1, red);
  for (int i0 = w; i0 < n; i0 += 4 * TRI_NW) {
    double rv[4][4], dv[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = (i0 + TRI_NW * q < n) ? i0 + TRI_NW * q : n - 1;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = i + lane + WAVE * c;
        const int jc = j < n ? j : n - 1;
        rv[q][c] = T[(long)i * NPAD + jc];
        dv[q][c] = dl[jc];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + TRI_NW * q;
      double sum = 0.0;
      for (int c = 0; c < 4; ++c)
        if (i < n && i + lane + WAVE * c < n) sum += fabs(rv[q][c]) * dv[q][c];
      // (n <= 256 per pass of four 64-lane chunks; wider rows: the remaining chunks)
      for (int j = i + lane + WAVE * 4; i < n && j < n; j += WAVE) sum += fabs(T[(long)i * NPAD + j]) * dl[j];
      sum = wave_sum(sum);
      if (lane == 0 && i < n) rowsR[i] = sum;
    }
  }
  __syncthreads();
  double rinf = 0.0;
  for (int i = tid; i < n; i += TRI_NT) rinf = fmax(rinf, rowsR[i]);
  rinf = block_max(rinf, red);
  const double k2 = (r1 * rinf) * (zm * ym) * (1.0 + 1.0e-9);
  const bool passed = k2 <= kmax;                       // (NaN / inf fail)
  if (tid == 0) {
    a.cert_done[b] = passed ? 1 : 0;
    if (passed) {
      if (a.k2_out) a.k2_out[b] = k2;
      if (a.lam_out) a.lam_out[b] = fmin(r1 * rinf, (double)n);
    }
  }
}

// ---- conditioning gate: a PROVEN bound on kappa_2 of the equilibrated system -----------------------
// The normal-equations path loses kappa_2(C) eps where C = R'^T R' is the equilibrated system matrix
// (unit diagonal) the step is solved from.  An estimate of sigma_min(R') by inverse iteration is a
// LOWER bound on ||R'^-1||, i.e. it can only err on the unsafe side.  This kernel computes an UPPER
// bound instead, from the explicit inverse:
//     Y = R'^-T   (lower triangular; 16 x 16 tiles by FP64 MFMA, the inverses of the diagonal tiles
//                  come from the Cholesky kernel:  Y_ii = R'_ii^-T,
//                  Y_ij = -R'_ii^-T sum_{k=j}^{i-1} R'_ki^T Y_kj   for j < i)
//     1 / lambda_min(C) = ||Y||_2^2 <= ||Y||_1 ||Y||_inf ,   lambda_max(C) = ||R'||_2^2 <= ||R'||_1 ||R'||_inf
//     K2 = ||R'||_1 ||R'||_inf ||Y||_1 ||Y||_inf  >=  kappa_2(C)
// (all four norms are exact sums of absolute values, accumulated in a fixed order) and keeps the
// problem on the normal-equations path only if K2 <= GRAM_K2_MAX.  DESIGN.md 3.0 has the error bound
// this gives for the step.  NWP waves work on one problem: 8 (a whole workgroup) or 1 (N <= 80: eight problems per
// workgroup, no workgroup barrier).
template <int NWP>
__global__ __launch_bounds__(GR_NT, 4) void gram_cond_kernel(GramCholArgs a) {
  constexpr int PT = WAVE * NWP;
  constexpr int PPW = GR_NW / NWP;
  constexpr int UMAX = (NWP == 8) ? 3 : 5;              // column tiles of a row block per wave
  extern __shared__ double sh_all[];
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int pslot = wv / NWP;
  const int pidx = (int)blockIdx.x * PPW + pslot;
  if (pidx >= a.count) return;                          // (NWP == 1 only: wave-uniform)
  const int b = pidx;
  const int tid = (int)threadIdx.x % PT, lane = tid & 63;
  const int w = wv % NWP;
  const int lr = lane >> 4, lc = lane & 15;
  if (a.mask && a.mask[b] <= 1) return;
  if (a.fb_mask[b] != 0) return;                        // already failed on a pivot
  if (a.cert_done && a.cert_done[b]) return;            // already proven inside the factor kernel (N <= 80)
  const int NPAD = a.NPAD;
  const int n = a.ncols_dev ? a.ncols_dev[b] - 1 : a.n;
  if (n <= 0) return;
  const int NTn = (n + 15) / 16;
  auto psync = [&]() {
    if (NWP == 8) __syncthreads();
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  };
  double* sh = sh_all + (size_t)pslot * (6 * (size_t)NPAD + 16 * NWP + 64);
  double* dl = sh;                      // [NPAD] column scales: R'[i][j] = T[i][j] dl[j]
  double* cs4 = dl + NPAD;              // [NPAD][4] column sums of |Y|, one slot per lane row
  double* rs = cs4 + 4 * NPAD;          // [NWP][16] row-sum partials of the current block row
  double* vals = rs + 16 * NWP;         // [64] reduction scratch
  double* rowsR = vals + 64;            // [NPAD] row sums of |R'|
  const double* T = a.G + (long)b * NPAD * NPAD;
  double* Y = a.ywork + (long)b * NPAD * NPAD;
  const double* Rinv = a.rinv + (long)b * (NPAD / 16) * 256;
  for (int j = tid; j < NPAD; j += PT) dl[j] = a.dsc[(long)b * NPAD + j];
  psync();
  auto reduce_max = [&](double v) -> double {           // max over the threads of this problem
    v = wave_max(v);
    if (NWP == 1) return v;
    psync();
    if (lane == 0) vals[w] = v;
    psync();
    double t = vals[0];
    for (int q = 1; q < NWP; ++q) t = fmax(t, vals[q]);
    return t;
  };
  // Stage 0 has been here (N > 80, GramCholArgs::cert_open): it could not settle the problem, but it left
  // Lambda_0 = min(||R'||_1 ||R'||_inf, n) >= lambda_max(C) — or the verdict "hopeless" from the smallest pivot.  The
  // explicit inverse below would only produce looser bounds than the shifted factorisation of the third stage proves
  // anyway: the problem goes there directly, with tau from Lambda = min(Lambda_0, ||C||_F) (one pass over the Gram).
  if constexpr (NWP == 8) {
    const double open0 = a.cert_open ? a.cert_open[b] : 0.0;
    if (open0 != 0.0) {
      const double kmax = a.k2_max > 0.0 ? a.k2_max : GRAM_K2_MAX;
      double lam = open0;
      if (open0 > 0.0 && a.cert_flag) {
        const int* gidx = a.gather ? a.gather + (long)b * a.stride_vec : nullptr;
        auto src = [&](int i) -> int { return gidx ? (i < n ? gidx[i] : a.n) : i; };
        const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;
        const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
        const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
        double* scl = cs4;                  // [NPAD] cs_j dl_j
        double* tdl = cs4 + NPAD;           // [NPAD] e_j^2 dl_j^2
        for (int j = tid; j < NPAD; j += PT) {
          const double cs = (csv && j < n) ? csv[j] : 1.0;
          const double ej = (edv && j < n) ? edv[j] : 0.0;
          scl[j] = cs * dl[j];
          tdl[j] = (ej * ej) * dl[j] * dl[j];
        }
        psync();
        double cf = 0.0;                    // this wave's share of ||C||_F^2 (fixed order)
        int q = 0;
        for (int j = 0; j < NTn; ++j) {
          for (int i = 0; i <= j; ++i, ++q) {
            if (q % NWP != w) continue;     // (wave-uniform)
            double c2 = 0.0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int row = 16 * i + lr + 4 * g, col = 16 * j + lc;
              double v = 0.0;
              if (row < n && col < n) {
                int sr_ = src(row), sc_ = src(col);
                if (sr_ > sc_) { const int t_ = sr_; sr_ = sc_; sc_ = t_; }
                v = Gs[(long)sr_ * NPAD + sc_] * scl[row] * scl[col];
                if (row == col) v += tdl[row];
              }
              c2 = fma(v, v, c2);
            }
            cf = fma((i == j) ? 1.0 : 2.0, wave_sum(c2), cf);
          }
        }
        psync();
        if (lane == 0) vals[w] = cf;
        psync();
        cf = 0.0;
        for (int qq = 0; qq < NWP; ++qq) cf += vals[qq];
        lam = fmin(lam, sqrt(cf));                        // lambda_max(C) <= ||C||_F
      }
      if (tid == 0) {
        if (a.k2_out) a.k2_out[b] = __builtin_inf();     // (no proven bound from here; the third stage writes k2_max)
        if (open0 > 0.0 && a.cert_flag && lam >= 1.0 && is_finite(lam)) {
          if (a.lam_out) a.lam_out[b] = lam;
          a.cert_tau[b] = lam / kmax;
          a.cert_flag[b] = 1;
        } else {
          a.fb_mask[b] = a.n + 1;
          if (a.path_out) a.path_out[b] = a.n + 1;
          { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }
        }
      }
      return;
    }
  }
  // ---- ||R'||_1 (thread per column) and ||R'||_inf (wave per row) ----
  double r1 = 0.0;
  for (int j = tid; j < n; j += PT) {
    // (32 rows of loads in flight per pass: the passes are serialised by their waits, and the longest
    //  column has n rows; same order of additions as a plain loop over the rows)
    double sum = 0.0;
    for (int i0 = 0; i0 <= j; i0 += 32) {
      double rv[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) rv[u] = T[(long)((i0 + u <= j) ? i0 + u : j) * NPAD + j];
#pragma unroll
      for (int u = 0; u < 32; ++u) if (i0 + u <= j) sum += fabs(rv[u]);
    }
    r1 = fmax(r1, sum * dl[j]);
  }
  r1 = reduce_max(r1);
  if constexpr (NWP == 1) {
    // one wave per problem: four rows at a time, one per 16-lane group (64 sequential wave
    // reductions at n = 64 were 20 of this kernel's 46 us)
    for (int i0 = 0; i0 < n; i0 += 4) {
      const int i = i0 + lr;
      double sum = 0.0;
      if (i < n)
        for (int j = i + lc; j < n; j += 16) sum += fabs(T[(long)i * NPAD + j]) * dl[j];
      sum = row16_sum(sum);
      if (lc == 0 && i < n) rowsR[i] = sum;
    }
  } else {
    // four rows of a wave per pass, their loads issued together (clamped, unconditional; n <= 256: at
    // most four 64-lane chunks per row); per lane the same additions in the same order as row by row
    for (int i0 = w; i0 < n; i0 += 4 * NWP) {
      double rv[4][4], dv[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (i0 + NWP * q < n) ? i0 + NWP * q : n - 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = i + lane + WAVE * c;
          const int jc = j < n ? j : n - 1;
          rv[q][c] = T[(long)i * NPAD + jc];
          dv[q][c] = dl[jc];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + NWP * q;
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i < n && i + lane + WAVE * c < n) sum += fabs(rv[q][c]) * dv[q][c];
        sum = wave_sum(sum);
        if (lane == 0 && i < n) rowsR[i] = sum;
      }
    }
  }
  psync();
  double rinf = 0.0;
  for (int i = tid; i < n; i += PT) rinf = fmax(rinf, rowsR[i]);
  rinf = reduce_max(rinf);
  // ---- Y = R'^-T by block rows; row and column sums of |Y| on the way ----
  double csum[UMAX];
#pragma unroll
  for (int u = 0; u < UMAX; ++u) csum[u] = 0.0;
  double rmax = 0.0;                                    // threads 0..15: max over block rows of "their" row
  for (int i = 0; i < NTn; ++i) {
    double rsum[4] = {0.0, 0.0, 0.0, 0.0};
    const double* Ri = Rinv + (long)i * 256;
    const double dli = dl[16 * i + lc];
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      const int j = w + NWP * u;
      if (j <= i) {
        v4d Yt = {0.0, 0.0, 0.0, 0.0};
        if (j == i) {
#pragma unroll
          for (int g = 0; g < 4; ++g) Yt[g] = Ri[lc * 16 + lr + 4 * g];         // (R'_ii^-1)^T
        } else {
          v4d acc = {0.0, 0.0, 0.0, 0.0};
          for (int k = j; k < i; ++k) {
            double av[4], bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const long ro = (long)(16 * k + 4 * s + lr) * NPAD;
              av[s] = T[ro + 16 * i + lc];
              bv[s] = Y[ro + 16 * j + lc];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma_f64(av[s] * dli, bv[s], acc);
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) Yt = mfma_f64(-Ri[(4 * s + lr) * 16 + lc], acc[s], Yt);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * i + lr + 4 * g, col = 16 * j + lc;
          const double v = (row < n && col < n) ? Yt[g] : 0.0;
          Y[(long)row * NPAD + col] = v;
          const double av_ = fabs(v);
          rsum[g] += row16_sum(av_);
          csum[u] += av_;
        }
      }
    }
    if (lc == 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) rs[w * 16 + lr + 4 * g] = rsum[g];
    }
    psync();                                            // row sums in LDS; Y row block i visible
    if (tid < 16) {
      double t = 0.0;
      for (int q = 0; q < NWP; ++q) t += rs[q * 16 + tid];
      rmax = fmax(rmax, t);
    }
    psync();
  }
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    const int j = w + NWP * u;
    if (j < NTn) cs4[(16 * j + lc) * 4 + lr] = csum[u];
  }
  psync();
  double y1 = 0.0;
  for (int c = tid; c < n; c += PT)
    y1 = fmax(y1, (cs4[4 * c] + cs4[4 * c + 1]) + (cs4[4 * c + 2] + cs4[4 * c + 3]));
  y1 = reduce_max(y1);
  const double yinf = reduce_max(tid < 16 ? rmax : 0.0);
  double k2 = (r1 * rinf) * (y1 * yinf);
  const double kmax = a.k2_max > 0.0 ? a.k2_max : GRAM_K2_MAX;
  double lam = fmin(r1 * rinf, (double)n);              // lambda_max(C) <= ||R'||_1 ||R'||_inf, <= trace(C) = n
  if (!(k2 <= kmax)) {                                   // (uniform over the problem's threads)
    // The 1- / inf-norm products overestimate kappa_2 by 10 ... 1000 (profiles/r02p_gate_calibration.txt).
    // Second, tighter proven bound for a problem they reject:  lambda_max(C) <= ||C||_F  and
    // 1 / lambda_min(C) = ||C^-1||_2 <= ||C^-1||_F  with  C^-1 = Y^T Y  formed tile by tile (MFMA; only
    // its sum of squares is kept) and C rebuilt from the source Gram with the Cholesky's own scalings.
    // Measured overestimate 4 ... 30 on the ill-conditioned families.  Sums in a fixed order.
    const int* gidx = a.gather ? a.gather + (long)b * a.stride_vec : nullptr;
    auto src = [&](int i) -> int { return gidx ? (i < n ? gidx[i] : a.n) : i; };
    const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;
    const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
    const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
    double* scl = cs4;                  // [NPAD] cs_j dl_j   (cs4 is free now)
    double* tdl = cs4 + NPAD;           // [NPAD] e_j^2 dl_j^2
    psync();
    for (int j = tid; j < NPAD; j += PT) {
      const double cs = (csv && j < n) ? csv[j] : 1.0;
      const double ej = (edv && j < n) ? edv[j] : 0.0;
      scl[j] = cs * dl[j];
      tdl[j] = (ej * ej) * dl[j] * dl[j];
    }
    psync();
    double cf = 0.0, zf = 0.0;          // this wave's share of ||C||_F^2 / ||C^-1||_F^2
    int q = 0;
    for (int j = 0; j < NTn; ++j) {
      for (int i = 0; i <= j; ++i, ++q) {
        if (q % NWP != w) continue;     // (wave-uniform)
        const double wgt = (i == j) ? 1.0 : 2.0;
        double c2 = 0.0;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * i + lr + 4 * g, col = 16 * j + lc;
          double v = 0.0;
          if (row < n && col < n) {
            int sr_ = src(row), sc_ = src(col);
            if (sr_ > sc_) { const int t_ = sr_; sr_ = sc_; sc_ = t_; }
            v = Gs[(long)sr_ * NPAD + sc_] * scl[row] * scl[col];
            if (row == col) v += tdl[row];
          }
          c2 = fma(v, v, c2);
        }
        for (int k = j; k < NTn; ++k) {
          double av[4], bv[4];
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) {
            const long ro = (long)(16 * k + 4 * s2 + lr) * NPAD;
            av[s2] = Y[ro + 16 * i + lc];
            bv[s2] = Y[ro + 16 * j + lc];
          }
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) acc = mfma_f64(av[s2], bv[s2], acc);
        }
        const double z2 = (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
        cf = fma(wgt, wave_sum(c2), cf);
        zf = fma(wgt, wave_sum(z2), zf);
      }
    }
    if (NWP > 1) {
      psync();
      if (lane == 0) { vals[w] = cf; vals[8 + w] = zf; }
      psync();
      cf = 0.0; zf = 0.0;
      for (int qq = 0; qq < NWP; ++qq) { cf += vals[qq]; zf += vals[8 + qq]; }
    }
    const double k2f = sqrt(cf) * sqrt(zf);
    if (k2f < k2) k2 = k2f;
    lam = fmin(lam, sqrt(cf));                          // lambda_max(C) <= ||C||_F
  }
  if (tid == 0) {
    if (a.k2_out) a.k2_out[b] = k2;
    if (a.lam_out && lam >= 1.0) a.lam_out[b] = lam;
    if (!(k2 <= kmax)) {                                 // (NaN fails)
      // (a bound 64x above the gate is beyond what its overestimate — 3.5 ... 13 measured, 30 at the worst — can
      //  explain: such a problem is rejected here, without the third stage's factorisation)
      if (a.cert_flag && is_finite(k2) && lam >= 1.0 && k2 <= 64.0 * kmax) {
        // The norm bounds overestimate kappa_2 by 3.5 ... 13 where they decide: leave the verdict to the third
        // stage, a Cholesky factorisation of C - tau I with tau = Lambda / k2_max (launch_gram_cert_shift) —
        // it succeeds iff lambda_min(C) > tau, which proves kappa_2(C) <= Lambda / tau = k2_max.
        a.cert_tau[b] = lam / kmax;
        a.cert_flag[b] = 1;
      } else {
        a.fb_mask[b] = a.n + 1;
        if (a.path_out) a.path_out[b] = a.n + 1;
        { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }
      }
    }
  }
}

hipError_t launch_gram_gate(const GramCholArgs& a_in, int B, hipStream_t s, bool stage0_only) {
  GramCholArgs a = a_in;
  a.count = B;
  a.tri_ref = options_or_default(a.opt).tri_ref;
  if (stage0_only && !(a.NPAD > 80 && a.cert_done && a.dsc && a.cert_ym)) return hipErrorInvalidValue;
  // stage 0 (N > 80; the register-resident factor kernel of the small shapes carries its own first bound):
  // BLSQ_CERT0 = 0 switches it off
  if (a.NPAD > 80 && a.cert_done && a.dsc) {
    if (options_or_default(a.opt).on(OPT_CERT0)) {
      const size_t lds0 = sizeof(double) * (4 + 32 + 1) * (size_t)a.NPAD;
      hipError_t e0 = launch<gram_cert0_kernel>(dim3(B), dim3(TRI_NT), lds0, s, a);
      if (e0 != hipSuccess) return e0;
    } else {
      hipError_t me = hipMemsetAsync(a.cert_done, 0, sizeof(int) * (size_t)B, s);
      if (me != hipSuccess) return me;
      a.cert_open = nullptr;                            // (no stage 0: nothing for the norm stage to go by)
    }
  } else {
    a.cert_open = nullptr;
  }
  if (stage0_only) return hipSuccess;
  const size_t per1 = sizeof(double) * (6 * (size_t)a.NPAD + 16 * 1 + 64);
  const size_t per8 = sizeof(double) * (6 * (size_t)a.NPAD + 16 * 8 + 64);
  if (a.NPAD <= 80)                                     // one wave per problem, eight per workgroup
    return launch<gram_cond_kernel<1>>(dim3((B + GR_NW - 1) / GR_NW), dim3(GR_NT), per1 * GR_NW, s, a);
  return launch<gram_cond_kernel<8>>(dim3(B), dim3(GR_NT), per8, s, a);
}

#ifdef BLSQ_CHOL_STAMPS
int cert_debug_stamps(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_chol_st), sizeof(g_chol_st));
}
#endif
}  // namespace blsq
