// Factorisation side of the normal-equations path for N > 80 (gram_kernels.hip computes the Grams; chol_reg.hip
// factors N <= 80, cert_kernels.hip holds the certificate):
//
//   gram_chol_rl2_kernel<CERT>           equilibrated blocked Cholesky of D G D + E^2 (+ alpha I) or of a gathered
//                                        principal sub-matrix, straight from the kept Gram (chol16.h: the 16 x 16 chain)
//   gram_chol_kernel                     the left-looking reference of the same factor (option chol_rl = 0)
#include "gram_common.h"
#include "chol16.h"

namespace blsq {

#ifdef BLSQ_CHOL_STAMPS
static __device__ long long g_chol_st[4][20][8];       // this file's copy: every slot but [0][18] and [0][19]
#endif

// column-norm summary of the first n columns by ONE wave: min / max of sqrt(h_jj) and the sum of h_jj in a FIXED
// order (lane-strided partial sums, then a butterfly) — the same bits in every kernel that factors N > 80
__device__ __forceinline__ void colinfo_wave(const double* sq, int n, int lane, double& mn, double& mx, double& sm) {
  mn = __builtin_inf(); mx = 0.0; sm = 0.0;
  for (int j = lane; j < n; j += WAVE) {
    const double v = sq[j];
    mn = v < mn ? v : mn; mx = v > mx ? v : mx; sm = fma(v, v, sm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double omn = __shfl_xor(mn, o, WAVE), omx = __shfl_xor(mx, o, WAVE), osm = __shfl_xor(sm, o, WAVE);
    mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; sm = sm + osm;
  }
}

// ---- equilibrated blocked Cholesky, in place in the triangle slot -------------------------------
// Row block kb of R' :  S_j = C_{kb,j} - sum_{k<kb} R'_{k,kb}^T R'_{k,j}   (MFMA, operands from the
// rows already written),  R'_{kb,kb} = chol(S_kb) and its inverse on wave 0 (lane j owns column
// j, broadcasts by v_readlane),  R'_{kb,j} = R'_{kb,kb}^-T S_j  (MFMA; the accumulator layout of S is
// the B-operand layout).  What is stored is R = R' D^-1; operands are re-scaled on the fly.
//
// The same kernel factors the diagonally modified Grams of the trust-region systems (TRF):
//     H = D G D + diag(e^2) (+ alpha I on the first n columns),    D = diag(colscale, 1)
// whose Cholesky factor is the triangle of [R D | c; E | 0] (and of [R_aug; sqrt(alpha) I]).  With
// C = equil(G):  equil(H) = Theta^1/2 C Theta^1/2 + (I - Theta),  0 < Theta <= I diagonal, so its
// extreme eigenvalues lie inside those of C: a problem that passed the gate on C needs no new one.
// One workgroup (eight waves) per problem, N > 80: the left-looking reference of gram_chol_rl2_kernel, bit for bit
// (option chol_rl = 0; no default launch runs it).
__global__ __launch_bounds__(GR_NT, 4) void gram_chol_kernel(GramCholArgs a) {
  constexpr int UMAX = 3;                               // tiles of a row block per wave
  extern __shared__ double sh[];
  __shared__ double red[32];
  __shared__ double pminsh;
  const int pidx = (int)blockIdx.x;
  if (a.count_dev && pidx >= *a.count_dev) return;
  const int b = a.batch_list ? a.batch_list[pidx] : pidx;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int NPAD = a.NPAD;
  if (a.mask && a.mask[b] <= 1) {
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    return;
  }
  if (a.skip_path && a.skip_path[b] != 0 && !(a.qr_mask && a.qr_mask[b] == 0)) return;
  double tau = 0.0;                                     // certificate stage 3: factor C - tau I
  if (a.cert_shift) {
    if (!a.cert_flag[b]) return;                        // (uniform: only the problems the norm stage left open)
    tau = a.cert_tau[b];
  }
  // columns of this problem: all n (+ rhs), or the gathered free columns (+ rhs)
  const int N = a.ncols_dev ? a.ncols_dev[b] : a.n + 1;
  if (N <= 1) {                                         // (dogbox: every variable active — nothing to factor)
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    return;
  }
  const int n = N - 1;
  const int NT = (N + 15) / 16;
  const int* gidx = a.gather ? a.gather + (long)b * a.stride_vec : nullptr;
  // source row / column of H's index i  (the rhs is the source's column a.n)
  auto src = [&](int i) -> int { return gidx ? (i < n ? gidx[i] : a.n) : i; };
  const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;    // source Gram (may alias the output)
  double* Gb = a.G + (long)b * NPAD * NPAD;             // output triangle
  double* dl = sh;                 // [NPAD] equilibration 1 / sqrt(h_jj)
  double* sq = dl + NPAD;          // [NPAD] sqrt(h_jj)
  double* sc = sq + NPAD;          // [NPAD] colscale_j * dl_j  (scale applied to source entries)
  double* Dt = sc + NPAD;          // [256]  diagonal tile (row-major)
  double* Ri = Dt + 256;           // [256]  its inverse
  double* td = Ri + 256;           // [NPAD] (e_j^2 + alpha) * dl_j^2  (added to the diagonal of C)
  const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
  const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
  const double sa = a.diag_sqrt ? a.diag_sqrt[b] : 0.0;
  // 0. column scales from the diagonal of H
  int bad = 0;
  for (int j = tid; j < NPAD; j += GR_NT) {
    int sj;
    const double d = col_scale(Gs, NPAD, j, n, src, csv, edv, sa, tau, dl, sq, sc, td, bad, sj);
    if (a.dsc) a.dsc[(long)b * NPAD + j] = d;
  }
  if (a.colinfo) {                                      // (uniform) column-norm summary for the rank gate
    __syncthreads();
    double mn = __builtin_inf(), sm = 0.0, mx = 0.0;
    if (w == 0) colinfo_wave(sq, n, lane, mn, mx, sm);
    if (tid == 0) {
      a.colinfo[2 * (long)b] = mn; a.colinfo[2 * (long)b + 1] = sm;
      if (a.hmax) a.hmax[b] = mx * mx;
      if (a.lam_out) a.lam_out[b] = (double)n;
    }
  }
  // strictly lower tiles are part of the triangle's image: zero
  for (int r = 16 + w; r < (a.skip_zero ? 0 : NPAD); r += GR_NW) {
    const int cend = r & ~15;
    for (int c = lane; c < cend; c += WAVE) Gb[(long)r * NPAD + c] = 0.0;
  }
  bad = block_or(bad, red);
  if (tid == 0) pminsh = 1.0;
  __syncthreads();
  if (bad) {                                            // uniform: hand the problem to the QR tree
    if (tid == 0 && a.fb_mask) {
      a.fb_mask[b] = a.n + 1; { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }   // (the tree factors ALL n + 1 columns)
      if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = 0.0;
      if (a.path_out) a.path_out[b] = a.n + 1;
      if (a.k2_out && !a.cert_shift) a.k2_out[b] = 0.0;
    }
    return;
  }

  const bool stp = pidx == (a.count > 300 ? 300 : 0) && !a.cert_shift;   // (diagnostic stamps)
  (void)stp;
  for (int kb = 0; kb < NT; ++kb) {
    CST(stp && w == 0, 0, kb, 0); CST(stp && w == 3, 1, kb, 0);
    // ---- A. Schur complements of this row block (tile j = kb + w + 8 u) ----
    v4d S[UMAX];
    const double dk = dl[16 * kb + lc];
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      const int j = kb + w + GR_NW * u;
      S[u] = v4d{0.0, 0.0, 0.0, 0.0};
      if (j < NT) {
        const double dj = dl[16 * j + lc];
        const double scj = sc[16 * j + lc];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * kb + lr + 4 * g;
          const int col = 16 * j + lc;
          double v = 0.0;
          if (row < N && col < N) {
            int sr_ = src(row), sc_ = src(col);
            if (sr_ > sc_) { const int t_ = sr_; sr_ = sc_; sc_ = t_; }   // symmetric: stay in the upper tiles
            v = Gs[(long)sr_ * NPAD + sc_] * sc[row] * scj;
          }
          if (j == kb && lr + 4 * g == lc) v += td[row];
          S[u][g] = v;
        }
        for (int k = 0; k < kb; ++k) {
          double av[4], bv[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const long ro = (long)(16 * k + 4 * s + lr) * NPAD;
            av[s] = Gb[ro + 16 * kb + lc];
            bv[s] = Gb[ro + 16 * j + lc];
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) S[u] = mfma_f64(-(av[s] * dk), bv[s] * dj, S[u]);
        }
      }
    }
    // ---- B. wave 0: Cholesky of the diagonal tile and its inverse (chol16.h), straight from the
    // accumulators of its Schur complement ----
    CST(stp && w == 0, 0, kb, 1); CST(stp && w == 3, 1, kb, 1);
    if (w == 0) {
      const double pm = chol16_blocked3(S[0], Dt, Ri, n - 16 * kb, pminsh);
      if (lane == 0) pminsh = pm;
    }
    CST(stp && w == 0, 0, kb, 2);
    __syncthreads();
    CST(stp && w == 0, 0, kb, 3); CST(stp && w == 3, 1, kb, 3);
    if (a.rinv && w == GR_NW - 1) {                     // kept for the conditioning certificate (off the chain)
      double* ro = a.rinv + ((long)b * (NPAD / 16) + kb) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) ro[q * 64 + lane] = Ri[q * 64 + lane];
    }
    // ---- C. R'_{kb,j} = R'_{kb,kb}^-T S_j, stored as R = R' D^-1 ----
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      const int j = kb + w + GR_NW * u;
      if (j < NT) {
        v4d X = {0.0, 0.0, 0.0, 0.0};
        if (j == kb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) X[g] = Dt[(lr + 4 * g) * 16 + lc];
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) X = mfma_f64(Ri[(4 * s + lr) * 16 + lc], S[u][s], X);
        }
        const double sj = sq[16 * j + lc];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * kb + lr + 4 * g;
          const int colg = 16 * j + lc;
          double val = X[g] * sj;
          if (row >= n || row > colg || colg > n) val = 0.0;
          Gb[(long)row * NPAD + colg] = val;
        }
      }
    }
    CST(stp && w == 0, 0, kb, 4); CST(stp && w == 3, 1, kb, 4);
    __syncthreads();
    CST(stp && w == 0, 0, kb, 5); CST(stp && w == 3, 1, kb, 5);
  }
  if (16 * NT < NPAD && !a.skip_zero) {                  // sub-matrix: the rest of the slot is zero
    for (int r = w; r < NPAD; r += GR_NW) {
      const int c0 = (r < 16 * NT) ? 16 * NT : (r & ~15);
      for (int c = c0 + lane; c < NPAD; c += WAVE) Gb[(long)r * NPAD + c] = 0.0;
    }
  }
  if (tid == 0 && a.fb_mask) {
    const double floor_ = a.pivot_floor > 0.0 ? a.pivot_floor : 1.0 / GRAM_K2_MAX;
    const bool fail = !(pminsh >= floor_);
    if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = pminsh;
    a.fb_mask[b] = fail ? a.n + 1 : 0;
    if (a.path_out) a.path_out[b] = fail ? a.n + 1 : 0;
    if (fail) { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }
    if (fail && !a.cert_shift && a.k2_out) a.k2_out[b] = 0.0;      // (no bound for this factorisation)
    if (a.cert_shift) {
      a.cert_flag[b] = 0;
      if (!fail && a.k2_out) a.k2_out[b] = a.k2_max;    // proven: kappa_2 <= Lambda / tau
    }
  }
}

// ---- N > 80, right-looking, flag-driven: no workgroup barrier inside the factorisation ----------
// One workgroup of sixteen waves per problem: wave 0 runs the 16x16 chains, fifteen worker waves hold the tiles.  The
// whole (scaled) matrix lives in accumulators: the NT (NT + 1) / 2 <= 153 upper tiles are dealt CYCLICALLY over the
// fifteen workers (row-major tile q -> wave 1 + q % 15, slot q / 15: at most 11 slots) so that the shrinking trailing
// matrix stays balanced, and never leave the worker until their row block is final — no global-memory round trip
// inside the factorisation (gram_chol_kernel, the left-looking reference, re-reads finished rows from L2).  The
// arithmetic is that of gram_chol_kernel (same operands, same order: the same bits), scheduled along the critical path
// chain(kb) -> R'_{kb,kb+1} -> S_{kb+1,kb+1} -> chain(kb + 1):
//   * wave 0 only runs the 16x16 chains (and, with CERT, the certificate's forward solve of the block just factored,
//     while the workers solve its row): it waits for the flag "diagonal tile kb is in Dt", factors, raises "R'_kk and
//     its inverse are in LDS" — it never meets a barrier inside the loop, nor the stores of the workers;
//   * the owner of tile (kb, kb+1) solves it first and raises a flag; the owner of (kb+1, kb+1) waits for exactly
//     that tile, updates the diagonal tile and hands it to wave 0; only then come the other tiles of the row;
//   * wave 0 runs at s_setprio 1, and so do those two steps of their owners: each SIMD carries four waves, and the
//     chain's path must not queue behind the bulk trailing updates of the SIMD's other waves;
//   * the trailing update of a worker starts when a COUNTER says that all fifteen workers have published their
//     tiles of the row block — LDS flags and lgkmcnt waits only, so nobody waits for the acknowledgement of the
//     global stores of the factor (a __syncthreads does: vmcnt counts stores on gfx9);
//   * Dt, Ri and the row buffer are double-buffered by the parity of kb.  Buffer kb & 1 is written again at row block
//     kb + 2, whose chain needs S_{kb+2,kb+2}, i.e. its owner's trailing update with row kb, which waited for the
//     counter of row kb — every worker had then read Ri / Dt of kb and finished its trailing update of kb - 1.
//   * the source tiles are requested ALL AT ONCE at kernel entry (the old preamble paid one memory round trip per
//     tile slot: 37 us); wave 0 computes the column scales meanwhile, and the column summary is a wave reduction.
// Registers: 1024 threads leave 128 VGPRs per wave.  A worker keeps RL_SLR slots (80 or 72 VGPRs) in registers and
// the last one or two — the bottom-right tiles, solved last — in LDS (tailL).
__device__ __forceinline__ void spin_ge(const int* f, int v) {
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void raise_flag(int* f, int v, int lane) {      // (after this wave's LDS writes)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
enum { FL_DIAG = 0, FL_RINV = 1, FL_ROW1 = 2, FL_PUB = 3, FL_BAD = 4, FL_YB = 5, FL_YPUB = 6 };
static constexpr int RL_NT = 1024;                      // this kernel's workgroup: wave 0 (chains) + 15 workers
static constexpr int RL_NW = RL_NT / WAVE;
static constexpr int RL_NWK = RL_NW - 1;                // worker waves
static constexpr int RL_SL = (17 * 18 / 2 + RL_NWK - 1) / RL_NWK;   // tile slots per worker: 11 for NT <= 17
// slots in registers: 128 VGPRs hold no eleventh beside the rest of the worker's code, nor a tenth with CERT (both
// would spill to scratch)
template <bool CERT> constexpr int RL_SLR = CERT ? RL_SL - 2 : RL_SL - 1;

template <bool CERT>
__device__ __forceinline__ void chol_rl2_body(const GramCholArgs& a, const int b, double* sh, int* fl, double& pminsh) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int NPAD = a.NPAD;
  const bool stp = (int)blockIdx.x == 100 && !a.cert_shift; (void)stp;
  CST(stp && (w == 0 || w == 2), w == 0 ? 2 : 3, 17, 0);
  if (a.mask && a.mask[b] <= 1) {
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    return;
  }
  if (a.skip_path && a.skip_path[b] != 0 && !(a.qr_mask && a.qr_mask[b] == 0)) return;
  double tau = 0.0;                                     // certificate stage 3: factor C - tau I
  if (a.cert_shift) {
    if (!a.cert_flag[b]) return;                        // (uniform)
    tau = a.cert_tau[b];
  }
  const int N = a.ncols_dev ? a.ncols_dev[b] : a.n + 1;
  if (N <= 1) {                                         // (dogbox: every variable active — nothing to factor)
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    return;
  }
  const int n = N - 1;
  const int NT = (N + 15) / 16;
  const int NTP = NPAD / 16;
  const int* gidx = a.gather ? a.gather + (long)b * a.stride_vec : nullptr;
  const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;
  double* Gb = a.G + (long)b * NPAD * NPAD;
  double* dl = sh;                 // [NPAD]
  double* sq = dl + NPAD;          // [NPAD]
  double* sc = sq + NPAD;          // [NPAD]
  double* td = sc + NPAD;          // [NPAD]
  double* Dt = td + NPAD;          // [2][256]
  double* Ri = Dt + 512;           // [2][256]
  double* Rrow = Ri + 512;         // [2][NTP][256] finished tiles of a row block (operands of the trailing updates)
  int* gl = reinterpret_cast<int*>(Rrow + 2 * (size_t)NTP * 256);   // [NPAD] gathered source indices
  // The factor kernel's share of the certificate's stage 0 (GramCholArgs::cert_ym): the solve M(R')^T y = e and
  // the column sums of |R'| advance row block by row block as R' is produced — stage 0 then needs ONE pass over
  // the factor (the backward solve, with the row sums on the way) instead of four.  Fixed order: reproducible.
  double* yv = reinterpret_cast<double*>(gl + NPAD);     // [NPAD] y (final for the finished row blocks)
  double* csum = yv + NPAD;                              // [NPAD] sum_i |R'_ij| over the finished row blocks
  double* tailL = csum + NPAD;                           // [SL - SLR][15][256] the LDS-resident tile slots
  constexpr int SLR = RL_SLR<CERT>;
  constexpr bool cert = CERT;                            // (a launch with cert_ym set, never the shifted one)
  const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
  const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
  const double sa = a.diag_sqrt ? a.diag_sqrt[b] : 0.0;
  if (tid < 8) fl[tid] = 0;
  if (tid == 0) pminsh = 1.0;
  if (gidx) {                                           // (uniform) the index map of a gathered sub-matrix -> LDS
    for (int j = tid; j < NPAD; j += RL_NT) gl[j] = j < n ? gidx[j] : a.n;
  }
  __syncthreads();
  auto src = [&](int i) -> int { return gidx ? gl[i] : i; };     // (i < N)

  constexpr int NWK = RL_NWK, SL = RL_SL;
  const int ww = w - 1;
  // Wave 0 and the workers part here and meet again at the end: each side passes the barriers S and X on its own
  // path (wave-uniform branches), so that the tile slots, live only on the workers' side, do not crowd wave 0's code.
  // Bad column (uniform after X): the problem goes to the QR tree.
  auto to_tree = [&]() -> bool {
    if (!__hip_atomic_load(&fl[FL_BAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return false;
    if (tid == 0 && a.fb_mask) {
      a.fb_mask[b] = a.n + 1; { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }   // (the tree factors ALL n + 1 columns)
      if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = 0.0;
      if (a.path_out) a.path_out[b] = a.n + 1;
      if (a.k2_out && !a.cert_shift) a.k2_out[b] = 0.0;
    }
    return true;
  };
  // zeros outside the factor: strictly lower tiles, and everything beyond 16 NT (sub-matrix use)
  auto zero_rest = [&]() {
    for (int r = w; r < (a.skip_zero ? 0 : NPAD); r += RL_NW) {
      const int cend = (r < 16 * NT) ? (r & ~15) : NPAD;
      for (int c = lane; c < cend; c += WAVE) Gb[(unsigned)(r * NPAD + c)] = 0.0;
      if (r < 16 * NT)
        for (int c = 16 * NT + lane; c < NPAD; c += WAVE) Gb[(unsigned)(r * NPAD + c)] = 0.0;
    }
  };
  if (w == 0) {
    // column scales from the diagonal of H, by wave 0 alone: CW columns per lane in flight at once — their global
    // stores come after all of their loads
    int bad = 0;
    constexpr int CW = (17 * 16 + WAVE - 1) / WAVE;
    for (int j0 = 0; j0 < NPAD; j0 += CW * WAVE) {
      double d[CW];
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        const int j = j0 + WAVE * k + lane;
        if (j < NPAD) {
          int sj;
          d[k] = col_scale(Gs, NPAD, j, n, src, csv, edv, sa, tau, dl, sq, sc, td, bad, sj);
          if (cert) { yv[j] = 1.0; csum[j] = 0.0; }
        }
      }
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        const int j = j0 + WAVE * k + lane;
        if (a.dsc && j < NPAD) a.dsc[(long)b * NPAD + j] = d[k];
      }
    }
    if (__any(bad) && lane == 0) __hip_atomic_store(&fl[FL_BAD], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    CST(stp, 2, 17, 1);
    __syncthreads();                                    // S: the scales are in LDS
    if (a.colinfo) {                                    // column-norm summary for the rank gate
      double mn, mx, sm;
      colinfo_wave(sq, n, lane, mn, mx, sm);
      if (lane == 0) {
        a.colinfo[2 * (long)b] = mn; a.colinfo[2 * (long)b + 1] = sm;
        if (a.hmax) a.hmax[b] = mx * mx;
        if (a.lam_out) a.lam_out[b] = (double)n;
      }
    }
    __syncthreads();                                    // X: all source reads done before the first store
    CST(stp, 2, 17, 3);
    if (to_tree()) return;
    zero_rest();
    CST(stp, 2, 17, 4);
    __builtin_amdgcn_s_setprio(1);                      // the chains: the critical path of the whole factor
    double pmin = 1.0;
    for (int kb = 0; kb < NT; ++kb) {
      double* DtC = Dt + (kb & 1) * 256;
      double* RiC = Ri + (kb & 1) * 256;
      if (kb > 0) spin_ge(&fl[FL_DIAG], kb);            // the updated diagonal tile kb is in DtC
      CST(stp, 2, kb, 0);
      pmin = chol16_blocked3(DtC, RiC, n - 16 * kb, pmin);   // (chol16.h; ends with lgkmcnt(0))
      if (lane == 0) __hip_atomic_store(&fl[FL_RINV], kb + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      CST(stp, 2, kb, 1);
      if (a.rinv) {                                     // kept for the conditioning certificate
        double* ro = a.rinv + ((long)b * NTP + kb) * 256;
#pragma unroll
        for (int q = 0; q < 4; ++q) ro[q * 64 + lane] = RiC[q * 64 + lane];
      }
      if (cert) {
        // y of the block by forward substitution with |R'_kk| — once every worker has added its share of the row
        // block before (FL_YPUB) — and the tile's column sums.  Off the chain: the workers are solving row block kb
        // meanwhile, and wave 0 has the registers that a worker (ten tile slots) lacks.
        spin_ge(&fl[FL_YPUB], NWK * kb);
        const int i_ = lane & 15, gi = 16 * kb + i_;
        double Dc[16], cs_ = 0.0;
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
          const double v_ = fabs(DtC[s_ * 16 + i_]);
          Dc[s_] = s_ < i_ ? v_ : 0.0;
          if (s_ <= i_) cs_ += v_;
        }
        const double dg_ = DtC[i_ * 16 + i_];
        const bool live_ = gi < n && dg_ > 0.0;
        const double iv_ = live_ ? 1.0 / dg_ : 0.0;
        double r_ = live_ ? yv[gi] : 0.0;
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
          const double ys_ = read_lane(r_ * iv_, s_);
          if (i_ > s_) r_ = fma(Dc[s_], ys_, r_);
        }
        if (lane < 16 && gi < n) { yv[gi] = r_ * iv_; csum[gi] += cs_; }
        raise_flag(&fl[FL_YB], kb + 1, lane);
      }
    }
    if (lane == 0) pminsh = pmin;
  } else {
    // tile q (row-major over the upper tiles) -> worker q % 15, slot q / 15; packed (i | j << 8) per slot.  The
    // source tiles are requested all at once (raw; selected and scaled once the scales are in LDS).
    int tij[SL];
    v4d acc[SL];
    // slots t >= SLR live in LDS once scaled (t: a compile-time index in every unrolled loop below)
    auto get = [&](int t) -> v4d {
      if (t < SLR) return acc[t];
      const double* p_ = tailL + ((size_t)(t - SLR) * NWK + ww) * 256 + lane;
      return v4d{p_[0], p_[64], p_[128], p_[192]};
    };
    auto put = [&](int t, const v4d& v) {
      if (t < SLR) { acc[t] = v; return; }
      double* p_ = tailL + ((size_t)(t - SLR) * NWK + ww) * 256 + lane;
      p_[0] = v[0]; p_[64] = v[1]; p_[128] = v[2]; p_[192] = v[3];
    };
    {
      int i = 0, off = ww;                              // slot 0: q = ww
#pragma unroll
      for (int t = 0; t < SL; ++t) {
        while (i < NT && off >= NT - i) { off -= NT - i; ++i; }
        tij[t] = i < NT ? (i | ((i + off) << 8)) : -1;
        off += NWK;
      }
    }
    auto load_raw = [&](int t) -> v4d {                 // (raw; selected and scaled below)
      v4d v = {0.0, 0.0, 0.0, 0.0};
      if (tij[t] >= 0) {
        const int i = tij[t] & 255, j = tij[t] >> 8;
        const int col = 16 * j + lc;
        const int scolu = src(col), scol = col < N ? scolu : 0;     // (src reads gl[] below NPAD: unconditionally)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * i + lr + 4 * g;
          const int srow = src(row);
          int sr_ = row < N ? srow : 0, sc_ = scol;
          if (sr_ > sc_) { const int t_ = sr_; sr_ = sc_; sc_ = t_; }       // symmetric: stay in the upper tiles
          v[g] = Gs[(unsigned)(sr_ * NPAD + sc_)];
        }
      }
      return v;
    };
    // all at once: the register slots, then the LDS slots (whose stores wait for every load)
#pragma unroll
    for (int t = 0; t < SLR; ++t) acc[t] = load_raw(t);
#pragma unroll
    for (int t = SLR; t < SL; ++t) put(t, load_raw(t));
    CST(stp && w == 2, 3, 17, 1);
    __syncthreads();                                    // S: the scales are in LDS
    // the scaled source tiles (the source may alias the output: everything is read before anything is written)
#pragma unroll
    for (int t = 0; t < SL; ++t) {
      if (tij[t] >= 0) {
        const int i = tij[t] & 255, j = tij[t] >> 8;
        if (t >= SLR) acc[t] = get(t);
        const double scj = sc[16 * j + lc];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          // in place and by selects: both arms are computed on every lane (the empty asm keeps the compiler from
          // sinking them into exec-masked branches, which spill the tile — no room for a second one)
          const int row = 16 * i + lr + 4 * g, col = 16 * j + lc;
          double p = acc[t][g] * sc[row] * scj;
          asm volatile("" : "+v"(p));
          double v = (row < N && col < N) ? p : 0.0;
          double vd = v + td[row];
          asm volatile("" : "+v"(vd));
          acc[t][g] = (j == i && lr + 4 * g == lc) ? vd : v;
        }
        if (i == 0 && j == 0) {
#pragma unroll
          for (int g = 0; g < 4; ++g) Dt[(lr + 4 * g) * 16 + lc] = acc[t][g];
        }
        if (t >= SLR) put(t, acc[t]);
      }
    }
    CST(stp && w == 2, 3, 17, 2);
    __syncthreads();                                    // X
    CST(stp && w == 2, 3, 17, 3);
    if (to_tree()) return;
    zero_rest();
    CST(stp && w == 2, 3, 17, 4);
    for (int kb = 0; kb < NT; ++kb) {
      const double* DtC = Dt + (kb & 1) * 256;
      const double* RiC = Ri + (kb & 1) * 256;
      double* RrowC = Rrow + (size_t)(kb & 1) * NTP * 256;
      // this wave's slots of row block kb: tiles q0 .. q0 + NT - kb - 1
      const int q0 = kb * NT - kb * (kb - 1) / 2;
      const int t_lo = (q0 - ww + NWK - 1 + NWK) / NWK - 1;          // ceil((q0 - ww) / 15), q0 - ww >= -14
      const int t_hi = (q0 + NT - kb - 1 - ww + NWK) / NWK - 1;      // floor(.. / 15)
      const int t_one = ((q0 + 1 - ww) % NWK == 0 && kb + 1 < NT) ? (q0 + 1 - ww) / NWK : -1;   // slot of (kb, kb+1)
      const int q1 = q0 + NT - kb;                                     // tile (kb+1, kb+1)
      const int t_dia = ((q1 - ww) % NWK == 0 && kb + 1 < NT) ? (q1 - ww) / NWK : -1;
      CST(stp && w == 2, 3, kb, 5);
      spin_ge(&fl[FL_RINV], kb + 1);                    // R'_kk and its inverse are in LDS
      CST(stp && w == 2, 3, kb, 0);
      double rf[4];
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) rf[s_] = RiC[(4 * s_ + lr) * 16 + lc];
      // R'_{kb,j} = R'_{kb,kb}^-T S_j -> memory (as R = R' D^-1) and the LDS row buffer
      auto solve_tile = [&](int t, const v4d& S) {
        const int j = kb + (ww + NWK * t - q0);
        v4d X = {0.0, 0.0, 0.0, 0.0};
        if (j == kb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) X[g] = DtC[(lr + 4 * g) * 16 + lc];
        } else {
#pragma unroll
          for (int s_ = 0; s_ < 4; ++s_) X = mfma_f64(rf[s_], S[s_], X);
        }
        const double sj = sq[16 * j + lc];
        const double dj = dl[16 * j + lc];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * kb + lr + 4 * g;
          const int colg = 16 * j + lc;
          double val = X[g] * sj;
          if (row >= n || row > colg || colg > n) val = 0.0;
          Gb[(unsigned)(row * NPAD + colg)] = val;
          // the operand of the trailing updates is what the left-looking kernel reads back: the STORED
          // entry times its column's equilibration — all factor kernels agree bit for bit
          if (j != kb) RrowC[j * 256 + (lr + 4 * g) * 16 + lc] = val * dj;
        }
      };
      // 1. the critical tile (kb, kb + 1) first — steps 1 and 2 at raised priority: they are on the chain's path, the
      // other waves of the SIMD are in their bulk updates
      if (t_one >= 0 || t_dia >= 0) __builtin_amdgcn_s_setprio(1);
      if (t_one >= 0) {
        CST(stp, 1, kb, 0);
#pragma unroll
        for (int t = 0; t < SL; ++t) {
          if (t == t_one) solve_tile(t, get(t));
        }
        raise_flag(&fl[FL_ROW1], kb + 1, lane);
        CST(stp, 1, kb, 1);
      }
      // 2. the next diagonal tile: S_{kb+1,kb+1} -= R'_{kb,kb+1}^T R'_{kb,kb+1} -> Dt of the other parity
      if (t_dia >= 0) {
        spin_ge(&fl[FL_ROW1], kb + 1);
        CST(stp, 1, kb, 2);
        const double* Ra = RrowC + (kb + 1) * 256 + lr * 16 + lc;
        double* DtN = Dt + ((kb + 1) & 1) * 256;
#pragma unroll
        for (int t = 0; t < SL; ++t) {
          if (t == t_dia) {
            v4d S = get(t);
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) S = mfma_f64(-Ra[64 * s_], Ra[64 * s_], S);
            put(t, S);
#pragma unroll
            for (int g = 0; g < 4; ++g) DtN[(lr + 4 * g) * 16 + lc] = S[g];
          }
        }
        raise_flag(&fl[FL_DIAG], kb + 1, lane);
        CST(stp, 1, kb, 3);
      }
      if (t_one >= 0 || t_dia >= 0) __builtin_amdgcn_s_setprio(0);
      CST(stp && w == 2, 3, kb, 1);
      // 3. the other tiles of the row block
#pragma unroll
      for (int t = 0; t < SL; ++t) {
        if (t >= t_lo && t <= t_hi && t != t_one) solve_tile(t, get(t));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add(&fl[FL_PUB], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (cert) {                                       // (behind the counter: nobody's trailing update waits for this)
        // y_j += sum_s |R'_{kb,j}[s][.]| y_s and the column sums, for this wave's tiles of the row block (from the
        // row buffer; lane (lr, lc) holds rows lr + 4 g of column lc, the four lane rows are added in a fixed tree)
        if (kb + 1 < NT) spin_ge(&fl[FL_YB], kb + 1);
        for (int t = t_lo; t <= t_hi && kb + 1 < NT; ++t) {
          const int j = kb + (ww + NWK * t - q0);
          if (j == kb) continue;
          double p_ = 0.0, q_ = 0.0;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const double a_ = fabs(RrowC[j * 256 + (lr + 4 * g) * 16 + lc]);
            p_ = fma(a_, yv[16 * kb + lr + 4 * g], p_);
            q_ += a_;
          }
          p_ += __shfl_xor(p_, 16, WAVE); q_ += __shfl_xor(q_, 16, WAVE);
          p_ += __shfl_xor(p_, 32, WAVE); q_ += __shfl_xor(q_, 32, WAVE);
          if (lr == 0 && 16 * j + lc < n) { yv[16 * j + lc] += p_; csum[16 * j + lc] += q_; }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(&fl[FL_YPUB], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      CST(stp && w == 2, 3, kb, 2);
      if (kb + 1 >= NT) break;
      spin_ge(&fl[FL_PUB], NWK * (kb + 1));             // every worker's tiles of the row block are in RrowC
      CST(stp && w == 2, 3, kb, 3);
      // 4. trailing update of this wave's tiles (ascending rows; the next diagonal tile is done)
#pragma unroll
      for (int t = 0; t < SL; ++t) {
        if (t > t_hi && t != t_dia && tij[t] >= 0) {
          const int i = tij[t] & 255, j = tij[t] >> 8;
          const double* Ra = RrowC + i * 256 + lr * 16 + lc;
          const double* Rb = RrowC + j * 256 + lr * 16 + lc;
          v4d S = get(t);
#pragma unroll
          for (int s_ = 0; s_ < 4; ++s_) S = mfma_f64(-Ra[64 * s_], Rb[64 * s_], S);
          put(t, S);
        }
      }
      CST(stp && w == 2, 3, kb, 4);
    }
  }
  CST(stp && (w == 0 || w == 2), w == 0 ? 2 : 3, 18, 0);
  __syncthreads();
  CST(stp && (w == 0 || w == 2), w == 0 ? 2 : 3, 18, 1);
  if (cert && w == 0) {
    double ym_ = 0.0, r1_ = 0.0;
    for (int j = lane; j < n; j += WAVE) {
      ym_ = yv[j] > ym_ ? yv[j] : ym_;
      r1_ = csum[j] > r1_ ? csum[j] : r1_;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double oy = __shfl_xor(ym_, o, WAVE), orr = __shfl_xor(r1_, o, WAVE);
      ym_ = oy > ym_ ? oy : ym_; r1_ = orr > r1_ ? orr : r1_;
    }
    if (lane == 0) { a.cert_ym[b] = ym_; a.cert_r1[b] = r1_; }
  }
  if (tid == 0 && a.fb_mask) {
    const bool fail = !(pminsh >= (a.pivot_floor > 0.0 ? a.pivot_floor : 1.0 / GRAM_K2_MAX));
    if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = pminsh;
    a.fb_mask[b] = fail ? a.n + 1 : 0;
    if (a.path_out) a.path_out[b] = fail ? a.n + 1 : 0;
    if (fail) { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }
    if (fail && !a.cert_shift && a.k2_out) a.k2_out[b] = 0.0;      // (no bound for this factorisation)
    if (a.cert_shift) {
      a.cert_flag[b] = 0;
      if (!fail && a.k2_out) a.k2_out[b] = a.k2_max;    // proven: kappa_2 <= Lambda / tau
    }
  }
}

template <bool CERT>
__global__ __launch_bounds__(RL_NT, 1) void gram_chol_rl2_kernel(GramCholArgs a) {
  extern __shared__ double sh[];
  __shared__ double pminsh;
  __shared__ int fl[8];                                 // FL_*: hand-over flags and the publication counter
  const int pidx = (int)blockIdx.x;
  if (a.count_dev && pidx >= *a.count_dev) return;
  const int b = a.batch_list ? a.batch_list[pidx] : pidx;
  chol_rl2_body<CERT>(a, b, sh, fl, pminsh);
}

hipError_t launch_gram_chol(const GramCholArgs& a_in, int B, hipStream_t s) {
  GramCholArgs a = a_in;
  a.count = B;
  if (a.NPAD <= 80) return launch_gram_chol_reg(a, s);  // (chol_reg.hip)
  if (options_or_default(a.opt).i(OPT_CHOL_RL) != 0) {   // (per launch: tests compare the kernels)
    // Right-looking register kernel, flag-driven: 0.106 ms per problem on a CU of its own (one workgroup of 16 waves
    // per CU) against 0.27 ms for a PAIR of problems on a CU through the left-looking kernel (its Schur-complement
    // phase waits for L2: 190 of its 275 us, tools/chol_stamps.py).  BLSQ_CHOL_RL = 0 runs the left-looking one: the two
    // agree bit for bit (same operands, same order), so it is the reference, never a faster choice.
    const bool cert = a.cert_ym && !a.cert_shift;
    const size_t lds = sizeof(double) * (4 * (size_t)a.NPAD + 1024 + 2 * (size_t)(a.NPAD / 16) * 256 +
                                         2 * (size_t)a.NPAD +
                                         (size_t)(RL_SL - (cert ? RL_SLR<true> : RL_SLR<false>)) * RL_NWK * 256) +
                       sizeof(int) * (size_t)a.NPAD;
    if (cert) return launch<gram_chol_rl2_kernel<true>>(dim3(B), dim3(RL_NT), lds, s, a);
    return launch<gram_chol_rl2_kernel<false>>(dim3(B), dim3(RL_NT), lds, s, a);
  }
  if (a.cert_ym) {                                      // (only the flag-driven kernel has a share in stage 0)
    hipError_t me = hipMemsetAsync(a.cert_ym, 0, sizeof(double) * (size_t)B, s);
    if (me != hipSuccess) return me;
  }
  return launch<gram_chol_kernel>(dim3(B), dim3(GR_NT), sizeof(double) * (4 * (size_t)a.NPAD + 512), s, a);
}
hipError_t launch_gram_cert_shift(const GramCholArgs& a_in, int B, hipStream_t s) {
  if (!a_in.cert_flag || !a_in.cert_tau) return hipSuccess;
  GramCholArgs a = a_in;
  a.cert_shift = 1;
  a.G = a.ywork;                                        // (Y of the norm stage is dead by now)
  a.skip_zero = 1;
  a.pivot_floor = GRAM_CERT_PIVOT_FLOOR;
  a.dsc = nullptr; a.colinfo = nullptr; a.rinv = nullptr; a.cert_done = nullptr; a.unsettled = nullptr;
  a.dog = GramCholArgs::DogFinish{}; a.lmfin = GramCholArgs::LmFinish{};
  a.batch_list = nullptr; a.count_dev = nullptr; a.skip_path = nullptr; a.diag_sqrt = nullptr;
  a.qr_mask = nullptr; a.hmax = nullptr; a.lam_out = nullptr; a.pmin_out = nullptr;
  return launch_gram_chol(a, B, s);
}

#ifdef BLSQ_CHOL_STAMPS
int chol_reg_debug_stamps(long long* host);            // chol_reg.hip
int cert_debug_stamps(long long* host);                // cert_kernels.hip
// This file's copy, and every slot that a kernel of the other two files wrote (non-zero) over it: the register kernel's
// [0][19], stage 0's [0][18] and its block steps (stage 0 runs after the factor kernel of the same launch sequence).
int chol_debug_stamps(long long* host) {
  constexpr int NS = 4 * 20 * 8;
  long long part[NS];
  int e = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_chol_st), sizeof(g_chol_st));
  for (auto copy : {chol_reg_debug_stamps, cert_debug_stamps}) {
    if (e == 0) e = copy(part);
    for (int i = 0; e == 0 && i < NS; ++i)
      if (part[i] != 0) host[i] = part[i];
  }
  return e;
}
#endif
}  // namespace blsq
