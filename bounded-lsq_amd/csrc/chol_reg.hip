// Factorisation side of the normal-equations path for N <= 80: one wave per problem, the whole matrix in registers
// (gram_kernels.hip computes the Grams; chol_rl.hip factors N > 80, cert_kernels.hip holds the certificate):
//
//   gram_chol_reg_kernel    equilibrated blocked Cholesky of D G D + E^2 (+ alpha I) or of a gathered principal
//                           sub-matrix, straight from the kept Gram, with the first bound of the certificate and the
//                           TRF / dogbox finishes
//   lm_rounds_reg_kernel    the whole trust-region sub-problem after the factor in one launch
//
// At most 5 x 5 tiles: the 15 upper tiles of the equilibrated matrix are loaded ONCE into accumulators and never leave
// the wave until their row block is final.  Per row block: the chain of the diagonal tile straight from its accumulator
// (chol16.h), R'_{kb,j} = R'_kk^-T S_j by MFMA, and the right-looking update of the remaining tiles — whose MFMA
// operands are the rows just solved, already in the right layout (register s of a tile in the accumulator layout holds
// rows 4 s + lr: the operand fragment of k-step s).  No L2 round trip inside the factorisation (a left-looking kernel
// pays one per tile and finished row block: 20 exposed latencies at N = 65), no barrier.  Both kernels run that
// factorisation through the helpers below.
#include "gram_common.h"
#include "chol16.h"

namespace blsq {

#ifdef BLSQ_CHOL_STAMPS
static __device__ long long g_chol_st[4][20][8];       // this file's copy: [0][19] (chol_debug_stamps, chol_rl.hip)
#endif

static constexpr int MT = 5;                            // tile rows at most (N <= 80)
static constexpr int NTILE = MT * (MT + 1) / 2;
__device__ __forceinline__ int tix(int i, int j) { return i * MT - i * (i - 1) / 2 + (j - i); }   // upper tile (i, j)

// Per-wave LDS of both kernels, in doubles: eight [NPAD] vectors, the diagonal tile, the MT inverse diagonal tiles and
// 16 + 64 of scratch.
__host__ __device__ inline size_t reg_lds_doubles(int NPAD) { return 8 * (size_t)NPAD + 256 + MT * 256 + 16 + 64; }
struct RegLds {
  double *dl, *sq, *sc, *td;       // [NPAD] 1 / sqrt(h_jj), sqrt(h_jj), colscale_j dl_j, (e_j^2 + alpha) dl_j^2 - tau
  double *cv, *yv, *v0, *v1;       // [NPAD] c' = R'[:, n], R'^-1 c', and two vectors of the kernel's own
  double *Dt, *Ria, *tv, *xs;      // [256] diagonal tile (row-major), [MT][256] inverse diagonal tiles, [16], [64]
  __device__ RegLds(double* sh_all, int wv, int NPAD) {
    dl = sh_all + (size_t)wv * reg_lds_doubles(NPAD);
    sq = dl + NPAD; sc = sq + NPAD; td = sc + NPAD;
    cv = td + NPAD; yv = cv + NPAD; v0 = yv + NPAD; v1 = v0 + NPAD;
    Dt = v1 + NPAD; Ria = Dt + 256; tv = Ria + MT * 256; xs = tv + 16;
  }
};

// The scaled source tiles -> accumulators; src(i): the source row / column of index i < N.  Every tile's loads FIRST,
// from clamped indices and without a branch between them, then the scaling: a uniform `if (j < NT)` around each tile
// made fifteen basic blocks, i.e. fifteen memory round trips in a row (17 of gram_chol_reg_kernel's 57 us, 15 us per
// round of lm_rounds_reg_kernel, tools/reg_stamps.py).  The source may alias the output: the caller stores nothing
// before this has returned.  HOIST: the scales of a lane's rows and columns and the diagonal shifts are read first as
// well, with no branch around a tile (what is outside the N x N block scales to zero anyway); without it each tile
// behind `j < NT` reads its own — lm_rounds_reg_kernel, whose registers are full across its Newton loop, spills to
// scratch with the hoisted form.  The two give the same values.
template <bool HOIST, class Src>
__device__ __forceinline__ void reg_load_tiles(v4d (&acc)[NTILE], const double* Gs, int NPAD, int N, int NT,
                                               const double* sc, const double* td, Src&& src) {
  const int lane = threadIdx.x & 63, lr = lane >> 4, lc = lane & 15;
  int scol[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) { const int col = 16 * j + lc; scol[j] = src(col < N ? col : N - 1); }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    int srow[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { const int row = 16 * i + lr + 4 * g; srow[g] = src(row < N ? row : N - 1); }
#pragma unroll
    for (int j = i; j < MT; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int lo_ = srow[g] < scol[j] ? srow[g] : scol[j], hi_ = srow[g] < scol[j] ? scol[j] : srow[g];   // symmetric: upper tiles
        acc[tix(i, j)][g] = Gs[(long)lo_ * NPAD + hi_];
      }
    }
  }
  if constexpr (HOIST) {
    double scj_[MT], tdl_[MT], scr_[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int col = 16 * i + lc;
      scj_[i] = sc[col < NPAD ? col : NPAD - 1];
      tdl_[i] = td[col < NPAD ? col : NPAD - 1];
#pragma unroll
      for (int g = 0; g < 4; ++g) { const int row = 16 * i + lr + 4 * g; scr_[i][g] = sc[row < NPAD ? row : NPAD - 1]; }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int j = i; j < MT; ++j) {
        v4d v4;
        const int col = 16 * j + lc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * i + lr + 4 * g;
          double v = acc[tix(i, j)][g];
          v = (row < N && col < N) ? v * scr_[i][g] * scj_[j] : 0.0;
          if (j == i && lr + 4 * g == lc && row < 16 * NT) v += tdl_[i];
          v4[g] = v;
        }
        acc[tix(i, j)] = v4;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      double scr_[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) scr_[g] = sc[(16 * i + lr + 4 * g) < NPAD ? 16 * i + lr + 4 * g : NPAD - 1];
#pragma unroll
      for (int j = i; j < MT; ++j) {
        v4d v4 = {0.0, 0.0, 0.0, 0.0};
        if (j < NT) {
          const int col = 16 * j + lc;
          const double scj = sc[col];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int row = 16 * i + lr + 4 * g;
            double v = acc[tix(i, j)][g];
            v = (row < N && col < N) ? v * scr_[g] * scj : 0.0;
            if (j == i && lr + 4 * g == lc) v += td[row];
            v4[g] = v;
          }
        }
        acc[tix(i, j)] = v4;
      }
    }
  }
}

// The factorisation, row block by row block: the chain of the diagonal tile (R'_kk -> Dt, its inverse -> Ria[kb]),
// then R'_{kb,j} = R'_kk^-T S_j kept in the accumulators of row kb, then the right-looking update of the tiles below:
// (i, j) -= R'_{kb,i}^T R'_{kb,j}.  c' = R'[:, n] -> cv on the way.  chain(kb, Ri) runs after each chain and tile(kb, j,
// X) after each solved tile; with DIAG the diagonal tile R'_kk goes into its accumulator and through tile() as well.
// sync: the kernel's own wait at the end of a row block (Dt is rewritten by the next chain).  Returns the smallest pivot.
template <bool DIAG, class Chain, class Tile, class Sync>
__device__ __forceinline__ double reg_factor(v4d (&acc)[NTILE], double* Dt, double* Ria, double* cv, int n, int NT,
                                             Chain&& chain, Tile&& tile, Sync&& sync) {
  const int lane = threadIdx.x & 63, lr = lane >> 4, lc = lane & 15;
  const int jn = n >> 4, cn = n & 15;                   // tile column / column inside it of the rhs
  double pmin = 1.0;
#pragma unroll
  for (int kb = 0; kb < MT; ++kb) {
    if (kb < NT) {
      double* Ri = Ria + kb * 256;
      pmin = chol16_blocked3(acc[tix(kb, kb)], Dt, Ri, n - 16 * kb, pmin);
      if (kb == jn && lane < 16) cv[16 * kb + lane] = Dt[lane * 16 + cn];   // the rhs column through the diagonal tile
      chain(kb, Ri);
#pragma unroll
      for (int j = DIAG ? kb : kb + 1; j < MT; ++j) {
        if (j < NT) {
          v4d X = {0.0, 0.0, 0.0, 0.0};
          if (j == kb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) X[g] = Dt[(lr + 4 * g) * 16 + lc];
            acc[tix(kb, kb)] = X;
          } else {
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) X = mfma_f64(Ri[(4 * s_ + lr) * 16 + lc], acc[tix(kb, j)][s_], X);
            acc[tix(kb, j)] = X;
            if (j == jn && lc == cn) {
#pragma unroll
              for (int g = 0; g < 4; ++g) cv[16 * kb + lr + 4 * g] = X[g];
            }
          }
          tile(kb, j, X);
        }
      }
#pragma unroll
      for (int i = kb + 1; i < MT; ++i) {
#pragma unroll
        for (int j = i; j < MT; ++j) {
          if (j < NT) {
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_)
              acc[tix(i, j)] = mfma_f64(-acc[tix(kb, i)][s_], acc[tix(kb, j)][s_], acc[tix(i, j)]);
          }
        }
      }
      sync();
    }
  }
  return pmin;
}

// y = R'^-1 c' (rows and columns below n only; c' in cv, zeros beyond n in yv), block rows from the bottom -> yv:
// tile x vector by four FMAs per lane and tile and a 16-lane sum, the 16 x 16 diagonal solve a matvec with the inverse
// tile.  tv: 16 doubles of scratch; sync: the kernel's own wait.
template <class Sync>
__device__ __forceinline__ void reg_back_solve(const v4d (&acc)[NTILE], const double* Ria, const double* cv,
                                               double* yv, double* tv, int n, Sync&& sync) {
  const int lane = threadIdx.x & 63, lr = lane >> 4, lc = lane & 15;
  const int NTn = (n + 15) / 16;
#pragma unroll
  for (int kk = MT - 1; kk >= 0; --kk) {
    if (kk < NTn) {
      double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = kk + 1; j < MT; ++j) {
        if (j < NTn) {
          const double yj = yv[16 * j + lc];
#pragma unroll
          for (int g = 0; g < 4; ++g) part[g] = fma(acc[tix(kk, j)][g], yj, part[g]);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) part[g] = row16_sum(part[g]);
      if (lc == 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) tv[lr + 4 * g] = cv[16 * kk + lr + 4 * g] - part[g];
      }
      sync();
      const int nb = (n - 16 * kk < 16) ? n - 16 * kk : 16;
      const double* Rk = Ria + kk * 256;
      double yi = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) yi = fma(Rk[lc * 16 + c], (c < nb) ? tv[c] : 0.0, yi);
      if (lc >= nb) yi = 0.0;
      if (lr == 0) yv[16 * kk + lc] = yi;
      sync();
    }
  }
}

// ---- the factor kernel ---------------------------------------------------------------------------
// Same arguments, outputs and gate bookkeeping as gram_chol_kernel (chol_rl.hip); REG_NW problems per workgroup.
// What is stored is R = R' D^-1, in place in the triangle slot.
__global__ __launch_bounds__(REG_NT, 1) void gram_chol_reg_kernel(GramCholArgs a) {
  extern __shared__ double sh_all[];
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int pidx = reg_problem((int)blockIdx.x, wv);
  if (pidx >= a.count) return;                          // (wave-uniform)
  if (a.count_dev && pidx >= *a.count_dev) return;
  const int b = a.batch_list ? a.batch_list[pidx] : pidx;
  const int lane = threadIdx.x & 63, tid = lane;
  const int lr = lane >> 4, lc = lane & 15;
  const int NPAD = a.NPAD;
  auto wsync = []() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); };
  // LDS hand-over between the lanes of this one wave: its DS instructions execute in order, the compiler only has to
  // keep them in order too.  (A `vmcnt(0)` here also waits for every store of the factor issued so far — a round trip
  // to memory per row block on the critical path of a kernel that is one problem's latency.)
  auto lsync = []() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
  auto unsettle = [&]() { if (tid == 0 && a.unsettled) atomicAdd(a.unsettled, 1); };
  if (a.mask && a.mask[b] <= 1) {
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    unsettle();
    return;
  }
  if (a.skip_path && a.skip_path[b] != 0 && !(a.qr_mask && a.qr_mask[b] == 0)) return;
  double tau = 0.0;                                     // certificate stage 3: factor C - tau I
  if (a.cert_shift) {
    if (!a.cert_flag[b]) return;                        // (wave-uniform)
    tau = a.cert_tau[b];
  }
  const int N = a.ncols_dev ? a.ncols_dev[b] : a.n + 1;
  if (N <= 1) {                                         // (dogbox: every variable active — nothing to factor)
    if (tid == 0 && a.fb_mask) a.fb_mask[b] = 0;
    unsettle();
    return;
  }
  const int n = N - 1;
  const int NT = (N + 15) / 16;
  const int* gidx = a.gather ? a.gather + (long)b * a.stride_vec : nullptr;
  auto src = [&](int i) -> int { return gidx ? (i < n ? gidx[i] : a.n) : i; };
  const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;    // source Gram (may alias the output)
  double* Gb = a.G + (long)b * NPAD * NPAD;             // output triangle
  const RegLds L(sh_all, wv, NPAD);
  double *dl = L.dl, *sq = L.sq, *sc = L.sc, *td = L.td, *cv = L.cv, *yv = L.yv, *Dt = L.Dt, *Ria = L.Ria;
  double *tv = L.tv, *xs = L.xs;
  double* vv = L.v0;               // [NPAD] g of the free variables   (dogbox finish below)
  double* wq = L.v1;               // [NPAD] sq . g
  const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
  const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
  const double sa = a.diag_sqrt ? a.diag_sqrt[b] : 0.0;
  int* sidx = (int*)Ria;           // [NPAD] source indices — only until the tiles are loaded (Ria is free till then)
  const bool stpr = pidx == 500; (void)stpr;
  CST(stpr, 0, 19, 0);
  // 0. column scales from the diagonal of H
  int bad = 0;
  for (int j = tid; j < NPAD; j += WAVE) {
    int sj;
    const double d = col_scale(Gs, NPAD, j, n, src, csv, edv, sa, tau, dl, sq, sc, td, bad, sj);
    sidx[j] = sj < NPAD ? sj : 0;                       // source row / column of index j (always a valid one)
    if (a.dsc) a.dsc[(long)b * NPAD + j] = d;
  }
  wsync();
  if (a.colinfo && tid == 0) {                          // column-norm summary for the rank gate
    double mn = __builtin_inf(), sm = 0.0;
    double mx = 0.0;
    for (int j = 0; j < n; ++j) { const double v = sq[j]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; sm = fma(v, v, sm); }
    a.colinfo[2 * (long)b] = mn; a.colinfo[2 * (long)b + 1] = sm;
    if (a.hmax) a.hmax[b] = mx * mx;
    if (a.lam_out) a.lam_out[b] = (double)n;
    tv[0] = mn; tv[1] = sm;                             // (kept for the dogbox finish)
  }
  bad = __any(bad);
  CST(stpr, 0, 19, 1);
  // 1. the scaled source tiles -> accumulators
  v4d acc[NTILE];
  if (!bad) reg_load_tiles<true>(acc, Gs, NPAD, N, NT, sc, td, [&](int i) { return sidx[i]; });
  wsync();
  if (bad) {                                            // hand the problem to the QR tree
    if (tid == 0 && a.fb_mask) {
      a.fb_mask[b] = a.n + 1; { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }   // (the tree factors ALL n + 1 columns)
      if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = 0.0;
      if (a.path_out) a.path_out[b] = a.n + 1;
      if (a.k2_out && !a.cert_shift) a.k2_out[b] = 0.0;
    }
    unsettle();
    return;
  }
  // strictly lower tiles and everything beyond 16 NT are part of the triangle's image: zero
  // (tile by tile in the accumulators' lane layout: 4 stores per tile, none of them waited for)
#pragma unroll
  for (int ti = 0; ti < MT; ++ti) {
#pragma unroll
    for (int tj = 0; tj < MT; ++tj) {
      if (16 * ti < NPAD && 16 * tj < NPAD && (ti >= NT || tj < ti || tj >= NT)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * ti + lr + 4 * g, col = 16 * tj + lc;
          if (row < NPAD && col < NPAD) Gb[(long)row * NPAD + col] = 0.0;
        }
      }
    }
  }
  CST(stpr, 0, 19, 2);
  // 2. the factorisation; all 15 tiles of R' stay in registers (certificate), each row block is stored as R = R' D^-1
  const double pmin = reg_factor<true>(
      acc, Dt, Ria, cv, n, NT,
      [&](int kb, const double* Ri) {
        if (a.rinv) {                                   // kept for the conditioning certificate
          double* ro = a.rinv + ((long)b * (NPAD / 16) + kb) * 256;
#pragma unroll
          for (int q = 0; q < 4; ++q) ro[q * 64 + lane] = Ri[q * 64 + lane];
        }
      },
      [&](int kb, int j, const v4d& X) {
        const double sj = sq[16 * j + lc];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 16 * kb + lr + 4 * g;
          const int colg = 16 * j + lc;
          double val = X[g] * sj;
          if (row >= n || row > colg || colg > n) val = 0.0;
          Gb[(long)row * NPAD + colg] = val;
        }
      },
      lsync);
  const double kmax = a.k2_max > 0.0 ? a.k2_max : GRAM_K2_MAX;
  const bool fail = !(pmin >= (a.pivot_floor > 0.0 ? a.pivot_floor : 1.0 / GRAM_K2_MAX));
  if (tid == 0 && a.fb_mask) {
    if (a.pmin_out && !a.cert_shift) a.pmin_out[b] = pmin;
    a.fb_mask[b] = fail ? a.n + 1 : 0;
    if (a.path_out) a.path_out[b] = fail ? a.n + 1 : 0;
    if (fail) { const int fi_ = atomicAdd(a.fail_count, 1); if (a.fail_list) a.fail_list[fi_] = b; }
    if (fail && !a.cert_shift && a.k2_out) a.k2_out[b] = 0.0;      // (no bound for this factorisation)
    if (a.cert_shift) {
      a.cert_flag[b] = 0;
      if (!fail && a.k2_out) a.k2_out[b] = kmax;        // proven: kappa_2 <= Lambda / tau
    }
  }
  CST(stpr, 0, 19, 3);
  // 5. The first bound of the conditioning certificate (gram_cond_kernel below: same quantities, same
  //    definition) while R' and the inverse diagonal tiles are still at hand:
  //        K2 = ||R'||_1 ||R'||_inf ||Y||_1 ||Y||_inf ,   Y = R'^-T  column block by column block.
  //    K2 <= GRAM_K2_MAX settles the problem here; otherwise the separate kernel decides (it also
  //    has the tighter Frobenius bound).
  bool passed = false;
  if (a.cert_done) {
    double k2 = 0.0;
    if (!fail) {
      const int NTn = (n + 15) / 16;
      double r1 = 0.0, rinf = 0.0, y1 = 0.0, yinf = 0.0;
      double colp[MT];
#pragma unroll
      for (int jj = 0; jj < MT; ++jj) colp[jj] = 0.0;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (i < NTn) {
          double rp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int jj = i; jj < MT; ++jj) {
            if (jj < NTn) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int row = 16 * i + lr + 4 * g, col = 16 * jj + lc;
                const double v = (row < n && col < n) ? fabs(acc[tix(i, jj)][g]) : 0.0;
                rp[g] += v; colp[jj] += v;
              }
            }
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) rinf = fmax(rinf, row16_sum(rp[g]));
        }
      }
      rinf = wave_max(rinf);
#pragma unroll
      for (int jj = 0; jj < MT; ++jj) {
        if (jj < NTn) {
          xs[lane] = colp[jj];
          lsync();
          r1 = fmax(r1, (xs[lc] + xs[16 + lc]) + (xs[32 + lc] + xs[48 + lc]));
          lsync();
        }
      }
      r1 = wave_max(r1);
      double rsY[MT][4];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) rsY[i][g] = 0.0;
#pragma unroll
      for (int jj = 0; jj < MT; ++jj) {
        if (jj < NTn) {
          v4d Yc[MT];
          double cY = 0.0;
#pragma unroll
          for (int i = jj; i < MT; ++i) {
            if (i < NTn) {
              v4d Yt = {0.0, 0.0, 0.0, 0.0};
              if (i == jj) {
#pragma unroll
                for (int g = 0; g < 4; ++g) Yt[g] = Ria[jj * 256 + lc * 16 + lr + 4 * g];   // (R'_jj^-1)^T
              } else {
                v4d av = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = jj; kk < i; ++kk) {
#pragma unroll
                  for (int s_ = 0; s_ < 4; ++s_) av = mfma_f64(acc[tix(kk, i)][s_], Yc[kk][s_], av);
                }
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) Yt = mfma_f64(-Ria[i * 256 + (4 * s_ + lr) * 16 + lc], av[s_], Yt);
              }
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int row = 16 * i + lr + 4 * g, col = 16 * jj + lc;
                const double v = (row < n && col < n) ? Yt[g] : 0.0;
                Yt[g] = v;
                const double av_ = fabs(v);
                rsY[i][g] += row16_sum(av_);
                cY += av_;
              }
              Yc[i] = Yt;
            }
          }
          xs[lane] = cY;
          lsync();
          y1 = fmax(y1, (xs[lc] + xs[16 + lc]) + (xs[32 + lc] + xs[48 + lc]));
          lsync();
        }
      }
      y1 = wave_max(y1);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) yinf = fmax(yinf, rsY[i][g]);
      yinf = wave_max(yinf);
      k2 = (r1 * rinf) * (y1 * yinf);
      passed = k2 <= kmax;                              // (NaN fails)
    }
    if (tid == 0) {
      a.cert_done[b] = passed ? 1 : 0;
      if (passed && a.k2_out) a.k2_out[b] = k2;
    }
  }
  CST(stpr, 0, 19, 4);
  // 5b. TRF finish (GramCholArgs::lmfin): the `sure` branch of lm_gate_kernel, same expressions
  if (a.lmfin.fast && tid == 0) {
    bool finished = false;
    if (!fail && passed && a.colinfo && a.lmfin.enable != 0 && a.lmfin.m >= n) {
      const double mn = tv[0], sm = tv[1];
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
    if (!finished) unsettle();
  }
  CST(stpr, 0, 19, 5);
  // 6. dogbox finish (GramCholArgs::dog): what dog_gate_solve_kernel computes for a problem on this path —
  //    Cauchy step -(g.g)/(J_f g . J_f g) g_f with |J_f g_f| = |R g_f|, and, when the column-norm bound
  //    already proves the free block full rank (the `sure` case there), the Newton step -R_f^-1 c_f —
  //    from the register tiles:  R = R' diag(sq),  c = c' sq_n.
  if (a.dog.g) {
    bool finished = false;
    if (!fail && a.colinfo) {
      const int NTn = (n + 15) / 16;
      const double mn = tv[0], sm = tv[1];
      lsync();
      const double* gb = a.dog.g + (long)b * a.stride_vec;
      double gg = 0.0;
      for (int q = lane; q < NPAD; q += WAVE) {
        const double gq = (q < n) ? gb[gidx ? gidx[q] : q] : 0.0;
        vv[q] = gq; wq[q] = gq * sq[q]; yv[q] = 0.0;
        gg = fma(gq, gq, gg);
      }
      gg = wave_sum(gg);
      lsync();
      double uu = 0.0;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (i < NTn) {
          double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int jj = i; jj < MT; ++jj) {
            if (jj < NTn) {
              const double wj = wq[16 * jj + lc];
#pragma unroll
              for (int g = 0; g < 4; ++g) part[g] = fma(acc[tix(i, jj)][g], wj, part[g]);
            }
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const double u = row16_sum(part[g]);
            if (lc == 0 && 16 * i + lr + 4 * g < n) uu = fma(u, u, uu);
          }
        }
      }
      uu = wave_sum(uu);
      const double fac = -gg / uu;
      for (int q = lane; q < n; q += WAVE) a.dog.cauchy[(long)b * a.stride_vec + q] = fac * vv[q];
      const int mx = a.dog.m > n ? a.dog.m : n;
      const bool sure = is_finite(sm) && sm > 0.0 && (GRAM_SMIN_PROVEN * mn > LM_GATE_MARGIN * DBL_EPS * mx * sqrt(sm));
      if (a.dog.enable != 0 && a.dog.m >= n && sure) {
        // y = R'^-1 c', newton = -sq_n dl . y
        reg_back_solve(acc, Ria, cv, yv, tv, n, lsync);
        const double sqn = sq[n];
        for (int q = lane; q < n; q += WAVE) a.dog.newton[(long)b * a.stride_vec + q] = -(sqn * dl[q] * yv[q]);
        finished = true;
      }
    }
    if (tid == 0) {
      a.dog.done[b] = finished ? 1 : 0;
      if (finished) { a.dog.fast[b] = 1; a.dog.ncols_jac[b] = 0; }
      if (!(finished && passed)) unsettle();
    }
  }
  CST(stpr, 0, 19, 6);
}

// ---- N <= 80: ALL Newton rounds of a problem in one launch ----------------------------------------
// The safeguarded Newton iteration on alpha (trust_region.py:126-150) factors H + alpha I once per
// round.  For N <= 80 one wave owns a problem for the whole iteration: per round the factor of
// gram_chol_reg_kernel (tiles in registers, nothing stored), p = -R^-1 c by block back substitution
// and q = R^-T p by block forward substitution straight from the register tiles (tile x vector: four
// FMAs per lane and tile + a 16-lane DPP sum, or a four-row sum through LDS for the transposed
// product; the 16 x 16 diagonal solves are matvecs with the inverse tiles the chain produces anyway),
// then the scalar update of lm_update_kernel, verbatim.  No launch, no counter read-back and no
// triangle written between rounds (six stream operations per round otherwise, each with its dispatch
// gap).  Everything happens in the equilibrated system:  R = R' diag(sq),  c = c' sq_n  =>
//     p_j = -sq_n dl_j (R'^-1 c')_j ,      q = R'^-T (dl . p) .
__device__ __forceinline__ double lm_restart_reg(double lo, double hi) {     // trust_region.py:128,134
  const double gm = sqrt(lo * hi);
  return (0.001 * hi > gm) ? 0.001 * hi : gm;
}
// The launch first does what lm_start_kernel does — the Gauss-Newton step from the AUGMENTED factor
// (its stored triangle, column scales and inverse diagonal tiles are re-loaded: R' = R diag(dl)), the
// acceptance test |p| <= Delta and the bracket (trust_region.py:116-130) — for every
// normal-equations-path problem of the batch (the others are left to lm_start and the round loop,
// LmState.fused_gram): no list, no counter, and the same arithmetic for a problem whatever else its
// batch holds.
__global__ __launch_bounds__(REG_NT, 1) void lm_rounds_reg_kernel(GramCholArgs a, LmState lm,
                                                                 const double* Delta_in,
                                                                 const double* alpha_in) {
  extern __shared__ double sh_all[];
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int b = reg_problem((int)blockIdx.x, wv);
  if (b >= lm.B) return;
  if (lm.path && lm.path[b] != 0) return;               // (Householder-path problem: lm_start and the round loop)
  const int lane = threadIdx.x & 63, lr = lane >> 4, lc = lane & 15;
  if (!lm.fast[b]) {
    if (lane == 0) lm.ncols_lm[b] = 0;
    return;
  }
  double* scv = lm.sc + (long)b * 16;
  int* stv = lm.st + (long)b * 4;
  int phase = LM_EVAL;
  const int NPAD = a.NPAD, n = a.n, N = n + 1;
  const int NT = (N + 15) / 16, NTn = (n + 15) / 16;
  const RegLds L(sh_all, wv, NPAD);
  double *dl = L.dl, *sq = L.sq, *sc = L.sc, *td = L.td, *cv = L.cv, *Dt = L.Dt, *Ria = L.Ria, *tv = L.tv, *xs = L.xs;
  double* yv = L.yv;               // [NPAD] R'^-1 c', then dl . p
  double* pv = L.v0;               // [NPAD] p
  double* zv = L.v1;               // [NPAD] R'^-T (dl . p)
  auto wsync = []() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); };
  const double* Gs = a.Gsrc + (long)b * NPAD * NPAD;
  const double* csv = a.colscale ? a.colscale + (long)b * a.stride_vec : nullptr;
  const double* edv = a.diag_vec ? a.diag_vec + (long)b * a.stride_vec : nullptr;
  v4d acc[NTILE];
  double sqn = 1.0;

  // p = -sq_n dl . y -> pv,  w = dl . p -> yv;  returns |p|
  auto form_p = [&]() -> double {
    double pp = 0.0;
    for (int j = lane; j < NPAD; j += WAVE) {
      const double pj = (j < n) ? -(sqn * dl[j] * yv[j]) : 0.0;
      pv[j] = pj;
      pp = fma(pj, pj, pp);
    }
    wsync();
    for (int j = lane; j < NPAD; j += WAVE) yv[j] = (j < n) ? dl[j] * pv[j] : 0.0;
    const double pn_ = sqrt(wave_sum(pp));
    wsync();
    return pn_;
  };
  // z = R'^-T w (w in yv), block rows from the top -> zv;  returns |z|^2
  auto fwd_solve = [&]() -> double {
#pragma unroll
    for (int kk = 0; kk < MT; ++kk) {
      if (kk < NTn) {
        double part = 0.0;
#pragma unroll
        for (int j = 0; j < kk; ++j) {
#pragma unroll
          for (int g = 0; g < 4; ++g) part = fma(acc[tix(j, kk)][g], zv[16 * j + lr + 4 * g], part);
        }
        xs[lane] = part;
        wsync();
        const double tot = (xs[lc] + xs[16 + lc]) + (xs[32 + lc] + xs[48 + lc]);
        if (lr == 0) tv[lc] = yv[16 * kk + lc] - tot;
        wsync();
        const int nb = (n - 16 * kk < 16) ? n - 16 * kk : 16;
        const double* Rk = Ria + kk * 256;
        double zi = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) zi = fma(Rk[c * 16 + lc], (c <= lc) ? tv[c] : 0.0, zi);
        if (lc >= nb) zi = 0.0;
        if (lr == 0) zv[16 * kk + lc] = zi;
        wsync();
      }
    }
    double qq = 0.0;
    for (int j = lane; j < NPAD; j += WAVE) { const double zj = (j < n) ? zv[j] : 0.0; qq = fma(zj, zj, qq); }
    return wave_sum(qq);
  };

  double alpha, lo, hi, phi, dphi, Delta;
  int it, n_iter;
  // ---- the augmented factor back into registers:  R' = R diag(dl),  Ri from the factor kernel ----
  Delta = Delta_in[b];
  const double* Ra = lm.Raug + (long)b * NPAD * NPAD;
  const double* dsc = a.dsc + (long)b * NPAD;
  const double* rinv = a.rinv + (long)b * (NPAD / 16) * 256;
  for (int j = lane; j < NPAD; j += WAVE) { dl[j] = dsc[j]; yv[j] = 0.0; pv[j] = 0.0; zv[j] = 0.0; }
  for (int e = lane; e < NT * 256; e += WAVE) Ria[e] = rinv[e];
  wsync();
  sqn = 1.0 / dl[n];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = i; j < MT; ++j) {
      v4d v4 = {0.0, 0.0, 0.0, 0.0};
      if (j < NT) {
        const int col = 16 * j + lc;
        const double dj = dl[col];
#pragma unroll
        for (int g = 0; g < 4; ++g) v4[g] = Ra[(long)(16 * i + lr + 4 * g) * NPAD + col] * dj;
      }
      acc[tix(i, j)] = v4;
    }
  }
  for (int r = lane; r < NPAD; r += WAVE) cv[r] = (r < n) ? Ra[(long)r * NPAD + n] * dl[n] : 0.0;
  wsync();
  // |R^T c| = sq_n |sq . (R'^T c')|  (alpha_upper = |A^T b| / Delta, trust_region.py:111-113)
  double gg = 0.0;
#pragma unroll
  for (int kk = 0; kk < MT; ++kk) {
    if (kk < NTn) {
      double part = 0.0;
#pragma unroll
      for (int j = 0; j <= kk; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) part = fma(acc[tix(j, kk)][g], cv[16 * j + lr + 4 * g], part);
      }
      xs[lane] = part;
      wsync();
      const double tot = (xs[lc] + xs[16 + lc]) + (xs[32 + lc] + xs[48 + lc]);
      const int col = 16 * kk + lc;
      const double gj = (col < n) ? tot / dl[col] : 0.0;
      if (lr == 0) gg = fma(gj, gj, gg);
      wsync();
    }
  }
  const double gnorm = sqn * sqrt(wave_sum(gg));
  reg_back_solve(acc, Ria, cv, yv, tv, n, wsync);
  const double pn = form_p();
  for (int j = lane; j < n; j += WAVE) lm.ph[(long)b * lm.ld + j] = pv[j];
  if (pn <= Delta) {                                    // trust_region.py:116-117
    if (lane == 0) {
      scv[SC_ALPHA] = 0.0; stv[ST_NITER] = 0; stv[ST_PHASE] = LM_IDLE; scv[SC_DELTA] = Delta;
      lm.ncols_lm[b] = 0;
    }
    return;
  }
  const double qq = fwd_solve();                        // phi(0), phi'(0) -> alpha_lower (:121-123)
  phi = pn - Delta;
  dphi = -qq / pn;
  hi = gnorm / Delta;
  lo = -phi / dphi;
  alpha = alpha_in[b];                                  // :127-130 (full rank)
  if (alpha < lo || alpha > hi) alpha = lm_restart_reg(lo, hi);   // :133-134, iteration 0
  it = 0; n_iter = 0;
  if (lane == 0) scv[SC_DELTA] = Delta;
  for (int guard = 0; guard < 12; ++guard) {
    const double sa = sqrt(alpha);
    // ---- factor of H + alpha I (as gram_chol_reg_kernel; no gather, nothing stored) ----
    for (int j = lane; j < NPAD; j += WAVE) {
      int bad = 0, sj;                                  // (the problem has passed the gate; no gather)
      col_scale(Gs, NPAD, j, n, [](int i) { return i; }, csv, edv, sa, 0.0, dl, sq, sc, td, bad, sj);
      yv[j] = 0.0; pv[j] = 0.0; zv[j] = 0.0;
    }
    wsync();
    sqn = sq[n];
    reg_load_tiles<false>(acc, Gs, NPAD, N, NT, sc, td, [](int i) { return i; });
    wsync();
    reg_factor<false>(acc, Dt, Ria, cv, n, NT, [](int, const double*) {}, [](int, int, const v4d&) {}, wsync);
    reg_back_solve(acc, Ria, cv, yv, tv, n, wsync);
    const double pn = form_p();
    bool finished = false;
    if (phase == LM_FINAL) {
      finished = true;                                  // p at the updated alpha, rescale test on the STALE phi (:149)
    } else {
      const double qq = fwd_solve();
      // ---- the update of lm_update_kernel (trust_region.py:136-146) ----
      phi = pn - Delta;
      dphi = -qq / pn;
      if (fabs(phi) < 0.01 * Delta) {                   // :138-139
        finished = true;
        n_iter = it + 1;
      } else {
        if (phi < 0.0) hi = alpha;                      // :141-142
        const double ratio = phi / dphi;
        const double cand = alpha - ratio;
        lo = (cand > lo) ? cand : lo;                   // :145
        alpha -= (phi + Delta) * ratio / Delta;         // :146
        ++it;
        if (it >= 10) {                                 // max_iter reached: final p at the new alpha
          n_iter = 10;
          phase = LM_FINAL;
        } else {
          if (alpha < lo || alpha > hi) alpha = lm_restart_reg(lo, hi);   // :133-134 of the next pass
          phase = LM_EVAL;
        }
      }
    }
    if (finished) {
      const double f = (phi > 0.0) ? Delta / pn : 1.0;  // :149-150
      for (int j = lane; j < n; j += WAVE) lm.ph[(long)b * lm.ld + j] = pv[j] * f;
      break;
    }
  }
  if (lane == 0) {
    scv[SC_ALPHA] = alpha; scv[SC_LO] = lo; scv[SC_HI] = hi; scv[SC_PHI] = phi; scv[SC_DPHI] = dphi;
    stv[ST_IT] = it; stv[ST_PHASE] = LM_IDLE; stv[ST_NITER] = n_iter;
    lm.sa[b] = sqrt(alpha);
    lm.ncols_lm[b] = 0;
  }
}

hipError_t launch_lm_rounds_reg(const GramCholArgs& c, const LmState& lm, const double* Delta,
                                const double* alpha_in, hipStream_t s) {
  const size_t lds = sizeof(double) * reg_lds_doubles(c.NPAD) * REG_NW;
  return launch<lm_rounds_reg_kernel>(dim3(reg_grid(lm.B)), dim3(REG_NT), lds, s, c, lm, Delta, alpha_in);
}

// launch_gram_chol for NPAD <= 80 (a.count set): one wave per problem, REG_NW per workgroup
hipError_t launch_gram_chol_reg(const GramCholArgs& a, hipStream_t s) {
  const size_t lds = sizeof(double) * reg_lds_doubles(a.NPAD) * REG_NW;
  return launch<gram_chol_reg_kernel>(dim3(reg_grid(a.count)), dim3(REG_NT), lds, s, a);
}

#ifdef BLSQ_CHOL_STAMPS
int chol_reg_debug_stamps(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_chol_st), sizeof(g_chol_st));
}
#endif

}  // namespace blsq
