// C-ABI entry points (include/blsq.h): the TRF plans — factor / step / fetch — and the row-split (TSQR) plans.
#include "blsq_host.h"

// ================================================================== TRF ====
namespace blsq_host {


int trf_alloc_state(blsq_trf_plan* p) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, ld = p->ld;
  const size_t mat = (size_t)ld * ld;
  if (int rc_ = alloc_all(ctx, {
          {&p->X, sizeof(double) * B * mat, "hipMalloc(p->X)"},
          {&p->vecs, sizeof(double) * (size_t)B * ld * 13, "hipMalloc(p->vecs)"},
          {&p->scal2, sizeof(double) * (size_t)B * 8, "hipMalloc(p->scal2)"},
          {&p->sweeps, sizeof(int) * (size_t)B, "hipMalloc(p->sweeps)"},
          {&p->o_vec, sizeof(double) * (size_t)B * ld * 4, "hipMalloc(p->o_vec)"},
          {&p->o_hits, sizeof(long long) * (size_t)B * ld, "hipMalloc(p->o_hits)"},
          {&p->o_act, sizeof(long long) * (size_t)B * ld, "hipMalloc(p->o_act)"},
          {&p->o_scal, sizeof(double) * (size_t)B * 8, "hipMalloc(p->o_scal)"},
          {&p->o_info, sizeof(int) * (size_t)B * 4, "hipMalloc(p->o_info)"},
          {&p->in_scal, sizeof(double) * (size_t)B * 2, "hipMalloc(p->in_scal)"},
      })) return rc_;
  HIPCHK(ctx, hipMemsetAsync(p->vecs.p, 0, p->vecs.bytes, ctx->stream));
  double* v = p->vecs.as<double>();
  const size_t vs = (size_t)B * ld;
  TrfState& st = p->st;
  st.B = B; st.m = p->m_total; st.n = p->n; st.ld = ld;
  st.X = p->X.as<double>();
  st.x = v; st.lb = v + vs; st.ub = v + 2 * vs; st.scale = v + 3 * vs;
  st.g = v + 4 * vs; st.v = v + 5 * vs; st.d = v + 6 * vs; st.g_h = v + 7 * vs;
  st.diag_h = v + 8 * vs; st.s = v + 9 * vs; st.uf = v + 10 * vs; st.ediag = v + 11 * vs;
  st.scale_in = v + 12 * vs;
  double* sc = p->scal2.as<double>();
  st.srange = sc; st.g_norm = sc + 2 * (size_t)B; st.theta = sc + 3 * (size_t)B;
  double* ov = p->o_vec.as<double>();
  p->out.step_h = ov; p->out.step = ov + vs; p->out.x_new = ov + 2 * vs;
  p->out.p_h_tr = ov + 3 * vs;
  p->out.hits = p->o_hits.as<long long>();
  p->out.active_new = p->o_act.as<long long>();
  p->out.scal = p->o_scal.as<double>();
  p->out.info = p->o_info.as<int>();
  if (int rc_ = alloc_all(ctx, {
          {&p->lm_sa, sizeof(double) * (size_t)B, "hipMalloc(p->lm_sa)"},
          {&p->lm_Xa, sizeof(double) * B * mat, "hipMalloc(p->lm_Xa)"},
          {&p->lm_ints, sizeof(int) * ((size_t)B * 9 + 16), "hipMalloc(p->lm_ints)"},
          {&p->aug_colinfo, sizeof(double) * (size_t)B * 2, "hipMalloc(p->aug_colinfo)"},
          {&p->aug_hmax, sizeof(double) * (size_t)B, "hipMalloc(p->aug_hmax)"},
          {&p->aug_lam, sizeof(double) * (size_t)B, "hipMalloc(p->aug_lam)"},
          {&p->aug_ym, sizeof(double) * (size_t)B, "hipMalloc(p->aug_ym)"},
          {&p->aug_r1, sizeof(double) * (size_t)B, "hipMalloc(p->aug_r1)"},
          {&p->aug_open, sizeof(double) * (size_t)B, "hipMalloc(p->aug_open)"},
          {&p->aug_mask, sizeof(int) * (size_t)B, "hipMalloc(p->aug_mask)"},
          {&p->lm_sc, sizeof(double) * (size_t)B * 16, "hipMalloc(p->lm_sc)"},
          {&p->lm_ph, sizeof(double) * vs, "hipMalloc(p->lm_ph)"},
      })) return rc_;
  HIPCHK(ctx, hipMemsetAsync(p->lm_sa.p, 0, p->lm_sa.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->aug_ym.p, 0, p->aug_ym.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->aug_open.p, 0, p->aug_open.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->lm_Xa.p, 0, p->lm_Xa.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->lm_ints.p, 0, p->lm_ints.bytes, ctx->stream));
  {
    LmState& lm = p->lm;
    lm.B = B; lm.m = p->m_total; lm.n = p->n; lm.ld = ld; lm.opt = &ctx->opt;
    lm.Raug = p->X.as<double>(); lm.sa = p->lm_sa.as<double>(); lm.Xa = p->lm_Xa.as<double>();
    lm.g_h = p->st.g_h;
    int* ii = p->lm_ints.as<int>();
    lm.fast = ii; lm.ncols_jac = ii + B; lm.ncols_lm = ii + 2 * (size_t)B; lm.st = ii + 3 * (size_t)B;
    lm.active_count = ii + 7 * (size_t)B;
    lm.active_list = ii + 7 * (size_t)B + 16; lm.round = 0;
    lm.sc = p->lm_sc.as<double>(); lm.ph = p->lm_ph.as<double>();
    // Householder-path problems: the SVD-free Newton iteration costs one small stacked QR per
    // iteration.  Measured in round 1 (8192..16384 problems per launch, Delta mix 10/0.5; SVD-free vs
    // Jacobi-SVD step-solves/s): 64x8 5.3M vs 3.4M, 128x16 6.2M vs 2.9M (one panel: the QR is trivial),
    // 256x32 1.55M vs 1.73M, 512x40 0.90M vs 0.90M, 512x48 0.98M vs 0.89M, 512x64 0.76M vs 0.70M.  So for
    // THEM the Jacobi SVD keeps the band 16 < n < 48, where a round of tiny two-panel QRs costs as much
    // as the whole in-LDS SVD.  Normal-equations-path problems have no such band: their rounds are one
    // launch (lm_rounds_reg_kernel) — 256x32: 6.6M vs 2.4M, 512x40: 5.1M vs 1.3M, 128x24: 9.8M vs 2.9M.
    // BLSQ_SVDFREE_MIN_N overrides the upper edge of the band (0: none), BLSQ_NO_SVDFREE=1 forces the SVD.
    const int min_n = ctx->opt.i(OPT_SVDFREE_MIN_N);
    const bool band = p->n > 16 && p->n < min_n;
    p->lm_enable = ctx->opt.i(OPT_NO_SVDFREE) == 1 ? 0 : 1;
    p->lm_gate_mask = p->lm_enable ? (band ? 2 : 3) : 0;
  }
  // CSNE tier: single-rank plans of its shapes with the normal-equations front end on (BLSQ_CSNE = 0: off)
  if (p->tree.gram && p->nranks == 1 && csne_supported(p->m, p->n) && ctx->opt.on(OPT_CSNE)) {
    int rc = p->csne.build(ctx, B, p->m, p->n, ld, /*with_hp=*/true);
    if (rc) return rc;
    const CsneState& cs = p->csne.cs;
    p->st.csne = cs.flag; p->st.csne_hp = cs.hp;
    p->lm.csne = cs.flag; p->lm.csne_ne = cs.ne; p->lm.csne_alpha = cs.ralpha;
  }
  p->aug_RP = std::max(aug_rows(p->n), ld);
  if (aug_rows(p->n) > RMAX) return ctx->bad(4, "n too large for the augmented system (n <= 512)");
  p->aug_LDP = 0;
  return 0;
}

// ---- after the front end --------------------------------------------------------------------------
// Two ways into the n-space path:
//   trf_after_triangle   a triangle [R c] of [J f] is given for every problem (front end off, TSQR
//                        merge): prep from R, stacked QR of [R D; E]
//   trf_gram_stage ...   the normal-equations path: prep from the Gram, H = D G D + E^2 factored by
//                        Cholesky, and the conditioning gate applied to THAT factor — the system the
//                        step is solved from.  No triangle of J is ever formed for such a problem;
//                        a problem the gate rejects is factored by the Householder tree and prepared
//                        again from its triangle (trf_fallback_stage).
int trf_finish(blsq_trf_plan* p) {
  blsq_ctx* ctx = p->ctx;
  if (p->use_qr || p->njac != 0 || !p->gate_done) p->x_dirty = true;   // (a stacked QR or a Jacobi launch may follow)
  if (p->use_qr) {
    // E = 0 (unbounded problems): [R D | c] is the triangle already — written by a copy, masked out of the QR
    if (int rc_ = ctx->run(K_QR_AUG, "launch_trf_aug_trivial", [&] {
          return launch_trf_aug_trivial(p->st, p->path, p->aug_mask.as<int>(), nullptr, ctx->stream);
        })) return rc_;
    QrArgs q = p->tree.base_args();
    q.ncols_dev = p->aug_mask.as<int>();
    // source = R read in place, columns scaled by d on the fly, on top of the VIRTUAL block
    // E = diag(ediag): [R D | c ; E | 0] is never written to memory
    q.A = p->st.Rt; q.strideA = (long)p->ld * p->ld; q.ldA = p->ld;
    q.rowsA = aug_block_rows(p->n) + p->n;
    q.vdiag_row0 = aug_block_rows(p->n); q.vdiag_vec = p->st.ediag;
    q.colscale = p->st.d; q.stride_vec = p->ld;
    q.F = nullptr; q.strideF = 0;
    q.rows_per_leaf = p->aug_RP; q.RP = p->aug_RP; q.LDP = p->aug_LDP;
    q.Rout = p->st.X;
    q.stack_rows = aug_block_rows(p->n); // [R D; E]: two upper-triangular blocks
    if (int rc_ = ctx->run(K_QR_AUG, "launch_qr(aug)", [&] { return launch_qr(q, 1, p->B, ctx->stream); })) return rc_;
  }
  // rank gate: clearly full-rank problems skip the SVD (lm_kernels.hip)
  if (!p->gate_done) {
    p->lm.jac_count = nullptr;
    if (int rc_ = ctx->run(K_LM_GATE, "launch_lm_gate", [&] {
          return launch_lm_gate(p->lm, p->lm_gate_mask, ctx->stream);
        })) return rc_;
    p->njac = -1;
  }
  p->gate_done = false;
  if (p->njac == 0) return 0;             // nobody needs the SVD: no launch
  return run_jacobi(p, p->st.X, p->st.s, p->st.uf, p->st.srange, p->lm.ncols_jac);
}

// redo: the problems were prepared from their Gram already in this factor call — start again from the
// scale the caller passed (a 'jac' scaling update is applied once, to the caller's vector)
int trf_after_triangle(blsq_trf_plan* p, const double* Rt, int scale_mode, int redo = 0) {
  blsq_ctx* ctx = p->ctx;
  p->st.Rt = Rt; p->st.Gk = nullptr; p->st.path = nullptr;
  p->path = nullptr; p->use_chol = false; p->use_qr = true;
  p->lm.path = nullptr; p->lm.colinfo = nullptr; p->lm.hmax = nullptr; p->lm.k2 = nullptr; p->gram_valid = false;
  p->tree.path_valid = false; p->tree.any_gram = false; p->tree.any_qr = true;
  p->gate_done = false;
  if (int rc_ = ctx->run(K_PREP, "launch_trf_prep", [&] {
        return launch_trf_prep(p->st, scale_mode, 0, nullptr, redo, ctx->stream);
      })) return rc_;
  return trf_finish(p);
}

GramCholArgs trf_chol_args(blsq_trf_plan* p, const int* mask) {
  QrTree& t = p->tree;
  GramCholArgs c = t.gate_args(mask);
  c.G = p->st.X; c.colscale = p->st.d; c.diag_vec = p->st.ediag;
  c.colinfo = p->aug_colinfo.as<double>();
  c.hmax = p->aug_hmax.as<double>(); c.lam_out = p->aug_lam.as<double>();
  if (p->csne.on) c.pmin_out = p->csne.pmin.as<double>();
  if (p->ld > 80) {
    c.cert_ym = p->aug_ym.as<double>(); c.cert_r1 = p->aug_r1.as<double>();
    // (cert_direct = 0: every open problem through the norm stage, the explicit inverse)
    c.cert_open = p->ctx->opt.on(OPT_CERT_DIRECT) ? p->aug_open.as<double>() : nullptr;
  }
  // (N <= 80: the register-resident factor kernel also does the rank gate's sure case; N > 80: stage 0 of the certificate
  //  does — gram_cert0_kernel — for the problems it certifies.  `unsettled` counts the others.)
  c.lmfin.fast = p->lm.fast; c.lmfin.ncols_jac = p->lm.ncols_jac; c.lmfin.sc = p->lm.sc; c.lmfin.st = p->lm.st;
  c.unsettled = t.fb_count() + 2;
  c.lmfin.m = p->lm.m; c.lmfin.enable = (p->lm_gate_mask >> 1) & 1;
  return c;
}

// the second half of the certificate + the rank gate of the trust-region solver (counters:
// fb_count()[0] problems that leave the path, [1] problems for the SVD)
int trf_gate_tail(blsq_trf_plan* p, const GramCholArgs& c, bool full = true) {
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  if (int rc_ = t.run_cert(ctx, c)) return rc_;
  // The rank gate runs BEFORE the verdict is read back: in the common case (no problem leaves this
  // path) its result stands, and the same read-back tells whether anybody needs the Jacobi SVD at all.
  p->lm.path = t.path_rw();
  p->lm.colinfo = p->aug_colinfo.as<double>();
  p->lm.jac_count = t.fb_count() + 1;
  // (normal-equations-path problems only: a problem the certificate has just rejected gets its triangle first and
  //  is gated by trf_finish afterwards — estimating the rank of its abandoned factor here cost the latency of one
  //  problem's inverse iteration for nothing; such a problem counts as "needs the SVD" until then, which the verdict
  //  logic ignores whenever a problem left the path)
  //  (`full`: every problem is refreshed by this call — a masked call keeps the others' state as it is)
  return ctx->run(K_LM_GATE, "launch_lm_gate", [&] {
    return launch_lm_gate(p->lm, full ? (p->lm_gate_mask & 2) : p->lm_gate_mask, ctx->stream);
  });
}

// prep from the Gram, Cholesky of H with the pivot gate, conditioning gate; *nfb = problems of this
// call that must go to the Householder tree (their indices are flagged in tree.fb_mask()).
int trf_gram_stage(blsq_trf_plan* p, int scale_mode, const int* mask, int* nfb, bool defer = false) {
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  p->st.Rt = t.Rfinal(); p->st.Gk = t.gram_keep.as<double>(); p->st.path = t.path_rw();
  const PackVecs* pk = nullptr;
  { int rc_ = take_pack(p, mask, &pk); if (rc_) return rc_; }
  if (int rc_ = ctx->run(K_PREP, "launch_trf_prep(gram)", [&] {
        return launch_trf_prep(p->st, scale_mode, 1, mask, 0, ctx->stream, pk);
      })) return rc_;
  GramCholArgs c = trf_chol_args(p, mask);
  c.skip_zero = p->x_dirty ? 0 : 1;
  if (!mask) p->x_dirty = false;                        // (every slot is rewritten, zeros included, by this launch)
  if (int rc_ = ctx->run(K_AUG_CHOL, "launch_gram_chol(aug)", [&] {
        return launch_gram_chol(c, p->B, ctx->stream);
      })) return rc_;
  // second guess (N <= 80): the Cholesky kernel settles EVERY problem itself — certificate by its first
  // bound, rank gate by the column-norm bound — as it did in the last call: then the certificate and gate
  // launches would both be empty and are not enqueued (resolve() checks the settled counter)
  // N > 80: stage 0 of the certificate is still launched (it IS what settles a problem there) — the norm stage, the
  // shifted factorisation and the rank gate, three launches that would find nothing to do, are not.
  bool skip_tail = defer && p->guess_settled && c.lmfin.fast != nullptr;
  if (skip_tail && p->ld > 80 && (!c.cert_ym || !ctx->opt.on(OPT_CERT0))) skip_tail = false;
  int rc;
  if (skip_tail) {
    p->lm.path = t.path_rw();
    p->lm.colinfo = p->aug_colinfo.as<double>();
    if (p->ld > 80) {
      if (int rc_ = ctx->run(K_GRAM_GATE, "launch_gram_gate(stage 0)", [&] {
            return launch_gram_gate(c, p->B, ctx->stream, /*stage0_only=*/true);
          })) return rc_;
    }
  } else if ((rc = trf_gate_tail(p, c, mask == nullptr))) return rc;
  if (defer) {                              // the counters travel; the verdict is read by resolve()
    verdict_arm(p, skip_tail, p->pend_dJ, p->pend_df, p->pend_ldJ, p->pend_scale_mode);
    *nfb = 0;
  } else {                                  // (the synchronous verdict: published and polled for instead of a blit and a
    //  stream synchronisation)
    if ((rc = gate_verdict(p, /*polled=*/true, mask != nullptr, c.unsettled != nullptr, nfb))) return rc;
  }
  t.note_paths(ctx, *nfb, mask != nullptr);
  p->path = t.path_rw();
  p->use_chol = t.any_gram;
  p->use_qr = t.any_qr;
  p->lm.path = p->path;
  // Newton systems of Householder-path problems from the Gram where alpha makes them provably well
  // conditioned (LmState::hmax; BLSQ_LM_CHOL_QRPATH = 0: always the stacked QR)
  {
    const bool on = ctx->opt.on(OPT_LM_CHOL_QRPATH);
    p->lm.hmax = on ? p->aug_hmax.as<double>() : nullptr;
    p->lm.lam = p->aug_lam.as<double>();
    p->lm.k2_max = t.k2_max;
    p->lm.k2 = t.gram_k2.as<double>();
    p->lm.colinfo = p->aug_colinfo.as<double>();         // (written for every problem the Cholesky kernel looked at)
    p->gram_valid = true;
  }
  return 0;
}

// CSNE tier, factor side: which of the nfb problems the certificate has just rejected keep their Gram-Cholesky factor
// as a preconditioner and have their steps corrected against J (CsneTier::select); *ntree = the problems left for the
// other tiers.
int trf_csne_select(blsq_trf_plan* p, const double* dJ, const double* df, int ldJ, int nfb, int* ntree, bool masked) {
  CsneTier& tier = p->csne;
  QrTree& t = p->tree;
  *ntree = nfb;
  if (!tier.on || !p->lm_enable) return 0;
  if (!tier.ensure_recordings()) { tier.on = false; return 0; }   // (no room: the other tiers)
  p->lm.csne_vec = tier.cs.rvec;
  int rc = tier.select(p->ctx, t, trf_chol_args(p, t.fb_mask()), nfb, ntree, masked, [&](const int* sel) {
    return launch_csne_select(tier.cs, p->lm, nfb, t.fb_list(), t.fb_mask(), t.fb_count(), t.path_rw(), sel,
                              tier.k2.as<double>(), tier.pmin.as<double>(), p->aug_colinfo.as<double>(), p->ctx->stream);
  });
  if (rc) return rc;
  tier.cs.J = dJ; tier.cs.strideJ = (long)p->m * ldJ; tier.cs.ldJ = ldJ; tier.cs.F = df; tier.cs.strideF = p->m;
  p->use_chol = t.any_gram; p->use_qr = t.any_qr;
  return 0;
}

// the problems the gate rejected: the tier takes what it can, the Householder tree on [J f] the rest, which are
// prepared again from their triangle
int trf_fallback_stage(blsq_trf_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode,
                       int nfb, bool masked = false) {
  blsq_ctx* ctx = p->ctx;
  int rc;
  {
    int ntree = nfb;
    if ((rc = trf_csne_select(p, dJ, df, ldJ, nfb, &ntree, masked))) return rc;
    nfb = ntree;
    if (nfb == 0) return 0;
  }
  rc = p->tree.run_fallback(ctx, dJ, df, ldJ, nfb);
  if (rc) return rc;
  if (int rc_ = ctx->run(K_PREP, "launch_trf_prep(redo)", [&] {
        return launch_trf_prep(p->st, scale_mode, 0, p->tree.fb_mask(), 1, ctx->stream);
      })) return rc_;
  return 0;
}

// the whole factor call from device-resident [J f] (mask: outer driver, fresh Jacobians only)
int trf_factor_core(blsq_trf_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode,
                    const int* mask, bool may_defer, bool gram_done) {
  blsq_ctx* ctx = p->ctx;
  int rc;
  if ((rc = verdict_drop(p))) return rc;
  if (!p->tree.gram) {
    if ((rc = p->tree.run_levels(ctx, dJ, df, ldJ, mask))) return rc;
    return trf_after_triangle(p, p->tree.Rfinal(), scale_mode);
  }
  if (!gram_done && (rc = p->tree.run_gram_only(ctx, dJ, df, ldJ, mask, false))) return rc;
  p->last_scale_mode = scale_mode;
  if (!mask) p->csne.count = 0;                           // (the prep launch clears every flag; trf_csne_select sets them anew)
  int nfb = 0;
  // (never in the n-band that always takes the SVD, nor right after a wrong guess)
  const bool defer = may_defer && !mask && verdict_may_guess(p) && p->lm_enable && p->pend_pin;
  if ((rc = trf_gram_stage(p, scale_mode, mask, &nfb, defer))) return rc;
  if (defer) { p->pend_dJ = dJ; p->pend_df = df; p->pend_ldJ = ldJ; p->pend_scale_mode = scale_mode; }
  if (nfb > 0 && (rc = trf_fallback_stage(p, dJ, df, ldJ, scale_mode, nfb, mask != nullptr))) return rc;
  if (nfb == 0 && mask && p->csne.count > 0 && (rc = p->csne.relist(ctx))) return rc;   // (refreshed problems have left the tier)
  return trf_finish(p);
}

}  // namespace blsq_host

// The verdict of an optimistic factor call.  *redo = false: nothing was pending, or the guess held.
// *redo = true: it did not — the state is now what the synchronous path would have left (fallback
// stage, rank gate, SVD), and whatever was computed from the guessed state must be computed again.
int blsq_trf_plan::resolve(bool* redo) {
  blsq_trf_plan* p = this;
  return verdict_resolve(
      p, redo, [&]() { return trf_gate_tail(p, trf_chol_args(p, nullptr)); },
      [&](int nfb) {
        QrTree& t = p->tree;
        p->use_chol = t.any_gram;
        p->use_qr = t.any_qr;
        p->lm.colinfo = p->aug_colinfo.as<double>();
        int rc;
        if (nfb > 0 && (rc = trf_fallback_stage(p, p->pend_dJ, p->pend_df, p->pend_ldJ, p->pend_scale_mode, nfb)))
          return rc;
        return trf_finish(p);
      });
}

namespace blsq_host {
// Safeguarded Newton iteration of the SVD-free problems: lock-step rounds of
// (factor of the system at the current alpha) + (two triangular solves + update).
//
// The kernels of round r run over the compacted list of the problems still iterating and leave
// when their index is beyond the DEVICE counter of that round, so the host does not have to know
// the count to launch them — only an upper bound (the previous round's count).  When every problem
// is on the normal-equations path the host therefore runs one round AHEAD of what it knows: it
// enqueues round r, then waits for the counter of round r (written by round r - 1, i.e. while
// round r executes).  The GPU does not idle on a host round trip for the rounds that had work in the
// plan's last call; from the first round that was empty then, the counter is read before the round is
// enqueued (no round of empty launches at the end).  Problems on the Householder path (stacked QR per
// round: several launches sized by the count) keep the synchronous loop.
int trf_lm_rounds(blsq_trf_plan* p, const double* dDelta, const double* dalpha_in) {
  blsq_ctx* ctx = p->ctx;
  int* counts = p->lm.active_count;
  hipError_t e;
  p->lm.fused_gram = 0;
  auto lm_system = [&] {                                 // H = D G D + E^2 from the kept Gram, as every factor below takes it
    GramCholArgs c{};
    c.opt = &ctx->opt;
    c.Gsrc = p->tree.gram_keep.as<double>(); c.NPAD = p->ld; c.n = p->n;
    c.colscale = p->st.d; c.diag_vec = p->st.ediag; c.stride_vec = p->ld;
    return c;
  };
  if (p->use_chol && p->lm_enable && p->ld <= 80) {
    // N <= 80: the Gauss-Newton step, the bracket and ALL rounds of every normal-equations-path problem
    // in ONE launch (one wave per problem iterates to the end; chol_reg.hip).  Householder-path
    // problems of the same batch go through lm_start and the round loop below.
    // BLSQ_LM_FUSED = 0: lm_start + the round-by-round loop for everybody.
    if (ctx->opt.on(OPT_LM_FUSED)) {
      GramCholArgs c = lm_system();
      c.rinv = p->tree.gram_rinv.as<double>(); c.dsc = p->tree.gram_dsc.as<double>();
      if (int rc_ = ctx->run(K_LM_CHOL, "launch_lm_rounds_reg", [&] {
            return launch_lm_rounds_reg(c, p->lm, dDelta, dalpha_in, ctx->stream);
          })) return rc_;
      if (!p->use_qr) return 0;
      p->lm.fused_gram = 1;
    }
  }
  int* pin = ctx->pin(PIN_LM_ROUND0);                    // slot of round r (PIN_LM_ROUND0 + r): pin + 4 r
  int pin_seq[16] = {0};
  bool rides[16] = {false};
  int ride_rounds = 0;                                   // rounds [0, ride_rounds) are enqueued before their counter is read
  if (!p->lm_counts_clean) HIPCHK(ctx, hipMemsetAsync(counts, 0, 16 * sizeof(int), ctx->stream));
  p->lm_counts_clean = false;
  if (int rc_ = ctx->run(K_LM_SOLVE, "launch_lm_start", [&] {
        return launch_lm_start(p->lm, dDelta, dalpha_in, ctx->stream);
      })) return rc_;
  auto read_back = [&](int r) -> hipError_t {            // counter of round r -> pin[r]
    // (a round that is enqueued ahead of its counter takes the counter along: lm_update_kernel of that round stores it)
    if (ride_rounds > r) { rides[r] = true; return hipSuccess; }
    return ctx->publish(counts + r, 1, pin + 4 * r, &pin_seq[r]);
  };
  auto landed = [&](int r) -> hipError_t { return ctx->await(pin + 4 * r, pin_seq[r]); };
  auto chol_round = [&](int round, int grid, const int* count_dev) -> hipError_t {
    // R_alpha = chol(D G D + E^2 + alpha I) straight from the Gram, active Gram-path problems
    GramCholArgs c = lm_system();
    c.G = p->lm.Xa; c.diag_sqrt = p->lm.sa;
    c.batch_list = p->lm.active_list + (size_t)(round & 1) * p->B;
    c.skip_path = p->path;
    c.qr_mask = p->lm.hmax ? p->lm.ncols_lm : nullptr;
    c.count_dev = count_dev;
    c.skip_zero = 1;                                    // (lm_Xa: zeroed at allocation, read by lm_update's solves only)
    return ctx->timed(K_LM_CHOL, [&] { return launch_gram_chol(c, grid, ctx->stream); });
  };
  // the stacked QR of [R_aug; sqrt(alpha) I] for the problems of the round whose mask says so (LmState::ncols_lm)
  auto qr_round = [&](int round, int grid, const int* count_dev) -> hipError_t {
    // source = [R_aug | c_aug] read in place, stacked on a VIRTUAL sqrt(alpha) I block
    QrArgs q = p->tree.base_args();
    q.A = p->lm.Raug; q.strideA = (long)p->ld * p->ld; q.ldA = p->ld;
    q.rowsA = aug_block_rows(p->n) + p->n;
    q.vdiag_row0 = aug_block_rows(p->n); q.vdiag = p->lm.sa;
    q.F = nullptr; q.strideF = 0; q.ncols_dev = p->lm.ncols_lm;
    q.batch_list = p->lm.active_list + (size_t)(round & 1) * p->B;   // only the active problems
    q.count_dev = count_dev;
    q.rows_per_leaf = p->aug_RP; q.RP = p->aug_RP; q.LDP = p->aug_LDP;
    q.Rout = p->lm.Xa;
    q.stack_rows = aug_block_rows(p->n);
    return ctx->timed(K_LM_QR, [&] { return launch_qr(q, 1, grid, ctx->stream); });
  };
  const bool chol_any = p->gram_valid && p->lm_enable && (p->use_chol || p->lm.hmax != nullptr) &&
                        !(p->lm.fused_gram && !p->lm.hmax);
  if (chol_any) ride_rounds = p->lm_rounds_last < 12 ? p->lm_rounds_last : 12;
  HIPCHK(ctx, read_back(0));
  // Run-ahead loop: whenever the Grams of the current problems are at hand.  Householder-path problems join
  // the Cholesky launch where their alpha allows it (LmState::hmax); the stacked QR of the round is enqueued
  // only while the batch holds such problems at all, over the same upper bound, and leaves at once for a
  // problem whose mask is 0.  Their triangles dirty the lm_Xa slots outside the factor: the solves never look.
  if (chol_any) {
    int bound = p->B;                                   // upper bound of the count of the round being enqueued
    // Rounds that had work in the LAST call of this plan are enqueued ahead of their counter, as described
    // above; from the first round that was empty last time on, the host looks at the counter first — the
    // GPU idles for one host round trip (~10 us) instead of running a round of three empty launches.
    const int ahead_rounds = p->lm_rounds_last;
    int done_rounds = 0;
    for (int round = 0; round < 12; ++round) {
      const bool ahead = round < ahead_rounds;
      if (!ahead) {
        HIPCHK(ctx, landed(round));
        const int active = pin[4 * round];
        if (active == 0) break;
        bound = active;
      }
      e = chol_round(round, bound, counts + round);
      if (e != hipSuccess) return ctx->fail(e, "launch_gram_chol(lm)");
      if (p->use_qr) {
        e = qr_round(round, bound, counts + round);
        if (e != hipSuccess) return ctx->fail(e, "launch_qr(lm)");
      }
      p->lm.round = round;
      if (rides[round]) {
        pin_seq[round] = ++ctx->pub_seq;
        p->lm.pub = PublishArgs{counts + round, 1, pin + 4 * round, pin_seq[round]};
      }
      e = ctx->timed(K_LM_SOLVE, [&] { return launch_lm_update(p->lm, bound, ctx->stream); });
      p->lm.pub = PublishArgs{nullptr, 0, nullptr, 0};
      if (e != hipSuccess) return ctx->fail(e, "launch_lm_update");
      HIPCHK(ctx, read_back(round + 1));
      if (ahead) {
        HIPCHK(ctx, landed(round));
        const int active = pin[4 * round];                  // what round `round` really worked on
        if (active == 0) break;                         // (the round just enqueued is empty)
        bound = active;
      }
      done_rounds = round + 1;
    }
    p->lm_rounds_last = done_rounds;
    return 0;
  }
  HIPCHK(ctx, landed(0));
  int active = pin[0];
  for (int round = 0; round < 12 && active > 0; ++round) {
    if (p->use_chol && !p->lm.fused_gram) {
      e = chol_round(round, active, nullptr);
      if (e != hipSuccess) return ctx->fail(e, "launch_gram_chol(lm)");
    }
    if (p->use_qr) {
      e = qr_round(round, active, nullptr);
      if (e != hipSuccess) return ctx->fail(e, "launch_qr(lm)");
    }
    p->lm.round = round;
    if (int rc_ = ctx->run(K_LM_SOLVE, "launch_lm_update", [&] {
          return launch_lm_update(p->lm, active, ctx->stream);
        })) return rc_;
    HIPCHK(ctx, read_back(round + 1));
    HIPCHK(ctx, landed(round + 1));
    active = pin[4 * (round + 1)];
  }
  return 0;
}

// CSNE tier, step side (csne_kernels.hip): ONE streaming pass over the caller's J for every recorded evaluation of
// every problem on the tier, then the n-space correction (replayed Newton iteration, corrected final step, H p for
// the step kernel).  Problems whose acceptance fails are listed in cs.fail_list (trf_csne_verdict).
int trf_csne_correct(blsq_trf_plan* p, const double* dDelta, const double* dalpha_in) {
  blsq_ctx* ctx = p->ctx;
  CsneTier& tier = p->csne;
  CsneState& cs = tier.cs;
  if (int rc_ = tier.pass_begin(ctx)) return rc_;
  if (int rc_ = ctx->run(K_CSNE_PASS, "launch_csne_pass_trf", [&] {
        return launch_csne_pass_trf(cs, p->st.d, tier.count, ctx->stream);
      })) return rc_;
  if (int rc_ = ctx->run(K_CSNE_FIX, "launch_csne_fix", [&] {
        return launch_csne_fix(cs, p->st, p->lm, dDelta, dalpha_in, tier.count, ctx->stream);
      })) return rc_;
  return 0;
}

// ... and what became of them: problems the tier declined in this step call leave it — factored by CholeskyQR2 / the
// Householder tree from the caller's J (still valid: the lifetime rule of the tier), prepared again from the triangle —
// and the step runs once more (*redo).
int trf_csne_verdict(blsq_trf_plan* p, bool* redo) {
  blsq_ctx* ctx = p->ctx;
  const CsneState& cs = p->csne.cs;
  QrTree& t = p->tree;
  int rc, nfail = 0;
  if ((rc = p->csne.pass_verdict(ctx, /*polled=*/true, &nfail))) return rc;
  if (nfail == 0) return 0;
  *redo = true;
  if ((rc = p->csne.reroute(ctx, t, nfail))) return rc;
  if ((rc = t.run_fallback(ctx, cs.J, cs.F, cs.ldJ, nfail))) return rc;
  if (int rc_ = ctx->run(K_PREP, "launch_trf_prep(csne redo)", [&] {
        return launch_trf_prep(p->st, p->last_scale_mode, 0, t.fb_mask(), 1, ctx->stream);
      })) return rc_;
  p->use_qr = true;
  p->gate_done = false; p->njac = -1;
  return trf_finish(p);
}

}  // namespace blsq_host

extern "C" int blsq_trf_plan_create(blsq_ctx* ctx, int B, int m, int n, blsq_trf_plan** out) {
  if (!ctx) return -1;
  if (out) *out = nullptr;
  if (int rc_ = step_plan_args(ctx, B, m, n, out)) return rc_;
  blsq_trf_plan* p = new blsq_trf_plan();
  p->m_total = m; p->nranks = 1;
  const int aug_rp = std::max(aug_rows(n), round_up(n + 1, 16));
  if (int rc_ = step_plan_init(ctx, p, B, m, n, (size_t)B * aug_rp, true, [p] { return trf_alloc_state(p); })) return rc_;
  *out = p;
  return 0;
}

extern "C" int blsq_trf_plan_destroy(blsq_trf_plan* p) { return step_plan_destroy(p); }

extern "C" int blsq_trf_factor_dev(blsq_trf_plan* p, const double* dJ, const double* df,
                                   const double* dx, const double* dlb, const double* dub,
                                   double* dscale_io, int scale_mode) {
  if (!p) return -1;
  if (int rc_ = factor_args(p->ctx, dJ, df, dx, dlb, dub, dscale_io, scale_mode)) return rc_;
  return factor_dev(p, dx, dlb, dub, dscale_io, scale_mode, nullptr,
                    [&] { return trf_factor_core(p, dJ, df, p->n, scale_mode, nullptr, true); });
}

extern "C" int blsq_trf_step_dev(blsq_trf_plan* p, const double* dDelta, const double* dalpha_in,
                                 double active_rtol) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dDelta) return ctx->bad(2, "Delta is NULL");
  if (!dalpha_in) return ctx->bad(3, "alpha is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // (pass 0 may run on the guessed state of an optimistic factor call; pass 1 only if the guess was wrong)
  // (... and one more if a problem leaves the CSNE tier in this call: it is factored by the next tier, then the step again)
  for (int pass = 0; pass < 4; ++pass) {
    int rc = trf_lm_rounds(p, dDelta, dalpha_in);
    if (rc) return rc;
    const int ncs = p->csne.count;
    if (ncs > 0 && (rc = trf_csne_correct(p, dDelta, dalpha_in))) return rc;
    const PublishArgs pub = verdict_rides(p);
    if ((rc = ctx->run(K_STEP, "launch_trf_step", [&] {
           return launch_trf_step(p->st, &p->lm, dDelta, dalpha_in, active_rtol, p->out, ctx->stream, &pub);
         }))) return rc;
    p->lm_counts_clean = true;              // (the step kernel leaves the round counters zeroed)
    bool redo = false;
    if ((rc = p->resolve(&redo))) return rc;
    // (no repair ran: the tier still holds the ncs problems of the pass)
    if (!redo && ncs > 0 && (rc = trf_csne_verdict(p, &redo))) return rc;
    if (!redo) break;
  }
  return 0;
}

extern "C" int blsq_trf_fetch_factor(blsq_trf_plan* p, double* g, double* g_norm, double* theta,
                                     double* scale, double* sing) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  int rc;
  if ((rc = p->resolve(nullptr))) return rc;
  if ((rc = get_vec(ctx, g, p->n, p->st.g, p->ld, p->B))) return rc;
  if ((rc = get_vec(ctx, scale, p->n, p->st.scale, p->ld, p->B))) return rc;
  if ((rc = get_vec(ctx, sing, p->n, p->st.s, p->ld, p->B))) return rc;
  if (g_norm) HIPCHK(ctx, hipMemcpyAsync(g_norm, p->st.g_norm, sizeof(double) * p->B,
                                         hipMemcpyDeviceToHost, ctx->stream));
  if (theta) HIPCHK(ctx, hipMemcpyAsync(theta, p->st.theta, sizeof(double) * p->B,
                                        hipMemcpyDeviceToHost, ctx->stream));
  return blsq_sync(ctx);
}

extern "C" int blsq_trf_debug_fast(blsq_trf_plan* p, int32_t* fast) {
  if (!p) return -1;
  if (!fast) return p->ctx->bad(2, "fast is NULL");
  return fetch_resolved(p, fast, p->lm.fast, sizeof(int));
}

extern "C" int blsq_trf_debug_cond(blsq_trf_plan* p, double* k2) { return debug_cond(p, k2); }

extern "C" int blsq_trf_debug_csne(blsq_trf_plan* p, int32_t* on_tier, double* eta) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  { int rc_ = p->resolve(nullptr); if (rc_) return rc_; }
  if (!p->csne.on) {
    for (int b = 0; b < p->B; ++b) { if (on_tier) on_tier[b] = 0; if (eta) eta[b] = 0.0; }
    return 0;
  }
  if (on_tier) HIPCHK(ctx, hipMemcpyAsync(on_tier, p->csne.cs.flag, sizeof(int) * p->B, hipMemcpyDeviceToHost, ctx->stream));
  if (eta) HIPCHK(ctx, hipMemcpyAsync(eta, p->csne.cs.eta, sizeof(double) * p->B, hipMemcpyDeviceToHost, ctx->stream));
  return blsq_sync(ctx);
}

extern "C" int blsq_trf_debug_sweeps(blsq_trf_plan* p, int32_t* sweeps) {
  if (!p) return -1;
  if (!sweeps) return p->ctx->bad(2, "sweeps is NULL");
  return fetch_resolved(p, sweeps, p->sweeps.p, sizeof(int));
}

extern "C" int blsq_trf_fetch_step(blsq_trf_plan* p, double* alpha_out, double* step_h,
                                   double* step, double* x_new, int64_t* hits,
                                   int64_t* active_new, double* predicted_reduction,
                                   double* step_h_norm, double* correction, int32_t* n_iter,
                                   int32_t* branch, int32_t* status, double* p_h_tr,
                                   double* to_bound, int32_t* choice) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, n = p->n, ld = p->ld;
  int rc;
  if ((rc = get_vec(ctx, step_h, n, p->out.step_h, ld, B))) return rc;
  if ((rc = get_vec(ctx, step, n, p->out.step, ld, B))) return rc;
  if ((rc = get_vec(ctx, x_new, n, p->out.x_new, ld, B))) return rc;
  if ((rc = get_vec(ctx, p_h_tr, n, p->out.p_h_tr, ld, B))) return rc;
  if ((rc = get_vec(ctx, (long long*)hits, n, p->out.hits, ld, B))) return rc;
  if ((rc = get_vec(ctx, (long long*)active_new, n, p->out.active_new, ld, B))) return rc;
  std::vector<double> sc;                   // [B][8]
  std::vector<int> inf;                     // [B][4]
  if ((rc = fetch_scal_info(p, &sc, &inf))) return rc;
  for (int b = 0; b < B; ++b) {
    if (predicted_reduction) predicted_reduction[b] = sc[8 * b + 0];
    if (step_h_norm) step_h_norm[b] = sc[8 * b + 1];
    if (correction) correction[b] = sc[8 * b + 2];
    if (alpha_out) alpha_out[b] = sc[8 * b + 3];
    if (to_bound) to_bound[b] = sc[8 * b + 4];
    if (n_iter) n_iter[b] = inf[4 * b + 0];
    if (branch) branch[b] = inf[4 * b + 1];
    if (choice) choice[b] = inf[4 * b + 2];
    if (status) status[b] = inf[4 * b + 3];
  }
  return 0;
}

extern "C" int blsq_trf_factor(blsq_trf_plan* p, const double* J, const double* f,
                               const double* x, const double* lb, const double* ub,
                               double* scale_io, int scale_mode, double* g, double* g_norm,
                               double* theta) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (int rc_ = factor_args(ctx, J, f, x, lb, ub, scale_io, scale_mode)) return rc_;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage_alloc(p);
  if (rc) return rc;
  if ((rc = put_state(p, x, lb, ub, scale_io, nullptr, hipMemcpyHostToDevice))) return rc;
  // [J f] crosses PCIe in sub-batches of problems on a copy stream; the Gram of sub-batch k runs while sub-batch
  // k + 1 is in flight — for caller buffers in page-locked memory (blsq_host_alloc), which are DMA'd straight.
  // BLSQ_H2D_PIPE = 0 / 1: never / always (pageable memory too).
  bool piped = false;
  {
    const int pipe_o = ctx->opt.i(OPT_H2D_PIPE);          // -1: page-locked sources only, 0 never, 1 always
    const size_t per = sizeof(double) * (size_t)p->m * (p->n + 1);
    const int sub = (int)std::max<size_t>(1, std::min<size_t>((size_t)p->B, ((size_t)96 << 20) / std::max<size_t>(per, 1)));
    // (page-locked source only — BLSQ_H2D_PIPE = 1 forces it for pageable memory too: there the runtime's own
    //  pin-on-the-fly path for ONE large copy reached 52-53 GB/s, sub-batches of it as little as 27)
    bool pinned_src = false;
    {
      hipPointerAttribute_t at{};
      if (hipPointerGetAttributes(&at, J) == hipSuccess) pinned_src = (at.type == hipMemoryTypeHost);
      else (void)hipGetLastError();                       // (plain malloc memory: "invalid value", not an error here)
    }
    const bool want = pipe_o < 0 ? pinned_src : pipe_o == 1;
    if (p->tree.gram && p->B >= 2 * sub && want) {
      piped = true;
      const int nsub = (p->B + sub - 1) / sub;
      while ((int)ctx->copy_ev.size() < nsub) {
        hipEvent_t ev = nullptr;
        HIPCHK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->copy_ev.push_back(ev);
      }
      for (int k = 0, k0 = 0; k0 < p->B; ++k, k0 += sub) {
        const int nb = std::min(sub, p->B - k0);
        const size_t jo = (size_t)k0 * p->m * p->n, fo = (size_t)k0 * p->m;
        HIPCHK(ctx, hipMemcpyAsync(p->in_J.as<double>() + jo, J + jo, sizeof(double) * (size_t)nb * p->m * p->n,
                                   hipMemcpyHostToDevice, ctx->copy_stream));
        HIPCHK(ctx, hipMemcpyAsync(p->in_f.as<double>() + fo, f + fo, sizeof(double) * (size_t)nb * p->m,
                                   hipMemcpyHostToDevice, ctx->copy_stream));
        HIPCHK(ctx, hipEventRecord(ctx->copy_ev[k], ctx->copy_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->copy_ev[k], 0));
        if ((rc = p->tree.run_gram_only(ctx, p->in_J.as<double>(), p->in_f.as<double>(), p->n, nullptr, false, k0, nb)))
          return rc;
      }
    }
  }
  if (!piped && (rc = stage_upload(p, J, f))) return rc;
  if ((rc = trf_factor_core(p, p->in_J.as<double>(), p->in_f.as<double>(), p->n, scale_mode, nullptr, false, piped)))
    return rc;
  return blsq_trf_fetch_factor(p, g, g_norm, theta,
                               scale_mode != BLSQ_SCALE_GIVEN ? scale_io : nullptr, nullptr);
}

extern "C" int blsq_trf_step(blsq_trf_plan* p, const double* Delta, double* alpha_io,
                             double active_rtol, double* step_h, double* step, double* x_new,
                             int64_t* hits, int64_t* active_new, double* predicted_reduction,
                             double* step_h_norm, double* correction, int32_t* n_iter,
                             int32_t* branch, int32_t* status) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!Delta) return ctx->bad(2, "Delta is NULL");
  if (!alpha_io) return ctx->bad(3, "alpha is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  double* dD = p->in_scal.as<double>();
  double* dA = dD + p->B;
  HIPCHK(ctx, hipMemcpyAsync(dD, Delta, sizeof(double) * p->B, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(dA, alpha_io, sizeof(double) * p->B, hipMemcpyHostToDevice, ctx->stream));
  int rc = blsq_trf_step_dev(p, dD, dA, active_rtol);
  if (rc) return rc;
  return blsq_trf_fetch_step(p, alpha_io, step_h, step, x_new, hits, active_new,
                             predicted_reduction, step_h_norm, correction, n_iter, branch,
                             status, nullptr, nullptr, nullptr);
}

// ================================================================= TSQR ====
extern "C" int blsq_tsqr_tri_ld(int n) { return round_up(n + 1, 16); }

extern "C" int blsq_tsqr_plan_create(blsq_ctx* ctx, int m_local, long long m_total, int n,
                                     int nranks, blsq_trf_plan** out) {
  if (!ctx) return -1;
  if (!out) return ctx->bad(6, "out is NULL");
  *out = nullptr;
  if (m_local <= 0) return ctx->bad(2, "m_local must be positive");
  if (m_total < m_local) return ctx->bad(3, "m_total must be >= m_local");
  if (n <= 0) return ctx->bad(4, "n must be positive");
  if (nranks <= 0) return ctx->bad(5, "nranks must be positive");
  if (nranks > 1 && !merge_fits(n)) return ctx->bad(4, "TSQR needs n <= 512");
  blsq_trf_plan* p = new blsq_trf_plan();
  p->nranks = nranks;
  // the GLOBAL row count enters the reference's rank test eps * m * s[0] (trust_region.py:109):
  // it must be the same number on every rank, whatever the sizes of the row blocks
  p->m_total = m_total > 2147483647LL ? 2147483647 : (int)m_total;
  const int NPAD = round_up(n + 1, 16);
  const int aug_rp = std::max(aug_rows(n), NPAD);
  // scratch must also cover the combine merges: nranks triangles, G per workgroup
  const int G = merge_group(n);
  const size_t comb_rows = (size_t)((nranks + G - 1) / G) * (size_t)(G * NPAD);
  // (no optimistic verdicts: blsq_tsqr_factor_dev reads its gate synchronously)
  if (int rc_ = step_plan_init(ctx, p, 1, m_local, n, std::max((size_t)aug_rp, comb_rows), false, [&] {
        if (p->tree.gram) p->tree.k2_max = gram_k2_max(m_total, ctx->opt.d(OPT_GRAM_K2_MAX));   // (the Gram sums over ALL ranks' rows)
        if (int rc = trf_alloc_state(p)) return rc;
        // Rcomb: two ping-pong levels for the combine tree
        return alloc_all(ctx, {{&p->Rcomb, sizeof(double) * 2 * (size_t)((nranks + G - 1) / G + 1) * NPAD * NPAD, "hipMalloc(Rcomb)"},
                               {&p->Rstack, sizeof(double) * (size_t)nranks * NPAD * NPAD, "hipMalloc(Rstack)"}});
      })) return rc_;
  *out = p;
  return 0;
}

extern "C" int blsq_tsqr_local_dev(blsq_trf_plan* p, const double* dJ_block,
                                   const double* df_block, double* dtri_out) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dJ_block) return ctx->bad(2, "J block is NULL");
  if (!df_block) return ctx->bad(3, "f block is NULL");
  if (!dtri_out) return ctx->bad(4, "tri_out is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = p->tree.run(ctx, dJ_block, df_block, p->n);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(dtri_out, p->tree.Rfinal(), sizeof(double) * p->ld * p->ld,
                             hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

namespace blsq_host {
// merge the stack of nranks triangles (rank order) and run the n-space path on the result
int tsqr_merge_and_finish(blsq_trf_plan* p, const double* dtri_stack, int scale_mode,
                          double* dscale_io, int redo = 0) {
  blsq_ctx* ctx = p->ctx;
  const int NPAD = p->ld;
  const double* src = dtri_stack;
  int ntri = p->nranks;
  const int G = merge_group(p->n);
  double* pp[2] = {p->Rcomb.as<double>(),
                   p->Rcomb.as<double>() + (size_t)((p->nranks + G - 1) / G + 1) * NPAD * NPAD};
  int flip = 0;
  while (ntri > 1) {
    QrArgs q = p->tree.base_args();
    q.A = src; q.strideA = 0; q.ldA = NPAD; q.rowsA = ntri * NPAD; q.F = nullptr; q.strideF = 0;
    q.stack_rows = NPAD;
    q.rows_per_leaf = G * NPAD;
    const int nleaf = (ntri + G - 1) / G;
    q.RP = std::max(round_up(std::min(q.rows_per_leaf, q.rowsA), 16), NPAD);
    q.Rout = pp[flip];
    if (int rc_ = ctx->run(K_QR_MERGE, "launch_qr(combine)", [&] {
          return launch_qr(q, nleaf, 1, ctx->stream);
        })) return rc_;
    src = pp[flip];
    flip ^= 1;
    ntri = nleaf;
  }
  int rc = trf_after_triangle(p, src, scale_mode, redo);
  if (rc) return rc;
  if (scale_mode != BLSQ_SCALE_GIVEN) {
    HIPCHK(ctx, hipMemcpyAsync(dscale_io, p->st.scale, sizeof(double) * p->n,
                               hipMemcpyDeviceToDevice, ctx->stream));
  }
  return 0;
}
}  // namespace blsq_host

extern "C" int blsq_tsqr_combine_dev(blsq_trf_plan* p, const double* dtri_stack,
                                     const double* dx, const double* dlb, const double* dub,
                                     double* dscale_io, int scale_mode) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dtri_stack) return ctx->bad(2, "tri stack is NULL");
  if (!dx || !dlb || !dub) return ctx->bad(3, "x/lb/ub is NULL");
  if (!dscale_io) return ctx->bad(6, "scale is NULL");
  if (scale_mode < 0 || scale_mode > 2) return ctx->bad(7, "scale_mode");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = put_state(p, dx, dlb, dub, dscale_io, nullptr, hipMemcpyDeviceToDevice);
  if (rc) return rc;
  return tsqr_merge_and_finish(p, dtri_stack, scale_mode, dscale_io);
}

// The whole factor call of one tall problem whose rows are split over the ranks of the ctx's
// communicator (blsq_comm_init), this rank's row block in, replicated factor state out:
//   normal-equations front end:  local Gram -> ncclAllReduce(sum) of the (n+1)^2 Gram -> Cholesky + gate
//                                (replicated, bit-identical on every rank)
//   if the gate rejects:         local Householder TSQR -> ncclAllGather of the triangles -> merge
// then the ordinary n-space path.  Everything is enqueued on the ctx stream; the only host wait is
// the read-back of the gate's verdict (one integer).
extern "C" int blsq_tsqr_factor_dev(blsq_trf_plan* p, const double* dJ_block, const double* df_block,
                                    const double* dx, const double* dlb, const double* dub,
                                    double* dscale_io, int scale_mode) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dJ_block) return ctx->bad(2, "J block is NULL");
  if (!df_block) return ctx->bad(3, "f block is NULL");
  if (!dx || !dlb || !dub) return ctx->bad(4, "x/lb/ub is NULL");
  if (!dscale_io) return ctx->bad(7, "scale is NULL");
  if (scale_mode < 0 || scale_mode > 2) return ctx->bad(8, "scale_mode");
  if (p->nranks > 1 && (!ctx->comm || ctx->comm_ranks != p->nranks))
    return ctx->bad(1, "the plan's ranks need a communicator of that size on this ctx (blsq_comm_init)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // (zero_counts: with the normal-equations front end the prep launch of the Gram stage packs the vectors and clears the
  //  gate counters — no pack launch, no fill)
  int rc = put_state(p, dx, dlb, dub, dscale_io, nullptr, hipMemcpyDeviceToDevice, true);
  if (rc) return rc;
  auto put_scale = [&]() -> int {
    if (scale_mode != BLSQ_SCALE_GIVEN)
      HIPCHK(ctx, hipMemcpyAsync(dscale_io, p->st.scale, sizeof(double) * p->n,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  };
  // max AND min over the ranks of a few integers (the ranks' copies must be equal): nv <= 4 values
  auto agree = [&](const int* vals, int nv, const char* what) -> int {
    double* d = p->Rstack.as<double>();                   // (free until the all-gather)
    double h[8];
    for (int i = 0; i < nv; ++i) { h[2 * i] = (double)vals[i]; h[2 * i + 1] = -(double)vals[i]; }
    HIPCHK(ctx, hipMemcpyAsync(d, h, sizeof(double) * 2 * nv, hipMemcpyHostToDevice, ctx->stream));
    RCCLCHK(ctx, g_rccl.AllReduce(d, d, (size_t)(2 * nv), ncclDouble, ncclMax, ctx->comm, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h, d, sizeof(double) * 2 * nv, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nv; ++i)
      if (h[2 * i] != -h[2 * i + 1]) {
        ctx->err = std::string("blsq_tsqr_factor_dev: the ranks disagree on ") + what +
                   " (x, bounds, scale, scale_mode, the plan's n / m_total and the BLSQ_* environment must be "
                   "identical on every rank)";
        return BLSQ_ERR_RANKS_DISAGREE;
      }
    return 0;
  };
  if (p->nranks > 1 && !p->ranks_agreed) {
    // once per plan, BEFORE the first data collective: a rank whose front end is switched off would enter
    // the all-gather while the others sit in the Gram's all-reduce
    const int cfg[3] = {p->tree.gram ? 1 : 0, p->n, p->m_total};
    if ((rc = agree(cfg, 3, "the plan (normal-equations front end on / off, n, m_total)"))) return rc;
    p->ranks_agreed = true;
  }
  int redo = 0;
  if (p->tree.gram) {
    if ((rc = p->tree.run_gram_only(ctx, dJ_block, df_block, p->n, nullptr, /*collective=*/true))) return rc;
    int nfb = 0;
    if ((rc = trf_gram_stage(p, scale_mode, nullptr, &nfb))) return rc;   // replicated: same verdict everywhere
    if (p->nranks > 1) {
      // ... which is checked, not assumed: the route (return here, or enter the all-gather below) is taken
      // from the max AND the min of the verdict over the ranks.  Ranks that disagree (inputs or environment
      // that differ between them) all fail with the same code instead of one of them waiting in a
      // collective the others never enter.
      const int vd[2] = {nfb, scale_mode};
      if ((rc = agree(vd, 2, "the gate's verdict"))) return rc;
    }
    if (nfb == 0) {
      if ((rc = trf_finish(p))) return rc;
      return put_scale();
    }
    redo = 1;                                             // (prepared from the Gram once already)
  }
  // Householder route: this rank's triangle, all-gather, replicated merge
  if ((rc = p->tree.run_levels(ctx, dJ_block, df_block, p->n, nullptr))) return rc;
  if (p->nranks == 1) {
    if ((rc = trf_after_triangle(p, p->tree.Rfinal(), scale_mode, redo))) return rc;
    return put_scale();
  }
  const size_t tri = (size_t)p->ld * p->ld;
  RCCLCHK(ctx, g_rccl.AllGather(p->tree.Rfinal(), p->Rstack.as<double>(), tri, ncclDouble, ctx->comm,
                                ctx->stream));
  return tsqr_merge_and_finish(p, p->Rstack.as<double>(), scale_mode, dscale_io, redo);
}
