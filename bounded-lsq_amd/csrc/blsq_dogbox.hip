// C-ABI entry points (include/blsq.h): the dogbox plans — factor / step / fetch.
#include "blsq_host.h"

// =============================================================== dogbox ====
namespace blsq_host {

int dog_alloc_state(blsq_dogbox_plan* p) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, ld = p->ld;
  const size_t mat = (size_t)ld * ld;
  const size_t vs = (size_t)B * ld;
  if (int rc_ = alloc_all(ctx, {
          {&p->S, sizeof(double) * B * mat, "hipMalloc(p->S)"},
          {&p->X, sizeof(double) * B * mat, "hipMalloc(p->X)"},
          {&p->vecs, sizeof(double) * vs * 10, "hipMalloc(p->vecs)"},
          {&p->ivecs, sizeof(int) * (vs + B), "hipMalloc(p->ivecs)"},
          {&p->scal2, sizeof(double) * (size_t)B * 4, "hipMalloc(p->scal2)"},
          {&p->sweeps, sizeof(int) * (size_t)B, "hipMalloc(p->sweeps)"},
          {&p->active, vs, "hipMalloc(p->active)"},
          {&p->onb, sizeof(long long) * vs, "hipMalloc(p->onb)"},
          {&p->o_vec, sizeof(double) * vs * 2, "hipMalloc(p->o_vec)"},
          {&p->o_onb, sizeof(long long) * vs, "hipMalloc(p->o_onb)"},
          {&p->o_scal, sizeof(double) * (size_t)B * 4, "hipMalloc(p->o_scal)"},
          {&p->o_info, sizeof(int) * (size_t)B * 4, "hipMalloc(p->o_info)"},
          {&p->in_scal, sizeof(double) * (size_t)B, "hipMalloc(p->in_scal)"},
          {&p->gate_ints, sizeof(int) * 3 * (size_t)B, "hipMalloc(p->gate_ints)"},
          {&p->colinfo, sizeof(double) * 2 * (size_t)B, "hipMalloc(p->colinfo)"},
      })) return rc_;
  p->svdfree_enable = ctx->opt.i(OPT_NO_SVDFREE) == 1 ? 0 : 1;
  if (p->tree.gram && csne_supported(p->m, p->n) && ctx->opt.on(OPT_CSNE) && p->svdfree_enable) {
    int rc = p->csne.build(ctx, B, p->m, p->n, ld, /*with_hp=*/false);
    if (rc) return rc;
    p->st.csne = p->csne.cs.flag; p->st.csne_k2 = p->csne.k2.as<double>();
  }
  HIPCHK(ctx, hipMemsetAsync(p->gate_ints.p, 0, p->gate_ints.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->S.p, 0, p->S.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->X.p, 0, p->X.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(p->vecs.p, 0, p->vecs.bytes, ctx->stream));
  double* v = p->vecs.as<double>();
  DogState& st = p->st;
  st.B = B; st.m = p->m; st.n = p->n; st.ld = ld; st.opt = &ctx->opt;
  st.S = p->S.as<double>(); st.X = p->X.as<double>();
  st.x = v; st.lb = v + vs; st.ub = v + 2 * vs; st.scale = v + 3 * vs; st.g = v + 4 * vs;
  st.s = v + 5 * vs; st.uf = v + 6 * vs; st.newton = v + 7 * vs; st.cauchy = v + 8 * vs;
  st.scale_in = v + 9 * vs;
  st.on_bound = p->on_bound = p->onb.as<long long>();
  st.free_idx = p->ivecs.as<int>(); st.ncols = p->ivecs.as<int>() + vs;
  st.srange = p->scal2.as<double>(); st.g_norm = p->scal2.as<double>() + 2 * (size_t)B;
  st.active = p->active.as<unsigned char>();
  p->out.step = p->o_vec.as<double>(); p->out.x_new = p->o_vec.as<double>() + vs;
  p->out.on_bound_new = p->o_onb.as<long long>();
  p->out.scal = p->o_scal.as<double>(); p->out.info = p->o_info.as<int>();
  return 0;
}

// the free-column QR (Householder-path problems), rank gate + Newton step, SVD for the rest
int dog_finish(blsq_dogbox_plan* p, const int* path, bool any_qr, bool any_gram, const int* done = nullptr) {
  blsq_ctx* ctx = p->ctx;
  if (any_qr) {
    QrArgs q = p->tree.base_args();
    q.A = p->st.S; q.strideA = (long)p->ld * p->ld; q.ldA = p->ld; q.rowsA = p->n;
    q.F = nullptr; q.strideF = 0; q.ncols_dev = p->st.ncols;
    q.require_path = path;
    q.rows_per_leaf = p->ld; q.RP = p->ld;
    q.Rout = p->st.X;
    if (int rc_ = ctx->run(K_QR_AUG, "launch_qr(free block)", [&] {
          return launch_qr(q, 1, p->B, ctx->stream);
        })) return rc_;
  }
  int* gfast = p->gate_ints.as<int>();
  int* gmask = gfast + p->B;
  p->st.fast = gfast;
  if (!p->gate_done) {
    // (done: problems whose steps stand already — the CSNE tier's corrected ones when the finish runs a second time)
    if (int rc_ = ctx->run(K_LM_GATE, "launch_dog_gate_solve", [&] {
          return launch_dog_gate_solve(p->st, gfast, gmask, p->svdfree_enable, path,
                                       (path && any_gram) ? p->colinfo.as<double>() : nullptr, nullptr, done,
                                       ctx->stream);
        })) return rc_;
    p->njac = -1;
  }
  p->gate_done = false;
  if (p->njac != 0)
    if (int rc_ = run_jacobi(p, p->st.X, p->st.s, p->st.uf, p->st.srange, gmask)) return rc_;
  if (int rc_ = ctx->run(K_STEP, "launch_dog_solve", [&] {
        return launch_dog_solve(p->st, gfast, ctx->stream);
      })) return rc_;
  return 0;
}

// a triangle [R c] of [J f] for every problem (front end off)
int dog_after_triangle(blsq_dogbox_plan* p, int scale_mode) {
  blsq_ctx* ctx = p->ctx;
  p->st.Rt = p->tree.Rfinal(); p->st.Gk = nullptr; p->st.path = nullptr;
  p->tree.path_valid = false; p->tree.any_gram = false; p->tree.any_qr = true;
  p->gate_done = false;
  if (int rc_ = ctx->run(K_PREP, "launch_dog_prep", [&] {
        return launch_dog_prep(p->st, scale_mode, 0, nullptr, 0, ctx->stream);
      })) return rc_;
  return dog_finish(p, nullptr, true, false);
}

GramCholArgs dog_chol_args(blsq_dogbox_plan* p, const int* mask) {
  QrTree& t = p->tree;
  GramCholArgs c = t.gate_args(mask);
  c.G = p->st.X; c.ncols_dev = p->st.ncols; c.gather = p->st.free_idx;
  c.colinfo = p->colinfo.as<double>();
  if (p->csne.on) c.pmin_out = p->csne.pmin.as<double>();
  if (p->ld <= 80) {                        // (the register-resident kernel also finishes the gate / Newton / Cauchy work)
    int* gf_ = p->gate_ints.as<int>();
    c.dog.g = p->st.g; c.dog.newton = p->st.newton; c.dog.cauchy = p->st.cauchy;
    c.dog.fast = gf_; c.dog.ncols_jac = gf_ + p->B; c.dog.done = gf_ + 2 * (size_t)p->B;
    c.unsettled = t.fb_count() + 2;
    c.dog.m = p->m; c.dog.enable = p->svdfree_enable;
  }
  return c;
}

// the second half of the certificate + rank gate + Newton / Cauchy steps of the problems the Cholesky
// kernel has not settled itself (counters: fb_count()[0] problems that leave the path, [1] that need the SVD)
int dog_gate_tail(blsq_dogbox_plan* p, const GramCholArgs& c) {
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  if (int rc_ = t.run_cert(ctx, c)) return rc_;
  int* gfast = p->gate_ints.as<int>();
  p->st.fast = gfast;
  if (int rc_ = ctx->run(K_LM_GATE, "launch_dog_gate_solve", [&] {
        return launch_dog_gate_solve(p->st, gfast, gfast + p->B, p->svdfree_enable, t.path_rw(),
                                     p->colinfo.as<double>(), t.fb_count() + 1, c.dog.g ? c.dog.done : nullptr,
                                     ctx->stream);
      })) return rc_;
  return 0;
}

// CSNE tier, dogbox (csne_kernels.hip).  Of the nfb problems the certificate has just rejected
// (tree.fb_list()) those whose free-block factor qualifies keep it as a preconditioner; *ntree = the others.
int dog_csne_select(blsq_dogbox_plan* p, int nfb, int* ntree, bool masked) {
  CsneTier& tier = p->csne;
  QrTree& t = p->tree;
  *ntree = nfb;
  if (!tier.on) return 0;
  if (!tier.ensure_recordings()) { tier.on = false; p->st.csne = nullptr; return 0; }
  int* gfast = p->gate_ints.as<int>();
  // (the bound over the plan's factor arguments: the same gather)
  return tier.select(p->ctx, t, dog_chol_args(p, t.fb_mask()), nfb, ntree, masked, [&](const int* sel) {
    return launch_csne_select_dog(tier.cs, p->m, p->st.ncols, gfast, gfast + p->B, nfb, t.fb_list(), t.fb_mask(),
                                  t.fb_count(), t.path_rw(), sel, tier.k2.as<double>(), tier.pmin.as<double>(),
                                  p->colinfo.as<double>(), p->ctx->stream);
  });
}

// ... and the correction itself, at FACTOR time (the Newton step of dogbox.py:197 does not depend on Delta): the cheap
// steps of the problems on the tier scattered to full length, ONE pass over J, one corrected solve each.  Problems
// whose measured correction is too large leave the tier: *nfail of them, listed in tree.fb_list() / fb_mask().
int dog_csne_correct(blsq_dogbox_plan* p, const double* dJ, const double* df, int ldJ, int* nfail) {
  blsq_ctx* ctx = p->ctx;
  CsneTier& tier = p->csne;
  CsneState& cs = tier.cs;
  *nfail = 0;
  if (tier.count <= 0) return 0;
  cs.J = dJ; cs.strideJ = (long)p->m * ldJ; cs.ldJ = ldJ; cs.F = df; cs.strideF = p->m;
  if (int rc_ = tier.pass_begin(ctx)) return rc_;
  if (int rc_ = ctx->run(K_CSNE_PASS, "launch_csne_pass_dog", [&] {
        const hipError_t e = launch_dog_csne_scatter(cs, p->st, tier.count, ctx->stream);
        return e == hipSuccess ? launch_csne_pass_dog(cs, tier.count, ctx->stream) : e;
      })) return rc_;
  if (int rc_ = ctx->run(K_CSNE_FIX, "launch_dog_csne_fix", [&] {
        return launch_dog_csne_fix(cs, p->st, tier.count, ctx->stream);
      })) return rc_;
  if (int rc_ = tier.pass_verdict(ctx, /*polled=*/false, nfail)) return rc_;
  if (*nfail > 0) return tier.reroute(ctx, p->tree, *nfail);
  return 0;
}

// what follows the certificate's verdict "nfb problems leave the normal-equations path": the tier's selection, the
// next tiers' factorisation of the rest (CholeskyQR2 / tree) + their prep from the triangle, the plan's finish, the
// tier's correction — and once more for the problems the correction declined
int dog_repair(blsq_dogbox_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode, int nfb, bool masked) {
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  int rc;
  if (nfb > 0) {
    int ntree = nfb;
    if ((rc = dog_csne_select(p, nfb, &ntree, masked))) return rc;
    nfb = ntree;
  } else if (masked && p->csne.count > 0) {                // (refreshed problems have left the tier: the list from the flags)
    if ((rc = p->csne.relist(ctx))) return rc;
  }
  for (int pass = 0; pass < 2; ++pass) {
    if (nfb > 0) {
      if ((rc = t.run_fallback(ctx, dJ, df, ldJ, nfb))) return rc;
      if (int rc_ = ctx->run(K_PREP, "launch_dog_prep(redo)", [&] {
            return launch_dog_prep(p->st, scale_mode, 0, t.fb_mask(), 1, ctx->stream);
          })) return rc_;
    }
    if ((rc = dog_finish(p, t.path_rw(), t.any_qr, t.any_gram, pass > 0 && p->csne.on ? p->csne.cs.flag : nullptr))) return rc;
    int nfail = 0;
    if (pass == 0 && (rc = dog_csne_correct(p, dJ, df, ldJ, &nfail))) return rc;
    if (nfail == 0) break;
    nfb = nfail;                                           // (declined: the next tier, then the finish once more)
    p->gate_done = false; p->njac = -1;
  }
  return 0;
}

// The whole factor call from device-resident [J f].  Normal-equations path (as TRF): g and the
// column norms from the Gram, the triangle of [J[:, free] | f] as the Cholesky factor of the gathered
// principal sub-matrix G[free ++ rhs, free ++ rhs], and the conditioning gate applied to THAT factor
// — the system lstsq(J_free, -f) is solved from (dogbox.py:197).  No triangle of J is formed; a problem
// the gate rejects goes through the Householder tree and is prepared again from its triangle.
int dog_factor_core(blsq_dogbox_plan* p, const double* dJ, const double* df, int ldJ, int scale_mode,
                    const int* mask, bool may_defer) {
  blsq_ctx* ctx = p->ctx;
  QrTree& t = p->tree;
  int rc;
  if ((rc = verdict_drop(p))) return rc;
  if (!t.gram) {
    if ((rc = t.run_levels(ctx, dJ, df, ldJ, mask))) return rc;
    return dog_after_triangle(p, scale_mode);
  }
  if ((rc = t.run_gram_only(ctx, dJ, df, ldJ, mask, false))) return rc;
  p->st.Rt = t.Rfinal(); p->st.Gk = t.gram_keep.as<double>(); p->st.path = t.path_rw();
  const PackVecs* pk = nullptr;
  { int rc_ = take_pack(p, mask, &pk); if (rc_) return rc_; }
  if (int rc_ = ctx->run(K_PREP, "launch_dog_prep(gram)", [&] {
        return launch_dog_prep(p->st, scale_mode, 1, mask, 0, ctx->stream, pk);
      })) return rc_;
  const GramCholArgs c = dog_chol_args(p, mask);
  if (int rc_ = ctx->run(K_AUG_CHOL, "launch_gram_chol(free block)", [&] {
        return launch_gram_chol(c, p->B, ctx->stream);
      })) return rc_;
  const bool defer = may_defer && !mask && verdict_may_guess(p) && p->svdfree_enable && p->pend_pin;
  // second guess (N <= 80): the Cholesky kernel settles EVERY problem itself, as it did in the last call —
  // then the certificate, gate and solve launches would all be empty and are not enqueued at all
  const bool skip_tail = defer && p->guess_settled && c.dog.g != nullptr;
  p->st.fast = p->gate_ints.as<int>();
  if (!skip_tail && (rc = dog_gate_tail(p, c))) return rc;
  int nfb = 0;
  if (defer) {                              // guess: nobody leaves the path, nobody needs the SVD (resolve() checks)
    verdict_arm(p, skip_tail, dJ, df, ldJ, scale_mode);
  } else if ((rc = gate_verdict(p, /*polled=*/false, mask != nullptr, c.unsettled != nullptr, &nfb))) return rc;
  t.note_paths(ctx, nfb, mask != nullptr);
  if (!mask) p->csne.count = 0;                           // (the prep launch cleared every flag; dog_csne_select sets them anew)
  if (skip_tail) { p->gate_done = false; return 0; }
  return dog_repair(p, dJ, df, ldJ, scale_mode, nfb, mask != nullptr);
}

}  // namespace blsq_host

// the verdict of an optimistic dogbox factor call (as blsq_trf_plan::resolve)
int blsq_dogbox_plan::resolve(bool* redo) {
  blsq_dogbox_plan* p = this;
  return verdict_resolve(
      p, redo, [&]() { return dog_gate_tail(p, dog_chol_args(p, nullptr)); },
      [&](int nfb) { return dog_repair(p, p->pend_dJ, p->pend_df, p->pend_ldJ, p->pend_scale_mode, nfb, false); });
}

extern "C" int blsq_dogbox_plan_create(blsq_ctx* ctx, int B, int m, int n,
                                       blsq_dogbox_plan** out) {
  if (!ctx) return -1;
  if (out) *out = nullptr;
  if (int rc_ = step_plan_args(ctx, B, m, n, out)) return rc_;
  blsq_dogbox_plan* p = new blsq_dogbox_plan();
  if (int rc_ = step_plan_init(ctx, p, B, m, n, (size_t)B * round_up(n + 1, 16), true, [p] { return dog_alloc_state(p); }))
    return rc_;
  *out = p;
  return 0;
}

extern "C" int blsq_dogbox_plan_destroy(blsq_dogbox_plan* p) { return step_plan_destroy(p); }

extern "C" int blsq_dogbox_factor_dev(blsq_dogbox_plan* p, const double* dJ, const double* df,
                                      const double* dx, const double* dlb, const double* dub,
                                      double* dscale_io, int scale_mode,
                                      const int64_t* don_bound) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (int rc_ = factor_args(ctx, dJ, df, dx, dlb, dub, dscale_io, scale_mode)) return rc_;
  if (!don_bound) return ctx->bad(9, "on_bound is NULL");
  return factor_dev(p, dx, dlb, dub, dscale_io, scale_mode, don_bound,
                    [&] { return dog_factor_core(p, dJ, df, p->n, scale_mode, nullptr, true); });
}

extern "C" int blsq_dogbox_step_dev(blsq_dogbox_plan* p, const double* dDelta) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dDelta) return ctx->bad(2, "Delta is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int pass = 0; pass < 2; ++pass) {    // (pass 1 only after a wrong optimistic guess)
    const PublishArgs pub = verdict_rides(p);
    int rc = ctx->run(K_STEP, "launch_dog_step", [&] {
      return launch_dog_step(p->st, dDelta, p->out, ctx->stream, &pub);
    });
    if (rc) return rc;
    bool redo = false;
    if ((rc = p->resolve(&redo))) return rc;
    if (!redo) break;
  }
  return 0;
}

extern "C" int blsq_dogbox_fetch_factor(blsq_dogbox_plan* p, double* g, uint8_t* active_set,
                                        double* g_norm, int32_t* all_active, double* scale,
                                        double* newton_full, double* cauchy_full) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, n = p->n, ld = p->ld;
  int rc;
  if ((rc = p->resolve(nullptr))) return rc;
  if ((rc = get_vec(ctx, g, n, p->st.g, ld, B))) return rc;
  if ((rc = get_vec(ctx, scale, n, p->st.scale, ld, B))) return rc;
  if ((rc = get_vec(ctx, (unsigned char*)active_set, n, p->st.active, ld, B))) return rc;
  if (g_norm) HIPCHK(ctx, hipMemcpyAsync(g_norm, p->st.g_norm, sizeof(double) * B,
                                         hipMemcpyDeviceToHost, ctx->stream));
  std::vector<int> nc(B), fidx;
  HIPCHK(ctx, hipMemcpyAsync(nc.data(), p->st.ncols, sizeof(int) * B, hipMemcpyDeviceToHost,
                             ctx->stream));
  std::vector<double> nw, ca;
  if (newton_full || cauchy_full) {
    fidx.resize((size_t)B * ld); nw.resize((size_t)B * ld); ca.resize((size_t)B * ld);
    HIPCHK(ctx, hipMemcpyAsync(fidx.data(), p->st.free_idx, sizeof(int) * fidx.size(),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(nw.data(), p->st.newton, sizeof(double) * nw.size(),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ca.data(), p->st.cauchy, sizeof(double) * ca.size(),
                               hipMemcpyDeviceToHost, ctx->stream));
  }
  if ((rc = blsq_sync(ctx))) return rc;
  for (int b = 0; b < B; ++b) {
    if (all_active) all_active[b] = (nc[b] == 0) ? 1 : 0;
    if (newton_full || cauchy_full) {
      for (int j = 0; j < n; ++j) {
        if (newton_full) newton_full[(size_t)b * n + j] = 0.0;
        if (cauchy_full) cauchy_full[(size_t)b * n + j] = 0.0;
      }
      for (int q = 0; q + 1 < nc[b]; ++q) {
        const int j = fidx[(size_t)b * ld + q];
        if (newton_full) newton_full[(size_t)b * n + j] = nw[(size_t)b * ld + q];
        if (cauchy_full) cauchy_full[(size_t)b * n + j] = ca[(size_t)b * ld + q];
      }
    }
  }
  return 0;
}

extern "C" int blsq_dogbox_debug_cond(blsq_dogbox_plan* p, double* k2) { return debug_cond(p, k2); }

extern "C" int blsq_dogbox_debug_fast(blsq_dogbox_plan* p, int32_t* fast) {
  if (!p) return -1;
  if (!fast) return p->ctx->bad(2, "fast is NULL");
  return fetch_resolved(p, fast, p->gate_ints.p, sizeof(int));
}

extern "C" int blsq_dogbox_debug_sweeps(blsq_dogbox_plan* p, int32_t* sweeps) {
  if (!p) return -1;
  if (!sweeps) return p->ctx->bad(2, "sweeps is NULL");
  return fetch_resolved(p, sweeps, p->sweeps.p, sizeof(int));
}

extern "C" int blsq_dogbox_fetch_step(blsq_dogbox_plan* p, double* step, double* x_new,
                                      int64_t* on_bound_new, uint8_t* tr_hit,
                                      double* predicted_reduction, double* step_scaled_norm,
                                      uint8_t* fallback, int32_t* status) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, n = p->n, ld = p->ld;
  int rc;
  if ((rc = get_vec(ctx, step, n, p->out.step, ld, B))) return rc;
  if ((rc = get_vec(ctx, x_new, n, p->out.x_new, ld, B))) return rc;
  if ((rc = get_vec(ctx, (long long*)on_bound_new, n, p->out.on_bound_new, ld, B))) return rc;
  std::vector<double> sc;                   // [B][4]
  std::vector<int> inf;                     // [B][4]
  if ((rc = fetch_scal_info(p, &sc, &inf))) return rc;
  for (int b = 0; b < B; ++b) {
    if (predicted_reduction) predicted_reduction[b] = sc[4 * b + 0];
    if (step_scaled_norm) step_scaled_norm[b] = sc[4 * b + 1];
    if (tr_hit) tr_hit[b] = (uint8_t)inf[4 * b + 0];
    if (fallback) fallback[b] = (uint8_t)inf[4 * b + 1];
    if (status) status[b] = inf[4 * b + 3];
  }
  return 0;
}

extern "C" int blsq_dogbox_factor(blsq_dogbox_plan* p, const double* J, const double* f,
                                  const double* x, const double* lb, const double* ub,
                                  double* scale_io, int scale_mode, const int64_t* on_bound,
                                  double* g, uint8_t* active_set, double* g_norm,
                                  int32_t* all_active) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (int rc_ = factor_args(ctx, J, f, x, lb, ub, scale_io, scale_mode)) return rc_;
  if (!on_bound) return ctx->bad(9, "on_bound is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage_alloc(p);
  if (rc == 0) rc = stage_upload(p, J, f);
  if (rc == 0) rc = put_state(p, x, lb, ub, scale_io, on_bound, hipMemcpyHostToDevice);
  if (rc) return rc;
  if ((rc = dog_factor_core(p, p->in_J.as<double>(), p->in_f.as<double>(), p->n, scale_mode, nullptr)))
    return rc;
  return blsq_dogbox_fetch_factor(p, g, active_set, g_norm, all_active,
                                  scale_mode != BLSQ_SCALE_GIVEN ? scale_io : nullptr, nullptr,
                                  nullptr);
}

extern "C" int blsq_dogbox_step(blsq_dogbox_plan* p, const double* Delta, double* step,
                                double* x_new, int64_t* on_bound_new, uint8_t* tr_hit,
                                double* predicted_reduction, double* step_scaled_norm,
                                uint8_t* fallback, int32_t* status) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!Delta) return ctx->bad(2, "Delta is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  double* dD = p->in_scal.as<double>();
  HIPCHK(ctx, hipMemcpyAsync(dD, Delta, sizeof(double) * p->B, hipMemcpyHostToDevice, ctx->stream));
  int rc = blsq_dogbox_step_dev(p, dD);
  if (rc) return rc;
  return blsq_dogbox_fetch_step(p, step, x_new, on_bound_new, tr_hit, predicted_reduction,
                                step_scaled_norm, fallback, status);
}

