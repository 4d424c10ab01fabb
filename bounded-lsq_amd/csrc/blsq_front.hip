// The factorisation front end of a plan (QrTree: Gram / certificate / CholeskyQR2 / Householder tree), the CSNE
// tier's host state (CsneTier) and the plumbing of the entry points (StepPlan), shared by the TRF and the dogbox plans
// (blsq_host.h).
#include "blsq_host.h"

namespace blsq_host {

int QrTree::build(blsq_ctx* ctx, int B_, int rows, int n_, size_t extra_rp_rows) {
  B = B_; m = rows; n = n_; opt = &ctx->opt;
  N = n + 1; NPAD = round_up(N, 16); NP = NPAD / 16;
  if (NPAD > RMAX) return ctx->bad(4, "n too large (n + 1 must be <= 1024)");
  int cur_rows = rows;
  bool first = true;
  size_t max_slot_rows = extra_rp_rows;   // max over launches of nslot*RP
  size_t max_slots = (size_t)B;
  while (true) {
    Level L;
    L.rowsA = cur_rows;
    if (first) {
      L.nleaf = std::max(1, (cur_rows + RMAX - 1) / RMAX);
      if (L.nleaf > 1 && !merge_fits(n))
        return ctx->bad(4, "m > 1024 needs n <= 512 (TSQR merge capacity)");
      L.rows_per_leaf = round_up((cur_rows + L.nleaf - 1) / L.nleaf, 16);
      if (L.rows_per_leaf < NPAD && L.nleaf > 1) L.rows_per_leaf = NPAD;
      L.nleaf = std::max(1, (cur_rows + L.rows_per_leaf - 1) / L.rows_per_leaf);
    } else {
      const int G = merge_group(n);   // triangles merged per workgroup (>= 2)
      L.rows_per_leaf = G * NPAD;
      L.nleaf = (cur_rows + L.rows_per_leaf - 1) / L.rows_per_leaf;
    }
    L.RP = std::max(round_up(std::min(L.rows_per_leaf, std::max(cur_rows, 1)), 16), NPAD);
    if (qr_staged_tiles(L.RP, first ? 0 : NPAD, N) > QR_MAX_TILES)
      return ctx->bad(3, "leaf does not fit LDS");
    L.LDP = 0;
    if (int rc_ = alloc_all(ctx, {{&L.R, sizeof(double) * (size_t)B * L.nleaf * NPAD * NPAD, "hipMalloc(R level)"}}))
      return rc_;
    max_slot_rows = std::max(max_slot_rows, (size_t)B * L.nleaf * L.RP);
    max_slots = std::max(max_slots, (size_t)B * L.nleaf);
    levels.push_back(std::move(L));
    if (levels.back().nleaf == 1) break;
    cur_rows = levels.back().nleaf * NPAD;
    first = false;
  }
  if (int rc_ = alloc_all(ctx, {{&V, sizeof(double) * max_slot_rows * NP * 16, "hipMalloc(V scratch)"},
                                {&T, sizeof(double) * max_slots * NP * 256, "hipMalloc(T scratch)"}}))
    return rc_;
  gram = want_gram && gram_supported(rows, n) && ctx->opt.on(OPT_GRAM);
  if (gram) {
    gram_nchunk = gram_chunks(rows);
    const size_t tri = sizeof(double) * (size_t)B * NPAD * NPAD;
    if (int rc_ = alloc_all(ctx, {
            {&gram_part, gram_nchunk > 1 ? tri * gram_nchunk : 0, "hipMalloc(partial Grams)"},
            {&gram_dsc, sizeof(double) * (size_t)B * NPAD, "hipMalloc(Gram scales)"},
            {&gram_keep, tri, "hipMalloc(Grams)"},
            {&gram_rinv, sizeof(double) * (size_t)B * NP * 256, "hipMalloc(Gram tile inverses)"},
            {&gram_ywork, tri, "hipMalloc(Gram gate work)"},
            {&gram_k2, sizeof(double) * (size_t)B, "hipMalloc(Gram gate bound)"},
            {&gram_cert, sizeof(int) * (size_t)B, "hipMalloc(Gram certificate flags)"},
            {&gram_cflag, sizeof(int) * (size_t)B, "hipMalloc(certificate stage 3)"},
            {&gram_ctau, sizeof(double) * (size_t)B, "hipMalloc(certificate stage 3)"},
            {&gram_ints, sizeof(int) * (3 * (size_t)B + 4), "hipMalloc(Gram mask)"},   // launch mask, count, path, list
        })) return rc_;
    hipError_t e = hipMemsetAsync(gram_cflag.p, 0, gram_cflag.bytes, ctx->stream);
    if (e != hipSuccess) return ctx->fail(e, "hipMalloc(certificate stage 3)");
    k2_max = gram_k2_max(rows, ctx->opt.d(OPT_GRAM_K2_MAX));
    cqr2 = cqr2_supported(rows, n) && ctx->opt.on(OPT_CQR2);
    e = hipMemsetAsync(gram_cert.p, 0, gram_cert.bytes, ctx->stream);
    if (e != hipSuccess) return ctx->fail(e, "hipMemsetAsync(Gram certificate flags)");
    e = hipMemsetAsync(gram_k2.p, 0, gram_k2.bytes, ctx->stream);
    if (e != hipSuccess) return ctx->fail(e, "hipMemsetAsync(Gram gate bound)");
    e = hipMemsetAsync(gram_keep.p, 0, gram_keep.bytes, ctx->stream);      // (lower tiles are never written)
    if (e != hipSuccess) return ctx->fail(e, "hipMemsetAsync(Grams)");
    e = hipMemsetAsync(gram_ints.p, 0xFF, gram_ints.bytes, ctx->stream);   // path: all QR until factored
    if (e != hipSuccess) return ctx->fail(e, "hipMemsetAsync(Gram mask)");
  }
  return 0;
}

hipError_t QrTree::gram_sum(blsq_ctx* ctx, GramArgs g, double* Gp, double* Gout, int count, const int* red_mask,
                            int red_count) {
  g.G = gram_nchunk > 1 ? Gp : Gout;
  return ctx->timed(K_GRAM, [&] {
    bool fused = false;
    const hipError_t e = launch_gram(g, gram_nchunk, count, ctx->stream, Gout, &fused);
    if (e != hipSuccess || gram_nchunk == 1 || fused) return e;
    return launch_gram_reduce(Gp, gram_nchunk, NPAD, Gout, red_mask, red_count, ctx->stream);
  });
}

int QrTree::run_gram(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* mask,
                     int* nfallback, bool collective) {
  HIPCHK(ctx, hipMemsetAsync(fb_count(), 0, sizeof(int), ctx->stream));
  int rc = run_gram_only(ctx, dJ, df, ldJ, mask, collective);
  if (rc) return rc;
  // the plain Gram into the triangle slot: no diagonal modification, no list of the rejected, no in-kernel certificate
  GramCholArgs c = gate_args(mask);
  c.G = levels.back().R.as<double>();
  c.stride_vec = 0; c.fail_list = nullptr; c.cert_done = nullptr;
  if (int rc_ = ctx->run(K_GRAM_CHOL, "launch_gram_chol", [&] {
        return launch_gram_chol(c, B, ctx->stream);
      })) return rc_;
  if ((rc = run_cert(ctx, c))) return rc;
  const int* cnt = nullptr;
  HIPCHK(ctx, ctx->read_blocking(PIN_GATE, fb_count(), 1, &cnt));
  *nfallback = cnt[0];
  return 0;
}

GramCholArgs QrTree::gate_args(const int* mask) const {
  GramCholArgs c{};
  c.opt = opt;
  c.Gsrc = gram_keep.as<double>(); c.NPAD = NPAD; c.n = n; c.stride_vec = NPAD;
  c.mask = mask; c.fb_mask = fb_mask(); c.fail_count = fb_count(); c.path_out = path_rw();
  c.fail_list = fb_list();
  c.dsc = gram_dsc.as<double>();
  c.rinv = gram_rinv.as<double>(); c.ywork = gram_ywork.as<double>(); c.k2_out = gram_k2.as<double>();
  c.cert_done = gram_cert.as<int>();
  c.k2_max = k2_max; c.pivot_floor = 1.0 / k2_max;
  c.cert_flag = gram_cflag.as<int>(); c.cert_tau = gram_ctau.as<double>();
  return c;
}

int QrTree::run_cert(blsq_ctx* ctx, const GramCholArgs& c) {
  return ctx->run(K_GRAM_GATE, "launch_gram_gate", [&] {
    const hipError_t e = launch_gram_gate(c, B, ctx->stream);
    return e == hipSuccess ? launch_gram_cert_shift(c, B, ctx->stream) : e;
  });
}

int QrTree::run_gram_only(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* mask,
                          bool collective, int k0, int nb) {
  if (nb < 0) nb = B;
  const size_t tri = (size_t)NPAD * NPAD;
  GramArgs g{};
  g.opt = opt;
  g.J = dJ + (size_t)k0 * m * ldJ; g.strideJ = (long)m * ldJ; g.ldJ = ldJ; g.F = df + (size_t)k0 * m; g.strideF = m;
  g.m = m; g.n = n; g.NPAD = NPAD; g.mask = mask ? mask + k0 : nullptr;
  double* Gk = gram_keep.as<double>() + (size_t)k0 * tri;
  double* Gp = gram_nchunk > 1 ? gram_part.as<double>() + (size_t)k0 * gram_nchunk * tri : nullptr;
  hipError_t e = gram_sum(ctx, g, Gp, Gk, nb, g.mask, nb);
  if (e != hipSuccess) return ctx->fail(e, "launch_gram");
  if (collective && ctx->comm && ctx->comm_ranks > 1)
    RCCLCHK(ctx, g_rccl.AllReduce(Gk, Gk, (size_t)nb * NPAD * NPAD, ncclDouble, ncclSum, ctx->comm,
                                  ctx->stream));
  return 0;
}

int QrTree::run_levels(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* ncols_mask,
                       const int* list, int count) {
  for (size_t l = 0; l < levels.size(); ++l) {
    const Level& L = levels[l];
    QrArgs q = base_args();
    q.ncols_dev = ncols_mask;
    q.batch_list = list;
    if (l == 0) {
      q.A = dJ; q.strideA = (long)m * ldJ; q.ldA = ldJ; q.rowsA = m;
      q.F = df; q.strideF = m;
    } else {
      const Level& Pv = levels[l - 1];
      q.A = Pv.R.as<double>(); q.strideA = (long)Pv.nleaf * NPAD * NPAD;
      q.ldA = NPAD; q.rowsA = Pv.nleaf * NPAD; q.F = nullptr; q.strideF = 0;
      q.stack_rows = NPAD;
    }
    q.rows_per_leaf = L.rows_per_leaf; q.RP = L.RP; q.LDP = L.LDP;
    q.Rout = L.R.as<double>();
    if (int rc_ = ctx->run(l == 0 ? K_QR_LEAF : K_QR_MERGE, "launch_qr", [&] {
          return launch_qr(q, L.nleaf, list ? count : B, ctx->stream);
        })) return rc_;
  }
  return 0;
}

int QrTree::run_fallback(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, int nfb) {
  if (!cqr2 || !gram) return run_levels(ctx, dJ, df, ldJ, fb_mask(), fb_list(), nfb);
  hipError_t e = hipSuccess;
  // W = J R1^-1 and w_f for the LISTED problems only (list position, not problem index): sized by the high-water mark
  // of the list, grown geometrically — a single rejected problem of a 512-problem batch costs 8 MB, not 4.3 GB.
  if ((size_t)nfb > cq_cap) {
    const size_t cap = std::min<size_t>((size_t)B, std::max<size_t>((size_t)nfb, 2 * cq_cap));
    cq_W.release(); cq_Wf.release();
    e = cq_W.alloc(sizeof(double) * cap * m * n);
    if (e == hipSuccess) e = cq_Wf.alloc(sizeof(double) * cap * m);
    if (e != hipSuccess) {                              // no room for the second pass: the tree does it all
      cq_W.release(); cq_Wf.release(); cq_cap = 0;
      (void)hipGetLastError();
      return run_levels(ctx, dJ, df, ldJ, fb_mask(), fb_list(), nfb);
    }
    cq_cap = cap;
  }
  if (!cq_G2.p) {
    e = cq_G2.alloc(sizeof(double) * (size_t)B * NPAD * NPAD);
    if (e == hipSuccess) e = cq_R2.alloc(sizeof(double) * (size_t)B * NPAD * NPAD);
    if (e == hipSuccess) e = cq_R1.alloc(sizeof(double) * (size_t)B * NPAD * NPAD);
    if (e == hipSuccess) e = hipMemsetAsync(cq_R1.p, 0, cq_R1.bytes, ctx->stream);
    if (e == hipSuccess) e = cq_z.alloc(sizeof(double) * (size_t)B * NPAD);
    if (e == hipSuccess) e = cq_ints.alloc(sizeof(int) * (4 * (size_t)B + 4));
    if (e == hipSuccess) e = hipMemsetAsync(cq_G2.p, 0, cq_G2.bytes, ctx->stream);   // (lower tiles are never written)
    if (e == hipSuccess) e = hipMemsetAsync(cq_R2.p, 0, cq_R2.bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(cq_ints.p, 0, cq_ints.bytes, ctx->stream);
    if (e != hipSuccess) {                              // no room for the second pass: the tree does it all
      cq_G2.release(); cq_R1.release(); cq_R2.release(); cq_z.release(); cq_ints.release();
      cqr2 = false;
      (void)hipGetLastError();
      return run_levels(ctx, dJ, df, ldJ, fb_mask(), fb_list(), nfb);
    }
  }
  int* piv1 = cq_ints.as<int>();
  int* runm = piv1 + B;
  int* piv2 = piv1 + 2 * (size_t)B;
  int* tmask = piv1 + 3 * (size_t)B;
  int* cnt = piv1 + 4 * (size_t)B;
  double* Rf = levels.back().R.as<double>();
  double* R1 = cq_R1.as<double>();
  // 1. R1 | c = chol of the plain Gram (listed problems) into scratch, its tile inverses and scales
  GramCholArgs c{};
  c.opt = opt;
  c.Gsrc = gram_keep.as<double>(); c.G = R1; c.NPAD = NPAD; c.n = n; c.skip_zero = 1;
  c.batch_list = fb_list(); c.fb_mask = piv1; c.fail_count = cnt;
  c.dsc = gram_dsc.as<double>(); c.rinv = gram_rinv.as<double>(); c.ywork = gram_ywork.as<double>();
  c.k2_max = 1e300; c.pivot_floor = 1e-14;
  if (int rc_ = ctx->run(K_GRAM_CHOL, "launch_gram_chol(cqr2 first factor)", [&] {
        return launch_gram_chol(c, nfb, ctx->stream);
      })) return rc_;
  // 2. Y = R1'^-T by the certificate's kernel, which also bounds kappa_2 of the equilibrated plain Gram: the
  //    second pass multiplies by the EXPLICIT inverse, whose error enters the triangle as eps kappa(J) (measured:
  //    step error 2e-18 kappa, tools/cqr2_check.py), so the tier takes a problem only if that PROVEN bound is
  //    below CQR2_K2_MAX = 1e12 (kappa(J D) <= 1e6: error <= 2e-12); beyond, the Householder tree.
  GramCholArgs cy = c;
  cy.batch_list = nullptr; cy.mask = fb_mask(); cy.k2_max = CQR2_K2_MAX;
  // (the bound on the PLAIN equilibrated Gram also bounds the augmented system's — its spectrum lies inside,
  //  chol_rl.hip — so it replaces the missing / larger bound of a rejected problem: the rank gate uses it)
  cy.k2_out = gram_k2.as<double>();
  if (int rc_ = ctx->run(K_GRAM_GATE, "launch_gram_gate(cqr2 inverse)", [&] {
        return launch_gram_gate(cy, B, ctx->stream);
      })) return rc_;
  // 3. z = R^-1 c, launch mask;  4. W = J R^-1, w_f = f - J z
  Cqr2Args q{};
  q.J = dJ; q.strideJ = (long)m * ldJ; q.ldJ = ldJ; q.F = df; q.strideF = m;
  q.m = m; q.n = n; q.NPAD = NPAD; q.list = fb_list(); q.run = runm;
  q.Y = gram_ywork.as<double>(); q.dsc = gram_dsc.as<double>(); q.R1 = R1; q.z = cq_z.as<double>();
  q.Wj = cq_W.as<double>(); q.strideW = (long)m * n; q.Wf = cq_Wf.as<double>(); q.strideWf = m;
  if (int rc_ = ctx->run(K_CQR2_APPLY, "launch_cqr2_apply", [&] {
        const hipError_t ep = launch_cqr2_prep(q, nfb, piv1, runm, ctx->stream);
        return ep == hipSuccess ? launch_cqr2_apply(q, nfb, ctx->stream) : ep;
      })) return rc_;
  // 5. G2 = [W w_f]^T [W w_f]  (the launch over the list, the reduction over the run mask)
  GramArgs g{};
  g.opt = opt;
  g.J = q.Wj; g.strideJ = q.strideW; g.ldJ = n; g.F = q.Wf; g.strideF = m;
  g.m = m; g.n = n; g.NPAD = NPAD; g.mask = runm; g.list = fb_list();   // (compacted: all XCDs)
  g.src_by_pos = 1;                                   // (W holds the listed problems only)
  double* G2 = cq_G2.as<double>();
  e = gram_sum(ctx, g, gram_part.as<double>(), G2, nfb, runm, B);
  if (e != hipSuccess) return ctx->fail(e, "launch_gram(cqr2 second pass)");
  // 6. R2 | c2 = chol(G2)
  GramCholArgs c2{};
  c2.opt = opt;
  c2.Gsrc = G2; c2.G = cq_R2.as<double>(); c2.NPAD = NPAD; c2.n = n;
  c2.batch_list = fb_list(); c2.mask = runm; c2.fb_mask = piv2; c2.fail_count = cnt + 1;
  c2.k2_max = 1e300; c2.pivot_floor = 0.25;           // (G2 ~ I: a pivot below 1/2 means the first pass failed)
  if (int rc_ = ctx->run(K_GRAM_CHOL, "launch_gram_chol(cqr2 second factor)", [&] {
        return launch_gram_chol(c2, nfb, ctx->stream);
      })) return rc_;
  // 7. acceptance + R~ = R2 [R c; 0 1] into the triangle slot;  8. the tree for what is left
  if (int rc_ = ctx->run(K_CQR2_COMBINE, "launch_cqr2_combine", [&] {
        return launch_cqr2_combine(q, nfb, runm, piv2, G2, cq_R2.as<double>(), Rf, tmask, ctx->cq_accept_dev.as<unsigned long long>(),
            ctx->stream);
      })) return rc_;
  return run_levels(ctx, dJ, df, ldJ, tmask, fb_list(), nfb);
}

void QrTree::note_paths(blsq_ctx* ctx, int nfb, bool masked) {
  ctx->gram_fallback += nfb;
  ctx->gram_fast += B - nfb;              // (masked problems count as fast: diagnostics only)
  // a masked call refreshes some problems only: the others keep their earlier path
  if (!masked || !path_valid) { any_qr = nfb > 0 || masked; any_gram = nfb < B; }
  else { any_qr = any_qr || nfb > 0; any_gram = true; }
  path_valid = true;
}

int QrTree::run(blsq_ctx* ctx, const double* dJ, const double* df, int ldJ, const int* ncols_mask, bool collective) {
  if (gram && df != nullptr) {
    int nfb = 0;
    int rc = run_gram(ctx, dJ, df, ldJ, ncols_mask, &nfb, collective);
    if (rc) return rc;
    note_paths(ctx, nfb, ncols_mask != nullptr);
    if (nfb == 0) return 0;
    ncols_mask = fb_mask();                 // only the problems the gate rejected
  }
  else { any_gram = false; any_qr = true; path_valid = false; }
  return run_levels(ctx, dJ, df, ldJ, ncols_mask);
}

}  // namespace blsq_host

// ---- CSNE tier ------------------------------------------------------------------------------------

int CsneTier::build(blsq_ctx* ctx, int B, int m, int n, int ld, bool with_hp) {
  const char* what = "hipMalloc(CSNE state)";
  if (int rc_ = alloc_all(ctx, {{&ints, sizeof(int) * (5 * (size_t)B + 8), what},
                                {&pmin, sizeof(double) * (size_t)B, what},
                                {&eta, sizeof(double) * (size_t)B, what},
                                {&k2, sizeof(double) * (size_t)B, what},
                                {&alpha, sizeof(double) * (size_t)B * CSNE_MAXE, what},
                                {&hp, with_hp ? sizeof(double) * (size_t)B * ld : 0, what}}))
    return rc_;
  for (DevBuf* b : {&ints, &pmin, &eta, &k2}) HIPCHK(ctx, hipMemsetAsync(b->p, 0, b->bytes, ctx->stream));
  cs.B = B; cs.m = m; cs.n = n; cs.ld = ld;
  int* ii = ints.as<int>();
  cs.flag = ii; cs.list = ii + B; cs.fail_list = ii + 2 * (size_t)B; cs.ne = ii + 3 * (size_t)B;
  cs.counts = ii + 5 * (size_t)B;                     // (sel_mask: ii + 4 B; scratch counter: counts + 4)
  cs.ralpha = alpha.as<double>(); cs.hp = hp.as<double>(); cs.eta = eta.as<double>();
  csne_geometry(m, &cs.rows_per_wg, &cs.nchunk);
  cs.NE = with_hp ? CSNE_MAXE : 1;
  on = true;
  return 0;
}

// (TRF: 52 KB per problem at n = 256; dogbox records one evaluation, the Newton step)
bool CsneTier::ensure_recordings() {
  if (!vec.p && vec.alloc(sizeof(double) * (size_t)cs.B * CSNE_MAXE * 3 * cs.ld) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  cs.rvec = vec.as<double>();
  return true;
}

// (grows geometrically; hipFree waits for the stream)
int CsneTier::grow_part(blsq_ctx* ctx, size_t need) {
  if (need <= part_cap) return 0;
  const size_t cap = std::max(need, 2 * part_cap);
  if (int rc_ = alloc_all(ctx, {{&part, sizeof(double) * cap, "hipMalloc(CSNE partial sums)"}})) {
    part_cap = 0;
    return rc_;
  }
  part_cap = cap;
  cs.part = part.as<double>();
  return 0;
}

int CsneTier::relist(blsq_ctx* ctx) {
  hipError_t e = launch_csne_reroute(cs, -1, nullptr, nullptr, nullptr, ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_csne_reroute(relist)");
  const int* c = nullptr;
  HIPCHK(ctx, ctx->read_blocking(PIN_CSNE_LIST, cs.counts, 1, &c));
  count = c[0];
  return 0;
}

int CsneTier::pass_begin(blsq_ctx* ctx) {
  if (int rc_ = grow_part(ctx, (size_t)count * cs.nchunk * ((size_t)cs.NE * cs.ld + 16))) return rc_;
  HIPCHK(ctx, hipMemsetAsync(cs.counts + 1, 0, sizeof(int), ctx->stream));
  return 0;
}

int CsneTier::pass_verdict(blsq_ctx* ctx, bool polled, int* nfail) {
  const int* c = nullptr;
  HIPCHK(ctx, polled ? ctx->read_polled(PIN_CSNE_FAIL_POLLED, cs.counts + 1, 1, &c)
                     : ctx->read_blocking(PIN_CSNE_FAIL, cs.counts + 1, 1, &c));
  *nfail = c[0];
  ctx->csne_steps += (unsigned long long)(count - *nfail);
  ctx->csne_declined += (unsigned long long)*nfail;
  return 0;
}

int CsneTier::reroute(blsq_ctx* ctx, QrTree& t, int nfail) {
  hipError_t e = launch_csne_reroute(cs, nfail, t.fb_list(), t.fb_mask(), t.path_rw(), ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_csne_reroute");
  count -= nfail;
  t.any_qr = true;
  return 0;
}

int CsneTier::select(blsq_ctx* ctx, QrTree& t, const GramCholArgs& chol, int nfb, int* ntree, bool masked,
                     const std::function<hipError_t(const int* sel_mask)>& launch_select) {
  const int B = cs.B;
  int* sel = ints.as<int>() + 4 * (size_t)B;
  HIPCHK(ctx, hipMemsetAsync(sel, 0, sizeof(int) * (size_t)B, ctx->stream));
  // the norm stage alone, into the tier's own outputs: everything else either solver's factor / certificate launches
  // would write or read is cleared (a field the solver never set is null already)
  GramCholArgs cy = chol;
  cy.fb_mask = sel; cy.fail_count = cs.counts + 4; cy.fail_list = nullptr; cy.path_out = nullptr;
  cy.cert_done = nullptr; cy.cert_flag = nullptr; cy.cert_tau = nullptr; cy.cert_open = nullptr;
  cy.cert_ym = nullptr; cy.cert_r1 = nullptr; cy.unsettled = nullptr;
  cy.lmfin = GramCholArgs::LmFinish{}; cy.dog = GramCholArgs::DogFinish{};
  cy.lam_out = nullptr; cy.hmax = nullptr; cy.colinfo = nullptr; cy.pmin_out = nullptr;
  cy.k2_max = CSNE_K2_MAX; cy.k2_out = k2.as<double>();
  if (int rc_ = ctx->run(K_GRAM_GATE, "launch_gram_gate(csne bound)", [&] {
        return launch_gram_gate(cy, B, ctx->stream);
      })) return rc_;
  const hipError_t e = launch_select(sel);
  if (e != hipSuccess) return ctx->fail(e, "launch_csne_select");
  // two counters to the host: the problems left for the tree, the problems on the tier
  const int* c = nullptr;
  HIPCHK(ctx, ctx->read_blocking(PIN_CSNE_LIST, t.fb_count(), 1, &c, cs.counts));
  *ntree = c[0];
  count = c[1];
  ctx->csne_routed += (unsigned long long)(nfb - *ntree);
  if (!masked) t.any_qr = *ntree > 0;                     // (a masked call keeps the others' paths: any_qr stays)
  t.any_gram = t.any_gram || *ntree < nfb;
  return 0;
}

// ---- what the TRF and the dogbox entry points share (StepPlan) ---------------------------------------------------
namespace blsq_host {

int step_plan_args(blsq_ctx* ctx, int B, int m, int n, const void* out) {
  if (!out) return ctx->bad(5, "out is NULL");
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n <= 0) return ctx->bad(4, "n must be positive");
  return 0;
}

int step_plan_init(blsq_ctx* ctx, StepPlan* p, int B, int m, int n, size_t extra_rp_rows, bool verdicts,
                   const std::function<int()>& alloc_state) {
  p->ctx = ctx; p->B = B; p->m = m; p->n = n;
  hipError_t e = hipSetDevice(ctx->device);
  int rc = e == hipSuccess ? 0 : ctx->fail(e, "hipSetDevice(ctx->device)");
  if (rc == 0) rc = p->tree.build(ctx, B, m, n, extra_rp_rows);
  if (rc == 0) { p->ld = p->tree.NPAD; rc = alloc_state(); }
  if (rc == 0 && verdicts) {
    p->optimistic = ctx->opt.on(OPT_OPTIMISTIC);
    e = p->pend_pin.alloc(4, hipHostMallocCoherent);
    if (e != hipSuccess) rc = ctx->fail(e, "optimistic-verdict resources");
  }
  if (rc == 0 && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    rc = ctx->fail(e, "hipStreamSynchronize(ctx->stream)");
  if (rc != 0) { step_plan_destroy(p); return rc; }
  ctx->plans.push_back(p);
  return 0;
}

int step_plan_destroy(StepPlan* p) {
  if (!p) return -1;
  hipStreamSynchronize(p->ctx->stream);
  { auto& v = p->ctx->plans; v.erase(std::remove(v.begin(), v.end(), p), v.end()); }
  delete p;
  return 0;
}

int factor_args(blsq_ctx* ctx, const void* J, const void* f, const void* x, const void* lb, const void* ub,
                const void* scale, int scale_mode) {
  if (!J) return ctx->bad(2, "J is NULL");
  if (!f) return ctx->bad(3, "f is NULL");
  if (!x || !lb || !ub) return ctx->bad(4, "x/lb/ub is NULL");
  if (!scale) return ctx->bad(7, "scale is NULL");
  if (scale_mode < 0 || scale_mode > 2) return ctx->bad(8, "scale_mode");
  return 0;
}

int stage_alloc(StepPlan* p) {
  if (p->in_J.p && p->in_f.p) return 0;
  return alloc_all(p->ctx, {{&p->in_J, sizeof(double) * (size_t)p->B * p->m * p->n, "hipMalloc(J staging)"},
                            {&p->in_f, sizeof(double) * (size_t)p->B * p->m, "hipMalloc(f staging)"}});
}

int stage_upload(StepPlan* p, const double* J, const double* f) {
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, hipMemcpyAsync(p->in_J.p, J, p->in_J.bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(p->in_f.p, f, p->in_f.bytes, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

int put_state(StepPlan* p, const double* x, const double* lb, const double* ub, const double* scale,
              const int64_t* on_bound, hipMemcpyKind kind, bool zero_counts) {
  blsq_ctx* ctx = p->ctx;
  int rc;
  if (kind == hipMemcpyDeviceToDevice) {                // one launch instead of four (five) strided copies
    p->pack_pend = zero_counts && p->tree.gram;
    p->tree.fb_zeroed = p->pack_pend;
    PackVecs pv{{x, lb, ub, scale, on_bound}, {p->vec(0), p->vec(1), p->vec(2), p->scale(), on_bound ? p->on_bound : nullptr},
                p->pack_pend ? p->tree.fb_count() : nullptr, 3};
    if (p->pack_pend) { p->pack_pv = pv; return 0; }
    hipError_t e = launch_pack_vecs(pv, p->n, p->ld, p->B, ctx->stream);
    if (e != hipSuccess) return ctx->fail(e, "launch_pack_vecs");
    return 0;
  }
  if ((rc = put_vec(ctx, p->vec(0), p->ld, x, p->n, p->B, kind))) return rc;
  if ((rc = put_vec(ctx, p->vec(1), p->ld, lb, p->n, p->B, kind))) return rc;
  if ((rc = put_vec(ctx, p->vec(2), p->ld, ub, p->n, p->B, kind))) return rc;
  if ((rc = put_vec(ctx, p->scale(), p->ld, scale, p->n, p->B, kind))) return rc;
  if (on_bound)
    HIPCHK(ctx, hipMemcpy2DAsync(p->on_bound, sizeof(long long) * p->ld, on_bound, sizeof(long long) * p->n,
                                 sizeof(long long) * p->n, p->B, kind, ctx->stream));
  return 0;
}

int scale_back(StepPlan* p, double* dscale_io, int scale_mode) {
  blsq_ctx* ctx = p->ctx;
  if (scale_mode == BLSQ_SCALE_GIVEN || !dscale_io) return 0;
  HIPCHK(ctx, hipMemcpy2DAsync(dscale_io, sizeof(double) * p->n, p->scale(), sizeof(double) * p->ld,
                               sizeof(double) * p->n, p->B, hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

int fetch_resolved(StepPlan* p, void* dst, const void* src, size_t item) {
  blsq_ctx* ctx = p->ctx;
  { int rc_ = p->resolve(nullptr); if (rc_) return rc_; }
  HIPCHK(ctx, hipMemcpyAsync(dst, src, item * p->B, hipMemcpyDeviceToHost, ctx->stream));
  return blsq_sync(ctx);
}

int debug_cond(StepPlan* p, double* k2) {
  if (!p) return -1;
  if (!k2) return p->ctx->bad(2, "k2 is NULL");
  if (!p->tree.gram) { for (int b = 0; b < p->B; ++b) k2[b] = 0.0; return 0; }
  return fetch_resolved(p, k2, p->tree.gram_k2.p, sizeof(double));
}

int fetch_scal_info(StepPlan* p, std::vector<double>* sc, std::vector<int>* inf) {
  blsq_ctx* ctx = p->ctx;
  sc->resize(p->o_scal.bytes / sizeof(double));
  inf->resize(p->o_info.bytes / sizeof(int));
  HIPCHK(ctx, hipMemcpyAsync(sc->data(), p->o_scal.p, p->o_scal.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(inf->data(), p->o_info.p, p->o_info.bytes, hipMemcpyDeviceToHost, ctx->stream));
  return blsq_sync(ctx);
}

int gate_verdict(StepPlan* p, bool polled, bool masked, bool settles, int* nfb) {
  blsq_ctx* ctx = p->ctx;
  const int* c = nullptr;
  HIPCHK(ctx, polled ? ctx->read_polled(PIN_GATE_POLLED, p->tree.fb_count(), 3, &c)
                     : ctx->read_blocking(PIN_GATE, p->tree.fb_count(), 3, &c));
  *nfb = c[0];
  p->gate_done = (*nfb == 0);
  p->njac = p->gate_done ? c[1] : -1;
  if (!masked) { p->guess_ok = (*nfb == 0 && p->njac == 0); p->guess_settled = (settles && c[2] == 0); }
  return 0;
}

int run_jacobi(StepPlan* p, double* X, double* s, double* uf, double* srange, const int* ncols_dev) {
  blsq_ctx* ctx = p->ctx;
  JacobiArgs ja{};
  ja.X = X; ja.strideX = (long)p->ld * p->ld; ja.ld = p->ld; ja.ncols_dev = ncols_dev;
  ja.N = p->n + 1; ja.s = s; ja.uf = uf; ja.srange = srange;
  ja.sweeps = p->sweeps.as<int>(); ja.max_sweeps = 40;
  return ctx->run(K_JACOBI, "launch_jacobi", [&] { return launch_jacobi(ja, p->B, ctx->stream); });
}

int take_pack(StepPlan* p, const int* mask, const PackVecs** pk) {
  *pk = nullptr;
  QrTree& t = p->tree;
  if (!t.fb_zeroed) HIPCHK(p->ctx, hipMemsetAsync(t.fb_count(), 0, 3 * sizeof(int), p->ctx->stream));
  t.fb_zeroed = false;
  if (!p->pack_pend) return 0;
  p->pack_pend = false;
  if (!mask) { *pk = &p->pack_pv; return 0; }
  hipError_t e = launch_pack_vecs(p->pack_pv, p->n, p->ld, p->B, p->ctx->stream);
  if (e != hipSuccess) return p->ctx->fail(e, "launch_pack_vecs");
  return 0;
}

int verdict_published(StepPlan* p) {
  if (!p->pend_unpub) return 0;
  p->pend_unpub = false;
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, ctx->publish(p->tree.fb_count(), 3, p->pend_pin, &p->pend_seq));
  return 0;
}

int verdict_drop(StepPlan* p) {
  if (!p->pending) return 0;
  blsq_ctx* ctx = p->ctx;
  p->pending = false;
  { int rc_ = verdict_published(p); if (rc_) return rc_; }
  HIPCHK(ctx, ctx->await(p->pend_pin, p->pend_seq));
  const int nfb_ = p->pend_pin[0], njac_ = p->pend_pin[1];
  if (p->pend_tail) { if (!verdict_settled(p)) p->guess_settled = false; }
  else if (nfb_ > 0 || njac_ > 0) {
    p->guess_ok = false;
    verdict_wrong(p);
    ctx->gram_fast -= nfb_; ctx->gram_fallback += nfb_;
  } else verdict_right(p);
  return 0;
}

}  // namespace blsq_host
