// C-ABI entry points (include/blsq.h): parameter covariance from the final Jacobian.
//   tree (Householder TSQR of the plain J, or of J with its free columns first)  ->  cov_inverse  ->  cov_product
//   pseudo-inverse route (7h):                                      the same tree  ->  Jacobi SVD of the triangle
//                                                                   ->  cov_pinv_weights  ->  cov_pinv_product
//   row forms (7i, blsq_cov_rows*): the factor either route has left in the plan  ->  cov_rows (pinv: the factor is
//                                                                   refined by the first such call, cov_pinv_rowfactor)
#include "blsq_host.h"

extern "C" int blsq_cov_plan_create(blsq_ctx* ctx, int B, int m, int n, blsq_cov_plan** out) {
  if (!ctx) return -1;
  if (!out) return ctx->bad(5, "out is NULL");
  *out = nullptr;
  if (B <= 0 || B > 65535) return ctx->bad(2, "B must be in 1..65535");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n <= 0) return ctx->bad(4, "n must be positive");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  blsq_cov_plan* p = new blsq_cov_plan();
  p->ctx = ctx; p->B = B; p->m = m; p->n = n;
  p->tree.want_gram = false;
  int rc = 0;
  const int npad = round_up(n + 1, 16);
  if (m > RMAX && !merge_fits(n) && npad + 16 <= RMAX) {
    p->fold = true; p->NPAD = npad;
    const size_t np = (size_t)npad / 16;
    rc = alloc_all(ctx, {{&p->fR, sizeof(double) * (size_t)B * npad * npad, "hipMalloc(covariance triangles)"},
                         {&p->fS, sizeof(double) * (size_t)B * RMAX * npad, "hipMalloc(covariance stack)"},
                         {&p->fV, sizeof(double) * (size_t)B * np * RMAX * 16, "hipMalloc(V scratch)"},
                         {&p->fT, sizeof(double) * (size_t)B * np * 256, "hipMalloc(T scratch)"}});
    if (rc == 0) {
      const hipError_t e = hipMemsetAsync(p->fS.p, 0, p->fS.bytes, ctx->stream);   // (columns >= n stay zero)
      if (e != hipSuccess) rc = ctx->fail(e, "hipMemsetAsync(covariance stack)");
    }
  } else {
    rc = p->tree.build(ctx, B, m, n, 0);
    p->NPAD = p->tree.NPAD;
  }
  if (rc == 0) {
    const size_t tri = sizeof(double) * (size_t)B * p->NPAD * p->NPAD;
    rc = alloc_all(ctx, {{&p->zf, sizeof(double) * (size_t)B * m, "hipMalloc(covariance rhs)"},
                         {&p->X, tri, "hipMalloc(covariance inverse)"},
                         {&p->kept_status, sizeof(int) * (size_t)B, "hipMalloc(covariance status)"}});
  }
  if (rc == 0) {
    hipError_t e = hipMemsetAsync(p->zf.p, 0, p->zf.bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->X.p, 0, p->X.bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = ctx->fail(e, "hipMemsetAsync(covariance plan)");
  }
  if (rc != 0) { blsq_cov_plan_destroy(p); return rc; }
  *out = p;
  return 0;
}

extern "C" int blsq_cov_plan_destroy(blsq_cov_plan* p) {
  if (!p) return -1;
  hipStreamSynchronize(p->ctx->stream);
  delete p;
  return 0;
}

namespace {
// The triangle of a plan past the tree's merge capacity (m > 1024, n > 512): the first 1024 rows as one dense leaf,
// then [R; next rows] again and again — every launch one workgroup per problem on at most 1024 rows.
int cov_fold(blsq_cov_plan* p, const double* dJ) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, m = p->m, n = p->n, NPAD = p->NPAD;
  QrArgs q{};
  q.opt = &ctx->opt;
  q.N = n + 1; q.NPAD = NPAD; q.NPmax = NPAD / 16;
  q.V = p->fV.as<double>(); q.T = p->fT.as<double>();
  q.Rout = p->fR.as<double>();
  q.A = dJ; q.strideA = (long)m * n; q.ldA = n; q.rowsA = RMAX;
  q.F = p->zf.as<double>(); q.strideF = m;
  q.rows_per_leaf = RMAX; q.RP = RMAX;
  if (int rc_ = ctx->run(K_QR_LEAF, "launch_qr(covariance fold)", [&] { return launch_qr(q, 1, B, ctx->stream); }))
    return rc_;
  const int chunk = RMAX - NPAD;
  for (int r = RMAX; r < m; r += chunk) {
    const int c = std::min(chunk, m - r);
    HIPCHK(ctx, hipMemcpy2DAsync(p->fS.p, sizeof(double) * (size_t)RMAX * NPAD, p->fR.p,
                                 sizeof(double) * (size_t)NPAD * NPAD, sizeof(double) * (size_t)NPAD * NPAD, B,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    QrArgs s = q;
    s.A = p->fS.as<double>(); s.strideA = (long)RMAX * NPAD; s.ldA = NPAD; s.rowsA = NPAD + c;
    s.F = nullptr; s.strideF = 0;                     // (column n of the stack: zeros)
    s.rows_per_leaf = s.RP = round_up(NPAD + c, 16);
    if (int rc_ = ctx->run(K_QR_MERGE, "launch_qr(covariance fold)", [&] {
          const hipError_t e = launch_cov_stack(B, m, n, r, c, dJ, p->fS.as<double>(), RMAX, NPAD, ctx->stream);
          return e == hipSuccess ? launch_qr(s, 1, B, ctx->stream) : e;
        })) return rc_;
  }
  return 0;
}
}  // namespace

namespace {
// The triangle of every problem in the plan's Rfinal slot: of the plain J, or with a mask of J gathered with its free
// columns first (perm, nfree: the plan's; nullptr without a mask).  want_ncols: nfree + 1 per problem into jncols.
int cov_triangle(blsq_cov_plan* p, const double* dJ, const long long* dactive, int lda, const int** perm_out,
                 const int** nfree_out, bool want_ncols) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, m = p->m, n = p->n;
  const double* src = dJ;
  *perm_out = nullptr;
  *nfree_out = nullptr;
  if (dactive) {
    if (!p->perm.p) {
      if (int rc_ = alloc_all(ctx, {{&p->perm, sizeof(int) * (size_t)B * n, "hipMalloc(covariance permutation)"},
                                    {&p->nfree, sizeof(int) * (size_t)B, "hipMalloc(covariance free counts)"},
                                    {&p->Jp, sizeof(double) * (size_t)B * m * n, "hipMalloc(covariance gather)"}}))
        return rc_;
    }
    if (int rc_ = ctx->run(K_COV_GATHER, "launch_cov_gather", [&] {
          const hipError_t e = launch_cov_perm(B, n, dactive, lda, p->perm.as<int>(), p->nfree.as<int>(),
                                               want_ncols ? p->jncols.as<int>() : nullptr, ctx->stream);
          return e == hipSuccess ? launch_cov_gather(B, m, n, dJ, p->perm.as<int>(), p->Jp.as<double>(), ctx->stream)
                                 : e;
        })) return rc_;
    src = p->Jp.as<double>(); *perm_out = p->perm.as<int>(); *nfree_out = p->nfree.as<int>();
  }
  return p->fold ? cov_fold(p, src) : p->tree.run_levels(ctx, src, p->zf.as<double>(), n, nullptr);
}
}  // namespace

namespace {
// A covariance call has run to its end: what blsq_cov_rows* needs of it stays with the plan (the factor is where the
// route left it; the caller's status buffer is copied, not kept)
int cov_keep(blsq_cov_plan* p, blsq_cov_plan::Kept route, bool masked, const int* dstatus) {
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, hipMemcpyAsync(p->kept_status.p, dstatus, sizeof(int) * (size_t)p->B, hipMemcpyDeviceToDevice,
                             ctx->stream));
  p->kept = route; p->kept_masked = masked; p->kept_refined = false;
  return 0;
}
}  // namespace

namespace blsq_host {
int cov_core(blsq_cov_plan* p, const double* dJ, const long long* dactive, int lda, double* dcov, double* drcond,
             int* dstatus) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, m = p->m, n = p->n, NPAD = p->NPAD;
  const int* perm = nullptr;
  const int* nfree = nullptr;
  p->kept = blsq_cov_plan::KEPT_NONE; p->kept_staged = false;   // (the slots are being overwritten)
  if (int rc_ = cov_triangle(p, dJ, dactive, lda, &perm, &nfree, false)) return rc_;
  if (int rc_ = ctx->run(K_COV_INVERSE, "launch_cov_inverse", [&] {
        return launch_cov_inverse(B, m, n, NPAD, p->Rfinal(), p->X.as<double>(), nfree, dcov, drcond, dstatus,
                                  ctx->stream);
      })) return rc_;
  if (int rc_ = ctx->run(K_COV_PRODUCT, "launch_cov_product", [&] {
        return launch_cov_product(B, n, NPAD, p->X.as<double>(), nfree, perm, dstatus, dcov, ctx->stream);
      })) return rc_;
  return cov_keep(p, blsq_cov_plan::KEPT_REGULAR, dactive != nullptr, dstatus);
}

int cov_rows_core(blsq_cov_plan* p, int rows, const double* dA, const double* dscale, double* dout) {
  blsq_ctx* ctx = p->ctx;
  const bool pinv = p->kept == blsq_cov_plan::KEPT_PINV;
  const int* perm = p->kept_masked ? p->perm.as<int>() : nullptr;
  const int* nfree = p->kept_masked ? p->nfree.as<int>() : nullptr;
  const bool refine = pinv && !p->kept_refined;      // the first row-form call after a pinv covariance call
  if (refine && !p->rowgram.p)
    if (int rc_ = alloc_all(ctx, {{&p->rowgram, p->X.bytes, "hipMalloc(covariance row Gram)"}})) return rc_;
  if (int rc_ = ctx->run(K_COV_ROWS, "launch_cov_rows", [&] {
        if (refine) {
          const hipError_t e = launch_cov_pinv_rowfactor(p->B, p->n, p->NPAD, p->Rfinal(), p->pw.as<double>(), nfree,
                                                         p->kept_status.as<int>(), p->rowgram.as<double>(),
                                                         p->X.as<double>(), ctx->stream);
          if (e != hipSuccess) return e;
        }
        return launch_cov_rows(p->B, rows, p->n, p->NPAD, pinv ? 1 : 0, dA, perm, nfree, p->X.as<double>(), nullptr,
                               p->kept_status.as<int>(), dscale, dout, ctx->stream);
      })) return rc_;
  if (refine) p->kept_refined = true;
  return 0;
}

// Jacobi sweeps granted to a covariance triangle (as the step plans' factor calls)
static constexpr int COV_MAX_SWEEPS = 40;

int cov_pinv_core(blsq_cov_plan* p, const double* dJ, const long long* dactive, int lda, const double* dscale,
                  double* dcov, int* drank, double* drcond, double* dkept, int* dstatus) {
  blsq_ctx* ctx = p->ctx;
  const int B = p->B, m = p->m, n = p->n, NPAD = p->NPAD;
  if (!p->js.p) {
    const size_t vec = sizeof(double) * (size_t)B * NPAD;
    if (int rc_ = alloc_all(ctx, {{&p->js, vec, "hipMalloc(covariance singular values)"},
                                  {&p->juf, vec, "hipMalloc(covariance Jacobi rhs)"},
                                  {&p->jsrange, sizeof(double) * (size_t)B * 2, "hipMalloc(covariance Jacobi range)"},
                                  {&p->jsweeps, sizeof(int) * (size_t)B, "hipMalloc(covariance Jacobi sweeps)"},
                                  {&p->jncols, sizeof(int) * (size_t)B, "hipMalloc(covariance Jacobi widths)"},
                                  {&p->pw, vec, "hipMalloc(covariance weights)"}}))
      return rc_;
  }
  const int* perm = nullptr;
  const int* nfree = nullptr;
  p->kept = blsq_cov_plan::KEPT_NONE; p->kept_staged = false;
  if (int rc_ = cov_triangle(p, dJ, dactive, lda, &perm, &nfree, true)) return rc_;
  double* tri = const_cast<double*>(p->Rfinal());    // rotated in place: the next call rebuilds it
  JacobiArgs ja{};
  ja.X = tri; ja.strideX = (long)NPAD * NPAD; ja.ld = NPAD;
  ja.ncols_dev = dactive ? p->jncols.as<int>() : nullptr;
  ja.N = n + 1; ja.s = p->js.as<double>(); ja.uf = p->juf.as<double>(); ja.srange = p->jsrange.as<double>();
  ja.sweeps = p->jsweeps.as<int>(); ja.max_sweeps = COV_MAX_SWEEPS;
  if (int rc_ = ctx->run(K_JACOBI, "launch_jacobi(covariance)", [&] { return launch_jacobi(ja, B, ctx->stream); }))
    return rc_;
  if (int rc_ = ctx->run(K_COV_PINV_WEIGHTS, "launch_cov_pinv_weights", [&] {
        return launch_cov_pinv_weights(B, m, n, NPAD, tri, p->js.as<double>(), p->jsweeps.as<int>(), COV_MAX_SWEEPS,
                                       nfree, p->pw.as<double>(), dcov, drank, drcond, dkept, dstatus, ctx->stream);
      })) return rc_;
  if (int rc_ = ctx->run(K_COV_PINV_PRODUCT, "launch_cov_pinv_product", [&] {
        return launch_cov_pinv_product(B, n, NPAD, tri, p->pw.as<double>(), nfree, perm, dstatus, dscale, dcov,
                                       ctx->stream);
      })) return rc_;
  return cov_keep(p, blsq_cov_plan::KEPT_PINV, dactive != nullptr, dstatus);
}
}  // namespace blsq_host

extern "C" int blsq_cov_dev(blsq_cov_plan* p, const double* dJ, const int64_t* dactive, double* dcov, double* drcond,
                            int32_t* dstatus) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!dJ) return ctx->bad(2, "J is NULL");
  if (!dcov) return ctx->bad(4, "cov is NULL");
  if (!drcond) return ctx->bad(5, "rcond is NULL");
  if (!dstatus) return ctx->bad(6, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return cov_core(p, dJ, reinterpret_cast<const long long*>(dactive), p->n, dcov, drcond, dstatus);
}

namespace {
// the device outputs of a plan's host-pointer calls (allocated on first use)
int cov_outputs(blsq_cov_plan* p) {
  if (p->o_cov.p) return 0;
  const size_t B = (size_t)p->B;
  return alloc_all(p->ctx, {{&p->o_cov, sizeof(double) * B * p->n * p->n, "hipMalloc(covariance output)"},
                            {&p->o_rcond, sizeof(double) * B, "hipMalloc(covariance output)"},
                            {&p->o_status, sizeof(int) * B, "hipMalloc(covariance output)"}});
}
// the inputs of a host-pointer call into the plan's staging (allocated on first use): J, the mask and the scale if given
int cov_stage_inputs(blsq_cov_plan* p, const double* J, const int64_t* active, const double* scale) {
  blsq_ctx* ctx = p->ctx;
  const size_t B = (size_t)p->B, nJ = sizeof(double) * B * p->m * p->n, nA = sizeof(int64_t) * B * p->n;
  if (!p->in_J.p)
    if (int rc_ = alloc_all(ctx, {{&p->in_J, nJ, "hipMalloc(covariance input)"}})) return rc_;
  if (active && !p->in_act.p)
    if (int rc_ = alloc_all(ctx, {{&p->in_act, nA, "hipMalloc(covariance input)"}})) return rc_;
  if (scale && !p->in_scale.p)
    if (int rc_ = alloc_all(ctx, {{&p->in_scale, sizeof(double) * B, "hipMalloc(covariance input)"}})) return rc_;
  HIPCHK(ctx, hipMemcpyAsync(p->in_J.p, J, nJ, hipMemcpyHostToDevice, ctx->stream));
  if (active) HIPCHK(ctx, hipMemcpyAsync(p->in_act.p, active, nA, hipMemcpyHostToDevice, ctx->stream));
  if (scale) HIPCHK(ctx, hipMemcpyAsync(p->in_scale.p, scale, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}
int cov_download(blsq_cov_plan* p, double* cov, double* rcond, int32_t* status) {
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, hipMemcpyAsync(cov, p->o_cov.p, p->o_cov.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(rcond, p->o_rcond.p, p->o_rcond.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(status, p->o_status.p, p->o_status.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // namespace

extern "C" int blsq_cov(blsq_cov_plan* p, const double* J, const int64_t* active, double* cov, double* rcond,
                        int32_t* status) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (!J) return ctx->bad(2, "J is NULL");
  if (!cov) return ctx->bad(4, "cov is NULL");
  if (!rcond) return ctx->bad(5, "rcond is NULL");
  if (!status) return ctx->bad(6, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc_ = cov_stage_inputs(p, J, active, nullptr)) return rc_;
  if (int rc_ = cov_to_host(p, p->in_J.as<double>(), active ? p->in_act.as<long long>() : nullptr, p->n, cov, rcond,
                            status))
    return rc_;
  p->kept_staged = true;                              // (in_J holds this call's J: blsq_cov_rows with A = NULL)
  return 0;
}

namespace {
int cov_pinv_outputs(blsq_cov_plan* p) {
  if (int rc_ = cov_outputs(p)) return rc_;
  if (p->o_rank.p) return 0;
  const size_t B = (size_t)p->B;
  return alloc_all(p->ctx, {{&p->o_rank, sizeof(int) * B, "hipMalloc(covariance output)"},
                            {&p->o_kept, sizeof(double) * B, "hipMalloc(covariance output)"}});
}
int cov_pinv_download(blsq_cov_plan* p, double* cov, int32_t* rank, double* rcond, double* kept, int32_t* status) {
  blsq_ctx* ctx = p->ctx;
  HIPCHK(ctx, hipMemcpyAsync(rank, p->o_rank.p, p->o_rank.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(kept, p->o_kept.p, p->o_kept.bytes, hipMemcpyDeviceToHost, ctx->stream));
  return cov_download(p, cov, rcond, status);
}
int cov_pinv_args(blsq_ctx* ctx, const void* J, const void* cov, const void* rank, const void* rcond, const void* kept,
                  const void* status) {
  if (!J) return ctx->bad(2, "J is NULL");
  if (!cov) return ctx->bad(5, "cov is NULL");
  if (!rank) return ctx->bad(6, "rank is NULL");
  if (!rcond) return ctx->bad(7, "rcond is NULL");
  if (!kept) return ctx->bad(8, "kept_rcond is NULL");
  if (!status) return ctx->bad(9, "status is NULL");
  return 0;
}
}  // namespace

extern "C" int blsq_cov_pinv_dev(blsq_cov_plan* p, const double* dJ, const int64_t* dactive, const double* dscale,
                                 double* dcov, int32_t* drank, double* drcond, double* dkept_rcond,
                                 int32_t* dstatus) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (int rc_ = cov_pinv_args(ctx, dJ, dcov, drank, drcond, dkept_rcond, dstatus)) return rc_;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return cov_pinv_core(p, dJ, reinterpret_cast<const long long*>(dactive), p->n, dscale, dcov, drank, drcond,
                       dkept_rcond, dstatus);
}

extern "C" int blsq_cov_pinv(blsq_cov_plan* p, const double* J, const int64_t* active, const double* scale,
                             double* cov, int32_t* rank, double* rcond, double* kept_rcond, int32_t* status) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (int rc_ = cov_pinv_args(ctx, J, cov, rank, rcond, kept_rcond, status)) return rc_;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc_ = cov_stage_inputs(p, J, active, scale)) return rc_;
  if (int rc_ = cov_pinv_to_host(p, p->in_J.as<double>(), active ? p->in_act.as<long long>() : nullptr, p->n,
                                 scale ? p->in_scale.as<double>() : nullptr, cov, rank, rcond, kept_rcond, status))
    return rc_;
  p->kept_staged = true;
  return 0;
}

// ---- row forms through the kept factor ------------------------------------------------------------
extern "C" int blsq_cov_rows_dev(blsq_cov_plan* p, int rows, const double* dA, const double* dscale, double* dout) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (p->kept == blsq_cov_plan::KEPT_NONE) return ctx->bad(1, "no covariance factor yet (call blsq_cov* first)");
  if (rows <= 0) return ctx->bad(2, "rows must be positive");
  if (!dA) return ctx->bad(3, "A is NULL");
  if (!dout) return ctx->bad(5, "out is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return cov_rows_core(p, rows, dA, dscale, dout);
}

extern "C" int blsq_cov_rows(blsq_cov_plan* p, int rows, const double* A, const double* scale, double* out) {
  if (!p) return -1;
  blsq_ctx* ctx = p->ctx;
  if (p->kept == blsq_cov_plan::KEPT_NONE) return ctx->bad(1, "no covariance factor yet (call blsq_cov* first)");
  if (rows <= 0) return ctx->bad(2, "rows must be positive");
  if (!A && !p->kept_staged) return ctx->bad(3, 
                         "A is NULL and the last covariance call staged no J (blsq_cov / blsq_cov_pinv do)");
  if (!A && rows != p->m) return ctx->bad(2, "A is NULL: rows must be the plan's m");
  if (!out) return ctx->bad(5, "out is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t B = (size_t)p->B, nA = sizeof(double) * B * rows * p->n, nO = sizeof(double) * B * rows;
  if (p->r_out.bytes < nO)                            // staging grows on demand
    if (int rc_ = alloc_all(ctx, {{&p->r_out, nO, "hipMalloc(row form output)"}})) return rc_;
  if (A && p->r_A.bytes < nA)
    if (int rc_ = alloc_all(ctx, {{&p->r_A, nA, "hipMalloc(row form input)"}})) return rc_;
  if (scale && !p->r_scale.p)
    if (int rc_ = alloc_all(ctx, {{&p->r_scale, sizeof(double) * B, "hipMalloc(row form scale)"}})) return rc_;
  if (A) HIPCHK(ctx, hipMemcpyAsync(p->r_A.p, A, nA, hipMemcpyHostToDevice, ctx->stream));
  if (scale) HIPCHK(ctx, hipMemcpyAsync(p->r_scale.p, scale, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  if (int rc_ = cov_rows_core(p, rows, A ? p->r_A.as<double>() : p->in_J.as<double>(),
                              scale ? p->r_scale.as<double>() : nullptr, p->r_out.as<double>()))
    return rc_;
  HIPCHK(ctx, hipMemcpyAsync(out, p->r_out.p, nO, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

namespace blsq_host {
int cov_pinv_to_host(blsq_cov_plan* p, const double* dJ, const long long* dmask, int lda, const double* dscale,
                     double* cov, int32_t* rank, double* rcond, double* kept_rcond, int32_t* status) {
  if (int rc_ = cov_pinv_outputs(p)) return rc_;
  if (int rc_ = cov_pinv_core(p, dJ, dmask, lda, dscale, p->o_cov.as<double>(), p->o_rank.as<int>(),
                              p->o_rcond.as<double>(), p->o_kept.as<double>(), p->o_status.as<int>()))
    return rc_;
  return cov_pinv_download(p, cov, rank, rcond, kept_rcond, status);
}

// blsq_outer_covariance (blsq_outer.hip) on the driver's resident J: mask (device, int64 [B][lda]) or nullptr
int cov_to_host(blsq_cov_plan* p, const double* dJ, const long long* dmask, int lda, double* cov, double* rcond,
                int32_t* status) {
  if (int rc_ = cov_outputs(p)) return rc_;
  if (int rc_ = cov_core(p, dJ, dmask, lda, p->o_cov.as<double>(), p->o_rcond.as<double>(), p->o_status.as<int>()))
    return rc_;
  return cov_download(p, cov, rcond, status);
}
}  // namespace blsq_host
