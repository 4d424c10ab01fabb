// C-ABI entry points (include/blsq.h): the batched, device-resident outer drivers and the finite-difference Jacobians.
#include "blsq_host.h"

#include <cmath>

// ==================================================== batched outer drivers ===
struct blsq_outer {
  blsq_outer() = default;
  blsq_outer(const blsq_outer&) = delete;
  blsq_outer& operator=(const blsq_outer&) = delete;
  ~blsq_outer() {                      // the driver owns its plans (each destroy synchronises the stream first)
    if (trf) blsq_trf_plan_destroy(trf);
    if (dog) blsq_dogbox_plan_destroy(dog);
    if (cov) blsq_cov_plan_destroy(cov);
  }
  blsq_ctx* ctx = nullptr;
  int method = 0, B = 0, m = 0, n = 0, ld = 0;
  blsq_trf_plan* trf = nullptr;
  blsq_dogbox_plan* dog = nullptr;
  DevBuf x0, xc, xt, f, ft, J, dvec, ivec, counts;
  DevBuf fsc, lobj, fscale;            // robust loss only: scaled f [B][m], objective [B], f_scale [B]
  int loss = BLSQ_LOSS_LINEAR;
  blsq_cov_plan* cov = nullptr;        // blsq_outer_covariance: created on first use
  DevBuf covmask;                      // [B][n] int64: the active mask of a 'trf' driver (from x, as the host reports it)
  DevBuf covscale;                     // [B] obj / (m - n): blsq_outer_covariance_pinv with variance_scale
  DevBuf covnobs;                      // [B] int: the points each problem kept (blsq_outer_covariance_pinv_nobs)
  bool scaled_early = false;           // robust loss: the accepted problems' J were scaled by blsq_outer_covariance
  bool cov_fresh = false;              // the covariance plan's factor is that of the resident J (blsq_outer_leverage);
                                       // cleared by start, begin, propose and judge
  DevBuf lev;                          // [B][m] leverages
  OuterState st{};
  int jac_scaling = 0;
  double xtol = 0.0;
  bool started = false, begun = false;
  int last_accepted = 0;
};

extern "C" int blsq_outer_create(blsq_ctx* ctx, int method, int B, int m, int n,
                                 blsq_outer** out) {
  if (!ctx) return -1;
  if (!out) return ctx->bad(6, "out is NULL");
  *out = nullptr;
  if (method != 0 && method != 1) return ctx->bad(2, "method must be 0 (trf) or 1 (dogbox)");
  blsq_outer* o = new blsq_outer();
  o->ctx = ctx; o->method = method; o->B = B; o->m = m; o->n = n;
  int rc = (method == 0) ? blsq_trf_plan_create(ctx, B, m, n, &o->trf)
                         : blsq_dogbox_plan_create(ctx, B, m, n, &o->dog);
  if (rc) { delete o; return rc; }
  StepPlan* sp = (method == 0) ? static_cast<StepPlan*>(o->trf) : o->dog;
  o->ld = sp->ld;
  const size_t vn = sizeof(double) * (size_t)B * n, vm = sizeof(double) * (size_t)B * m;
  hipError_t e = hipSuccess;
  auto al = [&](DevBuf& b, size_t bytes) { if (e == hipSuccess) e = b.alloc(bytes); };
  al(o->x0, vn); al(o->xc, vn); al(o->xt, vn); al(o->f, vm); al(o->ft, vm);
  al(o->J, vm * n); al(o->dvec, sizeof(double) * (size_t)B * 5);
  al(o->ivec, sizeof(int) * (size_t)B * 8); al(o->counts, sizeof(int) * 2);
  if (e != hipSuccess) { blsq_outer_destroy(o); return ctx->fail(e, "hipMalloc(outer driver)"); }
  OuterState& st = o->st;
  st.B = B; st.m = m; st.n = n; st.ld = o->ld; st.method = method;
  st.x = sp->vec(0); st.lb = sp->vec(1); st.ub = sp->vec(2); st.scale = sp->scale();
  st.o_scal = sp->o_scal.as<double>(); st.o_info = sp->o_info.as<int>();
  if (method == 0) {
    blsq_trf_plan* p = o->trf;
    st.g_norm_fac = p->st.g_norm; st.v = p->st.v; st.ncols = nullptr; st.on_bound = nullptr;
    st.o_step = p->out.step; st.o_xnew = p->out.x_new; st.o_onb = nullptr;
  } else {
    blsq_dogbox_plan* p = o->dog;
    st.g_norm_fac = p->st.g_norm; st.v = nullptr; st.ncols = p->st.ncols; st.on_bound = p->st.on_bound;
    st.o_step = p->out.step; st.o_xnew = p->out.x_new; st.o_onb = p->out.on_bound_new;
  }
  st.x0 = o->x0.as<double>(); st.xc = o->xc.as<double>(); st.xt = o->xt.as<double>();
  st.f = o->f.as<double>(); st.ft = o->ft.as<double>();
  double* dv = o->dvec.as<double>();
  st.Delta = dv; st.alpha = dv + B; st.obj = dv + 2 * (size_t)B; st.gnorm = dv + 3 * (size_t)B;
  st.actual = dv + 4 * (size_t)B;
  int* iv = o->ivec.as<int>();
  st.nfev = iv; st.njev = iv + B; st.pending = iv + 2 * (size_t)B; st.result = iv + 3 * (size_t)B;
  st.done = iv + 4 * (size_t)B; st.at_top = iv + 5 * (size_t)B; st.accepted = iv + 6 * (size_t)B;
  st.ncols_fac = iv + 7 * (size_t)B;
  st.counts = o->counts.as<int>();
  *out = o;
  return 0;
}

extern "C" int blsq_outer_destroy(blsq_outer* o) {
  if (!o) return 0;
  hipStreamSynchronize(o->ctx->stream);
  delete o;
  return 0;
}

extern "C" int blsq_outer_buffers(blsq_outer* o, double** x, double** x_trial, double** f,
                                  double** f_trial, double** J, int32_t** accepted) {
  if (!o) return -1;
  if (x) *x = o->st.xc;
  if (x_trial) *x_trial = o->st.xt;
  if (f) *f = o->st.f;
  if (f_trial) *f_trial = o->st.ft;
  if (J) *J = o->J.as<double>();
  if (accepted) *accepted = o->st.accepted;
  return 0;
}

extern "C" int blsq_outer_start(blsq_outer* o, const double* x0, const double* x_start,
                                const double* lb, const double* ub, const double* scale,
                                int jac_scaling, double ftol, double xtol, double gtol,
                                int max_nfev) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!x0) return ctx->bad(2, "x0 is NULL");
  if (!x_start) return ctx->bad(3, "x_start is NULL");
  if (!lb || !ub) return ctx->bad(4, "lb/ub is NULL");
  if (!scale) return ctx->bad(6, "scale is NULL");
  if (max_nfev <= 0) return ctx->bad(11, "max_nfev must be positive");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int B = o->B, n = o->n, ld = o->ld;
  OuterState& st = o->st;
  int rc;
  if ((rc = put_vec(ctx, st.x, ld, x_start, n, B, hipMemcpyHostToDevice))) return rc;
  if ((rc = put_vec(ctx, st.lb, ld, lb, n, B, hipMemcpyHostToDevice))) return rc;
  if ((rc = put_vec(ctx, st.ub, ld, ub, n, B, hipMemcpyHostToDevice))) return rc;
  if ((rc = put_vec(ctx, st.scale, ld, scale, n, B, hipMemcpyHostToDevice))) return rc;
  const size_t vn = sizeof(double) * (size_t)B * n;
  HIPCHK(ctx, hipMemcpyAsync(st.x0, x0, vn, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.xc, x_start, vn, hipMemcpyHostToDevice, ctx->stream));
  if (o->method == 1) {
    // on_bound_0 from x0 == lb / ub exactly (dogbox.py:152-154)
    std::vector<long long> ob((size_t)B * n);
    for (size_t i = 0; i < ob.size(); ++i) ob[i] = (x0[i] == lb[i]) ? -1 : ((x0[i] == ub[i]) ? 1 : 0);
    HIPCHK(ctx, hipMemcpy2DAsync(st.on_bound, sizeof(long long) * ld, ob.data(),
                                 sizeof(long long) * n, sizeof(long long) * n, B,
                                 hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  st.ftol = ftol; st.xtol = xtol; st.gtol = gtol; st.max_nfev = max_nfev;
  o->xtol = xtol; o->jac_scaling = jac_scaling ? 1 : 0;
  o->started = true; o->begun = false; o->last_accepted = 0; o->scaled_early = false; o->cov_fresh = false;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int blsq_outer_set_loss(blsq_outer* o, int loss, const double* f_scale) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (o->started) return ctx->bad(1, "blsq_outer_set_loss must be called before blsq_outer_start");
  if (loss < BLSQ_LOSS_LINEAR || loss > BLSQ_LOSS_ARCTAN) return ctx->bad(2, "loss must be one of BLSQ_LOSS_*");
  if (loss == BLSQ_LOSS_LINEAR) {
    o->loss = loss;
    o->st.lobj = nullptr;
    return 0;
  }
  if (!f_scale) return ctx->bad(3, "f_scale is NULL");
  for (int b = 0; b < o->B; ++b)
    if (!(f_scale[b] > 0.0) || !std::isfinite(f_scale[b])) return ctx->bad(3, "f_scale must be positive and finite");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t vm = sizeof(double) * (size_t)o->B * o->m, vb = sizeof(double) * (size_t)o->B;
  hipError_t e = hipSuccess;
  if (!o->fsc.p) e = o->fsc.alloc(vm);
  if (e == hipSuccess && !o->lobj.p) e = o->lobj.alloc(vb);
  if (e == hipSuccess && !o->fscale.p) e = o->fscale.alloc(vb);
  if (e != hipSuccess) return ctx->fail(e, "hipMalloc(outer driver loss)");
  HIPCHK(ctx, hipMemcpyAsync(o->fscale.p, f_scale, vb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  o->loss = loss;
  o->st.lobj = o->lobj.as<double>();
  return 0;
}

namespace blsq_host {
// robust loss: J <- diag(w) J and the scaled f of the problems selected by `mask` (nullptr: all)
static int outer_loss_scale(blsq_outer* o, const int* mask) {
  blsq_ctx* ctx = o->ctx;
  return ctx->run(K_LOSS_SCALE, "launch_loss_scale", [&] {
    return launch_loss_scale(o->B, o->m, o->n, o->loss, o->fscale.as<double>(), o->st.f, o->J.as<double>(),
                             o->fsc.as<double>(), mask, ctx->stream);
  });
}
// robust loss: the objective of every problem at `f` into st.lobj
static int outer_loss_cost(blsq_outer* o, const double* f) {
  blsq_ctx* ctx = o->ctx;
  return ctx->run(K_LOSS_COST, "launch_loss_cost", [&] {
    return launch_loss_cost(o->B, o->m, o->loss, o->fscale.as<double>(), f, o->lobj.as<double>(), nullptr, ctx->stream);
  });
}
// factor the problems selected by `mask` (nullptr: all) from the driver's J / f buffers (the scaled f with a loss)
int outer_factor(blsq_outer* o, int scale_mode, const int* mask) {
  const double* f = (o->loss != BLSQ_LOSS_LINEAR) ? o->fsc.as<double>() : o->st.f;
  if (o->method == 0) {
    blsq_trf_plan* p = o->trf;
    return trf_factor_core(p, o->J.as<double>(), f, p->n, scale_mode, mask);
  }
  blsq_dogbox_plan* p = o->dog;
  return dog_factor_core(p, o->J.as<double>(), f, p->n, scale_mode, mask);
}
}  // namespace blsq_host

extern "C" int blsq_outer_begin(blsq_outer* o) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->started) return ctx->bad(1, "blsq_outer_start has not been called");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  o->cov_fresh = false;
  int rc;
  if (o->loss != BLSQ_LOSS_LINEAR) {     // every J is fresh
    if ((rc = outer_loss_scale(o, nullptr))) return rc;
    if ((rc = outer_loss_cost(o, o->st.f))) return rc;
  }
  rc = outer_factor(o, o->jac_scaling ? BLSQ_SCALE_JAC_INIT : BLSQ_SCALE_GIVEN, nullptr);
  if (rc) return rc;
  hipError_t e = launch_outer_begin(o->st, ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_outer_begin");
  o->begun = true; o->last_accepted = 0;
  return 0;
}

extern "C" int blsq_outer_propose(blsq_outer* o, int32_t* n_active) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->begun) return ctx->bad(1, "blsq_outer_begin has not been called");
  if (!n_active) return ctx->bad(2, "n_active is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  o->cov_fresh = false;
  int rc;
  if (o->last_accepted > 0) {            // fresh Jacobians: factor those problems only
    if (o->loss != BLSQ_LOSS_LINEAR && !o->scaled_early && (rc = outer_loss_scale(o, o->st.accepted))) return rc;
    o->scaled_early = false;
    rc = outer_factor(o, o->jac_scaling ? BLSQ_SCALE_JAC_UPDATE : BLSQ_SCALE_GIVEN,
                      o->st.ncols_fac);
    if (rc) return rc;
    o->last_accepted = 0;
  }
  hipError_t e = launch_outer_top(o->st, ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_outer_top");
  rc = (o->method == 0) ? blsq_trf_step_dev(o->trf, o->st.Delta, o->st.alpha, o->xtol)
                        : blsq_dogbox_step_dev(o->dog, o->st.Delta);
  if (rc) return rc;
  HIPCHK(ctx, hipMemsetAsync(o->st.counts, 0, sizeof(int) * 2, ctx->stream));
  e = launch_outer_trial(o->st, ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_outer_trial");
  const int* c = nullptr;
  HIPCHK(ctx, ctx->read_blocking(PIN_OUTER, o->st.counts, 1, &c));
  *n_active = c[0];
  return 0;
}

extern "C" int blsq_outer_judge(blsq_outer* o, int32_t* n_accepted) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->begun) return ctx->bad(1, "blsq_outer_begin has not been called");
  if (!n_accepted) return ctx->bad(2, "n_accepted is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  o->cov_fresh = false;
  int rc;
  if (o->loss != BLSQ_LOSS_LINEAR && (rc = outer_loss_cost(o, o->st.ft))) return rc;
  hipError_t e = launch_outer_judge(o->st, ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_outer_judge");
  const int* c = nullptr;
  HIPCHK(ctx, ctx->read_blocking(PIN_OUTER, o->st.counts + 1, 1, &c));
  *n_accepted = c[0];
  o->last_accepted = c[0];
  return 0;
}

extern "C" int blsq_outer_fetch(blsq_outer* o, double* x, double* f, double* obj,
                                double* optimality, int64_t* on_bound, int32_t* nfev,
                                int32_t* njev, int32_t* status) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int B = o->B, n = o->n, m = o->m, ld = o->ld;
  const OuterState& st = o->st;
  auto d2h = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!dst) return 0;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
  };
  int rc;
  if ((rc = d2h(x, st.xc, sizeof(double) * (size_t)B * n))) return rc;
  if ((rc = d2h(f, st.f, sizeof(double) * (size_t)B * m))) return rc;
  if ((rc = d2h(obj, st.obj, sizeof(double) * B))) return rc;
  if ((rc = d2h(optimality, st.gnorm, sizeof(double) * B))) return rc;
  if ((rc = d2h(nfev, st.nfev, sizeof(int) * B))) return rc;
  if ((rc = d2h(njev, st.njev, sizeof(int) * B))) return rc;
  if ((rc = d2h(status, st.result, sizeof(int) * B))) return rc;
  if (on_bound) {
    if (o->method == 1) {
      HIPCHK(ctx, hipMemcpy2DAsync(on_bound, sizeof(long long) * n, st.on_bound,
                                   sizeof(long long) * ld, sizeof(long long) * n, B,
                                   hipMemcpyDeviceToHost, ctx->stream));
    } else {
      memset(on_bound, 0, sizeof(int64_t) * (size_t)B * n);
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// Covariance of every problem from the driver's resident J.  Under a robust loss J must hold diag(w) J for EVERY
// problem: blsq_outer_propose scales the Jacobians a judge has just accepted before it factors them, so between a
// judge and the next propose those are still unscaled — they are scaled here, once (propose then leaves them alone).
// The mask of free_only: dogbox's on_bound; for 'trf' find_active_constraints(x, lb, ub, rtol = xtol) (trf.py:257), the
// mask the host reports for the x blsq_outer_fetch returns.
namespace {
// what both covariance calls do first: pending verdicts, the plan, the early scaling, the mask of free_only
int outer_cov_prepare(blsq_outer* o, int free_only, const long long** mask, int* lda) {
  blsq_ctx* ctx = o->ctx;
  int rc;
  if ((rc = ctx_resolve_pending(ctx))) return rc;
  if (!o->cov && (rc = blsq_cov_plan_create(ctx, o->B, o->m, o->n, &o->cov))) return rc;
  if (o->loss != BLSQ_LOSS_LINEAR && o->last_accepted > 0 && !o->scaled_early) {
    if ((rc = outer_loss_scale(o, o->st.accepted))) return rc;
    o->scaled_early = true;
  }
  *mask = nullptr;
  *lda = o->n;
  if (free_only) {
    if (o->method == 1) { *mask = reinterpret_cast<const long long*>(o->st.on_bound); *lda = o->ld; }
    else {
      if (!o->covmask.p)
        if ((rc = alloc_all(ctx, {{&o->covmask, sizeof(long long) * (size_t)o->B * o->n, "hipMalloc(trf mask)"}})))
          return rc;
      const hipError_t e = launch_cov_trf_mask(o->B, o->n, o->ld, o->xtol, o->st.xc, o->st.lb, o->st.ub,
                                               o->covmask.as<long long>(), ctx->stream);
      if (e != hipSuccess) return ctx->fail(e, "launch_cov_trf_mask");
      *mask = o->covmask.as<long long>();
    }
  }
  return 0;
}
}  // namespace

extern "C" int blsq_outer_covariance(blsq_outer* o, int free_only, double* cov, double* rcond, int32_t* status) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->begun) return ctx->bad(1, "blsq_outer_begin has not been called");
  if (!cov) return ctx->bad(3, "cov is NULL");
  if (!rcond) return ctx->bad(4, "rcond is NULL");
  if (!status) return ctx->bad(5, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const long long* mask = nullptr;
  int lda = o->n;
  o->cov_fresh = false;
  if (int rc = outer_cov_prepare(o, free_only, &mask, &lda)) return rc;
  if (int rc = cov_to_host(o->cov, o->J.as<double>(), mask, lda, cov, rcond, status)) return rc;
  o->cov_fresh = true;
  return 0;
}

// The pseudo-inverse covariance of every problem (blsq_cov_pinv_dev on the resident J, same rules as above);
// variance_scale: times obj[b] / (m - n) of the resident objective, applied by the product kernel.
extern "C" int blsq_outer_covariance_pinv(blsq_outer* o, int free_only, int variance_scale, double* cov, int32_t* rank,
                                          double* rcond, double* kept_rcond, int32_t* status) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->begun) return ctx->bad(1, "blsq_outer_begin has not been called");
  if (variance_scale && o->m <= o->n) return ctx->bad(3, "variance_scale needs m > n");
  if (!cov) return ctx->bad(4, "cov is NULL");
  if (!rank) return ctx->bad(5, "rank is NULL");
  if (!rcond) return ctx->bad(6, "rcond is NULL");
  if (!kept_rcond) return ctx->bad(7, "kept_rcond is NULL");
  if (!status) return ctx->bad(8, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const long long* mask = nullptr;
  int lda = o->n;
  o->cov_fresh = false;
  if (int rc = outer_cov_prepare(o, free_only, &mask, &lda)) return rc;
  const double* dscale = nullptr;
  if (variance_scale) {
    if (!o->covscale.p)
      if (int rc = alloc_all(ctx, {{&o->covscale, sizeof(double) * (size_t)o->B, "hipMalloc(variance scale)"}}))
        return rc;
    const hipError_t e = launch_cov_variance(o->B, o->m, o->n, o->st.obj, o->covscale.as<double>(), ctx->stream);
    if (e != hipSuccess) return ctx->fail(e, "launch_cov_variance");
    dscale = o->covscale.as<double>();
  }
  if (int rc = cov_pinv_to_host(o->cov, o->J.as<double>(), mask, lda, dscale, cov, rank, rcond, kept_rcond, status))
    return rc;
  o->cov_fresh = true;
  return 0;
}

// blsq_outer_covariance_pinv with the variance factor obj[b] / (nobs[b] - n) of every problem: the counts
// are uploaded once, the sibling of the variance kernel turns them into the scale the product kernel applies.
extern "C" int blsq_outer_covariance_pinv_nobs(blsq_outer* o, int free_only, const int32_t* nobs, double* cov,
                                               int32_t* rank, double* rcond, double* kept_rcond, int32_t* status) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->begun) return ctx->bad(1, "blsq_outer_begin has not been called");
  if (!nobs) return ctx->bad(3, "nobs is NULL");
  for (int b = 0; b < o->B; ++b)
    if (nobs[b] < 0 || nobs[b] > o->m) return ctx->bad(3, "nobs entry outside 0 .. m");
  if (!cov) return ctx->bad(4, "cov is NULL");
  if (!rank) return ctx->bad(5, "rank is NULL");
  if (!rcond) return ctx->bad(6, "rcond is NULL");
  if (!kept_rcond) return ctx->bad(7, "kept_rcond is NULL");
  if (!status) return ctx->bad(8, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const long long* mask = nullptr;
  int lda = o->n;
  o->cov_fresh = false;
  if (int rc = outer_cov_prepare(o, free_only, &mask, &lda)) return rc;
  if (!o->covscale.p)
    if (int rc = alloc_all(ctx, {{&o->covscale, sizeof(double) * (size_t)o->B, "hipMalloc(variance scale)"}}))
      return rc;
  if (!o->covnobs.p)
    if (int rc = alloc_all(ctx, {{&o->covnobs, sizeof(int) * (size_t)o->B, "hipMalloc(nobs)"}})) return rc;
  // (pageable source: the copy has left `nobs` when the call returns)
  HIPCHK(ctx, hipMemcpyAsync(o->covnobs.p, nobs, sizeof(int) * (size_t)o->B, hipMemcpyHostToDevice, ctx->stream));
  const hipError_t e = launch_cov_variance_nobs(o->B, o->n, o->st.obj, o->covnobs.as<int>(), o->covscale.as<double>(),
                                                ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_cov_variance_nobs");
  if (int rc = cov_pinv_to_host(o->cov, o->J.as<double>(), mask, lda, o->covscale.as<double>(), cov, rank, rcond,
                                kept_rcond, status))
    return rc;
  o->cov_fresh = true;
  return 0;
}

// Leverages h_i = (J C J^T)_ii of the resident J through the factor the driver's last covariance call left in its
// plan (blsq_cov_rows_dev).  A missing or stale factor is an error: nothing is recomputed silently.
extern "C" int blsq_outer_leverage(blsq_outer* o, double* h, int32_t* status) {
  if (!o) return -1;
  blsq_ctx* ctx = o->ctx;
  if (!o->cov_fresh || !o->cov)
    return ctx->bad(1, "no current covariance factor: call blsq_outer_covariance / _pinv after the last begin / propose / judge");
  if (!h) return ctx->bad(2, "h is NULL");
  if (!status) return ctx->bad(3, "status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nh = sizeof(double) * (size_t)o->B * o->m;
  if (!o->lev.p)
    if (int rc = alloc_all(ctx, {{&o->lev, nh, "hipMalloc(leverages)"}})) return rc;
  if (int rc = cov_rows_core(o->cov, o->m, o->J.as<double>(), nullptr, o->lev.as<double>())) return rc;
  HIPCHK(ctx, hipMemcpyAsync(h, o->lev.p, nh, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(status, o->cov->kept_status.p, sizeof(int) * (size_t)o->B, hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// ================================================== robust loss functions ===
extern "C" int blsq_loss_cost_dev(blsq_ctx* ctx, int B, int m, int loss, const double* df_scale, const double* df,
                                  double* dobj, const int32_t* dmask) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (loss < BLSQ_LOSS_LINEAR || loss > BLSQ_LOSS_ARCTAN) return ctx->bad(4, "loss must be one of BLSQ_LOSS_*");
  if (!df_scale) return ctx->bad(5, "f_scale is NULL");
  if (!df) return ctx->bad(6, "f is NULL");
  if (!dobj) return ctx->bad(7, "obj is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc_ = ctx->run(K_LOSS_COST, "launch_loss_cost", [&] {
        return launch_loss_cost(B, m, loss, df_scale, df, dobj, dmask, ctx->stream);
      })) return rc_;
  return 0;
}

extern "C" int blsq_loss_scale_dev(blsq_ctx* ctx, int B, int m, int n, int loss, const double* df_scale,
                                   const double* df, double* dJ_io, double* df_scaled, const int32_t* dmask) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n <= 0) return ctx->bad(4, "n must be positive");
  if (loss < BLSQ_LOSS_LINEAR || loss > BLSQ_LOSS_ARCTAN) return ctx->bad(5, "loss must be one of BLSQ_LOSS_*");
  if (!df_scale) return ctx->bad(6, "f_scale is NULL");
  if (!df) return ctx->bad(7, "f is NULL");
  if (!dJ_io) return ctx->bad(8, "J is NULL");
  if (!df_scaled) return ctx->bad(9, "f_scaled is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc_ = ctx->run(K_LOSS_SCALE, "launch_loss_scale", [&] {
        return launch_loss_scale(B, m, n, loss, df_scale, df, dJ_io, df_scaled, dmask, ctx->stream);
      })) return rc_;
  return 0;
}

// ============================================= finite-difference Jacobians ===
extern "C" int blsq_fd_points_dev(blsq_ctx* ctx, int B, int n, int method, const double* dx,
                                  const double* dlb, const double* dub, const double* drel_step,
                                  double* dX, double* dh, uint8_t* done_sided) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (n <= 0) return ctx->bad(3, "n must be positive");
  if (method != 2 && method != 3) return ctx->bad(4, "method must be 2 or 3");
  if (!dx || !dlb || !dub) return ctx->bad(5, "x/lb/ub is NULL");
  if (!dX || !dh || !done_sided) return ctx->bad(9, "output is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipError_t e = launch_fd_points(B, n, method, dx, dlb, dub, drel_step, dX, dh, done_sided,
                                  ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_fd_points");
  return 0;
}

extern "C" int blsq_fd_assemble_dev(blsq_ctx* ctx, int B, int m, int n, int method,
                                    const double* dx, const double* dh,
                                    const uint8_t* done_sided, const double* df0,
                                    const double* dF, double* dJ, const int32_t* dmask) {
  if (!ctx) return -1;
  if (B <= 0 || B > 65535) return ctx->bad(2, "B must be in 1..65535");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n <= 0) return ctx->bad(4, "n must be positive");
  if (method != 2 && method != 3) return ctx->bad(5, "method must be 2 or 3");
  if (!dx || !dh || !done_sided || !df0 || !dF) return ctx->bad(6, "input is NULL");
  if (!dJ) return ctx->bad(11, "J is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipError_t e = launch_fd_assemble(B, m, n, method, dx, dh, done_sided, df0, dF, dJ, dmask,
                                    ctx->stream);
  if (e != hipSuccess) return ctx->fail(e, "launch_fd_assemble");
  return 0;
}
