// Built-in fit models: the table behind blsq_model_count / blsq_model_info and the entry point blsq_model_eval_dev
// (include/blsq.h; kernel: model_kernels.hip), its mapped form blsq_model_eval_map_dev (7k), and the term
// table behind blsq_term_count / blsq_term_info with the composite entry blsq_model_eval_comp_dev (7l), and the entry
// that takes the estimator for all of them, blsq_model_eval_est_dev (7m), and the one that takes the sampling as well,
// blsq_model_eval_bin_dev (7n), and the one that takes the NaN policy too, blsq_model_eval_nan_dev (7o).
#include "blsq_host.h"

namespace {

struct ModelRow {
  const char* name;
  int coords;        // rows of t per data point
  int n_base;        // parameters besides the terms (the offset c; gauss2d: all five)
  int n_per_term;    // parameters per term (0: a fixed n = n_base)
};
// in the order of the BLSQ_MODEL_* enum
const ModelRow kModels[] = {
    {"poly", 1, 0, 1}, {"exp_sum", 1, 1, 2}, {"gauss_sum", 1, 1, 3}, {"lorentz_sum", 1, 1, 3}, {"gauss2d", 2, 5, 0}};
constexpr int kModelCount = (int)(sizeof(kModels) / sizeof(kModels[0]));
static_assert(kModelCount == BLSQ_MODEL_GAUSS2D + 1, "one row per BLSQ_MODEL_*");

bool model_n_fits(const ModelRow& r, int n) {
  if (n < 1 || n > BLSQ_MODEL_MAX_N) return false;
  if (r.n_per_term == 0) return n == r.n_base;
  return n > r.n_base && (n - r.n_base) % r.n_per_term == 0;
}

struct TermRow {
  const char* name;
  int n_per_term;
};
// in the order of the BLSQ_TERM_* enum
const TermRow kTerms[] = {{"gauss", 3}, {"lorentz", 3}, {"pvoigt", 4}, {"exp", 2}, {"poly", 1}};
constexpr int kTermCount = (int)(sizeof(kTerms) / sizeof(kTerms[0]));
static_assert(kTermCount == BLSQ_TERM_POLY + 1, "one row per BLSQ_TERM_*");

}  // namespace

extern "C" int blsq_model_count(void) { return kModelCount; }

extern "C" int blsq_model_info(int model, const char** name, int* coords, int* n_base, int* n_per_term) {
  if (model < 0 || model >= kModelCount) return -1;
  const ModelRow& r = kModels[model];
  if (name) *name = r.name;
  if (coords) *coords = r.coords;
  if (n_base) *n_base = r.n_base;
  if (n_per_term) *n_per_term = r.n_per_term;
  return 0;
}

extern "C" int blsq_model_eval_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, const double* dt,
                                   long t_stride, const double* dy, const double* dw, long w_stride, const double* dP,
                                   double* df, double* dJ, const int32_t* dmask) {
  if (!ctx) return -1;
  if (model < 0 || model >= kModelCount) return ctx->bad(2, "model must be one of BLSQ_MODEL_*");
  const ModelRow& r = kModels[model];
  if (B <= 0) return ctx->bad(3, "B must be positive");
  if (reps <= 0) return ctx->bad(4, "reps must be positive");
  if (m <= 0) return ctx->bad(5, "m must be positive");
  if (!model_n_fits(r, n)) return ctx->bad(6, "n does not fit the model (or exceeds BLSQ_MODEL_MAX_N)");
  if (!dt) return ctx->bad(7, "t is NULL");
  if (t_stride != 0 && t_stride != (long)r.coords * m) return ctx->bad(8, "t_stride must be 0 or coords * m");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(11, "w_stride must be 0 or m");
  if (!dP) return ctx->bad(12, "P is NULL");
  if (!df && !dJ) return ctx->bad(13, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(14, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->run(K_MODEL_EVAL, "launch_model_eval", [&] {
    return launch_model_eval(model, B, reps, m, n, dt, t_stride, dy, dw, w_stride, dP, df, dJ, dmask, ctx->stream);
  });
}

extern "C" int blsq_model_eval_map_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, int nf,
                                       const int32_t* pmap, const double* dt, long t_stride, const double* dy,
                                       const double* dw, long w_stride, const double* dX, const double* dPfix,
                                       double* df, double* dJ, const int32_t* dmask) {
  if (!ctx) return -1;
  if (model < 0 || model >= kModelCount) return ctx->bad(2, "model must be one of BLSQ_MODEL_*");
  const ModelRow& r = kModels[model];
  if (B <= 0) return ctx->bad(3, "B must be positive");
  if (reps <= 0) return ctx->bad(4, "reps must be positive");
  if (m <= 0) return ctx->bad(5, "m must be positive");
  if (!model_n_fits(r, n)) return ctx->bad(6, "n does not fit the model (or exceeds BLSQ_MODEL_MAX_N)");
  if (nf < 1 || nf > n) return ctx->bad(7, "nf must be in 1 .. n");
  if (!pmap) return ctx->bad(8, "pmap is NULL");
  bool used[BLSQ_MODEL_MAX_N] = {};
  bool any_fixed = false;
  for (int j = 0; j < n; ++j) {
    if (pmap[j] < -1 || pmap[j] >= nf) return ctx->bad(19, "pmap entry outside -1 .. nf - 1");
    if (pmap[j] < 0) any_fixed = true;
    else used[pmap[j]] = true;
  }
  for (int k = 0; k < nf; ++k)
    if (!used[k]) return ctx->bad(20, "pmap leaves a variable k < nf unused");
  if (!dt) return ctx->bad(9, "t is NULL");
  if (t_stride != 0 && t_stride != (long)r.coords * m) return ctx->bad(10, "t_stride must be 0 or coords * m");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(13, "w_stride must be 0 or m");
  if (!dX) return ctx->bad(14, "X is NULL");
  if (any_fixed && !dPfix) return ctx->bad(15, "Pfix is NULL although pmap holds a parameter fixed");
  if (!df && !dJ) return ctx->bad(16, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(17, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->run(K_MODEL_EVAL, "launch_model_eval_map", [&] {
    return launch_model_eval_map(model, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ,
                                 dmask, ctx->stream);
  });
}

extern "C" int blsq_term_count(void) { return kTermCount; }

extern "C" int blsq_term_info(int term, const char** name, int* n_per_term) {
  if (term < 0 || term >= kTermCount) return -1;
  if (name) *name = kTerms[term].name;
  if (n_per_term) *n_per_term = kTerms[term].n_per_term;
  return 0;
}

extern "C" int blsq_model_eval_comp_dev(blsq_ctx* ctx, int ncomp, const int32_t* fam, const int32_t* cnt, int B,
                                        int reps, int m, int n, int nf, const int32_t* pmap, const double* dt,
                                        long t_stride, const double* dy, const double* dw, long w_stride,
                                        const double* dX, const double* dPfix, double* df, double* dJ,
                                        const int32_t* dmask) {
  if (!ctx) return -1;
  if (ncomp < 1 || ncomp > BLSQ_MODEL_MAX_COMP) return ctx->bad(2, "ncomp must be in 1 .. BLSQ_MODEL_MAX_COMP");
  if (!fam) return ctx->bad(3, "fam is NULL");
  if (!cnt) return ctx->bad(4, "cnt is NULL");
  long total = 0;
  for (int c = 0; c < ncomp; ++c) {
    if (fam[c] < 0 || fam[c] >= kTermCount) return ctx->bad(3, "fam entry must be one of BLSQ_TERM_*");
    if (cnt[c] < 1) return ctx->bad(4, "cnt entry must be at least 1");
    total += (long)cnt[c] * kTerms[fam[c]].n_per_term;
  }
  if (B <= 0) return ctx->bad(5, "B must be positive");
  if (reps <= 0) return ctx->bad(6, "reps must be positive");
  if (m <= 0) return ctx->bad(7, "m must be positive");
  if (n < 1 || n > BLSQ_MODEL_MAX_N || total != n)
    return ctx->bad(8, "n must be the parameters of the components together (and at most BLSQ_MODEL_MAX_N)");
  bool any_fixed = false;
  if (!pmap) {
    if (nf != n) return ctx->bad(9, "nf must equal n without a pmap");
  } else {
    if (nf < 1 || nf > n) return ctx->bad(9, "nf must be in 1 .. n");
    bool used[BLSQ_MODEL_MAX_N] = {};
    for (int j = 0; j < n; ++j) {
      if (pmap[j] < -1 || pmap[j] >= nf) return ctx->bad(21, "pmap entry outside -1 .. nf - 1");
      if (pmap[j] < 0) any_fixed = true;
      else used[pmap[j]] = true;
    }
    for (int k = 0; k < nf; ++k)
      if (!used[k]) return ctx->bad(22, "pmap leaves a variable k < nf unused");
  }
  if (!dt) return ctx->bad(11, "t is NULL");
  if (t_stride != 0 && t_stride != (long)m) return ctx->bad(12, "t_stride must be 0 or m");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(15, "w_stride must be 0 or m");
  if (!dX) return ctx->bad(16, "X is NULL");
  if (any_fixed && !dPfix) return ctx->bad(17, "Pfix is NULL although pmap holds a parameter fixed");
  if (!df && !dJ) return ctx->bad(18, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(19, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->run(K_MODEL_EVAL, "launch_model_eval_comp", [&] {
    return launch_model_eval_comp(ncomp, fam, cnt, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix,
                                  df, dJ, dmask, ctx->stream);
  });
}

// One entry for every instance, with the estimator and the sampling (7n): the checks of the three entries
// above, then the launch of the entry it stands in for.  blsq_model_eval_est_dev numbers its arguments from est = 2,
// model = 3; blsq_model_eval_bin_dev has `sampling` in between, so every later argument is one further on (sh = 1);
// blsq_model_eval_nan_dev has `nan_policy` after that (sh = 2).
static int model_eval_checked(blsq_ctx* ctx, const char* what, int sh, int est, int sampling, int nan_policy, int model,
                              int ncomp,
                              const int32_t* fam, const int32_t* cnt, int B, int reps, int m, int n, int nf,
                              const int32_t* pmap, const double* dt, long t_stride, const double* dy, const double* dw,
                              long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                              const int32_t* dmask) {
  if (!ctx) return -1;
  if (est != BLSQ_EST_LSE && est != BLSQ_EST_POISSON) return ctx->bad(2, "est must be one of BLSQ_EST_*");
  if (sampling != BLSQ_SAMPLE_POINT && sampling != BLSQ_SAMPLE_BIN)
    return ctx->bad(3, "sampling must be one of BLSQ_SAMPLE_*");
  if (nan_policy != BLSQ_NAN_PROPAGATE && nan_policy != BLSQ_NAN_OMIT)
    return ctx->bad(4, "nan_policy must be one of BLSQ_NAN_*");
  if (model < -1 || model >= kModelCount)
    return ctx->bad(3 + sh, "model must be one of BLSQ_MODEL_*, or -1 for a composite");
  const bool comp = model < 0;
  long total = 0;
  if (!comp) {
    if (ncomp != 0) return ctx->bad(4 + sh, "ncomp must be 0 with a named model");
  } else {
    if (ncomp < 1 || ncomp > BLSQ_MODEL_MAX_COMP) return ctx->bad(4 + sh, "ncomp must be in 1 .. BLSQ_MODEL_MAX_COMP");
    if (!fam) return ctx->bad(5 + sh, "fam is NULL");
    if (!cnt) return ctx->bad(6 + sh, "cnt is NULL");
    for (int c = 0; c < ncomp; ++c) {
      if (fam[c] < 0 || fam[c] >= kTermCount) return ctx->bad(5 + sh, "fam entry must be one of BLSQ_TERM_*");
      if (cnt[c] < 1) return ctx->bad(6 + sh, "cnt entry must be at least 1");
      total += (long)cnt[c] * kTerms[fam[c]].n_per_term;
    }
  }
  if (B <= 0) return ctx->bad(7 + sh, "B must be positive");
  if (reps <= 0) return ctx->bad(8 + sh, "reps must be positive");
  if (m <= 0) return ctx->bad(9 + sh, "m must be positive");
  if (comp) {
    if (n < 1 || n > BLSQ_MODEL_MAX_N || total != n)
      return ctx->bad(10 + sh, "n must be the parameters of the components together (and at most BLSQ_MODEL_MAX_N)");
  } else if (!model_n_fits(kModels[model], n)) {
    return ctx->bad(10 + sh, "n does not fit the model (or exceeds BLSQ_MODEL_MAX_N)");
  }
  bool any_fixed = false;
  if (!pmap) {
    if (nf != n) return ctx->bad(11 + sh, "nf must equal n without a pmap");
  } else {
    if (nf < 1 || nf > n) return ctx->bad(11 + sh, "nf must be in 1 .. n");
    bool used[BLSQ_MODEL_MAX_N] = {};
    for (int j = 0; j < n; ++j) {
      if (pmap[j] < -1 || pmap[j] >= nf) return ctx->bad(23 + sh, "pmap entry outside -1 .. nf - 1");
      if (pmap[j] < 0) any_fixed = true;
      else used[pmap[j]] = true;
    }
    for (int k = 0; k < nf; ++k)
      if (!used[k]) return ctx->bad(24 + sh, "pmap leaves a variable k < nf unused");
  }
  const long coords = comp ? 1 : kModels[model].coords;
  if (!dt) return ctx->bad(13 + sh, "t is NULL");
  if (sampling == BLSQ_SAMPLE_BIN) {
    if (t_stride != 0 && t_stride != 2 * coords * m)
      return ctx->bad(14 + sh, "t_stride must be 0 or 2 * coords * m with BLSQ_SAMPLE_BIN");
  } else if (t_stride != 0 && t_stride != coords * m) {
    return ctx->bad(14 + sh, "t_stride must be 0 or coords * m");
  }
  if (est == BLSQ_EST_POISSON && !dy) return ctx->bad(15 + sh, "y is NULL: the Poisson estimator needs the counts");
  if (nan_policy == BLSQ_NAN_OMIT && !dy)
    return ctx->bad(15 + sh, "y is NULL: BLSQ_NAN_OMIT reads the missing points from it");
  if (est == BLSQ_EST_POISSON && dw) return ctx->bad(16 + sh, "w must be NULL with the Poisson estimator");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(17 + sh, "w_stride must be 0 or m");
  if (!dX) return ctx->bad(18 + sh, "X is NULL");
  if (any_fixed && !dPfix) return ctx->bad(19 + sh, "Pfix is NULL although pmap holds a parameter fixed");
  if (!df && !dJ) return ctx->bad(20 + sh, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(21 + sh, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->run(K_MODEL_EVAL, what, [&] {
    if (comp)
      return launch_model_eval_comp(ncomp, fam, cnt, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix,
                                    df, dJ, dmask, ctx->stream, est, sampling, nan_policy);
    if (pmap)
      return launch_model_eval_map(model, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ,
                                   dmask, ctx->stream, est, sampling, nan_policy);
    return launch_model_eval(model, B, reps, m, n, dt, t_stride, dy, dw, w_stride, dX, df, dJ, dmask, ctx->stream, est,
                             sampling, nan_policy);
  });
}

extern "C" int blsq_model_eval_est_dev(blsq_ctx* ctx, int est, int model, int ncomp, const int32_t* fam,
                                       const int32_t* cnt, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                                       const double* dt, long t_stride, const double* dy, const double* dw,
                                       long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                                       const int32_t* dmask) {
  return model_eval_checked(ctx, "launch_model_eval_est", 0, est, BLSQ_SAMPLE_POINT, BLSQ_NAN_PROPAGATE, model, ncomp,
                            fam, cnt, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask);
}

extern "C" int blsq_model_eval_bin_dev(blsq_ctx* ctx, int est, int sampling, int model, int ncomp, const int32_t* fam,
                                       const int32_t* cnt, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                                       const double* dt, long t_stride, const double* dy, const double* dw,
                                       long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                                       const int32_t* dmask) {
  return model_eval_checked(ctx, "launch_model_eval_bin", 1, est, sampling, BLSQ_NAN_PROPAGATE, model, ncomp, fam, cnt,
                            B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask);
}

extern "C" int blsq_model_eval_nan_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                                       const int32_t* fam, const int32_t* cnt, int B, int reps, int m, int n, int nf,
                                       const int32_t* pmap, const double* dt, long t_stride, const double* dy,
                                       const double* dw, long w_stride, const double* dX, const double* dPfix,
                                       double* df, double* dJ, const int32_t* dmask) {
  return model_eval_checked(ctx, "launch_model_eval_nan", 2, est, sampling, nan_policy, model, ncomp, fam, cnt, B, reps,
                            m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask);
}
