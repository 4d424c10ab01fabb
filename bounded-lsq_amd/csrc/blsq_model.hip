// Built-in fit models (include/blsq.h; kernel: model_kernels.hip): the model and term tables behind
// blsq_model_count / _info and blsq_term_count / _info, the entries blsq_linear_eval_dev, blsq_expr_check, blsq_expr_eval_dev, blsq_bvls_moments_dev, blsq_bvls_solve_dev, blsq_bvls_solve_eq_dev, blsq_response_apply_dev, blsq_varpro_expand_dev, blsq_varpro_reduce_dev, blsq_varpro_expand_global_dev, blsq_varpro_reduce_global_dev and blsq_varpro_cov_blocks_dev, and the eight entries blsq_model_eval_dev, _map_dev, _comp_dev,
// _est_dev, _bin_dev, _nan_dev, _global_dev and _tie_dev.  An entry fills a ModelEvalCall from its arguments (what its signature
// does not have is the default) and hands it to model_eval_checked with its EvalEntry: one list of checks, one launcher, and per entry
// only the argument numbers.
#include "blsq_host.h"

#include <cmath>

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

// in the order of the BLSQ_TERM_* enum; the parameters per term: MODEL_TERM_PARAMS (blsq_kernels.h)
const char* const kTermNames[] = {"gauss", "lorentz", "pvoigt", "exp", "poly"};
constexpr int kTermCount = (int)(sizeof(kTermNames) / sizeof(kTermNames[0]));
static_assert(kTermCount == BLSQ_TERM_POLY + 1, "one row per BLSQ_TERM_*");
static_assert(sizeof(MODEL_TERM_PARAMS) / sizeof(MODEL_TERM_PARAMS[0]) == kTermCount, "one count per BLSQ_TERM_*");

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

extern "C" int blsq_term_count(void) { return kTermCount; }

extern "C" int blsq_term_info(int term, const char** name, int* n_per_term) {
  if (term < 0 || term >= kTermCount) return -1;
  if (name) *name = kTermNames[term];
  if (n_per_term) *n_per_term = MODEL_TERM_PARAMS[term];
  return 0;
}

namespace {

// What tells the eight entries apart: the label of the launch, the kinds of model the entry takes, and the number a
// bad argument is reported by: its position in the entry's signature (ctx = 1; 0: the entry has no such argument).  The
// arguments come in runs that every signature has in the same order, so a run is given by its first number: fam and cnt
// follow ncomp; reps, m, n follow B; pmap follows nf; t_stride, y, w, w_stride, X follow t; J follows f.  The contents of
// pmap have no argument of their own: an entry outside -1 .. nf - 1 is `pmap_entry`, an unused variable the number after
// (the two past the entry's last argument).
// The global entry (7p) has one more run: shared and t_sstride follow S (`S` == 0: the entry has none of the three).
// The tie entry (7q) has that run and one more: tie_offset follows tie_ratio (`tie` == 0: the entry has neither).  Their
// contents are reported as pmap's are, by the two numbers after pmap's two: a ratio that is 0 or not finite, an offset
// that is not finite.  With the run of S the tie entry also takes S == 0: a plain batch, not a global evaluation.
struct EvalEntry {
  const char* label;
  bool composite;             // takes model == -1 with a component table (otherwise named models only)
  bool needs_pmap;
  int est, sampling, nan_policy, model, ncomp, B, nf, t, Pfix, f, pmap_entry;
  int S;
  int tie;
};
constexpr EvalEntry kEvalDev = {"launch_model_eval", false, false, 0, 0, 0, 2, 0, 3, 0, 7, 0, 13, 0};
constexpr EvalEntry kEvalMap = {"launch_model_eval_map", false, true, 0, 0, 0, 2, 0, 3, 7, 9, 15, 16, 19};
constexpr EvalEntry kEvalComp = {"launch_model_eval_comp", true, false, 0, 0, 0, 0, 2, 5, 9, 11, 17, 18, 21};
constexpr EvalEntry kEvalEst = {"launch_model_eval_est", true, false, 2, 0, 0, 3, 4, 7, 11, 13, 19, 20, 23};
constexpr EvalEntry kEvalBin = {"launch_model_eval_bin", true, false, 2, 3, 0, 4, 5, 8, 12, 14, 20, 21, 24};
constexpr EvalEntry kEvalNan = {"launch_model_eval_nan", true, false, 2, 3, 4, 5, 6, 9, 13, 15, 21, 22, 25};
constexpr EvalEntry kEvalGlobal = {"launch_model_eval_global", true, true, 2, 3, 4, 5, 6, 12, 16, 18, 24, 25, 28, 9};
constexpr EvalEntry kEvalTie = {"launch_model_eval_tie", true, true, 2, 3, 4, 5, 6, 12, 16, 20, 26, 27, 30, 9, 18};

// The checks of every entry, in the order of the arguments, and the launch.  A negative return names the argument.
int model_eval_checked(blsq_ctx* ctx, const EvalEntry& e, const ModelEvalCall& c) {
  if (!ctx) return -1;
  if (c.est != BLSQ_EST_LSE && c.est != BLSQ_EST_POISSON) return ctx->bad(e.est, "est must be one of BLSQ_EST_*");
  if (c.sampling != BLSQ_SAMPLE_POINT && c.sampling != BLSQ_SAMPLE_BIN)
    return ctx->bad(e.sampling, "sampling must be one of BLSQ_SAMPLE_*");
  if (c.nan_policy != BLSQ_NAN_PROPAGATE && c.nan_policy != BLSQ_NAN_OMIT)
    return ctx->bad(e.nan_policy, "nan_policy must be one of BLSQ_NAN_*");
  if (c.model < (e.composite ? -1 : 0) || c.model >= kModelCount)
    return ctx->bad(e.model, e.composite ? "model must be one of BLSQ_MODEL_*, or -1 for a composite"
                                         : "model must be one of BLSQ_MODEL_*");
  const bool comp = c.model < 0;
  const bool global = e.S != 0 && !(e.tie != 0 && c.S == 0);      // the tie entry with S == 0: a plain batch
  if (global && c.sampling != BLSQ_SAMPLE_POINT)
    return ctx->bad(e.sampling, "sampling must be BLSQ_SAMPLE_POINT: a global fit takes no bin-integrated model");
  if (global && !comp && kModels[c.model].coords != 1)
    return ctx->bad(e.model, "a global fit takes the models of one coordinate");
  const int m = c.m, n = c.n, nf = c.nf;
  long total = 0;
  if (!comp) {
    if (c.ncomp != 0) return ctx->bad(e.ncomp, "ncomp must be 0 with a named model");
  } else {
    if (c.ncomp < 1 || c.ncomp > BLSQ_MODEL_MAX_COMP)
      return ctx->bad(e.ncomp, "ncomp must be in 1 .. BLSQ_MODEL_MAX_COMP");
    if (!c.fam) return ctx->bad(e.ncomp + 1, "fam is NULL");
    if (!c.cnt) return ctx->bad(e.ncomp + 2, "cnt is NULL");
    for (int k = 0; k < c.ncomp; ++k) {
      if (c.fam[k] < 0 || c.fam[k] >= kTermCount) return ctx->bad(e.ncomp + 1, "fam entry must be one of BLSQ_TERM_*");
      if (c.cnt[k] < 1) return ctx->bad(e.ncomp + 2, "cnt entry must be at least 1");
      total += (long)c.cnt[k] * MODEL_TERM_PARAMS[c.fam[k]];
    }
  }
  if (global) {
    if (c.S < 1) return ctx->bad(e.S, e.tie ? "S must be 0 (a plain batch) or positive" : "S must be positive");
    if (!c.shared) return ctx->bad(e.S + 1, "shared is NULL");
  } else if (e.S != 0 && c.t_sstride != 0) {
    return ctx->bad(e.S + 2, "t_sstride must be 0 with S == 0");
  }
  if (c.B <= 0) return ctx->bad(e.B, "B must be positive");
  if (c.reps <= 0) return ctx->bad(e.B + 1, "reps must be positive");
  if (m <= 0) return ctx->bad(e.B + 2, "m must be positive");
  if (comp) {
    if (n < 1 || n > BLSQ_MODEL_MAX_N || total != n)
      return ctx->bad(e.B + 3, "n must be the parameters of the components together (and at most BLSQ_MODEL_MAX_N)");
  } else if (!model_n_fits(kModels[c.model], n)) {
    return ctx->bad(e.B + 3, "n does not fit the model (or exceeds BLSQ_MODEL_MAX_N)");
  }
  bool any_fixed = false;
  if (!c.pmap && !e.needs_pmap) {
    if (nf != n) return ctx->bad(e.nf, "nf must equal n without a pmap");
  } else {
    if (nf < 1 || nf > n) return ctx->bad(e.nf, "nf must be in 1 .. n");
    if (!c.pmap) return ctx->bad(e.nf + 1, "pmap is NULL");
    bool used[BLSQ_MODEL_MAX_N] = {};
    for (int j = 0; j < n; ++j) {
      if (c.pmap[j] < -1 || c.pmap[j] >= nf) return ctx->bad(e.pmap_entry, "pmap entry outside -1 .. nf - 1");
      if (c.pmap[j] < 0) any_fixed = true;
      else used[c.pmap[j]] = true;
    }
    for (int k = 0; k < nf; ++k)
      if (!used[k]) return ctx->bad(e.pmap_entry + 1, "pmap leaves a variable k < nf unused");
    if (c.tie_ratio || c.tie_offset) {         // (only the tie entry fills them)
      if (!c.tie_ratio) return ctx->bad(e.tie, "tie_ratio is NULL although tie_offset is given");
      if (!c.tie_offset) return ctx->bad(e.tie + 1, "tie_offset is NULL although tie_ratio is given");
      for (int j = 0; j < n; ++j) {
        if (c.pmap[j] < 0) continue;           // a fixed parameter: its entries are not read
        if (c.tie_ratio[j] == 0.0 || !std::isfinite(c.tie_ratio[j]))
          return ctx->bad(e.pmap_entry + 2, "tie_ratio entry must be finite and not 0");
        if (!std::isfinite(c.tie_offset[j])) return ctx->bad(e.pmap_entry + 3, "tie_offset entry must be finite");
      }
    }
  }
  if (global) {                              // nv = ns + S nl variables
    long ns = 0;
    for (int k = 0; k < nf; ++k) {
      if (c.shared[k] != 0 && c.shared[k] != 1) return ctx->bad(e.S + 1, "shared entry must be 0 or 1");
      ns += c.shared[k];
    }
    if (ns + (long)c.S * (nf - ns) > BLSQ_GLOBAL_MAX_NV)
      return ctx->bad(e.S, "ns + S * nl exceeds BLSQ_GLOBAL_MAX_NV variables");
    if (c.t_sstride != 0 && c.t_sstride != (long)m) return ctx->bad(e.S + 2, "t_sstride must be 0 or m");
  }
  const long coords = comp ? 1 : kModels[c.model].coords;
  if (!c.t) return ctx->bad(e.t, "t is NULL");
  if (global) {
    if (c.t_stride != 0 && c.t_stride != (c.t_sstride ? (long)c.S * m : (long)m))
      return ctx->bad(e.t + 1, "t_stride must be 0 or the abscissae of one group (m, with t_sstride == m: S * m)");
  } else if (c.sampling == BLSQ_SAMPLE_BIN) {
    if (c.t_stride != 0 && c.t_stride != 2 * coords * m)
      return ctx->bad(e.t + 1, "t_stride must be 0 or 2 * coords * m with BLSQ_SAMPLE_BIN");
  } else if (c.t_stride != 0 && c.t_stride != coords * m) {
    return ctx->bad(e.t + 1, "t_stride must be 0 or coords * m");
  }
  if (c.est == BLSQ_EST_POISSON && !c.y) return ctx->bad(e.t + 2, "y is NULL: the Poisson estimator needs the counts");
  if (c.nan_policy == BLSQ_NAN_OMIT && !c.y)
    return ctx->bad(e.t + 2, "y is NULL: BLSQ_NAN_OMIT reads the missing points from it");
  if (c.est == BLSQ_EST_POISSON && c.w) return ctx->bad(e.t + 3, "w must be NULL with the Poisson estimator");
  if (c.w && global) {
    if (c.w_stride != 0 && c.w_stride != (long)c.S * m) return ctx->bad(e.t + 4, "w_stride must be 0 or S * m");
  } else if (c.w && c.w_stride != 0 && c.w_stride != (long)m) {
    return ctx->bad(e.t + 4, "w_stride must be 0 or m");
  }
  if (!c.X) return ctx->bad(e.t + 5, "X is NULL (the parameter vectors)");
  if (any_fixed && !c.Pfix) return ctx->bad(e.Pfix, "Pfix is NULL although pmap holds a parameter fixed");
  if (!c.f && !c.J) return ctx->bad(e.f, "f and J are both NULL");
  if (c.J && c.reps != 1) return ctx->bad(e.f + 1, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->run(K_MODEL_EVAL, e.label, [&] { return launch_model_eval(c, ctx->stream); });
}

}  // namespace

extern "C" int blsq_model_eval_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, const double* dt,
                                   long t_stride, const double* dy, const double* dw, long w_stride, const double* dP,
                                   double* df, double* dJ, const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalDev, {BLSQ_EST_LSE, BLSQ_SAMPLE_POINT, BLSQ_NAN_PROPAGATE, model, 0, nullptr,
                                            nullptr, B, reps, m, n, n, nullptr, dt, t_stride, dy, dw, w_stride, dP,
                                            nullptr, df, dJ, dmask});
}

extern "C" int blsq_model_eval_map_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, int nf,
                                       const int32_t* pmap, const double* dt, long t_stride, const double* dy,
                                       const double* dw, long w_stride, const double* dX, const double* dPfix,
                                       double* df, double* dJ, const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalMap, {BLSQ_EST_LSE, BLSQ_SAMPLE_POINT, BLSQ_NAN_PROPAGATE, model, 0, nullptr,
                                            nullptr, B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX,
                                            dPfix, df, dJ, dmask});
}

extern "C" int blsq_model_eval_comp_dev(blsq_ctx* ctx, int ncomp, const int32_t* fam, const int32_t* cnt, int B,
                                        int reps, int m, int n, int nf, const int32_t* pmap, const double* dt,
                                        long t_stride, const double* dy, const double* dw, long w_stride,
                                        const double* dX, const double* dPfix, double* df, double* dJ,
                                        const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalComp, {BLSQ_EST_LSE, BLSQ_SAMPLE_POINT, BLSQ_NAN_PROPAGATE, -1, ncomp, fam, cnt,
                                             B, reps, m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df,
                                             dJ, dmask});
}

extern "C" int blsq_model_eval_est_dev(blsq_ctx* ctx, int est, int model, int ncomp, const int32_t* fam,
                                       const int32_t* cnt, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                                       const double* dt, long t_stride, const double* dy, const double* dw,
                                       long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                                       const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalEst, {est, BLSQ_SAMPLE_POINT, BLSQ_NAN_PROPAGATE, model, ncomp, fam, cnt, B, reps,
                                            m, n, nf, pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask});
}

extern "C" int blsq_model_eval_bin_dev(blsq_ctx* ctx, int est, int sampling, int model, int ncomp, const int32_t* fam,
                                       const int32_t* cnt, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                                       const double* dt, long t_stride, const double* dy, const double* dw,
                                       long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                                       const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalBin, {est, sampling, BLSQ_NAN_PROPAGATE, model, ncomp, fam, cnt, B, reps, m, n, nf,
                                            pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask});
}

extern "C" int blsq_model_eval_nan_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                                       const int32_t* fam, const int32_t* cnt, int B, int reps, int m, int n, int nf,
                                       const int32_t* pmap, const double* dt, long t_stride, const double* dy,
                                       const double* dw, long w_stride, const double* dX, const double* dPfix,
                                       double* df, double* dJ, const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalNan, {est, sampling, nan_policy, model, ncomp, fam, cnt, B, reps, m, n, nf, pmap,
                                            dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask});
}

extern "C" int blsq_model_eval_global_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                                          const int32_t* fam, const int32_t* cnt, int S, const int32_t* shared,
                                          long t_sstride, int G, int reps, int m, int n, int nf, const int32_t* pmap,
                                          const double* dt, long t_stride, const double* dy, const double* dw,
                                          long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                                          const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalGlobal, {est, sampling, nan_policy, model, ncomp, fam, cnt, G, reps, m, n, nf,
                                               pmap, dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask, S,
                                               shared, t_sstride});
}

extern "C" int blsq_model_eval_tie_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                                       const int32_t* fam, const int32_t* cnt, int S, const int32_t* shared,
                                       long t_sstride, int G, int reps, int m, int n, int nf, const int32_t* pmap,
                                       const double* tie_ratio, const double* tie_offset, const double* dt,
                                       long t_stride, const double* dy, const double* dw, long w_stride,
                                       const double* dX, const double* dPfix, double* df, double* dJ,
                                       const int32_t* dmask) {
  return model_eval_checked(ctx, kEvalTie, {est, sampling, nan_policy, model, ncomp, fam, cnt, G, reps, m, n, nf, pmap,
                                            dt, t_stride, dy, dw, w_stride, dX, dPfix, df, dJ, dmask, S,
                                            S > 0 ? shared : nullptr, t_sstride, tie_ratio, tie_offset});
}

// Linear residuals (linear_kernels.hip): no model, no table: the checks in the order of the arguments, then
// the launches (f, then J) as one timed call in the slot of the model evaluations.
extern "C" int blsq_linear_eval_dev(blsq_ctx* ctx, int B, int reps, int m, int n, const double* dA, long A_stride,
                                    const double* dy, const double* dw, long w_stride, const double* dX, double* df,
                                    double* dJ, const int32_t* dmask) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (reps <= 0) return ctx->bad(3, "reps must be positive");
  if (m <= 0) return ctx->bad(4, "m must be positive");
  if (n < 1 || n > BLSQ_LINEAR_MAX_N) return ctx->bad(5, "n must be in 1 .. BLSQ_LINEAR_MAX_N");
  if (!dA) return ctx->bad(6, "A is NULL");
  if (A_stride != 0 && A_stride != (long)m * n) return ctx->bad(7, "A_stride must be 0 or m * n");
  if (w_stride != 0 && w_stride != (long)m) return ctx->bad(10, "w_stride must be 0 or m");
  if (!dX) return ctx->bad(11, "X is NULL (the points)");
  if (!df && !dJ) return ctx->bad(12, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(13, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const LinearEvalCall c{B, reps, m, n, dA, A_stride, dy, dw, w_stride, dX, df, dJ, dmask};
  return ctx->run(K_MODEL_EVAL, "launch_linear_eval", [&] { return launch_linear_eval(c, ctx->stream); });
}

// Expression models (expr_kernels.hip): a program checked on the host alone, and its evaluation: the
// checks in the order of the arguments (the program's by expr_program_bad, whose finding `at` maps onto the entry's
// positions), then one timed call in the slot of the model evaluations.
extern "C" int blsq_expr_check(int nops, const uint64_t* ops, int root, int nconst, int nf, int npfix, int ncoord) {
  static const int at[] = {0, 1, 2, 3, 4, 5, 6, 7};          // EXPR_BAD_* -> the position in this signature
  return -at[expr_program_bad(nops, reinterpret_cast<const unsigned long long*>(ops), root, nconst, nf, npfix, ncoord)];
}

extern "C" int blsq_expr_eval_dev(blsq_ctx* ctx, int est, int nan_policy, int B, int reps, int m, int nf, int npfix,
                                  int ncoord, int nops, const uint64_t* ops, int root, int nconst, const double* consts,
                                  const double* dt, long t_stride, const double* dy, const double* dw, long w_stride,
                                  const double* dX, const double* dPfix, double* df, double* dJ, const int32_t* dmask) {
  if (!ctx) return -1;
  if (est != BLSQ_EST_LSE && est != BLSQ_EST_POISSON) return ctx->bad(2, "est must be one of BLSQ_EST_*");
  if (nan_policy != BLSQ_NAN_PROPAGATE && nan_policy != BLSQ_NAN_OMIT)
    return ctx->bad(3, "nan_policy must be one of BLSQ_NAN_*");
  if (B <= 0) return ctx->bad(4, "B must be positive");
  if (reps <= 0) return ctx->bad(5, "reps must be positive");
  if (m <= 0) return ctx->bad(6, "m must be positive");
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(ops);
  static const int at[] = {0, 10, 11, 12, 13, 7, 8, 9};      // EXPR_BAD_* -> the position in this signature
  static const char* const why[] = {
      "", "nops must be in 0 .. BLSQ_EXPR_MAX_OPS", "ops is NULL, or an op has an unknown opcode or an operand out of range",
      "root is not a valid operand", "nconst must be in 0 .. BLSQ_EXPR_MAX_CONST", "nf must be in 1 .. BLSQ_MODEL_MAX_N",
      "npfix must be in 0 .. BLSQ_MODEL_MAX_N", "ncoord must be in 1 .. BLSQ_EXPR_MAX_COORD"};
  if (const int bad = expr_program_bad(nops, words, root, nconst, nf, npfix, ncoord)) return ctx->bad(at[bad], why[bad]);
  if (nconst > 0 && !consts) return ctx->bad(14, "consts is NULL");
  if (!dt) return ctx->bad(15, "t is NULL");
  if (t_stride != 0 && t_stride != (long)ncoord * m) return ctx->bad(16, "t_stride must be 0 or ncoord * m");
  if (est == BLSQ_EST_POISSON && !dy) return ctx->bad(17, "y is NULL: the Poisson estimator needs the counts");
  if (nan_policy == BLSQ_NAN_OMIT && !dy) return ctx->bad(17, "y is NULL: BLSQ_NAN_OMIT reads the missing points from it");
  if (est == BLSQ_EST_POISSON && dw) return ctx->bad(18, "w must be NULL with the Poisson estimator");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(19, "w_stride must be 0 or m");
  if (!dX) return ctx->bad(20, "X is NULL (the points)");
  if (!dPfix && expr_reads_pfix(nops, words, root)) return ctx->bad(21, "Pfix is NULL although the program has a PFIX operand");
  if (!df && !dJ) return ctx->bad(22, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(23, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ExprEvalCall c{est, nan_policy, B, reps, m, nf, npfix, ncoord, nops, words, root, nconst, consts, dt, t_stride,
                       dy, dw, w_stride, dX, dPfix, df, dJ, dmask};
  return ctx->run(K_MODEL_EVAL, "launch_expr_eval", [&] { return launch_expr_eval(c, ctx->stream); });
}

// BVLS / NNLS (bvls_kernels.hip): the moments of a batch, and the whole active-set solve of every problem
// in one kernel.  The checks in the order of the arguments; each entry is one timed call in the slot of the model
// evaluations.
extern "C" int blsq_bvls_moments_dev(blsq_ctx* ctx, int B, int m, int n, const double* dA, long A_stride,
                                     const double* dy, const double* dw, long w_stride, double* dG, long G_stride,
                                     double* dc) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n < 1 || n > BLSQ_BVLS_MAX_N) return ctx->bad(4, "n must be in 1 .. BLSQ_BVLS_MAX_N");
  if (!dA) return ctx->bad(5, "A is NULL");
  if (A_stride != 0 && A_stride != (long)m * n) return ctx->bad(6, "A_stride must be 0 or m * n");
  if (!dy) return ctx->bad(7, "y is NULL");
  if (w_stride != 0 && w_stride != (long)m) return ctx->bad(9, "w_stride must be 0 or m");
  if (!dG) return ctx->bad(10, "G is NULL");
  if (G_stride != 0 && G_stride != (long)n * n) return ctx->bad(11, "G_stride must be 0 or n * n");
  if (G_stride == 0 && (A_stride != 0 || (dw && w_stride != 0)))
    return ctx->bad(11, "G_stride must be n * n with a matrix or weights per problem");
  if (!dc) return ctx->bad(12, "c is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const BvlsMomentsCall c{B, m, n, dA, A_stride, dy, dw, w_stride, dG, G_stride, dc};
  return ctx->run(K_MODEL_EVAL, "launch_bvls_moments", [&] { return launch_bvls_moments(c, ctx->stream); });
}

// the checks the two solve entries share (arguments 2 .. 22) -> 0, or the negative position
static int bvls_solve_args(blsq_ctx* ctx, int B, int m, int n, const double* dG, long G_stride, const double* dc,
                           const double* dlb, const double* dub, double tol, int max_pass, const double* dA,
                           long A_stride, const double* dy, long w_stride, double* dx, int32_t* don_bound,
                           double* dfun, double* dgrad, double* doptimality, int32_t* dstat) {
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (dA ? m <= 0 : m < 0) return ctx->bad(3, "m must be positive (without A: not negative; it is not read)");
  if (n < 1 || n > BLSQ_BVLS_MAX_N) return ctx->bad(4, "n must be in 1 .. BLSQ_BVLS_MAX_N");
  if (!dG) return ctx->bad(5, "G is NULL");
  if (G_stride != 0 && G_stride != (long)n * n) return ctx->bad(6, "G_stride must be 0 or n * n");
  if (!dc) return ctx->bad(7, "c is NULL");
  if (!dlb) return ctx->bad(8, "lb is NULL");
  if (!dub) return ctx->bad(9, "ub is NULL");
  if (tol != tol) return ctx->bad(10, "tol is not a number");
  if (max_pass < 0) return ctx->bad(11, "max_pass must not be negative");
  if (dA) {
    if (A_stride != 0 && A_stride != (long)m * n) return ctx->bad(13, "A_stride must be 0 or m * n");
    if (!dy) return ctx->bad(14, "y is NULL although A is given");
    if (w_stride != 0 && w_stride != (long)m) return ctx->bad(16, "w_stride must be 0 or m");
  }
  if (!dx) return ctx->bad(17, "x is NULL");
  if (!don_bound) return ctx->bad(18, "on_bound is NULL");
  if (dfun && !dA) return ctx->bad(19, "fun must be NULL without A");
  if (!dgrad) return ctx->bad(20, "grad is NULL");
  if (!doptimality) return ctx->bad(21, "optimality is NULL");
  if (!dstat) return ctx->bad(22, "stat is NULL");
  return 0;
}

extern "C" int blsq_bvls_solve_dev(blsq_ctx* ctx, int B, int m, int n, const double* dG, long G_stride,
                                   const double* dc, const double* dlb, const double* dub, double tol, int max_pass,
                                   const double* dA, long A_stride, const double* dy, const double* dw, long w_stride,
                                   double* dx, int32_t* don_bound, double* dfun, double* dgrad, double* doptimality,
                                   int32_t* dstat) {
  if (!ctx) return -1;
  const int bad = bvls_solve_args(ctx, B, m, n, dG, G_stride, dc, dlb, dub, tol, max_pass, dA, A_stride, dy, w_stride,
                                  dx, don_bound, dfun, dgrad, doptimality, dstat);
  if (bad != 0) return bad;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const BvlsSolveCall c{B, m, n, dG, G_stride, dc, dlb, dub, tol, max_pass, dA, dA ? A_stride : 0, dA ? dy : nullptr,
                        dA ? dw : nullptr, dA ? w_stride : 0, dx, don_bound, dfun, dgrad, doptimality, dstat};
  return ctx->run(K_MODEL_EVAL, "launch_bvls_solve", [&] { return launch_bvls_solve(c, ctx->stream); });
}

// The solve under one equality e^T x = d per problem: the arguments of blsq_bvls_solve_dev, then e,
// e_stride, d and the multiplier.
extern "C" int blsq_bvls_solve_eq_dev(blsq_ctx* ctx, int B, int m, int n, const double* dG, long G_stride,
                                      const double* dc, const double* dlb, const double* dub, double tol,
                                      int max_pass, const double* dA, long A_stride, const double* dy,
                                      const double* dw, long w_stride, double* dx, int32_t* don_bound, double* dfun,
                                      double* dgrad, double* doptimality, int32_t* dstat, const double* de,
                                      long e_stride, const double* dd, double* dmultiplier) {
  if (!ctx) return -1;
  const int bad = bvls_solve_args(ctx, B, m, n, dG, G_stride, dc, dlb, dub, tol, max_pass, dA, A_stride, dy, w_stride,
                                  dx, don_bound, dfun, dgrad, doptimality, dstat);
  if (bad != 0) return bad;
  if (!de) return ctx->bad(23, "e is NULL");
  if (e_stride != 0 && e_stride != (long)n) return ctx->bad(24, "e_stride must be 0 or n");
  if (!dd) return ctx->bad(25, "d is NULL");
  if (!dmultiplier) return ctx->bad(26, "multiplier is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const BvlsSolveCall c{B, m, n, dG, G_stride, dc, dlb, dub, tol, max_pass, dA, dA ? A_stride : 0, dA ? dy : nullptr,
                        dA ? dw : nullptr, dA ? w_stride : 0, dx, don_bound, dfun, dgrad, doptimality, dstat};
  const BvlsEqCall q{de, e_stride, dd, dmultiplier};
  return ctx->run(K_MODEL_EVAL, "launch_bvls_solve_eq", [&] { return launch_bvls_solve_eq(c, q, ctx->stream); });
}

// Instrument response (response_kernels.hip): the convolution of raw model values and of a raw Jacobian
// with a measured kernel, and the epilogue of a model evaluation behind it.  The checks in the order of the arguments,
// then the launches (f, then J) as one timed call in the slot of the model evaluations.
extern "C" int blsq_response_apply_dev(blsq_ctx* ctx, int est, int nan_policy, int B, int reps, int m, int nc, int L,
                                       int origin, const double* dh, long h_stride, const double* dg, const double* dG,
                                       const double* dy, const double* dw, long w_stride, double* df, double* dJ,
                                       const int32_t* dmask) {
  if (!ctx) return -1;
  if (est != BLSQ_EST_LSE && est != BLSQ_EST_POISSON) return ctx->bad(2, "est must be one of BLSQ_EST_*");
  if (nan_policy != BLSQ_NAN_PROPAGATE && nan_policy != BLSQ_NAN_OMIT)
    return ctx->bad(3, "nan_policy must be one of BLSQ_NAN_*");
  if (B <= 0) return ctx->bad(4, "B must be positive");
  if (reps <= 0) return ctx->bad(5, "reps must be positive");
  if (m <= 0 || m > BLSQ_RESPONSE_MAX_M) return ctx->bad(6, "m must be in 1 .. BLSQ_RESPONSE_MAX_M");
  if (nc <= 0) return ctx->bad(7, "nc must be positive");
  if (L < 1 || L > BLSQ_RESPONSE_MAX_L) return ctx->bad(8, "L must be in 1 .. BLSQ_RESPONSE_MAX_L");
  if (origin < 0 || origin >= L) return ctx->bad(9, "origin must be in 0 .. L - 1");
  if (!dh) return ctx->bad(10, "h is NULL (the kernel)");
  if (h_stride != 0 && h_stride != (long)L) return ctx->bad(11, "h_stride must be 0 or L");
  if (!dg && df) return ctx->bad(12, "g is NULL although f is asked for");
  if (!dg && dJ && est == BLSQ_EST_POISSON)
    return ctx->bad(12, "g is NULL: the Jacobian of the Poisson estimator needs the model values");
  if (!dG && dJ) return ctx->bad(13, "G is NULL although J is asked for");
  if (est == BLSQ_EST_POISSON && !dy) return ctx->bad(14, "y is NULL: the Poisson estimator needs the counts");
  if (nan_policy == BLSQ_NAN_OMIT && !dy) return ctx->bad(14, "y is NULL: BLSQ_NAN_OMIT reads the missing points from it");
  if (est == BLSQ_EST_POISSON && dw) return ctx->bad(15, "w must be NULL with the Poisson estimator");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(16, "w_stride must be 0 or m");
  if (!df && !dJ) return ctx->bad(17, "f and J are both NULL");
  if (dJ && reps != 1) return ctx->bad(18, "J requires reps == 1");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ResponseCall c{est, nan_policy, B, reps, m, nc, L, origin, dh, h_stride, dg, dG, dy, dw, w_stride, df, dJ, dmask};
  return ctx->run(K_MODEL_EVAL, "launch_response_apply", [&] { return launch_response_apply(c, ctx->stream); });
}

// Separable fits (varpro_kernels.hip): the solver variables expanded to model parameters with 1.0 in the
// linear slots, and the projection behind the model kernel's raw Jacobian.  lin and owner are host arrays that travel
// in the kernel arguments.  The checks in the order of the arguments; each entry is one timed call in the slot of the
// model evaluations.
namespace {

// lin is NULL, not ascending or leaves 0 .. n - 1
bool varpro_lin_bad(int n, int nl, const int32_t* lin) {
  if (!lin) return true;
  for (int k = 0; k < nl; ++k)
    if (lin[k] < 0 || lin[k] >= n || (k > 0 && lin[k] <= lin[k - 1])) return true;
  return false;
}

}  // namespace

extern "C" int blsq_varpro_expand_dev(blsq_ctx* ctx, int B, int n, int nl, const int32_t* lin, const double* dX,
                                      double* dP) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (n < 2 || n > BLSQ_MODEL_MAX_N) return ctx->bad(3, "n must be in 2 .. BLSQ_MODEL_MAX_N");
  if (nl < 1 || nl > BLSQ_VARPRO_MAX_NL || nl >= n)
    return ctx->bad(4, "nl must be in 1 .. BLSQ_VARPRO_MAX_NL and leave a non-linear parameter (nl < n)");
  if (varpro_lin_bad(n, nl, lin)) return ctx->bad(5, "lin is NULL or not ascending within 0 .. n - 1");
  if (!dX) return ctx->bad(6, "X is NULL (the solver variables)");
  if (!dP) return ctx->bad(7, "P is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const VarproExpandCall c{B, n, nl, lin, dX, dP};
  return ctx->run(K_MODEL_EVAL, "launch_varpro_expand", [&] { return launch_varpro_expand(c, ctx->stream); });
}

extern "C" int blsq_varpro_reduce_dev(blsq_ctx* ctx, int B, int m, int n, int nl, const int32_t* lin,
                                      const int32_t* owner, const double* dG, const double* dy, const double* dw,
                                      long w_stride, double* df, double* dJ, double* dc, int32_t* dinfo,
                                      const int32_t* dmask) {
  if (!ctx) return -1;
  if (B <= 0) return ctx->bad(2, "B must be positive");
  if (m <= 0) return ctx->bad(3, "m must be positive");
  if (n < 2 || n > BLSQ_MODEL_MAX_N) return ctx->bad(4, "n must be in 2 .. BLSQ_MODEL_MAX_N");
  if (nl < 1 || nl > BLSQ_VARPRO_MAX_NL || nl >= n)
    return ctx->bad(5, "nl must be in 1 .. BLSQ_VARPRO_MAX_NL and leave a non-linear parameter (nl < n)");
  if (m <= nl) return ctx->bad(3, "m must exceed nl: the linear parameters must leave a residual");
  if (varpro_lin_bad(n, nl, lin)) return ctx->bad(6, "lin is NULL or not ascending within 0 .. n - 1");
  if (!owner) return ctx->bad(7, "owner is NULL");
  for (int j = 0, at = 0; j < n; ++j) {
    const bool linear = at < nl && lin[at] == j;
    if (linear) ++at;
    if (linear ? owner[j] != -1 : (owner[j] < 0 || owner[j] >= nl))
      return ctx->bad(7, "owner must be -1 on lin and a position 0 .. nl - 1 in lin elsewhere");
  }
  if (!dG) return ctx->bad(8, "G is NULL (the raw Jacobian)");
  if (!dy) return ctx->bad(9, "y is NULL");
  if (dw && w_stride != 0 && w_stride != (long)m) return ctx->bad(11, "w_stride must be 0 or m");
  if (!df && !dJ && !dc) return ctx->bad(12, "f, J and c are all NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const VarproReduceCall c{B, m, n, nl, lin, owner, dG, dy, dw, w_stride, df, dJ, dc, dinfo, dmask};
  return ctx->run(K_MODEL_EVAL, "launch_varpro_reduce", [&] { return launch_varpro_reduce(c, ctx->stream); });
}

// Separable global fits (varpro_kernels.hip): the two stages above for G groups of S data sets that share
// some non-linear parameters, and the per-data-set blocks of the full covariance from the reduced one.  shared is a host
// array [n] of 0 / 1 flags over the model parameters, like lin and owner read during the call.
namespace {

// 0, or the position (S_at or shared_at) of what is wrong with the layout of a group
int varpro_global_bad(blsq_ctx* ctx, int S_at, int shared_at, int S, int n, int nl, const int32_t* lin,
                      const int32_t* shared) {
  if (S < 1) return ctx->bad(S_at, "S must be positive");
  if (!shared) return ctx->bad(shared_at, "shared is NULL");
  for (int j = 0, at = 0; j < n; ++j) {
    const bool linear = at < nl && lin[at] == j;
    if (linear) ++at;
    if (shared[j] != 0 && shared[j] != 1) return ctx->bad(shared_at, "shared must hold 0 or 1");
    if (linear && shared[j]) return ctx->bad(shared_at, "shared is set on a linear parameter");
  }
  if (varpro_global_nv(S, n, nl, lin, shared) < 0)
    return ctx->bad(S_at, "nv = nsh + S nloc exceeds BLSQ_GLOBAL_MAX_NV");
  return 0;
}

}  // namespace

extern "C" int blsq_varpro_expand_global_dev(blsq_ctx* ctx, int G, int S, int n, int nl, const int32_t* lin,
                                             const int32_t* shared, const double* dX, double* dP) {
  if (!ctx) return -1;
  if (G <= 0) return ctx->bad(2, "G must be positive");
  if (S > 0 && (long)G * S > 0x7fffffffL) return ctx->bad(3, "G S must fit an int");
  if (n < 2 || n > BLSQ_MODEL_MAX_N) return ctx->bad(4, "n must be in 2 .. BLSQ_MODEL_MAX_N");
  if (nl < 1 || nl > BLSQ_VARPRO_MAX_NL || nl >= n)
    return ctx->bad(5, "nl must be in 1 .. BLSQ_VARPRO_MAX_NL and leave a non-linear parameter (nl < n)");
  if (varpro_lin_bad(n, nl, lin)) return ctx->bad(6, "lin is NULL or not ascending within 0 .. n - 1");
  if (int rc = varpro_global_bad(ctx, 3, 7, S, n, nl, lin, shared)) return rc;
  if (!dX) return ctx->bad(8, "X is NULL (the solver variables)");
  if (!dP) return ctx->bad(9, "P is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const VarproExpandCall c{G, n, nl, lin, dX, dP};
  const VarproGlobalCall q{S, shared, nullptr, nullptr};
  return ctx->run(K_MODEL_EVAL, "launch_varpro_expand_global",
                  [&] { return launch_varpro_expand_global(c, q, ctx->stream); });
}

extern "C" int blsq_varpro_reduce_global_dev(blsq_ctx* ctx, int G, int S, int m, int n, int nl, const int32_t* lin,
                                             const int32_t* owner, const int32_t* shared, const double* dG,
                                             const double* dy, const double* dw, long w_stride, double* df, double* dJ,
                                             double* dc, int32_t* dinfo, double* dSinv, double* dTD,
                                             const int32_t* dmask) {
  if (!ctx) return -1;
  if (G <= 0) return ctx->bad(2, "G must be positive");
  if (S > 0 && (long)G * S > 0x7fffffffL) return ctx->bad(3, "G S must fit an int");
  if (m <= 0) return ctx->bad(4, "m must be positive");
  if (n < 2 || n > BLSQ_MODEL_MAX_N) return ctx->bad(5, "n must be in 2 .. BLSQ_MODEL_MAX_N");
  if (nl < 1 || nl > BLSQ_VARPRO_MAX_NL || nl >= n)
    return ctx->bad(6, "nl must be in 1 .. BLSQ_VARPRO_MAX_NL and leave a non-linear parameter (nl < n)");
  if (m <= nl) return ctx->bad(4, "m must exceed nl: the linear parameters must leave a residual");
  if (varpro_lin_bad(n, nl, lin)) return ctx->bad(7, "lin is NULL or not ascending within 0 .. n - 1");
  if (!owner) return ctx->bad(8, "owner is NULL");
  for (int j = 0, at = 0; j < n; ++j) {
    const bool linear = at < nl && lin[at] == j;
    if (linear) ++at;
    if (linear ? owner[j] != -1 : (owner[j] < 0 || owner[j] >= nl))
      return ctx->bad(8, "owner must be -1 on lin and a position 0 .. nl - 1 in lin elsewhere");
  }
  if (int rc = varpro_global_bad(ctx, 3, 9, S, n, nl, lin, shared)) return rc;
  if (!dG) return ctx->bad(10, "G is NULL (the raw Jacobian)");
  if (!dy) return ctx->bad(11, "y is NULL");
  if (dw && w_stride != 0 && w_stride != (long)S * m) return ctx->bad(13, "w_stride must be 0 or S m");
  if (!df && !dJ && !dc && !dSinv && !dTD) return ctx->bad(14, "f, J, c, Sinv and TD are all NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const VarproReduceCall c{G, m, n, nl, lin, owner, dG, dy, dw, w_stride, df, dJ, dc, dinfo, dmask};
  const VarproGlobalCall q{S, shared, dSinv, dTD};
  return ctx->run(K_MODEL_EVAL, "launch_varpro_reduce_global",
                  [&] { return launch_varpro_reduce_global(c, q, ctx->stream); });
}

extern "C" int blsq_varpro_cov_blocks_dev(blsq_ctx* ctx, int G, int S, int n, int nl, const int32_t* lin,
                                          const int32_t* shared, const double* dC, const double* dSinv,
                                          const double* dTD, const double* dscale, const int32_t* dinfo,
                                          const int32_t* dstatus, double* dcov) {
  if (!ctx) return -1;
  if (G <= 0) return ctx->bad(2, "G must be positive");
  if (S > 0 && (long)G * S > 0x7fffffffL) return ctx->bad(3, "G S must fit an int");
  if (n < 2 || n > BLSQ_MODEL_MAX_N) return ctx->bad(4, "n must be in 2 .. BLSQ_MODEL_MAX_N");
  if (nl < 1 || nl > BLSQ_VARPRO_MAX_NL || nl >= n)
    return ctx->bad(5, "nl must be in 1 .. BLSQ_VARPRO_MAX_NL and leave a non-linear parameter (nl < n)");
  if (varpro_lin_bad(n, nl, lin)) return ctx->bad(6, "lin is NULL or not ascending within 0 .. n - 1");
  if (int rc = varpro_global_bad(ctx, 3, 7, S, n, nl, lin, shared)) return rc;
  if (!dC) return ctx->bad(8, "C is NULL (the covariance of the reduced group)");
  if (!dSinv) return ctx->bad(9, "Sinv is NULL");
  if (!dTD) return ctx->bad(10, "TD is NULL");
  if (!dcov) return ctx->bad(14, "cov is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const VarproCovCall c{G, S, n, nl, lin, shared, dC, dSinv, dTD, dscale, dinfo, dstatus, dcov};
  return ctx->run(K_MODEL_EVAL, "launch_varpro_cov_blocks", [&] { return launch_varpro_cov_blocks(c, ctx->stream); });
}
