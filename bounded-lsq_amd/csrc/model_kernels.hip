// Built-in fit models evaluated on the device (blsq_model_eval_dev).
//
// For a batch of parameter vectors P [Q][n], Q = B * reps, q = b * reps + r:
//   f[q][i]    = w[b][i] * (model(t[b][.., i]; P[q]) - y[b][i])
//   J[q][i][j] = w[b][i] * d model / d p_j                               (reps == 1)
// Five closed-form families (BLSQ_MODEL_*); the formulas, operation by operation, are those of the numpy functions of
// bounded_lsq/_models.py.  Compiled with -ffp-contract=off, so a value does not depend on what the compiler fuses; the
// only difference from numpy is the last bit of exp().  No checking: a non-finite value passes through as IEEE gives it.
//
// Shape.  One WAVE owns one work item: 64 consecutive rows of one point q; a workgroup is 1, 2 or 4 independent waves
// (as many as the J tiles leave room for in LDS).  A lane owns row i, reads its parameters through wave-uniform (scalar)
// loads and evaluates the K terms once for both f and the J row.  f is stored directly (lane i -> f[q][i]).  The J
// tile of the 64 rows is one contiguous block of 64 n doubles in memory: a lane writes its row into the wave's LDS
// tile (row stride n | 1 doubles: odd, so the 16 lanes of an 8-byte LDS store group fall on 16 different bank pairs), and
// the wave then streams the tile out with consecutive lanes on consecutive addresses.  Store-bound: 8 m n bytes per
// problem; no MFMA, no scratch.
//
// Mapped instances (MAPPED = true; blsq_model_eval_map_dev).  The model's n parameters are a function of
// nf <= n solver variables: P_full[q][j] = X[q][pmap[j]], or Pfix[b][j] where pmap[j] == -1.  A wave expands its point's
// vector once (lane j produces P_full[q][j]) into 64 doubles of LDS of its own, and model_row reads p[] from there: every
// lane reads the same address, which LDS broadcasts.  The J row is written through row_put: column j goes to slot
// pmap[j] of a tile of row stride nf | 1: the first column of a slot is stored, later ones are added in ascending j
// (a sequential float64 sum), a column with pmap[j] == -1 is computed and dropped.  f is the residual of the unmapped
// instance at P_full, bit for bit.  The unmapped instances resolve row_put to the plain store and compile to the code
// they had before the flag existed.
//
// Composite instances (MODEL = MODEL_COMPOSITE; blsq_model_eval_comp_dev).  The model is a sum of up to 8
// components chosen at run time: {family BLSQ_TERM_*, count} pairs in a table that travels by value in the kernel
// arguments, as pm[] does, so the walk over it runs on scalar loads and the switch on the family is wave-uniform.  A
// component's terms are the *_term functions below, the ones the five closed instances are built from; its value is
// their sum in ascending order (poly: Horner), the model the sequential sum of the component values.  Parameters and
// Jacobian columns are the concatenation of the components' slices, so one running offset serves both.  The shell
// (staging, barriers, stream-out) is the one kernel below for every instance.
//
// Poisson instances (POISSON = true; blsq_model_eval_est_dev with BLSQ_EST_POISSON).  The residual is the
// signed square root of the Poisson deviance of the count y[b][i] under the model value mu, and the Jacobian row is the
// model's row times c = dr / dmu: poisson_rc below, operation by operation models.poisson_transform of
// bounded_lsq/_models.py.  The terms write their columns unweighted (wi = 1, w must be NULL); once the row's value is
// known the lane computes (r, c), stores f = r and multiplies the nc entries of its own LDS row by c (the mapped slots
// after their sums) before the barrier.  The row pass walks the addresses the puts walked, lane * (nc | 1) + k: at an odd
// stride both its 8-byte loads (groups of 32 lanes over 64 banks) and its stores (16 lanes over 32) find every lane of
// a group on a bank pair of its own.  No extra memory traffic but the one read of y that the residual needs anyway; LDS
// footprint and waves per workgroup are those of the least-squares instance.  The estimator is a template flag, not a
// field of ModelArgs: the least-squares instances are then the instructions they were before it existed, and the 24
// instances build in 4.3 s where the 12 took 3.8 s, next to files that take a minute, so build time does not argue for
// a runtime field, which would put the transform's registers and branch into every least-squares instance.
//
// Bin-integrated instances (BINNED = true; blsq_model_eval_bin_dev with BLSQ_SAMPLE_BIN).  The value of
// row i is the integral of the model over the bin [lo, hi], lo = t[b][0][i], hi = t[b][1][i] (gauss2d: the pixel
// [t[b][0][i], t[b][1][i]] x [t[b][2][i], t[b][3][i]]), and the columns are the integrals of the point-sampled columns:
// the *_bin functions below, operation by operation the _bfill_* functions of bounded_lsq/_models.py; erf, erfc, atan2,
// expm1 and exp are the only differences.  They feed the same puts, so the shell, the Poisson row pass and the stream-out
// are untouched.  A template flag for the reason given for POISSON: the point-sampled instances are the instructions
// they were.
//
// Omitting instances (OMIT = true; blsq_model_eval_nan_dev with BLSQ_NAN_OMIT).  Row i of problem b is left
// out of the fit where y[b][i] is NaN: the lane reads y first (y must not be NULL), tests y != y (the file is built
// without any finite-math flag) and, for such a row, evaluates nothing: t, w and the transform are not touched; it
// writes +0.0 into the nc slots of its LDS row and stores f = +0.0.  The branch is lane-divergent; the lanes that keep
// their row run the code of the instance without the flag, whose walk over the component table stays wave-uniform.  The
// shell is untouched, and the flag is a template flag for the reason given for POISSON: the 48 instances without it are
// the instructions they were, and the 96 build in 18 s where the 48 took 10 s.
//
// Global instances (MAP == MAP_GLOBAL; blsq_model_eval_global_dev).  G groups of S data sets share some of
// the map's slots: a group is one problem of S m rows and nv = ns + S nl variables.  The work items of a point run over
// its data sets (items = Q S ceil(m / 64)), so a wave still owns 64 rows of ONE data set s, s is wave-uniform, and the
// wave is a mapped wave in everything but its addresses: it expands its parameter vector from X[q][.] at the columns of
// data set s, stages its rows nf wide at stride nf | 1 through the same row_put (the host numbers the slots shared ones
// first, so the tile's columns are the variables [0, ns) and data set s's window in order), and runs the Poisson row
// pass and the OMIT branch over those nf slots alone.  Only the stream-out differs: the wave's rows are one contiguous
// block of nr nv doubles, which it writes with consecutive lanes on consecutive addresses, an element from the tile
// where its column is one of the data set's and +0.0 elsewhere.  The zeros never pass through arithmetic (a Poisson c
// of NaN multiplies the nf staged slots only), LDS does not depend on nv, and the waves per workgroup are the mapped
// instance's.  MAP is a template parameter for the reason given for POISSON; the bin-integrated and gauss2d global
// instances are not built (20 instances more: 116).
//
// Affine instances (AFFINE = true; blsq_model_eval_tie_dev with tie_ratio / tie_offset).  A tied parameter
// follows its slot by a ratio and an offset, P_full[q][j] = ratio[j] * X[q][.] + offset[j]; ratio[] and offset[], 64
// doubles each, travel by value in the kernel arguments behind everything the instance without the flag takes (TieArgs:
// 1 KB more, 1504 bytes for the composite global instance, under the 4 KB of the kernarg segment), so nothing is
// staged in LDS and the waves per workgroup are unchanged.  Two places differ.  The expansion: lane j computes v = p[k]
// and then r * v + d, the product first, where (r, d) != (1, 0), and keeps v otherwise (a -0.0 stays -0.0); parameters
// held at Pfix are untouched.  row_put: the value of column k is multiplied by ratio[k] before it is stored into, or
// added to, its slot: r * (wi * e), the model's weighted column first; k is wave-uniform, so ratio[k] is a scalar load, as
// the walk over the component table is.  The Poisson row pass, the OMIT branch and both stream-outs see slots that are
// summed already and are untouched.  The terms take the map as a deduced type (const signed char*, or the pair TieMap), so
// the instances without the flag are instantiated over the types they had, and AFFINE is a template flag for the reason
// given for POISSON: the 116 instances without it are the instructions they were.  Built for every mapped and global
// instance, gauss2d's mapped ones included (68 instances more: 184); the file builds in 13.5 s where the 116 took 8.4 s.
#include "../../include/blsq.h"
#include "blsq_device.h"
#include "blsq_kernels.h"
#include "poisson_rc.h"

#include <type_traits>

namespace blsq {

static constexpr int MODEL_ROWS = 64;                 // rows of one work item: one per lane
static constexpr int MODEL_LDS_BYTES = 48 * 1024;     // J tiles of one workgroup (n = 64: one wave, 33280 B)

struct ModelArgs {
  int m, n, reps, tiles;        // tiles = ceil(m / 64)
  long items;                   // Q * tiles
  const double* t; long t_stride;
  const double* y;
  const double* w; long w_stride;
  const double* P;
  double* f;
  double* J;
  const int* mask;
};

// The map of a mapped launch, behind the arguments every instance takes.  pm[j]: -1 (held at Pfix), the slot k for the
// first column of slot k (its leader), 64 + k for a later one.
struct ModelMapArgs : ModelArgs {
  int nf;                       // solver variables; P is X [Q][nf]
  const double* Pfix;           // [B][n]; read where pm[j] == -1 only
  signed char pm[MODEL_ROWS];
};
// The component table of a composite launch: entry c < ncomp is 16 bits, the family (BLSQ_TERM_*) in the low byte and
// the count (terms; poly: coefficients) in the high one; entries 0 .. 3 in `lo`, 4 .. 7 in `hi`, from bit 0 upwards.  Two
// words walked by shifts: a byte array indexed by c would be read through vector loads.
struct CompTable {
  int ncomp;
  unsigned long long lo, hi;
};
static_assert(BLSQ_MODEL_MAX_COMP == 8, "CompTable holds 8 entries of 16 bits");
// A global launch (7p): the map above with its slots renumbered, the ns shared ones first (pm[] then names a column of
// the tile in that order); data set s owns the variables [0, ns) and [ns + s nl, ns + s nl + nl) of the group's nv.
struct ModelGlobalArgs : ModelMapArgs {
  int S, ns, nl, nv;            // P is X [Q][nv]; Pfix [B][S][n]; w_stride is 0 or m per DATA SET
  long t_sstride;               // t of data set s of group g: t + g * t_stride + s * t_sstride
};
template <class Base> struct CompArgs : Base { CompTable tab; };
// An affine launch (7q): parameter j with pm[j] >= 0 is ratio[j] * (its slot's variable) + offset[j]; (1, 0) elsewhere.
// By value behind everything the instance without the flag takes, so that instance's arguments keep their offsets.
template <class Base> struct TieArgs : Base { double ratio[MODEL_ROWS], offset[MODEL_ROWS]; };
static constexpr int MODEL_COMPOSITE = -1;            // the MODEL of the composite instances (no BLSQ_MODEL_* id)
// MAP: how the solver's variables become the model's parameters
static constexpr int MAP_NONE = 0, MAP_PARAM = 1, MAP_GLOBAL = 2;
template <bool COMP, int MAP> struct ModelArgsBase { using type = ModelArgs; };
template <> struct ModelArgsBase<false, MAP_PARAM> { using type = ModelMapArgs; };
template <> struct ModelArgsBase<false, MAP_GLOBAL> { using type = ModelGlobalArgs; };
template <> struct ModelArgsBase<true, MAP_NONE> { using type = CompArgs<ModelArgs>; };
template <> struct ModelArgsBase<true, MAP_PARAM> { using type = CompArgs<ModelMapArgs>; };
template <> struct ModelArgsBase<true, MAP_GLOBAL> { using type = CompArgs<ModelGlobalArgs>; };
template <bool COMP, int MAP, bool AFFINE = false> struct ModelArgsOf {
  using Base = typename ModelArgsBase<COMP, MAP>::type;
  using type = std::conditional_t<AFFINE, TieArgs<Base>, Base>;
};
static_assert(sizeof(TieArgs<CompArgs<ModelGlobalArgs>>) <= 4096, "the largest argument struct fits the kernarg segment");

__device__ __forceinline__ int map_nf(const ModelArgs& A) { return A.n; }
__device__ __forceinline__ int map_nf(const ModelMapArgs& A) { return A.nf; }
__device__ __forceinline__ const signed char* map_pm(const ModelArgs&) { return nullptr; }
__device__ __forceinline__ const signed char* map_pm(const ModelMapArgs& A) { return A.pm; }
// What row_put needs of an affine instance's arguments: pm[] and ratio[], both indexed by the model's column.  The terms
// below take the map as a deduced type PM: const signed char* (as map_pm gives it) or this pair.
struct TieMap { const signed char* pm; const double* ratio; };
template <class Base> __device__ __forceinline__ TieMap map_pm(const TieArgs<Base>& A) { return {A.pm, A.ratio}; }
__device__ __forceinline__ const double* map_pfix(const ModelArgs&) { return nullptr; }
__device__ __forceinline__ const double* map_pfix(const ModelMapArgs& A) { return A.Pfix; }

// row[k] = v of model_row.  Unmapped: the plain store.  Mapped: into the slot of column k (columns arrive in ascending k).
template <bool MAPPED>
__device__ __forceinline__ void row_put(double* row, const signed char* pm, int k, double v) {
  if (!MAPPED) {
    row[k] = v;
  } else {
    const int c = pm[k];
    if (c >= MODEL_ROWS) row[c - MODEL_ROWS] = row[c - MODEL_ROWS] + v;
    else if (c >= 0) row[c] = v;
  }
}
// Affine: the mapped put of ratio[k] * v.  k is wave-uniform, so ratio[k] is a scalar load from the kernel arguments.
template <bool MAPPED>
__device__ __forceinline__ void row_put(double* row, TieMap map, int k, double v) {
  row_put<true>(row, map.pm, k, map.ratio[k] * v);
}

// ---- the terms.  Each evaluates one term whose parameters start at p[o], writes its columns o .. of the lane's J row
// through row_put (row == nullptr: f only) and returns the term's value.
#define PUT(k, v) row_put<MAPPED>(row, pm, (k), (v))
template <bool MAPPED, class PM>
__device__ __forceinline__ double exp_term(const double* __restrict__ p, int o, double t, double wi, double* row,
                                           PM pm) {
  const double a = p[o], r = p[o + 1];
  const double e = exp(-(r * t));
  const double g = a * e;
  if (row) { PUT(o, wi * e); PUT(o + 1, wi * (-(t * g))); }
  return g;
}

template <bool LORENTZ, bool MAPPED, class PM>
__device__ __forceinline__ double peak_term(const double* __restrict__ p, int o, double t, double wi, double* row,
                                            PM pm) {
  const double a = p[o], mu = p[o + 1], s = p[o + 2];
  const double z = (t - mu) / s;
  double e, g, dmu;
  if (!LORENTZ) {
    e = exp(-0.5 * (z * z));
    g = a * e;
    dmu = (g * z) / s;
  } else {
    e = 1.0 / (1.0 + z * z);
    g = a * e;
    dmu = (((2.0 * g) * e) * z) / s;
  }
  if (row) { PUT(o, wi * e); PUT(o + 1, wi * dmu); PUT(o + 2, wi * (dmu * z)); }
  return g;
}

// pseudo-Voigt (a, mu, s, eta): s is the half width at half maximum of both parts (the operations)
template <bool MAPPED, class PM>
__device__ __forceinline__ double pvoigt_term(const double* __restrict__ p, int o, double t, double wi, double* row,
                                              PM pm) {
  constexpr double LN2 = 0.6931471805599453;
  const double a = p[o], mu = p[o + 1], s = p[o + 2], eta = p[o + 3];
  const double z = (t - mu) / s;
  const double q = z * z;
  const double G = exp(-(LN2 * q));
  const double L = 1.0 / (1.0 + q);
  const double d = L - G;
  const double h = G + eta * d;
  if (row) {
    const double lg = LN2 * G;
    const double u = lg + eta * (L * L - lg);
    const double dmu = (((2.0 * a) * u) * z) / s;
    PUT(o, wi * h); PUT(o + 1, wi * dmu); PUT(o + 2, wi * (dmu * z)); PUT(o + 3, wi * (a * d));
  }
  return a * h;
}

// polynomial of d coefficients p[o .. o + d): the value by Horner, the columns t^k by repeated product
template <bool MAPPED, class PM>
__device__ __forceinline__ double poly_terms(const double* __restrict__ p, int o, int d, double t, double wi,
                                             double* row, PM pm) {
  double acc = p[o + d - 1];
  for (int k = d - 2; k >= 0; --k) acc = acc * t + p[o + k];          // Horner
  if (row) {
    double pw = 1.0;
    for (int k = 0; k < d; ++k) { PUT(o + k, wi * pw); pw = pw * t; }
  }
  return acc;
}

// ---- the bin-integrated terms (models.erf_diff, models.psi_pair and the _bfill_* functions)
static constexpr double SQRT_HALF = 0.7071067811865476;     // 1 / sqrt(2)
static constexpr double SQRT_PI_2 = 1.2533141373155001;     // sqrt(pi / 2)
static constexpr double SQRT_LN2 = 0.8325546111576977;      // sqrt(ln 2)
static constexpr double PV_GNORM = 1.0644670194312262;      // sqrt(pi / ln 2) / 2
static constexpr double PSI_X0 = 0.5;
static constexpr int PSI_TERMS = 16;

// erf(xh) - erf(xl): by erfc of the magnitudes where both arguments lie in one tail (no cancellation against 1)
__device__ __forceinline__ double erf_diff(double xl, double xh) {
  if (xl > 0.0 && xh > 0.0) return erfc(xl) - erfc(xh);
  if (xl < 0.0 && xh < 0.0) return erfc(-xh) - erfc(-xl);
  return erf(xh) - erf(xl);
}

__host__ __device__ constexpr double psi_fact(int k) {
  double v = 1.0;
  for (int i = 2; i <= k; ++i) v = v * (double)i;
  return v;
}

// psi(x) = -expm1(-x) / x and psi'(x) = (x exp(-x) + expm1(-x)) / x^2: as written where |x| >= PSI_X0, by PSI_TERMS terms
// of their series below (Horner; the coefficients are constants folded at compile time)
__device__ __forceinline__ void psi_pair(double x, double& ps, double& dp) {
  if (fabs(x) < PSI_X0) {
    ps = ((PSI_TERMS - 1) & 1 ? -1.0 : 1.0) / psi_fact(PSI_TERMS);
    dp = ((PSI_TERMS & 1 ? -1.0 : 1.0) * (double)PSI_TERMS) / psi_fact(PSI_TERMS + 1);
#pragma unroll
    for (int k = PSI_TERMS - 2; k >= 0; --k) {
      ps = ps * x + (k & 1 ? -1.0 : 1.0) / psi_fact(k + 1);
      dp = dp * x + (((k + 1) & 1 ? -1.0 : 1.0) * (double)(k + 1)) / psi_fact(k + 2);
    }
  } else {
    const double em = expm1(-x);
    ps = -em / x;
    dp = (x * exp(-x) + em) / (x * x);
  }
}

template <bool MAPPED, class PM>
__device__ __forceinline__ double exp_bin(const double* __restrict__ p, int o, double lo, double hi, double wi,
                                          double* row, PM pm) {
  const double a = p[o], r = p[o + 1];
  const double w = hi - lo;
  double ps, dp;
  psi_pair(r * w, ps, dp);
  const double wE = w * exp(-(r * lo));
  const double da = wE * ps;
  if (row) { PUT(o, wi * da); PUT(o + 1, wi * ((a * wE) * (w * dp - lo * ps))); }
  return a * da;
}

template <bool LORENTZ, bool MAPPED, class PM>
__device__ __forceinline__ double peak_bin(const double* __restrict__ p, int o, double lo, double hi, double wi,
                                           double* row, PM pm) {
  const double a = p[o], mu = p[o + 1], s = p[o + 2];
  const double zl = (lo - mu) / s, zh = (hi - mu) / s;
  double da;
  if (!LORENTZ) da = (s * SQRT_PI_2) * erf_diff(zl * SQRT_HALF, zh * SQRT_HALF);
  else da = s * atan2((hi - lo) / s, 1.0 + zh * zl);
  const double g = a * da;
  if (row) {
    double el, eh;
    if (!LORENTZ) { el = exp(-0.5 * (zl * zl)); eh = exp(-0.5 * (zh * zh)); }
    else { el = 1.0 / (1.0 + zl * zl); eh = 1.0 / (1.0 + zh * zh); }
    PUT(o, wi * da);
    PUT(o + 1, wi * (a * (el - eh)));
    PUT(o + 2, wi * (g / s - a * (zh * eh - zl * el)));
  }
  return g;
}

template <bool MAPPED, class PM>
__device__ __forceinline__ double pvoigt_bin(const double* __restrict__ p, int o, double lo, double hi, double wi,
                                             double* row, PM pm) {
  constexpr double LN2 = 0.6931471805599453;
  const double a = p[o], mu = p[o + 1], s = p[o + 2], eta = p[o + 3];
  const double zl = (lo - mu) / s, zh = (hi - mu) / s;
  const double IG = (s * PV_GNORM) * erf_diff(zl * SQRT_LN2, zh * SQRT_LN2);
  const double IL = s * atan2((hi - lo) / s, 1.0 + zh * zl);
  const double d = IL - IG;
  const double h = IG + eta * d;
  const double g = a * h;
  if (row) {
    const double ql = zl * zl, qh = zh * zh;
    const double Gl = exp(-(LN2 * ql)), Gh = exp(-(LN2 * qh));
    const double Ll = 1.0 / (1.0 + ql), Lh = 1.0 / (1.0 + qh);
    const double mG = Gl - Gh;
    const double uG = zh * Gh - zl * Gl;
    PUT(o, wi * h);
    PUT(o + 1, wi * (a * (mG + eta * ((Ll - Lh) - mG))));
    PUT(o + 2, wi * (g / s - a * (uG + eta * ((zh * Lh - zl * Ll) - uG))));
    PUT(o + 3, wi * (a * d));
  }
  return g;
}

// polynomial of d coefficients over the bin: column k is (hi^(k+1) - lo^(k+1)) / (k + 1), the powers by repeated product;
// the value the sequential sum of p_k times its column
template <bool MAPPED, class PM>
__device__ __forceinline__ double poly_bin(const double* __restrict__ p, int o, int d, double lo, double hi, double wi,
                                           double* row, PM pm) {
  double ph = hi, pl = lo, acc = 0.0;
  for (int k = 0; k < d; ++k) {
    const double c = (ph - pl) / (double)(k + 1);
    if (row) PUT(o + k, wi * c);
    const double v = p[o + k] * c;
    acc = (k == 0) ? v : acc + v;
    ph = ph * hi; pl = pl * lo;
  }
  return acc;
}

// The bin-integrated terms of one row of a named model: the family's terms and 'poly*1', as the composite walks them.
template <int MODEL, bool MAPPED, class PM>
__device__ __forceinline__ double model_row_bin(int n, int m, const double* __restrict__ tb, int i,
                                                const double* __restrict__ p, double wi, double* row,
                                                PM pm) {
  const double lo = tb[i], hi = tb[m + i];
  if (MODEL == BLSQ_MODEL_POLY) return poly_bin<MAPPED>(p, 0, n, lo, hi, wi, row, pm);
  if (MODEL == BLSQ_MODEL_EXP_SUM) {
    const int K = (n - 1) / 2;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double g = exp_bin<MAPPED>(p, 2 * k, lo, hi, wi, row, pm);
      acc = (k == 0) ? g : acc + g;
    }
    return acc + poly_bin<MAPPED>(p, n - 1, 1, lo, hi, wi, row, pm);
  }
  if (MODEL == BLSQ_MODEL_GAUSS_SUM || MODEL == BLSQ_MODEL_LORENTZ_SUM) {
    const int K = (n - 1) / 3;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double g = peak_bin<MODEL == BLSQ_MODEL_LORENTZ_SUM, MAPPED>(p, 3 * k, lo, hi, wi, row, pm);
      acc = (k == 0) ? g : acc + g;
    }
    return acc + poly_bin<MAPPED>(p, n - 1, 1, lo, hi, wi, row, pm);
  }
  // BLSQ_MODEL_GAUSS2D: t is [4][m], the pixel [lo, hi] x [vlo, vhi]
  const double vlo = tb[2 * m + i], vhi = tb[3 * m + i];
  const double a = p[0], u0 = p[1], v0 = p[2], s = p[3], c = p[4];
  const double zul = (lo - u0) / s, zuh = (hi - u0) / s;
  const double zvl = (vlo - v0) / s, zvh = (vhi - v0) / s;
  const double c1 = s * SQRT_PI_2;
  const double Iu = c1 * erf_diff(zul * SQRT_HALF, zuh * SQRT_HALF);
  const double Iv = c1 * erf_diff(zvl * SQRT_HALF, zvh * SQRT_HALF);
  const double da = Iu * Iv;
  const double ww = (hi - lo) * (vhi - vlo);
  if (row) {
    const double eul = exp(-0.5 * (zul * zul)), euh = exp(-0.5 * (zuh * zuh));
    const double evl = exp(-0.5 * (zvl * zvl)), evh = exp(-0.5 * (zvh * zvh));
    PUT(0, wi * da);
    PUT(1, wi * ((a * (eul - euh)) * Iv));
    PUT(2, wi * ((a * (evl - evh)) * Iu));
    PUT(3, wi * (a * ((Iu / s - (zuh * euh - zul * eul)) * Iv + Iu * (Iv / s - (zvh * evh - zvl * evl)))));
    PUT(4, wi * ww);
  }
  return a * da + c * ww;
}

// The terms of one row.  `row` is the lane's slice of the wave's LDS tile (nullptr: f only); returns the model value.
template <int MODEL, bool MAPPED, class PM>
__device__ __forceinline__ double model_row(int n, int m, const double* __restrict__ tb, int i,
                                            const double* __restrict__ p, double wi, double* row,
                                            PM pm) {
  if (MODEL == BLSQ_MODEL_POLY) return poly_terms<MAPPED>(p, 0, n, tb[i], wi, row, pm);
  if (MODEL == BLSQ_MODEL_EXP_SUM) {
    const double t = tb[i];
    const int K = (n - 1) / 2;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double g = exp_term<MAPPED>(p, 2 * k, t, wi, row, pm);
      acc = (k == 0) ? g : acc + g;
    }
    if (row) PUT(n - 1, wi);
    return acc + p[n - 1];
  }
  if (MODEL == BLSQ_MODEL_GAUSS_SUM || MODEL == BLSQ_MODEL_LORENTZ_SUM) {
    const double t = tb[i];
    const int K = (n - 1) / 3;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double g = peak_term<MODEL == BLSQ_MODEL_LORENTZ_SUM, MAPPED>(p, 3 * k, t, wi, row, pm);
      acc = (k == 0) ? g : acc + g;
    }
    if (row) PUT(n - 1, wi);
    return acc + p[n - 1];
  }
  // BLSQ_MODEL_GAUSS2D: t is [2][m]
  const double du = tb[i] - p[1], dv = tb[m + i] - p[2];
  const double a = p[0], s = p[3];
  const double r2 = du * du + dv * dv, s2 = s * s;
  const double e = exp(-0.5 * (r2 / s2));
  const double g = a * e;
  if (row) {
    PUT(0, wi * e);
    PUT(1, wi * ((g * du) / s2));
    PUT(2, wi * ((g * dv) / s2));
    PUT(3, wi * ((g * r2) / (s2 * s)));
    PUT(4, wi);
  }
  return g + p[4];
}
#undef PUT

// The row of a composite: the walk over the table.  c, fam, cnt and the offset o are wave-uniform.
// BINNED: t is lo and hi the bin's upper edge; otherwise hi is not read.
template <bool MAPPED, bool BINNED, class PM>
__device__ __forceinline__ double comp_row(const CompTable& tab, double t, double hi, const double* __restrict__ p,
                                           double wi, double* row, PM pm) {
  double acc = 0.0;
  int o = 0;                                   // first parameter, and first column, of the component
  unsigned long long ent = tab.lo;
  for (int c = 0; c < tab.ncomp; ++c, ent >>= 16) {
    if (c == 4) ent = tab.hi;
    const int fam = (int)(ent & 0xff), cnt = (int)((ent >> 8) & 0xff);
    double v = 0.0;
    switch (fam) {
      case BLSQ_TERM_GAUSS:
        for (int k = 0; k < cnt; ++k, o += 3) {
          const double g = BINNED ? peak_bin<false, MAPPED>(p, o, t, hi, wi, row, pm)
                                  : peak_term<false, MAPPED>(p, o, t, wi, row, pm);
          v = (k == 0) ? g : v + g;
        }
        break;
      case BLSQ_TERM_LORENTZ:
        for (int k = 0; k < cnt; ++k, o += 3) {
          const double g = BINNED ? peak_bin<true, MAPPED>(p, o, t, hi, wi, row, pm)
                                  : peak_term<true, MAPPED>(p, o, t, wi, row, pm);
          v = (k == 0) ? g : v + g;
        }
        break;
      case BLSQ_TERM_PVOIGT:
        for (int k = 0; k < cnt; ++k, o += 4) {
          const double g = BINNED ? pvoigt_bin<MAPPED>(p, o, t, hi, wi, row, pm)
                                  : pvoigt_term<MAPPED>(p, o, t, wi, row, pm);
          v = (k == 0) ? g : v + g;
        }
        break;
      case BLSQ_TERM_EXP:
        for (int k = 0; k < cnt; ++k, o += 2) {
          const double g = BINNED ? exp_bin<MAPPED>(p, o, t, hi, wi, row, pm)
                                  : exp_term<MAPPED>(p, o, t, wi, row, pm);
          v = (k == 0) ? g : v + g;
        }
        break;
      default:                                 // BLSQ_TERM_POLY (the host has checked the table)
        v = BINNED ? poly_bin<MAPPED>(p, o, cnt, t, hi, wi, row, pm)
                   : poly_terms<MAPPED>(p, o, cnt, t, wi, row, pm);
        o += cnt;
        break;
    }
    acc = (c == 0) ? v : acc + v;
  }
  return acc;
}

template <int MODEL, int MAP, bool POISSON, bool BINNED, bool OMIT, bool AFFINE>
__global__ __launch_bounds__(256) void model_eval_kernel(
    typename ModelArgsOf<MODEL == MODEL_COMPOSITE, MAP, AFFINE>::type A) {
  static_assert(!AFFINE || MAP != MAP_NONE, "an affine tie is part of a map");
  constexpr bool MAPPED = MAP != MAP_NONE, GLOBAL = MAP == MAP_GLOBAL;
  extern __shared__ double model_tiles[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);            // wave-uniform, in a scalar register
  const int wpb = blockDim.x >> 6;
  const long item = (long)blockIdx.x * wpb + wave;
  bool live = item < A.items;
  long q = 0;
  int r0 = 0;
  if (live) {
    q = item / A.tiles;
    r0 = (int)(item - q * A.tiles) * MODEL_ROWS;
  }
  // global: the items of a point run over its S data sets, so q counts (point, data set) pairs: the row blocks of f and
  // J.  qx is the point, g its group (the index of mask) and b the data set among all G S (the index of y, w and Pfix).
  long b = q / A.reps, g = b, qx = q;
  int s = 0;
  if constexpr (GLOBAL) {
    qx = q / A.S;
    s = (int)(q - qx * A.S);
    g = qx / A.reps;
    b = g * A.S + s;
  }
  if (live && A.mask && A.mask[g] == 0) live = false;                           // a masked problem is left untouched
  const int n = A.n, m = A.m;
  const int nc = map_nf(A);                                                     // columns of J: n, or nf when mapped
  const int ld = nc | 1;
  const int nr = live ? min(MODEL_ROWS, m - r0) : 0;
  // mapped: the waves' parameter vectors (64 doubles each) lie in front of the tiles
  double* tiles = MAPPED ? model_tiles + (size_t)wpb * MODEL_ROWS : model_tiles;
  double* tile = A.J ? tiles + (size_t)wave * MODEL_ROWS * ld : nullptr;
  const double* p = A.P + q * nc;
  if constexpr (GLOBAL) p = A.P + qx * A.nv;
  if constexpr (MAPPED) {
    double* pv = model_tiles + (size_t)wave * MODEL_ROWS;
    if (live && lane < n) {
      const int c = A.pm[lane];
      int k = c & (MODEL_ROWS - 1);
      if constexpr (GLOBAL) k = k < A.ns ? k : k + s * A.nl;                    // a local slot: data set s's window
      if constexpr (AFFINE) {              // r v + d, the product first; a plain copy where (r, d) == (1, 0)
        double v;
        if (c < 0) {
          v = map_pfix(A)[b * n + lane];
        } else {
          v = p[k];
          const double r = A.ratio[lane], d = A.offset[lane];
          if (r != 1.0 || d != 0.0) v = r * v + d;
        }
        pv[lane] = v;
      } else {
        pv[lane] = c < 0 ? map_pfix(A)[b * n + lane] : p[k];
      }
    }
    __syncthreads();                       // (the wave reads only its own vector; every wave arrives)
    p = pv;
  }
  if (lane < nr) {
    const int i = r0 + lane;
    bool omitted = false;
    if constexpr (OMIT) {                  // a NaN in y leaves the row out: zeros, and nothing of the row is read
      const double yi = A.y[b * m + i];
      omitted = yi != yi;
      if (omitted) {
        if (tile)
          for (int k = 0; k < nc; ++k) tile[lane * ld + k] = 0.0;
        if (A.f) A.f[q * m + i] = 0.0;
      }
    }
    if (!omitted) {
      const double* tb = A.t + g * A.t_stride;
      if constexpr (GLOBAL) tb += s * A.t_sstride;
      const double wi = (!POISSON && A.w) ? A.w[b * A.w_stride + i] : 1.0;
      double* row = tile ? tile + lane * ld : nullptr;
      double v;
      if constexpr (MODEL == MODEL_COMPOSITE && BINNED)
        v = comp_row<MAPPED, true>(A.tab, tb[i], tb[m + i], p, wi, row, map_pm(A));
      else if constexpr (MODEL == MODEL_COMPOSITE)
        v = comp_row<MAPPED, false>(A.tab, tb[i], 0.0, p, wi, row, map_pm(A));
      else if constexpr (BINNED) v = model_row_bin<MODEL, MAPPED>(n, m, tb, i, p, wi, row, map_pm(A));
      else v = model_row<MODEL, MAPPED>(n, m, tb, i, p, wi, row, map_pm(A));
      if constexpr (POISSON) {
        double r, c;
        poisson_rc(v, A.y[b * m + i], r, c);
        if (A.f) A.f[q * m + i] = r;
        if (row)
          for (int k = 0; k < nc; ++k) row[k] = c * row[k];
      } else if (A.f) {
        const double r = A.y ? v - A.y[b * m + i] : v;
        A.f[q * m + i] = A.w ? wi * r : r;
      }
    }
  }
  if constexpr (GLOBAL) {
    if (A.J) {
      __syncthreads();
      // the wave's rows are the contiguous block J[g][s m + r0 .. + nr)[0 .. nv): consecutive lanes on consecutive
      // addresses; an element comes from the tile where its column is a shared one or lies in data set s's window
      // (tile column = column - s nl there) and is +0.0 elsewhere
      const int nv = A.nv, ns = A.ns, off = s * A.nl;
      double* out = A.J + (q * m + r0) * (long)nv;
      const int total = nr * nv;
      int row = lane / nv, col = lane - row * nv;
      const int drow = WAVE / nv, dcol = WAVE - drow * nv;
      for (int e = lane; e < total; e += WAVE) {
        const int k = col < ns ? col : col - off;
        out[e] = (k < nc && (col < ns || k >= ns)) ? tile[row * ld + k] : 0.0;
        row += drow; col += dcol;
        if (col >= nv) { col -= nv; ++row; }
      }
    }
  } else if (A.J) {
    __syncthreads();                       // (every wave of the workgroup arrives: no early return above)
    // the wave's rows are the contiguous block J[q][r0 .. r0 + nr)[0 .. nc): lane l takes elements l, l + 64, ...
    double* out = A.J + (q * m + r0) * (long)nc;
    const int total = nr * nc;
    int row = lane / nc, col = lane - row * nc;
    const int drow = WAVE / nc, dcol = WAVE - drow * nc;
    for (int e = lane; e < total; e += WAVE) {
      out[e] = tile[row * ld + col];
      row += drow; col += dcol;
      if (col >= nc) { col -= nc; ++row; }
    }
  }
}

// The launch of instance <MODEL, MAP, AFFINE> with the flags `inst`: POISSON | BINNED << 1 | OMIT << 2.  The eight
// kernels take the same arguments: the part of `all` that the instance has.
// Instance <MODEL, MAP, AFFINE> with the flags; nullptr for the bin-integrated global instances, which are not built.
using AllModelArgs = TieArgs<CompArgs<ModelGlobalArgs>>;
template <int MODEL, int MAP, bool AFFINE, bool POISSON, bool BINNED, bool OMIT>
static constexpr auto model_instance() -> void (*)(typename ModelArgsOf<MODEL == MODEL_COMPOSITE, MAP, AFFINE>::type) {
  if constexpr (MAP == MAP_GLOBAL && BINNED) return nullptr;
  else return model_eval_kernel<MODEL, MAP, POISSON, BINNED, OMIT, AFFINE>;
}

template <int MODEL, int MAP, bool AFFINE>
static hipError_t launch_model_instance(int inst, dim3 g, dim3 blk, size_t lds, hipStream_t s,
                                        const AllModelArgs& all) {
  using Args = typename ModelArgsOf<MODEL == MODEL_COMPOSITE, MAP, AFFINE>::type;
  static void (*const kernels[8])(Args) = {
      model_instance<MODEL, MAP, AFFINE, false, false, false>(), model_instance<MODEL, MAP, AFFINE, true, false, false>(),
      model_instance<MODEL, MAP, AFFINE, false, true, false>(),  model_instance<MODEL, MAP, AFFINE, true, true, false>(),
      model_instance<MODEL, MAP, AFFINE, false, false, true>(),  model_instance<MODEL, MAP, AFFINE, true, false, true>(),
      model_instance<MODEL, MAP, AFFINE, false, true, true>(),   model_instance<MODEL, MAP, AFFINE, true, true, true>()};
  if (!kernels[inst]) return hipErrorInvalidValue;
  Args A;
  static_cast<typename ModelArgsBase<false, MAP>::type&>(A) = all;
  if constexpr (MODEL == MODEL_COMPOSITE) A.tab = all.tab;
  if constexpr (AFFINE)
    for (int j = 0; j < MODEL_ROWS; ++j) { A.ratio[j] = all.ratio[j]; A.offset[j] = all.offset[j]; }
  hipLaunchKernelGGL(kernels[inst], g, blk, lds, s, A);
  return hipGetLastError();
}

template <int MAP, bool AFFINE>
static hipError_t launch_model_kind(int model, int inst, dim3 g, dim3 blk, size_t lds, hipStream_t s,
                                    const AllModelArgs& all) {
  switch (model) {
    case MODEL_COMPOSITE: return launch_model_instance<MODEL_COMPOSITE, MAP, AFFINE>(inst, g, blk, lds, s, all);
    case BLSQ_MODEL_POLY: return launch_model_instance<BLSQ_MODEL_POLY, MAP, AFFINE>(inst, g, blk, lds, s, all);
    case BLSQ_MODEL_EXP_SUM: return launch_model_instance<BLSQ_MODEL_EXP_SUM, MAP, AFFINE>(inst, g, blk, lds, s, all);
    case BLSQ_MODEL_GAUSS_SUM: return launch_model_instance<BLSQ_MODEL_GAUSS_SUM, MAP, AFFINE>(inst, g, blk, lds, s, all);
    case BLSQ_MODEL_LORENTZ_SUM:
      return launch_model_instance<BLSQ_MODEL_LORENTZ_SUM, MAP, AFFINE>(inst, g, blk, lds, s, all);
    case BLSQ_MODEL_GAUSS2D:                                 // two coordinates: no global instance
      if constexpr (MAP == MAP_GLOBAL) return hipErrorInvalidValue;
      else return launch_model_instance<BLSQ_MODEL_GAUSS2D, MAP, AFFINE>(inst, g, blk, lds, s, all);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_model_eval(const ModelEvalCall& c, hipStream_t s) {
  const bool poisson = c.est == BLSQ_EST_POISSON, bin = c.sampling == BLSQ_SAMPLE_BIN, omit = c.nan_policy == BLSQ_NAN_OMIT;
  if ((!poisson && c.est != BLSQ_EST_LSE) || (!bin && c.sampling != BLSQ_SAMPLE_POINT) ||
      (!omit && c.nan_policy != BLSQ_NAN_PROPAGATE))
    return hipErrorInvalidValue;
  if (((poisson || omit) && !c.y) || (poisson && c.w)) return hipErrorInvalidValue;   // both read y; Poisson takes no w
  if (c.n < 1 || c.n > MODEL_ROWS) return hipErrorInvalidValue;
  const bool global = c.S > 0;
  if (global && (bin || !c.pmap || !c.shared)) return hipErrorInvalidValue;
  const bool affine = c.tie_ratio || c.tie_offset;
  if (affine && (!c.tie_ratio || !c.tie_offset || !c.pmap)) return hipErrorInvalidValue;
  AllModelArgs A;
  A.m = c.m; A.n = c.n; A.reps = c.reps; A.tiles = (c.m + MODEL_ROWS - 1) / MODEL_ROWS;
  A.items = (long)c.B * c.reps * (global ? c.S : 1) * A.tiles;
  A.t = c.t; A.t_stride = c.t_stride; A.y = c.y; A.w = c.w; A.w_stride = c.w_stride; A.P = c.X; A.f = c.f; A.J = c.J;
  A.mask = c.mask;
  int nc = c.n;                                      // columns of J
  if (c.pmap) {                                      // nf, Pfix and pm[] from the host's pmap [n]
    nc = A.nf = c.nf; A.Pfix = c.Pfix;
    if (c.nf < 1 || c.nf > c.n) return hipErrorInvalidValue;
    int slot[MODEL_ROWS];                            // the tile column of slot k: k, or (global) the shared slots first
    for (int k = 0; k < c.nf; ++k) slot[k] = k;
    if (global) {
      int ns = 0, nl = 0;
      for (int k = 0; k < c.nf; ++k) ns += c.shared[k] != 0;
      A.S = c.S; A.ns = ns; A.nl = c.nf - ns; A.t_sstride = c.t_sstride;
      const long nv = ns + (long)c.S * A.nl;
      if (nv > BLSQ_GLOBAL_MAX_NV) return hipErrorInvalidValue;
      A.nv = (int)nv;
      A.w_stride = c.w_stride ? c.m : 0;             // per data set: the rows of [B][S m] are [B S][m]
      for (int k = 0, sh = 0; k < c.nf; ++k) slot[k] = c.shared[k] ? sh++ : ns + nl++;
    }
    bool seen[MODEL_ROWS] = {};
    for (int j = 0; j < MODEL_ROWS; ++j) {
      int k = -1;
      if (j < c.n && c.pmap[j] >= 0) {
        if (c.pmap[j] >= c.nf) return hipErrorInvalidValue;
        k = seen[c.pmap[j]] ? MODEL_ROWS + slot[c.pmap[j]] : slot[c.pmap[j]];
        seen[c.pmap[j]] = true;
      }
      A.pm[j] = (signed char)k;
      A.ratio[j] = (affine && k >= 0) ? c.tie_ratio[j] : 1.0;      // entries of fixed parameters are not read
      A.offset[j] = (affine && k >= 0) ? c.tie_offset[j] : 0.0;
    }
  }
  A.tab = {};
  if (c.model == MODEL_COMPOSITE) {
    if (c.ncomp < 1 || c.ncomp > BLSQ_MODEL_MAX_COMP) return hipErrorInvalidValue;
    A.tab.ncomp = c.ncomp;
    int total = 0;
    for (int k = 0; k < c.ncomp; ++k) {
      const int fam = c.fam[k], cnt = c.cnt[k];
      if (fam < 0 || fam > BLSQ_TERM_POLY || cnt < 1 || cnt > MODEL_ROWS) return hipErrorInvalidValue;
      (k < 4 ? A.tab.lo : A.tab.hi) |= (unsigned long long)(fam | (cnt << 8)) << (16 * (k & 3));
      total += cnt * MODEL_TERM_PARAMS[fam];
    }
    if (total != c.n) return hipErrorInvalidValue;   // the kernel's offsets stay inside the n parameters and columns
  }
  // LDS of one wave: mapped, its parameter vector; with J, its tile at row stride nc | 1.  Waves per workgroup: 4 / 2 / 1
  const size_t wave_bytes = sizeof(double) * MODEL_ROWS * (size_t)((c.pmap ? 1 : 0) + (c.J ? (nc | 1) : 0));
  int wpb = 4;
  while (wpb > 1 && wave_bytes * wpb > (size_t)MODEL_LDS_BYTES) wpb >>= 1;
  if (wave_bytes * wpb > (size_t)MODEL_LDS_BYTES) return hipErrorInvalidValue;
  const long grid = (A.items + wpb - 1) / wpb;
  if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
  const int inst = (int)poisson | (int)bin << 1 | (int)omit << 2;
  const dim3 g((unsigned)grid), blk(64 * wpb);
  const size_t lds = wave_bytes * wpb;
  if (affine)
    return global ? launch_model_kind<MAP_GLOBAL, true>(c.model, inst, g, blk, lds, s, A)
                  : launch_model_kind<MAP_PARAM, true>(c.model, inst, g, blk, lds, s, A);
  if (global) return launch_model_kind<MAP_GLOBAL, false>(c.model, inst, g, blk, lds, s, A);
  return c.pmap ? launch_model_kind<MAP_PARAM, false>(c.model, inst, g, blk, lds, s, A)
                : launch_model_kind<MAP_NONE, false>(c.model, inst, g, blk, lds, s, A);
}

}  // namespace blsq
