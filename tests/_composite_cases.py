"""Inputs shared by tests/test_composite_cpu.py and tests/test_composite_gpu.py: the specs and seeded evaluation points
of the kernel-level comparisons, the rounding-error bound of one evaluation of a composite model (the derivation is in
the docstring of test_composite_gpu.py::test_kernel_against_longdouble) and the seeded fit problems of the end-to-end
tests."""
import numpy as np

from bounded_lsq import models

from _model_cases import worst_ratio  # noqa: F401  (the case modules hand it on)

LD = np.longdouble
EPS = np.finfo(float).eps

# the specs of the kernel-level tests: component order, every family, n = 64 (one wave per workgroup), 8 components
EIGHT = "gauss+lorentz+pvoigt+exp+poly*2+gauss+lorentz*2+poly*1"
KERNEL_SPECS = ["gauss+poly*2", "poly*1+gauss", "exp*2+poly*1", "gauss*2+lorentz+pvoigt+poly*3", "pvoigt*15+poly*4",
                EIGHT]
ROWS = [1, 63, 64, 65, 130]
# the variants of one (spec, m): B, per-problem t, reps, w (None / 1: shared / 2: per problem), y given
VARIANTS = [(B, pp, reps, wk, yk) for B in (1, 3) for pp in (False, True) for reps in (1, 3) for wk in (None, 1, 2)
            for yk in (False, True)]

# rounding counts of a pseudo-Voigt term (the docstring named above): its value, and its columns a, mu, s, eta
PV_F, PV_J = 13, (11, 24, 27, 10)


def _columns(M):
    """(family, index within the term or None for poly) of every parameter."""
    out = []
    for fam, K in M.components:
        w = models.TERMS[fam].n_per_term
        out += [(fam, None if fam == "poly" else i % w) for i in range(K * w)]
    return out


def comp_inputs(spec, B, m, seed=0, per_problem=False):
    """As _model_cases.case_inputs: amplitudes, widths, rates and coefficients in [0.5, 1.5], centres in [-1.5, 1.5]
    inside the coordinate range [-2, 2] ([0, 4] for a spec of decays without peaks); eta uniform in [0.1, 0.9]."""
    rng = np.random.default_rng(seed)
    M = models.compose(spec)
    P = rng.uniform(0.5, 1.5, (B, M.n))
    cols = _columns(M)
    mu = [j for j, (fam, i) in enumerate(cols) if fam in ("gauss", "lorentz", "pvoigt") and i == 1]
    eta = [j for j, (fam, i) in enumerate(cols) if fam == "pvoigt" and i == 3]
    P[:, mu] = rng.uniform(-1.5, 1.5, (B, len(mu)))
    P[:, eta] = rng.uniform(0.1, 0.9, (B, len(eta)))
    fams = {fam for fam, K in M.components}
    lo, hi = (0.0, 4.0) if "exp" in fams and not fams & {"gauss", "lorentz", "pvoigt"} else (-2.0, 2.0)
    x = np.sort(rng.uniform(lo, hi, ((B,) if per_problem else ()) + (m,)), axis=-1)
    return x, P


def magnitudes(spec, x, P):
    """In np.longdouble, for P (Q, n) and x broadcastable against it: per summand of the model (every term, every
    monomial of a polynomial) the magnitude ``T`` (Q, m, S) its error is bounded relative to, the exponent's argument
    ``A`` (Q, m, S) (0 where there is none) and the rounding count ``cf`` (S,); per column of the Jacobian the magnitude
    ``Jm`` (Q, m, n), the count ``cj`` (n,) and ``col_term`` (n,), the summand whose argument enters it; and S."""
    M = models.compose(spec)
    P = np.asarray(P, dtype=LD)
    x = np.asarray(x, dtype=LD)
    Jref = M.jac(x, P)
    Jm = np.abs(Jref)
    col = lambda k: P[:, k, np.newaxis]                                            # noqa: E731
    T, A, cf, cj, col_term = [], [], [], [], []
    o = 0
    for fam, K in M.components:
        for k in range(K):
            s_idx = len(T)
            if fam == "poly":
                T.append(np.abs(col(o) * x ** k + 0 * x))
                A.append(0 * T[-1])
                cf.append(4); cj.append(8); col_term.append(s_idx)
                o += 1
                continue
            if fam == "exp":
                arg = -(col(o + 1) * x)
                T.append(np.abs(col(o) * np.exp(arg)))
                cj += [8, 8]
            else:
                z = (x - col(o + 1)) / col(o + 2)
                if fam == "gauss":
                    arg = -z * z / 2
                    T.append(np.abs(col(o) * np.exp(arg)))
                    cj += [8, 8, 8]
                elif fam == "lorentz":
                    arg = 0 * z
                    T.append(np.abs(col(o) / (1 + z * z)))
                    cj += [8, 8, 8]
                else:                                            # pvoigt: relative to the sums of absolute values
                    a, s, eta = np.abs(col(o)), np.abs(col(o + 2)), np.abs(col(o + 3))
                    q = z * z
                    arg = -(LD(models.LN2) * q)
                    G, L = np.exp(arg), 1 / (1 + q)
                    lg = LD(models.LN2) * G
                    Sh = G + eta * (L + G)
                    Su = lg + eta * (L * L + lg)
                    T.append(a * Sh)
                    Jm[:, :, o] = Sh + 0 * x
                    Jm[:, :, o + 1] = 2 * a * np.abs(z) / s * Su
                    Jm[:, :, o + 2] = 2 * a * q / s * Su
                    Jm[:, :, o + 3] = a * (L + G)
                    cj += list(PV_J)
            A.append(arg + 0 * T[-1])
            cf.append(PV_F if fam == "pvoigt" else 4)
            w = models.TERMS[fam].n_per_term
            col_term += [s_idx] * w
            o += w
    return (np.stack(T, axis=-1), np.stack(A, axis=-1), np.array(cf), Jm, np.array(cj), np.array(col_term), len(T))


def bounds_of(spec, x, P, w, y, reps=1):
    """The allowed error of every entry of f (Q, m) and of J (Q, m, n) with the longdouble references:
    -> f_ref, J_ref, f_tol, J_tol.  w: None, (m,) or (B, m); y: None or (B, m); Q = B * reps."""
    M = models.compose(spec)
    Pl = np.asarray(P, dtype=LD)
    xl = np.asarray(x, dtype=LD)
    if xl.ndim > 1:                                            # per problem: one copy per point
        xl = np.repeat(xl, reps, axis=0)
    T, A, cf, Jm, cj, col_term, K = magnitudes(spec, xl, Pl)
    wl = np.ones((), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    if wl.ndim == 2:
        wl = np.repeat(wl, reps, axis=0)
    yl = np.zeros((), dtype=LD) if y is None else np.repeat(np.asarray(y, dtype=LD), reps, axis=0)
    f_ref = wl * (M.f(xl, Pl) - yl)
    J_ref = wl[..., np.newaxis] * M.jac(xl, Pl)
    f_tol = 2 * EPS * np.abs(wl) * (np.sum(T * (cf + K + 2 * np.abs(A)), axis=-1) + np.abs(yl))
    J_tol = 2 * EPS * np.abs(wl)[..., np.newaxis] * Jm * (cj + K + 2 * np.abs(A[:, :, col_term]))
    return f_ref, J_ref, f_tol + 0 * f_ref, J_tol


def variant_inputs(spec, m, variant):
    """x, P, w, y of one variant of (spec, m), drawn once per call from seeds that depend on the case alone."""
    B, per_problem, reps, wk, yk = variant
    key = [sum(spec.encode()), m, B, reps]
    rng = np.random.default_rng(key + [1])
    W = rng.uniform(0.5, 2.0, (B, m))
    Y = rng.standard_normal((B, m))
    x, P = comp_inputs(spec, B * reps, m, seed=key, per_problem=False)
    if per_problem:
        x = comp_inputs(spec, B, m, seed=key, per_problem=True)[0]
    return x, P, {None: None, 1: W[0], 2: W}[wk], Y if yk else None


def numpy_weighted(spec, x, P, w, y, reps, per_problem):
    """The float64 numpy definition, weighted as curve_fit_batch weights it: f (Q, m) and J (Q, m, n)."""
    M = models.compose(spec)
    xr = np.repeat(x, reps, axis=0) if per_problem else x
    wr = 1.0 if w is None else (np.repeat(w, reps, axis=0) if w.ndim == 2 else w)
    yr = 0.0 if y is None else np.repeat(y, reps, axis=0)
    wj = wr if np.ndim(wr) == 0 else np.asarray(wr)[..., np.newaxis]
    return wr * (M.f(xr, P) - yr), wj * M.jac(xr, P)


# ---- end-to-end fit problems ---------------------------------------------------------------------------------------
# label -> (spec, truth, tied, index of an eta boxed inside [0, 1] or None)
FITS = {
    "slope": ("gauss*2+poly*2", [1.5, -0.8, 0.4, 1.0, 0.7, 0.5, 0.2, 0.1], None, None),
    "pvoigt": ("pvoigt+poly*2", [1.5, 0.2, 0.6, 0.5, 0.2, 0.1], None, 3),
    "tied": ("gauss+lorentz+poly*1", [1.5, -0.7, 0.5, 1.0, 0.8, 0.5, 0.2], {5: 2}, None),
}
SIGMA = 0.01
FIT_ROWS = [33, 70]


def fit_problem(label, m, B=8, seed=0):
    """B data sets on [-2, 2], as _model_cases.fit_problem: the truth perturbed by 5 % per problem (tied parameters
    equal), noise of sigma = 0.01, p0 10 % off the truth (the sign drawn per parameter) and a box of
    +-(0.4 |p| + 0.2) around the truth, an eta's clipped to [0, 1].
    -> dict(spec, x, Y, P0, bounds, truth, tied)"""
    spec, truth, tied, eta = FITS[label]
    rng = np.random.default_rng([seed, m, sorted(FITS).index(label)])
    truth = np.asarray(truth) * (1 + 0.05 * rng.uniform(-1, 1, (B, len(truth))))
    for j, i in (tied or {}).items():
        truth[:, j] = truth[:, i]
    x = np.linspace(-2.0, 2.0, m)
    Y = models.compose(spec).f(x, truth) + SIGMA * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    for j, i in (tied or {}).items():
        P0[:, j] = P0[:, i]
    half = 0.4 * np.abs(truth) + 0.2
    lb, ub = truth - half, truth + half
    if eta is not None:
        lb[:, eta], ub[:, eta] = np.maximum(lb[:, eta], 0.0), np.minimum(ub[:, eta], 1.0)
    return dict(spec=spec, x=x, Y=Y, P0=P0, bounds=(lb, ub), truth=truth, tied=tied)
