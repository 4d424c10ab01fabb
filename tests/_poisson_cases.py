"""Inputs shared by tests/test_poisson_cpu.py and tests/test_poisson_gpu.py: the grid and the extended
precision reference of the transform test, the model instances, seeded inputs and error bound of the kernel-level
comparison (the derivation is in the docstring of test_poisson_gpu.py::test_kernel_against_definition), and the seeded
count data of the end-to-end fits."""
import functools

import numpy as np

from bounded_lsq import models

import _composite_cases as cc
import _model_cases as mc

LD = np.longdouble
EPS = np.finfo(float).eps
U0 = models.POISSON_U0

# ---- the transform against extended precision ------------------------------------------------------------------------
# Measured (x86-64 glibc, 80-bit long double) over transform_grid(): the worst relative error of r and of c in units of
# eps = 2^-52, (a) where mu >= y / 2 and at y == 0, (b) times mu / y where mu < y / 2, (c) over the whole grid, whose worst
# point is its corner u = -1 + 1e-12.  DESIGN.md 7m records them; the tests allow twice as much.
MEASURED = {"r": (2.56, 1.12, 1.13e10), "c": (2.80, 0.88, 1.13e10)}
REF_SWITCH = 0.25            # |u| below which the unsimplified formulas in long double lose more than 0.02 eps


def transform_grid():
    """mu (Y, U) and y (Y, 1): y over 1e-3 .. 1e9 (49 values) and one row y == 0; u = mu / y - 1 over [-1 + 1e-12, 1e6]
    with 0, denormal-small |u|, +-U0 (1 +- 2^-40), +-U0, both branches densely and 4000 uniform draws in (-1, 1)."""
    us = [0.0]
    for sgn in (1.0, -1.0):
        us += list(sgn * np.logspace(-320, -300, 5))
        us += list(sgn * np.logspace(-30, np.log10(U0), 4000))
        us += [sgn * U0 * (1 - 2.0 ** -40), sgn * U0 * (1 + 2.0 ** -40), sgn * U0]
    us += list(np.logspace(np.log10(U0), 6, 4000))
    us += list(-np.logspace(np.log10(U0), 0, 4000)[:-1])
    us += list(-1 + np.logspace(-12, -1, 400))
    us += list(np.random.default_rng(0).uniform(-1, 1, 4000))
    u = np.array(us)
    y = np.logspace(-3, 9, 49)[:, np.newaxis]
    mu = np.maximum(y * (1 + u), y * 1e-12)
    mu0 = np.resize(np.logspace(-6, 9, 2000), (1, u.size))          # the row of y == 0
    return np.concatenate([mu, mu0]), np.concatenate([y, [[0.0]]])


def unsimplified(mu, y):
    """r and c by the formulas of the definition as they are written, in np.longdouble:
    D = 2 [mu - y + y ln(y / mu)] (the y ln term 0 at y == 0), r = sign(mu - y) sqrt(D), c = (1 - y / mu) / r."""
    mu, y = np.broadcast_arrays(np.asarray(mu, dtype=LD), np.asarray(y, dtype=LD))
    with np.errstate(all="ignore"):
        yl = np.where(y > 0, y * np.log(np.where(y > 0, y, 1) / mu), 0)
        D = 2 * (mu - y + yl)
        r = np.sign(mu - y) * np.sqrt(D)
        c = (1 - y / mu) / r
    return r, c


def reference(mu, y):
    """The reference of the transform test, in np.longdouble: ``unsimplified`` where |u| >= REF_SWITCH and at y == 0.
    Nearer to mu == y those formulas cancel in long double as well (D loses 2 eps_ld / u^2: 0.02 eps at |u| = 1 / 4,
    all its digits at |u| ~ 1e-10, and c is 0 / 0 at u == 0), so there D = y u^2 2 phi(u) is summed from 60 terms of the
    series of phi (the remainder is below 4^-60), with the limits r = 0, c = 1 / sqrt(mu) at u == 0."""
    mu, y = np.broadcast_arrays(np.asarray(mu, dtype=LD), np.asarray(y, dtype=LD))
    r, c = unsimplified(mu, y)
    with np.errstate(all="ignore"):
        d = mu - y
        u = np.where(y > 0, d / np.where(y > 0, y, 1), 1)
        near = np.abs(u) < REF_SWITCH
        us = np.where(near, u, 0)
        phi = np.zeros_like(us)
        for k in range(59, -1, -1):
            phi = phi * us + LD(-1) ** k / LD(k + 2)
        s = np.sqrt(2 * phi / np.where(y > 0, y, 1))
        r = np.where(near, d * s, r)
        c = np.where(near, 1 / (mu * s), c)
    return r, c


def rel_err(got, ref):
    """|got - ref| / |ref| in units of eps; 0 where both are 0, inf where only ref is."""
    got = np.asarray(got).astype(LD)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / np.abs(ref) / EPS
    return np.where(ref == 0, np.where(got == 0, 0, np.inf), e)


# ---- the kernel against the definition -------------------------------------------------------------------------------
# label -> (named model or composite spec, n, fixed, tied)
INSTANCES = {
    "gauss_sum": ("gauss_sum", 7, None, None),
    "exp_sum": ("exp_sum", 5, None, None),
    "gauss2d": ("gauss2d", 5, None, None),
    "gauss_sum-map": ("gauss_sum", 7, [1], {5: 2}),
    "composite": ("gauss+pvoigt+poly*2", 9, None, None),
    "composite-map": ("gauss+pvoigt+poly*2", 9, [6], {5: 2}),
}
# parameters of an instance's model that scale a term (set to 0 for the problem whose model is its offset alone), the
# offset, and parameters that must vanish with them (the slope of poly*2)
AMPLITUDES = {"gauss_sum": ([0, 3], 6, []), "exp_sum": ([0, 2], 4, []), "gauss2d": ([0], 4, []),
              "gauss+pvoigt+poly*2": ([0, 3], 7, [8])}
ROWS = [1, 63, 64, 65, 130]
B = 3
LOG1P_ULP = 2                # the error allowed to the device's log1p, in ulp


is_composite = functools.partial(mc.is_composite, INSTANCES)
model_of = functools.partial(mc.model_of, INSTANCES)
map_of = functools.partial(mc.map_of, INSTANCES)


def kernel_case(label, m, reps, per_problem):
    """Seeded inputs of one kernel comparison -> dict(x, P, X, Pfix, y, pm):  P (Q, n) the full parameters of every
    point (tied copies made), X what the entry takes (P, or its nf leaders), Pfix (B, n).  Problem 0 is its offset alone,
    at the integer 3 (every amplitude 0), so mu == 3 exactly at all its points; the others are the well-scaled draws of
    the model tests (a composite's p0 raised by 4 so that its line stays positive).  The counts y (B, m) follow mu at the
    first point of each problem through eight patterns in turn: 0, mu itself, mu / (1 +- 0.2) (|u| < U0), mu / (1 +- 0.3)
    (|u| > U0), the next integer above mu, mu / 4 (u = 3)."""
    name, n, fixed, tied = INSTANCES[label]
    M, pm = model_of(label), map_of(label)
    Q = B * reps
    seed = [sum(label.encode()), m, reps]
    if is_composite(label):
        x, P = cc.comp_inputs(name, Q, m, seed=seed)
        if per_problem:
            x = cc.comp_inputs(name, B, m, seed=seed, per_problem=True)[0]
    else:
        x, P = mc.case_inputs(name, n, Q, m, seed=seed)
        if per_problem:
            x = mc.case_inputs(name, n, B, m, seed=seed, per_problem=True)[0]
    amps, off, zero = AMPLITUDES[name]
    if is_composite(label):
        P[:, off] += 4.0
    P[:reps, amps + zero] = 0.0
    P[:reps, off] = 3.0
    Pfix = np.ascontiguousarray(P[::reps])
    if pm is not None:
        X = np.ascontiguousarray(pm.reduce_x(P))
        P = pm.expand_x(X, np.repeat(Pfix, reps, axis=0))
    else:
        X = P
    xr = np.repeat(x, reps, axis=0) if per_problem else x
    mu = M.f(xr, P)[::reps]                                           # (B, m): the first point of each problem
    pattern = (np.arange(m)[np.newaxis, :] + 3 * np.arange(B)[:, np.newaxis]) % 8
    y = np.choose(pattern, [0 * mu, mu, mu / 1.2, mu / 0.8, mu / 1.3, mu / 0.7, np.floor(mu) + 1, mu / 4])
    return dict(x=x, P=P, X=X, Pfix=Pfix, y=np.ascontiguousarray(y), pm=pm)


def transform_counts(u, pos):
    """The rounding counts T_r and T_c of the transform's own operations in units of eps, for u = mu / y - 1 where
    `pos` (y > 0), and at y == 0 (the docstring of test_kernel_against_definition derives them)."""
    with np.errstate(all="ignore"):
        N = u - np.log1p(u)
        direct = 7 + (2 * np.abs(u) + 2 * np.abs(u) / (1 + u) + LOG1P_ULP * np.abs(np.log1p(u))) / N
    e_phi = np.where(np.abs(u) < U0 * (1 - 1e-6), 3, direct)
    T = e_phi / 2 + 3.5
    return np.where(pos, T, 2), np.where(pos, T, 3)


def kernel_bounds(label, case, reps):
    """-> r_ref (Q, m), J_ref (Q, m, nc), r_tol, J_tol: the longdouble definition at the case's points and the allowed
    error of every entry."""
    name, n, fixed, tied = INSTANCES[label]
    pm = case["pm"]
    if is_composite(label):
        v_ref, Jm_ref, v_tol, Jm_tol = cc.bounds_of(name, case["x"], case["P"], None, None, reps=reps)
        xl = np.asarray(case["x"], dtype=LD)
        Jabs = cc.magnitudes(name, np.repeat(xl, reps, axis=0) if xl.ndim > 1 else xl, np.asarray(case["P"], dtype=LD))[3]
    else:
        v_ref, Jm_ref, v_tol, Jm_tol = mc.bounds_of(name, case["x"], case["P"], None, None, reps=reps)
        Jabs = np.abs(Jm_ref)
    if pm is not None:                     # a slot: the sequential sum of its columns, one rounding per addition
        extra = np.array([len(pm.group(k)) - 1 for k in range(pm.nf)])
        Jabs = pm.reduce_jac(Jabs)
        Jm_ref, Jm_tol = pm.reduce_jac(Jm_ref), pm.reduce_jac(Jm_tol) + 2 * EPS * extra * Jabs
    yl = np.repeat(np.asarray(case["y"], dtype=LD), reps, axis=0)
    r_ref, c_ref = models.poisson_transform(v_ref, yl)
    pos = yl > 0
    with np.errstate(all="ignore"):
        u = np.where(pos, (v_ref - yl) / np.where(pos, yl, 1), 0)
    T_r, T_c = transform_counts(u, pos)
    r_tol = np.abs(c_ref) * v_tol + 2 * EPS * T_r * np.abs(r_ref)
    J_tol = np.abs(c_ref)[..., np.newaxis] * (Jm_tol + Jabs * (2 * EPS * (T_c + 1) + v_tol / v_ref)[..., np.newaxis])
    return r_ref, c_ref[..., np.newaxis] * Jm_ref, r_tol, J_tol


def numpy_definition(label, case, reps):
    """The float64 definition at the case's points: the route of a callable.  -> r (Q, m), J (Q, m, nc)."""
    M, pm = model_of(label), case["pm"]
    x = case["x"]
    xr = np.repeat(x, reps, axis=0) if x.ndim > (1 if M.coords == 1 else 2) else x
    yr = np.repeat(case["y"], reps, axis=0)
    jac = M.jac if pm is None else (lambda xd, P: pm.reduce_jac(M.jac(xd, P)))
    return (models.poisson_residual(M.f, yr)(xr, case["P"]), models.poisson_jacobian(M.f, jac, yr)(xr, case["P"]))


# ---- end to end ------------------------------------------------------------------------------------------------------
FIT_SPEC = "gauss+poly*1"
TWO_SPEC = "gauss*2+poly*1"                    # two lines that share one width: tied={5: 2}
FIT_SEED = 2


def fit_problem(B=8, m=96, seed=FIT_SEED, two=False):
    """B spectra of m = 96 channels on [-2, 2]: one Gaussian line (a ~ 20 counts at the peak, mu ~ 0.2, s ~ 0.5; the
    truth perturbed by 5 % per problem) over a background of 0.4 counts per channel, so that every problem has empty
    channels; the counts are drawn once from the Poisson law.  p0 is 10 % off the truth; the box holds a >= 0, the
    line inside the window, 0.1 <= s <= 2 and the background >= 1e-3, which keeps the model positive.
    two: a second line (a ~ 12 at mu ~ -0.9) of the first one's width, for ``tied={5: 2}``.
    -> dict(spec, x, Y, P0, bounds, truth)"""
    rng = np.random.default_rng([seed, B, m, int(two)])
    base = [20.0, 0.4, 0.35, 12.0, -0.9, 0.35, 0.4] if two else [20.0, 0.2, 0.5, 0.4]
    n = len(base)
    truth = np.array(base) * (1 + 0.05 * rng.uniform(-1, 1, (B, n)))
    if two:
        truth[:, 5] = truth[:, 2]
    spec = TWO_SPEC if two else FIT_SPEC
    x = np.linspace(-2.0, 2.0, m)
    Y = rng.poisson(models.compose(spec).f(x, truth)).astype(float)
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    if two:
        P0[:, 5] = P0[:, 2]
    peak_lb, peak_ub = [0.0, -2.0, 0.1], [200.0, 2.0, 2.0]
    lb = np.broadcast_to(peak_lb * (n // 3) + [1e-3], (B, n)).copy()
    ub = np.broadcast_to(peak_ub * (n // 3) + [50.0], (B, n)).copy()
    return dict(spec=spec, x=x, Y=Y, P0=P0, bounds=(lb, ub), truth=truth)


def score(spec, x, Y, P, pm=None):
    """The Poisson score sum_i (1 - y_i / mu_i) dmu_i / dp_j and the sum of the absolute values of its summands, both
    (B, n) (with a map: over the nf solver variables)."""
    M = models.resolve(spec)
    mu, J = M.f(x, P), M.jac(x, P)
    if pm is not None:
        J = pm.reduce_jac(J)
    S = (1 - Y / mu)[:, :, np.newaxis] * J
    return S.sum(axis=1), np.abs(S).sum(axis=1)
