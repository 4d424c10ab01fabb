"""Inputs shared by tests/test_models_cpu.py and tests/test_models_gpu.py: seeded evaluation points for the kernel-level
comparisons, the rounding-error bound of one model evaluation, and the seeded fit problems of the end-to-end tests."""
import numpy as np

from bounded_lsq import ParamMap, models

LD = np.longdouble
EPS = np.finfo(float).eps


# ---- the instance tables of the case modules: label -> (name or spec, n, fixed, tied, ...) -------------------------------
def is_composite(instances, label):
    return "+" in instances[label][0]


def model_of(instances, label):
    return models.resolve(instances[label][0])


def map_of(instances, label):
    name, n, fixed, tied = instances[label][:4]
    return None if fixed is None and tied is None else ParamMap(n, fixed, tied)


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol, the difference taken in the precision of `ref`; where tol is 0 the values must be equal
    (0), or the ratio is inf."""
    got = np.asarray(got)
    d = np.abs(got.astype(np.result_type(got, ref)) - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(tol > 0, d / np.where(tol > 0, tol, 1), np.where(d == 0, 0.0, np.inf))
    return float(np.max(ratio))


def case_inputs(name, n, B, m, seed=0, per_problem=False):
    """Well-scaled parameters and coordinates of a model: amplitudes and widths in [0.5, 1.5], centres inside the
    coordinate range [-2, 2] ([0, 4] for the decays)."""
    rng = np.random.default_rng(seed)
    M = models.get(name)
    P = rng.uniform(0.5, 1.5, (B, n))
    if name in ("gauss_sum", "lorentz_sum"):
        P[:, 1:-1:3] = rng.uniform(-1.5, 1.5, P[:, 1:-1:3].shape)
    if name == "gauss2d":
        P[:, 1:3] = rng.uniform(-1.0, 1.0, (B, 2))
    lo, hi = (0.0, 4.0) if name == "exp_sum" else (-2.0, 2.0)
    shape = ((B,) if per_problem else ()) + ((m,) if M.coords == 1 else (2, m))
    x = np.sort(rng.uniform(lo, hi, shape), axis=-1)
    if M.coords == 2:                               # (the second coordinate is not ordered like the first)
        x[..., 1, :] = rng.permuted(x[..., 1, :], axis=-1)
    return x, P


def summands(name, x, P):
    """In np.longdouble, for parameters P (Q, n) and coordinates x broadcastable against them: the summands of the
    model ``T`` (Q, m, S) — the K terms, then the offset c (poly: the n monomials p_k t^k) —, the exponent's argument
    of each ``A`` (Q, m, S) (0 where there is none), the number of terms K, and ``col_term`` (n,): the summand whose
    argument enters column j of the Jacobian."""
    M = models.get(name)
    P = np.asarray(P, dtype=LD)
    x = np.asarray(x, dtype=LD)
    Q, n = P.shape
    K = M.terms(n)
    col = lambda k: P[:, k, np.newaxis]                                            # noqa: E731
    if name == "poly":
        T = np.stack([col(k) * x ** k + 0 * x for k in range(n)], axis=-1)
        return T, np.zeros_like(T), n, np.zeros(n, dtype=int)
    T, A = [], []
    if name == "gauss2d":
        r2 = (x[..., 0, :] - col(1)) ** 2 + (x[..., 1, :] - col(2)) ** 2
        arg = -r2 / (2 * col(3) ** 2)
        T.append(col(0) * np.exp(arg))
        A.append(arg)
        col_term = np.array([0, 0, 0, 0, 1])
    else:
        w = M.n_per_term
        for k in range(K):
            if name == "exp_sum":
                arg = -(col(2 * k + 1) * x)
                T.append(col(2 * k) * np.exp(arg))
            else:
                z = (x - col(3 * k + 1)) / col(3 * k + 2)
                arg = -z * z / 2 if name == "gauss_sum" else 0 * z
                T.append(col(3 * k) * (np.exp(arg) if name == "gauss_sum" else 1 / (1 + z * z)))
            A.append(arg)
        col_term = np.array([j // w for j in range(n - 1)] + [K])
    T.append(col(n - 1) + 0 * T[0])
    A.append(0 * T[0])
    return np.stack(T, axis=-1), np.stack(A, axis=-1), K, col_term


def bounds_of(name, x, P, w, y, reps=1):
    """The allowed error of every entry of f (Q, m) and of J (Q, m, n) (test_models_gpu.py: the derivation), with the
    longdouble references ``f_ref``, ``J_ref``.  w: None, (m,) or (B, m); y: None or (B, m); Q = B * reps."""
    M = models.get(name)
    Pl = np.asarray(P, dtype=LD)
    Q, n = Pl.shape
    xl = np.asarray(x, dtype=LD)
    if xl.ndim > (1 if M.coords == 1 else 2):                  # per problem: one copy per point
        xl = np.repeat(xl, reps, axis=0)
    T, A, K, col_term = summands(name, xl, Pl)
    wl = np.ones((), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    if wl.ndim == 2:
        wl = np.repeat(wl, reps, axis=0)
    yl = np.zeros((), dtype=LD) if y is None else np.repeat(np.asarray(y, dtype=LD), reps, axis=0)
    f_ref = wl * (M.f(xl, Pl) - yl)
    Jm = M.jac(xl, Pl)
    J_ref = wl[..., np.newaxis] * Jm
    f_tol = 2 * EPS * np.abs(wl) * (np.sum(np.abs(T) * (4 + K + 2 * np.abs(A)), axis=-1) + np.abs(yl))
    J_tol = 2 * EPS * np.abs(wl)[..., np.newaxis] * np.abs(Jm) * (8 + K + 2 * np.abs(A[:, :, col_term]))
    return f_ref, J_ref, f_tol + 0 * f_ref, J_tol


# ---- end-to-end fit problems ---------------------------------------------------------------------------------------
# label -> (name, truth, coordinate range)
FITS = {
    "poly4": ("poly", [1.0, -0.5, 0.3, 0.2], (-2.0, 2.0)),
    "exp1": ("exp_sum", [2.0, 1.0, 0.5], (0.0, 4.0)),
    "exp2": ("exp_sum", [3.0, 2.5, 1.5, 0.4, 0.2], (0.0, 4.0)),
    "gauss1": ("gauss_sum", [1.5, 0.2, 0.6, 0.3], (-2.0, 2.0)),
    "gauss2": ("gauss_sum", [1.5, -0.8, 0.4, 1.0, 0.7, 0.5, 0.2], (-2.0, 2.0)),
    "lorentz1": ("lorentz_sum", [1.5, 0.1, 0.5, 0.2], (-2.0, 2.0)),
    "gauss2d": ("gauss2d", [2.0, 0.3, -0.2, 0.8, 0.1], (-2.0, 2.0)),
}
GRID = {33: (3, 11), 70: (7, 10)}                  # gauss2d: m points as a grid over [-2, 2]^2
SIGMA = 0.01


def fit_problem(label, m, B=8, seed=0):
    """B data sets of one family: the truth perturbed by 5 % per problem, noise of sigma = 0.01, p0 10 % off the
    truth (the sign drawn per parameter) and a box of +-(0.4 |p| + 0.2) around the truth.
    -> dict(name, x, Y, P0, bounds, truth)"""
    name, truth, (lo, hi) = FITS[label]
    rng = np.random.default_rng([seed, m, sorted(FITS).index(label)])
    truth = np.asarray(truth) * (1 + 0.05 * rng.uniform(-1, 1, (B, len(truth))))
    if name == "gauss2d":
        gu, gv = GRID[m]
        U, V = np.meshgrid(np.linspace(lo, hi, gu), np.linspace(lo, hi, gv), indexing="ij")
        x = np.stack([U.ravel(), V.ravel()])
    else:
        x = np.linspace(lo, hi, m)
    Y = models.get(name).f(x, truth) + SIGMA * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    return dict(name=name, x=x, Y=Y, P0=P0, bounds=(truth - half, truth + half), truth=truth)
