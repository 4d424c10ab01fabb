"""Cases of the affine-tie tests: the maps and data of the kernel cases of blsq_model_eval_tie_dev, the
doublet fit problems and their independent reference.  No GPU and no library: numpy and scipy only.

The reference (``reference``) is ``scipy.optimize.least_squares`` on a residual written here from ``models.*.f`` with the
constraint spelled out by hand (mu2 = mu1 + 0.6, a2 = 0.5 a1, s2 = s1) and an analytic Jacobian written the same way:
it never touches ``ParamMap`` or ``GlobalMap``."""
import functools

import numpy as np
from scipy.optimize import least_squares

from bounded_lsq import models

from _global_cases import draw_params

# ---- kernel cases ----------------------------------------------------------------------------------------------------
# label: (spec, n, fixed, tied, shared, S, B, m, t kind, w kind, NaN pattern)
#   S == 0: a plain batch of B problems (shared is None); S >= 1: B groups of S data sets
#   t kind: 'shared' (m,), 'set' (S, m; S >= 1 only), 'group' (B, S, m) / (B, m);  w kind: None, 'shared', 'group'
#   NaN pattern (used under BLSQ_NAN_OMIT only): None, 'row0', 'last', 'r63_64', 'set' (a whole problem's rows but one)
DOUBLET = "gauss*2+poly*1"                                 # (a1, mu1, s1, a2, mu2, s2, c)
DOUBLET_TIED = {4: (1, 1.0, 0.42), 3: (0, 0.5), 5: 2}
BIG = "pvoigt*15+poly*4"                                   # n = 64: one wave per workgroup
KERNEL_CASES = {
    "doublet": (DOUBLET, 7, None, DOUBLET_TIED, None, 0, 3, 65, "shared", "shared", "row0"),
    "doublet_m1": (DOUBLET, 7, None, DOUBLET_TIED, None, 0, 1, 1, "group", None, None),
    "doublet_s2": (DOUBLET, 7, None, DOUBLET_TIED, [1, 2], 2, 3, 130, "group", "group", "r63_64"),
    "key_below": (DOUBLET, 7, None, {0: (3, 2.0)}, [3], 1, 1, 63, "set", None, "last"),
    "negative": (DOUBLET, 7, None, {4: (1, -1.0), 5: (2, -1.5, 3.0)}, None, 0, 3, 64, "group", "group", "set"),
    "three_ratios": ("gauss*3+poly*1", 10, None, {3: (0, 2.0 / 3.0), 6: (0, 1.0 / 3.0), 5: 2, 8: (2, 1.0, 0.0)},
                     [1, 2], 3, 1, 64, "set", "shared", "last"),
    "fixed_next": ("lorentz_sum", 7, [2, 6], {3: (0, 0.5, 0.1)}, None, 0, 3, 63, "shared", "group", "row0"),
    "gauss_sum": ("gauss_sum", 7, None, {4: (1, 1.0, 0.42), 5: (2, 1.25)}, [2], 2, 1, 65, "shared", "shared", None),
    "gauss2d": ("gauss2d", 5, None, {2: (1, 1.0, 0.3)}, None, 0, 3, 65, "group", "shared", "r63_64"),
    "big_odd": (BIG, 64, None, {6: (2, 1.5)}, None, 0, 1, 65, "shared", None, "row0"),                   # nf = 63
    "big_even": (BIG, 64, None, {6: (2, 1.5), 10: (2, 0.5, 0.01)}, [60, 61, 62, 63], 2, 1, 65, "set", "shared", None),
}
# the same maps with every tie made trivial: (i, ratio, offset) -> (i, 1.0, 0.0)
TRIVIAL_CASES = ("doublet", "doublet_s2", "three_ratios", "fixed_next", "gauss2d")


def trivial(tied):
    """`tied` with every ratio 1 and every offset 0, in the three tuple forms and the int form by turns."""
    out = {}
    for c, (j, v) in enumerate(tied.items()):
        i = v[0] if isinstance(v, tuple) else v
        out[j] = [i, (i,), (i, 1.0), (i, 1.0, 0.0)][c % 4]
    return out


def plain(tied):
    return {j: (v[0] if isinstance(v, tuple) else v) for j, v in tied.items()}


def kernel_case(label, seed=0, trivial_ties=False):
    """The arrays of one kernel case in the shape (B, S', ...), S' = max(S, 1): P (B, S', n) (also the template of the
    fixed parameters), t (point abscissae; gauss2d: rows u, v), y (B, S', m) counts with zeros, w, the NaN mask."""
    spec, n, fixed, tied, shared, S, B, m, tk, wk, nan = KERNEL_CASES[label]
    if trivial_ties:
        tied = trivial(tied)
    Se = max(S, 1)
    rng = np.random.default_rng([seed, len(label), m, S])
    if spec == "gauss2d":
        P = np.empty((B, Se, 5))
        for j, (lo, hi) in enumerate([(2.0, 5.0), (-1.0, 1.0), (-1.0, 1.0), (0.5, 1.5), (1.0, 3.0)]):
            P[..., j] = rng.uniform(lo, hi, (B, Se))
    else:
        P = draw_params(rng, spec, n, (B, Se))
    coords = 2 if spec == "gauss2d" else 1
    lead = {"shared": (), "set": (Se,), "group": (B, Se)}[tk]
    t = np.sort(rng.uniform(-3.0, 3.0, lead + (coords, m)), axis=-1)
    if coords == 1:
        t = t[..., 0, :]
    y = rng.poisson(4.0, (B, Se, m)).astype(float)
    y[..., ::5] = 0.0
    w = None if wk is None else rng.uniform(0.5, 2.0, (m,) if wk == "shared" else (B, Se, m))
    om = np.zeros((B, Se, m), dtype=bool)
    b, s = B - 1, Se // 2
    if nan == "row0":
        om[b, s, 0] = om[0, 0, 0] = True
    elif nan == "last":
        om[b, s, m - 1] = True
    elif nan == "r63_64":
        om[b, s, 63:65] = True
    elif nan == "set":
        om[b, s, 1:] = True
    return dict(label=label, spec=spec, n=n, fixed=fixed, tied=tied, shared=shared, S=S, B=B, m=m, P=P, t=t, y=y, w=w,
                omitted=om, coords=coords)


# ---- fit cases: the doublet ------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)
SPLIT, RATIO = 0.6, 0.5
FIT_TIED = {4: (1, 1.0, SPLIT), 3: (0, RATIO), 5: 2}       # nf = 4 of n = 7: the variables (a1, mu1, s1, c)
B_FIT, M_FIT, N_FIT = 8, 80, 7
FIT_CASES = ("lse", "poisson", "omit", "bound", "global", "single")


def full(z):
    """By hand: the seven parameters from the variables (a1, mu1, s1, c), z (..., 4)."""
    a1, mu1, s1, c = (z[..., k] for k in range(4))
    return np.stack([a1, mu1, s1, RATIO * a1, mu1 + SPLIT, s1, c], axis=-1)


def chain(J):
    """By hand: the Jacobian over (a1, mu1, s1, c) from the model's (..., m, 7)."""
    return np.stack([J[..., 0] + RATIO * J[..., 3], J[..., 1] + J[..., 4], J[..., 2] + J[..., 5], J[..., 6]], axis=-1)


def _truth(rng, shape, counts=False):
    z = np.empty(shape + (4,))
    z[..., 0] = rng.uniform(60.0, 120.0, shape) if counts else rng.uniform(5.0, 10.0, shape)
    z[..., 1] = rng.uniform(-1.5, -0.5, shape)
    z[..., 2] = rng.uniform(0.5, 0.8, shape)
    z[..., 3] = rng.uniform(5.0, 10.0, shape) if counts else rng.uniform(1.0, 2.0, shape)
    return z


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """One fit problem: x (m,), Y, P0 and bounds over all 7 parameters (a member's own p0 is deliberately wrong: it is
    ignored), the keywords beyond the data in `kw`.  'global': Y (G, S, m) with the width shared; 'single': B = 1.
    Built once; nobody writes into it."""
    rng = np.random.default_rng([11, FIT_CASES.index(name)])
    M = models.compose(DOUBLET)
    m, n = M_FIT, N_FIT
    x = np.linspace(-4.0, 4.0, m)
    shape = {"global": (2, 3), "single": (1,)}.get(name, (B_FIT,))
    zt = _truth(rng, shape, counts=name == "poisson")
    if name == "global":
        zt[..., 2] = zt[:, :1, 2]                           # one width per group
    Pt = full(zt)
    mu = M.f(x, Pt.reshape(-1, n)).reshape(shape + (m,))
    lb, ub = np.full(shape + (n,), -np.inf), np.full(shape + (n,), np.inf)
    lb[..., [2, 5]] = 0.1
    kw = dict(sigma=0.05)
    if name == "poisson":
        Y = rng.poisson(mu).astype(float)
        kw = dict(estimator="poisson", absolute_sigma=True)
        lb[..., [0, 3]], lb[..., 6] = 0.0, 1e-3             # the model stays positive
    else:
        Y = mu + 0.05 * rng.standard_normal(mu.shape)
    if name == "omit":                                      # padded data: problem b has 72 + b points
        for b in range(B_FIT):
            Y[b, 72 + b:] = np.nan
        kw = dict(sigma=0.05, nan_policy="omit")
    if name == "bound":                                     # a bound on mu2 alone, active at the solution
        ub[..., 4] = Pt[..., 4] - 0.05
    z0 = zt * (1.0 + 0.04 * rng.uniform(-1.0, 1.0, zt.shape))
    if name == "bound":
        z0[..., 1] = np.minimum(z0[..., 1], ub[..., 4] - SPLIT - 0.02)
    if name == "global":
        z0[..., 2] = z0[:, :1, 2]
    P0 = full(z0)
    P0[..., [3, 4, 5]] = [1.0, 0.0, 1.0]                    # the members' own starts: ignored
    for a in (x, Y, P0, lb, ub, z0):
        a.setflags(write=False)
    return dict(name=name, spec=DOUBLET, n=n, m=m, tied=FIT_TIED, x=x, Y=Y, P0=P0, z0=z0, bounds=(lb, ub), kw=kw,
                shared=[2] if name == "global" else None)


def _solve(M, x, y, z0, zl, zu, sigma, poisson, layout=None, method="trf"):
    """scipy on the hand-written residual of one problem (layout None) or one group (layout: data set -> the four
    variables of its doublet among the group's).  Analytic Jacobian, tolerances at machine level; 'dogbox' for the case
    with an active bound, where it ends on the bound exactly."""
    keep = ~np.isnan(y)

    def parts(z):
        sets = [z] if layout is None else [z[ix] for ix in layout]
        ys = [y] if layout is None else list(y)
        ks = [keep] if layout is None else list(keep)
        return sets, ys, ks

    def residual(z):
        out = []
        for zs, ysv, k in zip(*parts(z)):
            mu = M.f(x[k], full(zs)[None])[0]
            out.append(models.poisson_transform(mu, ysv[k])[0] if poisson else (mu - ysv[k]) / sigma)
        return np.concatenate(out)

    def jacobian(z):
        sets, ys, ks = parts(z)
        rows = []
        for s, (zs, ysv, k) in enumerate(zip(sets, ys, ks)):
            P = full(zs)[None]
            J = chain(M.jac(x[k], P)[0])
            J = models.poisson_transform(M.f(x[k], P)[0], ysv[k])[1][:, None] * J if poisson else J / sigma
            if layout is None:
                rows.append(J)
            else:
                R = np.zeros((J.shape[0], z.size))
                np.add.at(R, (slice(None), np.asarray(layout[s])), J)
                rows.append(R)
        return np.concatenate(rows)

    first = res = least_squares(residual, z0, jac=jacobian, bounds=(zl, zu), method=method, ftol=1e-15, xtol=1e-15,
                                gtol=1e-15, max_nfev=4000)
    for _ in range(3):                                      # polished: restarted from its own solution, which resets the
        res = least_squares(residual, res.x, jac=jacobian, bounds=(zl, zu), method=method, ftol=None,      # trust region;
                            xtol=1e-15, gtol=1e-15, max_nfev=4000)                 # no stop on a flat cost
    res.status, res.nfev = min(first.status, res.status), first.nfev    # (convergence from the case's start is the first run's)
    return res, jacobian(res.x), int(keep.sum())


@functools.lru_cache(maxsize=None)
def reference(name):
    """popt and pcov of case `name` in the shapes of its Y's leading axes + (7,) / (7, 7), the scipy results, and whether
    every problem converged from the case's start (scipy's status > 0): the screening of the inputs."""
    case = fit_case(name)
    M = models.compose(DOUBLET)
    x, Y, z0, n = case["x"], case["Y"], case["z0"], case["n"]
    lb, ub = case["bounds"]
    poisson = case["kw"].get("estimator") == "poisson"
    sigma = case["kw"].get("sigma", 1.0)
    # the box of (a1, mu1, s1, c), by hand: the member's box moved through its tie and intersected
    zl = np.stack([np.maximum(lb[..., 0], lb[..., 3] / RATIO), np.maximum(lb[..., 1], lb[..., 4] - SPLIT),
                   np.maximum(lb[..., 2], lb[..., 5]), lb[..., 6]], axis=-1)
    zu = np.stack([np.minimum(ub[..., 0], ub[..., 3] / RATIO), np.minimum(ub[..., 1], ub[..., 4] - SPLIT),
                   np.minimum(ub[..., 2], ub[..., 5]), ub[..., 6]], axis=-1)
    lead = Y.shape[:-1]
    popt, pcov, results, ok = np.empty(lead + (n,)), np.zeros(lead + (n, n)), [], True
    T = np.zeros((n, 4))                                    # by hand: d full / d z
    T[0, 0], T[1, 1], T[2, 2], T[3, 0], T[4, 1], T[5, 2], T[6, 3] = 1.0, 1.0, 1.0, RATIO, 1.0, 1.0, 1.0

    def finish(res, J, nobs):                               # over all variables, as scipy's curve_fit has it
        nv = res.x.size
        C = np.linalg.pinv(J.T @ J)
        if not case["kw"].get("absolute_sigma", False):
            C = C * (2.0 * res.cost / (nobs - nv))
        return C

    if name == "global":
        G, S = lead
        for g in range(G):
            layout = [[1 + 3 * s, 2 + 3 * s, 0, 3 + 3 * s] for s in range(S)]     # the width first, then (a1, mu1, c)
            nv = 1 + 3 * S
            zz0, zzl, zzu = np.empty(nv), np.full(nv, -np.inf), np.full(nv, np.inf)
            for s in range(S):
                for k, v in enumerate(layout[s]):
                    if k != 2 or s == 0:
                        zz0[v] = z0[g, s, k]
                    zzl[v], zzu[v] = max(zzl[v], zl[g, s, k]), min(zzu[v], zu[g, s, k])
            res, J, nobs = _solve(M, x, Y[g], zz0, zzl, zzu, sigma, poisson, layout)
            C = finish(res, J, nobs)
            results.append(res)
            ok = ok and res.status > 0
            for s in range(S):
                ix = np.asarray(layout[s])
                popt[g, s] = full(res.x[ix])
                pcov[g, s] = T @ C[np.ix_(ix, ix)] @ T.T
    else:
        for b in range(lead[0]):
            res, J, nobs = _solve(M, x, Y[b], z0[b], zl[b], zu[b], sigma, poisson,
                                  method="dogbox" if name == "bound" else "trf")
            results.append(res)
            ok = ok and res.status > 0
            popt[b] = full(res.x)
            pcov[b] = T @ finish(res, J, nobs) @ T.T
    popt.setflags(write=False)
    pcov.setflags(write=False)
    return popt, pcov, results, ok
