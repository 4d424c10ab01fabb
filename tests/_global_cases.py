"""Cases of the global-fit tests: the kernel cases of blsq_model_eval_global_dev, the fit problems of
``curve_fit_global`` and their independent reference.  No GPU and no library: numpy and scipy only.

The reference (``reference``) is ``scipy.optimize.least_squares`` on a residual written here from ``models.*.f`` over the
concatenated data of a group, with the variable layout spelled out by hand: it never touches ``GlobalMap``."""
import functools

import numpy as np
from scipy.optimize import least_squares

from bounded_lsq import models

# ---- kernel cases ----------------------------------------------------------------------------------------------------
# label: (spec, n, fixed, tied, shared, S, G, m, t kind, w kind, NaN pattern, negative model values)
#   t kind: 'shared' (m,), 'set' (S, m), 'group' (G, S, m);  w kind: None, 'shared' (m,), 'group' (G, S m)
#   NaN pattern: None, 'row0', 'last', 'r63_64' (rows 63 and 64 of one data set), 'set' (one whole data set)
BIG = "pvoigt*15+poly*4"                                  # nf = 64: one wave per workgroup; S = 4: nv = 4 + 4 * 60 = 244
MIXED = "gauss*2+lorentz+pvoigt+poly*3"                   # n = 16
KERNEL_CASES = {
    "gauss_s2": ("gauss_sum", 4, None, None, [1, 2], 2, 3, 65, "shared", "shared", None, False),
    "gauss_s7": ("gauss_sum", 4, None, None, [1, 2], 7, 1, 63, "set", "group", "row0", False),
    "poly_neg": ("poly", 3, None, None, [0], 3, 3, 130, "group", None, "r63_64", True),
    "exp_rates": ("exp_sum", 5, None, None, [1, 3], 2, 1, 64, "set", "shared", "last", False),
    "mixed": (MIXED, 16, [2], {4: 1}, [1, 4, 7, 11, 13], 3, 3, 65, "group", "group", "set", False),
    "mixed_m1": (MIXED, 16, [2], {4: 1}, [1, 4, 7, 11, 13], 2, 1, 1, "set", "shared", None, False),
    "all_shared": ("gauss_sum", 4, None, None, [0, 1, 2, 3], 3, 1, 1, "shared", None, None, False),
    "big": (BIG, 64, None, None, [60, 61, 62, 63], 4, 1, 65, "shared", "shared", "row0", False),
    "one_set": ("gauss_sum", 4, [3], None, [0, 1, 2], 1, 3, 64, "group", "shared", None, False),
}


def param_names(spec, n):
    """The role of every parameter: 'a', 'mu', 's', 'eta', 'r' or 'pK'."""
    equiv = {"gauss_sum": "gauss*%d+poly*1" % ((n - 1) // 3), "lorentz_sum": "lorentz*%d+poly*1" % ((n - 1) // 3),
             "exp_sum": "exp*%d+poly*1" % ((n - 1) // 2), "poly": "poly*%d" % n}
    return [nm.split(".")[1] for nm in models.compose(equiv.get(spec, spec)).param_names]


def draw_params(rng, spec, n, shape, scale=1.0):
    """Parameters of shape + (n,) with every peak inside t in [-3, 3] and a positive model."""
    P = np.empty(shape + (n,))
    for j, role in enumerate(param_names(spec, n)):
        lo, hi = {"a": (2.0 * scale, 5.0 * scale), "mu": (-1.0, 1.0), "s": (0.5, 1.5), "eta": (0.2, 0.8),
                  "r": (0.2, 0.9), "p0": (1.0 * scale, 3.0 * scale)}.get(role, (-0.05, 0.05))
        P[..., j] = rng.uniform(lo, hi, shape)
    return P


def kernel_case(label, seed=0):
    """The arrays of one kernel case: P (G, S, n) (also the template of the fixed parameters), t, y (G, S, m) counts with
    zeros, w, the NaN mask (G, S, m) and the map's keywords."""
    spec, n, fixed, tied, shared, S, G, m, tk, wk, nan, neg = KERNEL_CASES[label]
    rng = np.random.default_rng([seed, len(label), m, S])
    P = draw_params(rng, spec, n, (G, S))
    if neg:
        P[:, 1, 1] = -5.0                                  # data set 1 (a local slope): negative model values for t > 0.6
    t = np.sort(rng.uniform(-3.0, 3.0, {"shared": (m,), "set": (S, m), "group": (G, S, m)}[tk]), axis=-1)
    y = rng.poisson(4.0, (G, S, m)).astype(float)
    y[..., ::5] = 0.0
    w = None if wk is None else rng.uniform(0.5, 2.0, (m,) if wk == "shared" else (G, S * m))
    om = np.zeros((G, S, m), dtype=bool)
    g, s = G - 1, S // 2
    if nan == "row0":
        om[g, s, 0] = om[0, 0, 0] = True
    elif nan == "last":
        om[g, s, m - 1] = True
    elif nan == "r63_64":
        om[g, s, 63:65] = True
    elif nan == "set":
        om[g, s, :] = True
    return dict(label=label, spec=spec, n=n, fixed=fixed, tied=tied, shared=shared, S=S, G=G, m=m, P=P, t=t, y=y, w=w,
                omitted=om)


# ---- fit cases -------------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)
SPEC, N, SHARED = "gauss+poly*1", 4, [1, 2]               # (a, mu, s, c): position and width belong to the group
G_FIT, S_FIT = 4, 5
FIT_CASES = ("lse33", "lse70", "poisson", "ragged", "soft_l1", "fixtied")


def _truth(rng, G, S, counts=False):
    P = np.empty((G, S, N))
    P[..., 0] = rng.uniform(60.0, 120.0, (G, S)) if counts else rng.uniform(5.0, 10.0, (G, S))
    P[..., 1] = rng.uniform(-0.5, 0.5, (G, 1))
    P[..., 2] = rng.uniform(0.8, 1.3, (G, 1))
    P[..., 3] = rng.uniform(5.0, 10.0, (G, S)) if counts else rng.uniform(1.0, 2.0, (G, S))
    return P


def _box(G, S, n, width_cols):
    lb, ub = np.full((G, S, n), -np.inf), np.full((G, S, n), np.inf)
    lb[..., width_cols] = 0.1
    return lb, ub


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """One fit problem: the arguments of ``curve_fit_global`` (`kw` holds the keywords beyond the data) and what the
    reference needs.  Built once; nobody writes into it."""
    rng = np.random.default_rng([7, FIT_CASES.index(name)])
    spec, n, shared, fixed, tied, kw = SPEC, N, SHARED, None, None, {}
    G, S = G_FIT, S_FIT
    M = models.compose(spec)
    if name in ("lse33", "lse70", "soft_l1"):
        m = 33 if name == "lse33" else 70
        x = np.linspace(-4.0, 4.0, m) if name == "lse33" else \
            np.linspace(-4.0, 4.0, m)[None, :] + 0.1 * np.arange(S)[:, None]           # (S, m): per data set
        Pt = _truth(rng, G, S)
        Y = M.f(np.broadcast_to(x, (G, S, m)).reshape(G * S, m), Pt.reshape(-1, n)).reshape(G, S, m)
        Y = Y + 0.05 * rng.standard_normal(Y.shape)
        kw = dict(sigma=0.05)
        if name == "soft_l1":
            Y[:, :, ::9] += 0.3                            # outliers
            kw = dict(sigma=0.05, loss="soft_l1", f_scale=2.0)
        lb, ub = _box(G, S, n, [2])
    elif name == "poisson":
        m = 33
        x = np.linspace(-4.0, 4.0, m)
        Pt = _truth(rng, G, S, counts=True)
        Y = rng.poisson(M.f(x, Pt.reshape(-1, n)).reshape(G, S, m)).astype(float)
        kw = dict(estimator="poisson", absolute_sigma=True)
        lb, ub = _box(G, S, n, [2])
        lb[..., 0], lb[..., 3] = 0.0, 1e-3                 # the model stays positive
    elif name == "ragged":
        G, S = 1, 3
        Pt = _truth(rng, G, S)
        xs = [np.linspace(-4.0, 4.0, k) for k in (40, 64, 70)]
        ys = [M.f(xs[s], Pt[0, s:s + 1])[0] + 0.05 * rng.standard_normal(xs[s].size) for s in range(S)]
        x, Y = models.pad_ragged(xs, ys)                   # (S, 70) each, NaN behind the shorter sets
        Y = Y[None]
        kw = dict(sigma=0.05, nan_policy="omit")
        lb, ub = _box(G, S, n, [2])
    else:                                                  # fixtied: two peaks of one width over a held baseline
        spec, n, shared, fixed, tied = "gauss*2+poly*1", 7, [1, 2, 4, 5], [6], {5: 2}
        M = models.compose(spec)
        m = 70
        x = np.linspace(-4.0, 4.0, m)
        Pt = np.empty((G, S, n))
        Pt[..., 0] = rng.uniform(5.0, 10.0, (G, S))
        Pt[..., 1] = rng.uniform(-1.8, -1.2, (G, 1))
        Pt[..., 2] = Pt[..., 5] = rng.uniform(0.6, 0.9, (G, 1))
        Pt[..., 3] = rng.uniform(4.0, 8.0, (G, S))
        Pt[..., 4] = rng.uniform(1.2, 1.8, (G, 1))
        Pt[..., 6] = 1.5
        Y = M.f(x, Pt.reshape(-1, n)).reshape(G, S, m) + 0.05 * rng.standard_normal((G, S, m))
        kw = dict(sigma=0.05)
        lb, ub = _box(G, S, n, [2, 5])
    P0 = Pt * (1.0 + 0.04 * rng.uniform(-1.0, 1.0, Pt.shape))
    if fixed:
        P0[..., fixed] = Pt[..., fixed]
    for a in (x, Y, P0, lb, ub):
        a.setflags(write=False)
    return dict(name=name, spec=spec, n=n, shared=shared, fixed=fixed, tied=tied, G=G, S=S, m=Y.shape[-1], x=x, Y=Y,
                P0=P0, bounds=(lb, ub), kw=kw)


def _layout(case):
    """By hand: the free leaders, which of them are shared, and for parameter j of data set s its variable (or None)."""
    n, S = case["n"], case["S"]
    fixed, tied = set(case["fixed"] or ()), dict(case["tied"] or {})
    leaders = [j for j in range(n) if j not in fixed and j not in tied]
    sh = [j for j in leaders if j in case["shared"]]
    lo = [j for j in leaders if j not in case["shared"]]
    nv = len(sh) + S * len(lo)

    def var(j, s):
        if j in fixed:
            return None
        j = tied.get(j, j)
        return sh.index(j) if j in sh else len(sh) + s * len(lo) + lo.index(j)
    return sh, lo, nv, var


@functools.lru_cache(maxsize=None)
def reference(name):
    """popt (G, S, n), pcov (G, S, n, n), the scipy results and nv of case `name`: every group solved on its own by
    ``scipy.optimize.least_squares`` ('trf', 3-point differences, tolerances 1e-13) on the concatenated residual."""
    case = fit_case(name)
    G, S, m, n = case["G"], case["S"], case["m"], case["n"]
    M = models.compose(case["spec"])
    sh, lo, nv, var = _layout(case)
    kw = case["kw"]
    sigma = kw.get("sigma", 1.0)
    lb, ub = case["bounds"]
    popt, pcov, results = np.empty((G, S, n)), np.zeros((G, S, n, n)), []
    for g in range(G):
        keep = ~np.isnan(case["Y"][g])                     # (S, m): the compressed data of a ragged group
        xg = np.broadcast_to(case["x"], (S, m))

        def params(z):
            P = np.array(case["P0"][g])
            for s in range(S):
                for j in range(n):
                    if var(j, s) is not None:
                        P[s, j] = z[var(j, s)]
            return P

        def residual(z):
            P = params(z)
            out = []
            for s in range(S):
                mu = M.f(xg[s][keep[s]], P[s:s + 1])[0]
                y = case["Y"][g, s][keep[s]]
                out.append(models.poisson_transform(mu, y)[0] if kw.get("estimator") == "poisson" else (mu - y) / sigma)
            return np.concatenate(out)

        z0, zl, zu = np.empty(nv), np.full(nv, -np.inf), np.full(nv, np.inf)
        for s in range(S):
            for j in range(n):
                v = var(j, s)
                if v is not None:
                    if j in sh + lo and (s == 0 or j in lo):
                        z0[v] = case["P0"][g, s, j]
                    zl[v], zu[v] = max(zl[v], lb[g, s, j]), min(zu[v], ub[g, s, j])
        res = least_squares(residual, z0, jac="3-point", bounds=(zl, zu), method="trf", ftol=1e-13, xtol=1e-13,
                            gtol=1e-13, loss=kw.get("loss", "linear"), f_scale=kw.get("f_scale", 1.0), max_nfev=2000)
        results.append(res)
        C = np.linalg.pinv(res.jac.T @ res.jac)
        if not kw.get("absolute_sigma", False):
            C = C * (2.0 * res.cost / (int(keep.sum()) - nv))
        popt[g] = params(res.x)
        for s in range(S):
            for j1 in range(n):
                for j2 in range(n):
                    if var(j1, s) is not None and var(j2, s) is not None:
                        pcov[g, s, j1, j2] = C[var(j1, s), var(j2, s)]
    popt.setflags(write=False)
    pcov.setflags(write=False)
    return popt, pcov, results, nv
