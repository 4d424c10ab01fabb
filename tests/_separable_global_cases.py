"""What the tests of the separable global fits share: the grid of the kernel tests, the caps of Sinv and
TD, the data of the whole fits and their references.  Not collected as a test.

Kernel grid: (m, nl, na; S; nsh) — the resident / streamed boundary (64 / 65 rows) and the tile counts of
DESIGN.md 7v, each with nv = nsh + S (na - nsh) <= 256.

Caps against np.longdouble (``_varpro._reduce_full``), per data set, on the vetted cases of tests/_separable_cases.py:
    TD:   per column i, max_p |TD[p, i] - ref| / (|w G_i|_2 |c_owner(i)|) <= 32 kappa_2(Phi_w) eps     (the J metric of 7v)
    Sinv: |Sinv - ref|_inf / |ref|_inf <= 32 kappa_2(Phi_w)^2 eps              (the conditioning of inverting S)
A column of TD is the least-squares solution for a random column of G, whose residual is as large as the column: the
scheme of 7v alone leaves kappa eps |T| with |T| up to |G_i| / sigma_min, 31 to 57 times the TD cap on the ill-conditioned
case (kappa = 2e5).  TD therefore comes from T after one more correction whose residual is formed in extended precision
(double-double in the kernel, np.longdouble in the definition); with it the float64 definition stays below 0.06 of both
caps on every case.
Cov-blocks against the numpy definition on the device's own C, Sinv and TD: a plain summation bound,
    |d| <= 4 (na + 1)^2 eps (|Sinv| + |TD| |C| |TD|^T)   and the analogues |TD| |C|, |C| for the other blocks."""
import functools

import numpy as np

import bounded_lsq
from bounded_lsq import models
from bounded_lsq._varpro import _reduce_full

import _separable_cases as sc

LD = np.longdouble
EPS = np.finfo(np.float64).eps
CAP = 32.0
GRID = ((2, 1, 1, 3, 1), (5, 2, 2, 2, 1), (63, 5, 11, 4, 6), (64, 5, 11, 4, 11), (65, 16, 48, 3, 40),
        (130, 3, 61, 2, 30), (257, 16, 1, 7, 1))
GROUPS = (1, 3)


class GroupCase:
    """G groups of S data sets of random raw Jacobians, in the manner of ``_separable_cases.Case``."""

    def __init__(self, m, nl, na, S, nsh, G, seed):
        rng = np.random.default_rng(seed)
        n, B = nl + na, G * S
        self.m, self.nl, self.na, self.n, self.S, self.G, self.nsh = m, nl, na, n, S, G, nsh
        self.lin = np.sort(rng.choice(n, nl, replace=False)).astype(np.int32)
        self.owner = rng.integers(0, nl, n).astype(np.int32)
        self.owner[self.lin] = -1
        self.non = np.flatnonzero(self.owner >= 0)
        self.shared_pos = np.sort(rng.choice(na, nsh, replace=False))              # positions within non
        self.shared = np.zeros(n, dtype=np.int32)
        self.shared[self.non[self.shared_pos]] = 1
        self.gm = bounded_lsq.GlobalMap(na, S, self.shared_pos)
        self.nv = self.gm.nv
        self.Graw = rng.standard_normal((B, m, n))
        c0 = rng.uniform(0.5, 2.0, (B, nl)) * rng.choice([-1.0, 1.0], (B, nl))
        self.y = np.einsum("bip,bp->bi", self.Graw[:, :, self.lin], c0) + 0.1 * rng.standard_normal((B, m))
        self.X = rng.standard_normal((G, self.nv))
        self.ws = {"none": None, "shared": rng.uniform(0.5, 2.0, m), "per_problem": rng.uniform(0.5, 2.0, (B, m))}

    def only(self, g):
        """Group g alone, as a case of G = 1 (views of the same numbers)."""
        c = object.__new__(GroupCase)
        c.__dict__.update(self.__dict__)
        rows = slice(g * self.S, (g + 1) * self.S)
        c.G, c.Graw, c.y, c.X = 1, self.Graw[rows], self.y[rows], self.X[g:g + 1]
        c.ws = dict(self.ws, per_problem=self.ws["per_problem"][rows])
        return c


@functools.lru_cache(maxsize=None)
def group_case(m, nl, na, S, nsh, G):
    return GroupCase(m, nl, na, S, nsh, G, 100000 * G + 1000 * m + 10 * nl + na + S)


def expand_definition(cs, X=None):
    """P (G S, n) of X (G, nv): the definition of blsq_varpro_expand_global_dev."""
    X = cs.X if X is None else X
    return models.varpro_expand(cs.gm.split_x(X).reshape(cs.G * cs.S, cs.na), cs.lin, cs.n)


# ---- Sinv and TD against np.longdouble on the vetted cases ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_full(m, nl, na, wform, ill=False):
    """(f, J, c, info, Sinv, TD) of a case of tests/_separable_cases.py in np.longdouble; computed once and shared."""
    cs = sc.case(m, nl, na, ill)
    w = cs.ws[wform]
    out = _reduce_full(cs.G.astype(LD), cs.y.astype(LD), None if w is None else w.astype(LD), cs.lin, cs.owner)
    for a in out:
        a.setflags(write=False)
    return out


def fractions_full(cs, wform, ref, Sinv, TD):
    """The two metrics of the module docstring as fractions of their caps, the worst over the B data sets."""
    w = cs.weights(wform)
    kappa = cs.kappa(wform)
    c_ref, Sinv_ref, TD_ref = ref[2], ref[4], ref[5]
    col = np.linalg.norm(w[:, :, None] * cs.G[:, :, cs.non], axis=1)                         # (B, na)
    own = np.abs(c_ref[:, cs.owner[cs.non]])
    err = np.max(np.abs(TD.astype(LD) - TD_ref), axis=1) / (col * own)
    td = float(np.max(err / (CAP * kappa * EPS)[:, None]))
    ninf = lambda A: np.max(np.sum(np.abs(A), axis=2), axis=1)                               # noqa: E731
    si = float(np.max(ninf(Sinv.astype(LD) - Sinv_ref) / ninf(Sinv_ref) / (CAP * kappa ** 2 * EPS)))
    return {"TD": td, "Sinv": si}


def cov_bound(C, Sinv, TD, gm, lin, scale):
    """The entrywise bound of the cov-blocks kernel against the numpy definition: (..., S, n, n)."""
    na = gm.n
    mag = models.separable_global_cov(np.abs(C), np.abs(Sinv), -np.abs(TD), gm, None if scale is None else np.abs(scale),
                                      lin)
    return 4.0 * (na + 1) ** 2 * EPS * np.abs(mag)


# ---- whole fits ------------------------------------------------------------------------------------------------------
TOLS = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)
NOISE = 0.01
# name: (spec, truth, shared, m, G, S, abscissae, sigma)
FITS = {
    "exp": ("exp*2+poly*1", np.array([3.0, 0.7, 1.5, 3.1, 0.2]), (1, 3), 33, 4, 5, "shared", False),
    "gauss": ("gauss+poly*1", np.array([2.0, 0.2, 0.4, 0.3]), (1, 2), 70, 4, 5, "per_set", False),
    "local": ("gauss+poly*1", np.array([2.0, 0.2, 0.4, 0.3]), (2,), 70, 4, 5, "per_set", True),
    "large": ("exp*2+poly*1", np.array([3.0, 1.0, 1.5, 3.1, 0.2]), (1, 3), 16, 2, 300, "shared", False),
}
STARTS = {"exp": {1: 0.9, 3: 2.6}, "gauss": {1: 0.25, 2: 0.45}, "local": {1: 0.25, 2: 0.45},
          "large": {1: 1.0, 3: 1.5}}                                      # the non-linear entries of p0


@functools.lru_cache(maxsize=None)
def fit_data(name):
    """(spec, n, shared, xdata, truth (G, S, n), ydata (G, S, m), sigma or None, p0 plain, p0 separable) of a fit: the
    shared parameters have one value per group, the amplitudes and baselines (and a local non-linear parameter) are
    jittered per data set; noise 0.01 (times sigma).  p0 plain starts the linear entries at the truth; p0 separable has
    NaN there."""
    spec, truth, shared, m, G, S, xs, with_sigma = FITS[name]
    rng = np.random.default_rng(len(name) + 31)
    M = models.resolve(spec)
    n = truth.size
    lin, owner = models.linear_params(spec, n)
    P = np.tile(truth, (G, S, 1))
    P[..., lin] *= 1.0 + 0.3 * rng.uniform(-1.0, 1.0, (G, S, lin.size))
    for j in np.flatnonzero(owner >= 0):
        if j in shared:
            P[..., j] *= 1.0 + 0.02 * rng.standard_normal((G, 1))
        else:
            P[..., j] += 0.05 * rng.standard_normal((G, S))
    if xs == "shared":
        x = np.linspace(0.0, 3.0, m)
        xr = x
    else:
        x = np.linspace(-2.0, 2.0, m) + 0.1 * rng.uniform(-1.0, 1.0, (S, 1))
        xr = np.broadcast_to(x, (G, S, m)).reshape(G * S, m)
    sigma = rng.uniform(0.5, 2.0, (G, S, m)) if with_sigma else None
    Y = M.f(xr, P.reshape(G * S, n)).reshape(G, S, m)
    Y = Y + NOISE * (1.0 if sigma is None else sigma) * rng.standard_normal((G, S, m))
    p0 = P.copy()
    for j, v in STARTS[name].items():
        p0[..., j] = v
    p0_sep = p0.copy()
    p0_sep[..., lin] = np.nan
    for a in (x, P, Y, p0, p0_sep) + (() if sigma is None else (sigma,)):
        a.setflags(write=False)
    return spec, n, shared, x, P, Y, sigma, p0, p0_sep


def reduced_residual(name, g):
    """The reduced residual of group g written out: ``np.linalg.lstsq`` per data set -> (fun(alpha vector), x0, gmap).
    The reference of the fits; it shares nothing with ``varpro_reduce``."""
    spec, n, shared, x, P, Y, sigma, p0, _ = fit_data(name)
    M = models.resolve(spec)
    G, S, m = Y.shape
    gm, lin, owner, non = models.separable_global_map(spec, n, S, shared)
    w = np.ones((S, m)) if sigma is None else 1.0 / sigma[g]
    xr = x if x.ndim == 1 else np.broadcast_to(x, (S, m))

    def fun(v, want_c=False):
        Pm = models.varpro_expand(gm.split_x(v), lin, n)                      # (S, n)
        Phi = M.jac(xr, Pm)[:, :, lin]
        out, cs = [], []
        for s in range(S):
            A = w[s][:, None] * Phi[s]
            c = np.linalg.lstsq(A, w[s] * Y[g, s], rcond=None)[0]
            out.append(A @ c - w[s] * Y[g, s])
            cs.append(c)
        return (np.concatenate(out), np.array(cs)) if want_c else np.concatenate(out)
    return fun, gm.reduce_x(p0[g][:, non]), gm


@functools.lru_cache(maxsize=None)
def scipy_reference(name, g):
    """(popt (S, n), the scipy result) of group g by scipy's ``least_squares`` on ``reduced_residual``."""
    from scipy.optimize import least_squares
    spec, n, shared, x, P, Y, sigma, p0, _ = fit_data(name)
    fun, x0, gm = reduced_residual(name, g)
    lin, owner = models.linear_params(spec, n)
    res = least_squares(fun, x0, method="trf", ftol=1e-14, xtol=1e-14, gtol=1e-14)
    popt = models.varpro_expand(gm.split_x(res.x), lin, n)
    popt[:, lin] = fun(res.x, True)[1]
    return popt, res


def full_blocks(name, g, popt, which, absolute_sigma=False):
    """The (n, n) blocks `which` of the covariance of the FULL problem of group g at `popt` (S, n): the numpy inverse of
    the dense J^T J over all ns + S (n - ns) columns of the plain global fit, times obj / (M - nv_full)."""
    spec, n, shared, x, P, Y, sigma, p0, _ = fit_data(name)
    M = models.resolve(spec)
    G, S, m = Y.shape
    gfull = bounded_lsq.GlobalMap(n, S, shared)
    w = np.ones((S, m)) if sigma is None else 1.0 / sigma[g]
    xr = x if x.ndim == 1 else np.broadcast_to(x, (S, m))
    J = gfull.reduce_jac(w[:, :, None] * M.jac(xr, popt))
    r = (w * (M.f(xr, popt) - Y[g])).ravel()
    C = np.linalg.inv(J.T @ J)
    if not absolute_sigma:
        C = C * (r @ r / (S * m - gfull.nv))
    return np.stack([C[np.ix_(gfull.cols[s], gfull.cols[s])] for s in which])


def agree_with_reference(ref, out, what):
    """popt to rtol 1e-6 / atol 1e-9, and pcov to atol 1e-6 after dividing BOTH by the reference's standard deviations
    (so a wrong variance factor shows)."""
    np.testing.assert_allclose(out[0], ref[0], rtol=1e-6, atol=1e-9, err_msg=str(what))
    d = np.sqrt(np.einsum("...ii->...i", ref[1]))
    norm = d[..., :, None] * d[..., None, :]
    np.testing.assert_allclose(out[1] / norm, ref[1] / norm, rtol=0, atol=1e-6, err_msg=str(what))
