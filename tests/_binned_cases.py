"""Inputs shared by tests/test_binned_cpu.py and tests/test_binned_gpu.py: the grid, the 40-digit
quadrature reference and the measured error figures of the definition test; the model instances, seeded inputs and
first-order error bound of the kernel-level comparison; and the histogram problems of the end-to-end fits."""
import functools

import numpy as np
from scipy import special

from bounded_lsq import models

import _poisson_cases as pc
from _model_cases import worst_ratio  # noqa: F401  (handed on to the tests)

EPS = np.finfo(float).eps

# ---- the definition against 40-digit quadrature ------------------------------------------------------------------------
# Measured (x86-64, numpy + scipy.special float64) over definition_grid(): per term the worst
#     |error| / (eps * magnitude * conditioning)
# of the value and of every column, where `magnitude` is the sum of the absolute values of the summands of the form used
# (value of a gauss: |a s sqrt(pi/2)| (|E_h| + |E_l|) with E the erf or erfc values of the branch taken, so that
# magnitude / |value| is the cancellation factor of the form) and `conditioning` is 1 + max(zl^2, zh^2) for the terms with a
# Gaussian part (the relative sensitivity of erfc(z / sqrt2) and of exp(-z^2 / 2) to the rounding of z) and 1 otherwise.
# The tests allow twice as much.  DESIGN.md 7n records them.
MEASURED = {"gauss": 0.54, "lorentz": 1.53, "pvoigt": 0.34, "exp": 1.86, "poly": 0.85, "gauss2d": 0.84}
# No grid point of any term may lose more than its cancellation factor explains: the error of a VALUE stays below
# LOSS_CAP eps times cancellation factor times conditioning.  2^7: seven bits, against the 53 a plain erf difference loses.
LOSS_CAP = 128.0

ZL = np.concatenate([-np.array([8.0, 6.5, 5.0, 3.0, 1.5, 0.7, 0.2]), [0.0], np.array([0.1, 0.6, 1.4, 2.9, 4.8, 6.4, 8.0])])
WS = np.array([1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0, 3.0])
XS = np.concatenate([[-1e-12, -1e-9, -1e-3, -0.3, -0.4999999, -0.5, -2.0, -10.0, 0.0],
                     [1e-300, 1e-12, 1e-9, 1e-3, 0.3, 0.4999999, 0.5, 0.7, 1.0, 2.0, 5.0, 12.0, 30.0]])


def definition_grid(term, sub=False):
    """Parameters P (G, n_per_term) and bins lo, hi (G,) of one term.  Peaks: zl over [-8, 8] crossed with w / s over
    1e-3 .. 3 (both edges in either tail, bins that straddle the centre) for a = 200, mu = 0.3, s = 1.1 (pvoigt:
    eta = 0.4); exp: x = r w over -10 .. 30 through 0 and +-1e-12, at lo = 0.25 and lo = -1.5 with w = 0.8; poly*4:
    bins of those widths at lo over [-3, 3].  sub: every second zl and every second width (the columns)."""
    zl, ws = (ZL[::2], WS[::2]) if sub else (ZL, WS)
    if term in ("gauss", "lorentz", "pvoigt"):
        a, mu, s = 200.0, 0.3, 1.1
        Z, W = (g.ravel() for g in np.meshgrid(zl, ws, indexing="ij"))
        lo = mu + s * Z
        hi = lo + s * W
        P = np.tile([a, mu, s] + ([0.4] if term == "pvoigt" else []), (Z.size, 1))
        return P, lo, hi
    if term == "exp":
        xs = XS[::2] if sub else XS
        w = 0.8
        lo = np.concatenate([np.full(xs.size, 0.25), np.full(xs.size, -1.5)])
        r = np.concatenate([xs, xs]) / w
        return np.stack([np.full(r.size, 3.0), r], axis=1), lo, lo + w
    if term == "poly":
        L, W = (g.ravel() for g in np.meshgrid(np.linspace(-3.0, 3.0, 7 if not sub else 4), ws, indexing="ij"))
        return np.tile([1.5, -0.7, 0.4, 0.2], (L.size, 1)), L, L + W
    raise ValueError(term)


def gauss2d_grid():
    """Pixels (G, 4) ulo, uhi, vlo, vhi around and far from the centre of P = (a, u0, v0, s, c)."""
    P = np.array([200.0, 0.3, -0.2, 1.1, 5.0])
    zs, ws = np.array([-7.0, -2.0, -0.3, 0.5, 4.0]), np.array([1e-2, 0.7, 2.0])
    ZU, ZV, W = (g.ravel() for g in np.meshgrid(zs, zs[::-1][:3], ws, indexing="ij"))
    ulo, vlo = P[1] + P[3] * ZU, P[2] + P[3] * ZV
    return P, np.stack([ulo, ulo + P[3] * W, vlo, vlo + 0.5 * P[3] * W], axis=1)


def point_term_mp(term):
    """The point-sampled term as an mpmath function of (t, p)."""
    import mpmath as mp
    if term == "gauss":
        return lambda t, p: p[0] * mp.exp(-((t - p[1]) / p[2]) ** 2 / 2)
    if term == "lorentz":
        return lambda t, p: p[0] / (1 + ((t - p[1]) / p[2]) ** 2)
    if term == "pvoigt":
        def pv(t, p):
            q = ((t - p[1]) / p[2]) ** 2
            G, L = mp.exp(-mp.log(2) * q), 1 / (1 + q)
            return p[0] * (G + p[3] * (L - G))
        return pv
    if term == "exp":
        return lambda t, p: p[0] * mp.exp(-p[1] * t)
    if term == "poly":
        return lambda t, p: sum(p[k] * t ** k for k in range(len(p)))
    raise ValueError(term)


def quad_reference(term, P, lo, hi, want_J):
    """mp.quad of the point-sampled term at 40 digits over each bin -> value (G,) and, want_J, its columns (G, n) by
    mp.diff of the quadrature with respect to each parameter; arrays of mpf."""
    import mpmath as mp
    mp.mp.dps = 40
    fun = point_term_mp(term)
    G, n = P.shape
    val = np.empty(G, dtype=object)
    J = np.empty((G, n), dtype=object)
    for g in range(G):
        p = [mp.mpf(float(v)) for v in P[g]]
        a, b = mp.mpf(float(lo[g])), mp.mpf(float(hi[g]))
        pts = [a, b] if not (a < p[1] < b and term != "exp" and term != "poly") else [a, p[1], b]

        def I(q):
            return mp.quad(lambda t: fun(t, q), pts)
        val[g] = I(p)
        if want_J:
            for j in range(n):
                J[g, j] = mp.diff(lambda v: I(p[:j] + [v] + p[j + 1:]), p[j])
    return val, (J if want_J else None)


def err_over(got, ref, scale):
    """|got - ref| / (eps * scale), elementwise, for float64 `got` against mpf `ref`; 0 where both are 0."""
    import mpmath as mp
    out = np.zeros(np.shape(got))
    for idx in np.ndindex(*np.shape(got)):
        d = abs(mp.mpf(float(got[idx])) - ref[idx])
        out[idx] = 0.0 if d == 0 else float(d / (mp.mpf(EPS) * mp.mpf(float(scale[idx]))))
    return out


def erf_parts(xl, xh):
    """The two values whose difference ``models.erf_diff`` returns (first - second) and whether the plain erf branch was
    taken."""
    up, dn = (xl > 0) & (xh > 0), (xl < 0) & (xh < 0)
    first = np.where(up, special.erfc(xl), np.where(dn, special.erfc(-xh), special.erf(xh)))
    second = np.where(up, special.erfc(xh), np.where(dn, special.erfc(-xl), special.erf(xl)))
    return first, second, ~(up | dn)


def term_magnitudes(term, P, lo, hi):
    """Per grid point: the magnitude of the value (G,) and of every column (G, n) (the sums of the absolute values of
    the summands of the forms of ``models.binned``), and the conditioning factor (G,)."""
    a = [np.abs(P[:, k]) for k in range(P.shape[1])]
    p = [P[:, k] for k in range(P.shape[1])]
    one = np.ones(lo.shape)
    if term == "poly":
        n = P.shape[1]
        cols = np.stack([(np.abs(hi) ** (k + 1) + np.abs(lo) ** (k + 1)) / (k + 1) for k in range(n)], axis=1)
        return np.sum(np.abs(P) * cols, axis=1), cols, one
    if term == "exp":
        w = hi - lo
        ps, dp = models.psi_pair(p[1] * w)
        wE = w * np.exp(-(p[1] * lo))
        x = p[1] * w
        with np.errstate(all="ignore"):
            big = (np.abs(x * np.exp(-x)) + np.abs(np.expm1(-x))) / (x * x)
        dpm = np.where(np.abs(x) < models.PSI_X0, np.abs(dp), big)
        da = wE * ps
        return a[0] * da, np.stack([da, a[0] * wE * (w * dpm + np.abs(lo) * ps)], axis=1), one
    s = p[2]
    zl, zh = (lo - p[1]) / s, (hi - p[1]) / s
    cond = 1 + np.maximum(zl * zl, zh * zh)
    atn = np.abs(s) * np.arctan2((hi - lo) / s, 1 + zh * zl)
    Ll, Lh = 1 / (1 + zl * zl), 1 / (1 + zh * zh)
    if term == "lorentz":
        dmu, ds = Ll + Lh, np.abs(zh) * Lh + np.abs(zl) * Ll
        return a[0] * atn, np.stack([atn, a[0] * dmu, a[0] * (atn / np.abs(s) + ds)], axis=1), one
    k, norm, ex = ((models.SQRT_HALF, models.SQRT_PI_2, 0.5) if term == "gauss"
                   else (models.SQRT_LN2, models.PV_GNORM, models.LN2))
    f1, f2, _ = erf_parts(zl * k, zh * k)
    IG = np.abs(s) * norm * (np.abs(f1) + np.abs(f2))
    el, eh = np.exp(-ex * zl * zl), np.exp(-ex * zh * zh)
    gm, gs = el + eh, np.abs(zh) * eh + np.abs(zl) * el
    if term == "gauss":
        return a[0] * IG, np.stack([IG, a[0] * gm, a[0] * (IG / np.abs(s) + gs)], axis=1), cond
    eta = a[3]
    h = IG + eta * (atn + IG)
    dmu = gm + eta * (Ll + Lh + gm)
    ds = gs + eta * (np.abs(zh) * Lh + np.abs(zl) * Ll + gs)
    return a[0] * h, np.stack([h, a[0] * dmu, a[0] * (h / np.abs(s) + ds), a[0] * (atn + IG)], axis=1), cond


# ---- the kernel against the definition ---------------------------------------------------------------------------------
# Measured on an MI355X (tests/test_binned_gpu.py::test_device_functions_stay_inside_their_allowance, which prints them):
# the worst difference between the device's function and the float64 one of numpy / scipy.special on the same argument,
# in units of eps times the value (erfc: times ``erfc_weight``, 1 + x^2), seen through a one-term bin-integrated model on a
# dense grid.  The kernel bound allows each function twice the figure.  DESIGN.md 7n records them.
# A figure below 0.5 is recorded as 0.5 (exp 0.29; erf and expm1 showed nothing beyond the roundings the measurement
# subtracts).
DEVICE_ULP = {"exp": 0.5, "erf": 0.5, "erfc": 2.92, "atan2": 1.0, "expm1": 0.5}
ALLOW = {k: 2.0 * v for k, v in DEVICE_ULP.items()}
TINY = np.finfo(float).tiny                  # a result below the smallest normal number is not held to a relative bound

ROWS = pc.ROWS
B = pc.B
COMP = "gauss+pvoigt+exp+poly*2"
# label -> (named model or composite spec, n, fixed, tied, edge range)
INSTANCES = {
    "gauss_sum": ("gauss_sum", 7, None, None, (-2.0, 2.0)),
    "lorentz_sum": ("lorentz_sum", 7, None, None, (-2.0, 2.0)),
    "exp_sum": ("exp_sum", 5, None, None, (0.0, 4.0)),
    "poly": ("poly", 4, None, None, (0.0, 4.0)),
    "gauss2d": ("gauss2d", 5, None, None, (-2.0, 2.0)),
    "gauss_sum-map": ("gauss_sum", 7, [1], {5: 2}, (-2.0, 2.0)),
    "composite": (COMP, 11, None, None, (-2.0, 2.0)),
    "composite-map": (COMP, 11, [8], {5: 2}, (-2.0, 2.0)),
}


is_composite = functools.partial(pc.mc.is_composite, INSTANCES)
model_of = functools.partial(pc.mc.model_of, INSTANCES)
map_of = functools.partial(pc.mc.map_of, INSTANCES)


def components_of(label):
    name, n = INSTANCES[label][:2]
    return models.binned(name)._components(n)


def kernel_case(label, m, reps, per_problem):
    """Seeded inputs of one kernel comparison -> dict(x, P, X, Pfix, y, ylse, w, pm).  x: the edges as rows, (2, m)
    contiguous bins of random widths over the instance's range when shared, (B, 2, m) bins with gaps (hi drawn inside
    the gap to the next lo) per problem; gauss2d: pixels of sides in [0.05, 0.5].  P (Q, n): amplitudes, widths, rates
    and coefficients in [0.5, 1.5], centres in [-1.5, 1.5] (a composite's p0 raised by 4: its line stays positive).
    Problem 1 has its first peak 30 s outside the range (s = 0.05, the centre at the upper end + 1.5: every bin lies in
    one tail of it) and its decay at r = 1e-9; problem 2 has its first decay at r = 0 (exp_sum: the second at 1e-9).
    y: counts following mu through the eight patterns of ``_poisson_cases.kernel_case``; ylse, w: data and weights of
    the least-squares launches."""
    name, n, fixed, tied, (lo, hi) = INSTANCES[label]
    Mb, pm = models.binned(name), map_of(label)
    Q = B * reps
    rng = np.random.default_rng([sum(label.encode()), m, reps, int(per_problem)])
    P = rng.uniform(0.5, 1.5, (Q, n))
    o = 0
    far, r_cols = [], []
    if name == "gauss2d":
        P[:, 1:3] = rng.uniform(-1.0, 1.0, (Q, 2))
        far = [(1, 3)]
    else:
        for fam, K in components_of(label):
            w = models.TERMS[fam].n_per_term
            for k in range(K if fam != "poly" else 0):
                if fam in ("gauss", "lorentz", "pvoigt"):
                    P[:, o + 1] = rng.uniform(-1.5, 1.5, Q)
                    if not far:
                        far = [(o + 1, o + 2)]
                    if fam == "pvoigt":
                        P[:, o + 3] = rng.uniform(0.1, 0.9, Q)
                if fam == "exp":
                    r_cols.append(o + 1)
                o += w
            if fam == "poly":
                if is_composite(label):
                    P[:, o] += 4.0
                o += K
    for mu_c, s_c in far:
        P[reps:2 * reps, s_c] = 0.05
        P[reps:2 * reps, mu_c] = hi + 30 * 0.05
    if r_cols:
        P[2 * reps:, r_cols[0]] = 0.0
        P[reps:2 * reps, r_cols[0]] = 1e-9
        if len(r_cols) > 1:
            P[2 * reps:, r_cols[1]] = 1e-9
    if Mb.coords == 2:
        shape = ((B,) if per_problem else ()) + (m,)
        ul, vl = rng.uniform(lo, hi - 0.5, shape), rng.uniform(lo, hi - 0.5, shape)
        x = np.stack([ul, ul + rng.uniform(0.05, 0.5, shape), vl, vl + rng.uniform(0.05, 0.5, shape)], axis=-2)
    elif per_problem:
        e = np.sort(rng.uniform(lo, hi, (B, m + 1)), axis=-1)
        x = np.stack([e[:, :-1], e[:, :-1] + rng.uniform(0.5, 1.0, (B, m)) * (e[:, 1:] - e[:, :-1])], axis=-2)
    else:
        x = models.bin_rows(np.sort(rng.uniform(lo, hi, m + 1)))
    x = np.ascontiguousarray(x)
    Pfix = np.ascontiguousarray(P[::reps])
    if pm is not None:
        X = np.ascontiguousarray(pm.reduce_x(P))
        P = pm.expand_x(X, np.repeat(Pfix, reps, axis=0))
    else:
        X = P
    xr = np.repeat(x, reps, axis=0) if per_problem else x
    mu = Mb.f(xr, P)[::reps]
    pattern = (np.arange(m)[np.newaxis, :] + 3 * np.arange(B)[:, np.newaxis]) % 8
    y = np.choose(pattern, [0 * mu, mu, mu / 1.2, mu / 0.8, mu / 1.3, mu / 0.7, np.floor(mu) + 1, mu / 4])
    return dict(x=x, P=P, X=X, Pfix=Pfix, y=np.ascontiguousarray(y), ylse=rng.standard_normal((B, m)),
                w=rng.uniform(0.5, 2.0, (B, m)), pm=pm, per_problem=per_problem)


class Q:
    """A float64 array `v` as the definition computes it, with a first-order bound `e` of the difference between the
    device's value and it.  An operation whose operands are both exact (e == 0) is exact: the kernel performs the
    definition's operations in its order without contraction, so equal inputs give equal bits.  Otherwise the operands'
    bounds are propagated and eps |result| is added: the two roundings, half an ulp each, of the differing results."""

    __array_ufunc__ = None                       # ndarray op Q goes to Q's reflected method

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=float)
        self.e = np.zeros(self.v.shape) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x)

    def _done(self, other, v, e):
        inexact = (self.e > 0) | (other.e > 0)
        return Q(v, np.where(inexact, e + EPS * np.abs(v), 0.0))

    def __add__(self, o):
        o = Q.of(o)
        return self._done(o, self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Q.of(o)
        return self._done(o, self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Q.of(o)
        return self._done(o, self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = Q.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return self._done(o, v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return Q.of(o) - self

    def __rtruediv__(self, o):
        return Q.of(o) / self

    def __neg__(self):
        return Q(-self.v, self.e)


def fn(name, v):
    """The value `v` of the device function `name` at an exact argument: within its allowance of numpy's."""
    v = np.asarray(v, dtype=float)
    return Q(v, ALLOW[name] * (EPS * np.abs(v) + TINY))


def erfc_weight(x):
    """The factor by which the allowance of erfc grows in the tail: scipy.special.erfc forms exp(-x^2) from the rounded
    square, so the DEFINITION's own relative error grows like x^2 eps / 2 (the device's erfc and scipy's
    differ by 125 eps near x = 20 and by less than a handful of eps below x = 1), and the device is compared against it."""
    return 1.0 + x * x


def q_erf_diff(xl, xh):
    first, second, mid = erf_parts(xl, xh)
    up = (xl > 0) & (xh > 0)
    x1, x2 = np.where(up, xl, xh), np.where(up, xh, xl)                    # the arguments of `first` and `second`
    A1 = np.where(mid, ALLOW["erf"], ALLOW["erfc"] * erfc_weight(x1))
    A2 = np.where(mid, ALLOW["erf"], ALLOW["erfc"] * erfc_weight(x2))
    return Q(first, A1 * (EPS * np.abs(first) + TINY)) - Q(second, A2 * (EPS * np.abs(second) + TINY))


def q_psi(x):
    """psi and psi' of ``models.psi_pair``: exact arithmetic below PSI_X0, expm1 and exp above."""
    ps, dp = models.psi_pair(x)
    small = np.abs(x) < models.PSI_X0
    with np.errstate(all="ignore"):
        xs = np.where(small, 1.0, x)
        em, ex = fn("expm1", np.expm1(-xs)), fn("exp", np.exp(-xs))
        qp = -em / xs
        qd = (xs * ex + em) / (xs * xs)
    return Q(ps, np.where(small, 0.0, qp.e)), Q(dp, np.where(small, 0.0, qd.e))


def q_term(fam, lo, hi, p):
    """The operations of one term of ``models.binned`` on Q values: -> value, [columns]."""
    if fam == "exp":
        a, r = p
        w = hi - lo
        ps, dp = q_psi(r * w)
        wE = w * fn("exp", np.exp(-(r * lo)))
        da = wE * ps
        return a * da, [da, (a * wE) * (w * dp - lo * ps)]
    a, mu, s = p[:3]
    zl, zh = (lo - mu) / s, (hi - mu) / s
    if fam in ("lorentz", "pvoigt"):
        IL = s * fn("atan2", np.arctan2((hi - lo) / s, 1.0 + zh * zl))
        Ll, Lh = 1.0 / (1.0 + zl * zl), 1.0 / (1.0 + zh * zh)
    if fam == "lorentz":
        g = a * IL
        return g, [IL, Q(a * (Ll - Lh)), g / s - a * (zh * Lh - zl * Ll)]
    if fam == "gauss":
        da = (s * models.SQRT_PI_2) * q_erf_diff(zl * models.SQRT_HALF, zh * models.SQRT_HALF)
        el, eh = fn("exp", np.exp(-0.5 * (zl * zl))), fn("exp", np.exp(-0.5 * (zh * zh)))
        g = a * da
        return g, [da, a * (el - eh), g / s - a * (zh * eh - zl * el)]
    eta = p[3]
    Gl, Gh = fn("exp", np.exp(-(models.LN2 * (zl * zl)))), fn("exp", np.exp(-(models.LN2 * (zh * zh))))
    IG = (s * models.PV_GNORM) * q_erf_diff(zl * models.SQRT_LN2, zh * models.SQRT_LN2)
    d = IL - IG
    h = IG + eta * d
    g = a * h
    mG = Gl - Gh
    uG = zh * Gh - zl * Gl
    return g, [h, a * (mG + eta * ((Ll - Lh) - mG)), g / s - a * (uG + eta * ((zh * Lh - zl * Ll) - uG)), a * d]


def q_model(label, x, P):
    """The bin-integrated model of `label` at rows x (.., 2 coords, m) and full parameters P (Q, n) on Q values:
    -> value (Q, m), columns [n of (Q, m)].  Polynomials hold no device function: their values are exact."""
    name, n = INSTANCES[label][:2]
    col = lambda k: P[:, k, np.newaxis]                                                # noqa: E731
    if name == "gauss2d":
        ulo, uhi, vlo, vhi = (x[..., r, :] for r in range(4))
        a, u0, v0, s, c = (col(k) for k in range(5))
        zul, zuh, zvl, zvh = (ulo - u0) / s, (uhi - u0) / s, (vlo - v0) / s, (vhi - v0) / s
        c1 = s * models.SQRT_PI_2
        Iu = c1 * q_erf_diff(zul * models.SQRT_HALF, zuh * models.SQRT_HALF)
        Iv = c1 * q_erf_diff(zvl * models.SQRT_HALF, zvh * models.SQRT_HALF)
        da = Iu * Iv
        ww = (uhi - ulo) * (vhi - vlo)
        eul, euh = fn("exp", np.exp(-0.5 * (zul * zul))), fn("exp", np.exp(-0.5 * (zuh * zuh)))
        evl, evh = fn("exp", np.exp(-0.5 * (zvl * zvl))), fn("exp", np.exp(-0.5 * (zvh * zvh)))
        cols = [da, (a * (eul - euh)) * Iv, (a * (evl - evh)) * Iu,
                a * ((Iu / s - (zuh * euh - zul * eul)) * Iv + Iu * (Iv / s - (zvh * evh - zvl * evl))),
                Q(ww + 0 * a)]
        return a * da + c * ww, cols
    lo, hi = x[..., 0, :], x[..., 1, :]
    acc, cols, o = None, [], 0
    for fam, K in components_of(label):
        if fam == "poly":
            ph, pl, v = hi, lo, None
            for k in range(K):
                c = (ph - pl) / (k + 1)
                cols.append(Q(c + 0 * col(o)))
                v = col(o) * c if v is None else v + col(o) * c
                ph, pl = ph * hi, pl * lo
                o += 1
            v = Q(v)
        else:
            w = models.TERMS[fam].n_per_term
            v = None
            for k in range(K):
                g, cs = q_term(fam, lo, hi, [col(o + i) for i in range(w)])
                v = g if v is None else v + g
                cols += cs
                o += w
        acc = v if acc is None else acc + v
    return acc, cols


def expected(label, case, est, reps, weighted=True):
    """The float64 definition of what the entry returns for `case`, and the allowed difference of every entry:
    -> f (Q, m), J (Q, m, nc), f_tol, J_tol.  est 0: f = w (mu - ylse), J = w dmu (weighted: w per problem, else
    w = 1); est 1: the deviance residuals of the counts y and c dmu, with the transform's own roundings counted as in
    tests/test_poisson_gpu.py::test_kernel_against_definition (``_poisson_cases.transform_counts``; both sides are
    float64 here, each within eps T of the exact value)."""
    pm = case["pm"]
    x = np.repeat(case["x"], reps, axis=0) if case["per_problem"] else case["x"]
    v, cols = q_model(label, x, case["P"])
    if pm is not None:                           # a slot: the sequential sum of its columns in ascending order
        slots = []
        for k in range(pm.nf):
            grp = sorted(pm.group(k))
            s = cols[grp[0]]
            for j in grp[1:]:
                s = s + cols[j]
            slots.append(s)
        cols = slots
    if est == 0:
        w = np.repeat(case["w"], reps, axis=0) if weighted else None
        r = v - np.repeat(case["ylse"], reps, axis=0)
        f = w * r if weighted else r
        Jq = [w * c if weighted else c for c in cols]
    else:
        y = np.repeat(case["y"], reps, axis=0)
        rr, cc = models.poisson_transform(v.v, y)
        pos = y > 0
        with np.errstate(all="ignore"):
            u = np.where(pos, (v.v - y) / np.where(pos, y, 1), 0)
        T_r, T_c = pc.transform_counts(u, pos)
        f = Q(rr, np.abs(cc) * v.e + 2 * EPS * T_r * np.abs(rr))
        cq = Q(cc, np.abs(cc) * (2 * EPS * T_c + v.e / np.abs(v.v)))
        Jq = [cq * c for c in cols]
    return (f.v, np.stack([c.v for c in Jq], axis=-1), f.e, np.stack([c.e for c in Jq], axis=-1))


# ---- end to end ----------------------------------------------------------------------------------------------------
TRUTH = np.array([200.0, 0.3, 1.0, 5.0])           # a, mu, s, c of 'gauss_sum' (n = 4): the problem of DESIGN.md 7n's table
TOL = dict(ftol=1e-13, xtol=1e-13, gtol=1e-13)


def table_problem(width=1.5, m=24, Bn=4):
    """Noise-free bin contents of gauss + constant, 24 contiguous bins `width` s wide, the peak 0.37 off the centre of
    the range; the truth perturbed by up to 3 % per problem, p0 10 % off.  -> dict(name, edges, centres, Y, P0, bounds,
    truth)"""
    rng = np.random.default_rng([11, m, Bn])
    truth = TRUTH * (1 + 0.03 * rng.uniform(-1, 1, (Bn, 4)))
    truth[0] = TRUTH
    edges = (0.3 - 0.37) + width * (np.arange(m + 1) - m / 2)
    Y = models.binned("gauss_sum").f(edges, truth)
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    lb = np.broadcast_to([0.0, -10.0, 0.1, 0.0], (Bn, 4)).copy()
    ub = np.broadcast_to([1e4, 10.0, 10.0, 100.0], (Bn, 4)).copy()
    return dict(name="gauss_sum", edges=edges, centres=0.5 * (edges[:-1] + edges[1:]), width=width, Y=Y, P0=P0,
                bounds=(lb, ub), truth=truth)


def histogram_problem(Bn=8, m=48, seed=5):
    """Seeded Poisson histograms of 'gauss+poly*1': m bins 1.5 s wide over the line (a density of ~60 counts per unit
    at the peak, s ~ 0.5, a background density of ~2), drawn once.  -> dict(spec, edges, Y, P0, bounds, truth)"""
    rng = np.random.default_rng([seed, Bn, m])
    truth = np.array([60.0, 0.2, 0.5, 2.0]) * (1 + 0.05 * rng.uniform(-1, 1, (Bn, 4)))
    edges = 0.2 + 0.75 * (np.arange(m + 1) - m / 2)
    spec = "gauss+poly*1"
    Y = rng.poisson(models.binned(spec).f(edges, truth)).astype(float)
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    lb = np.broadcast_to([0.0, -3.0, 0.1, 1e-3], (Bn, 4)).copy()
    ub = np.broadcast_to([1e4, 3.0, 3.0, 100.0], (Bn, 4)).copy()
    return dict(spec=spec, edges=edges, Y=Y, P0=P0, bounds=(lb, ub), truth=truth)


def pixel_problem(Bn=4, side=8, seed=9):
    """Seeded Poisson images of a pixel-integrated gauss2d on a side x side grid of unit pixels (m = 64): a spot of
    s ~ 1.1 pixels, ~400 counts, over a background of ~2 counts per pixel.  -> dict(x (4, m), Y, P0, bounds, truth)"""
    rng = np.random.default_rng([seed, Bn, side])
    truth = np.array([55.0, 3.7, 4.2, 1.1, 2.0]) * (1 + 0.05 * rng.uniform(-1, 1, (Bn, 5)))
    U, V = (g.ravel().astype(float) for g in np.meshgrid(np.arange(side), np.arange(side), indexing="ij"))
    x = np.stack([U, U + 1, V, V + 1])
    Y = rng.poisson(models.binned("gauss2d").f(x, truth)).astype(float)
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    lb = np.broadcast_to([0.0, 0.0, 0.0, 0.3, 1e-3], (Bn, 5)).copy()
    ub = np.broadcast_to([1e4, 8.0, 8.0, 4.0, 100.0], (Bn, 5)).copy()
    return dict(x=x, Y=Y, P0=P0, bounds=(lb, ub), truth=truth)


def binned_score(name, x, Y, P, pm=None):
    """The Poisson score of the bin-integrated model, as ``_poisson_cases.score``: -> S, sum |summands|, both (B, n)."""
    M = models.binned(name)
    mu, J = M.f(x, P), M.jac(x, P)
    if pm is not None:
        J = pm.reduce_jac(J)
    S = (1 - Y / mu)[:, :, np.newaxis] * J
    return S.sum(axis=1), np.abs(S).sum(axis=1)
