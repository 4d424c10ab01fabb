"""`curve_fit` / `curve_fit_batch` on the GPU: the plumbing against this package's own `least_squares` and
`covariance(..., pinv=True)`, and the results against scipy.optimize.curve_fit(method='trf').

Covariances are compared in the project's metric, max |C - C*|_ij / sqrt(C*_ii C*_jj), against the mpmath reference of
the final Jacobian (tests/_pinv_ref.py), bounded by max(4 x the float64 recipe's error, 8 n eps)."""
import warnings

import numpy as np
import pytest
import scipy.optimize as so
from scipy.linalg import cholesky, solve_triangular

import _cov_ref as ref
import _pinv_ref as pref

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
TOL = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


# ---- models ------------------------------------------------------------------------------------------
def gauss(x, a, mu, w):
    return a * np.exp(-0.5 * ((x - mu) / w) ** 2)


def dgauss(x, a, mu, w):
    e = np.exp(-0.5 * ((x - mu) / w) ** 2)
    return np.stack([e, a * e * (x - mu) / w ** 2, a * e * (x - mu) ** 2 / w ** 3], axis=1)


def twoexp(x, a, k, b, l):
    return a * np.exp(-k * x) + b * np.exp(-l * x)


def dtwoexp(x, a, k, b, l):
    e1, e2 = np.exp(-k * x), np.exp(-l * x)
    return np.stack([e1, -a * x * e1, e2, -b * x * e2], axis=1)


def _data(model, x, p, seed):
    rng = np.random.default_rng(seed)
    sigma = 0.02 * (1 + 0.5 * rng.uniform(size=x.size))
    return model(x, *p) + sigma * rng.standard_normal(x.size), sigma


PLUMBING = [
    ("gauss", gauss, dgauss, np.linspace(-3, 3, 60), [2.4, 0.0, 1.0], [2.0, 0.2, 1.2], (-np.inf, np.inf)),
    ("gauss bounded", gauss, dgauss, np.linspace(-3, 3, 60), [2.4, 0.0, 1.0], [2.0, 0.2, 1.2],
     ([0.0, -1.0, 0.1], [2.2, 1.0, 5.0])),                         # the amplitude is cut off at 2.2
    ("twoexp", twoexp, dtwoexp, np.linspace(0, 4, 80), [3.0, 2.0, 1.0, 0.3], [2.5, 1.5, 1.5, 0.5], (-np.inf, np.inf)),
    ("twoexp bounded", twoexp, dtwoexp, np.linspace(0, 4, 80), [3.0, 2.0, 1.0, 0.3], [2.5, 1.5, 1.5, 0.5],
     ([0.0, 0.0, 0.0, 0.0], [10.0, 10.0, 10.0, 10.0])),
]


@pytest.mark.parametrize("label,model,dmodel,x,truth,p0,bounds", PLUMBING, ids=[c[0] for c in PLUMBING])
def test_plumbing(ctx, label, model, dmodel, x, truth, p0, bounds):
    import bounded_lsq
    y, sigma = _data(model, x, truth, 31)
    m, n = x.size, len(p0)
    kw = dict(bounds=bounds, options={"ctx": ctx})
    popt, pcov = bounded_lsq.curve_fit(model, x, y, p0=p0, sigma=sigma, jac=dmodel, **kw)
    popt_a, pcov_a = bounded_lsq.curve_fit(model, x, y, p0=p0, sigma=sigma, jac=dmodel, absolute_sigma=True, **kw)
    w = 1.0 / sigma
    res = bounded_lsq.least_squares(lambda p: w * (model(x, *p) - y), p0, jac=lambda p: w[:, None] * dmodel(x, *p), **kw)
    assert res.success
    assert np.array_equal(popt, res.x) and np.array_equal(popt_a, res.x)
    C, rank, rcond, kept, status = bounded_lsq.covariance(res.jac, ctx=ctx, pinv=True)
    assert status == 0 and rank == n
    assert np.array_equal(pcov_a, C)
    want = C * (res.obj_value / (m - n))
    assert np.all(np.abs(pcov - want) <= 2 * np.spacing(np.abs(want)))
    assert np.array_equal(pcov, pcov.T)
    # finite differences ('2-point', jac=None) reach the same fit
    # (both to tight tolerances: what is left is the 1e-8 relative error of the forward differences in the
    # stationarity condition, amplified by the conditioning of these fits — 2e-6 at most in scipy's own hands)
    popt_fd, _ = bounded_lsq.curve_fit(model, x, y, p0=p0, sigma=sigma, **kw, **TOL)
    popt_an, _ = bounded_lsq.curve_fit(model, x, y, p0=p0, sigma=sigma, jac=dmodel, **kw, **TOL)
    np.testing.assert_allclose(popt_fd, popt_an, rtol=1e-4, atol=1e-7)
    out = bounded_lsq.curve_fit(model, x, y, p0=p0, sigma=sigma, jac=dmodel, full_output=True, **kw)
    assert np.array_equal(out[2]["fvec"], res.fun) and out[2]["nfev"] == res.nfev and out[4] == res.status


# ---- against scipy: models linear in the parameters -------------------------------------------------------


def _poly4():
    x = np.linspace(-1, 1, 50)
    A = np.vander(x, 5, increasing=True)
    rng = np.random.default_rng(41)
    sigma = 0.1 * (1 + rng.uniform(size=50))
    y = A @ np.array([1.0, -2.0, 0.5, 3.0, -1.0]) + sigma * rng.standard_normal(50)

    def f(x, a, b, c, d, e):
        return a + x * (b + x * (c + x * (d + x * e)))

    return f, (lambda x, *p: A), x, y, sigma, sigma, 5


def _basis6(duplicate=False):
    x = np.linspace(0, 2, 200)
    cols = [np.ones_like(x), x, np.sin(3 * x), np.cos(3 * x), np.exp(-x), x * x]
    if duplicate:
        cols[5] = cols[2]                                          # two identical basis functions
    A = np.stack(cols, axis=1)
    rng = np.random.default_rng(42)
    i = np.arange(200)
    S = 0.01 * (0.6 ** np.abs(i[:, None] - i[None, :])) * (1 + 0.5 * np.sin(0.1 * i))[:, None] \
        * (1 + 0.5 * np.sin(0.1 * i))[None, :]                      # an AR(1)-like covariance, positive definite
    y = A @ np.array([0.5, -1.0, 2.0, 0.7, 1.5, 0.3]) + cholesky(S, lower=True) @ rng.standard_normal(200)

    def f(x, a, b, c, d, e, g):
        return A @ np.array([a, b, c, d, e, g])

    return f, (lambda x, *p: A), x, y, S, S, 6


@pytest.mark.parametrize("make", [_poly4, _basis6], ids=["poly4 m=50", "basis6 m=200 2-D sigma"])
def test_linear_models_against_scipy(ctx, make):
    import bounded_lsq
    f, df, x, y, sigma, _, n = make()
    m = y.size
    p0 = np.zeros(n)
    popt, pcov = bounded_lsq.curve_fit(f, x, y, p0=p0, sigma=sigma, jac=df, options={"ctx": ctx}, **TOL)
    popt_s, pcov_s = so.curve_fit(f, x, y, p0=p0, sigma=sigma, jac=df, method='trf', **TOL)
    np.testing.assert_allclose(popt, popt_s, rtol=1e-9, atol=1e-12)
    # the transformed Jacobian does not depend on p: one reference serves both
    A = df(x)
    # (formed as curve_fit forms it, so that it is the Jacobian of both fits to the bit)
    J = (1.0 / sigma)[:, None] * A if np.ndim(sigma) == 1 else \
        solve_triangular(cholesky(sigma, lower=True), A, lower=True)
    r = pref.reference_small(J)
    assert r["rank"] == n

    def s2(p):
        res = (1.0 / sigma) * (f(x, *p) - y) if np.ndim(sigma) == 1 else \
            solve_triangular(cholesky(sigma, lower=True), f(x, *p) - y, lower=True)
        return float(res @ res) / (m - n)
    s2_o, s2_s = s2(popt), s2(popt_s)
    print("s^2: ours %.17g, scipy %.17g, relative difference %.3g (allowed %.3g)"
          % (s2_o, s2_s, abs(s2_o - s2_s) / s2_s, 16 * m * EPS))
    assert abs(s2_o - s2_s) <= 16 * m * EPS * s2_s
    pref.check(pcov / s2_o, r, "ours: pcov / s^2")
    e_s = ref.cov_error(pcov_s / s2_s, r["C"])
    print("scipy: pcov / s^2 error %.3g" % e_s)
    assert e_s <= r["bound"]
    assert ref.cov_error(pcov / s2_o, np.asarray(pcov_s / s2_s, dtype=ref.LD)) <= 2 * r["bound"] * (1 + 1e-10)
    _, pcov_abs = bounded_lsq.curve_fit(f, x, y, p0=p0, sigma=sigma, jac=df, absolute_sigma=True,
                                        options={"ctx": ctx}, **TOL)
    pref.check(pcov_abs, r, "ours: absolute_sigma")


def test_rank_deficient_linear_model(ctx):
    import bounded_lsq
    f, df, x, y, S, _, n = _basis6(duplicate=True)
    m = y.size
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # no 'could not be estimated' warning
        popt, pcov = bounded_lsq.curve_fit(f, x, y, p0=np.zeros(n), sigma=S, jac=df, absolute_sigma=True,
                                           options={"ctx": ctx}, **TOL)
    assert np.all(np.isfinite(pcov))
    J = solve_triangular(cholesky(S, lower=True), df(x), lower=True)
    r = pref.reference_small(J)
    assert r["rank"] == n - 1
    pref.check(pcov, r, "rank-deficient basis: pcov (absolute_sigma)")
    L = cholesky(S, lower=True)
    res = bounded_lsq.least_squares(lambda p: solve_triangular(L, f(x, *p) - y, lower=True), np.zeros(n),
                                    jac=lambda p: J, covariance=True, options={"ctx": ctx}, **TOL)
    assert res.x_covariance is None                                # the inverse route has nothing here
    res = bounded_lsq.least_squares(lambda p: solve_triangular(L, f(x, *p) - y, lower=True), np.zeros(n),
                                    jac=lambda p: J, covariance='pinv', options={"ctx": ctx}, **TOL)
    assert res.x_covariance_rank == n - 1 and res.x_covariance_rcond < 1e-13
    # the scaled one against scipy's own
    _, pcov_v = bounded_lsq.curve_fit(f, x, y, p0=np.zeros(n), sigma=S, jac=df, options={"ctx": ctx}, **TOL)
    popt_s, pcov_s = so.curve_fit(f, x, y, p0=np.zeros(n), sigma=S, jac=df, method='trf', **TOL)
    s2 = res.obj_value / (m - n)
    fs = solve_triangular(L, f(x, *popt_s) - y, lower=True)
    s2_s = float(fs @ fs) / (m - n)
    assert abs(s2 - s2_s) <= 16 * m * EPS * s2_s
    pref.check(pcov_v / s2, r, "rank-deficient basis: pcov / s^2")
    assert ref.cov_error(pcov_s / s2_s, r["C"]) <= r["bound"]


def test_nonlinear_bounded_model_against_scipy(ctx):
    import bounded_lsq
    x = np.linspace(-3, 3, 60)
    y, sigma = _data(gauss, x, [2.4, 0.0, 1.0], 31)
    bounds = ([0.0, -1.0, 0.1], [2.2, 1.0, 5.0])
    popt, _ = bounded_lsq.curve_fit(gauss, x, y, p0=[2.0, 0.2, 1.2], sigma=sigma, jac=dgauss, bounds=bounds,
                                    options={"ctx": ctx}, **TOL)
    popt_s, _ = so.curve_fit(gauss, x, y, p0=[2.0, 0.2, 1.2], sigma=sigma, jac=dgauss, bounds=bounds, method='trf',
                             **TOL)
    np.testing.assert_allclose(popt, popt_s, rtol=1e-6, atol=1e-9)
    assert abs(popt[0] - 2.2) < 1e-6                                # on its bound


# ---- curve_fit_batch -------------------------------------------------------------------------------------
def _peaks(B=9, m=60):
    x = np.linspace(-3, 3, m)
    rng = np.random.default_rng(21)
    truth = np.array([[2 + 0.1 * b, 0.05 * (b - 4), 0.8 + 0.05 * b] for b in range(B)])
    sig = 0.02 * (1 + 0.5 * rng.uniform(size=(B, m)))
    Y = truth[:, 0:1] * np.exp(-0.5 * ((x - truth[:, 1:2]) / truth[:, 2:3]) ** 2) + sig * rng.standard_normal((B, m))
    P0 = truth * np.array([1.2, 1.0, 1.15]) + np.array([0.0, 0.1, 0.0])

    def fb(x, P):
        return P[:, 0:1] * np.exp(-0.5 * ((x - P[:, 1:2]) / P[:, 2:3]) ** 2)

    def jb(x, P):
        a, mu, w = P[:, 0:1], P[:, 1:2], P[:, 2:3]
        e = np.exp(-0.5 * ((x - mu) / w) ** 2)
        return np.stack([e, a * e * (x - mu) / w ** 2, a * e * (x - mu) ** 2 / w ** 3], axis=2)
    return x, Y, sig, P0, fb, jb


@pytest.fixture(scope="module")
def peaks_alone(ctx):
    """curve_fit on each of the nine problems alone (computed once)."""
    import bounded_lsq
    x, Y, sig, P0, fb, jb = _peaks()
    return [bounded_lsq.curve_fit(gauss, x, Y[b], p0=P0[b], sigma=sig[b], jac=dgauss, options={"ctx": ctx},
                                  ftol=1e-10, xtol=1e-10, gtol=1e-10) for b in range(Y.shape[0])]


@pytest.mark.parametrize("driver", ["host", "device"])
def test_curve_fit_batch(ctx, peaks_alone, driver):
    import bounded_lsq
    x, Y, sig, P0, fb, jb = _peaks()
    B, m = Y.shape
    n = 3
    kw = dict(sigma=sig, jac=jb, driver=driver, ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    popt, pcov, res = bounded_lsq.curve_fit_batch(fb, x, Y, P0, **kw)
    _, pcov_abs, _ = bounded_lsq.curve_fit_batch(fb, x, Y, P0, absolute_sigma=True, **kw)
    assert popt.shape == (B, n) and pcov.shape == (B, n, n) and len(res) == B
    for b in range(B):
        assert res[b].success and res[b].x_covariance_rank == n
        np.testing.assert_allclose(popt[b], peaks_alone[b][0], rtol=1e-9, atol=1e-12)
        # the covariance of the batch's own final Jacobian, within the bound; scaled by ITS s^2
        r = pref.reference_small(res[b].jac)
        s2 = res[b].obj_value / (m - n)
        pref.check(pcov[b] / s2, r, "%s problem %d: pcov / s^2" % (driver, b))
        pref.check(pcov_abs[b], r, "%s problem %d: absolute_sigma" % (driver, b))
        assert np.array_equal(pcov[b], res[b].x_covariance)
        # ... and curve_fit's on the problem alone, as far as two fits that agree to 1e-9 in popt can
        np.testing.assert_allclose(pcov[b], peaks_alone[b][1], rtol=1e-6, atol=0)


@pytest.mark.parametrize("driver", ["host", "device"])
def test_curve_fit_batch_keeps_going_past_a_problem_that_hits_max_nfev(ctx, driver):
    import bounded_lsq
    x, Y, sig, P0, fb, jb = _peaks()
    B = Y.shape[0]
    kw = dict(sigma=sig, jac=jb, driver=driver, ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    good = bounded_lsq.curve_fit_batch(fb, x, Y, P0, maxfev=9, **kw)
    assert all(r.success for r in good[2])
    far = P0.copy()
    far[4] = [50.0, 0.0, 0.05]                                      # needs well over 9 evaluations
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        popt, pcov, res = bounded_lsq.curve_fit_batch(fb, x, Y, far, maxfev=9, **kw)
    assert res[4].status == 0 and not res[4].success and res[4].nfev == 9
    assert np.all(np.isnan(popt[4])) and np.all(np.isnan(pcov[4]))
    for b in range(B):
        if b != 4:
            assert res[b].success
            assert np.array_equal(popt[b], good[0][b]) and np.array_equal(pcov[b], good[1][b]), b
