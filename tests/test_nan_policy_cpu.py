"""Missing data in batch fits (nan_policy='omit') on the host: the numpy definition ``models.omit_residual`` /
``omit_jacobian``, ``count_observed``, ``pad_ragged``, the keyword checks of ``curve_fit_batch`` on a stubbed solve,
``curve_fit``'s error paths against scipy's, the per-problem variance factor, and the fit problems of the GPU file."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.optimize as so
from scipy.optimize import OptimizeResult, OptimizeWarning

import bounded_lsq
from bounded_lsq import ParamMap, models

import _nan_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu(*a, **k):
    raise AssertionError("the GPU was touched")


@pytest.fixture
def nogpu(monkeypatch):
    from bounded_lsq import _abi, _hip_step
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)


# ---- the definition ------------------------------------------------------------------------------------------------
def _host_models():
    """label -> (fres(x, P), jres(x, P) of the whole residual for data (x, y, sigma), P (B, n), x, m): a named, a
    composite, a mapped, a Poisson and a binned host model."""
    rng = np.random.default_rng(5)
    B, m = 3, 9
    x = np.sort(rng.uniform(0.0, 4.0, (B, m)), axis=1)
    out = {}

    def lse(M, x):
        def make(y, sg):
            return (lambda xx, P: (M.f(xx, P) - y) / sg), (lambda xx, P: M.jac(xx, P) / sg[:, :, None])
        return make
    G = models.get("gauss_sum")
    out["named"] = (lse(G, x), rng.uniform(0.5, 2.0, (B, 4)), x)
    C = models.compose("gauss+lorentz+poly*2")
    out["composite"] = (lse(C, x), rng.uniform(0.5, 2.0, (B, 8)), x)
    pm = ParamMap(7, fixed=[6], tied={5: 2})
    P7 = rng.uniform(0.5, 2.0, (B, 7))

    def mapped(y, sg):
        G7 = models.get("gauss_sum")
        f = pm.wrap_f(G7.f, P7)
        j = pm.wrap_jac(G7.jac, P7)
        return (lambda xx, X: (f(xx, X) - y) / sg), (lambda xx, X: j(xx, X) / sg[:, :, None])
    out["mapped"] = (mapped, pm.reduce_x(P7), x)

    def poisson(y, sg):
        return models.poisson_residual(G.f, y), models.poisson_jacobian(G.f, G.jac, y)
    out["poisson"] = (poisson, rng.uniform(0.5, 2.0, (B, 4)), x)
    Bn = models.binned("gauss_sum")
    edges = np.stack([x, x + 0.2], axis=1)                                   # rows lo, hi: (B, 2, m)
    out["binned"] = (lse(Bn, edges), rng.uniform(0.5, 2.0, (B, 4)), edges)
    return out, B, m


@pytest.mark.parametrize("label", ["named", "composite", "mapped", "poisson", "binned"])
def test_omit_is_zero_exactly_where_ydata_is_nan(label):
    """Zeros exactly where ydata is NaN, although sigma and the abscissa are NaN there too; every other entry has the bits
    of the unwrapped function on data with the NaN replaced by 1.0."""
    cases, B, m = _host_models()
    make, P, x = cases[label]
    rng = np.random.default_rng(6)
    y_clean = rng.uniform(1.0, 5.0, (B, m))
    sg_clean = rng.uniform(0.5, 2.0, (B, m))
    om = np.zeros((B, m), dtype=bool)
    om[0, 0] = om[1, m - 1] = True
    om[2, ::2] = True
    y = np.where(om, np.nan, y_clean)
    sg = np.where(om, np.nan, sg_clean)
    xn = np.where(om[:, None, :] if x.ndim == 3 else om, np.nan, x)
    fres, jres = make(y, sg)
    f = models.omit_residual(fres, y)(xn, P)
    J = models.omit_jacobian(jres, y)(xn, P)
    f_ref, j_ref = make(np.where(om, 1.0, y_clean), sg_clean)
    f_ref, J_ref = f_ref(x, P), j_ref(x, P)
    assert f.shape == (B, m) and J.shape == (B, m, P.shape[1])
    assert np.all(f.view(np.uint64)[om] == 0) and np.all(J.view(np.uint64)[om] == 0)          # +0.0, not -0.0
    assert np.array_equal(f[~om].view(np.uint64), f_ref[~om].view(np.uint64))
    assert np.array_equal(J[~om].view(np.uint64), J_ref[~om].view(np.uint64))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(J)) and np.any(f[~om] != 0)


def test_count_observed():
    y = np.array([[1.0, np.nan, 3.0, np.inf], [np.nan] * 4, [0.0, -np.inf, 2.0, 5.0]])
    k = models.count_observed(y)
    assert k.dtype == np.int32 and k.tolist() == [3, 0, 4]
    with pytest.raises(ValueError, match=r"shape \(B, m\)"):
        models.count_observed(np.ones(4))
    assert models.NAN_POLICIES == ('propagate', 'omit')


def test_pad_ragged():
    xs = [np.arange(3.0), np.arange(5.0) * 2, [7.0]]
    ys = [np.ones(3), np.arange(5.0), [2.0]]
    X, Y = models.pad_ragged(xs, ys)
    assert X.shape == Y.shape == (3, 5) and X.dtype == Y.dtype == np.float64
    assert np.array_equal(X[0], [0, 1, 2, 2, 2]) and np.array_equal(X[1], np.arange(5.0) * 2)
    assert np.array_equal(X[2], [7.0] * 5)
    assert np.array_equal(np.isnan(Y), [[0, 0, 0, 1, 1], [0] * 5, [0, 1, 1, 1, 1]])
    assert np.array_equal(Y[1], np.arange(5.0)) and Y[2, 0] == 2.0
    assert models.count_observed(Y).tolist() == [3, 5, 1]
    with pytest.raises(ValueError, match="data set 1: x has 5 points, y has 4"):
        models.pad_ragged(xs, [np.ones(3), np.ones(4), [2.0]])
    with pytest.raises(ValueError):
        models.pad_ragged(xs, ys[:2])
    with pytest.raises(ValueError, match="1-D"):
        models.pad_ragged([np.ones((2, 2))], [np.ones((2, 2))])


# ---- curve_fit_batch: the keyword on a stubbed solve ---------------------------------------------------------------
class _BatchSolve:
    def __init__(self):
        self.calls = []

    def __call__(self, fun, X0, jac, **kw):
        self.calls.append(dict(kw, fun=fun, jac=jac, X0=X0))
        B, n = X0.shape
        F = fun(X0) if callable(fun) else np.zeros((B, fun.m))
        out = []
        for b in range(B):
            r = OptimizeResult(x=X0[b] + b, fun=F[b], jac=np.ones((F.shape[1], n)), obj_value=2.0,
                               x_covariance=np.eye(n) * (b + 1), status=1, active_mask=np.zeros(n, dtype=int))
            r.success = True
            out.append(r)
        return out


X6 = np.linspace(0.0, 1.0, 6)


def fb(x, P):
    return P[:, 0:1] + P[:, 1:2] * x


def jb(x, P):
    return np.broadcast_to(np.stack([np.ones_like(x), x], axis=1), (P.shape[0], x.size, 2))


@pytest.fixture
def solve(monkeypatch, nogpu):
    from bounded_lsq import _curve_fit
    s = _BatchSolve()
    monkeypatch.setattr(_curve_fit, "least_squares_batch", s)
    return s


def _ydata():
    Y = np.stack([1.0 + 2.0 * X6, 2.0 + X6, 3.0 * X6 + 1.0])
    Y[0, 1] = Y[2, 4] = Y[2, 5] = np.nan
    return Y


def test_keyword_validation(solve):
    Y, P0 = _ydata(), np.ones((3, 2))
    with pytest.raises(ValueError, match="The input contains nan values"):
        bounded_lsq.curve_fit_batch(fb, X6, Y, P0, nan_policy='raise')
    bounded_lsq.curve_fit_batch(fb, X6, np.nan_to_num(Y, nan=1.0), P0, nan_policy='raise')          # no NaN: fine
    for bad in ('propagate', 'drop', 'Omit'):
        with pytest.raises(ValueError, match="`nan_policy` must be None, 'raise' or 'omit'"):
            bounded_lsq.curve_fit_batch(fb, X6, Y, P0, nan_policy=bad)
    Y0 = Y.copy()
    Y0[1] = np.nan
    with pytest.raises(ValueError, match="problem 1 has no point left"):
        bounded_lsq.curve_fit_batch(fb, X6, Y0, P0, nan_policy='omit')
    assert len(solve.calls) == 1


def test_poisson_checks_look_at_the_kept_points(solve):
    Y, P0 = np.abs(_ydata()), np.ones((3, 2))
    kw = dict(estimator='poisson', nan_policy='omit')
    bounded_lsq.curve_fit_batch(fb, X6, Y, P0, **kw)
    Yi = Y.copy()
    Yi[1, 2] = np.inf
    with pytest.raises(ValueError, match="must be finite"):
        bounded_lsq.curve_fit_batch(fb, X6, Yi, P0, **kw)
    Yn = Y.copy()
    Yn[1, 2] = -1.0
    with pytest.raises(ValueError, match="must not be negative"):
        bounded_lsq.curve_fit_batch(fb, X6, Yn, P0, **kw)
    with pytest.raises(ValueError, match="must be finite"):                   # a NaN and no policy: still an error
        bounded_lsq.curve_fit_batch(fb, X6, Y, P0, estimator='poisson')
    assert len(solve.calls) == 1


def test_omit_wraps_the_callables_and_reports_nobs(solve):
    """The residual and Jacobian handed to the solve are zero at the omitted points (a NaN sigma there is accepted),
    `_nobs` carries the counts, the results gain nobs / omitted, and a problem with nobs <= n gets pcov = inf under one
    warning while its mates keep theirs."""
    Y, P0 = _ydata(), np.ones((3, 2))
    Y[1, :4] = np.nan                                                         # problem 1 keeps 2 = n points
    sig = np.random.default_rng(1).uniform(0.5, 2.0, Y.shape)
    sig[np.isnan(Y)] = np.nan
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        popt, pcov, res = bounded_lsq.curve_fit_batch(fb, X6, Y, P0, sigma=sig, jac=jb, nan_policy='omit')
    assert [w.category for w in rec] == [OptimizeWarning]
    c = solve.calls[0]
    assert c["_nobs"].tolist() == [5, 2, 4] and c["_variance_scale"] is True
    om = np.isnan(Y)
    F, J = c["fun"](P0), c["jac"](P0)
    assert np.all(F[om] == 0) and np.all(J[om] == 0) and np.all(np.isfinite(F)) and np.all(np.isfinite(J))
    ref = (1.0 / np.where(om, 1.0, sig)) * (fb(X6, P0) - np.where(om, 0.0, Y))       # transform * (f - y)
    assert np.array_equal(F[~om], ref[~om])
    assert [r.nobs for r in res] == [5, 2, 4] and all(np.array_equal(r.omitted, om[b]) for b, r in enumerate(res))
    assert np.all(np.isinf(pcov[1])) and np.array_equal(pcov[0], np.eye(2)) and np.array_equal(pcov[2], 3 * np.eye(2))
    # without the keyword nothing of this is passed on
    bounded_lsq.curve_fit_batch(fb, X6, np.nan_to_num(Y, nan=1.0), P0)
    assert "_nobs" not in solve.calls[1] and not hasattr(res[0], "nothing")


def test_device_fit_carries_the_policy(solve):
    Y, P0 = _ydata(), np.ones((3, 4))
    Y[2, 5] = 1.0                                                             # every problem keeps more than n = 4
    sig = np.ones_like(Y)
    sig[np.isnan(Y)] = np.inf
    bounded_lsq.curve_fit_batch('gauss_sum', X6, Y, P0, sigma=sig, driver='device', nan_policy='omit')
    fit = solve.calls[0]["fun"]
    assert isinstance(fit, models.DeviceFit) and fit.nan_policy == 'omit'
    bounded_lsq.curve_fit_batch('gauss_sum', X6, np.nan_to_num(Y, nan=1.0), P0, driver='device')
    assert solve.calls[1]["fun"].nan_policy == 'propagate'
    with pytest.raises(ValueError, match="unknown NaN policy"):
        models.DeviceFit('gauss_sum', 4, X6, Y, nan_policy='raise')


# ---- curve_fit: scipy's keyword, scipy's errors --------------------------------------------------------------------
def line(x, a, b):
    return a + b * x


def _both_raise(kwargs, y):
    with pytest.raises(Exception) as es:
        so.curve_fit(line, X6, y, method='trf', **kwargs)
    with pytest.raises(type(es.value)) as eo:
        bounded_lsq.curve_fit(line, X6, y, **kwargs)
    assert str(eo.value) == str(es.value), (str(eo.value), str(es.value))
    return es.value


def test_curve_fit_error_paths_are_scipys(nogpu):
    y = 1.0 + 2.0 * X6
    yn = y.copy()
    yn[2] = np.nan
    assert "propagate" in str(_both_raise(dict(nan_policy='propagate'), yn))
    assert "nan values" in str(_both_raise(dict(nan_policy='raise'), yn))
    assert "nan_policy must be one of" in str(_both_raise(dict(nan_policy='drop'), yn))
    assert isinstance(_both_raise(dict(), yn), ValueError)                    # check_finite resolves to True
    assert isinstance(_both_raise(dict(nan_policy='omit', check_finite=True), yn), ValueError)


def test_curve_fit_omit_drops_points_and_sigma(monkeypatch, nogpu):
    """'omit' hands the solver the compressed problem: the points where x or y is NaN are gone, with the matching entries
    of a 1-D sigma and the rows and columns of a 2-D one; also through the mapped route."""
    from bounded_lsq import _curve_fit
    seen = []

    def fake(func, p0, **kw):
        seen.append(np.asarray(func(np.asarray(p0, float))))
        return OptimizeResult(x=np.asarray(p0, float), fun=seen[-1], success=True, status=1, message="", nfev=1,
                              obj_value=1.0, x_covariance=np.eye(len(p0)))
    monkeypatch.setattr(_curve_fit, "least_squares", fake)
    y = 1.0 + 2.0 * X6
    yn, xn = y.copy(), X6.copy()
    yn[2] = xn[4] = np.nan
    keep = np.array([1, 1, 0, 1, 0, 1], dtype=bool)
    sg = np.linspace(1.0, 2.0, 6)
    bounded_lsq.curve_fit(line, xn, yn, p0=[0.5, 0.5], sigma=sg, nan_policy='omit')
    assert np.array_equal(seen[-1], (1.0 / sg[keep]) * (line(X6[keep], 0.5, 0.5) - y[keep]))
    S = np.diag(sg ** 2)
    bounded_lsq.curve_fit(line, xn, yn, p0=[0.5, 0.5], sigma=S, nan_policy='omit')
    np.testing.assert_allclose(seen[-1], (line(X6[keep], 0.5, 0.5) - y[keep]) / sg[keep], rtol=1e-15)
    bounded_lsq.curve_fit(line, xn, yn, p0=[0.5, 0.5], nan_policy='omit', fixed=[1])
    assert np.array_equal(seen[-1], line(X6[keep], 0.5, 0.5) - y[keep])


# ---- the variance factor -------------------------------------------------------------------------------------------
def test_variance_scales_per_problem():
    from bounded_lsq import _cov
    res = [OptimizeResult(obj_value=6.0, jac=np.ones((10, 3))), OptimizeResult(obj_value=4.0, jac=np.ones((10, 3))),
           OptimizeResult(obj_value=2.0, jac=np.ones((10, 3))), OptimizeResult(obj_value=5.0, jac=np.ones((10, 3)))]
    assert np.array_equal(_cov.variance_scales(res), [6 / 7, 4 / 7, 2 / 7, 5 / 7])
    got = _cov.variance_scales(res, np.array([9, 4, 3, 2], dtype=np.int32))
    assert np.array_equal(got, [6.0 / 6, 4.0 / 1, np.inf, np.inf])
    with pytest.raises(ValueError, match=r"shape \(B,\)"):
        _cov.variance_scales(res, np.array([9, 4]))


# ---- the ABI -------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_entries():
    from bounded_lsq import _abi
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"enum\s*\{\s*BLSQ_NAN_PROPAGATE\s*=\s*0\s*,\s*BLSQ_NAN_OMIT\s*\}", src)
    lib = _abi.load()
    for name, nargs in (("blsq_model_eval_nan_dev", 24), ("blsq_outer_covariance_pinv_nobs", 8)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(_abi.SIGNATURES[name][1]) == nargs and hasattr(lib, name)


# ---- the fit problems of the GPU file ------------------------------------------------------------------------------
def test_fit_problems_keep_more_points_than_parameters():
    """Every problem of every batch the GPU file fits keeps nobs > nf, every pattern occurs, and the lone fits on the
    compressed data recover the truth with scipy (so the reference alone satisfies the condition)."""
    for m in nc.FIT_ROWS:
        pr = nc.fit_problem(m)
        om = nc.fit_omitted(pr)
        k = models.count_observed(nc.blanked(pr["Y"], om))
        assert np.all(k > nc.NF) and k[0] == m and k[4] == m
        assert all(5 <= m - k[b] <= 20 and om[b, -1] and not om[b, 0] for b in (1, 5))
        assert all(m - k[b] == max(1, m // 10) for b in (2, 6)) and all(m - k[b] >= 2 for b in (3, 7))
        M = models.compose(nc.SPEC)
        for b in range(8):
            x, y = pr["x"][~om[b]], pr["Y"][b][~om[b]]
            popt, _ = so.curve_fit(lambda t, *p: M.f(t, np.asarray(p)[None])[0], x, y, p0=pr["P0"][b],
                                   bounds=(pr["bounds"][0][b], pr["bounds"][1][b]), method='trf')
            np.testing.assert_allclose(popt, pr["truth"][b], rtol=0.05, atol=0.02)
    h = nc.histogram_problem()
    k = models.count_observed(nc.blanked(h["Y"], h["omitted"]))
    assert np.all(k > nc.NF) and k[0] == 40 and np.all(k[1:] < 40) and np.all(h["Y"] >= 0)
    assert np.all(models.binned(nc.SPEC).f(h["edges"], h["bounds"][0]) > 0)   # the box keeps the model positive
    r = nc.ragged_scans()
    assert [x.size for x in r["xs"]] == [40, 64, 70] == [y.size for y in r["ys"]]
