"""`curve_fit` / `curve_fit_batch` without a GPU: argument handling and every error path, each with the exception type
and message scipy.optimize.curve_fit gives for the same call; the solve itself is stubbed where a test gets that far."""
import warnings

import numpy as np
import pytest
import scipy.optimize as so
from scipy.optimize import OptimizeResult, OptimizeWarning

X = np.linspace(0.0, 1.0, 6)
Y = 1.0 + 2.0 * X


def line(x, a, b):
    return a + b * x


def _no_gpu(*a, **k):
    raise AssertionError("the GPU was touched")


@pytest.fixture
def nogpu(monkeypatch):
    from bounded_lsq import _abi, _hip_step
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)


def _both_raise(kwargs_ours, kwargs_scipy=None, f=line, x=X, y=Y):
    """The same call on scipy's curve_fit (method='trf') and ours: same exception type, same message."""
    import bounded_lsq
    ks = dict(kwargs_scipy if kwargs_scipy is not None else kwargs_ours)
    ks.setdefault("method", "trf")
    with pytest.raises(Exception) as es:
        so.curve_fit(f, x, y, **ks)
    with pytest.raises(type(es.value)) as eo:
        bounded_lsq.curve_fit(f, x, y, **kwargs_ours)
    assert str(eo.value) == str(es.value), (str(eo.value), str(es.value))
    return es.value


@pytest.mark.parametrize("kw", [
    dict(sigma=np.ones(5)),                                     # wrong 1-D length
    dict(sigma=np.ones((6, 5))),                                # wrong 2-D shape
    dict(sigma=np.ones((2, 3, 1))),
    dict(sigma=-np.eye(6)),                                     # not positive definite
    dict(sigma=np.ones((6, 6))),                                # singular
    dict(p0=[1.0, 1.0], args=(1,)),                             # 'args' is not supported
    dict(p0=[1.0, 1.0], bounds=([0, 0], [1, 1], [2, 2])),       # bounds of three elements
], ids=["sigma-1d", "sigma-2d", "sigma-3d", "sigma-negative", "sigma-singular", "args", "bounds"])
def test_error_paths_are_scipys(nogpu, kw):
    e = _both_raise(kw)
    assert isinstance(e, ValueError)


def test_more_error_paths_are_scipys(nogpu):
    assert isinstance(_both_raise({}, f=lambda *a: a[1] + a[2] * a[0]), ValueError)      # no signature to inspect
    assert isinstance(_both_raise({}, f=lambda x: x), ValueError)                         # no parameter at all
    assert isinstance(_both_raise(dict(p0=[1.0, 1.0]), y=np.array([])), ValueError)       # empty ydata
    Ynan = Y.copy()
    Ynan[2] = np.nan
    assert isinstance(_both_raise(dict(p0=[1.0, 1.0]), y=Ynan), ValueError)               # check_finite
    Xinf = X.copy()
    Xinf[0] = np.inf
    assert isinstance(_both_raise(dict(p0=[1.0, 1.0]), x=Xinf), ValueError)
    assert isinstance(_both_raise(dict(p0=[2.0, 1.0], bounds=([0, 0], [1, 3]))), ValueError)   # infeasible p0
    assert isinstance(_both_raise(dict(p0=[0.5, 1.0], bounds=([1, 0], [0, 3]))), ValueError)   # lb >= ub


def test_method_lm_is_not_implemented(nogpu):
    import bounded_lsq
    with pytest.raises(NotImplementedError, match="method='lm'"):
        bounded_lsq.curve_fit(line, X, Y, p0=[1.0, 1.0], method='lm')
    with pytest.raises(NotImplementedError, match="method='lm'"):
        bounded_lsq.least_squares(lambda p: p, [1.0], method='lm')


class _Solve:
    """A stand-in for least_squares that records its call and returns a fixed result (no GPU)."""

    def __init__(self, m, n, success=True, cov=None, obj=3.0):
        self.m, self.n, self.success, self.obj = m, n, success, obj
        self.cov = np.eye(n) if cov is None else cov
        self.calls = []

    def __call__(self, fun, x0, **kw):
        self.calls.append(dict(kw, x0=np.array(x0, dtype=float), fun=fun))
        f0 = fun(np.asarray(x0, dtype=float))
        r = OptimizeResult(x=np.array(x0, dtype=float), fun=np.asarray(f0), jac=np.ones((self.m, self.n)),
                           obj_value=self.obj, nfev=7, njev=3, status=2 if self.success else 0,
                           x_covariance=None if self.cov is None else self.cov.copy(), x_covariance_rank=self.n)
        r.success = self.success
        r.message = "`ftol` termination condition is satisfied." if self.success else \
            "The maximum number of function evaluations is exceeded."
        return r


@pytest.fixture
def solve(monkeypatch, nogpu):
    from bounded_lsq import _curve_fit

    def install(*a, **k):
        s = _Solve(*a, **k)
        monkeypatch.setattr(_curve_fit, "least_squares", s)
        return s
    return install


def test_p0_none_inspects_the_signature_and_starts_feasible(solve):
    import bounded_lsq

    def model(x, a, b, c):
        return a + b * x + c * x * x

    s = solve(6, 3)
    popt, pcov = bounded_lsq.curve_fit(model, X, Y)
    assert np.array_equal(s.calls[0]["x0"], np.ones(3)) and popt.shape == (3,) and pcov.shape == (3, 3)
    bounded_lsq.curve_fit(model, X, Y, bounds=([0.0, -np.inf, -np.inf], [4.0, 5.0, np.inf]))
    assert np.array_equal(s.calls[1]["x0"], [2.0, 4.0, 1.0])      # middle, ub - 1, 1: scipy's _initialize_feasible
    bounded_lsq.curve_fit(model, X, Y, bounds=so.Bounds([3.0, -1.0, -1.0], [np.inf, 1.0, 1.0]))
    assert np.array_equal(s.calls[2]["x0"], [4.0, 0.0, 0.0])
    c = s.calls[0]
    assert c["jac"] == '2-point' and c["method"] == 'trf' and c["covariance"] == 'pinv' and c["max_nfev"] is None


def test_maxfev_is_renamed_and_keywords_pass_through(solve):
    import bounded_lsq
    s = solve(6, 2)
    bounded_lsq.curve_fit(line, X, Y, p0=[1, 1], maxfev=55, loss='huber', f_scale=0.3, ftol=1e-11, method='dogbox')
    c = s.calls[0]
    assert c["max_nfev"] == 55 and "maxfev" not in c
    assert (c["loss"], c["f_scale"], c["ftol"], c["method"]) == ('huber', 0.3, 1e-11, 'dogbox')
    bounded_lsq.curve_fit(line, X, Y, p0=[1, 1], max_nfev=9)
    assert s.calls[1]["max_nfev"] == 9


def test_sigma_forms_give_scipys_residuals_and_jacobians(solve):
    import bounded_lsq
    from scipy.optimize import _minpack_py as mp
    rng = np.random.default_rng(0)
    p = np.array([0.3, -1.2])
    L = np.tril(rng.standard_normal((6, 6))) + 4 * np.eye(6)
    cov2d = L @ L.T

    def dline(x, a, b):
        return np.stack([np.ones_like(x), x], axis=1)

    for sigma in (None, 2.5, np.array([2.5]), rng.uniform(0.5, 2.0, 6), cov2d):
        s = solve(6, 2)
        bounded_lsq.curve_fit(line, X, Y, p0=p, sigma=sigma, jac=dline)
        c = s.calls[0]
        if sigma is None:
            tr = None
        else:
            sg = np.asarray(sigma)
            tr = 1.0 / sg if sg.ndim < 2 else np.linalg.cholesky(sg)
        want_f = mp._wrap_func(line, X, Y, tr)(p)
        want_J = tr * dline(X, *p) if np.ndim(sigma) == 0 and sigma is not None else mp._wrap_jac(dline, X, tr)(p)
        assert np.array_equal(c["fun"](p), want_f)
        assert np.array_equal(np.asarray(c["jac"](p)), want_J)


def test_pcov_scaling_inf_fill_and_warning(solve):
    import bounded_lsq
    cov = np.array([[2.0, 0.5], [0.5, 1.0]])
    s = solve(6, 2, cov=cov, obj=3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        popt, pcov = bounded_lsq.curve_fit(line, X, Y, p0=[1, 1])
        assert np.array_equal(pcov, cov * (3.0 / 4.0))             # obj / (m - n)
        popt, pcov = bounded_lsq.curve_fit(line, X, Y, p0=[1, 1], absolute_sigma=True)
        assert np.array_equal(pcov, cov)
    # m <= n: inf and the warning, as scipy (method='trf') on the same data
    x2, y2 = X[:2], Y[:2]
    s = solve(2, 2, cov=cov)
    with pytest.warns(OptimizeWarning, match="Covariance of the parameters could not be estimated") as w:
        popt, pcov = bounded_lsq.curve_fit(line, x2, y2, p0=[1, 1])
    assert np.all(np.isinf(pcov)) and pcov.shape == (2, 2)
    with pytest.warns(OptimizeWarning) as ws:
        _, pcov_s = so.curve_fit(line, x2, y2, p0=[1, 1], method='trf')
    assert np.all(np.isinf(pcov_s)) and str(ws[0].message) == str(w[0].message)
    with warnings.catch_warnings():                                # absolute_sigma: no scaling, no warning
        warnings.simplefilter("error")
        _, pcov = bounded_lsq.curve_fit(line, x2, y2, p0=[1, 1], absolute_sigma=True)
        assert np.array_equal(pcov, cov)
    # no covariance at all (J not finite)
    s = solve(6, 2)
    s.cov = None
    with pytest.warns(OptimizeWarning):
        _, pcov = bounded_lsq.curve_fit(line, X, Y, p0=[1, 1], absolute_sigma=True)
    assert np.all(np.isinf(pcov))


def test_unsuccessful_solve_raises_and_full_output(solve):
    import bounded_lsq
    solve(6, 2, success=False)
    with pytest.raises(RuntimeError) as e:
        bounded_lsq.curve_fit(line, X, Y, p0=[1, 1])
    with pytest.raises(RuntimeError) as es:
        so.curve_fit(lambda x, a, b: a * np.exp(b * x), X, Y, p0=[1, 1], method='trf', maxfev=1)
    assert str(e.value) == str(es.value) == \
        "Optimal parameters not found: The maximum number of function evaluations is exceeded."
    solve(6, 2)
    out = bounded_lsq.curve_fit(line, X, Y, p0=[1.5, 0.5], full_output=True)
    assert len(out) == 5
    popt, pcov, info, mesg, ier = out
    ref = so.curve_fit(line, X, Y, p0=[1.5, 0.5], full_output=True, method='trf')
    assert sorted(info) == sorted(ref[2]) == ["fvec", "nfev"]
    assert np.array_equal(info["fvec"], line(X, 1.5, 0.5) - Y) and info["nfev"] == 7
    assert ier == 2 and mesg == "`ftol` termination condition is satisfied."


# ---- curve_fit_batch -----------------------------------------------------------------------------
class _BatchSolve:
    def __init__(self, fail=()):
        self.calls, self.fail = [], fail

    def __call__(self, fun, X0, jac, **kw):
        self.calls.append(dict(kw, fun=fun, jac=jac, X0=X0))
        B, n = X0.shape
        F = fun(X0)
        out = []
        for b in range(B):
            r = OptimizeResult(x=X0[b] + b, fun=F[b], jac=np.ones((F.shape[1], n)), obj_value=2.0,
                               x_covariance=np.eye(n) * (b + 1), status=0 if b in self.fail else 1)
            r.success = r.status > 0
            out.append(r)
        return out


def test_curve_fit_batch_arguments(monkeypatch, nogpu):
    import bounded_lsq
    from bounded_lsq import _curve_fit
    s = _BatchSolve(fail=(1,))
    monkeypatch.setattr(_curve_fit, "least_squares_batch", s)
    B, m, n = 3, 6, 2
    Yb = np.stack([Y, 2 * Y, 3 * Y])
    P0 = np.ones((B, n))

    def fb(x, P):
        return P[:, 0:1] + P[:, 1:2] * x

    def jb(x, P):
        return np.broadcast_to(np.stack([np.ones_like(x), x], axis=1), (P.shape[0], x.size, 2))

    sig = np.random.default_rng(1).uniform(0.5, 2.0, (B, m))
    popt, pcov, res = bounded_lsq.curve_fit_batch(fb, X, Yb, P0, sigma=sig, jac=jb, maxfev=30, driver='device')
    c = s.calls[0]
    assert c["covariance"] == 'pinv' and c["_variance_scale"] is True and c["driver"] == 'device'
    assert c["max_nfev"] == 30 and c["method"] == 'trf'
    assert np.array_equal(c["fun"](P0), (1.0 / sig) * (fb(X, P0) - Yb))
    assert np.array_equal(c["jac"](P0), (1.0 / sig)[:, :, None] * jb(X, P0))
    assert popt.shape == (B, n) and pcov.shape == (B, n, n) and len(res) == B
    assert np.all(np.isnan(popt[1])) and np.all(np.isnan(pcov[1]))           # not converged: NaN rows, no exception
    assert np.array_equal(popt[2], P0[2] + 2) and np.array_equal(pcov[2], 3 * np.eye(n))
    for sigma in (2.0, sig[0]):
        bounded_lsq.curve_fit_batch(fb, X, Yb, P0, sigma=sigma, absolute_sigma=True)
        c = s.calls[-1]
        assert c["_variance_scale"] is False and c["jac"] == '2-point'
        assert np.array_equal(c["fun"](P0), (1.0 / sigma) * (fb(X, P0) - Yb))
    with pytest.raises(ValueError, match="2-D covariance"):
        bounded_lsq.curve_fit_batch(fb, X, Yb, P0, sigma=np.eye(m))
    with pytest.raises(ValueError, match="incorrect shape"):
        bounded_lsq.curve_fit_batch(fb, X, Yb, P0, sigma=np.ones(5))
    with pytest.raises(ValueError, match="'args' is not a supported keyword argument."):
        bounded_lsq.curve_fit_batch(fb, X, Yb, P0, args=(1,))
    with pytest.raises(ValueError, match=r"`ydata` must have shape \(B, m\)"):
        bounded_lsq.curve_fit_batch(fb, X, Y, P0)
    with pytest.raises(ValueError, match=r"`p0` must have shape \(B, n\)"):
        bounded_lsq.curve_fit_batch(fb, X, Yb, np.ones(n))
    # m <= n without absolute_sigma: inf and the warning
    with pytest.warns(OptimizeWarning, match="Covariance of the parameters could not be estimated"):
        popt, pcov, _ = bounded_lsq.curve_fit_batch(fb, X[:2], Yb[:, :2], P0)
    assert np.all(np.isinf(pcov[0])) and np.all(np.isnan(pcov[1])) and s.calls[-1]["_variance_scale"] is False
    assert "curve_fit" in bounded_lsq.__all__ and "curve_fit_batch" in bounded_lsq.__all__
