"""Global fits without a GPU: ``GlobalMap`` against its definition, ``curve_fit_global`` with the solve
stubbed, and the vetting of the fit cases of tests/_global_cases.py against scipy."""
import os
import re
import warnings

import numpy as np
import pytest
from scipy.optimize import OptimizeResult, OptimizeWarning

import bounded_lsq
from bounded_lsq import GlobalMap, ParamMap, models

import _global_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- GlobalMap -------------------------------------------------------------------------------------------------------
def test_layout_and_column():
    gm = GlobalMap(4, 3, [1, 2])
    assert (gm.n, gm.S, gm.nf, gm.ns, gm.nl, gm.nv) == (4, 3, 4, 2, 2, 8)
    assert gm.slot_shared.tolist() == [False, True, True, False]
    # shared slots first, ascending; then the local slots of data set 0, 1, 2, ascending
    assert [[gm.column(k, s) for k in range(4)] for s in range(3)] == [[2, 0, 1, 3], [4, 0, 1, 5], [6, 0, 1, 7]]
    assert np.array_equal(gm.cols, [[2, 0, 1, 3], [4, 0, 1, 5], [6, 0, 1, 7]])
    # a boolean mask, a fixed and a tied parameter: slots are those of ParamMap(6, [0], {4: 2}) = leaders 1, 2, 3, 5
    gm = GlobalMap(6, 2, np.array([0, 0, 1, 0, 1, 1], dtype=bool), fixed=[0], tied={4: 2})
    assert gm.pm.leaders.tolist() == [1, 2, 3, 5] and gm.slot_shared.tolist() == [False, True, False, True]
    assert (gm.ns, gm.nl, gm.nv) == (2, 2, 6)
    assert gm.cols.tolist() == [[2, 0, 3, 1], [4, 0, 5, 1]]
    # a tied key is shared through its leader, named or not
    assert GlobalMap(6, 2, [2, 5], fixed=[0], tied={4: 2}).cols.tolist() == gm.cols.tolist()
    allsh = GlobalMap(3, 4, [0, 1, 2])
    assert (allsh.nl, allsh.nv) == (0, 3) and allsh.cols.tolist() == [[0, 1, 2]] * 4
    with pytest.raises(ValueError):
        gm.column(4, 0)
    with pytest.raises(ValueError):
        gm.column(0, 2)


def test_value_errors_name_the_index():
    with pytest.raises(ValueError, match=r"`shared` index 1 is fixed"):
        GlobalMap(4, 2, [1, 2], fixed=[1])
    with pytest.raises(ValueError, match=r"`shared` index 3 is tied to parameter 0, which is not shared"):
        GlobalMap(4, 2, [3], tied={3: 0})
    with pytest.raises(ValueError, match=r"`shared` index 4 is outside 0 \.\. 3"):
        GlobalMap(4, 2, [4])
    with pytest.raises(ValueError, match=r"`shared` index -1 is outside"):
        GlobalMap(4, 2, [-1])
    for empty in ([], np.zeros(4, dtype=bool)):
        with pytest.raises(ValueError, match=r"nothing is shared.*curve_fit_batch"):
            GlobalMap(4, 2, empty)
    with pytest.raises(ValueError, match=r"boolean `shared` must have shape"):
        GlobalMap(4, 2, np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="`S` must be a positive integer"):
        GlobalMap(4, 0, [1])
    with pytest.raises(ValueError, match="`fixed` index 9"):                   # the ParamMap's own checks still speak
        GlobalMap(4, 2, [1], fixed=[9])


@pytest.mark.parametrize("fixed, tied", [(None, None), ([0], {4: 2}), ([1, 5], {3: 0})])
def test_one_data_set_is_the_param_map(fixed, tied):
    """S = 1 with every slot shared: every method array_equal to ParamMap's."""
    n, G, m = 6, 3, 5
    rng = np.random.default_rng(0)
    pm = ParamMap(n, fixed, tied)
    gm = GlobalMap(n, 1, pm.leaders, fixed, tied)
    assert gm.nv == pm.nf and gm.cols.tolist() == [list(range(pm.nf))]
    P = rng.standard_normal((G, n))
    X = rng.standard_normal((G, pm.nf))
    J = rng.standard_normal((G, m, n))
    C = rng.standard_normal((G, pm.nf, pm.nf))
    lb, ub = -rng.uniform(0.1, 1.0, P.shape), rng.uniform(0.1, 1.0, P.shape)      # (every box holds 0: they intersect)
    mask = rng.integers(-1, 2, (G, pm.nf))
    assert np.array_equal(gm.reduce_x(P[:, None]), pm.reduce_x(P))
    assert np.array_equal(gm.expand_x(X, P[:, None])[:, 0], pm.expand_x(X, P))
    assert np.array_equal(gm.reduce_jac(J[:, None]), pm.reduce_jac(J))
    for a, b in zip(gm.reduce_bounds(lb[:, None], ub[:, None]), pm.reduce_bounds(lb, ub)):
        assert np.array_equal(a, b)
    assert np.array_equal(gm.expand_cov(C)[:, 0], pm.expand_cov(C))
    assert np.array_equal(gm.expand_mask(mask)[:, 0], pm.expand_mask(mask))
    assert np.array_equal(gm.matrix(), pm.matrix())

    def f(x, Pq):
        return np.sin(Pq @ np.arange(1.0, n + 1))[:, None] * x

    def jac(x, Pq):
        return (np.cos(Pq @ np.arange(1.0, n + 1))[:, None, None] * x[None, :, None]) * np.arange(1.0, n + 1)
    x = np.linspace(0.0, 1.0, m)
    assert np.array_equal(gm.wrap_f(f, P[:, None])(x, X), pm.wrap_f(f, P)(x, X))
    assert np.array_equal(gm.wrap_jac(jac, P[:, None])(x, X), pm.wrap_jac(jac, P)(x, X))


MAPS = [dict(n=4, S=3, shared=[1, 2]), dict(n=6, S=2, shared=[2, 5], fixed=[0], tied={4: 2}),
        dict(n=7, S=4, shared=[1, 2, 4, 5], fixed=[6], tied={5: 2}), dict(n=3, S=5, shared=[0, 1, 2])]


def _dense(gm, J_full):
    """reduce_jac by explicit loops: (G, S, m, n) -> (G, S m, nv)."""
    G, S, m, n = J_full.shape
    out = np.zeros((G, S * m, gm.nv))
    for g in range(G):
        for s in range(S):
            for i in range(m):
                started = set()
                for j in range(n):
                    k = gm.pm.pmap[j]
                    if k < 0:
                        continue
                    c = gm.column(k, s)
                    out[g, s * m + i, c] = out[g, s * m + i, c] + J_full[g, s, i, j] if c in started else J_full[g, s, i, j]
                    started.add(c)
    return out


@pytest.mark.parametrize("kw", MAPS)
def test_methods_against_explicit_loops(kw):
    gm = GlobalMap(**kw)
    n, S, G, m = gm.n, gm.S, 2, 3
    rng = np.random.default_rng(1)
    P = rng.standard_normal((G, S, n))
    # reduce_x: a shared variable starts from data set 0; expand_x puts it back into every data set
    X = gm.reduce_x(P)
    assert X.shape == (G, gm.nv)
    for s in range(S):
        for k in range(gm.nf):
            src = 0 if gm.slot_shared[k] else s
            assert np.array_equal(X[:, gm.column(k, s)], P[:, src, gm.pm.leaders[k]])
    Pe = gm.expand_x(X, P)
    assert Pe.shape == (G, S, n)
    for j in range(n):
        k = gm.pm.pmap[j]
        for s in range(S):
            assert np.array_equal(Pe[:, s, j], P[:, s, j] if k < 0 else X[:, gm.column(k, s)])
    assert np.array_equal(gm.reduce_x(Pe), X)
    # reduce_jac: the dense matrix, and +0.0 in the bits of every column outside a data set's own
    J = rng.standard_normal((G, S, m, n))
    Jr = gm.reduce_jac(J)
    assert Jr.shape == (G, S * m, gm.nv) and np.array_equal(Jr, _dense(gm, J))
    for s in range(S):
        other = np.setdiff1d(np.arange(gm.nv), gm.cols[s])
        assert not Jr[:, s * m:(s + 1) * m][:, :, other].view(np.int64).any()
    # expand_cov: the diagonal blocks of T C T^T
    C = rng.standard_normal((G, gm.nv, gm.nv))
    T = gm.matrix()
    assert T.shape == (S * n, gm.nv)
    full = T @ C @ T.T
    E = gm.expand_cov(C)
    assert E.shape == (G, S, n, n)
    for s in range(S):
        assert np.array_equal(E[:, s], full[:, s * n:(s + 1) * n, s * n:(s + 1) * n])
    # expand_mask
    mask = rng.integers(-1, 2, (G, gm.nv))
    Em = gm.expand_mask(mask)
    for j in range(n):
        k = gm.pm.pmap[j]
        for s in range(S):
            assert np.array_equal(Em[:, s, j], np.zeros(G, dtype=mask.dtype) if k < 0 else mask[:, gm.column(k, s)])


def test_reduce_bounds_intersects_over_data_sets_and_members():
    gm = GlobalMap(4, 3, [1, 3], tied={3: 1})              # slots: 0 (local), 1 = {1, 3} (shared), 2 (local)
    lb = np.full((2, 3, 4), -10.0)
    ub = np.full((2, 3, 4), 10.0)
    lb[0, 2, 1], ub[0, 1, 3], lb[1, 0, 3] = -1.0, 2.0, -3.0
    lb[0, 1, 0], ub[1, 2, 2] = -5.0, 7.0
    lo, hi = gm.reduce_bounds(lb, ub)
    assert lo.shape == hi.shape == (2, gm.nv) and gm.nv == 1 + 3 * 2
    assert lo[:, 0].tolist() == [-1.0, -3.0] and hi[:, 0].tolist() == [2.0, 10.0]
    assert lo[0, gm.column(0, 1)] == -5.0 and hi[1, gm.column(2, 2)] == 7.0
    ub[1, 1, 1] = -4.0                                      # below lb[1, 0, 3] = -3: an empty box across data sets
    with pytest.raises(ValueError, match=r"shared parameters \[1, 3\] do not intersect"):
        gm.reduce_bounds(lb, ub)


@pytest.mark.parametrize("kw", MAPS[:3])
def test_wrap_jac_against_central_differences_of_wrap_f(kw):
    gm = GlobalMap(**kw)
    n, S, G, m = gm.n, gm.S, 2, 4
    rng = np.random.default_rng(2)
    A = rng.standard_normal((n, m))

    def f(x, Pq):                                           # (G S, n) -> (G S, m)
        return np.sin(Pq @ A) * x

    def jac(x, Pq):
        return (np.cos(Pq @ A) * x)[:, :, None] * A.T[None]
    x = np.linspace(0.5, 1.5, m)
    Pfix = rng.standard_normal((G, S, n))
    X = rng.standard_normal((G, gm.nv))
    wf, wj = gm.wrap_f(f, Pfix), gm.wrap_jac(jac, Pfix)
    J = wj(x, X)
    assert wf(x, X).shape == (G, S * m) and J.shape == (G, S * m, gm.nv)
    h = 1e-6
    for v in range(gm.nv):
        E = np.zeros(gm.nv)
        E[v] = h
        np.testing.assert_allclose(J[:, :, v], (wf(x, X + E) - wf(x, X - E)) / (2 * h), rtol=0, atol=1e-8)


# ---- curve_fit_global with the solve stubbed ---------------------------------------------------------------------------
def _no_gpu(*a, **k):
    raise AssertionError("this test must not reach the GPU")


@pytest.fixture
def nogpu(monkeypatch):
    from bounded_lsq import _abi, _hip_step
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)


class _Solve:
    def __init__(self, fail=()):
        self.calls, self.fail = [], fail

    def __call__(self, fun, X0, jac, **kw):
        self.calls.append(dict(kw, fun=fun, jac=jac, X0=X0))
        B, n = X0.shape
        Mrows = fun.m if hasattr(fun, "open_device") else fun(X0).shape[1]
        out = []
        for b in range(B):
            r = OptimizeResult(x=X0[b] + b, fun=np.full(Mrows, 2.0), jac=np.ones((Mrows, n)), obj_value=2.0,
                               x_covariance=np.arange(1.0, n * n + 1).reshape(n, n) * (b + 1),
                               status=0 if b in self.fail else 1)
            r.success = r.status > 0
            out.append(r)
        return out


@pytest.fixture
def solve(monkeypatch, nogpu):
    from bounded_lsq import _curve_fit
    s = _Solve(fail=(1,))
    monkeypatch.setattr(_curve_fit, "least_squares_batch", s)
    return s


def _problem(G=3, S=2, m=6, n=4):
    rng = np.random.default_rng(3)
    x = np.linspace(-2.0, 2.0, m)
    P0 = np.empty((G, S, n))
    P0[..., 0], P0[..., 1], P0[..., 2], P0[..., 3] = 3.0, rng.uniform(-0.3, 0.3, (G, S)), 1.0, 0.5
    Y = rng.uniform(1.0, 4.0, (G, S, m))
    return x, Y, P0


def test_front_end_shapes_bounds_and_results(solve):
    G, S, m, n = 3, 2, 6, 4
    x, Y, P0 = _problem(G, S, m, n)
    gm = GlobalMap(n, S, [1, 2])
    lb = np.full((G, S, n), -np.inf)
    ub = np.full((G, S, n), np.inf)
    lb[..., 2] = 0.1
    lb[0, 1, 1], ub[0, 0, 1] = -0.9, 0.8                     # the shared mu of group 0: intersected over its data sets
    sig = np.random.default_rng(4).uniform(0.5, 2.0, (S, m))
    popt, pcov, res = bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], sigma=sig, bounds=(lb, ub), maxfev=30)
    c = solve.calls[0]
    assert c["covariance"] == "pinv" and c["_variance_scale"] is True and c["driver"] == "host"
    assert c["max_nfev"] == 30 and c["method"] == "trf" and "_nobs" not in c
    X0 = gm.reduce_x(P0)
    assert np.array_equal(c["X0"], X0) and c["X0"].shape == (G, gm.nv)
    lo, hi = c["bounds"]
    assert lo.shape == hi.shape == (G, gm.nv)
    assert lo[0, gm.column(1, 0)] == -0.9 and hi[0, gm.column(1, 0)] == 0.8 and np.all(lo[:, gm.column(2, 0)] == 0.1)
    F = models.get("gauss_sum").f(x, gm.expand_x(X0, P0).reshape(-1, n)).reshape(G, S * m)
    assert np.array_equal(c["fun"](X0), (1.0 / sig).reshape(-1) * (F - Y.reshape(G, S * m)))
    Jd = gm.reduce_jac(models.get("gauss_sum").jac(x, gm.expand_x(X0, P0).reshape(-1, n)).reshape(G, S, m, n))
    assert np.array_equal(c["jac"](X0), (1.0 / sig).reshape(-1)[None, :, None] * Jd)
    assert popt.shape == (G, S, n) and pcov.shape == (G, S, n, n) and len(res) == G
    assert np.all(np.isnan(popt[1])) and np.all(np.isnan(pcov[1]))               # not converged: NaN rows
    assert np.array_equal(popt[2], gm.expand_x(X0[2] + 2, P0[2]))
    assert np.array_equal(popt[2][0, 1:3], popt[2][1, 1:3])                       # shared: equal in all S rows
    assert np.array_equal(pcov[2], gm.expand_cov(res[2].x_covariance))
    r = res[2]
    assert r.x.shape == (gm.nv,) and r.x_covariance.shape == (gm.nv, gm.nv) and r.popt.shape == (S, n)
    assert r.global_map.nv == gm.nv and r.fun.shape == (S * m,) and r.jac.shape == (S * m, gm.nv)
    # one group: (S, m) in, (S, n) out
    popt1, pcov1, res1 = bounded_lsq.curve_fit_global("gauss_sum", x, Y[0], P0[0], [1, 2], absolute_sigma=True)
    assert popt1.shape == (S, n) and pcov1.shape == (S, n, n) and len(res1) == 1
    assert solve.calls[-1]["_variance_scale"] is False
    # a callable over (G S, n), per-data-set abscissae: it gets one row per data set
    seen = {}

    def fb(t, P):
        seen["t"], seen["P"] = t.shape, P.shape
        return P[:, 0:1] + P[:, 1:2] * t
    xs = np.stack([x, x + 1.0])
    bounded_lsq.curve_fit_global(fb, xs, Y, P0, [1], driver="device")
    c = solve.calls[-1]
    assert c["jac"] == "2-point" and c["driver"] == "device"
    assert c["fun"](c["X0"]).shape == (G, S * m) and seen == {"t": (G * S, m), "P": (G * S, n)}
    assert "curve_fit_global" in bounded_lsq.__all__ and "GlobalMap" in bounded_lsq.__all__


def test_front_end_device_route_builds_a_device_fit(solve):
    G, S, m, n = 3, 2, 6, 4
    x, Y, P0 = _problem(G, S, m, n)
    bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], driver="device", fixed=[3])
    fit = solve.calls[-1]["fun"]
    gm = fit.global_map
    assert isinstance(fit, models.DeviceFit) and solve.calls[-1]["jac"] is None
    assert (fit.B, fit.m, fit.n, fit.n_model) == (G, S * m, gm.nv, n) and gm.nv == 2 + S * 1
    assert fit.Pfix.shape == (G, S, n) and fit.ydata.shape == (G, S, m)


def test_front_end_omit_sums_the_kept_points_per_group(solve):
    G, S, m, n = 3, 2, 6, 4
    x, Y, P0 = _problem(G, S, m, n)
    Y = Y.copy()
    Y[0, 0, :2] = Y[0, 1, 5] = Y[2, 1, 3] = np.nan
    sig = np.ones((G, S, m))
    sig[0, 0, 0] = np.nan                                    # anything may stand at an omitted point
    popt, pcov, res = bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], sigma=sig, nan_policy="omit")
    c = solve.calls[-1]
    assert c["_nobs"].tolist() == [S * m - 3, S * m, S * m - 1] and c["_nobs"].dtype == np.int32
    F = c["fun"](c["X0"])
    assert not F[np.isnan(Y.reshape(G, -1))].view(np.int64).any() and np.all(np.isfinite(F))
    assert res[0].nobs == S * m - 3 and res[0].omitted.shape == (S, m) and res[0].omitted.sum() == 3
    # the variance-scale flag and the degrees of freedom: M - nv, and nobs_g - nv under omit
    gm = res[0].global_map
    assert c["_variance_scale"] is True
    Yfew = np.full((G, S, m), np.nan)
    Yfew[:, :, 0] = 1.0
    Yfew[1:, :, :] = Y[1:]                                   # group 0 keeps S points <= nv = 6
    with pytest.warns(OptimizeWarning, match="Covariance of the parameters could not be estimated"):
        popt, pcov, res = bounded_lsq.curve_fit_global("gauss_sum", x, Yfew, P0, [1, 2], nan_policy="omit")
    assert res[0].nobs == S <= gm.nv and np.all(np.isinf(pcov[0])) and np.all(np.isfinite(pcov[2]))
    with pytest.warns(OptimizeWarning):                      # M = 2 * 2 <= nv = 6: no flag, inf
        popt, pcov, _ = bounded_lsq.curve_fit_global("gauss_sum", x[:2], Y[:, :, 4:6], P0, [1, 2])
    assert solve.calls[-1]["_variance_scale"] is False and np.all(np.isinf(pcov[0]))
    Ybad = Y.copy()
    Ybad[2, 1, :] = np.nan
    with pytest.raises(ValueError, match=r"data set 1 of group 2 has no point left"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Ybad, P0, [1, 2], nan_policy="omit")
    with pytest.raises(ValueError, match="The input contains nan values"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], nan_policy="raise")


def test_front_end_poisson_wraps_after_the_map(solve):
    G, S, m, n = 3, 2, 6, 4
    x, Y, P0 = _problem(G, S, m, n)
    Yc = np.floor(Y)
    popt, pcov, res = bounded_lsq.curve_fit_global("gauss_sum", x, Yc, P0, [1, 2], estimator="poisson")
    c = solve.calls[-1]
    gm = res[0].global_map
    X0 = c["X0"]
    P = gm.expand_x(X0, P0).reshape(-1, n)
    mu = models.get("gauss_sum").f(x, P).reshape(G, S * m)
    r, cc = models.poisson_transform(mu, Yc.reshape(G, S * m))
    assert np.array_equal(c["fun"](X0), r)
    Jd = gm.reduce_jac(models.get("gauss_sum").jac(x, P).reshape(G, S, m, n))
    assert np.array_equal(c["jac"](X0), cc[:, :, None] * Jd)
    assert res[0].deviance == float(np.dot(res[0].fun, res[0].fun))
    with pytest.raises(ValueError, match="`sigma` must be None"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Yc, P0, [1, 2], estimator="poisson", sigma=1.0)


def test_front_end_rejections(solve):
    G, S, m, n = 3, 2, 6, 4
    x, Y, P0 = _problem(G, S, m, n)
    with pytest.raises(ValueError, match="`binned=True` is not supported"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], binned=True)
    with pytest.raises(ValueError, match="gauss2d.*one coordinate"):
        bounded_lsq.curve_fit_global("gauss2d", np.zeros((2, m)), Y, np.ones((G, S, 5)), [1, 2])
    # nv > 256: 'gauss*2+poly*1' with one shared parameter and S = 43 has 1 + 43 * 6 = 259 variables
    Sb = 43
    with pytest.raises(ValueError, match=r"nv = ns \+ S nl = 1 \+ 43 \* 6 = 259 variables, more than 256"):
        bounded_lsq.curve_fit_global("gauss*2+poly*1", x, np.ones((1, Sb, m)), np.ones((1, Sb, 7)), [1])
    with pytest.raises(ValueError, match="nothing is shared.*curve_fit_batch"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [])
    with pytest.raises(ValueError, match=r"`ydata` must have shape \(S, m\) or \(G, S, m\)"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y[0, 0], P0, [1, 2])
    with pytest.raises(ValueError, match=r"`p0` must have shape"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0[:, 0], [1, 2])
    with pytest.raises(ValueError, match=r"`xdata` of a global fit must have shape"):
        bounded_lsq.curve_fit_global("gauss_sum", np.zeros((G, m)), Y, P0, [1, 2])
    with pytest.raises(ValueError, match="incorrect shape"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], sigma=np.ones(m + 1))
    with pytest.raises(ValueError, match="callable `jac` cannot be combined"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], jac=lambda t, P: None)
    lb = np.full((G, S, n), -np.inf)
    ub = np.full((G, S, n), np.inf)
    lb[1, 0, 1], ub[1, 1, 1] = 0.5, 0.4
    with pytest.raises(ValueError, match="do not intersect over the data sets"):
        bounded_lsq.curve_fit_global("gauss_sum", x, Y, P0, [1, 2], bounds=(lb, ub))
    assert not solve.calls


def test_device_model_rejects_what_a_global_fit_does_not_take(nogpu):
    gm = GlobalMap(4, 2, [1, 2])
    x, Y, P0 = _problem(3, 2, 6, 4)
    with pytest.raises(ValueError, match="`binned=True` is not supported in a global fit"):
        models.DeviceFit("gauss_sum", 4, x, Y, global_map=gm, binned=True)
    with pytest.raises(ValueError, match="one coordinate"):
        models.DeviceFit("gauss2d", 5, x, Y, global_map=GlobalMap(5, 2, [1]))
    with pytest.raises(ValueError, match="`param_map` must be None"):
        models.DeviceFit("gauss_sum", 4, x, Y, global_map=gm, param_map=ParamMap(4, [0]))
    with pytest.raises(ValueError, match=r"`ydata` must have shape \(G, S, m\)"):
        models.DeviceFit("gauss_sum", 4, x, Y[:, 0], global_map=gm)


# ---- the interface ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_its_limit():
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    assert re.search(r"#define\s+BLSQ_GLOBAL_MAX_NV\s+256\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+blsq_model_eval_global_dev\s*\(([^)]*)\)", code)
    assert decl and len(decl.group(1).split(",")) == 27
    from bounded_lsq import _abi, _curve_fit
    assert len(_abi.SIGNATURES["blsq_model_eval_global_dev"][1]) == 27
    assert _curve_fit.GLOBAL_MAX_NV == 256


# ---- vetting of the fit cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FIT_CASES)
def test_reference_converges_from_the_start_of_every_group(name):
    """The independent reference of tests/test_global_gpu.py: scipy on the hand-written concatenated residual converges
    (status > 0) from the case's p0 for every group, inside the bounds, with a finite covariance."""
    case = gc.fit_case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        popt, pcov, results, nv = gc.reference(name)
    assert len(results) == case["G"] and all(r.status > 0 for r in results), [r.status for r in results]
    assert np.all(np.isfinite(popt)) and np.all(np.isfinite(pcov))
    lb, ub = case["bounds"]
    assert np.all(popt > lb) and np.all(popt < ub)           # an interior optimum: no bound is active
    assert nv == GlobalMap(case["n"], case["S"], case["shared"], case["fixed"], case["tied"]).nv
    for j in case["shared"]:                                  # a shared parameter has one value in its group
        assert np.all(popt[:, :, j] == popt[:, :1, j])
    free = [j for j in range(case["n"]) if j not in (case["fixed"] or ())]
    assert np.all(np.einsum("gsii->gsi", pcov)[:, :, free] > 0)
