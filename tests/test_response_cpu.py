"""Instrument response without a GPU: ``models.apply_response`` against np.convolve and against the double
loop of its definition, the wrappers against central differences, every ValueError, the routing of the keywords (the
solve replaced by a spy, the device by a recorder), the C-ABI of the new entry, and the end-to-end cases of
tests/_response_cases.py vetted with scipy alone: each converges strictly inside its box within 6 standard errors of the
truth, and the same data fitted WITHOUT the response misses the truth by more than that, so the GPU tests that reuse the
cases show something."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _abi, _curve_fit, models

import _response_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 17])
@pytest.mark.parametrize("m", [1, 5, 30])
def test_apply_response_is_the_slice_of_the_full_convolution(L, m):
    """L in {1, 2, 17} against m in {1, 5, 30}: L > m included; origin 0, L // 2, L - 1; shared and per-problem h."""
    rng = np.random.default_rng([L, m])
    g = rng.standard_normal((3, m))
    for origin in sorted({0, L // 2, L - 1}):
        h = rng.standard_normal(L)
        hb = rng.standard_normal((3, L))
        got, got_b = models.apply_response(g, h, origin), models.apply_response(g, hb, origin)
        assert got.shape == got_b.shape == (3, m) and got.dtype == np.float64
        for b in range(3):
            np.testing.assert_allclose(got[b], np.convolve(g[b], h)[origin:origin + m], rtol=0, atol=1e-13)
            np.testing.assert_allclose(got_b[b], np.convolve(g[b], hb[b])[origin:origin + m], rtol=0, atol=1e-13)
            np.testing.assert_allclose(got[b], rc.loop_reference(g[b], h, origin), rtol=0, atol=1e-13)
            np.testing.assert_allclose(got_b[b], rc.loop_reference(g[b], hb[b], origin), rtol=0, atol=1e-13)
        if L % 2 == 1 and origin == L // 2 and m >= L:
            np.testing.assert_allclose(got[0], np.convolve(g[0], h, "same"), rtol=0, atol=1e-13)
        np.testing.assert_array_equal(models.apply_response(g[0], h, origin), got[0])           # one problem, 1-D


def test_apply_response_keeps_extended_precision_and_takes_jacobian_columns():
    rng = np.random.default_rng(3)
    g, h = rng.standard_normal((2, 9)).astype(np.longdouble), rng.standard_normal(4)
    assert models.apply_response(g, h, 1).dtype == np.longdouble
    G = rng.standard_normal((2, 9, 3))
    hb = rng.standard_normal((2, 4))
    J = models.response_jacobian(lambda x, P: G, hb, 2)(None, None)
    assert J.shape == G.shape
    for b in range(2):
        for j in range(3):
            np.testing.assert_allclose(J[b, :, j], np.convolve(G[b, :, j], hb[b])[2:11], rtol=0, atol=1e-13)
    ident = models.apply_response(g, [1.0], 0)
    assert np.array_equal(ident, g)


@pytest.mark.parametrize("spec,h,origin", [("exp*2", rc.irf(), 0), ("gauss+poly*1", rc.irf(15, 7.0, 2.0), 7),
                                           ("gauss+poly*1", np.stack([rc.irf(5, 2.0, 1.0), rc.irf(5, 1.0, 0.7)]), 2)])
def test_wrappers_against_central_differences(spec, h, origin):
    M = models.compose(spec)
    x = np.arange(40, dtype=float)
    P = np.array([[50.0, 0.4, 20.0, 0.06], [40.0, 0.5, 25.0, 0.05]] if spec == "exp*2"
                 else [[30.0, 18.0, 3.0, 2.0], [25.0, 22.0, 4.0, 1.0]])
    f, jac = models.response_residual(M.f, h, origin), models.response_jacobian(M.jac, h, origin)
    J = jac(x, P)
    assert J.shape == (2, 40, M.n)
    for j in range(M.n):
        d = 1e-6 * np.abs(P[:, j])
        Pp, Pm = P.copy(), P.copy()
        Pp[:, j] += d
        Pm[:, j] -= d
        fd = (f(x, Pp) - f(x, Pm)) / (2 * d[:, None])
        np.testing.assert_allclose(J[:, :, j], fd, rtol=2e-7, atol=1e-7 * np.max(np.abs(J[:, :, j])))


# ---- the checks -------------------------------------------------------------------------------------------------------
X5, Y25, P24 = np.arange(5.0), np.ones((2, 5)), np.ones((2, 4))


@pytest.mark.parametrize("kw,match", [
    (dict(response=np.zeros(3)), "all zero"),
    (dict(response=[1.0, np.nan]), "finite"),
    (dict(response=[1.0, np.inf]), "finite"),
    (dict(response=np.ones(models.RESPONSE_MAX_L + 1)), "1 .. 1024"),
    (dict(response=np.ones(0)), "1 .. 1024"),
    (dict(response=np.ones(3), response_origin=3), "0 .. L - 1"),
    (dict(response=np.ones(3), response_origin=-1), "0 .. L - 1"),
    (dict(response=np.ones(3), response_origin=1.0), "integer"),
    (dict(response=np.ones((3, 3))), r"\(L,\) or \(B, L\)"),
    (dict(response=np.ones((2, 2, 2))), r"\(L,\) or \(B, L\)"),
    (dict(response=1.0), r"\(L,\) or \(B, L\)"),
])
@pytest.mark.parametrize("driver", ["host", "device"])
def test_a_bad_kernel_is_a_value_error_before_any_gpu_is_touched(kw, match, driver, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_abi, "Context", boom)
    monkeypatch.setattr(_curve_fit, "least_squares_batch", boom)
    with pytest.raises(ValueError, match=match):
        bounded_lsq.curve_fit_batch("gauss+poly*1", X5, Y25, P24, driver=driver, **kw)
    with pytest.raises(ValueError, match=match):
        bounded_lsq.curve_fit_batch(models.compose("gauss+poly*1").f, X5, Y25, P24, driver=driver, **kw)
    with pytest.raises(ValueError, match=match):
        models.evaluate("gauss+poly*1", X5, P24, **kw)
    with pytest.raises(ValueError, match=match):
        models.DeviceFit("gauss+poly*1", 4, X5, Y25, **kw)
    if np.ndim(kw["response"]) != 2:
        with pytest.raises(ValueError, match=match):
            bounded_lsq.curve_fit(lambda x, a, b: a * x + b, X5, np.ones(5), p0=[1.0, 1.0], **kw)


def test_what_a_response_does_not_combine_with_names_the_reason(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_abi, "Context", boom)
    monkeypatch.setattr(_curve_fit, "least_squares_batch", boom)
    h = np.ones(3)
    with pytest.raises(ValueError, match="not supported by `curve_fit_global`"):
        bounded_lsq.curve_fit_global("gauss+poly*1", X5, Y25, P24, shared=[1], response=h)
    for driver in ("host", "device"):
        with pytest.raises(ValueError, match="2 coordinates"):
            bounded_lsq.curve_fit_batch("gauss2d", np.ones((2, 5)), Y25, np.ones((2, 5)), response=h, driver=driver)
        rows = np.stack([X5, X5 + 1.0])                                     # bins as rows lo, hi: the gap form
        with pytest.raises(ValueError, match="contiguous bins"):
            bounded_lsq.curve_fit_batch("gauss+poly*1", rows, Y25, P24, response=h, binned=True, driver=driver)
    with pytest.raises(ValueError, match="2 coordinates"):
        models.evaluate("gauss2d", np.ones((2, 5)), np.ones((2, 5)), response=h)
    with pytest.raises(ValueError, match="contiguous bins"):
        models.evaluate("gauss+poly*1", np.stack([X5, X5 + 1.0]), P24, binned=True, response=h)
    with pytest.raises(ValueError, match="global fit"):
        models.DeviceFit("gauss+poly*1", 4, X5, np.ones((1, 2, 5)), global_map=bounded_lsq.GlobalMap(4, 2, [1]),
                         response=h)
    with pytest.raises(ValueError, match=r"shape \(L,\) in `curve_fit`"):
        bounded_lsq.curve_fit(lambda x, a, b: a * x + b, X5, np.ones(5), p0=[1.0, 1.0], response=np.ones((1, 3)))


# ---- routing ----------------------------------------------------------------------------------------------------------
class _Spy(Exception):
    pass


def _spied(monkeypatch, *args, **kw):
    """curve_fit_batch with the solve replaced by a spy -> (fun, x0, jac, keywords) as least_squares_batch gets them."""
    seen = {}

    def spy(fun, x0, jac, **k):
        seen.update(fun=fun, x0=x0, jac=jac, kw=k)
        raise _Spy()
    monkeypatch.setattr(_curve_fit, "least_squares_batch", spy)
    with pytest.raises(_Spy):
        bounded_lsq.curve_fit_batch(*args, **kw)
    return seen


@pytest.mark.parametrize("name", ["decay-sigma-exp2", "decay-counts-exp+poly", "line-omit", "line-tied-ratio",
                                  "decay-per-problem-h"])
def test_host_routes_hand_the_solver_the_definition(name, monkeypatch):
    """driver='host' with the spec, and the model's numpy functions as callables on either driver: what the solver is
    given is the residual and the Jacobian of tests/_response_cases.definition, in every bit."""
    case = rc.CASES[name]()
    M = models.compose(case["spec"])
    pm, fres, jres = rc.definition(case)
    X = case["P0"] if pm is None else pm.reduce_x(case["P0"])
    common = dict(bounds=case["bounds"], sigma=case["sigma"], response=case["h"], response_origin=case["origin"],
                  **case["kw"])
    with np.errstate(invalid="ignore"):
        want_f, want_J = fres(X), jres(X)
    for args, kw in (((case["spec"],), dict(driver="host")), ((M.f,), dict(jac=M.jac, driver="host")),
                     ((M.f,), dict(jac=M.jac, driver="device"))):
        seen = _spied(monkeypatch, *args, case["x"], case["Y"], case["P0"], **common, **kw)
        assert np.array_equal(seen["x0"], X)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(seen["fun"](X), want_f), (name, kw)
            assert np.array_equal(seen["jac"](X), want_J), (name, kw)
    seen = _spied(monkeypatch, M.f, case["x"], case["Y"], case["P0"], driver="host", **common)
    assert seen["jac"] == "2-point"


def test_without_the_keyword_nothing_is_wrapped(monkeypatch):
    case = rc.CASES["decay-sigma-exp2"]()
    M = models.compose(case["spec"])

    def boom(*a, **k):
        raise AssertionError("apply_response was reached")
    monkeypatch.setattr(models, "apply_response", boom)
    seen = _spied(monkeypatch, M.f, case["x"], case["Y"], case["P0"], jac=M.jac, sigma=case["sigma"])
    seen["fun"](case["P0"]), seen["jac"](case["P0"])
    seen = _spied(monkeypatch, case["spec"], case["x"], case["Y"], case["P0"], sigma=case["sigma"], driver="device")
    assert isinstance(seen["fun"], models.DeviceFit) and seen["fun"].response is None


class _Recorder:
    """Stands in for a context: hands out tokens for device memory and records every call of the library by name."""

    def __init__(self):
        self.calls, self.h, self.lib, self.freed, self._next = [], "ctx", self, [], 0

    def to_device(self, a):
        self._next += 1
        return ("dev", self._next, np.array(a, copy=True))

    def malloc(self, nbytes):
        self._next += 1
        return ("mem", self._next, int(nbytes))

    def free(self, p):
        self.freed.append(p)

    def check(self, rc_, what=""):
        assert rc_ == 0

    def adopt(self, plan):
        pass

    def __getattr__(self, name):
        if not name.startswith("blsq_"):
            raise AttributeError(name)

        def entry(*a):
            self.calls.append((name, a))
            return 0
        return entry


@pytest.mark.parametrize("name", ["decay-counts-exp2", "line-tied-ratio", "decay-per-problem-h"])
def test_device_route_binds_the_inner_entry_bare_and_the_response_entry_behind_it(name, monkeypatch):
    """The spec on driver='device': the solver gets a DeviceFit that carries the kernel; the DeviceModel it opens calls
    the inner entry exactly as ``models.evaluate`` would (y, w NULL, no estimator, no omission) into its scratch
    buffers, and blsq_response_apply_dev behind it with the data, the weights, the estimator and the policy."""
    case = rc.CASES[name]()
    seen = _spied(monkeypatch, case["spec"], case["x"], case["Y"], case["P0"], bounds=case["bounds"],
                  sigma=case["sigma"], driver="device", response=case["h"], response_origin=case["origin"], **case["kw"])
    fit = seen["fun"]
    assert isinstance(fit, models.DeviceFit) and seen["jac"] is None
    assert np.array_equal(fit.response, case["h"]) and fit.response_origin == case["origin"]
    ctx = _Recorder()
    dm = fit.open_device(ctx, -np.inf, np.inf)
    B, m, nf = fit.B, fit.m, fit.n
    poisson, omit = case["kw"].get("estimator") == "poisson", case["kw"].get("nan_policy") == "omit"
    L = case["h"].shape[-1]

    def split(call, inner_name):
        names = _abi.MODEL_EVAL_ARGS[inner_name]
        return dict(zip(names, call[1][1:]))

    dm.fun_dev("X", "F", 3)
    (inner, resp), ctx.calls = ctx.calls, []
    plain = models.DeviceModel(_Recorder(), case["spec"], B, m, fit.n_model, case["x"],
                               param_map=fit.param_map, Pfix=fit.Pfix)     # the same fit with ydata=None, no keyword
    plain.fun_dev("X", "F", 3)
    assert inner[0] == plain.ctx.calls[0][0] and inner[0].startswith("blsq_model_eval")
    a = split(inner, inner[0])
    assert a["y"] is None and a["w"] is None and a["X"] == "X" and a["reps"] == 3 and a["J"] is None
    assert a.get("est", 0) == 0 and a.get("nan_policy", 0) == 0
    g = a["f"]
    assert g[0] == "mem" and g[2] == 8 * B * 3 * m
    assert resp[0] == "blsq_response_apply_dev"
    (h_, est, nanp, B_, reps, m_, nc, L_, origin, d_h, h_stride, d_g, d_G, d_y, d_w, w_stride, f, J, mask) = resp[1]
    assert (h_, est, nanp, B_, reps, m_, nc, L_, origin) == ("ctx", int(poisson), int(omit), B, 3, m, nf, L,
                                                              case["origin"])
    assert np.array_equal(d_h[2], case["h"]) and h_stride == (L if case["h"].ndim == 2 else 0)
    assert d_g is g and d_G is None and (f, J, mask) == ("F", None, None)
    assert np.array_equal(d_y[2], case["Y"], equal_nan=True)
    assert (d_w is None) == (case["sigma"] is None) and w_stride in (0, m)

    dm.jac_dev("X", "J", "MASK")
    (inner, resp), ctx.calls = ctx.calls, []
    a = split(inner, inner[0])
    assert a["J"][0] == "mem" and a["J"][2] == 8 * B * m * nf and a["mask"] == "MASK" and a["reps"] == 1
    assert (a["f"] is g) if poisson else (a["f"] is None)                  # c of the Poisson Jacobian needs mu
    assert resp[1][11] is a["f"] and resp[1][12] is a["J"] and resp[1][16:] == (None, "J", "MASK")
    dm.fun_dev("X", "F", 5)                                                # more points than before: g grows
    assert ctx.calls[0][1][_abi.MODEL_EVAL_ARGS[inner[0]].index("f") + 1][2] == 8 * B * 5 * m and g in ctx.freed
    dm.close()
    assert {p[1] for p in ctx.freed if p[0] == "mem"} >= {a["J"][1]}


def test_curve_fit_wraps_a_callable_and_keeps_its_signature(monkeypatch):
    """One problem: f and a callable jac are convolved before the data are looked at; p0=None still counts the
    arguments of f; under 'omit' the model is evaluated on the whole grid and the NaN points are dropped afterwards."""
    h = rc.irf(5, 2.0, 1.0)
    x = np.arange(12.0)
    y = np.ones(12)
    y[[0, 11]] = np.nan

    def f(x, a, r):
        return a * np.exp(-r * x)

    def jac(x, a, r):
        return np.stack([np.exp(-r * x), -a * x * np.exp(-r * x)], axis=1)
    fc, jc, xs, ys, sg = _curve_fit._response_single(f, jac, x, y, np.arange(1.0, 13.0), "omit", h, 2)
    from inspect import getfullargspec
    assert getfullargspec(fc).args == ["x", "a", "r"]
    keep = ~np.isnan(y)
    assert np.array_equal(fc(xs, 3.0, 0.2), models.apply_response(f(x, 3.0, 0.2), h, 2)[keep])
    assert np.array_equal(jc(xs, 3.0, 0.2), models.apply_response(jac(x, 3.0, 0.2).T, h, 2).T[keep])
    assert np.array_equal(ys, y[keep]) and np.array_equal(sg, np.arange(1.0, 13.0)[keep]) and xs.shape == (10,)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_bound_and_refuses_a_null_context():
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    assert re.search(r"#define\s+BLSQ_RESPONSE_MAX_L\s+1024\b", src) and models.RESPONSE_MAX_L == 1024
    proto = re.search(r"int\s+blsq_response_apply_dev\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    params = [p.strip() for p in proto.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "est", "nan_policy", "B", "reps", "m", "nc", "L", "origin", "dh", "h_stride", "dg", "dG",
                     "dy", "dw", "w_stride", "df", "dJ", "dmask"]
    res, args = _abi.SIGNATURES["blsq_response_apply_dev"]
    assert res is C.c_int and len(args) == len(params)
    for p, t in zip(params, args):                                         # ints, longs and pointers line up
        want = C.c_void_p if "*" in p else C.c_long if p.startswith("long") else C.c_int
        assert t is want, (p, t)
    lib = _abi.load()
    fn = lib.blsq_response_apply_dev
    assert fn(None, 0, 0, 1, 1, 1, 1, 1, 0, None, 0, None, None, None, None, 0, None, None, None) == -1
    assert "blsq_response_apply_dev" not in _abi.MODEL_EVAL_ARGS           # a second stage, not a model-eval entry


# ---- the cases, with scipy alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases_show_something_to_scipy(name):
    case = rc.CASES[name]()
    for b in range(rc.B):
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            x, se, lb, ub, T = rc.scipy_fit(case, b)
            x0, se0, _, _, _ = rc.scipy_fit(case, b, with_response=False)
        assert np.all((x > lb) & (x < ub)), (name, b, x)
        assert np.all(np.isfinite(se)) and np.all(np.abs(x - T) <= 6 * se), (name, b, np.abs(x - T) / se)
        # without the response: measured in its own standard errors, or (a collapsed component has none) in those above
        se0 = np.where(np.isfinite(se0) & (se0 > 0), se0, se)
        assert np.max(np.abs(x0 - T) / se0) > 6, (name, b, np.abs(x0 - T) / se0)
