"""Composite fit models (bounded_lsq.models.compose) without a GPU: the grammar and its errors, the
bit-for-bit identities with the five closed families, the numpy Jacobians against central differences in extended
precision, the float64 numpy definition against its longdouble evaluation within the bound the GPU test holds the
kernel to, the library's term table, and the vetting of the end-to-end fit problems of tests/test_composite_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

import _composite_cases as cc
from _model_cases import case_inputs

LD = np.longdouble


# ---- grammar -------------------------------------------------------------------------------------------------------
def test_grammar_names_and_order():
    M = models.compose(" gauss * 2 + lorentz+poly*2 ")
    assert isinstance(M, models.CompositeModel)
    assert M.name == "gauss*2+lorentz*1+poly*2" and M.n == 11 and M.coords == 1
    assert M.components == (("gauss", 2), ("lorentz", 1), ("poly", 2))
    assert M.param_names == ("gauss0.a", "gauss0.mu", "gauss0.s", "gauss1.a", "gauss1.mu", "gauss1.s",
                             "lorentz0.a", "lorentz0.mu", "lorentz0.s", "poly0.p0", "poly0.p1")
    assert models.compose(M.name).name == M.name                       # the canonical spec is a fixed point
    # order is kept and a family may repeat
    R = models.compose("poly*1+gauss+exp+gauss+pvoigt")
    assert R.components == (("poly", 1), ("gauss", 1), ("exp", 1), ("gauss", 1), ("pvoigt", 1)) and R.n == 13
    assert R.param_names == ("poly0.p0", "gauss0.a", "gauss0.mu", "gauss0.s", "exp0.a", "exp0.r", "gauss1.a",
                             "gauss1.mu", "gauss1.s", "pvoigt0.a", "pvoigt0.mu", "pvoigt0.s", "pvoigt0.eta")
    assert [(t.name, t.id, t.n_per_term) for t in models.TERMS.values()] == [
        ("gauss", 0, 3), ("lorentz", 1, 3), ("pvoigt", 2, 4), ("exp", 3, 2), ("poly", 4, 1)]
    assert models.compose("pvoigt*15+poly*4").n == 64 and models.compose("poly*64").n == 64
    assert models.compose(cc.EIGHT).n == 24 and len(models.compose(cc.EIGHT).components) == 8
    assert M.terms(11) == 5
    for n in (10, 12, 0):
        with pytest.raises(ValueError, match="does not take n"):
            M.terms(n)
    x, per = M.check_xdata(np.zeros((3, 7)), 3, 7)
    assert per and x.shape == (3, 7) and not M.check_xdata(np.zeros(7), 3, 7)[1]
    with pytest.raises(ValueError, match="`xdata` of model"):
        M.check_xdata(np.zeros((2, 7)), 3, 7)


@pytest.mark.parametrize("spec,piece", [
    ("gauss+voigt*2", "voigt"), ("gauss_sum+poly*1", "gauss_sum"), ("gauss*0+poly*1", "gauss\\*0"),
    ("gauss*-1", "gauss\\*-1"), ("gauss*two", "gauss\\*two"), ("gauss*1.5", "gauss\\*1.5"), ("gauss*", "gauss\\*"),
    ("gauss++poly*1", "empty component"), ("+gauss", "empty component"), ("gauss+", "empty component"),
    ("", "empty component"), ("*3", "''"), ("gauss*2*2", "gauss\\*2\\*2"),
    ("+".join(["poly*1"] * 9), "9 components"), ("pvoigt*16+poly*1", "n = 65"), ("poly*65", "n = 65")])
def test_grammar_errors_name_the_piece(spec, piece):
    with pytest.raises(ValueError, match=piece):
        models.compose(spec)


def test_resolve_and_the_unchanged_registry():
    assert models.NAMES == ("poly", "exp_sum", "gauss_sum", "lorentz_sum", "gauss2d") and tuple(models.MODELS) == models.NAMES
    for name in models.NAMES:
        assert models.resolve(name) is models.get(name)
    M = models.compose("gauss+poly*1")
    assert models.resolve(M) is M
    assert models.resolve("gauss+poly*1").name == M.name and models.resolve("poly*3").name == "poly*3"
    for bad in ("gauss", "", None, 3):
        with pytest.raises(ValueError, match="unknown model"):
            models.get(bad)
        with pytest.raises(ValueError, match="unknown model"):
            models.resolve(bad)
    with pytest.raises(ValueError, match="unknown model"):
        models.get("gauss+poly*1")                                     # get takes the five names only


def test_term_table_matches_the_library():
    """blsq_term_count / blsq_term_info need no device; blsq_model_count stays 5."""
    from bounded_lsq import _abi
    lib = _abi.load()
    assert lib.blsq_term_count() == len(models.TERMS) == 5 and lib.blsq_model_count() == 5
    for name, T in models.TERMS.items():
        nm, npt = C.c_char_p(), C.c_int32()
        assert lib.blsq_term_info(T.id, C.byref(nm), C.byref(npt)) == 0
        assert (nm.value.decode(), npt.value) == (name, T.n_per_term)
    assert lib.blsq_term_info(0, None, None) == 0
    assert lib.blsq_term_info(5, None, None) != 0 and lib.blsq_term_info(-1, None, None) != 0


# ---- the identities with the closed families -----------------------------------------------------------------------
IDENTITIES = [("gauss*%d+poly*1", "gauss_sum", 3), ("lorentz*%d+poly*1", "lorentz_sum", 3), ("exp*%d+poly*1", "exp_sum", 2)]


@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "perproblem"])
@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["float64", "longdouble"])
def test_bit_for_bit_identities(dtype, per_problem):
    for fmt, name, w in IDENTITIES:
        for K in (1, 2, 5, 63 // w):
            n = w * K + 1
            x, P = case_inputs(name, n, 3, 19, seed=K, per_problem=per_problem)
            x, P = x.astype(dtype), P.astype(dtype)
            M, R = models.compose(fmt % K), models.get(name)
            assert M.n == n
            f, J = M.f(x, P), M.jac(x, P)
            assert f.dtype == dtype and J.dtype == dtype and f.shape == (3, 19) and J.shape == (3, 19, n)
            assert np.array_equal(f, R.f(x, P)) and np.array_equal(J, R.jac(x, P)), (name, K)
    for n in (1, 2, 7, 64):
        x, P = case_inputs("poly", n, 3, 19, seed=n, per_problem=per_problem)
        x, P = x.astype(dtype), P.astype(dtype)
        M, R = models.compose("poly*%d" % n), models.get("poly")
        assert np.array_equal(M.f(x, P), R.f(x, P)) and np.array_equal(M.jac(x, P), R.jac(x, P)), n


def test_component_order_is_the_summation_order():
    """'poly*1+gauss' adds the peak to the constant, 'gauss+poly*1' the constant to the peak: the same real number,
    the same parameters permuted — and the two orders of a three-component sum differ in some last bit."""
    x, P = cc.comp_inputs("gauss+lorentz+poly*1", 4, 200, seed=3)
    a = models.compose("gauss+lorentz+poly*1").f(x, P)
    b = models.compose("poly*1+lorentz+gauss").f(x, P[:, [6, 3, 4, 5, 0, 1, 2]])
    np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)
    assert not np.array_equal(a, b)
    g = models.compose("gauss").f(x, P[:, :3])
    lo = models.compose("lorentz").f(x, P[:, 3:6])
    assert np.array_equal(a, (g + lo) + P[:, 6:7]) and np.array_equal(b, (P[:, 6:7] + lo) + g)


# ---- the numpy Jacobian --------------------------------------------------------------------------------------------
JAC_SPECS = ["gauss*2", "lorentz*2", "pvoigt*2", "exp*2", "poly*5", "gauss*2+lorentz+pvoigt+exp+poly*3"]


@pytest.mark.parametrize("spec", JAC_SPECS)
@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "perproblem"])
def test_numpy_jac_against_central_differences_in_longdouble(spec, per_problem):
    """jac (float64) against (f(p + h e_j) - f(p - h e_j)) / 2h of the same function in np.longdouble, with the
    figures of tests/test_models_cpu.py: h = 1e-6, 1e-9 of the column's largest entry (its docstring: truncation
    h^2 / 6 |f'''| ~ 1e-11 at these parameters, quotient rounding 1e-13)."""
    B, m = 3, 17
    x, P = cc.comp_inputs(spec, B, m, seed=len(spec), per_problem=per_problem)
    M = models.compose(spec)
    F, J = M.f(x, P), M.jac(x, P)
    assert F.shape == (B, m) and F.dtype == np.float64 and J.shape == (B, m, M.n) and J.dtype == np.float64
    xl, Pl = x.astype(LD), P.astype(LD)
    assert M.f(xl, Pl).dtype == LD and M.jac(xl, Pl).dtype == LD
    h = LD(1e-6)
    for j in range(M.n):
        Pp, Pm = Pl.copy(), Pl.copy()
        Pp[:, j] += h
        Pm[:, j] -= h
        col = (M.f(xl, Pp) - M.f(xl, Pm)) / (2 * h)
        err = np.max(np.abs(col - J[:, :, j]))
        assert float(err) <= 1e-9 * max(1.0, float(np.max(np.abs(col)))), (spec, M.param_names[j], float(err))


@pytest.mark.parametrize("spec", cc.KERNEL_SPECS)
def test_float64_numpy_meets_the_kernel_bound(spec):
    """The float64 numpy definition against its longdouble evaluation within _composite_cases.bounds_of, for every
    spec, row count and variant of test_composite_gpu.py::test_kernel_against_longdouble: the bound is attainable by
    the formulas as written, so a failure there is the kernel's."""
    worst = 0.0
    for m in cc.ROWS:
        for variant in cc.VARIANTS:
            B, per_problem, reps, wk, yk = variant
            x, P, w, y = cc.variant_inputs(spec, m, variant)
            f_ref, J_ref, f_tol, J_tol = cc.bounds_of(spec, x, P, w, y, reps=reps)
            f, J = cc.numpy_weighted(spec, x, P, w, y, reps, per_problem)
            rf, rj = cc.worst_ratio(f, f_ref, f_tol), cc.worst_ratio(J, J_ref, J_tol)
            worst = max(worst, rf, rj)
            assert rf <= 1.0 and rj <= 1.0, (spec, m, variant, rf, rj)
    print("composite %s: numpy worst error / bound %.3f" % (spec, worst))


def test_the_bound_reduces_to_the_closed_families():
    """For 'gauss*K+poly*1' the bound is the one of tests/_model_cases.py for gauss_sum with K + 1 summands in place of
    K: never tighter, and wider by 2 eps |w| sum |term| at the most."""
    import _model_cases as mc
    x, P = case_inputs("gauss_sum", 7, 3, 40, seed=2)
    f_ref, J_ref, f_tol, J_tol = cc.bounds_of("gauss*2+poly*1", x, P, None, None)
    f_ref0, J_ref0, f_tol0, J_tol0 = mc.bounds_of("gauss_sum", x, P, None, None)
    assert np.array_equal(f_ref, f_ref0) and np.array_equal(J_ref, J_ref0)
    assert np.all(f_tol >= f_tol0) and np.all(J_tol >= J_tol0)
    assert np.all(f_tol <= f_tol0 * 1.2) and np.all(J_tol <= J_tol0 * 1.2)


# ---- curve_fit_batch(spec): the checks that need neither the library nor a device -----------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library, open a context or start the batch solver fails the test."""
    from bounded_lsq import _abi, _curve_fit

    def boom(*a, **k):
        raise AssertionError("a library or device call was reached")
    monkeypatch.setattr(_abi, "load", boom)
    monkeypatch.setattr(_abi.Context, "__init__", boom)
    monkeypatch.setattr(_curve_fit, "least_squares_batch", boom)


@pytest.mark.parametrize("driver", ["host", "device"])
def test_curve_fit_batch_value_errors_for_specs(no_library, driver):
    t = np.linspace(-2, 2, 12)
    Y = np.zeros((3, 12))
    kw = dict(driver=driver)
    spec = "gauss*2+lorentz+poly*2"
    with pytest.raises(ValueError, match="unknown family 'gaussian'"):
        bounded_lsq.curve_fit_batch("gaussian+poly*1", t, Y, np.ones((3, 4)), **kw)
    with pytest.raises(ValueError, match="K must be at least 1"):
        bounded_lsq.curve_fit_batch("gauss*0+poly*1", t, Y, np.ones((3, 4)), **kw)
    with pytest.raises(ValueError, match="n = 65"):
        bounded_lsq.curve_fit_batch("poly*65", t, Y, np.ones((3, 65)), **kw)
    for n in (10, 12):
        with pytest.raises(ValueError, match="does not take n"):
            bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, n)), **kw)
    with pytest.raises(ValueError, match="does not take n"):
        bounded_lsq.curve_fit_batch(models.compose(spec), t, Y, np.ones((3, 4)), **kw)
    for bad_x in (np.zeros(11), np.zeros((2, 12)), np.zeros((3, 11)), np.zeros((3, 1, 12))):
        with pytest.raises(ValueError, match="`xdata` of model"):
            bounded_lsq.curve_fit_batch(spec, bad_x, Y, np.ones((3, 11)), **kw)
    with pytest.raises(ValueError, match="callable `jac`"):
        bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, 11)), jac=lambda x, P: None, **kw)
    with pytest.raises(ValueError, match="`jac` must be"):
        bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, 11)), jac="cs", **kw)
    with pytest.raises(ValueError, match="2-D covariance"):
        bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, 11)), sigma=np.eye(12), **kw)
    with pytest.raises(ValueError, match="`driver`"):
        bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, 11)), driver="gpu")
    with pytest.raises(ValueError):                                     # the keywords' own checks come first as well
        bounded_lsq.curve_fit_batch(spec, t, Y, np.ones((3, 11)), tied={2: 11}, **kw)


def test_what_a_spec_hands_to_the_batch_solver(monkeypatch):
    """driver='device': a DeviceFit on the composite (with the map of fixed= / tied=) and jac None; driver='host': the
    numpy definition as callables."""
    from bounded_lsq import _curve_fit
    seen = {}

    class Stop(Exception):
        pass

    def fake(fun, x0, jac, **kw):
        seen.update(fun=fun, x0=x0, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, "least_squares_batch", fake)
    pr = cc.fit_problem("tied", 33)
    for f in (pr["spec"], models.compose(pr["spec"])):
        with pytest.raises(Stop):
            bounded_lsq.curve_fit_batch(f, pr["x"], pr["Y"], pr["P0"], driver="device", tied=pr["tied"], fixed=[6])
        fit = seen["fun"]
        assert isinstance(fit, models.DeviceFit) and isinstance(fit.model, models.CompositeModel)
        assert fit.model.name == "gauss*1+lorentz*1+poly*1" and (fit.n, fit.n_model) == (5, 7)
        assert seen["jac"] is None and seen["x0"].shape == (8, 5)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], pr["Y"], pr["P0"], driver="host")
    M = models.compose(pr["spec"])
    assert np.array_equal(seen["fun"](pr["P0"]), M.f(pr["x"], pr["P0"]) - pr["Y"])
    assert np.array_equal(seen["jac"](pr["P0"]), M.jac(pr["x"], pr["P0"]))


# ---- the end-to-end problems of the GPU test, vetted on the CPU ------------------------------------------------------
@pytest.mark.parametrize("m", cc.FIT_ROWS)
@pytest.mark.parametrize("label", list(cc.FITS))
def test_fit_problems_are_well_posed(label, m):
    """scipy.optimize.least_squares on the numpy definition from the test's P0 inside its box, per problem (a tie
    applied through ParamMap): it converges, with no variable on its bound, to within 6 standard errors of the truth
    (sigma^2 (J^T J)^-1 at the solution; 6 sigma over the ~350 fitted values of these problems leaves the chance of
    a miss below 1e-6) — so a failure of the GPU test on these problems points at the device code."""
    from scipy.optimize import least_squares
    pr = cc.fit_problem(label, m)
    M = models.compose(pr["spec"])
    n = M.n
    pm = bounded_lsq.ParamMap(n, None, pr["tied"]) if pr["tied"] else None
    for b in range(pr["P0"].shape[0]):
        P0, lb, ub = pr["P0"][b:b + 1], pr["bounds"][0][b:b + 1], pr["bounds"][1][b:b + 1]
        if pm is None:
            full = lambda v: v[np.newaxis]                                         # noqa: E731
            red_j = lambda J: J                                                    # noqa: E731
            x0, lo, hi = P0[0], lb[0], ub[0]
        else:
            full = lambda v: pm.expand_x(v[np.newaxis], P0)                        # noqa: E731
            red_j = pm.reduce_jac
            x0 = pm.reduce_x(P0)[0]
            lo, hi = (a[0] for a in pm.reduce_bounds(lb, ub))
        fun = lambda v: (M.f(pr["x"], full(v))[0] - pr["Y"][b]) / cc.SIGMA         # noqa: E731
        jac = lambda v: red_j(M.jac(pr["x"], full(v)))[0] / cc.SIGMA               # noqa: E731
        assert np.all(x0 > lo) and np.all(x0 < hi)
        res = least_squares(fun, x0, jac, bounds=(lo, hi), ftol=1e-10, xtol=1e-10, gtol=1e-10)
        assert res.success and res.status > 0, (label, m, b, res.status)
        assert np.all(res.x > lo) and np.all(res.x < hi), (label, m, b)
        se = np.sqrt(np.diag(np.linalg.inv(res.jac.T @ res.jac)))
        truth = pr["truth"][b] if pm is None else pm.reduce_x(pr["truth"][b:b + 1])[0]
        assert np.all(np.abs(res.x - truth) <= 6 * se), (label, m, b, np.abs(res.x - truth) / se)
        assert res.cost * 2 < 2.0 * m                                              # chi^2 of the order of m - n
