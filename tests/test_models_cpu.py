"""Built-in fit models (bounded_lsq.models) without a GPU: the registry against the rules for n and the library's own
table, the numpy Jacobians against central differences of the numpy functions in extended precision, and the argument
checks of ``curve_fit_batch(f='name')``, which are raised before any library or device call."""
import ctypes as C

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

from _model_cases import case_inputs

LD = np.longdouble
# name -> (n that fit, n that do not)
N_RULES = {
    "poly": ([1, 2, 7, 64], [0, 65]),
    "exp_sum": ([3, 5, 63], [1, 2, 4, 65]),
    "gauss_sum": ([4, 7, 64], [1, 3, 5, 6, 67]),
    "lorentz_sum": ([4, 7, 64], [1, 2, 5, 67]),
    "gauss2d": ([5], [1, 4, 6, 10]),
}
# one case per family (and two widths of the sums): name, n
JAC_CASES = [("poly", 1), ("poly", 6), ("exp_sum", 3), ("exp_sum", 7), ("gauss_sum", 4), ("gauss_sum", 10),
             ("lorentz_sum", 7), ("gauss2d", 5)]


def test_registry_and_n_rules():
    assert models.NAMES == ("poly", "exp_sum", "gauss_sum", "lorentz_sum", "gauss2d")
    assert [models.get(nm).id for nm in models.NAMES] == [0, 1, 2, 3, 4]
    assert [models.get(nm).coords for nm in models.NAMES] == [1, 1, 1, 1, 2]
    for name, (good, bad) in N_RULES.items():
        M = models.get(name)
        for n in good:
            K = M.terms(n)
            assert n == M.n_base + K * M.n_per_term or (M.n_per_term == 0 and n == M.n_base)
        for n in bad:
            with pytest.raises(ValueError, match="does not take n"):
                M.terms(n)
    assert models.get("gauss_sum").terms(64) == 21 and models.get("exp_sum").terms(7) == 3
    for bad in ("gauss", "", None, 3):
        with pytest.raises(ValueError, match="unknown model"):
            models.get(bad)


def test_registry_matches_the_library_table():
    """blsq_model_count / blsq_model_info need no device."""
    from bounded_lsq import _abi
    lib = _abi.load()
    assert lib.blsq_model_count() == len(models.NAMES)
    for i, name in enumerate(models.NAMES):
        nm, co, nb, nt = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.blsq_model_info(i, C.byref(nm), C.byref(co), C.byref(nb), C.byref(nt)) == 0
        M = models.get(name)
        assert (nm.value.decode(), co.value, nb.value, nt.value) == (name, M.coords, M.n_base, M.n_per_term)
    assert lib.blsq_model_info(len(models.NAMES), None, None, None, None) != 0
    assert lib.blsq_model_info(-1, None, None, None, None) != 0


@pytest.mark.parametrize("name,n", JAC_CASES, ids=["%s-%d" % c for c in JAC_CASES])
@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "perproblem"])
def test_numpy_jac_against_central_differences_in_longdouble(name, n, per_problem):
    """jac (float64) against (f(p + h e_j) - f(p - h e_j)) / 2h of the same function evaluated in np.longdouble.
    With h = 1e-6 on parameters of order 1 the truncation error is h^2 / 6 |f'''| ~ 1e-12 (third derivatives of these
    models at these parameters stay below 1e2: 1.7e-11), the rounding error of the longdouble quotient is
    2^-64 |f| / h ~ 1e-13 and the float64 Jacobian itself carries ~1e-15: 1e-9 relative to the largest entry of
    the column leaves two decades."""
    B, m = 3, 17
    x, P = case_inputs(name, n, B, m, seed=n, per_problem=per_problem)
    M = models.get(name)
    F, J = M.f(x, P), M.jac(x, P)
    assert F.shape == (B, m) and F.dtype == np.float64
    assert J.shape == (B, m, n) and J.dtype == np.float64
    xl, Pl = x.astype(LD), P.astype(LD)
    assert M.f(xl, Pl).dtype == LD and M.jac(xl, Pl).dtype == LD
    h = LD(1e-6)
    for j in range(n):
        Pp, Pm = Pl.copy(), Pl.copy()
        Pp[:, j] += h
        Pm[:, j] -= h
        col = (M.f(xl, Pp) - M.f(xl, Pm)) / (2 * h)
        err = np.max(np.abs(col - J[:, :, j]))
        assert float(err) <= 1e-9 * max(1.0, float(np.max(np.abs(col)))), (name, j, float(err))


def test_shared_and_per_problem_xdata_give_the_same_values():
    for name, n in JAC_CASES:
        x, P = case_inputs(name, n, 3, 9, seed=1)
        M = models.get(name)
        xb = np.broadcast_to(x, (3,) + x.shape).copy()
        assert np.array_equal(M.f(x, P), M.f(xb, P)) and np.array_equal(M.jac(x, P), M.jac(xb, P))


def test_non_finite_values_pass_through():
    t = np.array([-1.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        F = models.get("gauss_sum").f(t, np.array([[1.0, 0.0, 0.0, 0.5]]))       # s = 0: z = -inf, nan, inf
        assert F[0, 0] == 0.5 and np.isnan(F[0, 1]) and F[0, 2] == 0.5
        J = models.get("lorentz_sum").jac(t, np.array([[1.0, 0.0, 0.0, 0.5]]))
        assert np.isnan(J[0, 1, 0]) and J[0, 0, 0] == 0.0


# ---- curve_fit_batch(f='name'): the checks that need neither the library nor a device ----------------------------
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
def test_curve_fit_batch_value_errors_for_names(no_library, driver):
    t = np.linspace(-2, 2, 12)
    Y = np.zeros((3, 12))
    kw = dict(driver=driver)
    with pytest.raises(ValueError, match="unknown model"):
        bounded_lsq.curve_fit_batch("gaussian", t, Y, np.ones((3, 4)), **kw)
    with pytest.raises(ValueError, match="does not take n"):
        bounded_lsq.curve_fit_batch("gauss_sum", t, Y, np.ones((3, 5)), **kw)
    with pytest.raises(ValueError, match="does not take n"):
        bounded_lsq.curve_fit_batch("gauss2d", np.zeros((2, 12)), Y, np.ones((3, 4)), **kw)
    with pytest.raises(ValueError, match="does not take n"):
        bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 65)), **kw)
    for bad_x in (np.zeros(11), np.zeros((2, 12)), np.zeros((3, 11)), np.zeros((3, 1, 12))):
        with pytest.raises(ValueError, match="`xdata` of model"):
            bounded_lsq.curve_fit_batch("exp_sum", bad_x, Y, np.ones((3, 3)), **kw)
    for bad_x in (t, np.zeros((3, 12)), np.zeros((2, 2, 12)), np.zeros((3, 2, 11))):
        with pytest.raises(ValueError, match="`xdata` of model"):
            bounded_lsq.curve_fit_batch("gauss2d", bad_x, Y, np.ones((3, 5)), **kw)
    with pytest.raises(ValueError, match="callable `jac`"):
        bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 2)), jac=lambda x, P: None, **kw)
    with pytest.raises(ValueError, match="`jac` must be"):
        bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 2)), jac="cs", **kw)
    with pytest.raises(ValueError, match="2-D covariance"):
        bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 2)), sigma=np.eye(12), **kw)
    with pytest.raises(ValueError, match="`driver`"):
        bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 2)), driver="gpu")


def _capture(monkeypatch):
    from bounded_lsq import _curve_fit
    seen = {}

    class Stop(Exception):
        pass

    def fake(fun, x0, jac, **kw):
        seen.update(fun=fun, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, "least_squares_batch", fake)
    return seen, Stop


def test_jac_none_with_a_callable_still_means_two_point(monkeypatch):
    seen, Stop = _capture(monkeypatch)
    t = np.linspace(0, 1, 8)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(lambda x, P: P[:, :1] * x, t, np.zeros((2, 8)), np.ones((2, 1)))
    assert seen["jac"] == "2-point" and callable(seen["fun"])
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(lambda x, P: P[:, :1] * x, t, np.zeros((2, 8)), np.ones((2, 1)), jac=None)
    assert seen["jac"] == "2-point"
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(lambda x, P: P[:, :1] * x, t, np.zeros((2, 8)), np.ones((2, 1)), jac="3-point")
    assert seen["jac"] == "3-point"


def test_what_a_name_hands_to_the_batch_solver(monkeypatch):
    """driver='device': a DeviceFit and jac None (analytic on the device) or the finite-difference name;
    driver='host': the numpy functions as weighted callables."""
    seen, Stop = _capture(monkeypatch)
    x, P = case_inputs("gauss_sum", 4, 2, 8)
    Y = models.get("gauss_sum").f(x, P) + 0.25
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, sigma=0.5, driver="device")
    assert isinstance(seen["fun"], models.DeviceFit) and seen["jac"] is None and seen["kw"]["driver"] == "device"
    assert (seen["fun"].B, seen["fun"].m, seen["fun"].n) == (2, 8, 4)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, jac="2-point", driver="device")
    assert isinstance(seen["fun"], models.DeviceFit) and seen["jac"] == "2-point"
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, sigma=0.5, driver="host")
    np.testing.assert_array_equal(seen["fun"](P), 2.0 * (models.get("gauss_sum").f(x, P) - Y))    # (f - y) / sigma
    np.testing.assert_array_equal(seen["jac"](P), 2.0 * models.get("gauss_sum").jac(x, P))
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, jac="3-point", driver="host")
    assert seen["jac"] == "3-point" and callable(seen["fun"])


def test_least_squares_batch_refuses_device_callbacks_on_the_host_driver():
    x, P = case_inputs("poly", 2, 2, 8)
    fit = models.DeviceFit("poly", 2, x, np.zeros((2, 8)))
    with pytest.raises(ValueError, match="driver='device'"):
        bounded_lsq.least_squares_batch(fit, P, None, driver="host")
    with pytest.raises(ValueError, match="`jac` must be None"):
        bounded_lsq.least_squares_batch(fit, P, lambda X: None, driver="device")
    with pytest.raises(ValueError, match="`x0` must have shape"):
        bounded_lsq.least_squares_batch(fit, np.ones((2, 3)), None, driver="device")
