"""lsq_linear without a GPU: argument handling with the solve replaced by a spy, the new ABI entry as far as it can be
reached without a context, the numpy definition against explicit loops, and the vetting of the cases the GPU tests
(tests/test_lsq_linear_gpu.py) run: scipy solves every one of them, from the case's start, to far inside the margin the
routes are compared at."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
from scipy import optimize

import bounded_lsq
from bounded_lsq import _abi, _curve_fit, _hostmath, _linear

import _linear_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


class Stop(Exception):
    pass


@pytest.fixture
def spy(monkeypatch):
    """``least_squares_batch`` as `_linear` looks it up: records its arguments and stops."""
    seen = {}

    def solve(fun, x0, jac, **kw):
        seen.update(fun=fun, x0=x0, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_linear, "least_squares_batch", solve)
    return seen


def _data(B=3, m=7, n=4, shared=True, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n) if shared else (B, m, n))
    return A, rng.standard_normal((B, m))


# ---- argument handling ----------------------------------------------------------------------------------------------
def test_exports():
    for name in ("lsq_linear", "lsq_linear_batch", "LinearFit", "LinearDeviceModel"):
        assert getattr(bounded_lsq, name) is getattr(_linear, name) and name in bounded_lsq.__all__


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("driver", ["device", "host"])
def test_what_the_solver_receives(spy, shared, driver):
    A, b = _data(shared=shared)
    lo, hi = np.array([-1.0, -np.inf, 0.0, -np.inf]), np.array([1.0, 2.0, np.inf, np.inf])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # the tolerance mapping must not warn
        with pytest.raises(Stop):
            bounded_lsq.lsq_linear_batch(A, b, bounds=(lo, hi), method="dogbox", tol=1e-9, max_iter=17, driver=driver)
    kw = spy["kw"]
    assert kw["ftol"] == 1e-9 and kw["gtol"] == 1e-9 and kw["xtol"] == EPS
    assert kw["method"] == "dogbox" and kw["max_nfev"] == 17 and kw["scaling"] == 1.0 and kw["driver"] == driver
    assert kw["ctx"] is None and "loss" not in kw and "covariance" not in kw
    assert np.array_equal(kw["bounds"][0], np.broadcast_to(lo, (3, 4))) and kw["bounds"][0].shape == (3, 4)
    assert np.array_equal(kw["bounds"][1], np.broadcast_to(hi, (3, 4)))
    # the strictly feasible start: middle, ub - 1, lb + 1, 1
    assert np.array_equal(spy["x0"], np.broadcast_to([0.0, 1.0, 1.0, 1.0], (3, 4)))
    if driver == "device":
        fit = spy["fun"]
        assert isinstance(fit, bounded_lsq.LinearFit) and spy["jac"] is None
        assert (fit.B, fit.m, fit.n) == (3, 7, 4) and hasattr(fit, "open_device")
        assert np.array_equal(fit.A, A) and np.array_equal(fit.b, b)
    else:
        X = np.arange(12.0).reshape(3, 4)
        fun, jac = _linear.numpy_callbacks(A, b)
        assert np.array_equal(spy["fun"](X), fun(X)) and np.array_equal(spy["jac"](X), jac(X))


def test_default_tolerances_do_not_warn_in_the_real_clamp():
    from bounded_lsq._frontend import _clamp_tolerances
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _clamp_tolerances(1e-10, _linear.EPS, 1e-10) == (1e-10, EPS, 1e-10)


def test_one_problem_is_a_batch_of_one(spy):
    A, b = _data()
    with pytest.raises(Stop):
        bounded_lsq.lsq_linear(A, b[0], bounds=(0, np.inf), x0=[1.0, 2.0, 3.0, 4.0])
    assert spy["fun"].B == 1 and spy["x0"].shape == (1, 4) and np.array_equal(spy["x0"][0], [1, 2, 3, 4])
    assert spy["kw"]["ftol"] == spy["kw"]["gtol"] == 1e-10 and spy["kw"]["method"] == "trf"
    with pytest.raises(ValueError, match="lsq_linear_batch"):
        bounded_lsq.lsq_linear(A, b)


def test_shapes_of_A_and_b(spy):
    A, b = _data()
    with pytest.raises(ValueError, match="`A` must have shape"):
        bounded_lsq.lsq_linear_batch(A[0], b)
    with pytest.raises(ValueError, match="`b` must have shape"):
        bounded_lsq.lsq_linear_batch(A, b[None])
    with pytest.raises(ValueError, match="Inconsistent shapes between `A` and `b`"):
        bounded_lsq.lsq_linear_batch(A, b[:, :5])
    with pytest.raises(ValueError, match="same B"):
        bounded_lsq.lsq_linear_batch(np.stack([A, A]), b)
    with pytest.raises(ValueError, match="empty"):
        bounded_lsq.lsq_linear_batch(A[:, :0], b)
    with pytest.raises(ValueError, match="sigma"):
        bounded_lsq.lsq_linear_batch(A, b, sigma=np.ones(3))
    assert not spy                                            # nothing reached the solver


def test_bounds(spy):
    A, b = _data()
    with pytest.raises(ValueError, match="2 elements"):
        bounded_lsq.lsq_linear_batch(A, b, bounds=(0, 1, 2))
    with pytest.raises(ValueError, match="Inconsistent shapes between bounds and `A`"):
        bounded_lsq.lsq_linear_batch(A, b, bounds=(np.zeros(3), np.ones(4)))
    for lo, hi in ((0.0, 0.0), (np.array([0.0, 1.0, 0.0, 0.0]), np.array([1.0, 0.5, 1.0, 1.0]))):
        with pytest.raises(ValueError, match="strictly less"):
            bounded_lsq.lsq_linear_batch(A, b, bounds=(lo, hi))
    with pytest.raises(Stop):                                 # per-problem bounds (B, n) are taken
        bounded_lsq.lsq_linear_batch(A, b, bounds=(-np.ones((3, 4)), np.ones((3, 1))))
    assert spy["kw"]["bounds"][1].shape == (3, 4)


def test_methods(spy):
    A, b = _data()
    with pytest.raises(ValueError, match="'trf' or 'dogbox'.*'bvls' is not built"):
        bounded_lsq.lsq_linear_batch(A, b, method="bvls")
    with pytest.raises(ValueError, match="'trf' or 'dogbox'"):
        bounded_lsq.lsq_linear_batch(A, b, method="lm")
    with pytest.raises(ValueError, match="driver"):
        bounded_lsq.lsq_linear_batch(A, b, driver="gpu")
    with pytest.raises(ValueError, match="covariance"):
        bounded_lsq.lsq_linear_batch(A, b, covariance="all")
    with pytest.raises(ValueError, match="leverage"):
        bounded_lsq.lsq_linear_batch(A, b, leverage=True)
    assert not spy


def test_x0_outside_the_box_is_the_solver_s_error(monkeypatch):
    """The start goes to ``least_squares_batch`` as given; its own check refuses it before any GPU is touched."""
    A, b = _data()
    with pytest.raises(ValueError, match="`x0` is infeasible"):
        bounded_lsq.lsq_linear_batch(A, b, bounds=(0, 1), x0=np.full(4, 1.5), driver="host")
    with pytest.raises(ValueError, match="`x0` is infeasible"):
        bounded_lsq.lsq_linear_batch(A, b, bounds=(0, 1), x0=np.full(4, 1.5))
    with pytest.raises(ValueError, match="`x0` must have shape"):
        bounded_lsq.lsq_linear_batch(A, b, x0=np.zeros(3))


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_bound_and_exported():
    lib = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blsq.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+blsq_linear_eval_dev\s*\(([^)]*)\)\s*;", src).group(1)
    params = [" ".join(p.replace("*", " * ").split()) for p in proto.split(",")]
    assert params == ["blsq_ctx * ctx", "int B", "int reps", "int m", "int n", "const double * dA", "long A_stride",
                      "const double * dy", "const double * dw", "long w_stride", "const double * dX", "double * df",
                      "double * dJ", "const int32_t * dmask"]
    res, args = _abi.SIGNATURES["blsq_linear_eval_dev"]
    want = {"int": ctypes.c_int, "long": ctypes.c_long}
    assert res is ctypes.c_int and args == [_abi.vp] + [want.get(p.split()[0], _abi.vp) for p in params[1:]]
    assert hasattr(lib, "blsq_linear_eval_dev")
    assert "blsq_linear_eval_dev" not in _abi.MODEL_EVAL_ARGS  # no model, no table: not a row of the model entries


def test_a_null_context_is_argument_one():
    """Without a device there is no context, and an entry reports every other argument through one: the positions 2 to
    13 are held on the GPU (test_lsq_linear_gpu.py::test_bad_arguments_return_their_position)."""
    lib = _abi.load()
    assert lib.blsq_linear_eval_dev(None, 1, 1, 1, 1, None, 0, None, None, 0, None, None, None, None) == -1


# ---- definitions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("sigma", ["none", "scalar", "m", "per"])
def test_numpy_callbacks_against_explicit_loops(shared, sigma):
    B, m, n = 3, 5, 4
    A, b = _data(B, m, n, shared, seed=3)
    rng = np.random.default_rng(4)
    sg = {"none": None, "scalar": 0.5, "m": rng.uniform(0.5, 2, m), "per": rng.uniform(0.5, 2, (B, m))}[sigma]
    X = rng.standard_normal((B, n))
    fun, jac = _linear.numpy_callbacks(A, b, sg)
    F, J = fun(X), jac(X)
    assert F.shape == (B, m) and J.shape == (B, m, n)
    for p in range(B):
        Ap = A if shared else A[p]
        for i in range(m):
            w = 1.0 if sg is None else 1.0 / np.broadcast_to(sg, (B, m))[p, i]
            s = sum(float(Ap[i, j]) * float(X[p, j]) for j in range(n))
            assert abs(F[p, i] - w * (s - b[p, i])) <= 8 * EPS * w * (np.abs(Ap[i]) @ np.abs(X[p]) + abs(b[p, i]))
            for j in range(n):
                assert J[p, i, j] == w * Ap[i, j]             # one multiply (none without sigma)
    assert jac(X + 1.0) is J or np.array_equal(jac(X + 1.0), J)  # constant


def test_initialize_feasible_is_one_function_in_both_modules():
    assert _curve_fit._initialize_feasible is _hostmath._initialize_feasible is _linear._initialize_feasible
    lb = np.array([[-np.inf, 0.0, -np.inf, 2.0], [1.0, -3.0, -np.inf, -np.inf]])
    ub = np.array([[np.inf, np.inf, 4.0, 6.0], [np.inf, 5.0, -2.0, np.inf]])
    want = np.array([[1.0, 1.0, 3.0, 4.0], [2.0, 1.0, -3.0, 1.0]])
    assert np.array_equal(_hostmath._initialize_feasible(lb, ub), want)
    assert np.array_equal(_curve_fit._initialize_feasible(lb[0], ub[0]), want[0])


# ---- the fit cases of the GPU tests ---------------------------------------------------------------------------------
def _scipy_solutions(case, p):
    """x* by BVLS, and scipy's TRF on the linear residual from the case's start."""
    A = lc.problem_matrix(case, p)
    ref = optimize.lsq_linear(A, case["b"][p], bounds=(case["lb"][p], case["ub"][p]), method="bvls", tol=1e-14)
    assert ref.status > 0
    run = optimize.least_squares(lambda x: A @ x - case["b"][p], case["x0"][p], jac=lambda x: A,
                                 bounds=(case["lb"][p], case["ub"][p]), method="trf", ftol=None, xtol=None, gtol=1e-10)
    return ref, run


@pytest.mark.parametrize("name", list(lc.FIT_CASES))
def test_fit_cases_are_solved_by_scipy_well_inside_the_margin(name):
    case = lc.get(name)
    m, n, B = case["m"], case["n"], case["B"]
    assert np.all((case["x0"] > case["lb"]) & (case["x0"] < case["ub"]))
    for p in range(B):
        A = lc.problem_matrix(case, p)
        s = np.linalg.svd(A, compute_uv=False)
        assert s[0] / s[-1] <= 100.0
        ref, run = _scipy_solutions(case, p)
        xs = ref.x
        np.testing.assert_allclose(xs, case["xstar"][p], rtol=1e-9, atol=1e-12)      # the construction holds
        assert run.status == 1
        np.testing.assert_allclose(run.x, xs, rtol=1e-6, atol=1e-9)
        # strictly active: on the bound with a multiplier of the right sign and |g_j| >= 1; at least one, at most half
        g = A.T @ (A @ xs - case["b"][p])
        act = np.where(xs == case["lb"][p], -1, 0) + np.where(xs == case["ub"][p], 1, 0)
        assert np.array_equal(act, case["active"][p])
        k = np.count_nonzero(act)
        assert 1 <= k <= n // 2
        assert np.all(-act[act != 0] * g[act != 0] >= 1.0 - 1e-9) and np.all(np.abs(g[act == 0]) < 1e-9)
        free = act == 0
        assert np.all(np.minimum(xs - case["lb"][p], case["ub"][p] - xs)[free] > 0.2)
        # what keeps the status at 1 under gtol = ftol (tests/_linear_cases.py): an objective below 1
        r = A @ xs - case["b"][p]
        assert r @ r < 1.0


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", list(lc.FIT_CASES))
def test_scipy_ends_on_the_gradient_tolerance_with_the_tolerances_lsq_linear_sets(name, method):
    """The drivers of this package are scipy's; with gtol = ftol = 1e-10 and xtol = eps scipy's reach status 1 and x* on
    every case, which is what the GPU tests then ask of the device.  (dogbox can stall on a draw: _linear_cases.py.)"""
    case = lc.get(name)
    for p in range(case["B"]):
        A = lc.problem_matrix(case, p)
        run = optimize.least_squares(lambda x: A @ x - case["b"][p], case["x0"][p], jac=lambda x: A,
                                     bounds=(case["lb"][p], case["ub"][p]), method=method, ftol=1e-10, xtol=EPS,
                                     gtol=1e-10)
        assert run.status == 1, (name, p, run.status)
        np.testing.assert_allclose(run.x, case["xstar"][p], rtol=1e-6, atol=1e-9)


def test_nnls_and_unbounded_cases():
    c = lc.nnls_case()
    x, _ = optimize.nnls(c["A"], c["b"])
    np.testing.assert_allclose(x, c["xstar"], rtol=1e-9, atol=1e-12)
    assert np.count_nonzero(x == 0.0) == 2
    s = np.linalg.svd(c["A"], compute_uv=False)
    assert s[0] / s[-1] <= 100.0 and np.all(c["A"] >= 0)
    u = lc.fit_case(40, 6, 4, True, 201, unbounded=True)
    for p in range(4):
        x = np.linalg.lstsq(u["A"], u["b"][p], rcond=None)[0]
        np.testing.assert_allclose(x, u["xstar"][p], rtol=1e-9, atol=1e-12)
