"""CPU-side checks of the covariance feature: argument validation before any GPU is touched, the C-ABI entries and
their binding, and the extended-precision reference of tests/_cov_ref.py (closed forms, curve_fit's recipe)."""
import os
import re

import numpy as np
import pytest

import _cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
COV_ENTRIES = ["blsq_cov", "blsq_cov_dev", "blsq_cov_plan_create", "blsq_cov_plan_destroy", "blsq_outer_covariance"]


def _no_gpu(*a, **k):
    raise AssertionError("the GPU was touched before `covariance` was validated")


@pytest.mark.parametrize("bad", ["full", "True", 2, None, 1.0, [True], "Free"])
def test_covariance_argument_is_validated_before_the_gpu(bad, monkeypatch):
    import bounded_lsq
    from bounded_lsq import _abi, _hip_step
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)
    calls = []

    def fun(x):
        calls.append(1)
        return np.atleast_1d(x) - 1.0

    with pytest.raises(ValueError, match="`covariance` must be False, True or 'free'"):
        bounded_lsq.least_squares(fun, [0.5], covariance=bad)
    with pytest.raises(ValueError, match="`covariance` must be False, True or 'free'"):
        bounded_lsq.least_squares_batch(fun, np.zeros((2, 1)), lambda X: np.ones((2, 1, 1)), covariance=bad)
    with pytest.raises(ValueError, match="`covariance` must be False, True or 'free'"):
        bounded_lsq.least_squares_batch(fun, np.zeros((2, 1)), lambda X: np.ones((2, 1, 1)), covariance=bad,
                                        driver='device')
    assert not calls


def test_covariance_accepts_its_three_values():
    from bounded_lsq._cov import check_covariance
    assert check_covariance(False) is False and check_covariance(True) is True
    assert check_covariance(np.bool_(True)) is True
    assert check_covariance('free') == 'free'


def test_covariance_function_checks_shapes_before_the_gpu(monkeypatch):
    import bounded_lsq
    from bounded_lsq import _abi, _hip_step
    assert "covariance" in bounded_lsq.__all__
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)
    with pytest.raises(ValueError):
        bounded_lsq.covariance(np.zeros(3))
    with pytest.raises(ValueError):
        bounded_lsq.covariance(np.zeros((2, 3, 4, 5)))
    with pytest.raises(ValueError):
        bounded_lsq.covariance(np.ones((5, 3)), active_mask=np.zeros(4, dtype=int))
    with pytest.raises(ValueError):
        bounded_lsq.covariance(np.ones((2, 5, 3)), active_mask=np.zeros((3, 3), dtype=int))


def test_header_and_binding_agree_on_the_covariance_entries():
    from bounded_lsq import _abi
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _abi.load()
    for name in COV_ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, "not declared in include/blsq.h: " + name
        nargs = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _abi.SIGNATURES, "not bound in _abi.py: " + name
        res, args = _abi.SIGNATURES[name]
        assert len(args) == nargs, (name, len(args), nargs)
        assert hasattr(lib, name), "missing export: " + name
    assert "typedef struct blsq_cov_plan blsq_cov_plan;" in src
    # integer arguments are bound as integers: B, m, n of the plan, free_only of the driver call
    import ctypes as C
    assert _abi.SIGNATURES["blsq_cov_plan_create"][1][1:4] == [C.c_int] * 3
    assert _abi.SIGNATURES["blsq_outer_covariance"][1][1] == C.c_int


def test_timing_slots_of_the_covariance_kernels_precede_the_loss_slots():
    # (tests/test_loss_gpu.py pins the loss slots to the end of the table)
    src = open(os.path.join(ROOT, "bounded-lsq_amd", "csrc", "blsq_host.h")).read()
    names = re.search(r"kSlotNames\[K_NSLOT\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    names = re.findall(r'"([a-z0-9_]+)"', names)
    assert names[-5:] == ["cov_gather", "cov_inverse", "cov_product", "loss_cost", "loss_scale"]
    enum = re.search(r"enum Slot \{(.*?)\};", src, flags=re.S).group(1)
    assert len(re.findall(r"\bK_[A-Z0-9_]+", enum)) == len(names) + 1          # (+ K_NSLOT)


# ---- the reference helper ----------------------------------------------------------------------
def test_reference_reproduces_closed_forms():
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((40, 7)))
    # orthonormal in double only up to rounding: the reference must see exactly that, I + O(eps)
    r = ref.reference(Q)
    assert r["kind"] == "mpmath"
    assert ref.cov_error(np.eye(7), r["C"]) < 20 * EPS
    d = np.array([0.5, 2.0, 3.0, 1e-3, 7.0])
    J = np.zeros((9, 5))
    J[:5] = np.diag(d)
    for kind in ("mpmath", "longdouble"):
        r = ref.reference(J, force=kind)
        C = np.asarray(r["C"], dtype=float)
        assert np.array_equal(C != 0, np.eye(5, dtype=bool))
        assert np.allclose(np.diag(C), d ** -2.0, rtol=4 * EPS, atol=0)


def test_reference_agrees_with_curve_fit_recipe_when_well_conditioned():
    rng = np.random.default_rng(1)
    J = ref.make_jacobian(rng, 120, 12, 10.0, column_scales=True)
    r = ref.reference(J)
    assert r["err_reference"] * 100 <= r["err_recipe"] or r["err_reference"] < 1e-40
    assert r["err_recipe"] < 1e-13
    assert r["bound"] == max(4 * r["err_recipe"], 8 * 12 * EPS)
    # and curve_fit itself (absolute_sigma=True) returns the recipe's matrix for a linear model with this Jacobian
    from scipy.optimize import curve_fit
    y = J @ np.ones(12) + 0.01 * rng.standard_normal(120)
    _, pcov = curve_fit(lambda t, *p: J @ np.asarray(p), np.arange(120.0), y, p0=np.zeros(12), sigma=np.ones(120),
                        absolute_sigma=True, jac=lambda t, *p: J)
    assert ref.cov_error(pcov, r["C"]) < 1e-12


def test_both_references_agree_and_the_exact_residual_step_is_exact():
    rng = np.random.default_rng(2)
    J = ref.make_jacobian(rng, 96, 20, 50.0, grid=True)
    a = ref.reference(J, force="mpmath")
    b = ref.reference(J, force="longdouble")
    assert ref.cov_error(b["C"], a["C"]) < 1e-16
    # the Newton-Schulz second evaluation of the large cases, against mpmath: finer than longdouble itself
    C0 = ref.ld_covariance(J)
    C0q, corr = ref.newton_refined(J, C0)
    assert ref.cov_error(C0q + corr, a["C"]) < 1e-18
    # its exact products really are exact
    A = np.array([[3, -5], [1 << 40, 7]], dtype=object)
    B = np.array([[1 << 33, 2], [-9, (1 << 50) + 1]], dtype=object)
    assert np.array_equal(ref._exact_product(A, B, 14, 4, 14, 5), A.dot(B))


def test_squared_conditioning_route_is_refused_by_the_bound():
    # the issue's finding: at kappa ~ 1e6 a Cholesky of the (equilibrated) Gram misses the bound the recipe sets
    rng = np.random.default_rng(3)
    J = ref.make_jacobian(rng, 512, 64, 1e6, column_scales=True)
    r = ref.reference(J)
    d = 1.0 / np.sqrt(np.einsum('ij,ij->j', J, J))
    L = np.linalg.cholesky((J * d).T @ (J * d))
    Y = np.linalg.inv(L)
    Cchol = (Y.T @ Y) * np.outer(d, d)
    assert ref.cov_error(Cchol, r["C"]) > r["bound"]
    Rh = np.linalg.qr(J, mode='r')
    Xh = np.linalg.inv(Rh)
    assert ref.cov_error(Xh @ Xh.T, r["C"]) <= r["bound"]
