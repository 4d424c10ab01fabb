"""CPU-side checks of the pseudo-inverse covariance: the reference of tests/_pinv_ref.py checks itself, the gap
assertion fires, 'pinv' / 'free-pinv' and `pinv=` are validated before any GPU is touched, and the C-ABI carries the
three new entries."""
import os
import re

import numpy as np
import pytest

import _cov_ref as ref
import _pinv_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
PINV_ENTRIES = {"blsq_cov_pinv_dev": 9, "blsq_cov_pinv": 9, "blsq_outer_covariance_pinv": 8}


def _no_gpu(*a, **k):
    raise AssertionError("the GPU was touched before the arguments were validated")


# ---- the reference -------------------------------------------------------------------------------
def test_reference_small_checks_itself_on_the_rank_deficient_cases():
    for J, rank in ((pref.duplicated_column(11, 64, 8), 7), (pref.dependent_column(12), 17), (pref.wide(13), 6)):
        r = pref.reference_small(J)                       # (asserts 100x finer than the recipe, and the gap)
        assert r["rank"] == rank and r["zero"] == []
        assert r["err_reference"] * 100 <= r["err_recipe"]
        assert r["bound"] == max(4 * r["err_recipe"], 8 * J.shape[1] * EPS)
        # scipy's float64 recipe meets the bound it sets, with its own rank
        C = ref.svd_recipe(J)
        pref.check((C + C.T) / 2, r, "recipe")
        # Moore-Penrose: G C* G = G up to the dropped part
        G = J.T @ J
        Cs = np.asarray(r["C"], dtype=float)
        assert np.max(np.abs(G @ Cs @ G - G)) <= 1e-10 * np.max(np.abs(G))


def test_reference_small_zero_column_and_closed_form():
    J = pref.zero_column(14)
    r = pref.reference_small(J)
    assert r["rank"] == 4 and r["zero"] == [2]
    C = np.asarray(r["C"], dtype=float)
    assert np.all(C[2] == 0.0) and np.all(C[:, 2] == 0.0)
    with pytest.raises(AssertionError):                   # a result that is not exactly zero there is refused
        bad = C.copy()
        bad[2, 2] = 1e-300
        pref.check(bad, r)
    # diag(d) padded with a zero column: C* = diag(1 / d^2, 0)
    d = np.array([0.5, 2.0, 3.0])
    J = np.zeros((7, 4))
    J[:3, :3] = np.diag(d)
    r = pref.reference_small(J)
    assert r["rank"] == 3
    assert np.allclose(np.diag(np.asarray(r["C"], dtype=float)), [4.0, 0.25, 1 / 9.0, 0.0], rtol=4 * EPS, atol=0)
    # full rank: the pseudo-inverse reference is the inverse reference
    J = ref.make_jacobian(np.random.default_rng(1), 60, 6, 20.0)
    a, b = pref.reference_small(J), ref.reference(J)
    assert a["rank"] == 6 and ref.cov_error(a["C"], b["C"]) < 1e-17


def test_doubled_reference_is_the_pseudo_inverse():
    J, r = pref.doubled_case(5, 96, 10)
    assert J.shape == (96, 20) and r["rank"] == 10
    small = pref.reference_small(J)                        # the mpmath route on the same matrix
    assert small["rank"] == 10
    assert ref.cov_error(r["C"], small["C"]) < 1e-16
    assert r["err_recipe"] < 1e-13


def test_gap_assertion_fires():
    rng = np.random.default_rng(2)
    U, _ = np.linalg.qr(rng.standard_normal((50, 6)))
    V, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    thr = EPS * 50
    for s_last in (thr * 3.0, thr / 3.0, thr * 50.0):
        J = (U * np.array([1.0, 0.5, 0.3, 0.2, 0.1, s_last])) @ V.T
        with pytest.raises(pref.GapError):
            pref.reference_small(J)
    J = (U * np.array([1.0, 0.5, 0.3, 0.2, 0.1, 1e-6])) @ V.T      # far above: accepted, full rank
    assert pref.reference_small(J)["rank"] == 6
    with pytest.raises(pref.GapError):
        pref.assert_gap([1.0, 1e-13], 1e-14)
    pref.assert_gap([1.0, 1e-11, 1e-17, 0.0], 1e-14)


# ---- argument validation -------------------------------------------------------------------------
def test_pinv_modes_are_accepted_and_the_old_rejections_stay():
    from bounded_lsq._cov import check_covariance, is_pinv, is_free
    assert check_covariance('pinv') == 'pinv' and check_covariance('free-pinv') == 'free-pinv'
    assert is_pinv('pinv') and is_pinv('free-pinv') and not is_pinv(True) and not is_pinv('free')
    assert is_free('free') and is_free('free-pinv') and not is_free('pinv') and not is_free(True)
    for bad in ("full", "True", 2, None, 1.0, [True], "Free", "Pinv", "pinv-free", "free_pinv"):
        with pytest.raises(ValueError, match="`covariance` must be False, True or 'free'") as e:
            check_covariance(bad)
        assert "'pinv'" in str(e.value) and "'free-pinv'" in str(e.value)


@pytest.mark.parametrize("bad", ["Pinv", "pinv-free", "pseudo"])
def test_front_ends_validate_before_the_gpu(bad, monkeypatch):
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
    for driver in ('host', 'device'):
        with pytest.raises(ValueError, match="`covariance` must be False, True or 'free'"):
            bounded_lsq.least_squares_batch(fun, np.zeros((2, 1)), lambda X: np.ones((2, 1, 1)), covariance=bad,
                                            driver=driver)
    assert not calls


def test_covariance_function_validates_pinv_and_scale_before_the_gpu(monkeypatch):
    import bounded_lsq
    from bounded_lsq import _abi, _hip_step
    monkeypatch.setattr(_abi, "Context", _no_gpu)
    monkeypatch.setattr(_hip_step, "default_context", _no_gpu)
    J = np.ones((5, 3))
    for bad in ("yes", 1, None, 'pinv'):
        with pytest.raises(ValueError, match="`pinv` must be False or True"):
            bounded_lsq.covariance(J, pinv=bad)
    with pytest.raises(ValueError, match="`scale` needs pinv=True"):
        bounded_lsq.covariance(J, scale=2.0)
    with pytest.raises(ValueError, match="`scale` must be a scalar or have shape"):
        bounded_lsq.covariance(np.ones((2, 5, 3)), pinv=True, scale=np.ones(3))
    with pytest.raises(ValueError):
        bounded_lsq.covariance(np.zeros(3), pinv=True)
    with pytest.raises(ValueError):
        bounded_lsq.covariance(J, active_mask=np.zeros(4, dtype=int), pinv=True)


def test_outer_driver_signature():
    import inspect
    from bounded_lsq import OuterDriver
    sig = inspect.signature(OuterDriver.covariance)
    assert list(sig.parameters)[1:] == ["free_only", "pinv", "variance_scale"]
    assert all(sig.parameters[k].default is False for k in ("free_only", "pinv", "variance_scale"))


# ---- the C-ABI -----------------------------------------------------------------------------------
def test_header_and_binding_carry_the_three_entries():
    import ctypes as C
    from bounded_lsq import _abi
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _abi.load()
    for name, nargs in PINV_ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, "not declared in include/blsq.h: " + name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == nargs
        assert name in _abi.SIGNATURES, "not bound in _abi.py: " + name
        assert len(_abi.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name), "missing export: " + name
    assert _abi.SIGNATURES["blsq_outer_covariance_pinv"][1][1:3] == [C.c_int, C.c_int]


def test_timing_slots_of_the_pinv_kernels():
    src = open(os.path.join(ROOT, "bounded-lsq_amd", "csrc", "blsq_host.h")).read()
    names = re.search(r"kSlotNames\[K_NSLOT\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    names = re.findall(r'"([a-z0-9_]+)"', names)
    i = names.index("cov_gather")
    assert names[i - 2:i] == ["cov_pinv_weights", "cov_pinv_product"]
    enum = re.search(r"enum Slot \{(.*?)\};", src, flags=re.S).group(1)
    ids = re.findall(r"\bK_[A-Z0-9_]+", enum)
    assert ids.index("K_COV_PINV_WEIGHTS") == names.index("cov_pinv_weights")
    assert ids.index("K_COV_PINV_PRODUCT") == names.index("cov_pinv_product")
