"""CPU-side checks of the leverage feature: the references of tests/_lev_ref.py against closed forms, `influence`
against brute force, every ValueError of the new functions (raised before any GPU is touched), and the three new C-ABI
symbols with the place of the `cov_rows` timing slot."""
import os
import re

import numpy as np
import pytest

import _lev_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


# ---- the references ------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", ["mpmath", "longdouble"])
def test_reference_closed_forms(force):
    rng = np.random.default_rng(1)
    # m = n: the hat matrix is the identity
    J = ref.make_jacobian(rng, 12, 12, 1e2)
    r = ref.reference(J, force=force)
    assert r["kind"] == force and float(np.max(np.abs(r["h"] - 1))) <= 1e-15
    # orthonormal columns: h = row sums of squares
    Q, _ = np.linalg.qr(rng.standard_normal((40, 7)))
    r = ref.reference(Q, force=force)
    want = np.sum(Q.astype(ref.LD) ** 2, axis=1)
    assert float(np.max(np.abs(r["h"] - want))) <= 40 * EPS          # (Q is orthonormal to a few eps only)
    # sum h* = n, and the bound rule
    J = ref.make_jacobian(rng, 60, 9, 1e4, column_scales=True)
    r = ref.reference(J, force=force)
    assert abs(float(np.sum(r["h"])) - 9) <= 1e-15 * 60
    assert r["bound"] == max(4 * r["err_recipe"], 8 * 9 * EPS) and r["err_reference"] * 100 <= r["err_recipe"]


def test_reference_rows_of_another_matrix_and_both_recipes():
    rng = np.random.default_rng(2)
    J = ref.make_jacobian(rng, 50, 6, 1e3, column_scales=True)
    A = rng.standard_normal((11, 6))
    r = ref.reference(J, A, recipe=ref.recipe_rows(J, A))
    C = np.linalg.inv(J.T @ J)
    want = np.einsum("ij,jk,ik->i", A, C, A)
    assert np.allclose(np.asarray(r["h"], dtype=float), want, rtol=1e-8, atol=0.0)
    # the two recipes agree with each other on A = J to rounding, and a record serves a second recipe
    base = ref.reference(J)
    again = ref.reference(J, recipe=ref.recipe_rows(J, J), base=base)
    assert np.array_equal(again["h"], base["h"]) and again["err_reference"] == base["err_reference"]
    assert np.allclose(ref.recipe_regular(J), ref.recipe_rows(J, J), rtol=0.0, atol=1e-9)
    # duplicated columns: the leverages of the independent ones
    D = np.hstack([J, J[:, :2]])
    assert np.allclose(ref.recipe_rows(D, D), ref.recipe_regular(J), rtol=0.0, atol=1e-9)


# ---- influence -----------------------------------------------------------------------------------------
def test_influence_against_refitting_without_each_row():
    import bounded_lsq
    rng = np.random.default_rng(3)
    m, p = 30, 4
    J = rng.standard_normal((m, p))
    y = J @ rng.standard_normal(p) + 0.1 * rng.standard_normal(m)
    beta = np.linalg.lstsq(J, y, rcond=None)[0]
    f = J @ beta - y
    h = np.asarray(ref.reference(J)["h"], dtype=float)
    student, cook = bounded_lsq.influence(h, f, p)
    s2 = float(f @ f) / (m - p)
    for i in range(m):
        keep = np.arange(m) != i
        bi = np.linalg.lstsq(J[keep], y[keep], rcond=None)[0]
        d = J @ (beta - bi)
        assert abs(cook[i] - float(d @ d) / (p * s2)) <= 1e-10 * abs(cook[i])
        assert abs(student[i] - f[i] / np.sqrt(s2 * (1 - h[i]))) <= 1e-10 * abs(student[i])
    # batched, and IEEE at h = 1: no warning, no exception
    sb, cb = bounded_lsq.influence(np.stack([h, h]), np.stack([f, 2 * f]), np.array([p, p]))
    assert np.array_equal(sb[0], student) and np.allclose(cb[1], cook, rtol=1e-14, atol=0.0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s1, c1 = bounded_lsq.influence(np.array([1.0, 0.5, 0.5]), np.array([0.0, 1.0, -1.0]), 1)
    assert np.isnan(s1[0]) and np.isnan(c1[0]) and np.all(np.isfinite(s1[1:]))
    with pytest.raises(ValueError):
        bounded_lsq.influence(np.ones(3), np.ones(4), 1)
    with pytest.raises(ValueError):
        bounded_lsq.influence(np.ones((2, 3)), np.ones((2, 3)), np.ones(3))


# ---- argument errors, no GPU ------------------------------------------------------------------------------
def test_value_errors_are_raised_before_any_gpu_is_touched(monkeypatch):
    import bounded_lsq
    from bounded_lsq import _abi

    def no_gpu(*a, **k):
        raise AssertionError("the GPU must not be touched")
    monkeypatch.setattr(_abi, "Context", no_gpu)
    monkeypatch.setattr(_abi, "load", no_gpu)
    J = np.ones((6, 3))
    bad = [
        lambda: bounded_lsq.leverage(np.ones(6)),                                   # bad ndim
        lambda: bounded_lsq.leverage(np.ones((1, 2, 3, 4))),
        lambda: bounded_lsq.leverage(np.ones((0, 3))),                              # empty J
        lambda: bounded_lsq.leverage(np.ones((2, 6, 0))),
        lambda: bounded_lsq.leverage(J, np.zeros(4)),                               # bad mask shape
        lambda: bounded_lsq.leverage(np.ones((2, 6, 3)), np.zeros(3)),
        lambda: bounded_lsq.leverage(J, pinv=1),                                    # non-bool pinv
        lambda: bounded_lsq.leverage(J, pinv="yes"),
        lambda: bounded_lsq.prediction_variance(np.ones(6), J),
        lambda: bounded_lsq.prediction_variance(np.ones((0, 3)), J),
        lambda: bounded_lsq.prediction_variance(J, np.ones((4, 2))),                # J_new whose n differs
        lambda: bounded_lsq.prediction_variance(J, np.ones((1, 4, 3))),             # 3-D J_new for a single J
        lambda: bounded_lsq.prediction_variance(np.ones((2, 6, 3)), np.ones((3, 4, 3))),    # J_new whose B differs
        lambda: bounded_lsq.prediction_variance(np.ones((2, 6, 3)), np.ones((2, 4, 5))),
        lambda: bounded_lsq.prediction_variance(J, np.ones(3)),
        lambda: bounded_lsq.prediction_variance(J, np.ones((0, 3))),
        lambda: bounded_lsq.prediction_variance(J, J, np.zeros((2, 3))),            # bad mask shape
        lambda: bounded_lsq.prediction_variance(J, J, scale=np.ones(2)),            # bad scale shape
        lambda: bounded_lsq.prediction_variance(np.ones((2, 6, 3)), J, scale=np.ones(3)),
        lambda: bounded_lsq.prediction_variance(J, J, pinv=0),                      # non-bool pinv
        lambda: bounded_lsq.least_squares(lambda x: x, [1.0], leverage=True),        # leverage without a covariance mode
        lambda: bounded_lsq.least_squares(lambda x: x, [1.0], covariance=False, leverage=True),
        lambda: bounded_lsq.least_squares(lambda x: x, [1.0], covariance=True, leverage=1),
        lambda: bounded_lsq.least_squares_batch(lambda X: X, [[1.0]], lambda X: X[:, :, None], covariance=False,
                                                leverage=True),
        lambda: bounded_lsq.least_squares_batch(lambda X: X, [[1.0]], lambda X: X[:, :, None], leverage=True),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d did not raise" % k)


# ---- C-ABI ------------------------------------------------------------------------------------------------
NEW = {"blsq_cov_rows_dev": 5, "blsq_cov_rows": 5, "blsq_outer_leverage": 3}


def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C
    from bounded_lsq import _abi
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _abi.load()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src)
        assert decl, "not declared: " + name
        assert len(decl.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), "not exported: " + name
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    for name in ("blsq_cov_rows_dev", "blsq_cov_rows"):
        assert _abi.SIGNATURES[name][1][1] is C.c_int, "`rows` is an int"
        assert all(a is _abi.vp for k, a in enumerate(_abi.SIGNATURES[name][1]) if k != 1)
    assert all(a is _abi.vp for a in _abi.SIGNATURES["blsq_outer_leverage"][1])
    for mod, names in (("_leverage", ("leverage", "prediction_variance", "influence")),):
        import bounded_lsq
        for nm in names:
            assert getattr(bounded_lsq, nm) is getattr(getattr(bounded_lsq, mod), nm) and nm in bounded_lsq.__all__


def test_timing_slot_sits_directly_after_csne_fix():
    src = open(os.path.join(ROOT, "bounded-lsq_amd", "csrc", "blsq_host.h")).read()
    ids = [s.strip() for s in re.search(r"enum Slot \{(.*?)\};", src, flags=re.S).group(1).split(",")]
    ids = [re.sub(r"\s*=.*", "", s) for s in ids if s]
    names = re.findall(r'"([a-z0-9_]+)"', re.search(r"kSlotNames\[K_NSLOT\] = \{(.*?)\};", src, flags=re.S).group(1))
    assert len(names) == len(ids) - 1 and ids[-1] == "K_NSLOT"
    i = names.index("cov_rows")
    assert names[i - 1] == "csne_fix" and names[i + 1] == "cov_pinv_weights"
    assert ids.index("K_COV_ROWS") == i and ids[i - 1] == "K_CSNE_FIX"
