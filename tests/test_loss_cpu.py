"""Robust loss functions (`loss=`, `f_scale=` of scipy.optimize.least_squares) without a GPU: argument checks and their
order, the numpy restatement in _hostmath against scipy bit for bit, and the C-ABI entries."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_MSG = ("`loss` must be one of dict_keys(['linear', 'huber', 'soft_l1', 'cauchy', 'arctan']) "
            "or a callable.")


def _never(*a, **k):
    raise AssertionError("a callback ran before the arguments were checked")


# ---- least_squares ---------------------------------------------------------------------------------------------
def test_least_squares_rejects_an_unknown_loss_with_scipys_message():
    from bounded_lsq import least_squares
    with pytest.raises(ValueError) as e:
        least_squares(_never, [1.0], _never, loss='l1')
    assert str(e.value) == LOSS_MSG
    # scipy's message, word for word
    from scipy.optimize._lsq.least_squares import IMPLEMENTED_LOSSES
    assert LOSS_MSG == "`loss` must be one of {0} or a callable.".format(IMPLEMENTED_LOSSES.keys())


@pytest.mark.parametrize("f_scale", [0.0, -1.0, np.nan])
def test_least_squares_rejects_a_non_positive_f_scale(f_scale):
    from bounded_lsq import least_squares
    with pytest.raises(ValueError, match=r"^`f_scale` must be positive\.$"):
        least_squares(_never, [1.0], _never, loss='huber', f_scale=f_scale)


def test_least_squares_check_order():
    from bounded_lsq import least_squares
    # the method check comes first ...
    with pytest.raises(ValueError, match="`method` must be"):
        least_squares(_never, [1.0], _never, method='newton', loss='l1', f_scale=0.0)
    # ... then the loss, then f_scale, and both before every other check
    with pytest.raises(ValueError) as e:
        least_squares(_never, [1.0], _never, loss='l1', f_scale=0.0, bounds=(1, 2, 3))
    assert str(e.value) == LOSS_MSG
    with pytest.raises(ValueError, match="`f_scale` must be positive"):
        least_squares(_never, [1.0], _never, loss='cauchy', f_scale=0.0, bounds=(1, 2, 3))
    with pytest.raises(ValueError) as e:
        least_squares(_never, [1.0], _never, method='lm', loss='l1')
    assert str(e.value) == LOSS_MSG
    with pytest.raises(NotImplementedError):
        least_squares(_never, [1.0], _never, method='lm', loss='soft_l1')


# ---- least_squares_batch -----------------------------------------------------------------------------------------
def test_batch_rejects_an_unknown_loss_and_f_scale():
    from bounded_lsq import least_squares_batch
    X0 = np.ones((3, 2))
    with pytest.raises(ValueError, match="`method` must be"):
        least_squares_batch(_never, X0, _never, method='lm', loss='l1')
    with pytest.raises(ValueError) as e:
        least_squares_batch(_never, X0, _never, loss='l1', f_scale=-1.0)
    assert str(e.value) == LOSS_MSG
    for fs in (0.0, [1.0, 0.0, 2.0], np.array([1.0, np.nan, 1.0])):
        with pytest.raises(ValueError, match=r"^`f_scale` must be positive\.$"):
            least_squares_batch(_never, X0, _never, loss='huber', f_scale=fs)
    for fs in ([1.0, 2.0], np.ones((3, 2)), np.ones(4)):
        with pytest.raises(ValueError, match=r"^`f_scale` must be a scalar or broadcastable to \(B,\)\.$"):
            least_squares_batch(_never, X0, _never, loss='huber', f_scale=fs)
    # the f_scale shape is checked before the bounds
    with pytest.raises(ValueError, match="broadcastable to"):
        least_squares_batch(_never, X0, _never, loss='huber', f_scale=[1.0, 2.0], bounds=(1.0, 0.0))


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_batch_rejects_a_callable_loss_on_the_device_driver(method):
    from bounded_lsq import least_squares_batch

    def my_loss(z):
        return np.vstack([z, np.ones_like(z), np.zeros_like(z)])
    with pytest.raises(ValueError, match="callable `loss`.*driver='host'"):
        least_squares_batch(_never, np.ones((2, 2)), _never, method=method, loss=my_loss, driver='device')
    with pytest.raises(ValueError, match="callable `loss`"):          # before the FD Jacobian's context too
        least_squares_batch(_never, np.ones((2, 2)), '2-point', method=method, loss=my_loss, driver='device')


def test_outer_driver_set_loss_rejects_unknown_names():
    from bounded_lsq._outer import OuterDriver
    drv = object.__new__(OuterDriver)
    drv.B = 2
    with pytest.raises(ValueError) as e:
        drv.set_loss('l2')
    assert str(e.value) == LOSS_MSG


# ---- numpy restatement against scipy, bit for bit ------------------------------------------------------------------
def _residuals(f_scale):
    base = [0.0, -0.0, 1e-150, -1e-150, 1e-300, 1e150, -1e150, 1e-8, 0.3, -0.3, 1.0, -1.0, 2.5, -7.0, 1e5,
            -1e10, 123.456, np.nan, np.inf, -np.inf]
    rng = np.random.default_rng(5)
    edge = [f_scale, -f_scale, np.nextafter(f_scale, 0), np.nextafter(f_scale, 10)]   # z = 1 and its neighbours
    return np.array(base + edge + list(rng.standard_normal(40) * 10.0 ** rng.integers(-150, 150, 40)))


@pytest.mark.parametrize("loss", ['huber', 'soft_l1', 'cauchy', 'arctan'])
@pytest.mark.parametrize("f_scale", [0.1, 1.0, 7.0])
def test_hostmath_rho_and_scaling_equal_scipys_bit_for_bit(loss, f_scale):
    from scipy.optimize._lsq.least_squares import construct_loss_function
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from bounded_lsq import _hostmath as H
    f = _residuals(f_scale)
    m = f.size
    with np.errstate(all='ignore'):
        lf = construct_loss_function(m, loss, f_scale)
        rho_ref = lf(f.copy()).copy()
        cost_ref = lf(f.copy(), cost_only=True)
        J = np.random.default_rng(1).standard_normal((m, 5))
        J_ref, f_ref = scale_for_robust_loss_function(J.copy(), f.copy(), rho_ref.copy())
    rho = H.loss_rho(loss, f, f_scale)
    assert rho.shape == (3, m)
    np.testing.assert_array_equal(rho, rho_ref)                       # NaN where scipy has NaN, same values elsewhere
    fin = np.isfinite(rho_ref)
    assert rho[fin].tobytes() == rho_ref[fin].tobytes()               # ... and the same bits (signed zeros included)
    J_s, f_s = H.loss_scale(J, f, rho)
    np.testing.assert_array_equal(J_s, J_ref)
    np.testing.assert_array_equal(f_s, f_ref)
    fin = np.isfinite(f)                                              # the cost, without the non-finite entries too
    with np.errstate(all='ignore'):
        cost_fin = construct_loss_function(int(fin.sum()), loss, f_scale)(f[fin].copy(), cost_only=True)
    assert H.loss_cost(loss, f[fin], f_scale) == 2.0 * cost_fin       # the library's objective: 2 x scipy's cost
    assert np.isnan(H.loss_cost(loss, f, f_scale)) == np.isnan(cost_ref)


def test_hostmath_huber_switches_at_z_equal_one_inclusive():
    from bounded_lsq import _hostmath as H
    rho = H.loss_rho('huber', np.array([2.0, np.nextafter(2.0, 3.0)]), 2.0)     # z = 1 exactly, then just above
    assert rho[1, 0] == 1.0 and rho[2, 0] == 0.0
    assert rho[1, 1] < 1.0 and rho[2, 1] < 0.0


def test_hostmath_callable_loss_matches_scipy():
    from scipy.optimize._lsq.least_squares import construct_loss_function
    from bounded_lsq import _hostmath as H

    def my_loss(z):
        return np.vstack([np.log1p(z) * 2, 2 / (1 + z), -2 / (1 + z) ** 2])
    f = np.linspace(-5, 5, 11)
    ref = construct_loss_function(f.size, my_loss, 3.0)(f.copy())
    np.testing.assert_array_equal(H.loss_rho(my_loss, f, 3.0), ref)
    assert H.loss_cost(my_loss, f, 3.0) == 2 * construct_loss_function(f.size, my_loss, 3.0)(f, cost_only=True)


def test_hostmath_linear_is_sum_of_squares():
    from bounded_lsq import _hostmath as H
    f = np.random.default_rng(2).standard_normal(33)
    J = np.random.default_rng(3).standard_normal((33, 4))
    rho = H.loss_rho('linear', f, 1.0)
    np.testing.assert_array_equal(rho[0], f ** 2)
    J_s, f_s = H.loss_scale(J, f, rho)
    np.testing.assert_array_equal(J_s, J)
    np.testing.assert_array_equal(f_s, f)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_table_list_the_loss_entries():
    from bounded_lsq import _abi
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    for name in ("blsq_loss_cost_dev", "blsq_loss_scale_dev", "blsq_outer_set_loss"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _abi.SIGNATURES, name
        assert hasattr(_abi.load(), name), name
    enum = re.search(r"enum\s*\{\s*(BLSQ_LOSS_LINEAR[^}]*)\}", src).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    assert names == ["BLSQ_LOSS_LINEAR", "BLSQ_LOSS_HUBER", "BLSQ_LOSS_SOFT_L1", "BLSQ_LOSS_CAUCHY",
                     "BLSQ_LOSS_ARCTAN"]
    assert "BLSQ_LOSS_LINEAR = 0" in enum
    from bounded_lsq._hostmath import LOSSES
    assert [("BLSQ_LOSS_" + n.upper()) for n in LOSSES] == names


def test_loss_is_an_argument_not_a_switch():
    from bounded_lsq import _abi
    lib = _abi.load()
    import ctypes as C
    for i in range(lib.blsq_option_count()):
        nm, ev, doc = C.c_char_p(), C.c_char_p(), C.c_char_p()
        df = C.c_double(0.0)
        lib.blsq_option_info(i, C.byref(nm), C.byref(ev), C.byref(df), C.byref(doc))
        assert b"loss" not in nm.value.lower()
