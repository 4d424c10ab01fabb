"""Separable fits on the CPU: the structure tables, the numpy definition of the projection against itself
in np.longdouble, the gradient identity of Kaufman's Jacobian, a scipy solve over the reduced problem, and the errors
of the front end that need no device.  tests/test_separable_gpu.py holds the kernel and the fits to the same cases."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import bounded_lsq
from bounded_lsq import models

import _separable_cases as sc

LD = np.longdouble


# ---- linear_params ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, lin, owner", [
    ("gauss*1", [0], [-1, 0, 0]),
    ("lorentz*2", [0, 3], [-1, 0, 0, -1, 1, 1]),
    ("pvoigt*1", [0], [-1, 0, 0, 0]),
    ("exp*2", [0, 2], [-1, 0, -1, 1]),
    ("gauss+poly*2", [0, 3, 4], [-1, 0, 0, -1, -1]),
    ("poly*2+exp", [0, 1, 2], [-1, -1, -1, 2]),
    ("gauss*2+lorentz+pvoigt+exp+poly*3", [0, 3, 6, 9, 13, 15, 16, 17],
     [-1, 0, 0, -1, 1, 1, -1, 2, 2, -1, 3, 3, 3, -1, 4, -1, -1, -1]),
])
def test_linear_params_composites(spec, lin, owner):
    for model in (spec, models.compose(spec), models.binned(spec)):
        got_lin, got_owner = models.linear_params(model)
        assert got_lin.dtype == np.int32 and got_owner.dtype == np.int32
        assert got_lin.tolist() == lin and got_owner.tolist() == owner


@pytest.mark.parametrize("name, n, lin, owner", [
    ("exp_sum", 5, [0, 2, 4], [-1, 0, -1, 1, -1]),
    ("gauss_sum", 7, [0, 3, 6], [-1, 0, 0, -1, 1, 1, -1]),
    ("lorentz_sum", 4, [0, 3], [-1, 0, 0, -1]),
    ("gauss2d", 5, [0, 4], [-1, 0, 0, 0, -1]),
])
def test_linear_params_named(name, n, lin, owner):
    got_lin, got_owner = models.linear_params(name, n)
    assert got_lin.tolist() == lin and got_owner.tolist() == owner
    # the columns `lin` names do not depend on the linear parameters, and the others scale with their owner
    rng = np.random.default_rng(3)
    M = models.get(name)
    x = rng.uniform(-1, 1, (2, 9)) if M.coords == 2 else np.linspace(0.1, 2.0, 9)
    P = rng.uniform(0.5, 1.5, (1, n))
    P1 = P.copy()
    P1[:, lin] = 1.0
    J, J1 = M.jac(x, P), M.jac(x, P1)
    scale = np.where(np.asarray(owner) < 0, 1.0, P[0, np.asarray(lin)[np.maximum(owner, 0)]])
    np.testing.assert_allclose(J, J1 * scale, rtol=1e-13, atol=0)


def test_linear_params_needs_n():
    assert models.linear_params("gauss2d")[0].tolist() == [0, 4]
    with pytest.raises(ValueError, match="needs `n`"):
        models.linear_params("exp_sum")
    with pytest.raises(ValueError, match="does not take n = 4"):
        models.linear_params("exp_sum", 4)


def test_linear_params_errors():
    with pytest.raises(ValueError, match="structure of a formula is not known"):
        models.linear_params(models.expression("a*exp(-t/tau)+c", ("a", "tau", "c")))
    for model, n in (("poly", 3), ("poly*4", None), ("poly*2+poly*1", None)):
        with pytest.raises(ValueError, match="use `lsq_linear`"):
            models.linear_params(model, n)
    assert models.VARPRO_MAX_NL == 16
    assert models.linear_params("exp*15+poly*1")[0].size == 16
    with pytest.raises(ValueError, match="17 linear parameters, more than VARPRO_MAX_NL = 16"):
        models.linear_params("exp*15+poly*2")


def test_varpro_expand():
    X = np.arange(1.0, 7.0).reshape(2, 3)
    P = models.varpro_expand(X, [1, 3], 5)
    assert P.tolist() == [[1.0, 1.0, 2.0, 1.0, 3.0], [4.0, 1.0, 5.0, 1.0, 6.0]]
    assert models.varpro_expand(X[0].astype(LD), [0], 4).dtype == LD
    with pytest.raises(ValueError, match="n - nl = 2"):
        models.varpro_expand(X, [1, 3], 4)


# ---- varpro_reduce ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wform", sc.WFORMS)
@pytest.mark.parametrize("shape", sc.GRID + (sc.ILL + (True,),), ids=str)
def test_reduce_float64_against_longdouble(shape, wform):
    cs, ref = sc.case(*shape), sc.reference(*shape[:3], wform, *shape[3:])
    f, J, c, info = models.varpro_reduce(cs.G, cs.y, cs.ws[wform], cs.lin, cs.owner)
    assert f.dtype == np.float64 and ref[0].dtype == LD
    assert f.shape == (sc.B, cs.m) and J.shape == (sc.B, cs.m, cs.na) and c.shape == (sc.B, cs.nl)
    assert info.dtype == np.int32 and not info.any() and not ref[3].any()
    frac = sc.fractions(cs, wform, ref, f, J, c)
    print(shape, wform, "kappa %.3g" % cs.kappa(wform).max(), frac)
    assert max(frac.values()) <= 1.0, frac


def test_ill_conditioned_case_is_ill_conditioned_and_needs_the_correction():
    cs = sc.case(*sc.ILL, True)
    kappa = cs.kappa("none")
    assert np.all((kappa > 5e4) & (kappa < 1e6)), kappa
    # the projection without the correction step: normal equations alone, kappa^2 eps
    Pw, Aw = cs.G[:, :, cs.lin], np.concatenate([cs.G[:, :, cs.non], cs.y[:, :, None]], axis=2)
    T = np.linalg.solve(np.einsum("bip,biq->bpq", Pw, Pw), np.einsum("bip,biq->bpq", Pw, Aw))
    assert sc.fractions(cs, "none", sc.reference(*sc.ILL, "none", True), c=T[:, :, -1])["c"] > 100.0


def test_reduce_is_a_projection():
    cs = sc.case(63, 5, 11)
    f, J, c, info = sc.reference(63, 5, 11, "per_problem")
    w = cs.ws["per_problem"].astype(LD)
    Pw = w[:, :, None] * cs.G[:, :, cs.lin]
    np.testing.assert_allclose((w * (np.einsum("bip,bp->bi", cs.G[:, :, cs.lin].astype(LD), c) - cs.y)), f,
                               rtol=0, atol=1e-16)
    assert np.max(np.abs(np.einsum("bip,bi->bp", Pw, f))) < 1e-16          # f is orthogonal to range(Phi_w)
    assert np.max(np.abs(np.einsum("bip,bij->bpj", Pw, J))) < 1e-15        # and so is every column of J_K


def test_reduce_rank_deficient():
    cs = sc.case(63, 5, 11)
    G = cs.G.copy()
    G[1, :, cs.lin[3]] = G[1, :, cs.lin[0]]                               # two identical columns in problem 1
    G[2, :, cs.lin[2]] = 0.0                                              # a column of zeros in problem 2
    for dt in (np.float64, LD):
        f, J, c, info = models.varpro_reduce(G.astype(dt), cs.y.astype(dt), None, cs.lin, cs.owner)
        assert info.tolist() == [0, 1, 1]
        assert np.isnan(f[1:]).all() and np.isnan(J[1:]).all() and np.isnan(c[1:]).all()
        if dt is np.float64:
            good = models.varpro_reduce(cs.G, cs.y, None, cs.lin, cs.owner)
            for a, b in zip((f, J, c), good):
                assert np.array_equal(a[0], b[0])                          # the batch mate keeps its bits


def test_reduce_argument_errors():
    cs = sc.case(5, 2, 2)
    with pytest.raises(ValueError, match="ascending"):
        models.varpro_reduce(cs.G, cs.y, None, cs.lin[::-1], cs.owner)
    with pytest.raises(ValueError, match="`owner` must be -1 on `lin`"):
        models.varpro_reduce(cs.G, cs.y, None, cs.lin, np.zeros(4, dtype=int))
    with pytest.raises(ValueError, match="m = 2 points"):
        models.varpro_reduce(cs.G[:, :2], cs.y[:, :2], None, cs.lin, cs.owner)
    with pytest.raises(ValueError, match="use `lsq_linear`"):
        models.varpro_reduce(cs.G, cs.y, None, [0, 1, 2, 3], [-1] * 4)


# ---- the gradient identity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, binned", [("exp*2+poly*1", False), ("gauss*2+lorentz+poly*2", False),
                                          ("gauss2d", False), ("gauss+poly*1", True)])
def test_kaufman_jacobian_gives_the_exact_gradient(spec, binned):
    M, n, x, P, Y = sc.fit_data(spec, binned)
    lin, owner = models.linear_params(spec, n)
    non = np.flatnonzero(owner >= 0)
    sigma = np.linspace(0.5, 2.0, sc.FIT_M)
    fres = models.separable_residual(spec, Y.astype(LD), sigma.astype(LD), n, binned)
    jres = models.separable_jacobian(spec, Y.astype(LD), sigma.astype(LD), n, binned)
    X = (1.1 * P[:, non] + 0.02).astype(LD)
    xl = np.asarray(x, dtype=LD)
    g = np.einsum("bij,bi->bj", jres(xl, X), fres(xl, X))
    h = LD(1e-7)
    for j in range(non.size):
        E = np.zeros(non.size, dtype=LD)
        E[j] = h
        fd = (0.5 * np.sum(fres(xl, X + E) ** 2, axis=1) - 0.5 * np.sum(fres(xl, X - E) ** 2, axis=1)) / (2 * h)
        np.testing.assert_allclose(np.asarray(g[:, j], float), np.asarray(fd, float), rtol=1e-8,
                                   atol=1e-9 * float(np.max(np.abs(g))))


# ---- a scipy solve over the reduced problem --------------------------------------------------------------------------
def test_scipy_over_the_reduced_problem_reaches_the_full_optimum():
    truth, t = np.array([3.0, 0.7, 1.5, 3.1, 0.2]), np.linspace(0.0, 4.0, 130)
    M = models.compose("exp*2+poly*1")
    y = M.f(t, truth[None]) + 0.01 * np.random.default_rng(5).standard_normal((1, 130))
    lin, owner = models.linear_params(M)
    non = np.flatnonzero(owner >= 0)
    fres, jres = models.separable_residual(M, y), models.separable_jacobian(M, y)
    coef = models.separable_coefficients(M, y)
    tol = dict(xtol=1e-14, ftol=1e-14, gtol=1e-14)
    red = least_squares(lambda a: fres(t, a[None])[0], 1.3 * truth[non] + 0.05, jac=lambda a: jres(t, a[None])[0], **tol)
    full = least_squares(lambda p: M.f(t, p[None])[0] - y[0], truth, jac=lambda p: M.jac(t, p[None])[0], **tol)
    assert red.success and full.success and red.nfev <= 15
    popt = models.varpro_expand(red.x, lin, 5)
    popt[lin] = coef(t, red.x[None])[0]
    np.testing.assert_allclose(popt, full.x, rtol=1e-7, atol=1e-9)
    # (ftol ends a solve once the cost is flat to 1e-14: x within about 1e-7 of the optimum, the residuals likewise)
    np.testing.assert_allclose(fres(t, red.x[None])[0], full.fun, rtol=0, atol=1e-8)


# ---- the front end, before any device is touched ---------------------------------------------------------------------
def _fit(**kw):
    M, n, x, P, Y = sc.fit_data("exp*2+poly*1")
    args = dict(f="exp*2+poly*1", xdata=x, ydata=Y, p0=sc.start("exp*2+poly*1", P), separable=True, driver="device")
    args.update(kw)
    return bounded_lsq.curve_fit_batch(**args)


@pytest.mark.parametrize("kw, match", [
    (dict(f=lambda x, P: P[:, :1] * x), "needs a built-in model"),
    (dict(f=models.expression("a*exp(-t/tau)+c", ("a", "tau", "c"))), "expression model"),
    (dict(jac="2-point"), "`jac` must be None"),
    (dict(jac="3-point"), "`jac` must be None"),
    (dict(loss="huber"), "`loss` must be 'linear'"),
    (dict(estimator="poisson"), "estimator='poisson' is not yet supported"),
    (dict(nan_policy="omit"), "nan_policy='omit' is not yet supported"),
    (dict(fixed=[1]), "`fixed` / `tied` are not yet supported"),
    (dict(tied={3: 1}), "`fixed` / `tied` are not yet supported"),
    (dict(response=np.ones(3)), "`response` is not yet supported"),
    (dict(leverage=True), "leverage=True is not yet supported"),
    (dict(f="poly"), "use `lsq_linear`"),
    (dict(driver="gpu"), "`driver` must be"),
    (dict(separable=1), "`separable` must be False or True"),
    (dict(bounds=(0.0, np.inf)), r"parameter 0 \('exp0.a'\) is linear"),
    (dict(bounds=([-np.inf, 0, -np.inf, 0, -np.inf], [np.inf, 9, np.inf, 9, 5.0])), r"parameter 4 \('poly0.p0'\)"),
])
def test_front_end_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        _fit(**kw)


def test_device_fit_checks_without_a_device():
    M, n, x, P, Y = sc.fit_data("exp*2+poly*1")
    fit = models.DeviceFit("exp*2+poly*1", n, x, Y, separable=True)
    assert (fit.n, fit.n_model, fit.B, fit.m) == (2, 5, sc.FIT_B, sc.FIT_M)
    assert fit.lin.tolist() == [0, 2, 4]
    with pytest.raises(ValueError, match="estimator='poisson' is not yet supported"):
        models.DeviceFit("exp*2+poly*1", n, x, Y, separable=True, estimator="poisson")
    with pytest.raises(ValueError, match="more points than linear parameters"):
        models.DeviceFit("exp*2+poly*1", n, x[:3], Y[:, :3], separable=True)
    assert not models.DeviceFit("exp*2+poly*1", n, x, Y).separable
