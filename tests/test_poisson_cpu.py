"""The Poisson estimator without a GPU: ``models.poisson_transform`` against extended precision, the
deviance identity, the float64 definition inside the bound the kernel is held to, the end-to-end problems of
tests/test_poisson_gpu.py vetted with scipy, and the errors the front ends raise before they need a device."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import bounded_lsq
from bounded_lsq import ParamMap, models

import _poisson_cases as pc

LD = np.longdouble
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def grid():
    mu, y = pc.transform_grid()
    r, c = models.poisson_transform(mu, y)
    r_ref, c_ref = pc.reference(mu, y)
    return mu, np.broadcast_to(y, mu.shape), r, c, r_ref, c_ref


def test_transform_against_longdouble(grid):
    """float64 ``poisson_transform`` against the formulas of the definition in np.longdouble (``_poisson_cases.reference``
    says where those are taken as written and where, and why, from the series) over y = 0 and 1e-3 .. 1e9 and
    u = mu / y - 1 in [-1 + 1e-12, 1e6] with 0, denormal-small |u| and +-U0 (1 +- 2^-40).

    The bound is twice the measured worst relative error (``_poisson_cases.MEASURED``; the margin is for
    another libm's log1p and sqrt).  Measured in eps = 2^-52, r / c: 2.56 / 2.80 where mu >= y / 2 and at y == 0;
    below, the error grows like y / mu (u = (mu - y) / y keeps eps of absolute error, which log1p divides by
    1 + u = mu / y): 1.12 / 0.88 times y / mu; over the whole grid therefore 1.13e10 / 1.13e10, reached at its corner
    u = -1 + 1e-12.  All three are asserted: the last is the one figure for the whole grid, the first two hold the rest
    of it to what it achieves.  Also: the sign of r is the sign of mu - y exactly, r == 0 where mu == y, c is finite and
    positive everywhere, and the float64 and the longdouble evaluation of the function agree (the dtype is kept)."""
    mu, y, r, c, r_ref, c_ref = grid
    assert r.dtype == np.float64 and c.dtype == np.float64
    assert np.array_equal(np.sign(r), np.sign(mu - y))
    assert np.all(r[mu == y] == 0) and np.any(mu == y)
    assert np.all(np.isfinite(c)) and np.all(c > 0)
    near = mu >= y / 2
    ratio = np.where(near, 1.0, mu / np.where(y > 0, y, 1))
    for what, got, ref in (("r", r, r_ref), ("c", c, c_ref)):
        e = pc.rel_err(got, ref)
        a, b, whole = pc.MEASURED[what]
        worst = (float(e[near].max()), float((e * ratio)[~near].max()), float(e.max()))
        print("poisson_transform %s: worst relative error %.3f eps (mu >= y/2), %.3f eps * y/mu (below), %.3g eps (grid)"
              % ((what,) + worst))
        assert worst[0] <= 2 * a and worst[1] <= 2 * b and worst[2] <= 2 * whole, (what, worst)
    # longdouble in, longdouble out: the same function is its own reference within long double's rounding
    rl, cl = models.poisson_transform(mu.astype(LD), y.astype(LD))
    assert rl.dtype == LD and cl.dtype == LD
    assert float(pc.rel_err(rl, r_ref)[near].max()) < 0.05 and float(pc.rel_err(cl, c_ref)[near].max()) < 0.05


def test_branches_meet_at_u0():
    """The series and the direct form of phi on the two sides of |u| = U0, 2^-40 apart: each lies within twice the
    measured error of its branch from the reference (measured: r 0.76 / 2.40, c 0.99 / 2.68 eps for series / direct), so
    the two meet within a few eps."""
    y = np.logspace(-3, 9, 49)
    for sgn in (1.0, -1.0):
        for side in (1 - 2.0 ** -40, 1 + 2.0 ** -40):
            mu = y * (1 + sgn * pc.U0 * side)
            assert np.all((np.abs((mu - y) / y) < pc.U0) == (side < 1))               # the branch meant is the branch taken
            for what, got, ref in zip("rc", models.poisson_transform(mu, y), pc.reference(mu, y)):
                assert float(pc.rel_err(got, ref).max()) <= 2 * pc.MEASURED[what][0], (sgn, side, what)


def test_reference_series_meets_the_unsimplified_formulas():
    """Where both are accurate (0.2 <= |u| < 0.25: the unsimplified formulas lose 2 eps_ld / u^2 < 0.03 eps there) the
    two halves of the reference agree to 0.05 eps."""
    y = np.logspace(-3, 9, 25)[:, np.newaxis]
    u = np.concatenate([np.linspace(0.2, 0.2499, 500), -np.linspace(0.2, 0.2499, 500)])
    mu = y * (1 + u)
    for a, b in zip(pc.reference(mu, y), pc.unsimplified(mu, y)):
        assert float(pc.rel_err(a, b).max()) < 0.05


def test_deviance_identity_and_derivative(grid):
    """sum r^2 is the deviance 2 sum [mu - y + y ln(y / mu)] of the longdouble formula, and c is dr / dmu: a longdouble
    central difference of r (step 1e-6 mu: its truncation 1e-12 relative, its rounding 1e-13)."""
    rng = np.random.default_rng(3)
    mu = rng.uniform(0.05, 30.0, (16, 200))
    y = rng.poisson(mu).astype(float)
    y[0] = 0.0
    assert np.any(y == 0)
    r, c = models.poisson_transform(mu, y)
    yl, ml = y.astype(LD), mu.astype(LD)
    with np.errstate(all="ignore"):
        D = 2 * (ml - yl + np.where(yl > 0, yl * np.log(np.where(yl > 0, yl, 1) / ml), 0))
    np.testing.assert_allclose((r.astype(LD) ** 2).sum(axis=1), D.sum(axis=1), rtol=1e-14)
    h = 1e-6 * ml
    rp, rm = models.poisson_transform(ml + h, yl)[0], models.poisson_transform(ml - h, yl)[0]
    np.testing.assert_allclose(c, ((rp - rm) / (2 * h)).astype(float), rtol=1e-10)
    # and against the unsimplified derivative where it is defined well
    far = np.abs(mu - y) > 0.3 * y
    np.testing.assert_allclose(c[far], ((1 - yl / ml) / r.astype(LD))[far].astype(float), rtol=1e-13)


@pytest.mark.parametrize("label", list(pc.INSTANCES))
def test_float64_definition_meets_the_kernel_bound(label):
    """The float64 numpy definition (the route of a callable, and of driver='host') at the inputs of
    test_poisson_gpu.py::test_kernel_against_definition lies within the bound the kernel is held to there, which shows
    the bound attainable; and those inputs hold what they are meant to: zeros, mu == y exactly, both sides of U0."""
    worst = 0.0
    for m in pc.ROWS:
        for reps, per_problem in ((1, False), (1, True), (3, True)):
            case = pc.kernel_case(label, m, reps, per_problem)
            r_ref, J_ref, r_tol, J_tol = pc.kernel_bounds(label, case, reps)
            r, J = pc.numpy_definition(label, case, reps)
            assert np.all(np.isfinite(r)) and np.all(np.isfinite(J))
            worst = max(worst, pc.cc.worst_ratio(r, r_ref, r_tol), pc.cc.worst_ratio(J, J_ref, J_tol))
            assert np.all(r[:reps][:, case["y"][0] == 3.0] == 0)          # problem 0: mu == 3 at all its points
            if m >= 63 and reps == 1:
                y, mu = case["y"], pc.model_of(label).f(case["x"], case["P"])
                u = np.abs(mu[y > 0] / y[y > 0] - 1).astype(float)
                assert np.any(y == 0) and np.any(mu == y) and np.any((u > 0) & (u < pc.U0)) and np.any(u > pc.U0)
    print("poisson %s: numpy definition, worst error / bound %.3f" % (label, worst))
    assert worst <= 1.0


# ---- the end-to-end problems, vetted -----------------------------------------------------------------------------------
def scipy_fit(pr, b, poisson, pm=None):
    M = models.compose(pr["spec"])
    x, y = pr["x"], pr["Y"][b:b + 1]
    lb, ub = pr["bounds"][0][b], pr["bounds"][1][b]
    p0 = pr["P0"][b]
    full = (lambda v: v[np.newaxis]) if pm is None else (lambda v: pm.expand_x(v, pr["P0"][b])[np.newaxis])
    red = (lambda J: J) if pm is None else pm.reduce_jac
    if pm is not None:
        lb, ub = pm.reduce_bounds(lb, ub)
        p0 = pm.reduce_x(p0)
    if poisson:
        fun = lambda v: models.poisson_residual(M.f, y)(x, full(v))[0]                        # noqa: E731
        jac = lambda v: models.poisson_jacobian(M.f, lambda xd, P: red(M.jac(xd, P)), y)(x, full(v))[0]   # noqa: E731
    else:
        fun = lambda v: (M.f(x, full(v)) - y)[0]                                              # noqa: E731
        jac = lambda v: red(M.jac(x, full(v)))[0]                                             # noqa: E731
    return least_squares(fun, p0, jac=jac, bounds=(lb, ub), method="trf", ftol=1e-13, xtol=1e-13, gtol=1e-13)


def test_end_to_end_problems_are_fit_for_the_gpu_tests():
    """The seeded problems of test_poisson_gpu.py, solved with scipy over the numpy definition: every problem has empty
    channels, converges with no variable on a bound, has a vanishing Poisson score at its optimum
    (|sum_i (1 - y_i / mu_i) dmu_i / dp_j| < 1e-6 sum_i |...| for every j), and its maximum-likelihood popt differs from
    the least-squares popt by more than 1e-3 relative in at least one parameter: the estimator is seen to do something."""
    pr = pc.fit_problem()
    B = pr["Y"].shape[0]
    assert pr["Y"].shape == (8, 96) and np.all(np.any(pr["Y"] == 0, axis=1)) and np.all(pr["Y"] == np.round(pr["Y"]))
    for b in range(B):
        mle, lse = scipy_fit(pr, b, True), scipy_fit(pr, b, False)
        assert mle.success and lse.success and not np.any(mle.active_mask) and not np.any(lse.active_mask), b
        S, A = pc.score(pr["spec"], pr["x"], pr["Y"][b:b + 1], mle.x[np.newaxis])
        assert np.all(np.abs(S) < 1e-6 * A), (b, S / A)
        rel = np.abs(mle.x - lse.x) / np.abs(lse.x)
        assert rel.max() > 1e-3, (b, rel)
    # the fixed / tied variants of the GPU test: the width held at p0; two lines of one width: nothing on a bound either
    for prv, pm in ((pr, ParamMap(4, [2], None)), (pc.fit_problem(two=True), ParamMap(7, None, {5: 2}))):
        assert np.all(np.any(prv["Y"] == 0, axis=1))
        for b in range(B):
            mle = scipy_fit(prv, b, True, pm)
            assert mle.success and not np.any(mle.active_mask), (pm, b)
            S, A = pc.score(prv["spec"], prv["x"], prv["Y"][b:b + 1], pm.expand_x(mle.x, prv["P0"][b])[np.newaxis], pm)
            assert np.all(np.abs(S) < 1e-6 * A), (pm, b)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_validation_errors_need_no_device():
    pr = pc.fit_problem()
    x, Y, P0 = pr["x"], pr["Y"], pr["P0"]
    M = models.compose(pr["spec"])

    def batch(f=pr["spec"], Y=Y, **kw):
        return bounded_lsq.curve_fit_batch(f, x, Y, P0, bounds=pr["bounds"], **kw)
    for driver in ("host", "device"):
        for f in (pr["spec"], M.f):
            with pytest.raises(ValueError, match="unknown estimator"):
                batch(f, driver=driver, estimator="mle")
            with pytest.raises(ValueError, match="`sigma` must be None"):
                batch(f, driver=driver, estimator="poisson", sigma=1.0)
            bad = Y.copy()
            bad[3, 5] = -1.0
            with pytest.raises(ValueError, match="must not be negative"):
                batch(f, Y=bad, driver=driver, estimator="poisson")
            for v in (np.nan, np.inf):
                bad[3, 5] = v
                with pytest.raises(ValueError, match="must be finite"):
                    batch(f, Y=bad, driver=driver, estimator="poisson")
    with pytest.raises(ValueError, match="unknown estimator"):
        batch(estimator=None)

    def f1(t, a, mu, s, c):
        return M.f(t, np.array([[a, mu, s, c]]))[0]
    with pytest.raises(ValueError, match="unknown estimator"):
        bounded_lsq.curve_fit(f1, x, Y[0], p0=P0[0], estimator="ml")
    with pytest.raises(ValueError, match="unknown estimator"):
        bounded_lsq.curve_fit(f1, x, Y[0], p0=P0[0], estimator="ml", fixed=[2])
    with pytest.raises(ValueError, match="`sigma` must be None"):
        bounded_lsq.curve_fit(f1, x, Y[0], p0=P0[0], estimator="poisson", sigma=np.ones(96))
    with pytest.raises(ValueError, match="must not be negative"):
        bounded_lsq.curve_fit(f1, x, -Y[0] - 1, p0=P0[0], estimator="poisson")
    with pytest.raises(ValueError, match="must be finite"):
        bounded_lsq.curve_fit(f1, x, np.where(Y[0] == 0, np.inf, Y[0]), p0=P0[0], estimator="poisson",
                              check_finite=False)
    # the device objects check the same before they touch a context
    with pytest.raises(ValueError, match="unknown estimator"):
        models.DeviceFit(pr["spec"], 4, x, Y, estimator="huber")
    with pytest.raises(ValueError, match="`sigma` must be None"):
        models.DeviceFit(pr["spec"], 4, x, Y, sigma=1.0, estimator="poisson")
    with pytest.raises(ValueError, match="needs `ydata`"):
        models.DeviceModel(None, pr["spec"], 8, 96, 4, x, estimator="poisson")
    fit = models.DeviceFit(pr["spec"], 4, x, Y, estimator="poisson")
    assert fit.estimator == "poisson" and models.DeviceFit(pr["spec"], 4, x, Y).estimator == "lse"


def test_front_end_routes(monkeypatch):
    """driver='device' with a name hands ``least_squares_batch`` a DeviceFit that carries the estimator (and, without the
    keyword, one built exactly as before it existed); every other route hands it the wrapped numpy functions, whose
    Jacobian is c times the map-reduced Jacobian of the model."""
    from bounded_lsq import _curve_fit
    pr = pc.fit_problem()
    seen = {}

    class Stop(Exception):
        pass

    def spy(fun, x0, jac, **kw):
        seen.update(fun=fun, x0=x0, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, "least_squares_batch", spy)
    real = models.DeviceFit
    made = []
    monkeypatch.setattr(_curve_fit._models, "DeviceFit", lambda *a, **k: (made.append(k), real(*a, **k))[1])
    args = (pr["spec"], pr["x"], pr["Y"], pr["P0"])
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(*args, bounds=pr["bounds"], driver="device", estimator="poisson", fixed=[2])
    assert isinstance(seen["fun"], real) and seen["fun"].estimator == "poisson" and seen["jac"] is None
    assert seen["fun"].n == 3
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(*args, bounds=pr["bounds"], driver="device")
    assert "estimator" not in made[-1] and seen["fun"].estimator == "lse"
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(*args, bounds=pr["bounds"], driver="host", estimator="poisson", fixed=[2])
    pm = ParamMap(4, [2], None)
    M = models.compose(pr["spec"])
    X = pm.reduce_x(pr["P0"])
    r, c = models.poisson_transform(M.f(pr["x"], pr["P0"]), pr["Y"])
    assert np.array_equal(seen["fun"](X), r)
    assert np.array_equal(seen["jac"](X), c[:, :, None] * pm.reduce_jac(M.jac(pr["x"], pr["P0"])))
