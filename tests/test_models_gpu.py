"""Built-in fit models on the GPU: the kernel behind blsq_model_eval_dev against the numpy formulas in extended
precision, and ``curve_fit_batch(f='name')`` end to end against the same models passed as numpy callables."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

import _model_cases as mc
import _model_eval as me
from _model_eval import Dev, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble


# ---- kernel level --------------------------------------------------------------------------------------------------
def eval_dev(ctx, name, B, reps, m, n, x, per_problem, y, w, P, want_f=True, want_J=False, mask=None, fill=None):
    """blsq_model_eval_dev on host arrays -> (rc, f or None, J or None).  fill: the value f and J hold before."""
    M = models.get(name)
    Q = B * reps
    return me.run(ctx, "blsq_model_eval_dev", (Q, m), (Q, m, n), want_f, want_J, np.nan if fill is None else fill,
                  strict=True, model=M.id, B=B, reps=reps, m=m, n=n, t=x, t_stride=M.coords * m if per_problem else 0,
                  y=y, w=w, w_stride=me.w_stride(w, m), X=P, mask=mask)


# name, n: poly n = 1, 7, 64; exp_sum K = 1, 3; gauss_sum K = 1, 5, 21 (n = 64); lorentz_sum K = 2; gauss2d
KERNEL_CASES = [("poly", 1), ("poly", 7), ("poly", 64), ("exp_sum", 3), ("exp_sum", 7), ("gauss_sum", 4),
                ("gauss_sum", 16), ("gauss_sum", 64), ("lorentz_sum", 7), ("gauss2d", 5)]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name,n", KERNEL_CASES, ids=["%s-%d" % c for c in KERNEL_CASES])
def test_kernel_against_longdouble(ctx, name, n, m):
    """f and J of blsq_model_eval_dev against the numpy formulas evaluated in np.longdouble, over B in {1, 3},
    reps in {1, 3} (f), t shared and per problem, w NULL / shared / per problem, y NULL and given; m crosses the
    64-row tile (1, 63, 64, 65, 130 = two tiles and two rows) and n = 64 is the width at which a workgroup holds a
    single tile.

    The bound, per entry (eps = 2^-52; K the number of terms, n for the polynomial; arg_k the argument of the
    exponential of term k, 0 where there is none):

        |f - f_ref| <= 2 eps |w| [ sum_k |term_k| (4 + K + 2 |arg_k|) + |y| ]
        |J - J_ref| <= 2 eps |w| |dmodel/dp_j| (8 + K + 2 |arg_k(j)|)

    It counts the roundings of the formulas as bounded_lsq/_models.py and csrc/model_kernels.hip evaluate them, in
    units of eps relative to the term:
      * the argument: exp turns a relative error delta of its argument into delta |arg| of its value.  -(r t) is one
        rounding; z = (t - mu) / s is two (the inputs are exact, so the difference is one rounding, not a
        cancellation), z z doubles them and adds one, the factor -1/2 is exact: at most 5 |arg|; the 2-D Gaussian's
        (du du + dv dv) / (s s) is at most 6 |arg|.  These worst cases need every rounding at its limit with one
        sign; roundings of independent operations do not align, and the count carried in the bound is one rounding of
        the argument with the factor 2 of slack: 2 |arg|;
      * one transcendental of at most 1 ulp, and the products and quotients after it: a e is one more (f: 2 so far);
        the Lorentzian's 1 / (1 + z z) has 5 + 1 + 1 and a e one more, without an exponential.  A Jacobian entry has
        up to four more operations ((g z) / s z; ((2 g) e z) / s z; (g r2) / (s2 s) with r2 and s2 s rounded): c0 = 4
        for f and 8 for J, before the slack;
      * the sum of the K terms and c: K additions, each at most eps of the partial sum, which sum |term_k| bounds;
        Horner's rule for the polynomial is within (2 n - 1) eps sum |p_k t^k|, and t^k by repeated product within
        (k - 1) eps |t^k|;
      * - y and * w: one rounding each of the result, which sum |term_k| + |y| bounds (part of c0).
    The factor 2 in front is the slack over this count.  The float64 numpy functions must meet the same bound, which
    is asserted here as well: the kernel may differ from them in the last bit of exp() only.

    Measured (MI355X), worst error / bound over these cases, the kernel and numpy alike: poly 0.205, exp_sum 0.215,
    gauss_sum 0.222, lorentz_sum 0.169, gauss2d 0.276."""
    M = models.get(name)
    rng = np.random.default_rng([n, m])
    worst = {"device": 0.0, "numpy": 0.0}

    def check(got, ref, tol, who, what):
        ratio = np.abs(got.astype(LD) - ref) / np.where(tol > 0, tol, 1)
        ratio = np.where(tol > 0, ratio, np.where(got == ref, 0, np.inf))
        r = float(np.max(ratio))
        worst[who] = max(worst[who], r)
        assert r <= 1.0, (name, n, m, who, what, r)

    for B in (1, 3):
        for per_problem in (False, True):
            W = rng.uniform(0.5, 2.0, (B, m))
            Y = rng.standard_normal((B, m))
            for reps in (1, 3):
                x, P = mc.case_inputs(name, n, B * reps, m, seed=[n, m, B, reps], per_problem=False)
                if per_problem:
                    x = mc.case_inputs(name, n, B, m, seed=[n, m, B, reps], per_problem=True)[0]
                for w in (None, W[0], W):
                    for y in (None, Y):
                        f_ref, J_ref, f_tol, J_tol = mc.bounds_of(name, x, P, w, y, reps=reps)
                        want_J = reps == 1
                        rc, f, J = eval_dev(ctx, name, B, reps, m, n, x, per_problem, y, w, P, True, want_J)
                        assert rc == 0
                        what = (B, reps, per_problem, None if w is None else w.ndim, y is not None)
                        check(f, f_ref, f_tol, "device", ("f",) + what)
                        # the float64 numpy functions, weighted as curve_fit_batch weights them
                        xr = np.repeat(x, reps, axis=0) if per_problem else x
                        wr = 1.0 if w is None else (np.repeat(w, reps, axis=0) if w.ndim == 2 else w)
                        yr = 0.0 if y is None else np.repeat(y, reps, axis=0)
                        check(wr * (M.f(xr, P) - yr), f_ref, f_tol, "numpy", ("f",) + what)
                        if want_J:
                            check(J, J_ref, J_tol, "device", ("J",) + what)
                            wj = wr if np.ndim(wr) == 0 else np.asarray(wr)[..., np.newaxis]
                            check(wj * M.jac(xr, P), J_ref, J_tol, "numpy", ("J",) + what)
                            if y is None:                      # J alone (f = NULL) gives the same bits
                                rc, _, J2 = eval_dev(ctx, name, B, 1, m, n, x, per_problem, None, w, P, False, True)
                                assert rc == 0 and np.array_equal(J, J2)
    print("model %s n=%d m=%d: worst error / bound  device %.3f  numpy %.3f" % (name, n, m, worst["device"],
                                                                               worst["numpy"]))


@pytest.mark.parametrize("name,n,m", [("poly", 3, 65), ("gauss_sum", 7, 130), ("gauss_sum", 64, 70), ("gauss2d", 5, 64)])
def test_masked_problems_are_left_untouched(ctx, name, n, m):
    """mask = [1, 0, 1]: the masked problem keeps every bit of the sentinel in f and in J, the others keep none."""
    B = 3
    x, P = mc.case_inputs(name, n, B, m, seed=5, per_problem=True)
    sentinel = -6.02214076e23
    rc, f, J = eval_dev(ctx, name, B, 1, m, n, x, True, None, None, P, True, True, mask=[1, 0, 1], fill=sentinel)
    assert rc == 0
    s = np.float64(sentinel)
    assert np.all(f[1].view(np.uint64) == s.view(np.uint64)) and np.all(J[1].view(np.uint64) == s.view(np.uint64))
    assert not np.any(f[[0, 2]] == s) and not np.any(J[[0, 2]] == s)
    rc, f_all, J_all = eval_dev(ctx, name, B, 1, m, n, x, True, None, None, P, True, True)
    assert np.array_equal(f[[0, 2]], f_all[[0, 2]]) and np.array_equal(J[[0, 2]], J_all[[0, 2]])


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, model = 2, B, reps, m, n, t, t_stride, y, w,
    w_stride, P, f, J, mask); nothing is launched."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufP, out = d.up(np.zeros(64)), d.up(np.ones(64)), d.up(np.zeros(64))

        def call(model=2, B=1, reps=1, m=4, n=4, t=buf, ts=0, y=None, w=None, ws=0, P=bufP, f=out, J=None):
            return me.call(ctx, "blsq_model_eval_dev", True, model=model, B=B, reps=reps, m=m, n=n, t=t, t_stride=ts,
                           y=y, w=w, w_stride=ws, X=P, f=f, J=J, mask=None)
        assert call() == 0
        ctx.sync()
        assert call(model=5) == -2 and call(model=-1) == -2
        assert call(B=0) == -3 and call(reps=0) == -4 and call(m=0) == -5
        assert call(n=5) == -6 and call(n=67) == -6 and call(model=4, n=4) == -6 and call(model=0, n=65) == -6
        assert call(t=None) == -7 and call(ts=3) == -8 and call(model=4, n=5, ts=4) == -8
        assert call(w=buf, ws=3) == -11 and call(P=None) == -12 and call(f=None) == -13
        assert call(reps=2, J=out) == -14
        assert b"reps" in lib.blsq_last_error(h)
    finally:
        d.close()


def test_evaluate_against_numpy(ctx):
    for name, n in KERNEL_CASES:
        for per_problem in (False, True):
            x, P = mc.case_inputs(name, n, 3, 70, seed=2, per_problem=per_problem)
            got = models.evaluate(name, x, P, ctx=ctx)
            f_ref, _, f_tol, _ = mc.bounds_of(name, x, P, None, None)
            assert got.shape == (3, 70)
            assert np.all(np.abs(got.astype(LD) - f_ref) <= f_tol), name
            np.testing.assert_allclose(got, models.get(name).f(x, P), rtol=1e-13, atol=1e-14)
    with pytest.raises(ValueError):
        models.evaluate("gauss_sum", np.zeros(5), np.ones((2, 5)), ctx=ctx)


# ---- end to end ----------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)


def fit(ctx, pr, route, method, **kw):
    """route A: the numpy functions as callables, driver='device'; B: the name, driver='device'; C: the name,
    driver='host'."""
    M = models.get(pr["name"])
    common = dict(sigma=mc.SIGMA, bounds=pr["bounds"], method=method, ctx=ctx, **TOL)
    common.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if route == "A":
            return bounded_lsq.curve_fit_batch(M.f, pr["x"], pr["Y"], pr["P0"], jac=M.jac, driver="device", **common)
        return bounded_lsq.curve_fit_batch(pr["name"], pr["x"], pr["Y"], pr["P0"],
                                           driver="device" if route == "B" else "host", **common)


def normalised(pcov):
    d = np.sqrt(np.einsum("bii->bi", pcov))
    return pcov / (d[:, :, None] * d[:, None, :])


def agree(a, b, what, rtol_p=1e-6, atol_p=1e-9):
    np.testing.assert_allclose(b[0], a[0], rtol=rtol_p, atol=atol_p, err_msg=str(what))
    np.testing.assert_allclose(normalised(b[1]), normalised(a[1]), rtol=0, atol=1e-6, err_msg=str(what))
    dp = float(np.max(np.abs(b[0] - a[0]) / (np.abs(a[0]) + 1e-3)))
    dc = float(np.max(np.abs(normalised(b[1]) - normalised(a[1]))))
    return dp, dc


@pytest.fixture(scope="module")
def reference_fits(ctx):
    """Route A of every (family, m, method), computed once and left unchanged."""
    cache = {}

    def get(label, m, method):
        key = (label, m, method)
        if key not in cache:
            pr = mc.fit_problem(label, m)
            cache[key] = (pr, fit(ctx, pr, "A", method))
        return cache[key]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("m", [33, 70])
@pytest.mark.parametrize("label", list(mc.FITS))
def test_fit_by_name_agrees_with_the_callable(ctx, reference_fits, label, m, method):
    """B = 8 problems per family; the named model on the device (B) and on the host (C) against the same numpy
    functions as callables on the device driver (A): every problem succeeds on every route, popt to rtol 1e-6 /
    atol 1e-9 and the normalised pcov to 1e-6 (the suite's figures for two fits of one problem at these tolerances;
    tighter ones would test the termination rule: the routes differ in the last bits of model and Jacobian)."""
    pr, A = reference_fits(label, m, method)
    assert all(r.success for r in A[2]), [r.status for r in A[2]]
    fits = {}
    for route in ("B", "C"):
        R = fit(ctx, pr, route, method)
        assert all(r.success for r in R[2]), (route, [r.status for r in R[2]])
        dp, dc = agree(A, R, (label, m, method, route))
        fits[route] = R
        print("fit %s m=%d %s route %s: popt spread %.2e  normalised pcov spread %.2e  nfev <= %d"
              % (label, m, method, route, dp, dc, max(r.nfev for r in R[2])))
    # results[b].fun / .jac are the weighted residuals and Jacobian at popt
    B_ = fits["B"]
    M = models.get(pr["name"])
    np.testing.assert_allclose(np.stack([r.fun for r in B_[2]]), (M.f(pr["x"], B_[0]) - pr["Y"]) / mc.SIGMA,
                               rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(np.stack([r.jac for r in B_[2]]), M.jac(pr["x"], B_[0]) / mc.SIGMA, rtol=1e-9,
                               atol=1e-9)


def test_robust_loss_by_name(ctx):
    """loss='soft_l1' on gauss_sum, A against B: under a robust loss the Jacobian callback after a judge writes the
    accepted problems only (the masked write of the kernel)."""
    pr = mc.fit_problem("gauss2", 70)
    pr["Y"][:, ::9] += 0.3                                                 # outliers
    kw = dict(loss="soft_l1", f_scale=2.0)
    A = fit(ctx, pr, "A", "trf", **kw)
    R = fit(ctx, pr, "B", "trf", **kw)
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "soft_l1")
    print("soft_l1: nfev", [r.nfev for r in R[2]], "njev", [r.njev for r in R[2]])


def test_finite_differences_by_name(ctx):
    """jac='2-point' on exp_sum: FdJacobian on the device with the kernel as fun (reps = n), against the analytic
    route at the suite's figure for FD against analytic."""
    pr = mc.fit_problem("exp1", 33)
    an = fit(ctx, pr, "B", "trf")
    for jac in ("2-point", "3-point"):
        fd = fit(ctx, pr, "B", "trf", jac=jac)
        assert all(r.success for r in fd[2])
        np.testing.assert_allclose(fd[0], an[0], rtol=1e-4, atol=1e-7)


def test_leverage_by_name(ctx):
    pr = mc.fit_problem("lorentz1", 33)
    A = fit(ctx, pr, "A", "dogbox", leverage=True)
    R = fit(ctx, pr, "B", "dogbox", leverage=True)
    for ra, rb in zip(A[2], R[2]):
        assert rb.leverage.shape == (33,)
        np.testing.assert_allclose(rb.leverage, ra.leverage, rtol=1e-6, atol=1e-9)
        assert abs(rb.leverage.sum() - 4) < 1e-6                            # trace of the hat matrix = n


def test_named_device_route_calls_no_host_callback(ctx, monkeypatch):
    """Route B runs through run_device alone: run_host raises, and so do the numpy model functions."""
    from bounded_lsq import _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    pr = mc.fit_problem("gauss1", 33)
    M = models.get("gauss_sum")
    want = fit(ctx, pr, "B", "trf")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(M, "f", boom)
    monkeypatch.setattr(M, "jac", boom)
    calls = []
    real = _outer.OuterDriver.run_device
    monkeypatch.setattr(_outer.OuterDriver, "run_device",
                        lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    got = fit(ctx, pr, "B", "trf")
    assert calls == [1] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got_fd = fit(ctx, pr, "B", "trf", jac="2-point")
    assert calls == [1, 1] and all(r.success for r in got_fd[2])
    with pytest.raises(AssertionError, match="host callback"):
        fit(ctx, pr, "C", "trf")


def test_device_model_frees_its_buffers_and_own_context():
    """DeviceModel on a context of its own: close() is idempotent; curve_fit_batch without ctx opens and closes one."""
    pr = mc.fit_problem("poly4", 33)
    popt, pcov, res = bounded_lsq.curve_fit_batch("poly", pr["x"], pr["Y"], pr["P0"], sigma=mc.SIGMA, driver="device")
    assert all(r.success for r in res) and np.all(np.isfinite(pcov))
    from bounded_lsq import _abi
    c = _abi.Context(0)
    dm = models.DeviceModel(c, "poly", 8, 33, 4, pr["x"], pr["Y"], mc.SIGMA)
    assert dm.set_bounds(*pr["bounds"]) == dm.bounds_dev and len(dm.bounds_dev) == 2
    dm.close()
    dm.close()
    c.close()
