"""Missing data in batch fits on the GPU (nan_policy='omit'): the OMIT kernel instances behind
blsq_model_eval_nan_dev, bit for bit against blsq_model_eval_bin_dev at the kept rows and all-zero at the omitted ones;
the per-problem variance factor of the outer driver; and ``curve_fit_batch(..., nan_policy='omit')`` end to end against
lone fits of the compressed data."""
import itertools
import warnings

import numpy as np
import pytest
import scipy.optimize as so
from scipy.optimize import OptimizeWarning

import bounded_lsq
from bounded_lsq import models

import _nan_cases as nc
import _model_eval as me
from _model_eval import Dev, bits, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
LSE, POISSON = 0, 1                                    # BLSQ_EST_*
POINT, BIN = 0, 1                                      # BLSQ_SAMPLE_*
PROPAGATE, OMIT = 0, 1                                 # BLSQ_NAN_*


# ---- kernel level --------------------------------------------------------------------------------------------------
def evaluate(ctx, label, est, sampling, policy, B, reps, m, t, ts, y, w, X, Pfix, want_J, mask=None):
    """One launch on host arrays, f and J pre-filled with the sentinel -> (rc, f [B reps][m], J [B][m][nc] or None).
    policy None: blsq_model_eval_bin_dev (the entry of the parent); otherwise blsq_model_eval_nan_dev."""
    M, pm = nc.model_of(label), nc.map_of(label)
    n = nc.INSTANCES[label][1]
    ncol = n if pm is None else pm.nf
    Q = B * reps
    name, flags = "blsq_model_eval_nan_dev", dict(est=est, sampling=sampling, nan_policy=policy)
    if policy is None:
        name = "blsq_model_eval_bin_dev"
        del flags["nan_policy"]
    return me.run(ctx, name, (Q, m), (Q, m, ncol), True, want_J, nc.SENTINEL, strict=True, **flags, **me.model_args(M),
                  B=B, reps=reps, m=m, n=n, nf=ncol, pmap=None if pm is None else pm.pmap, t=t, t_stride=ts, y=y, w=w,
                  w_stride=me.w_stride(w, m), X=X, Pfix=Pfix, mask=mask)


def poisoned(case, om, w_kind, per_problem, sampling):
    """y with NaN at the omitted points; and NaN in whatever else belongs to an omitted point alone: its weight (per
    problem) and its abscissa or bin edges (per problem).  Shared arrays serve kept rows of other problems."""
    y = np.where(om, np.nan, case["y"])
    w = None if w_kind == 0 else case["w1"] if w_kind == 1 else np.where(om, np.nan, case["w2"])
    t = case["t"]
    if per_problem:
        t = np.where(om if t.ndim == 2 else om[:, None, :], np.nan, t)
    return t, y, w


@pytest.mark.parametrize("sampling", [POINT, BIN])
@pytest.mark.parametrize("est", [LSE, POISSON])
@pytest.mark.parametrize("label", list(nc.INSTANCES))
def test_omitted_rows_are_zero_and_kept_rows_keep_their_bits(ctx, label, est, sampling):
    """blsq_model_eval_nan_dev with BLSQ_NAN_OMIT over m in {1, 63, 64, 65, 130}, B in {1, 3} and every NaN pattern of
    ``_nan_cases.PATTERNS`` the shape has, each with the abscissa shared and per problem, each of those with reps 1 (f and
    J) and 3 (f); the weights (NULL, shared, per problem; least squares only) take turns, and the test ends by checking
    that every combination of (reps, t, w) has run.  All exact: at the kept rows f and J have the bits of
    blsq_model_eval_bin_dev (an entry of the parent) on the same inputs with the NaN replaced by 1.0; at the omitted rows
    every bit is 0; no sentinel survives.  The omitted points also carry NaN in their own weight and in their own
    abscissa or bin edges (where those are per problem), which the kept rows, of f and of J alike, must not see."""
    w_kinds = (0, 1, 2) if est == LSE else (0,)
    turns = itertools.cycle(w_kinds)
    seen = set()
    for m in nc.ROWS:
        for B in (1, 3):
            for pattern in nc.PATTERNS:
                om = nc.nan_pattern(pattern, B, m)
                if om is None:
                    assert pattern in ("seam", "tile", "problem")
                    continue
                assert om.shape == (B, m) and (om.any() or pattern == "none")
                for per_problem, reps in itertools.product((False, True), (1, 3)):
                    w_kind = next(turns)
                    seen.add((reps, per_problem, w_kind))
                    case = nc.kernel_inputs(label, m, B, reps, per_problem, sampling)
                    t, y, w = poisoned(case, om, w_kind, per_problem, sampling)
                    assert not per_problem or not om.any() or np.isnan(t).any()
                    w_ref = None if w_kind == 0 else case["w1"] if w_kind == 1 else case["w2"]
                    tail = (case["X"], case["Pfix"], reps == 1)
                    rc, f, J = evaluate(ctx, label, est, sampling, OMIT, B, reps, m, t, case["ts"], y, w, *tail)
                    rc0, f0, J0 = evaluate(ctx, label, est, sampling, None, B, reps, m, case["t"], case["ts"],
                                           np.where(om, 1.0, case["y"]), w_ref, *tail)
                    what = (label, est, sampling, m, B, pattern, reps, w_kind, per_problem)
                    assert rc == 0 and rc0 == 0, what
                    omq = np.repeat(om, reps, axis=0)
                    assert np.all(bits(f)[omq] == 0), what
                    assert np.array_equal(bits(f)[~omq], bits(f0)[~omq]), what
                    assert np.all(np.isfinite(f0)) and not np.any(f == nc.SENTINEL), what
                    if reps == 1:
                        assert np.all(bits(J)[om] == 0), what
                        assert np.array_equal(bits(J)[~om], bits(J0)[~om]), what
                        assert np.all(np.isfinite(J0)) and not np.any(J == nc.SENTINEL), what
    assert seen == set(itertools.product((1, 3), (False, True), w_kinds))


@pytest.mark.parametrize("label", list(nc.INSTANCES))
def test_propagate_is_the_parent_entry_bit_for_bit(ctx, label):
    """BLSQ_NAN_PROPAGATE: the outputs of blsq_model_eval_bin_dev in every bit, under both estimators and samplings, with
    clean data and (least squares) with a NaN in y, which then passes through."""
    for est, sampling, (m, reps, per_problem) in itertools.product(
            (LSE, POISSON), (POINT, BIN), ((130, 1, True), (65, 3, False))):
        case = nc.kernel_inputs(label, m, 3, reps, per_problem, sampling)
        w = case["w2"] if est == LSE else None
        for y in (case["y"],) + ((np.where(nc.nan_pattern("alternate", 3, m), np.nan, case["y"]),) if est == LSE else ()):
            args = (3, reps, m, case["t"], case["ts"], y, w, case["X"], case["Pfix"], reps == 1)
            a = evaluate(ctx, label, est, sampling, PROPAGATE, *args)
            b = evaluate(ctx, label, est, sampling, None, *args)
            assert a[0] == 0 and b[0] == 0 and np.array_equal(bits(a[1]), bits(b[1]))
            assert reps != 1 or np.array_equal(bits(a[2]), bits(b[2]))
            assert not np.any(a[1] == nc.SENTINEL)


@pytest.mark.parametrize("label", ["gauss_sum", "wide", "mapped"])
def test_masked_problems_keep_every_bit(ctx, label):
    """dmask = [1, 0, 1] under BLSQ_NAN_OMIT, per-problem t and w with NaN at the omitted points: the masked problem
    keeps the sentinel in f and J although it has omitted rows; the others have the bits of blsq_model_eval_bin_dev on the
    clean data at their kept rows and zeros at their omitted ones, with and without the mask."""
    m = 130
    case = nc.kernel_inputs(label, m, 3, 1, True, POINT)
    om = nc.nan_pattern("alternate", 3, m)
    t, y, w = poisoned(case, om, 2, True, POINT)
    args = (3, 1, m, t, case["ts"], y, w, case["X"], case["Pfix"], True)
    rc, f_all, J_all = evaluate(ctx, label, LSE, POINT, OMIT, *args)
    rc2, f, J = evaluate(ctx, label, LSE, POINT, OMIT, *args, mask=[1, 0, 1])
    rc0, f0, J0 = evaluate(ctx, label, LSE, POINT, None, 3, 1, m, case["t"], case["ts"], np.where(om, 1.0, case["y"]),
                           case["w2"], case["X"], case["Pfix"], True)
    assert rc == 0 and rc2 == 0 and rc0 == 0
    assert np.all(f[1] == nc.SENTINEL) and np.all(J[1] == nc.SENTINEL)
    assert np.array_equal(bits(f[[0, 2]]), bits(f_all[[0, 2]])) and np.array_equal(bits(J[[0, 2]]), bits(J_all[[0, 2]]))
    assert np.all(bits(f_all)[om] == 0) and np.all(bits(J_all)[om] == 0)
    assert np.array_equal(bits(f_all)[~om], bits(f0)[~om]) and np.array_equal(bits(J_all)[~om], bits(J0)[~om])
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(J0))


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, est = 2, sampling = 3, nan_policy = 4, model = 5,
    ncomp = 6, fam = 7, cnt = 8, B = 9, reps, m, n = 12, nf = 13, pmap = 14, t = 15, t_stride, y = 17, w = 18, w_stride,
    X = 20, Pfix = 21, f = 22, J = 23; -25 / -26 for the contents of pmap), blsq_last_error names it, and nothing is
    launched: the outputs keep their sentinel."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufP = d.up(np.ones(64)), d.up(np.ones(64))
        out, outJ = d.up(np.full(64, -7.0)), d.up(np.full(64, -7.0))

        def call(est=LSE, sampling=POINT, policy=OMIT, model=2, ncomp=0, fam=None, cnt=None, B=1, reps=1, m=4, n=4, nf=4,
                 pmap=None, t=buf, ts=0, y=buf, w=None, ws=0, X=bufP, Pfix=None, f=out, J=None):
            return me.call(ctx, "blsq_model_eval_nan_dev", True, est=est, sampling=sampling, nan_policy=policy,
                           model=model, ncomp=ncomp, fam=fam, cnt=cnt, B=B, reps=reps, m=m, n=n, nf=nf, pmap=pmap, t=t,
                           t_stride=ts, y=y, w=w, w_stride=ws, X=X, Pfix=Pfix, f=f, J=J, mask=None)
        bad = [(dict(est=2), -2, b"est"), (dict(sampling=2), -3, b"sampling"),
               (dict(policy=2), -4, b"nan_policy"), (dict(policy=-1), -4, b"nan_policy"),
               (dict(model=5), -5, b"model"), (dict(model=-2), -5, b"model"), (dict(ncomp=1), -6, b"ncomp"),
               (dict(model=-1, ncomp=0), -6, b"ncomp"), (dict(model=-1, ncomp=1, cnt=(4,)), -7, b"fam"),
               (dict(model=-1, ncomp=1, fam=(4,)), -8, b"cnt"), (dict(B=0), -9, b"B"), (dict(reps=0), -10, b"reps"),
               (dict(m=0), -11, b"m "), (dict(n=5, nf=5), -12, b"n "), (dict(nf=3), -13, b"nf"),
               (dict(nf=3, pmap=(0, 1, 2, 3)), -25, b"pmap"), (dict(nf=3, pmap=(0, 1, 1, -1), Pfix=bufP), -26, b"pmap"),
               (dict(t=None), -15, b"t is NULL"), (dict(ts=3), -16, b"t_stride"), (dict(sampling=BIN, ts=4), -16, b"t_stride"),
               (dict(y=None), -17, b"y is NULL"), (dict(y=None, est=POISSON), -17, b"y is NULL"),
               (dict(est=POISSON, w=buf), -18, b"w must be NULL"), (dict(w=buf, ws=3), -19, b"w_stride"),
               (dict(X=None), -20, b"X is NULL"), (dict(nf=3, pmap=(0, 1, 2, -1)), -21, b"Pfix"),
               (dict(f=None), -22, b"f and J"), (dict(reps=2, J=outJ), -23, b"reps")]
        for kw, want, word in bad:
            assert call(**kw) == want, (kw, want)
            assert word in lib.blsq_last_error(h), (kw, lib.blsq_last_error(h))
        ctx.sync()
        assert np.all(ctx.to_host(out, (64,), np.float64) == -7.0) and np.all(ctx.to_host(outJ, (64,), np.float64) == -7.0)
        assert call(policy=PROPAGATE, y=None) == 0                          # y is optional without the policy
        assert call() == 0 and call(ts=4, ws=4, w=buf) == 0 and call(nf=3, pmap=(0, 1, 2, -1), Pfix=bufP, J=outJ) == 0
        ctx.sync()
        assert not np.any(ctx.to_host(out, (4,), np.float64) == -7.0)
    finally:
        d.close()


# ---- the per-problem variance factor -------------------------------------------------------------------------------
def test_outer_driver_variance_factor_per_problem(ctx):
    """``OuterDriver.covariance_nobs(nobs)`` (blsq_outer_covariance_pinv_nobs) equals the unscaled pseudo-inverse
    covariance times obj / (nobs - n) computed in numpy to rtol 1e-14 (a single multiply differs by at most one
    rounding), and is not finite where nobs <= n; counts outside 0 .. m are refused."""
    from bounded_lsq import OuterDriver
    rng = np.random.default_rng(3)
    B, m, n = 4, 20, 3
    A = rng.standard_normal((B, m, n))
    y = rng.standard_normal((B, m))
    nobs = np.array([20, 11, 4, 3], dtype=np.int32)
    for b in range(B):                                  # zero rows, as the kernel leaves them
        A[b, nobs[b]:] = 0.0
        y[b, nobs[b]:] = 0.0
    X0 = np.zeros((B, n))
    with OuterDriver('trf', B, m, n, ctx=ctx) as drv:
        drv.start(X0, X0, -np.inf, np.inf, np.ones((B, n)), False, 1e-10, 1e-10, 1e-10, 100)
        R = drv.run_host(lambda X: np.einsum("bij,bj->bi", A, X) - y, lambda X: A)
        plain = drv.covariance(pinv=True)
        scaled = drv.covariance_nobs(nobs)
        uniform = drv.covariance(pinv=True, variance_scale=True)
        obj = R["obj"]
        with pytest.raises(ValueError, match="0 .. m"):
            drv.covariance_nobs(np.array([20, 21, 4, 3]))
        with pytest.raises(ValueError, match="shape"):
            drv.covariance_nobs(nobs[:3])
        rc = ctx.lib.blsq_outer_covariance_pinv_nobs(drv.h, 0, None, *[None] * 5)
        assert rc == -3 and b"nobs is NULL" in ctx.lib.blsq_last_error(ctx.h)
    assert np.all(obj[:2] > 0)
    for b in range(3):
        np.testing.assert_allclose(scaled[0][b], plain[0][b] * (obj[b] / (int(nobs[b]) - n)), rtol=1e-14, atol=0)
    assert not np.any(np.isfinite(np.diag(scaled[0][3])))
    assert all(np.array_equal(scaled[k], plain[k]) for k in (1, 2, 3, 4))
    np.testing.assert_allclose(scaled[0][0], uniform[0][0], rtol=1e-14, atol=0)         # nobs = m: the uniform factor


# ---- end to end ----------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)


def in_units_of(pcov, ref):
    """pcov with entry (i, j) divided by the standard deviations i and j of `ref`: the correlation matrix for pcov = ref."""
    d = np.sqrt(np.einsum("bii->bi", ref))
    return pcov / (d[:, :, None] * d[:, None, :])


def agree(a, b, what, rtol_p=1e-6, atol_p=1e-9):
    """popt to rtol 1e-6 / atol 1e-9 and the normalised pcov to 1e-6, the figures of tests/test_composite_gpu.py::agree for
    two routes to one optimum.  Both matrices are normalised by the standard deviations of the reference `a`, not each by
    its own, so the variance factor obj / (nobs - nf) of `b` does not cancel: a diagonal entry of `b` is its variance over
    the reference's, and degrees of freedom counted from m instead of nobs would put it 5 / 66 = 7 % or more off 1."""
    np.testing.assert_allclose(b[0], a[0], rtol=rtol_p, atol=atol_p, err_msg=str(what))
    got, ref = in_units_of(b[1], a[1]), in_units_of(a[1], a[1])
    print("%s: popt rel %.2e, pcov in the reference's units %.2e"
          % (what, np.max(np.abs(b[0] - a[0]) / (np.abs(a[0]) + 1e-3)), np.max(np.abs(got - ref))))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6, err_msg=str(what))


def batch_fit(ctx, spec, x, Y, P0, bounds, driver, method, **kw):
    common = dict(bounds=bounds, method=method, ctx=ctx, driver=driver, **TOL)
    common.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(spec, x, Y, P0, **common)


def lone_fits(ctx, spec, xs, ys, P0, bounds, method, **kw):
    """Every problem alone (B = 1) on its own compressed data, without the keyword -> (popt (B, n), pcov (B, n, n),
    results)."""
    out = [batch_fit(ctx, spec, xs[b], ys[b][None], P0[b:b + 1], (bounds[0][b:b + 1], bounds[1][b:b + 1]), "device",
                     method, **kw) for b in range(len(xs))]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), [o[2][0] for o in out]


@pytest.fixture(scope="module")
def lone_reference(ctx):
    """The lone fits of every (m, method), computed once and left unchanged."""
    cache = {}

    def get(m, method):
        if (m, method) not in cache:
            pr = nc.fit_problem(m)
            om = nc.fit_omitted(pr)
            xs = [pr["x"][~om[b]] for b in range(8)]
            ys = [pr["Y"][b][~om[b]] for b in range(8)]
            cache[(m, method)] = (pr, om, lone_fits(ctx, pr["spec"], xs, ys, pr["P0"], pr["bounds"], method,
                                                    sigma=nc.SIGMA, leverage=True))
        return cache[(m, method)]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("m", nc.FIT_ROWS)
def test_batch_with_omit_agrees_with_lone_fits(ctx, lone_reference, m, method):
    """B = 8 problems of 'gauss+poly*1' with the patterns of ``_nan_cases.fit_omitted`` (none, ragged tail, 10 % at
    random, a window on the peak's flank), fitted together with nan_policy='omit' on both drivers, against each problem
    fitted alone on its compressed data: popt, the normalised and the plain pcov (which holds nobs - nf), and the
    leverages: exactly 0 at the omitted rows, the lone fit's at the kept ones (rtol 1e-6 / atol 1e-9)."""
    pr, om, lone = lone_reference(m, method)
    assert all(r.success for r in lone[2])
    Yn = nc.blanked(pr["Y"], om)
    for driver in ("device", "host"):
        R = batch_fit(ctx, pr["spec"], pr["x"], Yn, pr["P0"], pr["bounds"], driver, method, sigma=nc.SIGMA,
                      nan_policy="omit", leverage=True)
        assert all(r.success for r in R[2]), (driver, [r.status for r in R[2]])
        agree(lone, R, (m, method, driver))
        for b, (rb, rl) in enumerate(zip(R[2], lone[2])):
            assert rb.nobs == m - om[b].sum() and np.array_equal(rb.omitted, om[b])
            assert np.all(bits(rb.leverage)[om[b]] == 0) and np.all(bits(rb.fun)[om[b]] == 0)
            assert np.all(bits(rb.jac)[om[b]] == 0)
            np.testing.assert_allclose(rb.leverage[~om[b]], rl.leverage, rtol=1e-6, atol=1e-9)


def test_poisson_binned_with_dead_channels(ctx):
    """estimator='poisson', binned=True on contiguous edges with dead channels blanked, absolute_sigma=True, on both
    drivers, against the lone fits of the live channels given as rows lo, hi: the case with no other way through."""
    h = nc.histogram_problem()
    om, edges = h["omitted"], h["edges"]
    rows = models.bin_rows(edges)
    kw = dict(estimator="poisson", binned=True, absolute_sigma=True)
    lone = lone_fits(ctx, h["spec"], [rows[:, ~om[b]] for b in range(6)], [h["Y"][b][~om[b]] for b in range(6)],
                     h["P0"], h["bounds"], "trf", **kw)
    assert all(r.success for r in lone[2])
    Yn = nc.blanked(h["Y"], om)
    for driver in ("device", "host"):
        R = batch_fit(ctx, h["spec"], edges, Yn, h["P0"], h["bounds"], driver, "trf", nan_policy="omit", **kw)
        assert all(r.success for r in R[2])
        agree(lone, R, ("poisson binned", driver))
        np.testing.assert_allclose([r.deviance for r in R[2]], [r.deviance for r in lone[2]], rtol=1e-9)
    with pytest.raises(ValueError, match="must be finite"):
        batch_fit(ctx, h["spec"], edges, Yn, h["P0"], h["bounds"], "device", "trf", **kw)


def test_ragged_scans(ctx):
    """``pad_ragged`` on scans of 40, 64 and 70 points, fitted together, against the three lone fits."""
    r = nc.ragged_scans()
    X, Y = models.pad_ragged(r["xs"], r["ys"])
    assert X.shape == (3, 70) and models.count_observed(Y).tolist() == [40, 64, 70]
    lone = lone_fits(ctx, nc.SPEC, r["xs"], r["ys"], r["P0"], r["bounds"], "trf", sigma=nc.SIGMA)
    for driver in ("device", "host"):
        R = batch_fit(ctx, nc.SPEC, X, Y, r["P0"], r["bounds"], driver, "trf", sigma=nc.SIGMA, nan_policy="omit")
        assert all(q.success for q in R[2]) and [q.nobs for q in R[2]] == [40, 64, 70]
        agree(lone, R, ("ragged", driver))


def test_finite_differences_and_robust_loss_with_omit(ctx, lone_reference):
    """jac='3-point' with omit against the analytic route (rtol 1e-4 / atol 1e-7, the figure of
    tests/test_composite_gpu.py for finite differences against analytic), and loss='soft_l1' with omit against the lone
    fits under the same loss (its figures for two routes to one optimum)."""
    pr, om, lone = lone_reference(33, "trf")
    Yn = nc.blanked(pr["Y"], om)
    fd = batch_fit(ctx, pr["spec"], pr["x"], Yn, pr["P0"], pr["bounds"], "device", "trf", sigma=nc.SIGMA,
                   nan_policy="omit", jac="3-point")
    assert all(r.success for r in fd[2]) and all(np.all(bits(r.jac)[om[b]] == 0) for b, r in enumerate(fd[2]))
    np.testing.assert_allclose(fd[0], lone[0], rtol=1e-4, atol=1e-7)
    Yo = pr["Y"].copy()
    Yo[:, ::9] += 0.3                                                      # outliers
    kw = dict(sigma=nc.SIGMA, loss="soft_l1", f_scale=2.0)
    lone_r = lone_fits(ctx, pr["spec"], [pr["x"][~om[b]] for b in range(8)], [Yo[b][~om[b]] for b in range(8)],
                       pr["P0"], pr["bounds"], "trf", **kw)
    R = batch_fit(ctx, pr["spec"], pr["x"], nc.blanked(Yo, om), pr["P0"], pr["bounds"], "device", "trf",
                  nan_policy="omit", **kw)
    assert all(r.success for r in R[2]) and all(r.success for r in lone_r[2])
    agree(lone_r, R, "soft_l1")


def test_device_model_takes_any_sigma_at_omitted_points(ctx):
    """``DeviceModel`` / ``DeviceFit`` themselves (not ``curve_fit_batch``, which cleans `sigma` first): a (B, m) `sigma`
    holding inf and NaN at the omitted points gives the bits of the clean `sigma` at the kept rows of f and J and zeros at
    the omitted ones, without a warning, and a fit driven by such a ``DeviceFit`` ends where the clean one does."""
    pr = nc.fit_problem(70)
    om = nc.fit_omitted(pr)
    B, m = om.shape
    Yn = nc.blanked(pr["Y"], om)
    rng = np.random.default_rng(9)
    sg = rng.uniform(0.005, 0.02, (B, m))
    sg_bad = np.where(om, np.where(np.arange(m) % 2 == 0, np.inf, np.nan), sg)
    assert not np.all(np.isfinite(sg_bad))
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for key, y, sigma, policy in (("bad", Yn, sg_bad, "omit"), ("clean", np.where(om, 1.0, pr["Y"]), sg, "propagate")):
            with models.DeviceModel(ctx, nc.SPEC, B, m, nc.NF, pr["x"], y, sigma, nan_policy=policy) as dm:
                d_x, d_f, d_J = ctx.to_device(pr["P0"]), ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * nc.NF)
                try:
                    dm.fun_dev(d_x, d_f, 1)
                    dm.jac_dev(d_x, d_J)
                    out[key] = (ctx.to_host(d_f, (B, m), np.float64), ctx.to_host(d_J, (B, m, nc.NF), np.float64))
                finally:
                    for p in (d_x, d_f, d_J):
                        ctx.free(p)
        for k in (0, 1):
            assert np.all(bits(out["bad"][k])[om] == 0)
            assert np.array_equal(bits(out["bad"][k])[~om], bits(out["clean"][k])[~om])
            assert np.all(np.isfinite(out["clean"][k]))
        fits = [bounded_lsq.least_squares_batch(
            models.DeviceFit(nc.SPEC, nc.NF, pr["x"], Yn, sigma, nan_policy="omit"), pr["P0"], None, bounds=pr["bounds"],
            driver="device", ctx=ctx, **TOL) for sigma in (sg_bad, np.where(om, 1.0, sg))]
    assert all(r.success for r in fits[0])
    for ra, rb in zip(*fits):
        assert np.array_equal(ra.x, rb.x) and np.array_equal(bits(ra.fun), bits(rb.fun))
        assert np.array_equal(bits(ra.jac), bits(rb.jac))


def test_underdetermined_problem_leaves_its_mates_alone(ctx):
    """One problem keeps nobs = nf points: its pcov is inf under exactly one OptimizeWarning, and its batch mates have the
    results they have when fitted without it."""
    pr = nc.fit_problem(33)
    om = nc.fit_omitted(pr)
    om[2] = True
    om[2, [4, 8, 10, 14]] = False                                           # four points on the peak: nobs = nf = 4
    Yn = nc.blanked(pr["Y"], om)
    kw = dict(bounds=pr["bounds"], sigma=nc.SIGMA, driver="device", ctx=ctx, nan_policy="omit", **TOL)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        popt, pcov, res = bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], Yn, pr["P0"], **kw)
    assert [w.category for w in rec] == [OptimizeWarning]
    assert res[2].nobs == 4 and np.all(np.isinf(pcov[2]))
    mates = [b for b in range(8) if b != 2]
    kw["bounds"] = (pr["bounds"][0][mates], pr["bounds"][1][mates])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        popt2, pcov2, res2 = bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], Yn[mates], pr["P0"][mates], **kw)
    assert np.array_equal(popt[mates], popt2) and np.array_equal(pcov[mates], pcov2)
    assert np.all(np.isfinite(pcov2))


def test_single_problem_against_scipy(ctx):
    """``curve_fit(..., nan_policy='omit')`` against scipy's (method='trf'): popt to rtol 1e-6 / atol 1e-9."""
    rng = np.random.default_rng(4)
    x = np.linspace(0.0, 4.0, 50)

    def f(t, a, k, c):
        return a * np.exp(-k * t) + c
    y = f(x, 2.5, 1.3, 0.5) + 0.01 * rng.standard_normal(x.size)
    y[[3, 17, 18, 40]] = np.nan
    sg = rng.uniform(0.5, 2.0, x.size)
    kw = dict(p0=[2.0, 1.0, 0.3], bounds=([0.0, 0.0, 0.0], [10.0, 5.0, 2.0]), sigma=sg, nan_policy="omit", **TOL)
    ref = so.curve_fit(f, x, y, method="trf", **kw)
    got = bounded_lsq.curve_fit(f, x, y, **kw)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-6, atol=1e-9)
    # beyond the issue's figure for popt: the variances, which hold ysize - n after the omission.  Another solver's
    # optimum 1e-6 away moves a variance by that times its logarithmic sensitivity (of order 1 to 10): 1e-4 allows ten
    # times that; the four omitted points would show as 4 / 43 = 9 %
    np.testing.assert_allclose(np.diag(got[1]), np.diag(ref[1]), rtol=1e-4)


def test_device_route_calls_the_new_entry_alone(ctx, monkeypatch):
    """The device route with omit runs through run_device alone and through blsq_model_eval_nan_dev alone: run_host and
    the numpy functions of the model raise, and no other model entry is looked up."""
    from bounded_lsq import _models, _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    pr = nc.fit_problem(33)
    om = nc.fit_omitted(pr)
    Yn = nc.blanked(pr["Y"], om)
    args = (ctx, pr["spec"], pr["x"], Yn, pr["P0"], pr["bounds"])
    kw = dict(sigma=nc.SIGMA, nan_policy="omit")
    want = batch_fit(*args, "device", "trf", **kw)
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    monkeypatch.setattr(_models, "omit_residual", boom)
    monkeypatch.setattr(_models, "omit_jacobian", boom)
    for T in _models.TERMS.values():
        monkeypatch.setattr(T, "fill", boom)
    counts = me.count_entries(ctx, monkeypatch)

    def tally():
        return {"nan": counts.get("blsq_model_eval_nan_dev", 0),
                "other": sum(v for k, v in counts.items() if k != "blsq_model_eval_nan_dev")}
    got = batch_fit(*args, "device", "trf", **kw)
    entries = tally()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert entries["nan"] > 0 and entries["other"] == 0
    fd = batch_fit(*args, "device", "trf", jac="2-point", **kw)
    entries = tally()
    assert all(r.success for r in fd[2]) and entries["other"] == 0
    with pytest.raises(AssertionError, match="host callback"):
        batch_fit(*args, "host", "trf", **kw)
