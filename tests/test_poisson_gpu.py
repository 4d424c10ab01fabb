"""The Poisson estimator on the GPU: the Poisson kernel instances behind blsq_model_eval_est_dev against
the numpy definition in extended precision, the entry with BLSQ_EST_LSE bit for bit against the three entries it stands
in for, and ``curve_fit_batch(..., estimator='poisson')`` end to end on count data across its routes."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import ParamMap, models

import _poisson_cases as pc
import _model_eval as me
from _model_eval import Dev, agree, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble
LSE, POISSON = 0, 1                                    # BLSQ_EST_*


# ---- kernel level --------------------------------------------------------------------------------------------------
def eval_est(ctx, label, est, reps, m, x, per_problem, y, w, X, Pfix=None, want_f=True, want_J=False, mask=None,
             fill=None, entry="est"):
    """blsq_model_eval_est_dev for the instance `label` on host arrays -> (rc, f or None, J or None); entry='old': the
    same call through the entry it stands in for (blsq_model_eval_dev, _map_dev or _comp_dev).  fill: the value f and J
    hold before."""
    M, pm = pc.model_of(label), pc.map_of(label)
    n = pc.INSTANCES[label][1]
    nc = n if pm is None else pm.nf
    Q = pc.B * reps
    if entry == "est":
        name = "blsq_model_eval_est_dev"
    elif pc.is_composite(label):
        name = "blsq_model_eval_comp_dev"
    else:
        name = "blsq_model_eval_dev" if pm is None else "blsq_model_eval_map_dev"
    return me.run(ctx, name, (Q, m), (Q, m, nc), want_f, want_J, np.nan if fill is None else fill, est=est,
                  **me.model_args(M), B=pc.B, reps=reps, m=m, n=n, nf=nc, pmap=None if pm is None else pm.pmap, t=x,
                  t_stride=M.coords * m if per_problem else 0, y=y, w=w, w_stride=me.w_stride(w, m), X=X,
                  Pfix=Pfix if pm is not None else None, mask=mask)


@pytest.mark.parametrize("m", pc.ROWS)
@pytest.mark.parametrize("label", list(pc.INSTANCES))
def test_kernel_against_definition(ctx, label, m):
    """f = r and J = c dmu/dp of blsq_model_eval_est_dev (BLSQ_EST_POISSON) against ``models.poisson_transform`` over the
    numpy model, both evaluated in np.longdouble: B = 3, reps in {1, 3} (f only for 3), t shared and per problem, m across
    the 64-row tile; gauss_sum n = 7, exp_sum n = 5, gauss2d, gauss_sum with one parameter fixed and one tied, and the
    composite 'gauss+pvoigt+poly*2' without and with a map.  The counts (``_poisson_cases.kernel_case``) hold zeros,
    points with mu == y exactly (problem 0 is its offset alone, at the integer 3: there r must be 0.0), |u| on both sides
    of U0 = 1 / 4, integers, and u = 3.

    The bound, per entry (eps = 2^-52; v_tol and Jm_tol the bounds of the model value and of its Jacobian column from
    ``_model_cases.bounds_of`` / ``_composite_cases.bounds_of`` with w = 1 and y = 0, derived in tests/test_models_gpu.py
    and tests/test_composite_gpu.py; |Jm| the column's magnitude there; with a map the slot's bound is the sum of its
    columns' plus 2 eps (g - 1) sum |Jm| for the g - 1 additions):

        |r - r_ref| <= |c| v_tol + 2 eps T_r |r|
        |J - J_ref| <= |c| Jm_tol + |c| |Jm| [2 eps (T_c + 1) + v_tol / mu]

      * the error of the model value reaches r through dr / dmu = c, and c through dc / dmu: c = 1 / (mu s) with
        s = sqrt(2 phi(u) / y) gives d ln c / d mu = -1 / mu - phi'(u) / (2 y phi(u)); phi decreases, and
        (1 + u) |phi' / phi| / 2 stays below 1 / 2 (it is 1 / 3 at u = 0 and tends to 1 / 2 as u grows and to 0 at
        u = -1), so |dc / dmu| <= c / mu; at y == 0, c = 1 / sqrt(2 mu) and it is c / (2 mu);
      * T_r and T_c count the roundings of the transform itself, relative to r and c, as poisson_transform and poisson_rc
        perform them, with the factor 2 of slack in front as in the model tests.  d = mu - y: 1; u = d / y: 2.
        The series (|u| < U0): an error delta of u moves phi by |u phi' / phi| delta <= 0.2 delta, the last Horner steps
        add 1 + 2 |u| / (1 - |u|) <= 1.7 and the truncation 1 / 8: e_phi = 3.  The direct form: the numerator
        N = u - log1p(u) carries 2 |u| (u itself) + 2 |u| / (1 + u) (u through log1p, whose derivative is 1 / (1 + u):
        this is the term that grows like y / mu where mu << y) + L |log1p(u)| (the device's log1p within L = 2 ulp), all
        relative to N, + 1 for the subtraction; u u: 5; the quotient: 1:
            e_phi = 7 + [2 |u| + 2 |u| / (1 + u) + 2 |log1p(u)|] / N            (57 at u = 1 / 4, 21 at u = 1)
        taken on both sides of U0 within 1e-6, where the model's own error may decide the branch.  2 phi is exact,
        / y: 1, the square root halves and adds 1: e_s = (e_phi + 1) / 2 + 1; r = d s: e_s + 2; c = 1 / (mu s): e_s + 2:
            T_r = T_c = e_phi / 2 + 3.5;        y == 0:  r = sqrt(2 mu): T_r = 2,  c = 1 / r: T_c = 3
        and the product c Jm adds the + 1.
    The float64 numpy definition meets the same bound on the same inputs
    (tests/test_poisson_cpu.py::test_float64_definition_meets_the_kernel_bound: worst error / bound 0.07 .. 0.20).  J
    computed with f = NULL gives the bits of J computed with f.

    Measured (MI355X), worst error / bound per instance over these cases, in the order of INSTANCES: 0.195, 0.077,
    0.135, 0.136, 0.120, 0.119."""
    worst = 0.0
    for reps, per_problem in ((1, False), (1, True), (3, False), (3, True)):
        case = pc.kernel_case(label, m, reps, per_problem)
        r_ref, J_ref, r_tol, J_tol = pc.kernel_bounds(label, case, reps)
        want_J = reps == 1
        rc, f, J = eval_est(ctx, label, POISSON, reps, m, case["x"], per_problem, case["y"], None, case["X"],
                            case["Pfix"], True, want_J)
        assert rc == 0
        assert np.all(f[:reps][:, case["y"][0] == 3.0] == 0.0)              # mu == y exactly
        rf = pc.cc.worst_ratio(f, r_ref, r_tol)
        worst = max(worst, rf)
        assert rf <= 1.0, (label, m, reps, per_problem, "f", rf)
        if want_J:
            rj = pc.cc.worst_ratio(J, J_ref, J_tol)
            worst = max(worst, rj)
            assert rj <= 1.0, (label, m, reps, per_problem, "J", rj)
            rc, _, J2 = eval_est(ctx, label, POISSON, 1, m, case["x"], per_problem, case["y"], None, case["X"],
                                 case["Pfix"], False, True)
            assert rc == 0 and np.array_equal(J, J2)
    print("poisson %s m=%d: worst error / bound  device %.3f" % (label, m, worst))


@pytest.mark.parametrize("label", list(pc.INSTANCES))
def test_lse_through_the_new_entry_is_bit_for_bit(ctx, label):
    """BLSQ_EST_LSE: f and J of blsq_model_eval_est_dev equal those of blsq_model_eval_dev / _map_dev / _comp_dev on the
    same inputs, with weights and data, in every bit; m = 130 and 65, reps 1 (f and J) and 3 (f)."""
    rng = np.random.default_rng(7)
    for m, reps, per_problem in ((130, 1, True), (65, 1, False), (65, 3, True)):
        case = pc.kernel_case(label, m, reps, per_problem)
        w = rng.uniform(0.5, 2.0, (pc.B, m))
        for wv, yv in ((w, case["y"]), (w[0], None), (None, None)):
            a = eval_est(ctx, label, LSE, reps, m, case["x"], per_problem, yv, wv, case["X"], case["Pfix"], True,
                         reps == 1)
            b = eval_est(ctx, label, LSE, reps, m, case["x"], per_problem, yv, wv, case["X"], case["Pfix"], True,
                         reps == 1, entry="old")
            assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])
            assert reps != 1 or np.array_equal(a[2], b[2])
            assert np.all(np.isfinite(a[1]))


@pytest.mark.parametrize("label", ["gauss_sum", "gauss_sum-map", "composite-map"])
def test_masked_problems_are_left_untouched(ctx, label):
    """mask = [1, 0, 1]: the masked problem keeps every bit of the sentinel in f and in J, the others keep none."""
    m = 130
    case = pc.kernel_case(label, m, 1, True)
    sentinel = -6.02214076e23
    args = (ctx, label, POISSON, 1, m, case["x"], True, case["y"], None, case["X"], case["Pfix"], True, True)
    rc, f, J = eval_est(*args, mask=[1, 0, 1], fill=sentinel)
    assert rc == 0
    s = np.float64(sentinel)
    assert np.all(f[1].view(np.uint64) == s.view(np.uint64)) and np.all(J[1].view(np.uint64) == s.view(np.uint64))
    assert not np.any(f[[0, 2]] == s) and not np.any(J[[0, 2]] == s)
    rc, f_all, J_all = eval_est(*args)
    assert np.array_equal(f[[0, 2]], f_all[[0, 2]]) and np.array_equal(J[[0, 2]], J_all[[0, 2]])


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, est = 2, model = 3, ncomp = 4, fam = 5, cnt = 6,
    B = 7, reps, m, n = 10, nf = 11, pmap = 12, t = 13, t_stride, y = 15, w = 16, w_stride, X = 18, Pfix = 19, f = 20,
    J = 21, mask; -23 / -24 for the contents of pmap; BLSQ_EST_POISSON: y NULL -15, w given -16); nothing is launched: the
    outputs keep their sentinel."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufP = d.up(np.zeros(64)), d.up(np.ones(64))
        out, outJ = d.up(np.full(64, -7.0)), d.up(np.full(64, -7.0))

        def call(est=POISSON, model=2, fam=None, cnt=None, ncomp=None, B=1, reps=1, m=4, n=4, nf=4, pmap=None, t=buf,
                 ts=0, y=bufP, w=None, ws=0, X=bufP, Pfix=None, f=out, J=None):
            nc = ncomp if ncomp is not None else (0 if fam is None else len(fam))
            return me.call(ctx, "blsq_model_eval_est_dev", True, est=est, model=model, ncomp=nc, fam=fam, cnt=cnt, B=B,
                           reps=reps, m=m, n=n, nf=nf, pmap=pmap, t=t, t_stride=ts, y=y, w=w, w_stride=ws, X=X, Pfix=Pfix,
                           f=f, J=J, mask=None)
        comp = dict(model=-1, fam=(0, 4), cnt=(1, 1))
        bad = [(dict(est=2), -2), (dict(est=-1), -2), (dict(model=5), -3), (dict(model=-2), -3),
               (dict(ncomp=1), -4), (dict(model=-1), -4), (dict(model=-1, ncomp=9, fam=(4,) * 9, cnt=(1,) * 9), -4),
               (dict(model=-1, ncomp=2, cnt=(1, 1)), -5), (dict(model=-1, fam=(0, 5), cnt=(1, 1)), -5),
               (dict(model=-1, ncomp=2, fam=(0, 4)), -6), (dict(model=-1, fam=(0, 4), cnt=(0, 1)), -6),
               (dict(B=0), -7), (dict(reps=0), -8), (dict(m=0), -9),
               (dict(n=5, nf=5), -10), (dict(model=4, n=4), -10), (dict(n=5, nf=5, **comp), -10),
               (dict(nf=3), -11), (dict(nf=5, pmap=(0, 1, 2, 3)), -11), (dict(nf=0, pmap=(0, 1, 2, 3)), -11),
               (dict(nf=3, **comp), -11),
               (dict(nf=3, pmap=(0, 1, 2, 3)), -23), (dict(nf=3, pmap=(0, 1, -2, 2)), -23),
               (dict(nf=3, pmap=(0, 1, 1, -1), Pfix=bufP), -24),
               (dict(t=None), -13), (dict(ts=3), -14), (dict(model=4, n=5, nf=5, ts=4), -14), (dict(ts=8, **comp), -14),
               (dict(y=None), -15), (dict(w=buf), -16), (dict(est=LSE, w=buf, ws=3), -17),
               (dict(X=None), -18), (dict(nf=3, pmap=(0, 1, 2, -1)), -19), (dict(f=None), -20),
               (dict(reps=2, J=outJ), -21)]
        for kw, want in bad:
            assert call(**kw) == want, (kw, want)
        assert b"reps" in lib.blsq_last_error(h)
        assert call(y=None) == -15 and b"Poisson" in lib.blsq_last_error(h)
        ctx.sync()
        assert np.all(ctx.to_host(out, (64,), np.float64) == -7.0) and np.all(ctx.to_host(outJ, (64,), np.float64) == -7.0)
        assert call() == 0 and call(est=LSE, y=None, w=buf, ws=4, ts=4) == 0 and call(J=outJ, **comp) == 0
        assert call(nf=3, pmap=(0, 1, 2, -1), Pfix=bufP, J=outJ) == 0
        ctx.sync()
        assert not np.any(ctx.to_host(out, (4,), np.float64) == -7.0)
    finally:
        d.close()


# ---- end to end ----------------------------------------------------------------------------------------------------
# The fits are solved to 1e-13: the score test below needs it.  The ftol rule stops a solve once a step changes the
# deviance by less than ftol times the deviance, and the deviance is quadratic in the distance to its minimum, so the score
# left at termination goes like sqrt(ftol): at the suite's usual 1e-10 the worst |score| / sum |summands| was 2.3e-6.
TOL = dict(ftol=1e-13, xtol=1e-13, gtol=1e-13)


def fit(ctx, pr, route, **kw):
    """route A: the numpy model and its Jacobian as callables, driver='device'; B: the spec, driver='device' (the
    kernel); C: the spec, driver='host'."""
    M = models.compose(pr["spec"])
    common = dict(bounds=pr["bounds"], ctx=ctx, estimator="poisson", absolute_sigma=True, **TOL)
    common.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if route == "A":
            common.setdefault("jac", M.jac)
            return bounded_lsq.curve_fit_batch(M.f, pr["x"], pr["Y"], pr["P0"], driver="device", **common)
        return bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], pr["Y"], pr["P0"],
                                           driver="device" if route == "B" else "host", **common)


@pytest.fixture(scope="module")
def problem():
    return pc.fit_problem()


@pytest.fixture(scope="module")
def device_fit(ctx, problem):
    """Route B of the plain problem, computed once and left unchanged."""
    return fit(ctx, problem, "B")


def test_fit_routes_agree_and_reach_the_likelihood_optimum(ctx, problem, device_fit):
    """B = 8 spectra of m = 96 channels with empty channels in each (tests/test_poisson_cpu.py vets them with scipy): the
    kernel (B), the numpy definition on the host driver (C) and the same definition as callables on the device driver (A)
    agree to the figures of tests/test_models_gpu.py; the Poisson score vanishes at the kernel's popt
    (|sum_i (1 - y_i / mu_i) dmu_i / dp_j| < 1e-6 sum_i |...|), nothing is on a bound, and the results carry the deviance
    residuals, the deviance and the Jacobian of the deviance residuals."""
    pr, R = problem, device_fit
    assert all(r.success for r in R[2]), [r.status for r in R[2]]
    for route in ("A", "C"):
        O = fit(ctx, pr, route)
        assert all(r.success for r in O[2]), (route, [r.status for r in O[2]])
        agree(O, R, route)
    popt = R[0]
    assert np.all(popt > pr["bounds"][0]) and np.all(popt < pr["bounds"][1])
    S, A = pc.score(pr["spec"], pr["x"], pr["Y"], popt)
    print("poisson fit: worst |score| / sum |summands| %.2e  nfev <= %d" % (float((np.abs(S) / A).max()),
                                                                         max(r.nfev for r in R[2])))
    assert np.all(np.abs(S) < 1e-6 * A)
    M = models.compose(pr["spec"])
    r_def, c_def = models.poisson_transform(M.f(pr["x"], popt), pr["Y"])
    np.testing.assert_allclose(np.stack([r.fun for r in R[2]]), r_def, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(np.stack([r.jac for r in R[2]]), c_def[:, :, None] * M.jac(pr["x"], popt), rtol=1e-9,
                               atol=1e-9)
    for b, r in enumerate(R[2]):
        assert r.obj_value == pytest.approx(float(np.dot(r_def[b], r_def[b])), rel=1e-9)
        assert r.deviance == pytest.approx(r.obj_value, rel=1e-12)
    # the estimator is seen to do something: least squares on the same data ends elsewhere
    L = bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], pr["Y"], pr["P0"], bounds=pr["bounds"], ctx=ctx,
                                    driver="device", **TOL)
    assert all(r.success for r in L[2])
    assert np.all(np.max(np.abs(popt - L[0]) / np.abs(L[0]), axis=1) > 1e-3)


def test_absolute_sigma_is_the_dispersion_factor(ctx, problem, device_fit):
    """absolute_sigma=False multiplies the covariance of absolute_sigma=True by obj_value / (m - nf), the quasi-Poisson
    dispersion, and changes nothing else."""
    pr, R = problem, device_fit
    Q = fit(ctx, pr, "B", absolute_sigma=False)
    assert np.array_equal(Q[0], R[0])
    m, nf = pr["Y"].shape[1], 4
    for b, r in enumerate(R[2]):
        np.testing.assert_allclose(Q[1][b], R[1][b] * (r.obj_value / (m - nf)), rtol=1e-13, atol=0)
    # pinv(J^T J) of the deviance-residual Jacobian: J^T J = sum_i c_i^2 dmu dmu^T
    M = models.compose(pr["spec"])
    c = models.poisson_transform(M.f(pr["x"], R[0]), pr["Y"])[1]
    Jm = M.jac(pr["x"], R[0])
    C = np.linalg.inv(np.einsum("bi,bij,bik->bjk", c * c, Jm, Jm))
    d = np.sqrt(np.einsum("bii->bi", C))
    dd = d[:, :, None] * d[:, None, :]
    np.testing.assert_allclose(R[1] / dd, C / dd, rtol=0, atol=1e-6)


def test_finite_differences_reach_the_same_optimum(ctx, problem, device_fit):
    """jac='2-point' / '3-point': FdJacobian on the device with the Poisson kernel as fun (reps = n, f only), against the
    analytic route at the suite's figure for FD against analytic."""
    for jac in ("2-point", "3-point"):
        fd = fit(ctx, problem, "B", jac=jac)
        assert all(r.success for r in fd[2])
        np.testing.assert_allclose(fd[0], device_fit[0], rtol=1e-4, atol=1e-7)


def test_fixed_and_tied_through_the_mapped_instance(ctx, problem):
    """fixed= (the width held at p0) and, on 'gauss*2+poly*1', tied= (the second line's width a copy of the first's):
    the mapped Poisson instance (B) against the callables (A); the score of the nf variables vanishes."""
    pr = problem
    A, R = fit(ctx, pr, "A", fixed=[2]), fit(ctx, pr, "B", fixed=[2])
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "fixed")
    assert np.array_equal(R[0][:, 2], pr["P0"][:, 2]) and np.all(R[1][:, 2, :] == 0)
    pm = ParamMap(4, [2], None)
    S, T = pc.score(pr["spec"], pr["x"], pr["Y"], R[0], pm)
    assert np.all(np.abs(S) < 1e-6 * T)
    # two lines with one width
    two = pc.fit_problem(two=True)
    A, R = fit(ctx, two, "A", tied={5: 2}), fit(ctx, two, "B", tied={5: 2})
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "tied")
    assert np.array_equal(R[0][:, 5], R[0][:, 2])
    pm = ParamMap(7, None, {5: 2})
    S, T = pc.score(two["spec"], two["x"], two["Y"], R[0], pm)
    assert np.all(np.abs(S) < 1e-6 * T)


def test_robust_loss_over_deviance_residuals(ctx, problem):
    """loss='soft_l1' with outliers, A against B: the Jacobian callback after a judge writes the accepted problems only
    (the masked write of the Poisson instance)."""
    pr = dict(problem)
    pr["Y"] = pr["Y"].copy()
    pr["Y"][:, ::17] += 9.0                                                # outliers
    kw = dict(loss="soft_l1", f_scale=2.0)
    A, R = fit(ctx, pr, "A", **kw), fit(ctx, pr, "B", **kw)
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "soft_l1")
    for r in R[2]:
        assert r.deviance == pytest.approx(float(np.dot(r.fun, r.fun)), rel=1e-12) and r.obj_value < r.deviance


def test_leverage_and_dogbox(ctx, problem):
    pr = problem
    A, R = fit(ctx, pr, "A", method="dogbox", leverage=True), fit(ctx, pr, "B", method="dogbox", leverage=True)
    agree(A, R, "dogbox")
    for ra, rb in zip(A[2], R[2]):
        np.testing.assert_allclose(rb.leverage, ra.leverage, rtol=1e-6, atol=1e-9)
        assert abs(rb.leverage.sum() - 4) < 1e-6                           # trace of the hat matrix = n


def test_device_route_goes_through_the_new_entry_alone(ctx, problem, device_fit, monkeypatch):
    """Route B runs through run_device and blsq_model_eval_est_dev alone: run_host and the numpy functions raise, the
    three older entries are not called; and without the keyword the new entry is not called."""
    from bounded_lsq import _models, _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    monkeypatch.setattr(_models, "poisson_transform", boom)
    entries = me.count_entries(ctx, monkeypatch)
    got = fit(ctx, problem, "B")
    assert np.array_equal(got[0], device_fit[0]) and np.array_equal(got[1], device_fit[1])
    assert set(entries) == {"blsq_model_eval_est_dev"}
    entries.clear()
    bounded_lsq.curve_fit_batch(problem["spec"], problem["x"], problem["Y"], problem["P0"], bounds=problem["bounds"],
                                ctx=ctx, driver="device", **TOL)
    assert set(entries) == {"blsq_model_eval_comp_dev"}


def test_curve_fit_equals_the_batch_row(ctx, problem, device_fit):
    """``curve_fit(f, ..., estimator='poisson')`` on problem 3 alone, with the analytic Jacobian, with jac=None and with
    fixed=, against row 3 of the batch (rtol 1e-6 as between two routes; 1e-4 for finite differences)."""
    pr, b = problem, 3
    M = models.compose(pr["spec"])

    def f(t, a, mu, s, c):
        return M.f(t, np.array([[a, mu, s, c]]))[0]

    def jac(t, a, mu, s, c):
        return M.jac(t, np.array([[a, mu, s, c]]))[0]
    common = dict(p0=pr["P0"][b], bounds=(pr["bounds"][0][b], pr["bounds"][1][b]), estimator="poisson", **TOL)
    popt, pcov, info, msg, ier = bounded_lsq.curve_fit(f, pr["x"], pr["Y"][b], jac=jac, absolute_sigma=True,
                                                       full_output=True, **common)
    np.testing.assert_allclose(popt, device_fit[0][b], rtol=1e-6, atol=1e-9)
    d = np.sqrt(np.diag(device_fit[1][b]))
    np.testing.assert_allclose(pcov / np.outer(d, d), device_fit[1][b] / np.outer(d, d), rtol=0, atol=1e-6)
    np.testing.assert_allclose(info["fvec"], device_fit[2][b].fun, rtol=1e-6, atol=1e-7)
    popt_q, pcov_q = bounded_lsq.curve_fit(f, pr["x"], pr["Y"][b], jac=jac, **common)
    dev = float(np.dot(info["fvec"], info["fvec"]))
    np.testing.assert_allclose(pcov_q, pcov * (dev / (96 - 4)), rtol=1e-9)
    popt_fd, _ = bounded_lsq.curve_fit(f, pr["x"], pr["Y"][b], **common)
    np.testing.assert_allclose(popt_fd, device_fit[0][b], rtol=1e-4, atol=1e-7)
    Rf = fit(ctx, pr, "B", fixed=[2])
    popt_f, pcov_f = bounded_lsq.curve_fit(f, pr["x"], pr["Y"][b], jac=jac, absolute_sigma=True, fixed=[2], **common)
    np.testing.assert_allclose(popt_f, Rf[0][b], rtol=1e-6, atol=1e-9)
    assert popt_f[2] == pr["P0"][b, 2] and np.all(pcov_f[2] == 0)
