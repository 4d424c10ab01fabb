"""Bin-integrated fit models on the GPU: the BINNED kernel instances behind blsq_model_eval_bin_dev against
the numpy definition ``models.binned``, the entry with BLSQ_SAMPLE_POINT bit for bit against blsq_model_eval_est_dev, and
``curve_fit_batch(..., binned=True)`` end to end on histogram data across its routes."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import ParamMap, models

import _binned_cases as bc
import _model_eval as me
from _model_eval import Dev, agree, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
LSE, POISSON = 0, 1                                    # BLSQ_EST_*
POINT, BIN = 0, 1                                      # BLSQ_SAMPLE_*
EPS = bc.EPS


# ---- kernel level --------------------------------------------------------------------------------------------------
def eval_bin(ctx, label, est, sampling, reps, m, x, per_problem, y, w, X, Pfix=None, want_f=True, want_J=False,
             mask=None, fill=None, entry="bin"):
    """blsq_model_eval_bin_dev for the instance `label` on host arrays -> (rc, f or None, J or None); entry='est': the
    same call (without the sampling) through blsq_model_eval_est_dev.  fill: the value f and J hold before."""
    M, pm = bc.model_of(label), bc.map_of(label)
    n = bc.INSTANCES[label][1]
    nc = n if pm is None else pm.nf
    Q = bc.B * reps
    return me.run(ctx, "blsq_model_eval_%s_dev" % entry, (Q, m), (Q, m, nc), want_f, want_J,
                  np.nan if fill is None else fill, est=est, sampling=sampling, **me.model_args(M), B=bc.B, reps=reps,
                  m=m, n=n, nf=nc, pmap=None if pm is None else pm.pmap, t=x,
                  t_stride=(2 if sampling == BIN else 1) * M.coords * m if per_problem else 0, y=y, w=w,
                  w_stride=me.w_stride(w, m), X=X, Pfix=Pfix if pm is not None else None, mask=mask)


def test_device_functions_stay_inside_their_allowance(ctx):
    """The device's exp, erf, erfc, atan2 and expm1 against numpy's / scipy.special's float64 on the same arguments, each
    seen through a one-term bin-integrated model whose output is that function times exactly known factors, over a dense
    grid: the worst difference in ulp of the value.  ``_binned_cases.DEVICE_ULP`` records what an MI355X gave; the
    kernel bound of the next test allows each function twice that, and so does this test.
        erf    'gauss*1', a = s = 1, mu = 0, bins that straddle 0: value = sqrt(pi / 2) (erf(xh) - erf(xl)), in units of
               sqrt(pi / 2) (|erf(xh)| + |erf(xl)|), less 2 for the subtraction and the product
        erfc   the same with both edges in one tail, 0.05 <= |zl| <= 30, each erfc value weighted by
               ``_binned_cases.erfc_weight`` (1 + x^2: scipy's erfc squares its argument before exp, so the definition's
               own error grows like that; unweighted the two differ by 125 eps near x = 20)
        exp    column mu of the same model: e_l - e_h, in units of e_l + e_h, less 1
        atan2  'lorentz*1', a = s = 1, mu = 0: the value is atan2(w, 1 + zh zl) itself
        expm1  'exp*1', a = 1, lo = 0, hi = 1: w times -expm1(-x) / x, |x| >= 1 / 2, less 2 for the quotient and the product"""
    rng = np.random.default_rng(17)
    G = 4096
    seen = {}

    def run(label_spec, n, x, P):
        M = models.compose(label_spec)
        m = x.shape[-1]
        rc, f, J = me.run(ctx, "blsq_model_eval_bin_dev", (1, m), (1, m, n), True, True, 0.0, strict=True, est=LSE,
                          sampling=BIN, **me.model_args(M), B=1, reps=1, m=m, n=n, nf=n, pmap=None, t=x, t_stride=0,
                          y=None, w=None, w_stride=0, X=P, Pfix=None, mask=None)
        assert rc == 0
        return f[0], J[0]
    # erf: straddling bins; erfc: both edges in one tail (either sign)
    lo = -rng.uniform(0.0, 6.0, G)
    x_mid = np.stack([lo, rng.uniform(0.0, 6.0, G)])
    zl = np.exp(rng.uniform(np.log(0.05), np.log(30.0), G))
    x_tail = np.stack([zl, np.minimum(zl * (1 + rng.uniform(1e-3, 1.0, G)), 36.0)])         # erfc stays a normal number
    x_tail[:, ::2] = -x_tail[::-1, ::2]
    P = np.array([[1.0, 0.0, 1.0]])
    for key, x in (("erf", x_mid), ("erfc", x_tail)):
        f, J = run("gauss*1", 3, x, P)
        ref = models.binned("gauss*1").f(x, P)[0]
        xa, xb = x[0] * models.SQRT_HALF, x[1] * models.SQRT_HALF
        a, b, _ = bc.erf_parts(xa, xb)
        if key == "erfc":                            # in units that grow with the definition's own error in the tail
            a, b = a * bc.erfc_weight(xa), b * bc.erfc_weight(xb)
        unit = EPS * models.SQRT_PI_2 * (np.abs(a) + np.abs(b))
        seen[key] = max(0.0, float(np.max(np.abs(f - ref) / unit)) - (2 if key == "erf" else 0))
        el, eh = np.exp(-0.5 * (x[0] * x[0])), np.exp(-0.5 * (x[1] * x[1]))
        ok = (el + eh) > 0
        e_ulp = float(np.max(np.abs(J[:, 1] - (el - eh))[ok] / (EPS * (el + eh)[ok]))) - 1
        seen["exp"] = max(seen.get("exp", 0.0), e_ulp)
    x = np.stack([rng.uniform(-30.0, 30.0, G), np.zeros(G)])
    x[1] = x[0] + np.exp(rng.uniform(np.log(1e-3), np.log(30.0), G))
    f, _ = run("lorentz*1", 3, x, P)
    ref = models.binned("lorentz*1").f(x, P)[0]
    seen["atan2"] = float(np.max(np.abs(f - ref) / (EPS * np.abs(ref))))
    # expm1: bins [0, w] at r = +-1, so that x = r w runs over both signs
    hi = np.concatenate([np.exp(rng.uniform(np.log(0.5), np.log(40.0), G // 2)),
                         -np.exp(rng.uniform(np.log(0.5), np.log(40.0), G // 2))])
    for r, sel in ((1.0, hi > 0), (-1.0, hi < 0)):
        xb = np.stack([np.zeros(sel.sum()), np.abs(hi[sel])])
        Pe = np.array([[1.0, r]])
        f, _ = run("exp*1", 2, xb, Pe)
        ref = models.binned("exp*1").f(xb, Pe)[0]
        seen["expm1"] = max(seen.get("expm1", 0.0), float(np.max(np.abs(f - ref) / (EPS * np.abs(ref)))) - 2)
    print("device functions against numpy, worst ulp: " + ", ".join("%s %.2f" % kv for kv in sorted(seen.items())))
    for key, v in seen.items():
        assert v <= bc.ALLOW[key], (key, v, bc.ALLOW[key])


@pytest.mark.parametrize("m", bc.ROWS)
@pytest.mark.parametrize("label", list(bc.INSTANCES))
def test_kernel_against_definition(ctx, label, m):
    """f and J of blsq_model_eval_bin_dev (BLSQ_SAMPLE_BIN) against the float64 numpy definition ``models.binned``, under
    both estimators: B = 3, reps 1 (f and J together, f alone, J alone: the same bits) and 3 (f), edges shared
    (contiguous bins, t_stride 0) and per problem (bins with gaps, t_stride 2 m; gauss2d 4 m), m across the 64-row tile.
    Instances: gauss_sum (n = 7), lorentz_sum (7), exp_sum (5), poly (4), gauss2d, gauss_sum with one parameter fixed and
    one tied, 'gauss+pvoigt+exp+poly*2' and its mapped form.  Problem 1 of every instance has a peak 30 s outside the
    edges, so every lane takes the erfc branch for it; problems 1 and 2 have decays at r = 1e-9 and r = 0 (the series).

    The bound is derived per entry by ``_binned_cases.expected``: the definition's operations are repeated on values that
    carry a first-order bound of the device's difference.  The kernel performs those operations in that order without
    contraction, so an operation on operands with equal bits gives equal bits (bound 0: polynomials and the Lorentzian's
    column mu must agree exactly); a device function at an exact argument is within its allowance A ulp of numpy's
    (``ALLOW``: twice the figure measured on an MI355X by the test above); every later operation propagates its operands'
    bounds to first order and adds eps |result| for the two roundings.  So the bound of a row is the sum over its terms of
    their magnitudes (the summands' absolute values, not the cancelled result) times A eps and the roundings behind it.
    Under Poisson the transform's own roundings are counted as in tests/test_poisson_gpu.py.

    Measured (MI355X), worst difference / bound per instance over these cases, in the order of INSTANCES: 0.685, 0.560,
    0.469, 0.074, 0.556, 0.687, 0.742, 0.680."""
    worst, where = 0.0, None
    for est in (LSE, POISSON):
        for reps, per_problem in ((1, False), (1, True), (3, False), (3, True)):
            case = bc.kernel_case(label, m, reps, per_problem)
            f_ref, J_ref, f_tol, J_tol = bc.expected(label, case, est, reps)
            y, w = (case["ylse"], case["w"]) if est == LSE else (case["y"], None)
            want_J = reps == 1
            args = (ctx, label, est, BIN, reps, m, case["x"], per_problem, y, w, case["X"], case["Pfix"])
            rc, f, J = eval_bin(*args, True, want_J)
            assert rc == 0
            assert np.all(np.isfinite(f))
            ratios = [("f", bc.worst_ratio(f, f_ref, f_tol))]
            if want_J:
                ratios.append(("J", bc.worst_ratio(J, J_ref, J_tol)))
                rc, f1, _ = eval_bin(*args, True, False)
                assert rc == 0 and np.array_equal(f, f1)
                rc, _, J1 = eval_bin(*args, False, True)
                assert rc == 0 and np.array_equal(J, J1)
            for what, r in ratios:
                if r > worst:
                    worst, where = r, (est, reps, per_problem, what)
    print("binned %s m=%d: worst difference / bound  %.3f" % (label, m, worst))
    assert worst <= 1.0, (label, m, worst, where)


@pytest.mark.parametrize("label", list(bc.INSTANCES))
def test_point_sampling_through_the_new_entry_is_bit_for_bit(ctx, label):
    """BLSQ_SAMPLE_POINT: f and J of blsq_model_eval_bin_dev equal those of blsq_model_eval_est_dev on the same inputs in
    every bit, under both estimators; m = 130 and 65, reps 1 (f and J) and 3 (f).  The points are the lower edges."""
    for m, reps, per_problem in ((130, 1, True), (65, 1, False), (65, 3, True)):
        case = bc.kernel_case(label, m, reps, per_problem)
        t = np.ascontiguousarray(case["x"][..., 0::2, :]) if bc.model_of(label).coords == 2 else \
            np.ascontiguousarray(case["x"][..., 0, :])
        P, pm = case["P"], case["pm"]
        tr = np.repeat(t, reps, axis=0) if per_problem else t
        mu = bc.model_of(label).f(tr, P)[::reps]
        assert np.all(mu > 0)
        for est, y, w in ((LSE, case["ylse"], case["w"]), (LSE, None, None), (POISSON, np.floor(mu) + 1, None)):
            a = eval_bin(ctx, label, est, POINT, reps, m, t, per_problem, y, w, case["X"], case["Pfix"], True, reps == 1)
            b = eval_bin(ctx, label, est, POINT, reps, m, t, per_problem, y, w, case["X"], case["Pfix"], True, reps == 1,
                         entry="est")
            assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])
            assert reps != 1 or np.array_equal(a[2], b[2])
            assert np.all(np.isfinite(a[1]))


@pytest.mark.parametrize("label", ["gauss_sum", "gauss2d", "gauss_sum-map", "composite-map"])
def test_masked_problems_are_left_untouched(ctx, label):
    """mask = [1, 0, 1]: the masked problem keeps every bit of the sentinel in f and in J, the others keep none."""
    m = 130
    case = bc.kernel_case(label, m, 1, True)
    sentinel = -6.02214076e23
    args = (ctx, label, POISSON, BIN, 1, m, case["x"], True, case["y"], None, case["X"], case["Pfix"], True, True)
    rc, f, J = eval_bin(*args, mask=[1, 0, 1], fill=sentinel)
    assert rc == 0
    s = np.float64(sentinel)
    assert np.all(f[1].view(np.uint64) == s.view(np.uint64)) and np.all(J[1].view(np.uint64) == s.view(np.uint64))
    assert not np.any(f[[0, 2]] == s) and not np.any(J[[0, 2]] == s)
    rc, f_all, J_all = eval_bin(*args)
    assert np.array_equal(f[[0, 2]], f_all[[0, 2]]) and np.array_equal(J[[0, 2]], J_all[[0, 2]])


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, est = 2, sampling = 3, model = 4, ncomp = 5, fam = 6,
    cnt = 7, B = 8, reps, m, n = 11, nf = 12, pmap = 13, t = 14, t_stride = 15, y = 16, w = 17, w_stride, X = 19,
    Pfix = 20, f = 21, J = 22, mask; -24 / -25 for the contents of pmap); with BLSQ_SAMPLE_BIN t_stride is 0 or
    2 * coords * m.  Nothing is launched: the outputs keep their sentinel."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufP = d.up(np.arange(64.0)), d.up(np.ones(64))
        out, outJ = d.up(np.full(64, -7.0)), d.up(np.full(64, -7.0))

        def call(est=POISSON, sampling=BIN, model=2, fam=None, cnt=None, ncomp=None, B=1, reps=1, m=4, n=4, nf=4,
                 pmap=None, t=buf, ts=0, y=bufP, w=None, ws=0, X=bufP, Pfix=None, f=out, J=None):
            nc = ncomp if ncomp is not None else (0 if fam is None else len(fam))
            return me.call(ctx, "blsq_model_eval_bin_dev", True, est=est, sampling=sampling, model=model, ncomp=nc,
                           fam=fam, cnt=cnt, B=B, reps=reps, m=m, n=n, nf=nf, pmap=pmap, t=t, t_stride=ts, y=y, w=w,
                           w_stride=ws, X=X, Pfix=Pfix, f=f, J=J, mask=None)
        comp = dict(model=-1, fam=(0, 4), cnt=(1, 1))
        bad = [(dict(est=2), -2), (dict(sampling=2), -3), (dict(sampling=-1), -3), (dict(model=5), -4),
               (dict(model=-2), -4), (dict(ncomp=1), -5), (dict(model=-1), -5),
               (dict(model=-1, ncomp=2, cnt=(1, 1)), -6), (dict(model=-1, fam=(0, 5), cnt=(1, 1)), -6),
               (dict(model=-1, ncomp=2, fam=(0, 4)), -7), (dict(model=-1, fam=(0, 4), cnt=(0, 1)), -7),
               (dict(B=0), -8), (dict(reps=0), -9), (dict(m=0), -10),
               (dict(n=5, nf=5), -11), (dict(model=4, n=4), -11), (dict(n=5, nf=5, **comp), -11),
               (dict(nf=3), -12), (dict(nf=5, pmap=(0, 1, 2, 3)), -12), (dict(nf=3, **comp), -12),
               (dict(nf=3, pmap=(0, 1, 2, 3)), -24), (dict(nf=3, pmap=(0, 1, 1, -1), Pfix=bufP), -25),
               (dict(t=None), -14), (dict(ts=4), -15), (dict(ts=3), -15), (dict(sampling=POINT, ts=8), -15),
               (dict(model=4, n=5, nf=5, ts=8), -15), (dict(ts=4, **comp), -15),
               (dict(y=None), -16), (dict(w=buf), -17), (dict(est=LSE, w=buf, ws=3), -18),
               (dict(X=None), -19), (dict(nf=3, pmap=(0, 1, 2, -1)), -20), (dict(f=None), -21),
               (dict(reps=2, J=outJ), -22)]
        for kw, want in bad:
            assert call(**kw) == want, (kw, want)
        assert b"reps" in lib.blsq_last_error(h)
        assert call(ts=4) == -15 and b"2 * coords * m" in lib.blsq_last_error(h)
        assert call(sampling=2) == -3 and b"sampling" in lib.blsq_last_error(h)
        ctx.sync()
        assert np.all(ctx.to_host(out, (64,), np.float64) == -7.0) and np.all(ctx.to_host(outJ, (64,), np.float64) == -7.0)
        assert call(ts=8) == 0 and call(sampling=POINT, ts=4) == 0 and call(model=4, n=5, nf=5, ts=16) == 0
        assert call(J=outJ, ts=8, **comp) == 0 and call(est=LSE, y=None, w=buf, ws=4) == 0
        assert call(nf=3, pmap=(0, 1, 2, -1), Pfix=bufP, J=outJ) == 0
        ctx.sync()
        assert not np.any(ctx.to_host(out, (4,), np.float64) == -7.0)
    finally:
        d.close()


@pytest.mark.parametrize("label", ["gauss_sum", "gauss2d", "composite"])
def test_evaluate_binned_equals_the_definition(ctx, label):
    """``models.evaluate(..., binned=True)`` within the bound of test_kernel_against_definition (w = 1, y = 0), for shared
    and per-problem edges, and for the m + 1 contiguous edges given 1-D."""
    name = bc.INSTANCES[label][0]
    for per_problem in (False, True):
        case = bc.kernel_case(label, 65, 1, per_problem)
        got = models.evaluate(name, case["x"], case["P"], ctx=ctx, binned=True)
        v, _ = bc.q_model(label, case["x"], case["P"])
        assert bc.worst_ratio(got, v.v, v.e) <= 1.0
    if bc.model_of(label).coords == 1:
        case = bc.kernel_case(label, 65, 1, False)
        edges = np.append(case["x"][0], case["x"][1, -1])
        assert np.array_equal(models.evaluate(name, edges, case["P"], ctx=ctx, binned=True),
                              models.evaluate(name, case["x"], case["P"], ctx=ctx, binned=True))


# ---- end to end ----------------------------------------------------------------------------------------------------
def fit(ctx, f, x, pr, driver, **kw):
    common = dict(bounds=pr["bounds"], ctx=ctx, binned=True, **bc.TOL)
    common.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(f, x, pr["Y"], pr["P0"], driver=driver, **common)


def test_noise_free_fit_recovers_the_truth_on_both_drivers(ctx):
    """The problem of the table in DESIGN.md 7n at bins 1.5 s wide (tests/test_binned_cpu.py): driver='device' and driver='host'
    with binned=True recover all four parameters to 1e-9 and agree in popt and pcov; the same data fitted point-sampled
    at the centres against y / w has |s / s_true - 1| > 0.05."""
    pr = bc.table_problem()
    D = fit(ctx, pr["name"], pr["edges"], pr, "device")
    H = fit(ctx, pr["name"], pr["edges"], pr, "host")
    for R in (D, H):
        assert all(r.success for r in R[2])
        assert np.all(np.abs(R[0] / pr["truth"] - 1) < 1e-9)
    np.testing.assert_allclose(D[0], H[0], rtol=1e-6, atol=1e-9)
    pt = bounded_lsq.curve_fit_batch(pr["name"], pr["centres"], pr["Y"] / pr["width"], pr["P0"], bounds=pr["bounds"],
                                     ctx=ctx, driver="device", **bc.TOL)
    assert all(r.success for r in pt[2])
    assert np.all(np.abs(pt[0][:, 2] / pr["truth"][:, 2] - 1) > 0.05)
    # pcov of a noise-free fit is 0 / 0 in its variance factor: the routes are compared on a noisy copy
    noisy = dict(pr)
    noisy["Y"] = pr["Y"] + 0.05 * np.random.default_rng(1).standard_normal(pr["Y"].shape)
    agree(fit(ctx, pr["name"], pr["edges"], noisy, "host"), fit(ctx, pr["name"], pr["edges"], noisy, "device"), "lse")


@pytest.fixture(scope="module")
def histogram():
    return bc.histogram_problem()


@pytest.fixture(scope="module")
def device_fit(ctx, histogram):
    """The device route of the Poisson histogram fit, computed once and left unchanged."""
    pr = histogram
    return fit(ctx, pr["spec"], pr["edges"], pr, "device", estimator="poisson", absolute_sigma=True)


def test_poisson_histogram_routes_agree_and_reach_the_likelihood_optimum(ctx, histogram, device_fit):
    """B = 8 seeded Poisson histograms of 'gauss+poly*1' in bins 1.5 s wide, estimator='poisson', absolute_sigma=True:
    the kernel and the numpy definition on the host driver agree; the Poisson score of the bin-integrated model vanishes
    at the kernel's popt (|sum_i (1 - y_i / mu_i) dmu_i / dp_j| < 1e-6 sum_i |...|, the threshold and the solve tolerances
    of tests/test_poisson_gpu.py); nothing is on a bound."""
    pr, R = histogram, device_fit
    assert all(r.success for r in R[2]), [r.status for r in R[2]]
    H = fit(ctx, pr["spec"], pr["edges"], pr, "host", estimator="poisson", absolute_sigma=True)
    assert all(r.success for r in H[2])
    agree(H, R, "poisson")
    assert np.all(R[0] > pr["bounds"][0]) and np.all(R[0] < pr["bounds"][1])
    S, A = bc.binned_score(pr["spec"], pr["edges"], pr["Y"], R[0])
    print("binned poisson fit: worst |score| / sum |summands| %.2e  nfev <= %d" % (float((np.abs(S) / A).max()),
                                                                                max(r.nfev for r in R[2])))
    assert np.all(np.abs(S) < 1e-6 * A)
    # the rows form with per-problem edges is the same fit
    rows = np.tile(models.bin_rows(pr["edges"]), (pr["Y"].shape[0], 1, 1))
    R2 = fit(ctx, pr["spec"], rows, pr, "device", estimator="poisson", absolute_sigma=True)
    assert np.array_equal(R2[0], R[0])


@pytest.mark.parametrize("kw", [dict(fixed=[2]), dict(tied={5: 2}), dict(jac="3-point"),
                                dict(loss="soft_l1", f_scale=2.0), dict(leverage=True), dict(method="dogbox")],
                         ids=["fixed", "tied", "3-point", "soft_l1", "leverage", "dogbox"])
def test_fit_options_compose_with_binned(ctx, histogram, kw):
    """One Poisson histogram fit each with fixed= and tied= (the mapped binned instance; tied on 'gauss*2+poly*1' with
    one width), jac='3-point', loss='soft_l1', leverage=True and method='dogbox': the device route against the host
    route."""
    pr = dict(histogram)
    spec = pr["spec"]
    if "tied" in kw:
        spec = "gauss*2+poly*1"
        rng = np.random.default_rng(4)
        ins = lambda a, v: np.concatenate([a[:, :3], np.broadcast_to(v, (a.shape[0], 3)), a[:, 3:]], axis=1)   # noqa: E731
        truth = ins(pr["truth"], [25.0, -2.5, 0.5])
        truth[:, 5] = truth[:, 2]
        pr["Y"] = rng.poisson(models.binned(spec).f(pr["edges"], truth)).astype(float)
        pr["P0"] = truth * 1.05
        pr["P0"][:, 5] = pr["P0"][:, 2]
        lb, ub = pr["bounds"]
        pr["bounds"] = (ins(lb, lb[0, :3]), ins(ub, ub[0, :3]))
    common = dict(estimator="poisson", absolute_sigma=True, **kw)
    D = fit(ctx, spec, pr["edges"], pr, "device", **common)
    H = fit(ctx, spec, pr["edges"], pr, "host", **common)
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    if kw.get("jac") == "3-point":
        np.testing.assert_allclose(D[0], H[0], rtol=1e-4, atol=1e-7)
    else:
        agree(H, D, kw)
    if "fixed" in kw:
        assert np.array_equal(D[0][:, 2], pr["P0"][:, 2]) and np.all(D[1][:, 2, :] == 0)
        S, T = bc.binned_score(spec, pr["edges"], pr["Y"], D[0], ParamMap(4, [2], None))
        assert np.all(np.abs(S) < 1e-6 * T)
    if "tied" in kw:
        assert np.array_equal(D[0][:, 5], D[0][:, 2])
    if "leverage" in kw:
        for rd, rh in zip(D[2], H[2]):
            np.testing.assert_allclose(rd.leverage, rh.leverage, rtol=1e-6, atol=1e-9)
            assert abs(rd.leverage.sum() - 4) < 1e-6


def test_pixel_integrated_gauss2d_under_poisson(ctx):
    """The estimator of localisation microscopy: a pixel-integrated gauss2d on an 8 x 8 grid of unit pixels (m = 64),
    estimator='poisson': device against host, the score vanishes, and the centre is found to a fraction of a pixel."""
    pr = bc.pixel_problem()
    D = fit(ctx, "gauss2d", pr["x"], pr, "device", estimator="poisson", absolute_sigma=True)
    H = fit(ctx, "gauss2d", pr["x"], pr, "host", estimator="poisson", absolute_sigma=True)
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    agree(H, D, "gauss2d")
    S, A = bc.binned_score("gauss2d", pr["x"], pr["Y"], D[0])
    assert np.all(np.abs(S) < 1e-6 * A)
    assert np.all(np.abs(D[0][:, 1:3] - pr["truth"][:, 1:3]) < 5 * np.sqrt(np.einsum("bii->bi", D[1])[:, 1:3]))
    assert np.all(np.abs(D[0][:, 1:3] - pr["truth"][:, 1:3]) < 0.25)


def test_device_route_goes_through_the_new_entry_alone(ctx, histogram, device_fit, monkeypatch):
    """binned=True with driver='device' runs through run_device and blsq_model_eval_bin_dev alone, under either
    estimator: run_host and the numpy functions raise, no older entry is called; and without the keyword the new entry is
    not called."""
    from bounded_lsq import _models, _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    for cls in (_models.CompositeModel, _models.BinnedModel):
        monkeypatch.setattr(cls, "f", boom)
        monkeypatch.setattr(cls, "jac", boom)
    monkeypatch.setattr(_models, "poisson_transform", boom)
    entries = me.count_entries(ctx, monkeypatch)
    pr = histogram
    got = fit(ctx, pr["spec"], pr["edges"], pr, "device", estimator="poisson", absolute_sigma=True)
    assert np.array_equal(got[0], device_fit[0]) and np.array_equal(got[1], device_fit[1])
    assert set(entries) == {"blsq_model_eval_bin_dev"}
    entries.clear()
    fit(ctx, pr["spec"], pr["edges"], pr, "device", fixed=[2])
    assert set(entries) == {"blsq_model_eval_bin_dev"}
    entries.clear()
    centres = 0.5 * (pr["edges"][:-1] + pr["edges"][1:])
    bounded_lsq.curve_fit_batch(pr["spec"], centres, pr["Y"], pr["P0"], bounds=pr["bounds"], ctx=ctx, driver="device",
                                **bc.TOL)
    assert set(entries) == {"blsq_model_eval_comp_dev"}
