"""Composite fit models on the GPU: the composite kernel instances behind blsq_model_eval_comp_dev against
the numpy definition in extended precision and, bit for bit, against the closed families and their own unmapped form,
and ``curve_fit_batch(spec)`` end to end against the same definition passed as numpy callables."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import ParamMap, models

import _composite_cases as cc
import _model_cases as mc
import _model_eval as me
from _model_eval import Dev, agree, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble


# ---- kernel level --------------------------------------------------------------------------------------------------
def eval_comp(ctx, spec, B, reps, m, x, per_problem, y, w, X, want_f=True, want_J=False, mask=None, fill=None,
              pmap=None, nf=None, Pfix=None):
    """blsq_model_eval_comp_dev on host arrays -> (rc, f or None, J or None).  fill: the value f and J hold before.
    pmap: None (unmapped: X is P) or the int map [n] with nf and Pfix."""
    M = models.compose(spec)
    Q = B * reps
    nc = M.n if pmap is None else nf
    return me.run(ctx, "blsq_model_eval_comp_dev", (Q, m), (Q, m, nc), want_f, want_J, np.nan if fill is None else fill,
                  strict=True, **me.model_args(M), B=B, reps=reps, m=m, n=M.n, nf=nc, pmap=pmap, t=x,
                  t_stride=m if per_problem else 0, y=y, w=w, w_stride=me.w_stride(w, m), X=X, Pfix=Pfix, mask=mask)


def eval_named(ctx, name, B, m, n, x, per_problem, P):
    """f and J of blsq_model_eval_dev (y = w = NULL)."""
    rc, f, J = me.run(ctx, "blsq_model_eval_dev", (B, m), (B, m, n), True, True, strict=True, model=models.get(name).id,
                      B=B, reps=1, m=m, n=n, t=x, t_stride=m if per_problem else 0, y=None, w=None, w_stride=0, X=P,
                      mask=None)
    assert rc == 0
    return f, J


@pytest.mark.parametrize("m", cc.ROWS)
@pytest.mark.parametrize("spec", cc.KERNEL_SPECS)
def test_kernel_against_longdouble(ctx, spec, m):
    """f and J of blsq_model_eval_comp_dev against the numpy definition evaluated in np.longdouble, over B in {1, 3},
    reps in {1, 3} (f only when reps > 1), t shared and per problem, w NULL / shared / per problem, y NULL and given;
    m crosses the 64-row tile and 'pvoigt*15+poly*4' is the width (n = 64) at which a workgroup holds a single wave.

    The bound, per entry (eps = 2^-52; K the total number of summands of the spec: every term and every monomial of
    a polynomial; arg_s the argument of the exponential of summand s, 0 where there is none; c_s and c_j the counts
    below; M_s and M_j the magnitude the entry is bounded relative to):

        |f - f_ref| <= 2 eps |w| [ sum_s M_s (c_s + K + 2 |arg_s|) + |y| ]
        |J - J_ref| <= 2 eps |w| M_j (c_j + K + 2 |arg_s(j)|)

    It is the bound of tests/test_models_gpu.py::test_kernel_against_longdouble, derived the same way:
      * gauss, lorentz, exp and poly evaluate the formulas of the closed families, operation by operation, so their
        counts are the ones derived there: M_s = |term_s|, c_s = 4; M_j = |d model / d p_j|, c_j = 8; the exponential's
        argument carries one rounding with the factor 2 of slack, 2 |arg|; the K additions of the sum, each at most
        eps of a partial sum that sum_s M_s bounds, give the + K; - y and * w are part of c_s.  For 'gauss*K+poly*1'
        this is the bound of gauss_sum with K + 1 summands in place of K (test_composite_cpu.py checks that).
      * pvoigt, in units of eps, with z = (t - mu) / s (2 roundings), q = z z (2 * 2 + 1 = 5), arg = LN2 q (6, carried
        as 2 |arg| like every exponent's argument):
          G = exp(-arg): 1 (+ 2 |arg|);  L = 1 / (1 + q): 1 + q is 5 + 1, the quotient 1 more: 7;
          d = L - G cancels at the peak centre, so its error is taken relative to L + G: max(7, 1 + 2 |arg|) and its
            own rounding: 8 + 2 |arg|;  eta d: 9 + 2 |arg| relative to |eta| (L + G);
          h = G + eta d: relative to S_h = G + |eta| (L + G): 9 + 2 |arg| and its own rounding: 10 + 2 |arg|;
          the term a h: 11, and - y, * w as for every summand 2 more: c_s = 13 with M_s = |a| S_h;
          column a = w h: c_j = 11, M_j = S_h;   column eta = w (a d): 8 + 1 + 1: c_j = 10, M_j = |a| (L + G);
          lg = LN2 G: 2 (+ 2 |arg|);  L L: 15;  L L - lg cancels likewise: relative to L L + lg: 15 and its own: 16;
          eta (..): 17;  u = lg + eta (..): relative to S_u = lg + |eta| (L L + lg): 17 and its own: 18;
          column mu = w (((2 a) u) z) / s: 2 a exact, * u: 1, * z: 2 + 1, / s: 1, * w: 1: c_j = 18 + 6 = 24 with
            M_j = |2 a z / s| S_u;   column s = w (dmu z): 2 + 1 more: c_j = 27 with M_j = |2 a z^2 / s| S_u.
    The factor 2 in front is the slack over this count.  The float64 numpy definition meets the same bound on the same
    inputs (tests/test_composite_cpu.py::test_float64_numpy_meets_the_kernel_bound), which shows it attainable; the
    kernel may differ from numpy in the last bit of exp() only.  J computed with f = NULL gives the bits of J computed
    with f.

    Measured (MI355X), worst error / bound per spec over these cases, in the order of KERNEL_SPECS: 0.265, 0.206,
    0.137, 0.203, 0.063, 0.159."""
    worst = 0.0
    for variant in cc.VARIANTS:
        B, per_problem, reps, wk, yk = variant
        x, P, w, y = cc.variant_inputs(spec, m, variant)
        f_ref, J_ref, f_tol, J_tol = cc.bounds_of(spec, x, P, w, y, reps=reps)
        want_J = reps == 1
        rc, f, J = eval_comp(ctx, spec, B, reps, m, x, per_problem, y, w, P, True, want_J)
        assert rc == 0
        rf = cc.worst_ratio(f, f_ref, f_tol)
        worst = max(worst, rf)
        assert rf <= 1.0, (spec, m, variant, "f", rf)
        if want_J:
            rj = cc.worst_ratio(J, J_ref, J_tol)
            worst = max(worst, rj)
            assert rj <= 1.0, (spec, m, variant, "J", rj)
            if not yk:                                         # J alone (f = NULL) gives the same bits
                rc, _, J2 = eval_comp(ctx, spec, B, 1, m, x, per_problem, None, w, P, False, True)
                assert rc == 0 and np.array_equal(J, J2)
    print("composite %s m=%d: worst error / bound  device %.3f" % (spec, m, worst))


@pytest.mark.parametrize("m", [65, 130])
@pytest.mark.parametrize("n", [4, 16, 64])
def test_bit_for_bit_against_the_closed_families(ctx, n, m):
    """'gauss*K+poly*1', 'lorentz*K+poly*1', 'exp*K+poly*1' and 'poly*n' through blsq_model_eval_comp_dev equal
    blsq_model_eval_dev of the family in f and J (K the largest with 3 K + 1 <= n, 2 K + 1 <= n)."""
    B = 3
    for fmt, name, width in (("gauss*%d+poly*1", "gauss_sum", 3), ("lorentz*%d+poly*1", "lorentz_sum", 3),
                             ("exp*%d+poly*1", "exp_sum", 2), ("poly*%d", "poly", 1)):
        K = n if name == "poly" else (n - 1) // width
        nn = n if name == "poly" else width * K + 1
        for per_problem in (False, True):
            x, P = mc.case_inputs(name, nn, B, m, seed=[n, m], per_problem=per_problem)
            f0, J0 = eval_named(ctx, name, B, m, nn, x, per_problem, P)
            rc, f, J = eval_comp(ctx, fmt % K, B, 1, m, x, per_problem, None, None, P, True, True)
            assert rc == 0 and np.array_equal(f, f0) and np.array_equal(J, J0), (name, nn, m, per_problem)


# the maps of the mapped tests, on 'gauss+lorentz+pvoigt+poly*2' (n = 12): a tie across components (the width of the
# lorentz to the width of the gauss), a fixed eta, a fixed poly coefficient, all three together, and the identity
MAP_SPEC = "gauss+lorentz+pvoigt+poly*2"
MAPS = {"tie": (None, {5: 2}), "eta": ([9], None), "coefficient": ([11], None), "all": ([9, 11], {5: 2, 7: 1}),
        "identity": (None, None)}


def check_mapped(ctx, spec, pm, B, m, seed):
    """The mapped instance against the unmapped one, with no tolerance: f at the expanded point, J reduced."""
    M = models.compose(spec)
    x, P = cc.comp_inputs(spec, B, m, seed=seed, per_problem=True)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, (B, m))
    y = rng.standard_normal((B, m))
    X = np.ascontiguousarray(pm.reduce_x(P))
    P_full = pm.expand_x(X, P)
    rc, f0, J0 = eval_comp(ctx, spec, B, 1, m, x, True, y, w, P_full, True, True)
    assert rc == 0
    rc, f, J = eval_comp(ctx, spec, B, 1, m, x, True, y, w, X, True, True, pmap=pm.pmap, nf=pm.nf, Pfix=P)
    assert rc == 0 and J.shape == (B, m, pm.nf)
    assert np.array_equal(f, f0), (spec, pm, m)
    assert np.array_equal(J, pm.reduce_jac(J0)), (spec, pm, m)
    rc, _, J2 = eval_comp(ctx, spec, B, 1, m, x, True, None, w, X, False, True, pmap=pm.pmap, nf=pm.nf, Pfix=P)
    assert rc == 0 and np.array_equal(J, J2)
    # reps > 1 (the finite-difference points): f only
    X3 = np.repeat(X, 3, axis=0) * (1 + 1e-3 * rng.standard_normal((3 * B, pm.nf)))
    rc, f3, _ = eval_comp(ctx, spec, B, 3, m, x, True, y, w, X3, True, False, pmap=pm.pmap, nf=pm.nf, Pfix=P)
    rc0, f30, _ = eval_comp(ctx, spec, B, 3, m, x, True, y, w, pm.expand_x(X3, np.repeat(P, 3, axis=0)), True, False)
    assert rc == 0 and rc0 == 0 and np.array_equal(f3, f30)
    return M


@pytest.mark.parametrize("m", [65, 130])
@pytest.mark.parametrize("label", list(MAPS))
def test_mapped_instance_bit_for_bit(ctx, label, m):
    fixed, tied = MAPS[label]
    pm = ParamMap(12, fixed, tied)
    check_mapped(ctx, MAP_SPEC, pm, 3, m, seed=[m, len(label)])


@pytest.mark.parametrize("nf", [22, 23, 24, 46, 47, 48, 63, 64])
def test_mapped_widths_across_the_lds_steps(ctx, nf):
    """n = 64 ('pvoigt*15+poly*4'): a wave's LDS is 512 (1 + (nf | 1)) bytes, so 48 KiB hold 4 waves up to nf = 22 / 23
    (12288 B each), 2 up to nf = 46 / 47 (24576 B) and 1 beyond; the widths on both sides of each step, by fixing
    64 - nf parameters (etas first, then widths tied to the first width)."""
    spec = "pvoigt*15+poly*4"
    drop = 64 - nf
    etas = [4 * k + 3 for k in range(15)]
    widths = [4 * k + 2 for k in range(1, 15)]
    centres = [4 * k + 1 for k in range(15)]
    fixed = etas[:min(drop, 15)]
    tied = {j: 2 for j in widths[:max(0, min(drop - 15, 14))]}
    fixed += centres[:max(0, drop - 29)]
    pm = ParamMap(64, fixed or None, tied or None)
    assert pm.nf == nf
    check_mapped(ctx, spec, pm, 2, 70, seed=[nf])


@pytest.mark.parametrize("spec,m,mapped", [("gauss+poly*2", 65, False), ("gauss*2+lorentz+pvoigt+poly*3", 130, False),
                                           ("pvoigt*15+poly*4", 70, False), (MAP_SPEC, 130, True)])
def test_masked_problems_are_left_untouched(ctx, spec, m, mapped):
    """mask = [1, 0, 1]: the masked problem keeps every bit of the sentinel in f and in J, the others keep none."""
    B = 3
    M = models.compose(spec)
    x, P = cc.comp_inputs(spec, B, m, seed=5, per_problem=True)
    kw = {}
    X = P
    if mapped:
        pm = ParamMap(M.n, *MAPS["all"])
        X = np.ascontiguousarray(pm.reduce_x(P))
        kw = dict(pmap=pm.pmap, nf=pm.nf, Pfix=P)
    sentinel = -6.02214076e23
    rc, f, J = eval_comp(ctx, spec, B, 1, m, x, True, None, None, X, True, True, mask=[1, 0, 1], fill=sentinel, **kw)
    assert rc == 0
    s = np.float64(sentinel)
    assert np.all(f[1].view(np.uint64) == s.view(np.uint64)) and np.all(J[1].view(np.uint64) == s.view(np.uint64))
    assert not np.any(f[[0, 2]] == s) and not np.any(J[[0, 2]] == s)
    rc, f_all, J_all = eval_comp(ctx, spec, B, 1, m, x, True, None, None, X, True, True, **kw)
    assert np.array_equal(f[[0, 2]], f_all[[0, 2]]) and np.array_equal(J[[0, 2]], J_all[[0, 2]])


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, ncomp = 2, fam = 3, cnt = 4, B, reps, m, n = 8,
    nf = 9, pmap = 10, t = 11, t_stride, y, w, w_stride = 15, X = 16, Pfix = 17, f = 18, J = 19, mask; -21 / -22 for the
    contents of pmap); nothing is launched: the outputs keep their sentinel."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufP = d.up(np.zeros(64)), d.up(np.ones(64))
        out, outJ = d.up(np.full(64, -7.0)), d.up(np.full(64, -7.0))

        def call(fam=(0, 4), cnt=(1, 1), ncomp=None, B=1, reps=1, m=4, n=4, nf=4, pmap=None, t=buf, ts=0, y=None,
                 w=None, ws=0, X=bufP, Pfix=None, f=out, J=None):
            nc = ncomp if ncomp is not None else len(fam)
            return me.call(ctx, "blsq_model_eval_comp_dev", True, ncomp=nc, fam=fam, cnt=cnt, B=B, reps=reps, m=m, n=n,
                           nf=nf, pmap=pmap, t=t, t_stride=ts, y=y, w=w, w_stride=ws, X=X, Pfix=Pfix, f=f, J=J, mask=None)
        bad = [(dict(ncomp=0), -2), (dict(ncomp=9, fam=(4,) * 9, cnt=(1,) * 9, n=9, nf=9), -2),
               (dict(fam=None, ncomp=2), -3), (dict(fam=(0, 5)), -3), (dict(fam=(-1, 4)), -3),
               (dict(cnt=None), -4), (dict(cnt=(0, 1)), -4), (dict(cnt=(1, -2)), -4),
               (dict(B=0), -5), (dict(reps=0), -6), (dict(m=0), -7),
               (dict(n=5, nf=5), -8), (dict(n=3, nf=3), -8), (dict(fam=(4,), cnt=(65,), n=65, nf=65), -8),
               (dict(fam=(2, 4), cnt=(16, 1), n=65, nf=65), -8),
               (dict(nf=3), -9), (dict(nf=5), -9), (dict(nf=0, pmap=(0, 1, 2, 3)), -9), (dict(nf=5, pmap=(0, 1, 2, 3)), -9),
               (dict(nf=3, pmap=(0, 1, 2, 3)), -21), (dict(nf=3, pmap=(0, 1, -2, 2)), -21),
               (dict(nf=3, pmap=(0, 1, 1, -1), Pfix=bufP), -22),
               (dict(t=None), -11), (dict(ts=3), -12), (dict(ts=8), -12), (dict(w=buf, ws=3), -15), (dict(X=None), -16),
               (dict(nf=3, pmap=(0, 1, 2, -1)), -17), (dict(f=None), -18), (dict(reps=2, J=outJ), -19)]
        for kw, want in bad:
            assert call(**kw) == want, (kw, want)
        assert b"reps" in lib.blsq_last_error(h)
        ctx.sync()
        assert np.all(ctx.to_host(out, (64,), np.float64) == -7.0) and np.all(ctx.to_host(outJ, (64,), np.float64) == -7.0)
        assert call() == 0 and call(ts=4, ws=4, w=buf) == 0 and call(nf=3, pmap=(0, 1, 2, -1), Pfix=bufP, J=outJ) == 0
        ctx.sync()
        assert not np.any(ctx.to_host(out, (4,), np.float64) == -7.0)
    finally:
        d.close()


def test_evaluate_against_numpy(ctx):
    for spec in ("gauss*2+lorentz+pvoigt+poly*3", "exp*2+poly*1"):
        for per_problem in (False, True):
            x, P = cc.comp_inputs(spec, 3, 70, seed=2, per_problem=per_problem)
            f_ref, _, f_tol, _ = cc.bounds_of(spec, x, P, None, None)
            for arg in (spec, models.compose(spec)):
                got = models.evaluate(arg, x, P, ctx=ctx)
                assert got.shape == (3, 70)
                assert np.all(np.abs(got.astype(LD) - f_ref) <= f_tol), spec
                np.testing.assert_allclose(got, models.compose(spec).f(x, P), rtol=1e-13, atol=1e-14)
    with pytest.raises(ValueError, match="does not take n"):
        models.evaluate("gauss+poly*1", np.zeros(5), np.ones((2, 5)), ctx=ctx)


# ---- end to end ----------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)


def fit(ctx, pr, route, method, **kw):
    """route A: the numpy definition as callables, driver='device'; B: the spec, driver='device'; C: the spec,
    driver='host'."""
    M = models.compose(pr["spec"])
    common = dict(sigma=cc.SIGMA, bounds=pr["bounds"], method=method, ctx=ctx, tied=pr["tied"], **TOL)
    common.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if route == "A":
            return bounded_lsq.curve_fit_batch(M.f, pr["x"], pr["Y"], pr["P0"], jac=M.jac, driver="device", **common)
        return bounded_lsq.curve_fit_batch(pr["spec"], pr["x"], pr["Y"], pr["P0"],
                                           driver="device" if route == "B" else "host", **common)


@pytest.fixture(scope="module")
def reference_fits(ctx):
    """Route A of every (problem, m, method), computed once and left unchanged."""
    cache = {}

    def get(label, m, method):
        key = (label, m, method)
        if key not in cache:
            pr = cc.fit_problem(label, m)
            cache[key] = (pr, fit(ctx, pr, "A", method))
        return cache[key]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("m", cc.FIT_ROWS)
@pytest.mark.parametrize("label", list(cc.FITS))
def test_fit_by_spec_agrees_with_the_callable(ctx, reference_fits, label, m, method):
    """B = 8 problems each (test_composite_cpu.py vets them with scipy): the spec on the device (B) and on the host
    (C) against the numpy definition as callables on the device driver (A): every problem succeeds on every route,
    popt to rtol 1e-6 / atol 1e-9 and the normalised pcov to 1e-6 (the figures of tests/test_models_gpu.py for two
    routes of one problem)."""
    pr, A = reference_fits(label, m, method)
    assert all(r.success for r in A[2]), [r.status for r in A[2]]
    fits = {}
    for route in ("B", "C"):
        R = fit(ctx, pr, route, method)
        assert all(r.success for r in R[2]), (route, [r.status for r in R[2]])
        agree(A, R, (label, m, method, route))
        fits[route] = R
    popt = fits["B"][0]
    lb, ub = pr["bounds"]
    assert np.all(popt >= lb) and np.all(popt <= ub)
    for j, i in (pr["tied"] or {}).items():
        assert np.array_equal(popt[:, j], popt[:, i])
    # results[b].fun is the weighted residual at popt
    M = models.compose(pr["spec"])
    np.testing.assert_allclose(np.stack([r.fun for r in fits["B"][2]]), (M.f(pr["x"], popt) - pr["Y"]) / cc.SIGMA,
                               rtol=1e-9, atol=1e-9)


def test_fixed_eta_and_composite_object(ctx):
    """fixed= on a composite (eta held at p0), and a CompositeModel in place of the spec."""
    pr = cc.fit_problem("pvoigt", 70)
    pr["P0"][:, 3] = pr["truth"][:, 3]
    A = fit(ctx, pr, "A", "trf", fixed=[3])
    R = fit(ctx, pr, "B", "trf", fixed=[3])
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "fixed eta")
    assert np.array_equal(R[0][:, 3], pr["P0"][:, 3]) and np.all(R[1][:, 3, :] == 0)
    R2 = bounded_lsq.curve_fit_batch(models.compose(pr["spec"]), pr["x"], pr["Y"], pr["P0"], sigma=cc.SIGMA,
                                     bounds=pr["bounds"], driver="device", ctx=ctx, fixed=[3], **TOL)
    assert np.array_equal(R2[0], R[0]) and np.array_equal(R2[1], R[1])


def test_robust_loss_by_spec(ctx):
    """loss='soft_l1' with outliers, A against B: the Jacobian callback after a judge writes the accepted problems
    only (the masked write of the kernel)."""
    pr = cc.fit_problem("slope", 70)
    pr["Y"][:, ::9] += 0.3                                                 # outliers
    kw = dict(loss="soft_l1", f_scale=2.0)
    A = fit(ctx, pr, "A", "trf", **kw)
    R = fit(ctx, pr, "B", "trf", **kw)
    assert all(r.success for r in A[2]) and all(r.success for r in R[2])
    agree(A, R, "soft_l1")


def test_finite_differences_by_spec(ctx):
    """jac='2-point' / '3-point': FdJacobian on the device with the kernel as fun (reps = nf), against the analytic
    route at the suite's figure for FD against analytic; with a tie, so through the mapped instance."""
    for label in ("slope", "tied"):
        pr = cc.fit_problem(label, 33)
        an = fit(ctx, pr, "B", "trf")
        for jac in ("2-point", "3-point"):
            fd = fit(ctx, pr, "B", "trf", jac=jac)
            assert all(r.success for r in fd[2])
            np.testing.assert_allclose(fd[0], an[0], rtol=1e-4, atol=1e-7)


def test_leverage_by_spec(ctx):
    for label, nf in (("pvoigt", 6), ("tied", 6)):
        pr = cc.fit_problem(label, 33)
        A = fit(ctx, pr, "A", "dogbox", leverage=True)
        R = fit(ctx, pr, "B", "dogbox", leverage=True)
        for ra, rb in zip(A[2], R[2]):
            assert rb.leverage.shape == (33,)
            np.testing.assert_allclose(rb.leverage, ra.leverage, rtol=1e-6, atol=1e-9)
            assert abs(rb.leverage.sum() - nf) < 1e-6                      # trace of the hat matrix = nf


def test_spec_device_route_calls_no_host_callback(ctx, monkeypatch):
    """Route B runs through run_device alone, and through the composite entry alone: run_host raises, and so do the
    numpy functions of the composite and of its terms."""
    from bounded_lsq import _models, _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    pr = cc.fit_problem("tied", 33)
    want = fit(ctx, pr, "B", "trf")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    for T in _models.TERMS.values():
        monkeypatch.setattr(T, "fill", boom)
    calls = []
    real = _outer.OuterDriver.run_device
    monkeypatch.setattr(_outer.OuterDriver, "run_device",
                        lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    counts = me.count_entries(ctx, monkeypatch)
    got = fit(ctx, pr, "B", "trf")
    entries = {"comp": counts.get("blsq_model_eval_comp_dev", 0),
               "named": counts.get("blsq_model_eval_dev", 0) + counts.get("blsq_model_eval_map_dev", 0)}
    assert calls == [1] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert entries["comp"] > 0 and entries["named"] == 0
    got_fd = fit(ctx, pr, "B", "trf", jac="2-point")
    assert calls == [1, 1] and all(r.success for r in got_fd[2])
    with pytest.raises(AssertionError, match="host callback"):
        fit(ctx, pr, "C", "trf")
