"""Fixed and tied parameters on the GPU: the mapped kernel instances (blsq_model_eval_map_dev) bit for bit against the
existing entry, and ``curve_fit_batch(f='name', fixed=, tied=)`` end to end against the reduced model written out by hand
— as numpy callables on the device driver (the route a user has without the keywords) and through scipy."""
import warnings

import numpy as np
import pytest
import scipy.optimize as so

import bounded_lsq
from bounded_lsq import models
from bounded_lsq._params import ParamMap

import _model_cases as mc
import _param_map_cases as pc
import _model_eval as me
from _model_eval import Dev, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu


# ---- kernel level --------------------------------------------------------------------------------------------------
def eval_both(ctx, name, B, reps, m, n, x, per_problem, y, w, P_full, maps, want_J, mask=None, fill=np.nan):
    """blsq_model_eval_dev at P_full, and blsq_model_eval_map_dev for every (pmap, nf, X, Pfix) of `maps`, on one set of
    device copies of the data -> (f_full, J_full), [(f_map, J_map), ...]."""
    M = models.get(name)
    Q = B * reps
    with Dev(ctx) as d:
        data = dict(model=M.id, B=B, reps=reps, m=m, n=n, t=d.up(x), t_stride=M.coords * m if per_problem else 0,
                    y=d.up(y), w=d.up(w), w_stride=me.w_stride(w, m),
                    mask=d.up(None if mask is None else np.asarray(mask, dtype=np.int32)))

        def run(entry, width, **more):
            rc, f, J = me.run(ctx, entry, (Q, m), (Q, m, width), True, want_J, fill, dev=d, strict=True, **data, **more)
            assert rc == 0, ctx.lib.blsq_last_error(ctx.h)
            return f, J
        full = run("blsq_model_eval_dev", n, X=P_full)
        got = [run("blsq_model_eval_map_dev", nf, nf=nf, pmap=pmap, X=X, Pfix=Pfix) for pmap, nf, X, Pfix in maps]
        return full, got


def split(pm, P, reps):
    """Points P (Q, n) -> X (Q, nf), the template Pfix (B, n) — NaN wherever the entry must not read it — and the
    expanded P_full (Q, n) that satisfies the ties."""
    X = np.ascontiguousarray(pm.reduce_x(P))
    Pfix = np.where(pm.pmap < 0, P[::reps], np.nan)
    return X, Pfix, pm.expand_x(X, np.repeat(Pfix, reps, axis=0))


def check_bits(ctx, name, n, m, maps, Bs=(1, 3)):
    """Over B, reps in {1, 3} (f), t shared / per problem, w NULL / shared / per problem, y NULL / given: f of the mapped
    entry equals f of the existing entry at the expanded point, J equals the float64 sequential column sums of its J,
    bit for bit.  Every map is evaluated at its own expanded point (the ties change it)."""
    rng = np.random.default_rng([n, m, 11])
    checked = 0
    for B in Bs:
        W, Y = rng.uniform(0.5, 2.0, (B, m)), rng.standard_normal((B, m))
        for per_problem in (False, True):
            for reps in (1, 3):
                x, P = mc.case_inputs(name, n, B * reps, m, seed=[n, m, B, reps], per_problem=False)
                if per_problem:
                    x = mc.case_inputs(name, n, B, m, seed=[n, m, B, reps], per_problem=True)[0]
                for w in (None, W[0], W):
                    for y in (None, Y):
                        for pm in maps:
                            X, Pfix, P_full = split(pm, P, reps)
                            if not np.any(pm.pmap < 0):
                                Pfix = None                                    # (NULL is allowed without a fixed entry)
                            (f_full, J_full), [(f_map, J_map)] = eval_both(
                                ctx, name, B, reps, m, n, x, per_problem, y, w, P_full,
                                [(pm.pmap, pm.nf, X, Pfix)], want_J=reps == 1)
                            what = (name, n, m, pm.pmap.tolist(), B, reps, per_problem, np.ndim(w), y is not None)
                            assert np.all(np.isfinite(f_full)), what
                            assert np.array_equal(f_map, f_full), what
                            if reps == 1:
                                assert J_map.shape == (B, m, pm.nf)
                                assert np.array_equal(J_map, pm.reduce_jac(J_full)), what
                            checked += 1
    return checked


@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", list(pc.KERNEL_N))
def test_mapped_kernel_bit_for_bit_against_the_existing_entry(ctx, name, m):
    """No tolerance: the existing entry is pinned to its longdouble bound by test_kernel_against_longdouble, and the
    mapped instances must be that entry plus exact copies and one sequential float64 sum per tied group.  m crosses the
    64-row tile; the maps are `_param_map_cases.kernel_maps`."""
    n = pc.KERNEL_N[name]
    maps = [ParamMap(n, fixed, tied) for _, fixed, tied in pc.kernel_maps(name)]
    assert check_bits(ctx, name, n, m, maps) == 48 * len(maps)


class _Identity:
    """The map Python never sends: nothing fixed, nothing tied, as a full-width pmap."""

    def __init__(self, n):
        self.n = self.nf = n
        self.pmap = np.arange(n, dtype=np.int32)
        self.reduce_x = lambda P: P
        self.expand_x = lambda X, Pfix: X.copy()
        self.reduce_jac = lambda J: J


@pytest.mark.parametrize("nf", [1, 23, 24, 47, 48, 63])
def test_launch_shape_edges(ctx, nf):
    """gauss_sum with n = 64 (K = 21): 4 waves per workgroup up to nf = 23, 2 up to 47, 1 beyond — the tile is counted
    at nf | 1, plus the parameter vector.  m = 65 and 130: a workgroup of several waves holds items of two points."""
    pm = ParamMap(64, *pc.edge_map(nf))
    assert pm.nf == nf
    for m in (65, 130):
        check_bits(ctx, "gauss_sum", 64, m, [pm], Bs=(3,))


def test_identity_map_is_accepted(ctx):
    """n = 7, nf = 7, pmap = 0 .. 6 and Pfix = NULL: the entry then reproduces the existing one, J included."""
    for m in (1, 65):
        check_bits(ctx, "gauss_sum", 7, m, [_Identity(7)])


MASK_CASES = [("poly", 65), ("exp_sum", 64), ("gauss_sum", 130), ("lorentz_sum", 63), ("gauss2d", 64)]


@pytest.mark.parametrize("name,m", MASK_CASES)
def test_masked_problems_are_left_untouched(ctx, name, m):
    """mask = [1, 0, 1]: the masked problem keeps every bit of the sentinel in f and in J; the others are the unmasked
    call's."""
    n, B = pc.KERNEL_N[name], 3
    _, fixed, tied = [mp for mp in pc.kernel_maps(name) if mp[0] == "mixed"][0]
    pm = ParamMap(n, fixed, tied)
    x, P = mc.case_inputs(name, n, B, m, seed=5, per_problem=True)
    X, Pfix, P_full = split(pm, P, 1)
    sentinel = np.float64(-6.02214076e23)
    arg = [(pm.pmap, pm.nf, X, Pfix)]
    _, [(f, J)] = eval_both(ctx, name, B, 1, m, n, x, True, None, None, P_full, arg, True, mask=[1, 0, 1],
                            fill=sentinel)
    bits = sentinel.view(np.uint64)
    assert np.all(f[1].view(np.uint64) == bits) and np.all(J[1].view(np.uint64) == bits)
    assert not np.any(f[[0, 2]] == sentinel) and not np.any(J[[0, 2]] == sentinel)
    _, [(f_all, J_all)] = eval_both(ctx, name, B, 1, m, n, x, True, None, None, P_full, arg, True)
    assert np.array_equal(f[[0, 2]], f_all[[0, 2]]) and np.array_equal(J[[0, 2]], J_all[[0, 2]])


def test_argument_errors_name_the_argument(ctx):
    """A negative return is the index of the bad argument (ctx = 1, model, B, reps, m, n, nf = 7, pmap = 8, t,
    t_stride, y, w, w_stride, X = 14, Pfix = 15, f = 16, J = 17, mask), -19 / -20 for the contents of pmap; the message
    names the argument and nothing is launched."""
    lib, h = ctx.lib, ctx.h
    d = Dev(ctx)
    try:
        buf, bufX, bufF, out = d.up(np.zeros(64)), d.up(np.ones(64)), d.up(np.ones(64)), d.up(np.zeros(64))

        def call(model=2, B=1, reps=1, m=4, n=4, nf=2, pmap=(0, -1, 1, 1), t=buf, ts=0, y=None, w=None, ws=0, X=bufX,
                 F=bufF, f=out, J=None):
            return me.call(ctx, "blsq_model_eval_map_dev", True, model=model, B=B, reps=reps, m=m, n=n, nf=nf, pmap=pmap,
                           t=t, t_stride=ts, y=y, w=w, w_stride=ws, X=X, Pfix=F, f=f, J=J, mask=None)

        def err():
            return lib.blsq_last_error(h)
        assert call() == 0
        ctx.sync()
        assert call(model=5) == -2 and call(model=-1) == -2 and b"model" in err()
        assert call(B=0) == -3 and call(reps=0) == -4 and call(m=0) == -5
        assert call(n=5) == -6 and call(model=4, n=4) == -6 and b"n does not fit" in err()
        assert call(nf=0) == -7 and call(nf=5) == -7 and b"nf" in err()
        assert call(pmap=None) == -8 and b"pmap" in err()
        assert call(pmap=(0, -2, 1, 1)) == -19 and call(pmap=(0, 2, 1, 1)) == -19 and b"pmap entry" in err()
        assert call(pmap=(1, -1, 1, 1)) == -20 and call(nf=3) == -20 and b"unused" in err()
        assert call(t=None) == -9 and b"t is NULL" in err()
        assert call(ts=3) == -10 and b"t_stride" in err()
        assert call(w=buf, ws=3) == -13 and b"w_stride" in err()
        assert call(X=None) == -14 and b"X is NULL" in err()
        assert call(F=None) == -15 and b"Pfix" in err()
        assert call(F=None, pmap=(0, 1, 1, 1)) == 0                            # nothing fixed: Pfix may be NULL
        assert call(f=None) == -16 and b"f and J" in err()
        assert call(reps=2, J=out) == -17 and b"reps" in err()
        ctx.sync()
    finally:
        d.close()


# ---- end to end ----------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)


def fit_mapped(ctx, pr, fixed, tied, method, driver="device", **kw):
    """The named model with the keywords."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(pr["name"], pr["x"], pr["Y"], pr["P0"], sigma=mc.SIGMA, bounds=pr["bounds"],
                                           method=method, driver=driver, ctx=ctx, fixed=fixed, tied=tied,
                                           **dict(TOL, **kw))


def fit_r1(ctx, pr, red, method, **kw):
    """R1: the hand-written reduced model as numpy callables over nf parameters, on the device driver."""
    f, jac, _ = pc.reduced_callables(red, pr["P0"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(f, pr["x"], pr["Y"], pr["X0"], sigma=mc.SIGMA, bounds=pr["bounds_red"],
                                           method=method, jac=jac, driver="device", ctx=ctx, **dict(TOL, **kw))


def fit_r2(pr, red, method):
    """R2: scipy.optimize.curve_fit on the same reduced model, problem by problem -> popt (B, nf), pcov, max nfev."""
    _, _, single = pc.reduced_callables(red, pr["P0"])
    B, m = pr["Y"].shape
    popt, pcov, nfev = [], [], 0
    for b in range(B):
        fb, jb = single(b)
        p, c, info, _, ier = so.curve_fit(fb, pr["x"], pr["Y"][b], p0=pr["X0"][b], sigma=np.full(m, mc.SIGMA),
                                          bounds=(pr["bounds_red"][0][b], pr["bounds_red"][1][b]), method=method,
                                          jac=jb, full_output=True, **TOL)
        assert ier > 0
        popt.append(p)
        pcov.append(c)
        nfev = max(nfev, info["nfev"])
    return np.stack(popt), np.stack(pcov), nfev


def normalised(pcov, by=None):
    d = np.sqrt(np.einsum("bii->bi", pcov if by is None else by))
    return pcov / (d[:, :, None] * d[:, None, :])


@pytest.fixture(scope="module")
def references(ctx):
    """(problem, R1, R2) of every (case, m, method), computed once and left unchanged."""
    cache = {}

    def get(i, m, method):
        if (i, m, method) not in cache:
            label, fixed, tied, red, groups = pc.E2E_CASES[i]
            pr = pc.mapped_problem(label, m, fixed, tied, groups)
            cache[(i, m, method)] = (pr, fit_r1(ctx, pr, red, method), fit_r2(pr, red, method))
        return cache[(i, m, method)]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("m", [33, 70])
@pytest.mark.parametrize("i", range(len(pc.E2E_CASES)), ids=pc.E2E_IDS)
def test_mapped_fit_against_the_hand_reduced_model_and_scipy(ctx, references, i, m, method):
    """B = 8 problems per case; the named model with fixed= / tied= on the device against R1 (the reduced model by hand,
    numpy callables on the device driver) and R2 (scipy.optimize.curve_fit on the same reduced model):
      * every problem succeeds on every route;
      * reduce_x(popt) against R1 and against R2: rtol 1e-6 / atol 1e-9;
      * pcov normalised by sqrt(diag diag^T) against R1: 1e-6; against R2 the difference is normalised by R2's own
        diagonal (which also holds the variances themselves to 1e-6): 1e-6.
    These are the suite's figures for two fits of one problem at tolerances 1e-10
    (test_fit_by_name_agrees_with_the_callable, test_nonlinear_bounded_model_against_scipy).  On the seeded data of
    `_param_map_cases.mapped_problem` scipy converges on all ten cases with both methods with nfev <= 10, and its own
    trf-vs-dogbox spread of popt is at most 0.038 of that tolerance: the reference alone sits 25 x inside it.  Seen on
    MI355X: the mapped route within 4.3e-9 (relative) of R1 and 3.8e-9 of R2 on every case.
    Then the structure of the full-size results: fixed values and tied copies exact, zero / copied rows of pcov."""
    label, fixed, tied, red, groups = pc.E2E_CASES[i]
    pr, R1, R2 = references(i, m, method)
    n = pr["P0"].shape[1]
    pm = ParamMap(n, fixed, tied)
    nf = len(groups)
    assert all(r.success for r in R1[2]), [r.status for r in R1[2]]
    popt, pcov, res = fit_mapped(ctx, pr, fixed, tied, method)
    assert all(r.success for r in res), [r.status for r in res]
    assert popt.shape == (8, n) and pcov.shape == (8, n, n)
    X = np.stack([popt[:, g[0]] for g in groups], axis=1)
    C = pcov[:, [g[0] for g in groups]][:, :, [g[0] for g in groups]]
    print("mapped %s m=%d %s: |X - R1| %.2e  |X - R2| %.2e  (rel.)  scipy nfev <= %d  mapped nfev <= %d"
          % (pc.E2E_IDS[i], m, method, np.max(np.abs(X - R1[0]) / (np.abs(R1[0]) + 1e-3)),
             np.max(np.abs(X - R2[0]) / (np.abs(R2[0]) + 1e-3)), R2[2], max(r.nfev for r in res)))
    np.testing.assert_allclose(X, R1[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(X, R2[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(normalised(C), normalised(R1[1]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(normalised(C, by=R2[1]), normalised(R2[1]), rtol=0, atol=1e-6)
    # structure
    assert np.array_equal(pm.reduce_x(popt), X)
    assert np.array_equal(popt[:, fixed], pr["P0"][:, fixed])
    for j, l in tied.items():
        assert np.array_equal(popt[:, j], popt[:, l])
        assert np.array_equal(pcov[:, j, :], pcov[:, l, :]) and np.array_equal(pcov[:, :, j], pcov[:, :, l])
    assert not pcov[:, fixed, :].any() and not pcov[:, :, fixed].any()
    for b, r in enumerate(res):
        assert r.jac.shape == (m, nf) and r.fun.shape == (m,)
        assert r.x.shape == (n,) and np.array_equal(r.x, popt[b])
        assert r.x_free.shape == (nf,) and np.array_equal(r.x_free, X[b])
        assert np.array_equal(r.param_map, pm.pmap)
        assert r.active_mask.shape == (n,) and not r.active_mask[fixed].any()
        assert np.array_equal(r.x_covariance, pcov[b])
    # results[b].fun / .jac: the weighted residuals and the Jacobian with respect to the solver's variables at popt
    f, jac, _ = pc.reduced_callables(red, pr["P0"])
    np.testing.assert_allclose(np.stack([r.fun for r in res]), (f(pr["x"], X) - pr["Y"]) / mc.SIGMA, rtol=1e-9,
                               atol=1e-9)
    np.testing.assert_allclose(np.stack([r.jac for r in res]), jac(pr["x"], X) / mc.SIGMA, rtol=1e-9, atol=1e-9)


CASE_TIE = 5                                     # gauss2, mu fixed, widths tied: nf = 4


def _one(i=CASE_TIE, m=70):
    label, fixed, tied, red, groups = pc.E2E_CASES[i]
    return pc.mapped_problem(label, m, fixed, tied, groups), fixed, tied, red, groups


def _free(popt, groups):
    return np.stack([popt[:, g[0]] for g in groups], axis=1)


def test_finite_differences_over_the_solver_variables(ctx):
    """jac='2-point' / '3-point' on the mapped device route (the mapped kernel with reps = nf, reduced bounds on the
    device) against its analytic route, at the suite's figure for FD against analytic."""
    pr, fixed, tied, red, groups = _one()
    an = fit_mapped(ctx, pr, fixed, tied, "trf")
    for jac in ("2-point", "3-point"):
        fd = fit_mapped(ctx, pr, fixed, tied, "trf", jac=jac)
        assert all(r.success for r in fd[2]) and fd[2][0].jac.shape == (70, 4)
        np.testing.assert_allclose(fd[0], an[0], rtol=1e-4, atol=1e-7)


def test_robust_loss_on_the_mapped_route(ctx):
    """loss='soft_l1' with outliers against R1: the Jacobian callback after a judge goes through the masked write."""
    pr, fixed, tied, red, groups = _one()
    pr["Y"][:, ::9] += 0.3
    kw = dict(loss="soft_l1", f_scale=2.0)
    R1 = fit_r1(ctx, pr, red, "trf", **kw)
    R = fit_mapped(ctx, pr, fixed, tied, "trf", **kw)
    assert all(r.success for r in R1[2]) and all(r.success for r in R[2])
    np.testing.assert_allclose(_free(R[0], groups), R1[0], rtol=1e-6, atol=1e-9)
    g0 = [g[0] for g in groups]
    np.testing.assert_allclose(normalised(R[1][:, g0][:, :, g0]), normalised(R1[1]), rtol=0, atol=1e-6)


def test_leverage_on_the_mapped_route(ctx):
    pr, fixed, tied, red, groups = _one(m=33)
    R1 = fit_r1(ctx, pr, red, "dogbox", leverage=True)
    R = fit_mapped(ctx, pr, fixed, tied, "dogbox", leverage=True)
    for ra, rb in zip(R1[2], R[2]):
        assert rb.leverage.shape == (33,)
        np.testing.assert_allclose(rb.leverage, ra.leverage, rtol=1e-6, atol=1e-9)
        assert abs(rb.leverage.sum() - len(groups)) < 1e-6                     # trace of the hat matrix = nf


def test_host_driver_with_the_name(ctx):
    pr, fixed, tied, red, groups = _one()
    R1 = fit_r1(ctx, pr, red, "trf")
    R = fit_mapped(ctx, pr, fixed, tied, "trf", driver="host")
    assert all(r.success for r in R[2]) and R[2][0].jac.shape == (70, 4) and R[2][0].x_free.shape == (4,)
    np.testing.assert_allclose(_free(R[0], groups), R1[0], rtol=1e-6, atol=1e-9)
    dev = fit_mapped(ctx, pr, fixed, tied, "trf")
    np.testing.assert_allclose(R[0], dev[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(normalised(R[1][:, [0, 2, 3, 6]][:, :, [0, 2, 3, 6]]),
                               normalised(dev[1][:, [0, 2, 3, 6]][:, :, [0, 2, 3, 6]]), rtol=0, atol=1e-6)


def test_mapped_device_route_calls_no_host_callback(ctx, monkeypatch):
    """The mapped named route runs through run_device alone: run_host raises, and so do the numpy model functions."""
    from bounded_lsq import _outer

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    pr, fixed, tied, red, groups = _one(m=33)
    M = models.get(pr["name"])
    want = fit_mapped(ctx, pr, fixed, tied, "trf")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(M, "f", boom)
    monkeypatch.setattr(M, "jac", boom)
    calls = []
    real = _outer.OuterDriver.run_device
    monkeypatch.setattr(_outer.OuterDriver, "run_device",
                        lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    got = fit_mapped(ctx, pr, fixed, tied, "trf")
    assert calls == [1] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got_fd = fit_mapped(ctx, pr, fixed, tied, "trf", jac="2-point")
    assert calls == [1, 1] and all(r.success for r in got_fd[2])
    with pytest.raises(AssertionError, match="host callback"):
        fit_mapped(ctx, pr, fixed, tied, "trf", driver="host")


def test_nothing_changes_without_the_keywords(ctx, monkeypatch):
    """fixed=[] / tied={} and the keywords absent: the same bits, through the unmapped entry; with a map: the mapped
    entry alone."""
    pr = mc.fit_problem("gauss2", 33)
    lib = me.Counting(ctx.lib, ("blsq_model_eval_dev", "blsq_model_eval_map_dev"))
    monkeypatch.setattr(ctx, "lib", lib)

    def run(**kw):
        return bounded_lsq.curve_fit_batch("gauss_sum", pr["x"], pr["Y"], pr["P0"], sigma=mc.SIGMA, bounds=pr["bounds"],
                                           driver="device", ctx=ctx, **dict(TOL, **kw))
    base = run()
    n_plain = lib.counts["blsq_model_eval_dev"]
    assert n_plain > 0 and lib.counts["blsq_model_eval_map_dev"] == 0
    for kw in (dict(fixed=[], tied={}), dict(fixed=None, tied=None), dict(fixed=np.zeros(7, dtype=bool))):
        got = run(**kw)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert not hasattr(got[2][0], "param_map")
    assert lib.counts == {"blsq_model_eval_dev": 4 * n_plain, "blsq_model_eval_map_dev": 0}
    got = run(tied={5: 2})
    assert all(r.success for r in got[2])
    assert lib.counts["blsq_model_eval_dev"] == 4 * n_plain and lib.counts["blsq_model_eval_map_dev"] > 0


# ---- curve_fit (single) --------------------------------------------------------------------------------------------
def _peak2(x, a1, mu1, s1, a2, mu2, s2, c):
    return (a1 * np.exp(-0.5 * ((x - mu1) / s1) ** 2) + a2 * np.exp(-0.5 * ((x - mu2) / s2) ** 2) + c)


def _dpeak2(x, a1, mu1, s1, a2, mu2, s2, c):
    cols = []
    for a, mu, s in ((a1, mu1, s1), (a2, mu2, s2)):
        z = (x - mu) / s
        e = np.exp(-0.5 * z * z)
        cols += [e, a * e * z / s, a * e * z * z / s]
    return np.stack(cols + [np.ones_like(x)], axis=1)


@pytest.mark.parametrize("jac", [None, "analytic"])
def test_curve_fit_single_against_scipy(ctx, jac):
    """curve_fit(fixed={1, 4}, tied={5: 2}) on problem 0 of the two-peak case against scipy on the hand-reduced model,
    at the figures of the batch test; jac=None differentiates the nf variables on both sides."""
    pr, fixed, tied, red, groups = _one()
    b, m = 0, 70
    _, _, single = pc.reduced_callables(red, pr["P0"])
    fb, jb = single(b)
    sig = np.full(m, mc.SIGMA)
    bounds = (pr["bounds"][0][b], pr["bounds"][1][b])
    popt, pcov, info, _, ier = bounded_lsq.curve_fit(
        _peak2, pr["x"], pr["Y"][b], p0=pr["P0"][b], sigma=sig, bounds=bounds, fixed=fixed, tied=tied,
        jac=None if jac is None else _dpeak2, full_output=True, options={"ctx": ctx}, **TOL)
    ps, cs = so.curve_fit(fb, pr["x"], pr["Y"][b], p0=pr["X0"][b], sigma=sig, method="trf",
                          bounds=(pr["bounds_red"][0][b], pr["bounds_red"][1][b]), jac=None if jac is None else jb, **TOL)
    g0 = [g[0] for g in groups]
    assert ier > 0 and popt.shape == (7,) and pcov.shape == (7, 7) and info["fvec"].shape == (m,)
    np.testing.assert_allclose(popt[g0], ps, rtol=1e-6, atol=1e-9)
    d = np.sqrt(np.diag(cs))
    np.testing.assert_allclose(pcov[np.ix_(g0, g0)] / np.outer(d, d), cs / np.outer(d, d), rtol=0, atol=1e-6)
    assert np.array_equal(popt[fixed], pr["P0"][b][fixed]) and popt[5] == popt[2]
    assert not pcov[fixed, :].any() and not pcov[:, fixed].any() and np.array_equal(pcov[5], pcov[2])
    # degrees of freedom m - nf: the variance factor against absolute_sigma=True
    pa, ca = bounded_lsq.curve_fit(_peak2, pr["x"], pr["Y"][b], p0=pr["P0"][b], sigma=sig, bounds=bounds, fixed=fixed,
                                   tied=tied, jac=None if jac is None else _dpeak2, absolute_sigma=True,
                                   options={"ctx": ctx}, **TOL)
    chi2 = float(np.sum(info["fvec"] ** 2))
    np.testing.assert_allclose(pcov[np.ix_(g0, g0)], ca[np.ix_(g0, g0)] * chi2 / (m - len(groups)), rtol=1e-9)
