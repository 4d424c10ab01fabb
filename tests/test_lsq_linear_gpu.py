"""lsq_linear on the GPU: the kernels of blsq_linear_eval_dev against an extended-precision reference and
against numpy bit for bit, the entry's argument checks, and whole bounded fits on the device route against the host
route and scipy's BVLS.  The cases are those tests/test_lsq_linear_cpu.py vets without a GPU.

Margins.  f: |f - f_ref| <= gamma_{n+1} w (|A||x| + |y|) with gamma_k = k eps / (1 - k eps), eps = 2^-52, f_ref in
numpy.longdouble: the forward bound of an inner product of n + 1 terms in any order (tests/_linear_cases.py: gamma).
J: exact.  Fits: rtol 1e-6 / atol 1e-9 between any two of the device route, the host route and x*, the margin the
package uses between two routes.  The worst fraction of each margin seen on an MI355X is in DESIGN.md 7r.
"""
import warnings

import numpy as np
import pytest
from scipy import optimize

import bounded_lsq
from bounded_lsq import _linear, _outer

import _linear_cases as lc
import _model_eval as me
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 130)
NS = (1, 2, 15, 16, 17, 64, 65, 130)
SENTINEL = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload
worst = {}                                                     # margin name -> worst fraction seen (printed at the end)


def note(name, frac):
    worst[name] = max(worst.get(name, 0.0), float(frac))


def lin_eval(ctx, A, X, y=None, w=None, want_f=True, want_J=False, mask=None, reps=1, B=None, J_fill=None):
    """blsq_linear_eval_dev on host arrays -> (rc, f (B * reps, m) or None, J (B, m, n) or None).  A (m, n) is shared
    (A_stride 0), A (B, m, n) per problem; w (m,) has stride 0, w (B, m) stride m."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, n = A.shape[-2:]
    Q = X.shape[0]
    B = Q // reps if B is None else B
    with me.Dev(ctx) as d:
        dA, dX, dy, dw = d.up(A), d.up(np.ascontiguousarray(X)), d.up(y), d.up(w)
        dm = d.up(None if mask is None else np.asarray(mask, dtype=np.int32))
        df = d.up(np.full((Q, m), np.nan)) if want_f else None
        dJ = d.up(np.full((B, m, n), SENTINEL) if J_fill is None else J_fill) if want_J else None
        rc = ctx.lib.blsq_linear_eval_dev(ctx.h, B, reps, m, n, dA, m * n if A.ndim == 3 else 0, dy, dw,
                                          m if (w is not None and w.ndim == 2) else 0, dX, df, dJ, dm)
        if rc != 0:
            return rc, None, None
        return (0, ctx.to_host(df, (Q, m), np.float64) if want_f else None,
                ctx.to_host(dJ, (B, m, n), np.float64) if want_J else None)


def _inputs(m, n, B, seed):
    rng = np.random.default_rng(seed)
    return dict(A=rng.standard_normal((B, m, n)), X=rng.standard_normal((B, 3, n)), y=rng.standard_normal((B, m)),
                wm=rng.uniform(0.5, 2.0, m), wB=rng.uniform(0.5, 2.0, (B, m)))


# ---- kernel, f ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_residual_against_extended_precision(ctx, m):
    """Every n, B, reps, shared and per-problem A, the three forms of w, with and without y; and for a shared A the
    bits of the same matrix replicated B times."""
    for n in NS:
        for B in (1, 3):
            d = _inputs(m, n, B, 1000 * m + 10 * n + B)
            for reps in (1, 3):
                X = d["X"][:, :reps]
                Xq = np.ascontiguousarray(X.reshape(B * reps, n))
                for shared in (True, False):
                    A = d["A"][0] if shared else d["A"]
                    for wname in (None, "wm", "wB"):
                        w = None if wname is None else d[wname]
                        for y in (d["y"], None):
                            what = (m, n, B, reps, shared, wname, y is not None)
                            rc, f, _ = lin_eval(ctx, A, Xq, y, w, reps=reps)
                            assert rc == 0, what
                            ref, mag = lc.residual_reference(A, X, y, w)
                            err = np.abs(f.reshape(B, reps, m).astype(np.longdouble) - ref)
                            bound = lc.gamma(n + 1) * mag
                            assert np.all(err <= bound), (what, float(np.max(err / bound)))
                            note("f / gamma_{n+1}", np.max(err / bound))
                    rep = np.ascontiguousarray(np.broadcast_to(d["A"][0], (B, m, n)))
                    f_sh = lin_eval(ctx, d["A"][0], Xq, d["y"], d["wB"], reps=reps)[1]
                    f_rep = lin_eval(ctx, rep, Xq, d["y"], d["wB"], reps=reps)[1]
                    assert same_bits(f_sh, f_rep), (m, n, B, reps)


def test_a_problem_s_residual_does_not_depend_on_its_batch(ctx):
    d = _inputs(65, 17, 3, 5)
    Xq = np.ascontiguousarray(d["X"].reshape(9, 17))
    f_all = lin_eval(ctx, d["A"], Xq, d["y"], d["wB"], reps=3)[1]
    for p in range(3):
        f_one = lin_eval(ctx, d["A"][p:p + 1], Xq[3 * p:3 * p + 3], d["y"][p:p + 1], d["wB"][p:p + 1], reps=3)[1]
        assert same_bits(f_one, f_all[3 * p:3 * p + 3])
        for r in range(3):                                     # nor on reps
            f_r = lin_eval(ctx, d["A"][p:p + 1], Xq[3 * p + r:3 * p + r + 1], d["y"][p:p + 1], d["wB"][p:p + 1])[1]
            assert same_bits(f_r[0], f_all[3 * p + r])


def test_non_finite_values_pass_through_as_in_numpy(ctx):
    m, n = 8, 17
    rng = np.random.default_rng(9)
    A = rng.standard_normal((m, n))
    x = rng.standard_normal(n)
    x[2] = np.inf
    A[0, 2] = 1.5                                              # +inf
    A[1, 5] = np.nan                                           # NaN (next to the inf of column 2)
    A[2, 2] = 0.0                                              # 0 * inf = NaN
    A[3, 2] = -2.0                                             # -inf
    A[4, 2], A[4, 7], x[7] = 1.0, np.inf, -1.0                 # inf - inf = NaN
    A[5, 2], A[5, 9] = 1.0, np.inf                             # inf * finite x[9], sign by x[9]
    A[5, 9] = np.inf if x[9] > 0 else -np.inf                  # ... made +inf: inf + inf = inf
    with np.errstate(invalid="ignore"):
        ref = A @ x
    assert np.isnan(ref[[1, 2, 4]]).all() and ref[0] == np.inf and ref[3] == -np.inf and ref[5] == np.inf
    rc, f, _ = lin_eval(ctx, A, x[None])
    assert rc == 0
    assert np.array_equal(np.isnan(f[0]), np.isnan(ref))
    assert np.array_equal(f[0][np.isinf(ref)], ref[np.isinf(ref)])
    assert not np.isfinite(ref).any()                          # (x[2] is infinite: every row meets it)
    x2 = rng.standard_normal(n)                                # a finite x: only the rows with a non-finite A
    with np.errstate(invalid="ignore"):
        ref2 = A @ x2
    f2 = lin_eval(ctx, A, x2[None])[1][0]
    assert np.array_equal(np.isnan(f2), np.isnan(ref2)) and np.array_equal(np.isinf(f2), np.isinf(ref2))
    assert np.array_equal(f2[np.isinf(ref2)], ref2[np.isinf(ref2)])
    ok = np.isfinite(ref2)                                     # the finite rows are not disturbed by their neighbours
    assert ok.sum() == 5
    lref, mag = lc.residual_reference(A[ok], x2[None, None], None, None)
    assert np.all(np.abs(f2[ok].astype(np.longdouble) - lref[0, 0]) <= lc.gamma(n + 1) * mag[0, 0])


# ---- kernel, J ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (63, 15), (64, 16), (65, 17), (130, 65), (130, 130), (3, 1)])
def test_jacobian_is_the_matrix_bit_for_bit_and_a_masked_problem_is_not_touched(ctx, m, n):
    """m n odd (8-byte copy) and even (16-byte vectors), one workgroup and several; NaN payloads and -0.0 survive."""
    B = 3
    d = _inputs(m, n, B, 77 + m + n)
    A = d["A"].copy()
    A[0].flat[0], A[-1].flat[-1] = -0.0, SENTINEL * 1          # (the payload is copied, not computed with)
    X = d["X"][:, 0]
    for shared in (True, False):
        Am = A[0] if shared else A
        for mask in (None, [1, 0, 1], [0, 0, 0], [0, 1, 0]):
            rc, _, J = lin_eval(ctx, Am, X, want_f=False, want_J=True, mask=mask)
            assert rc == 0
            for p in range(B):
                if mask is None or mask[p]:
                    assert same_bits(J[p], A[0] if shared else A[p]), (shared, mask, p)
                else:
                    assert same_bits(J[p], np.full((m, n), SENTINEL)), (shared, mask, p)
        for w in (d["wm"], d["wB"]):
            rc, _, J = lin_eval(ctx, Am, X, w=w, want_f=False, want_J=True, mask=[1, 0, 1])
            assert rc == 0
            for p in (0, 2):
                wp = w if w.ndim == 1 else w[p]
                with np.errstate(invalid="ignore"):
                    assert same_bits(J[p], wp[:, None] * (A[0] if shared else A[p])), (shared, w.ndim, p)
            assert same_bits(J[1], np.full((m, n), SENTINEL))


def test_jacobian_of_more_problems_than_the_grid_has_rows(ctx):
    """Shared A: a workgroup loads its vectors once and walks over its share of the problems (130 x 130: nine
    workgroups per matrix, 455 problem rows in the grid, 460 problems).  Per-problem A: 65540 problems of 1 x 1 against
    the 65535 rows a grid can have."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((130, 130))
    B = 460
    mask = (np.arange(B) % 7 != 3).astype(np.int32)
    rc, _, J = lin_eval(ctx, A, np.zeros((B, 130)), want_f=False, want_J=True, mask=mask)
    assert rc == 0
    assert all(same_bits(J[p], A) for p in np.flatnonzero(mask))
    assert all(same_bits(J[p], np.full((130, 130), SENTINEL)) for p in np.flatnonzero(mask == 0))
    B = 65540
    A1 = rng.standard_normal((B, 1, 1))
    rc, f, J = lin_eval(ctx, A1, np.ones((B, 1)), want_f=True, want_J=True)
    assert rc == 0 and same_bits(J, A1) and same_bits(f, A1[:, :, 0])


def test_f_and_J_in_one_call_are_the_two_separate_calls(ctx):
    d = _inputs(65, 17, 3, 21)
    X = d["X"][:, 0]
    for A in (d["A"], d["A"][0]):
        for w in (None, d["wm"], d["wB"]):
            rc, f, J = lin_eval(ctx, A, X, d["y"], w, want_f=True, want_J=True, mask=[1, 0, 1])
            assert rc == 0
            f1 = lin_eval(ctx, A, X, d["y"], w)[1]
            J1 = lin_eval(ctx, A, X, d["y"], w, want_f=False, want_J=True, mask=[1, 0, 1])[2]
            assert same_bits(f, f1) and same_bits(J, J1)


def test_bad_arguments_return_their_position(ctx):
    """ctx = 1, B, reps, m, n = 5, A, A_stride = 7, y, w, w_stride = 10, X, f (both outputs NULL) = 12, J (reps != 1) =
    13.  The checks come before any launch, so the device pointers may be anything: a small buffer stands in."""
    lib = ctx.lib
    with me.Dev(ctx) as d:
        p = d.up(np.zeros(64))

        def call(B=2, reps=1, m=4, n=3, A=p, A_stride=12, y=p, w=p, w_stride=4, X=p, f=p, J=None, mask=None, h=ctx.h):
            return lib.blsq_linear_eval_dev(h, B, reps, m, n, A, A_stride, y, w, w_stride, X, f, J, mask)
        assert call() == 0 and call(A_stride=0, w_stride=0, y=None, w=None) == 0 and call(f=None, J=p) == 0
        ctx.sync()
        assert call(h=None) == -1
        assert call(B=0) == -2 and call(B=-1) == -2
        assert call(reps=0) == -3
        assert call(m=0) == -4
        assert call(n=0) == -5 and call(n=1024, A_stride=0) == -5
        assert call(A=None) == -6
        assert call(A_stride=11) == -7 and call(A_stride=4) == -7
        assert call(w_stride=3) == -10 and call(w_stride=12) == -10
        assert call(X=None) == -11
        assert call(f=None, J=None) == -12
        assert call(reps=2, J=p) == -13 and call(reps=2, f=None, J=p) == -13
        assert call(B=0, reps=0, A=None) == -2                 # the first bad argument is the one reported
        assert b"invalid argument" in lib.blsq_last_error(ctx.h)
        assert call(reps=3, m=2, n=2, A_stride=4, w_stride=2) == 0   # (6 points of 2: inside the stand-in buffer)
        ctx.sync()


def test_launches_are_timed_in_the_model_eval_slot(ctx):
    d = _inputs(16, 4, 2, 1)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        lin_eval(ctx, d["A"][0], d["X"][:, 0], want_f=True, want_J=True)
        ctx.sync()
        t = ctx.timing_read()
    finally:
        ctx.timing(False)
    assert t["model_eval"][1] == 1 and sum(c for _, c in t.values()) == 1


# ---- fits -----------------------------------------------------------------------------------------------------------
TOL = 1e-10
_fits = {}


def solve(ctx, name, method, driver):
    """One solve per (case, method, driver) for all the tests that look at it."""
    key = (name, method, driver)
    if key not in _fits:
        c = lc.get(name)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _fits[key] = bounded_lsq.lsq_linear_batch(c["A"], c["b"], bounds=(c["lb"], c["ub"]), method=method, tol=TOL,
                                                      x0=c["x0"], driver=driver, ctx=ctx)
    return _fits[key]


_xstar = {}


def xstar(name):
    if name not in _xstar:
        c = lc.get(name)
        _xstar[name] = np.stack([optimize.lsq_linear(lc.problem_matrix(c, p), c["b"][p], bounds=(c["lb"][p], c["ub"][p]),
                                                     method="bvls", tol=1e-14).x for p in range(c["B"])])
    return _xstar[name]


def agree(a, b, what, name):
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9, err_msg=str(what))
    note(name, np.max(np.abs(a - b) / (1e-9 + 1e-6 * np.abs(b))))


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", list(lc.FIT_CASES))
def test_bounded_fits(ctx, name, method):
    c = lc.get(name)
    xs = xstar(name)
    dev, host = solve(ctx, name, method, "device"), solve(ctx, name, method, "host")
    assert len(dev) == len(host) == c["B"]
    Xd, Xh = np.stack([r.x for r in dev]), np.stack([r.x for r in host])
    agree(Xd, Xh, (name, method, "device / host"), "x device / host")
    agree(Xd, xs, (name, method, "device / x*"), "x device / x*")
    agree(Xh, xs, (name, method, "host / x*"), "x host / x*")
    for p, r in enumerate(dev):
        A, b, lb, ub = lc.problem_matrix(c, p), c["b"][p], c["lb"][p], c["ub"][p]
        assert np.all(r.x >= lb) and np.all(r.x <= ub)
        assert r.status == 1 and r.success and r.message, (name, method, p, r.status)
        res = A @ r.x - b
        opt = lc.cl_optimality(r.x, A.T @ res, lb, ub)
        assert opt <= TOL, (name, method, p, opt)
        note("optimality / tol", opt / TOL)
        ref, mag = lc.residual_reference(A, r.x[None, None], b[None], None)
        err = np.abs(r.fun.astype(np.longdouble) - ref[0, 0])
        assert np.all(err <= lc.gamma(c["n"] + 1) * mag[0, 0])
        note("fun / gamma_{n+1}", np.max(err / (lc.gamma(c["n"] + 1) * mag[0, 0])))
        assert r.cost == 0.5 * (r.fun @ r.fun)
        assert np.array_equal(r.active_mask, c["active"][p]), (name, method, p)
        assert np.array_equal(np.where(xs[p] == lb, -1, 0) + np.where(xs[p] == ub, 1, 0), c["active"][p])
        assert r.nit == r.nfev - 1 and r.nfev >= 2 and r.x_covariance is None


def test_unbounded_fit_is_lstsq(ctx):
    c = lc.fit_case(40, 6, 4, True, 201, unbounded=True)
    want = np.stack([np.linalg.lstsq(c["A"], c["b"][p], rcond=None)[0] for p in range(4)])
    for method in ("trf", "dogbox"):
        for driver in ("device", "host"):
            res = bounded_lsq.lsq_linear_batch(c["A"], c["b"], method=method, x0=c["x0"], driver=driver, ctx=ctx)
            agree(np.stack([r.x for r in res]), want, (method, driver), "x unbounded / lstsq")
            assert all(r.status == 1 and not r.active_mask.any() for r in res)
    res = bounded_lsq.lsq_linear_batch(c["A"], c["b"], ctx=ctx)            # the default start: ones
    agree(np.stack([r.x for r in res]), want, "default start", "x unbounded / lstsq")


def test_weighted_fit(ctx):
    """sigma (m,): the weighted problem is the one solved, on both routes; `fun` is the weighted residual."""
    c = lc.fit_case(40, 6, 4, False, 301, sigma=True)
    kw = dict(bounds=(c["lb"], c["ub"]), x0=c["x0"], sigma=c["sigma"], ctx=ctx)
    dev = bounded_lsq.lsq_linear_batch(c["A"], c["b"], driver="device", **kw)
    host = bounded_lsq.lsq_linear_batch(c["A"], c["b"], driver="host", **kw)
    agree(np.stack([r.x for r in dev]), np.stack([r.x for r in host]), "weighted", "x device / host")
    agree(np.stack([r.x for r in dev]), c["xstar"], "weighted / x*", "x device / x*")
    for p, r in enumerate(dev):
        assert r.status == 1 and np.array_equal(r.active_mask, c["active"][p])
        np.testing.assert_allclose(r.fun, (c["A"][p] @ r.x - c["b"][p]) / c["sigma"], rtol=1e-10, atol=1e-12)


def test_nnls_unmixing(ctx):
    c = lc.nnls_case()
    want, _ = optimize.nnls(c["A"], c["b"])
    for method in ("trf", "dogbox"):
        r = bounded_lsq.lsq_linear(c["A"], c["b"], bounds=(0, np.inf), method=method, ctx=ctx)
        assert r.status == 1 and np.all(r.x >= 0)
        agree(r.x, want, ("nnls", method), "x nnls / scipy.nnls")
        assert np.array_equal(r.active_mask, [0, 0, 0, -1, -1])


def test_one_problem_is_the_first_of_its_batch(ctx):
    c = lc.get("40x6-shared")
    for method in ("trf", "dogbox"):
        one = bounded_lsq.lsq_linear(c["A"], c["b"][0], bounds=(c["lb"][0], c["ub"][0]), method=method, tol=TOL,
                                     x0=c["x0"][0], ctx=ctx)
        first = solve(ctx, "40x6-shared", method, "device")[0]
        for k in ("x", "fun", "active_mask"):
            assert np.array_equal(one[k], first[k]), (method, k)
        assert (one.cost, one.optimality, one.nfev, one.nit, one.status) == \
            (first.cost, first.optimality, first.nfev, first.nit, first.status)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_covariance_is_the_covariance_of_A_over_the_free_variables(ctx, method):
    c = lc.get("40x6-own")
    res = bounded_lsq.lsq_linear_batch(c["A"], c["b"], bounds=(c["lb"], c["ub"]), method=method, x0=c["x0"], ctx=ctx,
                                       covariance=True, leverage=True)
    act = np.stack([r.active_mask for r in res])
    assert np.array_equal(act, c["active"])
    cov, rcond, status = bounded_lsq.covariance(c["A"], act, ctx=ctx)
    lev = bounded_lsq.leverage(c["A"], act, ctx=ctx)[0]
    for p, r in enumerate(res):
        assert status[p] == 0 and np.array_equal(r.x_covariance, cov[p]) and r.x_covariance_rcond == rcond[p]
        assert np.all(r.x_covariance[act[p] != 0] == 0.0)
        assert np.array_equal(r.leverage, lev[p])


# ---- routes ---------------------------------------------------------------------------------------------------------
def _counts(ctx, monkeypatch):
    proxy = me.Counting(ctx.lib)
    proxy.counts["blsq_linear_eval_dev"] = 0
    monkeypatch.setattr(ctx, "lib", proxy)
    return proxy.counts


def test_device_route_reaches_the_new_entry_alone(ctx, monkeypatch):
    c = lc.get("40x6-shared")
    before = solve(ctx, "40x6-shared", "trf", "device")

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_linear, "numpy_callbacks", boom)
    counts = _counts(ctx, monkeypatch)
    got = bounded_lsq.lsq_linear_batch(c["A"], c["b"], bounds=(c["lb"], c["ub"]), tol=TOL, x0=c["x0"], ctx=ctx)
    assert all(np.array_equal(g.x, r.x) for g, r in zip(got, before))
    assert set(counts) == {"blsq_linear_eval_dev"}
    # one f and one J at the start, then one f per step tried and one J per judged round with an accepted step
    assert counts["blsq_linear_eval_dev"] >= 2 + max(r.nfev for r in got) - 1
    # the finite-difference route asks for reps > 1 and gets the same solution
    counts["blsq_linear_eval_dev"] = 0
    fd = bounded_lsq.least_squares_batch(bounded_lsq.LinearFit(c["A"], c["b"]), c["x0"], "2-point",
                                         bounds=(c["lb"], c["ub"]), ftol=TOL, xtol=np.finfo(float).eps, gtol=TOL,
                                         driver="device", ctx=ctx)
    assert set(counts) == {"blsq_linear_eval_dev"} and counts["blsq_linear_eval_dev"] > 0
    np.testing.assert_allclose(np.stack([r.x for r in fd]), np.stack([r.x for r in before]), rtol=1e-6, atol=1e-9)


def test_curve_fit_batch_does_not_reach_the_new_entry(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    t = np.linspace(-1, 1, 20)
    P = rng.uniform(0.5, 1.5, (3, 3))
    Y = P[:, :1] + P[:, 1:2] * t + P[:, 2:] * t ** 2
    counts = _counts(ctx, monkeypatch)
    popt = bounded_lsq.curve_fit_batch("poly", t, Y, np.ones((3, 3)), driver="device", ctx=ctx)[0]
    np.testing.assert_allclose(popt, P, rtol=1e-6, atol=1e-9)
    assert counts["blsq_linear_eval_dev"] == 0 and any(v > 0 for k, v in counts.items() if "model_eval" in k)


def test_report_margins():
    """Not a check: prints the worst fraction of every margin the tests above used (run with -s to see it)."""
    for k in sorted(worst):
        print("margin %-24s worst fraction %.3g" % (k, worst[k]))
