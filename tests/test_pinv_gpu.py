"""Pseudo-inverse covariance on the GPU (blsq_cov_pinv*, blsq_outer_covariance_pinv, covariance='pinv' / 'free-pinv')
against the extended-precision references of tests/_pinv_ref.py.

Metric and bound are those of tests/test_cov_gpu.py: max |C - C*|_ij / sqrt(C*_ii C*_jj) <= max(4 x the error of scipy's
float64 SVD recipe against the same reference, 8 n eps).  Every test prints the figures it asserts on (-s)."""
import numpy as np
import pytest

import _cov_ref as ref
import _pinv_ref as pref

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


def _pinv(J, ctx, mask=None, scale=None):
    import bounded_lsq
    return bounded_lsq.covariance(J, mask, ctx=ctx, pinv=True, scale=scale)


def _rcond_figures(r, rcond, kept):
    """rcond = s_min / s_max over all values, kept_rcond over the kept ones, against the reference's values."""
    rel = np.sort(np.asarray(r["rel"]))[::-1]
    n = rel.size
    want_kept = rel[r["rank"] - 1]
    assert abs(kept - want_kept) <= 1e-10 * want_kept, (kept, want_kept)
    if r["rank"] == n:
        assert rcond == kept
    else:
        assert 0.0 <= rcond < EPS * 1e3, rcond           # a dropped value: at rounding level of s_max or below


# ---- rank-deficient inputs against the reference ---------------------------------------------------
SMALL = [("64x8 duplicated column", lambda: pref.duplicated_column(11, 64, 8), 7),
         ("300x18 kappa 1e3 + dependent column", lambda: pref.dependent_column(12), 17),
         ("6x10 wide", lambda: pref.wide(13), 6),
         ("40x5 zero column", lambda: pref.zero_column(14), 4)]


@pytest.mark.parametrize("label,make,rank", SMALL, ids=[c[0] for c in SMALL])
def test_rank_deficient_small(ctx, label, make, rank):
    J = make()
    r = pref.reference_small(J)
    assert r["rank"] == rank
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status == 0 and rk == rank, (status, rk)
    pref.check(C, r, label)
    _rcond_figures(r, rcond, kept)
    # covariance=True has nothing to say here
    import bounded_lsq
    C1, _, s1 = bounded_lsq.covariance(J, ctx=ctx)
    assert s1 == 1 and np.all(np.isnan(C1))


@pytest.mark.parametrize("m,na", [(600, 40), (900, 136)], ids=["600x80", "900x272"])
def test_rank_deficient_doubled(ctx, m, na):
    J, r = pref.doubled_case(5, m, na)
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status == 0 and rk == na, (status, rk)
    pref.check(C, r, "%dx%d doubled" % (m, 2 * na))
    _rcond_figures(r, rcond, kept)


# ---- full rank ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,kappa", [(65, 64, 1e2), (300, 17, 30.0)], ids=["65x64", "300x17"])
def test_full_rank_agrees_with_the_inverse(ctx, m, n, kappa):
    import bounded_lsq
    J = ref.make_jacobian(np.random.default_rng(300 + n), m, n, kappa)
    r = pref.full_rank(J)
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status == 0 and rk == n and rcond == kept
    e_pinv = pref.check(C, r, "%dx%d full rank" % (m, n))
    C1, _, s1 = bounded_lsq.covariance(J, ctx=ctx)
    assert s1 == 0
    e_inv = ref.cov_error(C1, r["C"])
    assert e_inv <= r["bound"]
    d = ref.cov_error(C, np.asarray(C1, dtype=ref.LD))
    print("pinv vs inverse: %.3g (their errors %.3g, %.3g)" % (d, e_pinv, e_inv))
    # the two results are within their own bounds of C*, so within the sum of each other (the metric's scaling by
    # C1 instead of C* moves it by a relative 1e-13 at most)
    assert d <= 2 * r["bound"] * (1 + 1e-10)


def test_sequential_fold_1200x600(ctx):
    J = ref.make_jacobian(np.random.default_rng(800), 1200, 600, 50.0, grid=True)
    r = pref.full_rank(J)
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status == 0 and rk == 600
    pref.check(C, r, "1200x600 (sequential fold)")


# ---- tile edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_tile_edges(ctx, n):
    m = 3 * n
    if n >= 2:
        J = pref.duplicated_column(40 + n, m, n)
        if n <= 32:
            r = pref.reference_small(J)
        else:                                   # n = 33: beyond the mpmath helper; [a ... a] has the closed form below
            r = _duplicate_closed_form(J)
        want = n - 1
    else:
        J = np.array([[3.0], [4.0], [12.0]])
        r = dict(C=np.array([[1.0 / 169.0]], dtype=ref.LD), rank=1, zero=[], rel=np.ones(1), err_recipe=0.0,
                 err_reference=0.0, bound=8 * EPS, kind="closed form")
        want = 1
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status == 0 and rk == want
    pref.check(C, r, "tile edge n = %d" % n)


def _duplicate_closed_form(J):
    """J = [A a_0] = A K with K = [I e_0], K K^T = diag(2, 1, ..., 1) and K^+ = K^T diag(1/2, 1, ..., 1); A has full
    rank, so (J^T J)^+ = K^+ C_A K^+^T:  C*[j, k] = d_j d_k C_A[p(j), p(k)] with p(last) = 0, d = 1/2 on the two copies
    and 1 elsewhere, C_A from the checked `_cov_ref.reference(A)`.  Exact: the factors are powers of two."""
    n = J.shape[1]
    rA = ref.reference(np.ascontiguousarray(J[:, :n - 1]))
    CA = np.asarray(rA["C"], dtype=ref.LD)
    p = list(range(n - 1)) + [0]
    d = np.ones(n, dtype=ref.LD)
    d[0] = d[n - 1] = 0.5
    C = CA[np.ix_(p, p)] * np.outer(d, d)
    s = np.linalg.svd(J, compute_uv=False)
    pref.assert_gap(s / s[0], EPS * max(J.shape))
    err_rec = ref.cov_error(ref.svd_recipe(J), C)
    return dict(C=C, rank=n - 1, zero=[], rel=s / s[0], err_recipe=err_rec, err_reference=rA["err_reference"],
                bound=max(4 * err_rec, 8 * n * EPS), kind="closed form")


# ---- the batch ---------------------------------------------------------------------------------------
def _batch_37():
    """37 problems of 300 x 17: ranks 17, 16 (a duplicated column) and 15, one all-zero J (index 5), one with a NaN
    (index 9); a mask per problem for the 'free-pinv' run."""
    rng = np.random.default_rng(77)
    B, m, n = 37, 300, 17
    J = np.empty((B, m, n))
    ranks = np.empty(B, dtype=int)
    for b in range(B):
        k = b % 3                                       # columns made dependent
        A = ref.make_jacobian(rng, m, n - k, 10.0 ** rng.uniform(0.3, 2.0))
        cols = [A] + [A[:, i:i + 1] for i in range(k)]
        J[b] = np.hstack(cols)[:, rng.permutation(n)]
        ranks[b] = n - k
    J[5] = 0.0
    ranks[5] = 0
    J[9, 123, 4] = np.nan
    ranks[9] = 0
    mask = (rng.uniform(size=(B, n)) < 0.3).astype(np.int64)
    mask[3] = 0
    mask[4] = 1                                         # every variable on a bound
    return J, ranks, mask


def test_batch_of_37(ctx):
    J, ranks, mask = _batch_37()
    B, m, n = J.shape
    C, rk, rcond, kept, status = _pinv(J, ctx)
    assert status[9] == 1 and np.all(np.isnan(C[9])) and rk[9] == 0
    assert np.array_equal(np.delete(status, 9), np.zeros(B - 1, dtype=np.int32))
    assert np.array_equal(np.delete(rk, 9), np.delete(ranks, 9)), (rk, ranks)
    assert np.all(C[5] == 0.0) and rcond[5] == 0.0 and kept[5] == 0.0
    for b in range(B):
        if b != 9:
            assert np.array_equal(C[b], C[b].T), b
    # every problem's bits are those of the problem run alone
    for b in range(B):
        one = _pinv(J[b], ctx)
        assert np.array_equal(one[0], C[b], equal_nan=True), b
        assert (one[1], one[4]) == (rk[b], status[b]) and one[2] == rcond[b] and one[3] == kept[b], b
    # parity of two against the reference (ranks 16 and 15)
    for b in (1, 2):
        pref.check(C[b], pref.reference_small(J[b]), "batch problem %d" % b)
    # the front end's view
    import bounded_lsq
    from scipy.optimize import OptimizeResult
    res = [OptimizeResult(jac=J[b], active_mask=mask[b], obj_value=1.0) for b in range(B)]
    bounded_lsq._cov.attach(res, 'pinv', ctx=ctx)
    assert res[9].x_covariance is None and res[9].x_covariance_rank == 0
    assert all(res[b].x_covariance is not None and res[b].x_covariance_rank == ranks[b] for b in range(B) if b != 9)
    assert np.array_equal(res[8].x_covariance, C[8]) and np.array_equal(res[10].x_covariance, C[10])


def test_batch_of_37_free(ctx):
    J, ranks, mask = _batch_37()
    B, m, n = J.shape
    C, rk, rcond, kept, status = _pinv(J, ctx, mask)
    for b in range(B):
        free = np.nonzero(mask[b] == 0)[0]
        act = np.nonzero(mask[b])[0]
        one = _pinv(J[b], ctx, mask[b])
        assert np.array_equal(one[0], C[b], equal_nan=True) and one[1] == rk[b] and one[4] == status[b], b
        if b == 9 and 4 in free:
            assert status[b] == 1 and np.all(np.isnan(C[b]))
            continue
        assert status[b] == 0, b
        assert np.array_equal(C[b], C[b].T), b
        assert np.all(C[b][act] == 0.0) and np.all(C[b][:, act] == 0.0), b
        if free.size == 0:
            assert rk[b] == 0 and np.all(C[b] == 0.0)
            continue
        # the rank is that of J_F alone (its bits need not be: the SVD kernel is specialised by n, not by |F|)
        sub = _pinv(np.ascontiguousarray(J[b][:, free]), ctx)
        assert sub[1] == rk[b] and sub[4] == 0, b
    assert status[4] == 0 and rk[4] == 0 and np.all(C[4] == 0.0)
    for b in (1, 2):
        free = np.nonzero(mask[b] == 0)[0]
        Jf = np.ascontiguousarray(J[b][:, free])
        pref.check(C[b][np.ix_(free, free)], pref.reference_small(Jf), "free block of problem %d" % b)


def test_scale(ctx):
    J, ranks, mask = _batch_37()
    J = J[:8]
    scale = np.random.default_rng(5).uniform(1e-3, 1e3, 8)
    C0 = _pinv(J, ctx)[0]
    C1 = _pinv(J, ctx, scale=scale)[0]
    want = C0 * scale[:, None, None]                     # (one rounding: the kernel multiplies the same accumulator)
    for b in range(8):
        assert np.all(np.abs(C1[b] - want[b]) <= np.spacing(np.abs(want[b]))), b
        assert np.array_equal(C1[b], C1[b].T)
    assert np.all(C1[5] == 0.0)
    one = _pinv(J[2], ctx, scale=3.0)[0]
    assert np.array_equal(one, _pinv(J[:3], ctx, scale=np.array([1.0, 2.0, 3.0]))[0][2])


# ---- the C-ABI on device pointers ------------------------------------------------------------------------
def test_device_pointer_call_and_argument_errors(ctx):
    import ctypes as C
    import bounded_lsq
    from bounded_lsq._abi import vp
    rng = np.random.default_rng(17)
    B, m, n = 3, 90, 33
    J = rng.standard_normal((B, m, n))
    J[1, :, 7] = J[1, :, 20]
    mask = (rng.uniform(size=(B, n)) < 0.3).astype(np.int64)
    scale = np.array([0.5, 2.0, 7.0])
    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "create")
    try:
        dJ, dM, dS = ctx.to_device(J), ctx.to_device(mask), ctx.to_device(scale)
        dC, dk, dr, dq, ds = (ctx.malloc(B * n * n * 8), ctx.malloc(B * 4), ctx.malloc(B * 8), ctx.malloc(B * 8),
                              ctx.malloc(B * 4))
        for dmask, hmask, dsc, hsc in ((None, None, None, None), (dM, mask, dS, scale)):
            ctx.check(ctx.lib.blsq_cov_pinv_dev(h, dJ, dmask, dsc, dC, dk, dr, dq, ds), "blsq_cov_pinv_dev")
            ctx.sync()
            got = (ctx.to_host(dC, (B, n, n), np.float64), ctx.to_host(dk, (B,), np.int32),
                   ctx.to_host(dr, (B,), np.float64), ctx.to_host(dq, (B,), np.float64),
                   ctx.to_host(ds, (B,), np.int32))
            want = bounded_lsq.covariance(J, hmask, ctx=ctx, pinv=True, scale=hsc)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert got[1][1] <= n - 1
        assert np.array_equal(ctx.to_host(dJ, (B, m, n), np.float64), J), "J must not be modified"
        # the plan serves the inverse route as well, before and after
        ctx.check(ctx.lib.blsq_cov_dev(h, dJ, None, dC, dr, ds), "blsq_cov_dev")
        ctx.sync()
        assert np.array_equal(ctx.to_host(ds, (B,), np.int32), [0, 1, 0])
        assert ctx.lib.blsq_cov_pinv_dev(h, None, None, None, dC, dk, dr, dq, ds) == -2
        assert ctx.lib.blsq_cov_pinv_dev(h, dJ, None, None, None, dk, dr, dq, ds) == -5
        assert ctx.lib.blsq_cov_pinv_dev(h, dJ, None, None, dC, None, dr, dq, ds) == -6
        for p in (dJ, dM, dS, dC, dk, dr, dq, ds):
            ctx.free(p)
    finally:
        ctx.lib.blsq_cov_plan_destroy(h)


def test_timing_slots(ctx):
    J, ranks, mask = _batch_37()
    ctx.timing(True)
    ctx.timing_reset()
    _pinv(J[:4], ctx, mask[:4])
    ctx.sync()
    T = ctx.timing_read()
    ctx.timing(False)
    assert T["cov_pinv_weights"][1] == 1 and T["cov_pinv_product"][1] == 1 and T["jacobi_svd"][1] == 1
    assert T["cov_gather"][1] == 1 and T["cov_inverse"][1] == 0 and T["cov_product"][1] == 0


# ---- the drivers -----------------------------------------------------------------------------------------
def _linear_batch(B=5, m=40, n=4, seed=3):
    """B linear models y = A_b p with one duplicated basis column in problem 1."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m, n))
    A[1, :, 3] = A[1, :, 0]
    y = np.einsum('bmn,n->bm', A, np.arange(1.0, n + 1)) + 0.05 * rng.standard_normal((B, m))

    def fun(X):
        return np.einsum('bmn,bn->bm', A, X) - y

    def jac(X):
        return A
    return fun, jac, A, y


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_device_driver_equals_host_driver(ctx, method):
    import bounded_lsq
    fun, jac, A, y = _linear_batch()
    B, m, n = A.shape
    X0 = np.zeros((B, n))
    out = {}
    for driver in ("host", "device"):
        out[driver] = bounded_lsq.least_squares_batch(fun, X0, jac, method=method, driver=driver, ctx=ctx,
                                                      covariance='pinv')
    for b in range(B):
        h, d = out["host"][b], out["device"][b]
        assert h.x_covariance_rank == d.x_covariance_rank == (n - 1 if b == 1 else n)
        r = pref.reference_small(h.jac)
        pref.check(h.x_covariance, r, "%s host, problem %d" % (method, b))
        pref.check(d.x_covariance, pref.reference_small(d.jac), "%s device, problem %d" % (method, b))
        assert np.array_equal(h.jac, d.jac) and np.array_equal(h.x_covariance, d.x_covariance)
    # True has nothing for the rank-deficient problem, 'pinv' has
    t = bounded_lsq.least_squares_batch(fun, X0, jac, method=method, driver='device', ctx=ctx, covariance=True)
    assert t[1].x_covariance is None and out["device"][1].x_covariance is not None
    assert "x_covariance_rank" not in t[0]


def test_outer_driver_variance_scale_and_free(ctx):
    from bounded_lsq import OuterDriver
    fun, jac, A, y = _linear_batch()
    B, m, n = A.shape
    lb = np.full((B, n), -np.inf)
    ub = np.full((B, n), np.inf)
    ub[:, 1] = 1.5                                       # the unconstrained optimum has p_1 = 2: cut off
    X0 = np.zeros((B, n))
    drv = OuterDriver('dogbox', B, m, n, ctx=ctx)
    try:
        drv.start(X0, X0, lb, ub, np.ones((B, n)), False, 1e-10, 1e-10, 1e-10, 100)
        R = drv.run_host(fun, jac)
        plain = drv.covariance(pinv=True)
        scaled = drv.covariance(pinv=True, variance_scale=True)
        free = drv.covariance(free_only=True, pinv=True, variance_scale=True)
        with pytest.raises(ValueError):
            drv.covariance(variance_scale=True)
    finally:
        drv.close()
    s2 = R["obj"] / (m - n)
    want = plain[0] * s2[:, None, None]
    assert np.all(np.abs(scaled[0] - want) <= np.spacing(np.abs(want)))
    for k in (1, 2, 3, 4):
        assert np.array_equal(plain[k], scaled[k])
    assert np.all(R["on_bound"][:, 1] == 1)
    import bounded_lsq
    fw = bounded_lsq.covariance(A, R["on_bound"], ctx=ctx, pinv=True, scale=s2)
    assert all(np.array_equal(a, b) for a, b in zip(free, fw))
    assert np.all(free[0][:, 1, :] == 0.0) and np.all(free[0][:, :, 1] == 0.0)


def test_robust_loss_covariance_between_judge_and_propose(ctx):
    """Under a robust loss the driver's J holds diag(w) J; the Jacobians a judge has just accepted are unscaled until the
    next propose.  A pinv covariance call in between scales them once: it sees diag(w) J for every problem, and the run
    goes on to the results of an undisturbed one."""
    import ctypes as C
    import bounded_lsq
    from bounded_lsq import OuterDriver, _hostmath as H
    B, m, n = 4, 50, 3
    t = np.linspace(0, 3, m)
    rng = np.random.default_rng(9)
    truth = np.array([[0.5 + 0.1 * b, 2.0 - 0.05 * b, -1.0 + 0.03 * b] for b in range(B)])
    Y = truth[:, 0:1] + truth[:, 1:2] * np.exp(truth[:, 2:3] * t) + 0.02 * rng.standard_normal((B, m))
    Y[:, ::7] += 2.0                                     # outliers

    def fun(P):
        return P[:, 0:1] + P[:, 1:2] * np.exp(P[:, 2:3] * t) - Y

    def jac(P):
        e = np.exp(P[:, 2:3] * t)
        return np.stack([np.ones_like(e), e, P[:, 1:2] * t * e], axis=2)

    X0 = np.tile([0.0, 1.0, -0.5], (B, 1))
    X0[:, 1] += 0.7 * np.arange(B)
    lb, ub = np.full((B, n), -np.inf), np.full((B, n), np.inf)
    fs = np.linspace(0.05, 0.5, B)
    loss = 'soft_l1'
    kw = dict(loss=loss, f_scale=fs, ftol=1e-10, xtol=1e-10, gtol=1e-10, max_nfev=200)
    calm = bounded_lsq.least_squares_batch(fun, X0, jac, driver='device', ctx=ctx, **kw)
    drv = OuterDriver('trf', B, m, n, ctx=ctx)
    calls = 0
    try:
        drv.set_loss(loss, fs)
        drv.start(X0, X0, lb, ub, np.ones((B, n)), False, 1e-10, 1e-10, 1e-10, 200)
        X = drv._down(drv.d_x, (B, n))
        drv._up(drv.d_f, fun(X), (B, m))
        drv._up(drv.d_J, jac(X), (B, m, n))
        drv.begin()
        itemJ = m * n * 8
        while drv.propose() > 0:
            Xt = drv._down(drv.d_x_trial, (B, n))
            drv._up(drv.d_f_trial, fun(Xt), (B, m))
            if drv.judge() > 0:
                acc = drv._down(drv.d_accepted, (B,), np.int32)
                X = drv._down(drv.d_x, (B, n))
                Jn = np.ascontiguousarray(jac(X))
                for b in np.nonzero(acc)[0]:
                    dst = C.c_void_p(drv.d_J.value + int(b) * itemJ)
                    ctx.check(ctx.lib.blsq_memcpy_h2d(ctx.h, dst, Jn[b].ctypes.data_as(C.c_void_p), itemJ), "h2d")
                if calls < 3:                            # between judge and propose
                    got = drv.covariance(pinv=True)
                    Jd = drv._down(drv.d_J, (B, m, n))
                    F = fun(X)
                    for b in range(B):
                        Js, _ = H.loss_scale(Jn[b], F[b], H.loss_rho(loss, F[b], fs[b]))
                        np.testing.assert_allclose(Jd[b], Js, rtol=1e-12, atol=0)   # (scaled once, not twice)
                    want = bounded_lsq.covariance(Jd, ctx=ctx, pinv=True)
                    assert all(np.array_equal(a, b) for a, b in zip(got, want))
                    calls += 1
        R = drv.fetch()
    finally:
        drv.close()
    assert calls == 3
    for b in range(B):
        assert (R["nfev"][b], R["njev"][b], R["status"][b]) == (calm[b].nfev, calm[b].njev, calm[b].status), b
        np.testing.assert_allclose(R["x"][b], calm[b].x, rtol=1e-9, atol=1e-12)
