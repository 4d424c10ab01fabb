"""Parameter covariance on the GPU (blsq_cov*, blsq_outer_covariance, `covariance=` of the front ends) against the
extended-precision references of tests/_cov_ref.py.

Error metric: max_ij |C - C*|_ij / sqrt(C*_ii C*_jj).  Bound per case: the error of scipy's float64 SVD recipe
(curve_fit's lines) on the same J against the same reference, times 4, with a floor of 8 n eps.  Every test prints the
figures it asserts on (run with -s to see them)."""
import json
import os

import numpy as np
import pytest

import _cov_ref as ref
from _problems import expfit_problem, EXPFIT_X0
from _suite import SUITE_BY_NAME

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


def _check(C, J, label, r=None):
    """C against the checked reference of J: symmetric to the bit, within the bound.  -> the reference record"""
    r = r or ref.reference(J)
    assert np.array_equal(C, C.T), (label, "not exactly symmetric")
    err = ref.cov_error(C, r["C"])
    print("%s: error %.3g, bound %.3g (recipe %.3g, reference %.3g, %s), ratio to bound %.3g"
          % (label, err, r["bound"], r["err_recipe"], r["err_reference"], r["kind"], err / r["bound"]))
    assert err <= r["bound"], (label, err, r["bound"])
    return r


# ---- parity ------------------------------------------------------------------------------------
SMALL = [("512x64 kappa 2", 512, 64, 2.0, True), ("512x64 kappa 1e3", 512, 64, 1e3, True),
         ("512x64 kappa 1e6", 512, 64, 1e6, True), ("64x64 (m = n)", 64, 64, 1e2, False),
         ("65x64 (m = n + 1)", 65, 64, 1e2, False)]
LARGE = [("4096x256", 4096, 256, 50.0), ("2048x80", 2048, 80, 50.0), ("900x272", 900, 272, 50.0),
         ("1200x600", 1200, 600, 50.0)]


@pytest.mark.parametrize("label,m,n,kappa,scales", SMALL, ids=[c[0] for c in SMALL])
def test_parity_mpmath(ctx, label, m, n, kappa, scales):
    import bounded_lsq
    rng = np.random.default_rng(100 + m + int(np.log10(kappa) * 7))
    J = ref.make_jacobian(rng, m, n, kappa, column_scales=scales)
    C, rcond, status = bounded_lsq.covariance(J, ctx=ctx)
    print("%s: kappa_2(J) = %.3g, rcond_1 = %.3g" % (label, np.linalg.cond(J), rcond))
    assert status == 0 and rcond >= EPS * m
    r = _check(C, J, label)
    assert r["kind"] == "mpmath"


@pytest.mark.parametrize("label,m,n,kappa", LARGE, ids=[c[0] for c in LARGE])
def test_parity_longdouble(ctx, label, m, n, kappa):
    import bounded_lsq
    rng = np.random.default_rng(200 + n)
    J = ref.make_jacobian(rng, m, n, kappa, grid=True)
    assert np.linalg.cond(J) <= 1e2
    C, rcond, status = bounded_lsq.covariance(J, ctx=ctx)
    assert status == 0
    r = _check(C, J, label)
    assert r["kind"] == "longdouble"


def _batch_300x17(B=37):
    rng = np.random.default_rng(317)
    return np.stack([ref.make_jacobian(rng, 300, 17, 10.0 ** rng.uniform(0.3, 2.0)) for _ in range(B)])


def test_parity_batch_of_37(ctx):
    import bounded_lsq
    J = _batch_300x17()
    C, rcond, status = bounded_lsq.covariance(J, ctx=ctx)
    assert C.shape == (37, 17, 17) and np.all(status == 0)
    worst = 0.0
    for b in range(37):
        r = ref.reference(J[b], force="longdouble")
        assert np.array_equal(C[b], C[b].T)
        err = ref.cov_error(C[b], r["C"])
        worst = max(worst, err / r["bound"])
        assert err <= r["bound"], (b, err, r["bound"])
    print("300x17, B = 37: worst ratio to the bound %.3g" % worst)


# ---- bits ----------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(ctx):
    import bounded_lsq
    J = _batch_300x17()
    rng = np.random.default_rng(5)
    P = ref.make_jacobian(rng, 300, 17, 30.0)
    alone = bounded_lsq.covariance(P, ctx=ctx)
    mask = np.zeros(17, dtype=int)
    mask[[2, 9]] = 1
    alone_free = bounded_lsq.covariance(P, mask, ctx=ctx)
    for pos in (0, 17, 36):
        Jb = J.copy()
        Jb[pos] = P
        C, rcond, status = bounded_lsq.covariance(Jb, ctx=ctx)
        assert np.array_equal(C[pos], alone[0]) and rcond[pos] == alone[1] and status[pos] == alone[2]
        M = (rng.uniform(size=(37, 17)) < 0.2).astype(int)
        M[pos] = mask
        C, rcond, status = bounded_lsq.covariance(Jb, M, ctx=ctx)
        assert np.array_equal(C[pos], alone_free[0]) and rcond[pos] == alone_free[1]


# ---- 'free' --------------------------------------------------------------------------------------
def _free_masks(rng, n):
    masks = {"none active": np.zeros(n, dtype=int)}
    one = np.ones(n, dtype=int)
    one[n // 3] = 0
    masks["all but one active"] = one
    for name, sl in (("first", slice(0, 5)), ("middle", slice(n // 2 - 2, n // 2 + 3)), ("last", slice(n - 5, n))):
        mk = np.zeros(n, dtype=int)
        mk[sl] = rng.choice([-1, 1], 5)
        masks["active columns " + name] = mk
    for k in range(3):
        masks["random %d" % k] = rng.choice([-1, 0, 0, 1], n)
    return masks


@pytest.mark.parametrize("m,n", [(200, 24), (512, 64)])
def test_free_covariance(ctx, m, n):
    import bounded_lsq
    rng = np.random.default_rng(7 + n)
    J = ref.make_jacobian(rng, m, n, 1e3, column_scales=True)
    masks = _free_masks(rng, n)
    names = list(masks)
    if n == 64:                                    # (the 50-digit references of 512 x 64 take seconds each)
        names = ["all but one active", "active columns middle", "random 0"]
    M = np.stack([masks[k] for k in names])
    C, rcond, status = bounded_lsq.covariance(np.broadcast_to(J, (len(names), m, n)), M, ctx=ctx)
    assert np.all(status == 0)
    for b, name in enumerate(names):
        F = np.nonzero(M[b] == 0)[0]
        A = np.nonzero(M[b] != 0)[0]
        assert np.all(C[b][A, :] == 0.0) and np.all(C[b][:, A] == 0.0), name
        assert not np.any(np.signbit(C[b][A, :])), name
        _check(np.ascontiguousarray(C[b][np.ix_(F, F)]), np.ascontiguousarray(J[:, F]), "%dx%d free, %s" % (m, n, name))


def test_zero_column_on_an_active_variable(ctx):
    import bounded_lsq
    rng = np.random.default_rng(11)
    J = ref.make_jacobian(rng, 120, 9, 20.0)
    J[:, 4] = 0.0
    mask = np.zeros(9, dtype=int)
    mask[4] = -1
    C, rcond, status = bounded_lsq.covariance(J, ctx=ctx)
    assert status == 1 and np.all(np.isnan(C))
    C, rcond, status = bounded_lsq.covariance(J, mask, ctx=ctx)
    assert status == 0 and rcond > 1e-4
    F = np.nonzero(mask == 0)[0]
    _check(np.ascontiguousarray(C[np.ix_(F, F)]), np.ascontiguousarray(J[:, F]), "zero column held fixed")
    assert np.all(C[4] == 0.0) and np.all(C[:, 4] == 0.0)


# ---- singular ------------------------------------------------------------------------------------
def test_singular_verdicts(ctx):
    import bounded_lsq
    rng = np.random.default_rng(13)
    m, n = 512, 64
    good = ref.make_jacobian(rng, m, n, 1e6, column_scales=True)
    zero = good.copy()
    zero[:, 10] = 0.0
    dup = good.copy()
    dup[:, 40] = dup[:, 3]
    thresh = EPS * m
    J = np.stack([good, zero, good, dup, good])
    C, rcond, status = bounded_lsq.covariance(J, ctx=ctx)
    print("rcond_1: regular kappa 1e6 %.3g, zero column %.3g, duplicated column %.3g, threshold %.3g"
          % (rcond[0], rcond[1], rcond[3], thresh))
    assert list(status) == [0, 1, 0, 1, 0]
    assert rcond[1] == 0.0 and 0.0 <= rcond[3] < thresh and rcond[0] > 1e3 * thresh
    assert np.all(np.isnan(C[1])) and np.all(np.isnan(C[3]))
    # the regular neighbours' bits are unchanged by the singular ones
    alone = bounded_lsq.covariance(good, ctx=ctx)
    for b in (0, 2, 4):
        assert np.array_equal(C[b], alone[0]) and rcond[b] == alone[1]
    # m < n: singular, not an error
    wide = rng.standard_normal((3, 20, 31))
    C, rcond, status = bounded_lsq.covariance(wide, ctx=ctx)
    assert np.all(status == 1) and np.all(np.isnan(C))
    # ... but regular once enough variables are held fixed (m >= |F|)
    mask = np.zeros((3, 31), dtype=int)
    mask[:, 12:] = 1
    C, rcond, status = bounded_lsq.covariance(wide, mask, ctx=ctx)
    assert np.all(status == 0)
    _check(np.ascontiguousarray(C[1][:12, :12]), np.ascontiguousarray(wide[1][:, :12]), "20x31 with 19 held fixed")


def test_singular_and_regular_side_by_side_in_a_batch_solve(ctx):
    import bounded_lsq
    t = np.linspace(0.0, 1.0, 25)
    Y = np.stack([(1.0 + b) * np.exp(-(0.5 + 0.2 * b) * t) for b in range(4)])
    dead = np.array([0.0, 1.0, 0.0, 1.0])          # problems 1 and 3 do not depend on their third parameter

    def fun(X):
        return X[:, :1] * np.exp(X[:, 1:2] * t[None]) + ((1 - dead) * X[:, 2])[:, None] * t[None] - Y

    def jac(X):
        e = np.exp(X[:, 1:2] * t[None])
        return np.stack([e, X[:, :1] * t[None] * e, (1 - dead)[:, None] * np.broadcast_to(t, (4, 25))], 2)

    X0 = np.tile([1.0, -1.0, 0.1], (4, 1))
    for driver in ('host', 'device'):
        res = bounded_lsq.least_squares_batch(fun, X0, jac, driver=driver, ctx=ctx, covariance=True)
        for b, r in enumerate(res):
            if dead[b]:
                assert r.x_covariance is None and r.x_covariance_rcond == 0.0, (driver, b)
            else:
                assert r.x_covariance is not None and r.x_covariance_rcond > 0, (driver, b)
                one = bounded_lsq.covariance(r.jac, ctx=ctx)
                assert np.array_equal(r.x_covariance, one[0]) and r.x_covariance_rcond == one[1], (driver, b)


# ---- end to end ----------------------------------------------------------------------------------
EXP_BOX = ([0.0, -2.0, 0.0, 0.0], [1.5, 0.0, 3.0, 2.0])     # the fit of tests/_problems.py: a = 2 is cut off at 1.5


def _expfit_batch(seeds):
    pairs = [expfit_problem(s) for s in seeds]
    return (lambda X: np.stack([p[0](x) for p, x in zip(pairs, X)]),
            lambda X: np.stack([p[1](x) for p, x in zip(pairs, X)]), pairs)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("mode", [True, "free"])
def test_end_to_end_three_ways(ctx, method, mode):
    import bounded_lsq
    from bounded_lsq import OuterDriver
    from bounded_lsq._hostmath import shift_into_interior
    seeds = [3, 4, 5]
    fun, jac, pairs = _expfit_batch(seeds)
    B, n, m = len(seeds), 4, 40
    X0 = np.tile(EXPFIT_X0, (B, 1))
    lb, ub = np.array(EXP_BOX[0]), np.array(EXP_BOX[1])
    seq = [bounded_lsq.least_squares(p[0], EXPFIT_X0, p[1], bounds=EXP_BOX, method=method, covariance=mode,
                                     options={"ctx": ctx}) for p in pairs]
    host = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver='host', ctx=ctx,
                                           covariance=mode)
    dev = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver='device', ctx=ctx,
                                          covariance=mode)
    # the driver itself
    drv = OuterDriver(method, B, m, n, ctx=ctx)
    try:
        xs = np.stack([shift_into_interior(X0[b], lb, ub, rstep=1e-10) for b in range(B)]) if method == 'trf' else X0
        drv.start(X0, xs, lb, ub, np.ones((B, n)), False, EPS ** 0.5, EPS ** 0.5, EPS ** 0.5, 100 * n)
        R = drv.run_host(fun, jac)
        Cd, rd, sd = drv.covariance(free_only=(mode == 'free'))
    finally:
        drv.close()
    print("%s: active masks %s" % (method, [list(r.active_mask) for r in seq]))
    if method == 'dogbox':
        assert any(np.any(r.active_mask != 0) for r in seq), "the fit must end on a bound"
    for b in range(B):
        s, h, d = seq[b], host[b], dev[b]
        assert s.x_covariance is not None and s.x_covariance_rcond > 0
        assert np.array_equal(s.active_mask, h.active_mask) and np.array_equal(s.active_mask, d.active_mask)
        if mode == 'free':
            A = np.nonzero(s.active_mask != 0)[0]
            F = np.nonzero(s.active_mask == 0)[0]
            Jref = np.ascontiguousarray(s.jac[:, F])
            for r in (s, h, d):
                assert np.all(r.x_covariance[A] == 0.0) and np.all(r.x_covariance[:, A] == 0.0)
        else:
            F = np.arange(n)
            Jref = s.jac
        rec = ref.reference(Jref)
        for name, r in (("sequential", s), ("host driver", h), ("device driver", d)):
            if np.array_equal(r.jac, s.jac):
                assert np.array_equal(r.x_covariance, s.x_covariance), (name, b)
                assert r.x_covariance_rcond == s.x_covariance_rcond
            _check(np.ascontiguousarray(r.x_covariance[np.ix_(F, F)]), Jref, "%s %s %s, problem %d"
                   % (method, mode, name, b), rec if np.array_equal(r.jac, s.jac) else ref.reference(
                       np.ascontiguousarray(r.jac[:, F])))
        assert sd[b] == 0 and np.array_equal(Cd[b], d.x_covariance) and rd[b] == d.x_covariance_rcond


@pytest.mark.parametrize("driver", ["sequential", "host", "device"])
def test_soft_l1_covariance_is_that_of_the_scaled_jacobian(ctx, driver):
    import bounded_lsq
    seeds = [3, 4]
    fun, jac, pairs = _expfit_batch(seeds)
    X0 = np.tile(EXPFIT_X0, (2, 1))
    if driver == "sequential":
        res = [bounded_lsq.least_squares(p[0], EXPFIT_X0, p[1], bounds=EXP_BOX, loss='soft_l1', f_scale=0.02,
                                         covariance=True, options={"ctx": ctx}) for p in pairs]
    else:
        res = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, loss='soft_l1', f_scale=0.02,
                                              driver=driver, ctx=ctx, covariance=True)
    for b, r in enumerate(res):
        plain = pairs[b][1](r.x)
        assert not np.allclose(r.jac, plain), "the loss must have scaled the Jacobian"
        C, rcond, status = bounded_lsq.covariance(r.jac, ctx=ctx)
        assert status == 0 and np.array_equal(r.x_covariance, C) and r.x_covariance_rcond == rcond
        _check(r.x_covariance, r.jac, "soft_l1 %s, problem %d" % (driver, b))


def test_default_leaves_results_as_they_were(ctx):
    import bounded_lsq
    fun, jac, pairs = _expfit_batch([3, 4])
    X0 = np.tile(EXPFIT_X0, (2, 1))
    fields = ("x", "fun", "jac", "obj_value", "optimality", "active_mask", "nfev", "njev", "status", "message",
              "success")

    def same(a, b):
        assert sorted(a.keys()) == sorted(list(fields) + ["x_covariance"])
        assert a.x_covariance is None
        for k in fields:
            assert np.array_equal(a[k], b[k]), k
        assert sorted(b.keys()) == sorted(list(fields) + ["x_covariance", "x_covariance_rcond"])

    for method in ("trf", "dogbox"):
        a = bounded_lsq.least_squares(pairs[0][0], EXPFIT_X0, pairs[0][1], bounds=EXP_BOX, method=method,
                                      options={"ctx": ctx})
        f = bounded_lsq.least_squares(pairs[0][0], EXPFIT_X0, pairs[0][1], bounds=EXP_BOX, method=method,
                                      options={"ctx": ctx}, covariance=False)
        t = bounded_lsq.least_squares(pairs[0][0], EXPFIT_X0, pairs[0][1], bounds=EXP_BOX, method=method,
                                      options={"ctx": ctx}, covariance=True)
        same(a, t)
        same(f, t)
        for driver in ("host", "device"):
            a = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver=driver, ctx=ctx)
            t = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver=driver, ctx=ctx,
                                                covariance='free')
            for ra, rt in zip(a, t):
                same(ra, rt)


def test_no_covariance_kernel_runs_by_default(ctx):
    import bounded_lsq
    fun, jac, pairs = _expfit_batch([3, 4])
    X0 = np.tile(EXPFIT_X0, (2, 1))
    slots = ("cov_gather", "cov_inverse", "cov_product")
    ctx.timing(True)
    ctx.timing_reset()
    bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, driver='device', ctx=ctx)
    ctx.sync()
    T = ctx.timing_read()
    assert all(T[s][1] == 0 for s in slots)
    ctx.timing_reset()
    bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, driver='device', ctx=ctx, covariance='free')
    ctx.sync()
    T = ctx.timing_read()
    ctx.timing(False)
    assert all(T[s][1] == 1 for s in slots), {s: T[s] for s in slots}


# ---- tie to the reference ------------------------------------------------------------------------
def test_agrees_with_the_reference_minpack_bridge(ctx):
    """tests/golden/cov_lm.json: x_covariance of the reference's least_squares(method='lm', scaling='jac') and d, the
    scaled difference to inv(J^T J) of the reference's own trf result.  Ours may differ by 10 d plus the parity floor."""
    import bounded_lsq
    gold = json.load(open(os.path.join(HERE, "golden", "cov_lm.json")))
    assert len(gold) == 3
    for name, g in sorted(gold.items()):
        p = SUITE_BY_NAME[name]
        Clm = np.array([[float.fromhex(v) for v in row] for row in g["x_covariance"]])
        n = Clm.shape[0]
        r = bounded_lsq.least_squares(p["fun"], p["x0"], p["jac"], method='trf', scaling='jac', covariance=True,
                                      options={"ctx": ctx})
        assert r.x_covariance is not None
        s = np.sqrt(np.diag(Clm))
        diff = float(np.max(np.abs(r.x_covariance - Clm) / np.outer(s, s)))
        bound = 10 * g["d"] + 8 * n * EPS
        print("%s: difference to the reference's lm covariance %.3g, d = %.3g, bound %.3g" % (name, diff, g["d"], bound))
        assert diff <= bound, (name, diff, bound)


# ---- C-ABI on device pointers --------------------------------------------------------------------
def test_device_pointer_call_and_argument_errors(ctx):
    import ctypes as C
    import bounded_lsq
    from bounded_lsq._abi import vp, BlsqError
    rng = np.random.default_rng(17)
    B, m, n = 3, 90, 33
    J = rng.standard_normal((B, m, n))
    mask = (rng.uniform(size=(B, n)) < 0.3).astype(np.int64)
    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "create")
    try:
        dJ, dM = ctx.to_device(J), ctx.to_device(mask)
        dC, dr, ds = ctx.malloc(B * n * n * 8), ctx.malloc(B * 8), ctx.malloc(B * 4)
        for dmask, hmask in ((None, None), (dM, mask)):
            ctx.check(ctx.lib.blsq_cov_dev(h, dJ, dmask, dC, dr, ds), "blsq_cov_dev")
            ctx.sync()
            got = (ctx.to_host(dC, (B, n, n), np.float64), ctx.to_host(dr, (B,), np.float64),
                   ctx.to_host(ds, (B,), np.int32))
            want = bounded_lsq.covariance(J, hmask, ctx=ctx)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(ctx.to_host(dJ, (B, m, n), np.float64), J), "J must not be modified"
        assert ctx.lib.blsq_cov_dev(h, None, None, dC, dr, ds) == -2
        assert ctx.lib.blsq_cov_dev(h, dJ, None, None, dr, ds) == -4
        for p in (dJ, dM, dC, dr, ds):
            ctx.free(p)
    finally:
        ctx.lib.blsq_cov_plan_destroy(h)
    bad = vp()
    assert ctx.lib.blsq_cov_plan_create(ctx.h, 1, 2000, 1010, C.byref(bad)) < 0     # m > 1024 needs n + 1 <= 1008
    assert ctx.lib.blsq_cov_plan_create(ctx.h, 1, 10, 1024, C.byref(bad)) < 0       # n + 1 <= 1024
    assert ctx.lib.blsq_cov_plan_create(ctx.h, 0, 10, 4, C.byref(bad)) == -2
    with pytest.raises(BlsqError):
        bounded_lsq.covariance(np.ones((1100, 1010)), ctx=ctx)
