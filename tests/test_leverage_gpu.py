"""Leverages and prediction variances on the GPU (blsq_cov_rows*, blsq_outer_leverage, `leverage=` of the front ends)
against the checked extended-precision references of tests/_lev_ref.py.

Error metric: max_i |h_i - h*_i|.  Bound per case: 4 x the error of the float64 recipe that matches the route (row sums
of U^2 for the regular route, of (A V / s)^2 for the pinv route and prediction_variance; scipy.linalg.svd) against the
same reference, with a floor of 8 n eps.  Every test prints the figures it asserts on (run with -s to see them).

MI355X figures (error / bound, worst case): regular route 0.51 (65x17, kappa 1e6 with column scales), pinv route 0.065
full rank and 0.089 with a mask, prediction_variance 0.21 (regular) and 0.28 (pinv).  Before the refinement of the pinv
factor the pinv route stood at 1.87 x its bound at 1030x272: error 9.0e-13, bound 4.8e-13."""
import ctypes as C

import numpy as np
import pytest

import _cov_ref as cref
import _lev_ref as ref
from _problems import expfit_problem, EXPFIT_X0

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


# ---- the cases and their references (each computed once, shared, never modified) --------------------------------
#        m     n    kappa  column scales
REGULAR = [(17, 1, 1.0, False), (16, 16, 1e2, False), (64, 16, 1e2, False), (65, 17, 1e6, True),
           (200, 33, 1e4, True), (512, 64, 1e3, False), (63, 15, 1e2, False),          # tile and chunk edges
           (1000, 40, 1e4, True),                                                      # many chunks
           (1100, 256, 1e2, False), (1030, 272, 1e3, True), (700, 300, 1e2, False),    # X beyond LDS, n > 256
           (1100, 520, 1e2, False)]                                                    # the fold plan
PINV_FULL = [(65, 17, 1e6, True), (200, 33, 1e4, True), (1030, 272, 1e3, True)]
PINV_DEFICIENT = [(64, 13, 3), (200, 28, 5), (40, 12, 12)]      # m, independent columns, exact duplicates appended


def _ids(cases):
    return ["x".join(str(v) for v in c[:2]) + "".join("-%g" % v for v in c[2:3]) for c in cases]


_cache = {}


def _jacobian(case):
    if ("J", case) not in _cache:
        m, n, kappa, scales = case
        rng = np.random.default_rng(1000 + 7 * m + n)
        J = ref.make_jacobian(rng, m, n, kappa, column_scales=scales)
        J.setflags(write=False)
        _cache["J", case] = J
    return _cache["J", case]


def _reference(case, route):
    """the checked reference of a case's leverages with the bound of `route` ('regular' / 'pinv'); the two
    extended-precision evaluations are shared between the routes"""
    if ("ref", case, route) not in _cache:
        J = _jacobian(case)
        other = _cache.get(("ref", case, "pinv" if route == "regular" else "regular"))
        recipe = ref.recipe_regular(J) if route == "regular" else ref.recipe_rows(J, J)
        _cache["ref", case, route] = ref.reference(J, recipe=recipe, base=other)
    return _cache["ref", case, route]


def _report(label, h, r, extra=""):
    err = ref.lev_error(h, r["h"])
    print("%s: error %.3g, bound %.3g (recipe %.3g, reference %.3g, %s), ratio to bound %.3g%s"
          % (label, err, r["bound"], r["err_recipe"], r["err_reference"], r["kind"], err / r["bound"], extra))
    return err


# ---- 1. parity, regular route ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REGULAR, ids=_ids(REGULAR))
def test_parity_regular(ctx, case):
    import bounded_lsq
    m, n = case[:2]
    J = _jacobian(case)
    h, p, status = bounded_lsq.leverage(J, ctx=ctx)
    r = _reference(case, "regular")
    assert status == 0 and p == n and h.shape == (m,)
    err = _report("regular %dx%d kappa %g" % case[:3], h, r, ", sum h - n = %.3g" % (float(np.sum(h)) - n))
    assert err <= r["bound"], (case, err, r["bound"])
    assert np.all(h >= 0.0) and np.all(h <= 1.0 + r["bound"])
    assert abs(float(np.sum(h.astype(LD))) - n) <= m * r["bound"]
    assert r["kind"] == ("mpmath" if m <= 512 and n <= 64 else "longdouble")


# ---- 2. parity, pinv route ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PINV_FULL, ids=_ids(PINV_FULL))
def test_parity_pinv_full_rank(ctx, case):
    import bounded_lsq
    m, n = case[:2]
    J = _jacobian(case)
    h, p, status = bounded_lsq.leverage(J, ctx=ctx, pinv=True)
    r = _reference(case, "pinv")
    assert status == 0 and p == n
    err = _report("pinv %dx%d kappa %g" % case[:3], h, r)
    assert err <= r["bound"], (case, err, r["bound"])
    assert np.all(h >= 0.0) and np.all(h <= 1.0 + r["bound"])
    assert abs(float(np.sum(h.astype(LD))) - n) <= m * r["bound"]


@pytest.mark.parametrize("m,k,d", PINV_DEFICIENT, ids=["%dx(%d+%d)" % c for c in PINV_DEFICIENT])
def test_parity_pinv_rank_deficient(ctx, m, k, d):
    """[A, A[:, :d]]: exact duplicate columns.  h* is the leverage of A alone, p = rank(A), sum h = p."""
    import bounded_lsq
    rng = np.random.default_rng(2000 + m + k)
    A = ref.make_jacobian(rng, m, k, 1e2)
    J = np.ascontiguousarray(np.hstack([A, A[:, :d]]))
    h, p, status = bounded_lsq.leverage(J, ctx=ctx, pinv=True)
    r = ref.reference(A, recipe=ref.recipe_rows(J, J), n_floor=k + d)
    assert status == 0 and p == k, (status, p)
    err = _report("pinv %dx(%d+%d)" % (m, k, d), h, r, ", sum h - p = %.3g" % (float(np.sum(h)) - p))
    assert err <= r["bound"], (err, r["bound"])
    assert abs(float(np.sum(h.astype(LD))) - p) <= m * r["bound"]
    # the regular route calls the same matrix singular: NaN rows, never a wrong number
    h1, p1, s1 = bounded_lsq.leverage(J, ctx=ctx)
    assert s1 == 1 and np.all(np.isnan(h1))


def test_parity_pinv_wide(ctx):
    """20 x 30 standard normal: the rows span their own space, so p = 20 and h* = 1 exactly (the hat matrix is I)."""
    import bounded_lsq
    J = np.random.default_rng(2030).standard_normal((20, 30))
    h, p, status = bounded_lsq.leverage(J, ctx=ctx, pinv=True)
    err_rec = float(np.max(np.abs(ref.recipe_rows(J, J) - 1.0)))
    bound = max(4 * err_rec, 8 * 30 * EPS)
    err = float(np.max(np.abs(h - 1.0)))
    print("pinv 20x30: error %.3g, bound %.3g (recipe %.3g), ratio to bound %.3g" % (err, bound, err_rec, err / bound))
    assert status == 0 and p == 20
    assert err <= bound


# ---- 3. free masks ---------------------------------------------------------------------------------------
def _free_batch():
    rng = np.random.default_rng(3096)
    m, n = 96, 20
    J = np.stack([ref.make_jacobian(rng, m, n, 1e2) for _ in range(5)])
    M = np.zeros((5, n), dtype=int)
    M[1, 11] = 1                                                  # nf = 19
    M[2] = 1
    M[2, [0, 3, 4, 9, 13, 16, 19]] = 0                            # nf = 7, scattered
    M[3] = -1
    M[3, 8] = 0                                                   # nf = 1
    M[4] = 1                                                      # nf = 0
    return J, M, [20, 19, 7, 1, 0]


@pytest.mark.parametrize("pinv", [False, True], ids=["regular", "pinv"])
def test_free_masks(ctx, pinv):
    import bounded_lsq
    J, M, nfs = _free_batch()
    h, p, status = bounded_lsq.leverage(J, M, ctx=ctx, pinv=pinv)
    assert h.shape == (5, 96) and list(p) == nfs and np.all(status == 0)
    assert np.all(h[4] == 0.0) and not np.any(np.signbit(h[4]))
    for b in range(4):
        Jf = np.ascontiguousarray(J[b][:, M[b] == 0])
        key = ("free", b)
        if key not in _cache:
            _cache[key] = ref.reference(Jf)
        r = ref.reference(Jf, recipe=ref.recipe_rows(Jf, Jf), base=_cache[key]) if pinv else _cache[key]
        alone, pa, sa = bounded_lsq.leverage(Jf, ctx=ctx, pinv=pinv)
        diff = float(np.max(np.abs(h[b] - alone)))
        err = _report("free %s nf = %d" % ("pinv" if pinv else "regular", nfs[b]), h[b], r,
                      ", difference to the columns alone %.3g" % diff)
        assert sa == 0 and pa == nfs[b]
        assert diff <= 2 * r["bound"], (b, diff, r["bound"])
        assert err <= r["bound"], (b, err, r["bound"])


# ---- 4. singular beside regular ----------------------------------------------------------------------------
def test_singular_beside_regular(ctx):
    import bounded_lsq
    rng = np.random.default_rng(4064)
    m, n = 64, 16
    J = np.stack([ref.make_jacobian(rng, m, n, 1e2) for _ in range(3)])
    J[1][:, 5] = 0.0
    h, p, status = bounded_lsq.leverage(J, ctx=ctx)
    assert list(status) == [0, 1, 0]
    assert np.all(np.isnan(h[1])) and np.all(np.isfinite(h[0])) and np.all(np.isfinite(h[2]))
    for b in (0, 2):
        alone = bounded_lsq.leverage(J[b], ctx=ctx)
        assert np.array_equal(h[b], alone[0]) and alone[2] == 0
    h, p, status = bounded_lsq.leverage(J, ctx=ctx, pinv=True)
    assert list(status) == [0, 0, 0] and list(p) == [n, n - 1, n]
    assert np.all(np.isfinite(h))
    Jf = np.ascontiguousarray(np.delete(J[1], 5, axis=1))
    r = ref.reference(Jf, recipe=ref.recipe_rows(J[1], J[1]), n_floor=n)
    err = _report("pinv with a zero column", h[1], r)
    assert err <= r["bound"]


# ---- 5. bits ---------------------------------------------------------------------------------------------
def test_bits(ctx):
    import bounded_lsq
    rng = np.random.default_rng(5128)
    J = np.stack([ref.make_jacobian(rng, 128, 24, 10.0 ** rng.uniform(0.3, 3.0)) for _ in range(37)])
    for pinv in (False, True):
        h, p, status = bounded_lsq.leverage(J, ctx=ctx, pinv=pinv)
        again = bounded_lsq.leverage(J, ctx=ctx, pinv=pinv)
        assert np.all(status == 0) and np.array_equal(h, again[0])
        for b in (0, 17, 36):
            alone = bounded_lsq.leverage(J[b], ctx=ctx, pinv=pinv)
            assert np.array_equal(h[b], alone[0]), (pinv, b)
        A = rng.standard_normal((65, 24))
        v65, _ = bounded_lsq.prediction_variance(J[3], A, ctx=ctx, pinv=pinv)
        v16, _ = bounded_lsq.prediction_variance(J[3], A[:16], ctx=ctx, pinv=pinv)
        assert v65.shape == (65,) and np.array_equal(v65[:16], v16), pinv


# ---- 6. prediction_variance ----------------------------------------------------------------------------------
PV_CASE = (200, 33, 1e4, True)
PV_ACTIVE = [0, 5, 6, 20, 32]


def _pv_reference(masked):
    """C* of the fit (the checked reference of tests/_cov_ref.py) over the free columns"""
    key = ("pv", masked)
    if key not in _cache:
        J = _jacobian(PV_CASE)
        F = np.setdiff1d(np.arange(33), PV_ACTIVE) if masked else np.arange(33)
        _cache[key] = (F, cref.reference(np.ascontiguousarray(J[:, F]))["C"])
    return _cache[key]


@pytest.mark.parametrize("masked", [False, True], ids=["all free", "masked"])
@pytest.mark.parametrize("pinv", [False, True], ids=["regular", "pinv"])
def test_prediction_variance(ctx, pinv, masked):
    import bounded_lsq
    J = _jacobian(PV_CASE)
    m, n = J.shape
    F, Cstar = _pv_reference(masked)
    mask = None
    if masked:
        mask = np.zeros(n, dtype=int)
        mask[PV_ACTIVE] = 1
    Jf = np.ascontiguousarray(J[:, F])
    rng = np.random.default_rng(6200)
    for m_new in (1, 17, 300):
        A = (rng.standard_normal((m_new, m)) / np.sqrt(m)) @ J       # rows of order one in the metric of the fit
        Af = np.ascontiguousarray(A[:, F])
        want = np.sum((Af.astype(LD) @ Cstar) * Af.astype(LD), axis=1)
        err_rec = float(np.max(np.abs(ref.recipe_rows(Jf, Af) - want)))
        bound = max(4 * err_rec, 8 * n * EPS)
        if masked:
            A[:, PV_ACTIVE] = 1e300                                  # never read: the parameters are held fixed
        var, status = bounded_lsq.prediction_variance(J, A, mask, ctx=ctx, pinv=pinv)
        err = float(np.max(np.abs(var.astype(LD) - want)))
        print("prediction_variance %s %s m_new = %d: error %.3g, bound %.3g (recipe %.3g), ratio to bound %.3g"
              % ("pinv" if pinv else "regular", "masked" if masked else "all free", m_new, err, bound, err_rec,
                 err / bound))
        assert status == 0 and var.shape == (m_new,)
        assert err <= bound, (m_new, err, bound)
        # scalar scale, and (B,) scales on a batch of the same fit: times the scale, under the scaled bound
        v3, _ = bounded_lsq.prediction_variance(J, A, mask, ctx=ctx, pinv=pinv, scale=3.0)
        assert float(np.max(np.abs(v3.astype(LD) - 3.0 * want))) <= 3.0 * bound
        sc = np.array([0.5, 7.0])
        Jb = np.stack([J, J])
        vb, sb = bounded_lsq.prediction_variance(Jb, np.stack([A, A]), None if mask is None else np.stack([mask, mask]),
                                                 ctx=ctx, pinv=pinv, scale=sc)
        assert vb.shape == (2, m_new) and np.all(sb == 0)
        for b in range(2):
            assert float(np.max(np.abs(vb[b].astype(LD) - sc[b] * want))) <= sc[b] * bound, (m_new, b)
        shared, _ = bounded_lsq.prediction_variance(Jb, A, None if mask is None else np.stack([mask, mask]), ctx=ctx,
                                                    pinv=pinv, scale=sc)
        assert np.array_equal(shared, vb)                            # a 2-D J_new serves every problem


# ---- 7. ABI rules ----------------------------------------------------------------------------------------
def test_abi_rules(ctx):
    import bounded_lsq
    from bounded_lsq._abi import vp, ptr
    rng = np.random.default_rng(7090)
    B, m, n = 3, 90, 33
    J = rng.standard_normal((B, m, n))
    mask = (rng.uniform(size=(B, n)) < 0.3).astype(np.int64)
    big = rng.standard_normal((B, 3 * m + 5, n))
    lib = ctx.lib
    h = vp()
    ctx.check(lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "create")
    try:
        dJ, dM, dbig = ctx.to_device(J), ctx.to_device(mask), ctx.to_device(big)
        dC, dr, ds = ctx.malloc(B * n * n * 8), ctx.malloc(B * 8), ctx.malloc(B * 4)
        dk, dR, dK = ctx.malloc(B * 4), ctx.malloc(B * 8), ctx.malloc(B * 8)
        dout, dbo = ctx.malloc(B * m * 8), ctx.malloc(B * big.shape[1] * 8)
        out = np.empty((B, m))
        # before any covariance call: a bad-argument error with a message, on both entries
        assert lib.blsq_cov_rows_dev(h, m, dJ, None, dout) < 0
        assert b"no covariance factor yet" in lib.blsq_last_error(ctx.h)
        assert lib.blsq_cov_rows(h, m, ptr(J), None, ptr(out)) < 0
        assert b"no covariance factor yet" in lib.blsq_last_error(ctx.h)
        cov, rcond, status = np.empty((B, n, n)), np.empty(B), np.empty(B, dtype=np.int32)
        for pinv in (False, True):
            for dmask, hmask in ((None, None), (dM, mask)):
                # device pointers: equal to the host-pointer results bit for bit
                if pinv:
                    ctx.check(lib.blsq_cov_pinv_dev(h, dJ, dmask, None, dC, dk, dr, dK, ds), "blsq_cov_pinv_dev")
                else:
                    ctx.check(lib.blsq_cov_dev(h, dJ, dmask, dC, dr, ds), "blsq_cov_dev")
                ctx.check(lib.blsq_cov_rows_dev(h, m, dJ, None, dout), "blsq_cov_rows_dev")
                ctx.check(lib.blsq_cov_rows_dev(h, big.shape[1], dbig, None, dbo), "blsq_cov_rows_dev")   # rows > m
                ctx.sync()
                got = ctx.to_host(dout, (B, m), np.float64)
                want = bounded_lsq.leverage(J, hmask, ctx=ctx, pinv=pinv)[0]
                assert np.array_equal(got, want), (pinv, hmask is not None)
                gotb = ctx.to_host(dbo, (B, big.shape[1]), np.float64)
                wantb = bounded_lsq.prediction_variance(J, big, hmask, ctx=ctx, pinv=pinv)[0]
                assert np.array_equal(gotb, wantb), (pinv, hmask is not None)
                # a device-pointer covariance call stages no J: A = NULL is an error
                assert lib.blsq_cov_rows(h, m, None, None, ptr(out)) < 0
        assert np.array_equal(ctx.to_host(dJ, (B, m, n), np.float64), J), "J must not be modified"
        # host pointers: A = NULL is the staged J, and needs rows == m
        ctx.check(lib.blsq_cov(h, ptr(J), ptr(mask), ptr(cov), ptr(rcond), ptr(status)), "blsq_cov")
        assert lib.blsq_cov_rows(h, m - 1, None, None, ptr(out)) < 0
        assert lib.blsq_cov_rows(h, m + 1, None, None, ptr(out)) < 0
        ctx.check(lib.blsq_cov_rows(h, m, None, None, ptr(out)), "blsq_cov_rows")
        assert np.array_equal(out, bounded_lsq.leverage(J, mask, ctx=ctx)[0])
        outb = np.empty((B, big.shape[1]))
        sc = np.array([1.0, 2.0, 0.25])
        ctx.check(lib.blsq_cov_rows(h, big.shape[1], ptr(big), ptr(sc), ptr(outb)), "blsq_cov_rows")      # rows > m
        assert np.array_equal(outb, bounded_lsq.prediction_variance(J, big, mask, ctx=ctx, scale=sc)[0])
        assert lib.blsq_cov_rows_dev(h, 0, dJ, None, dout) == -2
        assert lib.blsq_cov_rows_dev(h, m, None, None, dout) == -3
        assert lib.blsq_cov_rows_dev(h, m, dJ, None, None) == -5
        for p in (dJ, dM, dbig, dC, dr, ds, dk, dR, dK, dout, dbo):
            ctx.free(p)
    finally:
        lib.blsq_cov_plan_destroy(h)


# ---- 8. front ends -----------------------------------------------------------------------------------------
EXP_BOX = ([0.0, -2.0, 0.0, 0.0], [1.5, 0.0, 3.0, 2.0])     # the fit of tests/_problems.py: a = 2 is cut off at 1.5
FIELDS = ["x", "fun", "jac", "obj_value", "optimality", "active_mask", "nfev", "njev", "status", "message", "success",
          "x_covariance"]


def _expfit_batch(seeds):
    pairs = [expfit_problem(s) for s in seeds]
    return (lambda X: np.stack([p[0](x) for p, x in zip(pairs, X)]),
            lambda X: np.stack([p[1](x) for p, x in zip(pairs, X)]), pairs)


@pytest.mark.parametrize("mode", [True, "free", "pinv"], ids=["True", "free", "pinv"])
def test_front_ends_three_ways(ctx, mode):
    import bounded_lsq
    seeds = [3, 4, 5]
    fun, jac, pairs = _expfit_batch(seeds)
    B = len(seeds)
    X0 = np.tile(EXPFIT_X0, (B, 1))
    method = 'dogbox' if mode == 'free' else 'trf'              # (dogbox ends on the bound: a real mask)
    seq = [bounded_lsq.least_squares(p[0], EXPFIT_X0, p[1], bounds=EXP_BOX, method=method, covariance=mode,
                                     leverage=True, options={"ctx": ctx}) for p in pairs]
    host = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver='host', ctx=ctx,
                                           covariance=mode, leverage=True)
    dev = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver='device', ctx=ctx,
                                          covariance=mode, leverage=True)
    plain = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, method=method, driver='device', ctx=ctx,
                                            covariance=mode)
    extra = ["x_covariance_rcond"] + (["x_covariance_rank"] if mode == "pinv" else [])
    if mode == 'free':
        assert any(np.any(r.active_mask != 0) for r in seq), "the fit must end on a bound"
    for b in range(B):
        s, h, d = seq[b], host[b], dev[b]
        assert sorted(plain[b].keys()) == sorted(FIELDS + extra)              # without leverage: today's keys
        for name, r in (("sequential", s), ("host driver", h), ("device driver", d)):
            assert sorted(r.keys()) == sorted(FIELDS + extra + ["leverage"]), name
            assert r.x_covariance is not None and r.leverage.shape == (40,), name
            one = bounded_lsq.leverage(r.jac, r.active_mask if mode == 'free' else None, ctx=ctx, pinv=(mode == 'pinv'))
            assert one[2] == 0 and np.array_equal(r.leverage, one[0]), name
            assert float(np.max(np.abs(r.leverage - s.leverage))) <= 1e-12, name
        nf = int(np.count_nonzero(s.active_mask == 0)) if mode == 'free' else 4
        print("%s %s problem %d: sum h = %.15g (p = %d)" % (method, mode, b, float(np.sum(s.leverage)), nf))
        assert abs(float(np.sum(s.leverage)) - nf) <= 1e-10


def test_default_results_and_timing(ctx):
    """`cov_rows` runs exactly once with leverage=True and never otherwise; the default adds no key."""
    import bounded_lsq
    fun, jac, pairs = _expfit_batch([3, 4])
    X0 = np.tile(EXPFIT_X0, (2, 1))
    ctx.timing(True)
    counts = []
    for kw in ({}, {"covariance": True}, {"covariance": True, "leverage": True}):
        ctx.timing_reset()
        res = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, driver='device', ctx=ctx, **kw)
        ctx.sync()
        counts.append(ctx.timing_read()["cov_rows"][1])
        want = FIELDS + (["x_covariance_rcond"] if kw else []) + (["leverage"] if "leverage" in kw else [])
        assert all(sorted(r.keys()) == sorted(want) for r in res), kw
    ctx.timing(False)
    assert counts == [0, 0, 1], counts
    a = bounded_lsq.least_squares(pairs[0][0], EXPFIT_X0, pairs[0][1], bounds=EXP_BOX, options={"ctx": ctx})
    f = bounded_lsq.least_squares(pairs[0][0], EXPFIT_X0, pairs[0][1], bounds=EXP_BOX, options={"ctx": ctx},
                                  leverage=False)
    assert sorted(a.keys()) == sorted(f.keys()) == sorted(FIELDS)


def test_curve_fit_carries_the_leverage(ctx):
    import bounded_lsq
    rng = np.random.default_rng(8040)
    t = np.linspace(0.0, 4.0, 40)

    def model(t, a, b, c):
        return a * np.exp(b * t) + c

    def mjac(t, a, b, c):
        return np.stack([np.exp(b * t), a * t * np.exp(b * t), np.ones_like(t)], 1)

    y = model(t, 2.0, -0.7, 0.5) + 0.01 * rng.standard_normal(40)
    popt, pcov, info, mesg, ier = bounded_lsq.curve_fit(model, t, y, p0=[1.0, -0.1, 0.0], jac=mjac, full_output=True,
                                                        leverage=True, options={"ctx": ctx})
    assert sorted(info) == ["fvec", "leverage", "nfev"] and info["leverage"].shape == (40,)
    assert abs(float(np.sum(info["leverage"])) - 3) <= 1e-10
    popt2, pcov2, info2, _, _ = bounded_lsq.curve_fit(model, t, y, p0=[1.0, -0.1, 0.0], jac=mjac, full_output=True,
                                                      options={"ctx": ctx})
    assert sorted(info2) == ["fvec", "nfev"] and np.array_equal(popt, popt2) and np.array_equal(pcov, pcov2)
    # the band of the docstring's recipe: variance of the fitted curve at new abscissae
    Jm = mjac(t, *popt)
    s2 = float(np.sum(info["fvec"] ** 2)) / (40 - 3)
    var, status = bounded_lsq.prediction_variance(Jm, Jm[::7], ctx=ctx, pinv=True, scale=s2)
    want = np.einsum("ij,jk,ik->i", Jm[::7], pcov, Jm[::7])
    assert status == 0 and np.allclose(var, want, rtol=1e-6, atol=0.0)


def test_outer_driver_leverage_needs_a_fresh_factor(ctx):
    import bounded_lsq
    from bounded_lsq import OuterDriver
    from bounded_lsq._abi import BlsqError
    from bounded_lsq._hostmath import shift_into_interior
    fun, jac, pairs = _expfit_batch([3, 4])
    B, n, m = 2, 4, 40
    X0 = np.tile(EXPFIT_X0, (B, 1))
    lb, ub = np.array(EXP_BOX[0]), np.array(EXP_BOX[1])
    xs = np.stack([shift_into_interior(X0[b], lb, ub, rstep=1e-10) for b in range(B)])
    drv = OuterDriver('trf', B, m, n, ctx=ctx)
    try:
        drv.start(X0, xs, lb, ub, np.ones((B, n)), False, EPS ** 0.5, EPS ** 0.5, EPS ** 0.5, 100 * n)
        drv._up(drv.d_f, fun(xs), (B, m), "fun")
        drv._up(drv.d_J, jac(xs), (B, m, n), "jac")
        drv.begin()
        with pytest.raises(BlsqError, match="no current covariance factor"):
            drv.leverage()
        C0, r0, s0 = drv.covariance()
        h, status = drv.leverage()
        assert np.all(status == 0) and np.array_equal(h, bounded_lsq.leverage(jac(xs), ctx=ctx)[0])
        assert drv.propose() >= 0                                  # the factor is stale from here on
        with pytest.raises(BlsqError, match="no current covariance factor"):
            drv.leverage()
    finally:
        drv.close()


def test_soft_l1_leverage_is_that_of_the_scaled_jacobian(ctx):
    import bounded_lsq
    fun, jac, pairs = _expfit_batch([3, 4])
    X0 = np.tile(EXPFIT_X0, (2, 1))
    res = bounded_lsq.least_squares_batch(fun, X0, jac, bounds=EXP_BOX, loss='soft_l1', f_scale=0.02, driver='device',
                                          ctx=ctx, covariance=True, leverage=True)
    for b, r in enumerate(res):
        assert not np.allclose(r.jac, pairs[b][1](r.x)), "the loss must have scaled the Jacobian"
        h, p, status = bounded_lsq.leverage(r.jac, ctx=ctx)
        assert status == 0 and np.array_equal(r.leverage, h)
        hp = bounded_lsq.leverage(pairs[b][1](r.x), ctx=ctx)[0]
        assert not np.allclose(h, hp, rtol=1e-6, atol=0.0)
