"""Robust loss functions on the GPU: the kernels (loss_kernels.hip) against the numpy restatement, 'linear' as today's
library bit for bit, the device driver's first step against the CPU oracle, end-to-end fits against
scipy.optimize.least_squares(loss=, f_scale=), and the device driver's Jacobian never scaled twice."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LOSSES = ['linear', 'huber', 'soft_l1', 'cauchy', 'arctan']
ROBUST = LOSSES[1:]


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


def _check_w_and_fs(w_dev, fs_dev, f, rho):
    """w and f_s of the kernel against the numpy restatement: within 4 ulp relative, on top of the rounding bound of
    scipy's rho1 + 2 rho2 f^2 where its two terms cancel (huber / soft_l1 beyond f_scale: the sum is a small
    difference of two numbers whose own last bits differ between numpy's `**` and the device's sqrt / division;
    numpy's power is not correctly rounded, so no implementation can match its bits there)."""
    r1, r2 = rho[1], rho[2]
    with np.errstate(all='ignore'):
        a, t = r1, 2 * r2 * f ** 2
        js = a + t
        slack = 4 * EPS * (np.abs(a) + np.abs(t))
        w_lo = np.sqrt(np.maximum(js - slack, EPS)) * (1 - 4 * EPS)
        w_hi = np.sqrt(np.maximum(js + slack, EPS)) * (1 + 4 * EPS)
        nan = np.isnan(js)
        assert np.array_equal(np.isnan(w_dev), nan)
        ok = (w_dev >= w_lo) & (w_dev <= w_hi)
        assert ok[~nan].all(), (w_dev[~nan][~ok[~nan]][:4], js[~nan][~ok[~nan]][:4])
        # f_s = f * (rho1 / w): 4 ulp on top of w's own interval
        lo = f * (r1 / w_hi) * (1 - 4 * EPS)
        hi = f * (r1 / w_lo) * (1 + 4 * EPS)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        fin = np.isfinite(lo) & np.isfinite(hi)
        if fs_dev is None:
            return
        assert np.array_equal(np.isnan(fs_dev), np.isnan(f * (r1 / np.sqrt(np.maximum(js, EPS)))))
        ok = (fs_dev >= lo) & (fs_dev <= hi)
        assert ok[fin].all(), (fs_dev[fin][~ok[fin]][:4], lo[fin][~ok[fin]][:4], hi[fin][~ok[fin]][:4])


def _check_scaled_J(J_dev, J_true, f, rho):
    """J_dev = diag(w) J_true with w as _check_w_and_fs accepts it (w read off each row's largest entry)."""
    rows = np.arange(J_true.shape[0])
    j = np.argmax(np.abs(J_true), axis=1)
    w = J_dev[rows, j] / J_true[rows, j]
    _check_w_and_fs(w, None, f, rho)
    np.testing.assert_allclose(J_dev, J_true * w[:, None], rtol=4 * EPS, atol=0)


def _residuals(rng, B, m):
    f = rng.standard_normal((B, m)) * 10.0 ** rng.integers(-3, 3, (B, m))
    special = np.array([0.0, -0.0, 1e-150, -1e-150, 1e150, -1e150, 1.0, -1.0, np.nan, 1e-300, 3e5])
    k = min(m, special.size)
    f[:, :k] = special[:k]
    return f


def _scale_on_device(ctx, loss, fs, f, J, mask=None):
    B, m, n = J.shape
    d_fs, d_f, d_J = ctx.to_device(fs), ctx.to_device(f), ctx.to_device(J)
    d_fsc = ctx.to_device(np.full((B, m), 12345.0))
    d_mask = ctx.to_device(np.ascontiguousarray(mask, dtype=np.int32)) if mask is not None else None
    try:
        ctx.loss_scale_dev(B, m, n, LOSSES.index(loss), d_fs, d_f, d_J, d_fsc, d_mask)
        return ctx.to_host(d_J, (B, m, n), np.float64), ctx.to_host(d_fsc, (B, m), np.float64)
    finally:
        for p in (d_fs, d_f, d_J, d_fsc, d_mask):
            if p is not None:
                ctx.free(p)


def _cost_on_device(ctx, loss, fs, f, mask=None):
    B, m = f.shape
    d_fs, d_f = ctx.to_device(fs), ctx.to_device(f)
    d_obj = ctx.to_device(np.full(B, -7.0))
    d_mask = ctx.to_device(np.ascontiguousarray(mask, dtype=np.int32)) if mask is not None else None
    try:
        ctx.loss_cost_dev(B, m, LOSSES.index(loss), d_fs, d_f, d_obj, d_mask)
        return ctx.to_host(d_obj, (B,), np.float64)
    finally:
        for p in (d_fs, d_f, d_obj, d_mask):
            if p is not None:
                ctx.free(p)


# ---- 1. kernels against the numpy restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", [(5, 77, 13), (3, 301, 50), (7, 33, 1), (2, 1500, 3)])
def test_scale_and_cost_kernels_match_numpy(ctx, loss, shape):
    from bounded_lsq import _hostmath as H
    B, m, n = shape
    rng = np.random.default_rng(B * 1000 + m + n)
    f = _residuals(rng, B, m)
    fs = np.array([0.1, 1.0, 7.0, 2.5, 0.3, 1.0, 4.0][:B])
    J = rng.standard_normal((B, m, n))
    J[:, :, 0] = 1.0                                  # column 0 of the output is the kernel's own w
    J_out, fsc = _scale_on_device(ctx, loss, fs, f, J)
    for b in range(B):
        rho = H.loss_rho(loss, f[b], fs[b])
        _check_w_and_fs(J_out[b][:, 0], fsc[b], f[b], rho)      # column 0 = w
        w = J_out[b][:, :1]
        assert np.array_equal(J_out[b], J[b] * w, equal_nan=True)     # rows: w_i J_i, bit for bit
    obj = _cost_on_device(ctx, loss, fs, f)
    for b in range(B):
        fin = np.isfinite(f[b])
        rho0 = H.loss_rho(loss, f[b], fs[b])[0] / fs[b] ** 2
        if not fin.all():
            assert np.isnan(obj[b])
            continue
        want = fs[b] ** 2 * math.fsum(rho0)
        assert abs(obj[b] - want) <= 4 * EPS * abs(want), (obj[b], want)


def test_cost_skips_nan_free_problems_exactly_and_is_accurate(ctx):
    from bounded_lsq import _hostmath as H
    rng = np.random.default_rng(9)
    B, m = 6, 4099
    f = rng.standard_normal((B, m)) * 10.0 ** rng.integers(-150, 150, (B, m))
    fs = np.array([0.1, 1.0, 7.0, 0.1, 1.0, 7.0])
    for loss in LOSSES:
        obj = _cost_on_device(ctx, loss, fs, f)
        for b in range(B):
            want = fs[b] ** 2 * math.fsum(H.loss_rho(loss, f[b], fs[b])[0] / fs[b] ** 2)
            assert abs(obj[b] - want) <= 4 * EPS * abs(want), (loss, b, obj[b], want)


@pytest.mark.parametrize("shape,loss", [((1024, 512, 64), 'cauchy'), ((1, 250000, 128), 'soft_l1')])
def test_scale_kernel_large_shapes(ctx, shape, loss):
    from bounded_lsq import _hostmath as H
    B, m, n = shape
    rng = np.random.default_rng(3)
    f = rng.standard_normal((B, m)) * 3.0
    fs = np.full(B, 0.5)
    J = rng.standard_normal((B, m, n))
    J[:, :, 0] = 1.0
    mask = (np.arange(B) % 3 != 1).astype(np.int32) if B > 1 else np.ones(1, np.int32)
    J_out, fsc = _scale_on_device(ctx, loss, fs, f, J, mask)
    for b in range(B):
        if not mask[b]:
            assert J_out[b].tobytes() == J[b].tobytes()
            assert np.all(fsc[b] == 12345.0)
            continue
        if b % 97 == 0 or B == 1:                     # numpy on a sample of the problems
            _check_w_and_fs(J_out[b][:, 0], fsc[b], f[b], H.loss_rho(loss, f[b], fs[b]))
        assert np.array_equal(J_out[b], J[b] * J_out[b][:, :1])


def test_masked_problems_are_left_byte_identical(ctx):
    rng = np.random.default_rng(4)
    B, m, n = 9, 130, 17
    f, J = rng.standard_normal((B, m)), rng.standard_normal((B, m, n))
    fs = np.full(B, 0.7)
    mask = np.array([1, 0, 0, 1, 0, 1, 1, 0, 0], np.int32)
    J_out, fsc = _scale_on_device(ctx, 'huber', fs, f, J, mask)
    obj = _cost_on_device(ctx, 'huber', fs, f, mask)
    for b in range(B):
        if not mask[b]:
            assert J_out[b].tobytes() == J[b].tobytes()
            assert np.all(fsc[b] == 12345.0) and obj[b] == -7.0
        else:
            assert not np.array_equal(J_out[b], J[b])


def test_cost_bits_do_not_depend_on_the_batch(ctx):
    rng = np.random.default_rng(6)
    m = 777
    F = rng.standard_normal((300, m)) * 4.0
    fs = rng.uniform(0.2, 3.0, 300)
    for loss in ROBUST:
        big = _cost_on_device(ctx, loss, fs, F)
        for b in (0, 17, 299):
            one = _cost_on_device(ctx, loss, fs[b:b + 1], F[b:b + 1])
            assert one[0].tobytes() == big[b].tobytes(), (loss, b)


# ---- 2. 'linear' is today's library --------------------------------------------------------------------------------
def _expfit(B, m=60, seed=0, outliers=0.15):
    t = np.linspace(0, 3, m)
    truth, Y = [], []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        p = np.array([0.5 + 0.1 * b, 2.0 - 0.05 * b, -1.0 + 0.03 * b])
        y = p[0] + p[1] * np.exp(p[2] * t) + 0.02 * rng.standard_normal(m)
        k = rng.choice(m, int(outliers * m), replace=False)
        y[k] += rng.choice([-1, 1], k.size) * rng.uniform(1.0, 3.0, k.size)
        truth.append(p)
        Y.append(y)
    Y = np.array(Y)

    def fun(P):
        P = np.atleast_2d(P)
        return P[:, 0:1] + P[:, 1:2] * np.exp(P[:, 2:3] * t) - Y[:P.shape[0]]

    def jac(P):
        P = np.atleast_2d(P)
        e = np.exp(P[:, 2:3] * t)
        return np.stack([np.ones_like(e), e, P[:, 1:2] * t * e], axis=2)

    def fun_b(b):
        return lambda p: p[0] + p[1] * np.exp(p[2] * t) - Y[b]

    def jac_b(b):
        return lambda p: np.stack([np.ones_like(t), np.exp(p[2] * t), p[1] * t * np.exp(p[2] * t)], 1)
    return fun, jac, fun_b, jac_b, np.array(truth), t


def _same(r1, r2):
    assert r1.x.tobytes() == r2.x.tobytes()
    assert r1.fun.tobytes() == r2.fun.tobytes()
    assert r1.jac.tobytes() == r2.jac.tobytes()
    assert np.float64(r1.obj_value).tobytes() == np.float64(r2.obj_value).tobytes()
    assert (r1.nfev, r1.njev, r1.status) == (r2.nfev, r2.njev, r2.status)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_linear_loss_is_bit_identical_to_no_loss(ctx, method):
    from bounded_lsq import least_squares, least_squares_batch
    B = 4
    fun, jac, fun_b, jac_b, truth, t = _expfit(B)
    X0 = np.tile([0.0, 1.0, -0.5], (B, 1))
    bounds = ([-1.0, 0.0, -3.0], [3.0, 3.0, 0.0])
    for b in range(2):
        _same(least_squares(fun_b(b), X0[b], jac_b(b), bounds=bounds, method=method),
              least_squares(fun_b(b), X0[b], jac_b(b), bounds=bounds, method=method, loss='linear', f_scale=3.0))
    for driver in ('host', 'device'):
        ctx.timing(True)
        ctx.timing_reset()
        a = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, driver=driver, ctx=ctx)
        b_ = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, driver=driver, ctx=ctx, loss='linear',
                                 f_scale=[1.0, 2.0, 3.0, 4.0])
        ctx.sync()
        T = ctx.timing_read()
        ctx.timing(False)
        assert T["loss_cost"][1] == 0 and T["loss_scale"][1] == 0
        for r1, r2 in zip(a, b_):
            _same(r1, r2)
    # ... while a robust loss on the device driver does launch them
    ctx.timing(True)
    ctx.timing_reset()
    least_squares_batch(fun, X0, jac, bounds=bounds, method=method, driver='device', ctx=ctx, loss='soft_l1',
                        f_scale=0.1)
    ctx.sync()
    T = ctx.timing_read()
    ctx.timing(False)
    assert T["loss_cost"][1] > 0 and T["loss_scale"][1] > 0
    names = list(T)
    assert names[-2:] == ["loss_cost", "loss_scale"]


# ---- 3. the device driver's first step against the CPU oracle ------------------------------------------------------
@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("outliers", [False, True])
def test_first_step_of_the_device_driver_matches_the_oracle(ctx, method, bounded, loss, outliers):
    """One outer iteration through blsq_outer_* against the CPU oracle fed with the numpy-scaled J and f.  Without
    outliers every row keeps w well above sqrt(EPS): the parity tests' 1e-10 step bar.  With gross outliers, huber,
    cauchy and arctan clamp those rows to w = sqrt(EPS) and their scaled residuals grow to f rho1 / sqrt(EPS) ~ 1e7:
    the augmented system [J f] the step path factors then amplifies last-bit differences of the inputs (which scipy's
    own formula does not fix, see _check_w_and_fs) by ~1e6, and the bar is 1e-7 (soft_l1 never clamps: 1e-10)."""
    from oracle import blsq_oracle as orc
    from bounded_lsq import OuterDriver
    from bounded_lsq import _hostmath as H
    B, m, n = 3, 96, 5
    rng = np.random.default_rng(11)
    J = rng.standard_normal((B, m, n))
    f = rng.standard_normal((B, m)) * (2.0 if outliers else 0.3)
    if outliers:
        f[:, ::7] += 30.0                             # gross outliers
    x0 = rng.uniform(-0.5, 0.5, (B, n))
    if bounded:
        lb, ub = np.full((B, n), -1.0), np.full((B, n), 0.6)
    else:
        lb, ub = np.full((B, n), -np.inf), np.full((B, n), np.inf)
    fs = np.array([0.5, 1.0, 3.0]) if outliers else np.array([1.5, 2.0, 3.0])
    bar = 1e-7 if (outliers and loss != 'soft_l1') else 1e-10
    xs = np.stack([H.shift_into_interior(x0[b], lb[b], ub[b], rstep=1e-10) for b in range(B)]) \
        if method == 'trf' else x0.copy()
    drv = OuterDriver(method, B, m, n, ctx=ctx)
    try:
        drv.set_loss(loss, fs)
        drv.start(x0, xs, lb, ub, np.ones((B, n)), False, 1e-8, 1e-8, 1e-8, 100)
        drv._up(drv.d_f, f, (B, m))
        drv._up(drv.d_J, J, (B, m, n))
        drv.begin()
        Js = drv._down(drv.d_J, (B, m, n))
        assert drv.propose() == B
        Xt = drv._down(drv.d_x_trial, (B, n))
        R = drv.fetch()
    finally:
        drv.close()
    for b in range(B):
        rho = H.loss_rho(loss, f[b], fs[b])
        J_ref, f_ref = H.loss_scale(J[b], f[b], rho)
        _check_scaled_J(Js[b], J[b], f[b], rho)
        np.testing.assert_array_equal(R["f"][b], f[b])                    # the true residuals are kept
        np.testing.assert_allclose(R["obj"][b], H.loss_cost(loss, f[b], fs[b]), rtol=1e-13)
        if method == 'trf':
            g = J_ref.T @ f_ref
            Delta = np.linalg.norm(x0[b] / H.cl_vector(xs[b], g, lb[b], ub[b]) ** 0.5)
            _, So = orc.trf_step_solve(J_ref, f_ref, xs[b], lb[b], ub[b], np.ones(n), Delta, 0.0)
        else:
            Delta = np.linalg.norm(x0[b], ord=np.inf)
            ob = np.zeros(n, dtype=np.int64)
            _, So = orc.dogbox_step_solve(J_ref, f_ref, xs[b], lb[b], ub[b], np.ones(n), ob, Delta)
        step = Xt[b] - xs[b]
        err = np.linalg.norm(step - So.step) / np.linalg.norm(So.step)
        assert err < bar, (b, err)


# ---- 4. end to end against scipy -----------------------------------------------------------------------------------
TIGHT = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)


def _scipy_fit(fun, jac, x0, bounds, method, loss, f_scale):
    from scipy.optimize import least_squares as sls
    return sls(fun, x0, jac, bounds=bounds, method=method, loss=loss, f_scale=f_scale, max_nfev=2000, **TIGHT)


def _check_against_scipy(r, ref):
    np.testing.assert_allclose(r.x, ref.x, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(r.obj_value, 2 * ref.cost, rtol=1e-9)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("loss", ROBUST)
def test_nonlinear_robust_fits_match_scipy_through_all_three_drivers(method, loss):
    from bounded_lsq import least_squares, least_squares_batch
    B = 4
    fun, jac, fun_b, jac_b, truth, t = _expfit(B, m=80, seed=20)
    X0 = np.tile([0.0, 1.0, -0.5], (B, 1))
    bounds = ([-1.0, 0.0, -3.0], [3.0, 3.0, 0.0])
    fs = 0.1
    host = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, loss=loss, f_scale=fs, max_nfev=2000,
                               **TIGHT)
    dev = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, loss=loss, f_scale=fs, max_nfev=2000,
                              driver='device', **TIGHT)
    lin = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, max_nfev=2000, **TIGHT)
    # device vs host driver, per problem, at the default tolerances as the existing driver tests compare them (at
    # 1e-12 the last accept decisions rest on objective differences of a few ulps, which the two sums round apart)
    host_d = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, loss=loss, f_scale=fs)
    dev_d = least_squares_batch(fun, X0, jac, bounds=bounds, method=method, loss=loss, f_scale=fs, driver='device')
    for h, d in zip(host_d, dev_d):
        assert (d.nfev, d.njev, d.status) == (h.nfev, h.njev, h.status)
        np.testing.assert_allclose(d.x, h.x, rtol=1e-7, atol=1e-10)        # the xtol level
    for b in range(B):
        ref = _scipy_fit(fun_b(b), jac_b(b), X0[b], bounds, method, loss, fs)
        one = least_squares(fun_b(b), X0[b], jac_b(b), bounds=bounds, method=method, loss=loss, f_scale=fs,
                            max_nfev=2000, **TIGHT)
        for r in (one, host[b], dev[b]):
            _check_against_scipy(r, ref)
            np.testing.assert_array_equal(r.fun, fun_b(b)(r.x))            # true residuals
        np.testing.assert_allclose(one.jac, ref.jac, rtol=1e-5, atol=1e-8)  # the scaled Jacobian, as scipy
        np.testing.assert_allclose(dev[b].x, host[b].x, rtol=1e-6, atol=1e-9)
        assert np.linalg.norm(host[b].x - truth[b]) < np.linalg.norm(lin[b].x - truth[b]), b


def _linear_batch(B, m, n, seed):
    """y = A p + noise with 15 % gross outliers; J = A (linear in the parameters)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m, n))
    P = rng.uniform(-1.0, 1.0, (B, n))
    Y = np.einsum('bmn,bn->bm', A, P) + 0.1 * rng.standard_normal((B, m))
    for b in range(B):
        k = rng.choice(m, int(0.15 * m), replace=False)
        Y[b, k] += rng.choice([-1, 1], k.size) * rng.uniform(10.0, 30.0, k.size)

    def fun(X):
        X = np.atleast_2d(X)
        return np.einsum('bmn,bn->bm', A[:X.shape[0]], X) - Y[:X.shape[0]]

    def jac(X):
        return A[:np.atleast_2d(X).shape[0]].copy()
    return fun, jac, A, Y, P


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("loss", ROBUST)
def test_linear_in_parameters_batches_of_512x64_device_equals_host(method, loss):
    """512 x 64 problems, 15 % gross outliers, eight bounds of problem 1 below the truth: the device driver returns,
    problem by problem, what the host driver returns, and the objective is the loss cost of the true residuals.
    (scipy itself is not a reliable yardstick at this size: its scaled residuals in clamped rows reach ~1e7 and its
    iterations end on xtol at points that move with the last bits of the inputs; the nonlinear test above compares
    with scipy.)"""
    from bounded_lsq import least_squares_batch
    from bounded_lsq import _hostmath as H
    B, m, n = 3, 512, 64
    fun, jac, A, Y, P = _linear_batch(B, m, n, seed=31)
    lb = np.full((B, n), -np.inf)
    ub = np.full((B, n), np.inf)
    ub[1, :8] = P[1, :8] - 0.2
    lb[1, :8] = -3.0
    X0 = np.stack([np.linalg.lstsq(A[b], Y[b], rcond=None)[0] for b in range(B)])   # robust refinement of the LS fit
    X0 = np.clip(X0, lb + 1e-3, ub - 1e-3)
    fs = np.array([1.0, 1.0, 2.0])
    host = least_squares_batch(fun, X0, jac, bounds=(lb, ub), method=method, loss=loss, f_scale=fs)
    dev = least_squares_batch(fun, X0, jac, bounds=(lb, ub), method=method, loss=loss, f_scale=fs, driver='device')
    F = fun(np.stack([d.x for d in dev]))
    for b, (h, d) in enumerate(zip(host, dev)):
        assert (d.nfev, d.njev, d.status) == (h.nfev, h.njev, h.status), b
        np.testing.assert_allclose(d.x, h.x, rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(d.obj_value, h.obj_value, rtol=1e-9)
        np.testing.assert_allclose(d.fun, F[b], rtol=1e-12, atol=1e-12)      # the true residuals
        np.testing.assert_allclose(d.obj_value, H.loss_cost(loss, d.fun, fs[b]), rtol=1e-13)
        assert d.nfev > 1


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_fd_jacobians_difference_the_true_residuals(method):
    from bounded_lsq import least_squares_batch
    B = 3
    fun, jac, fun_b, jac_b, truth, t = _expfit(B, m=50, seed=40)
    X0 = np.tile([0.0, 1.0, -0.5], (B, 1))
    ex = least_squares_batch(fun, X0, jac, method=method, loss='cauchy', f_scale=0.1)
    for driver in ('host', 'device'):
        fd = least_squares_batch(fun, X0, '2-point', method=method, loss='cauchy', f_scale=0.1, driver=driver)
        for r1, r2 in zip(ex, fd):
            np.testing.assert_allclose(r2.x, r1.x, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(r2.obj_value, r1.obj_value, rtol=1e-8)


# ---- 5. no double scaling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_device_driver_scales_each_fresh_jacobian_once(ctx, method):
    from bounded_lsq import OuterDriver, least_squares_batch
    from bounded_lsq import _hostmath as H
    B = 6
    fun, jac, fun_b, jac_b, truth, t = _expfit(B, m=70, seed=50)
    m, n = 70, 3
    X0 = np.tile([0.0, 1.0, -0.5], (B, 1))
    X0[:, 1] += 0.7 * np.arange(B)                    # different paths: some trials rejected while others accept
    lb, ub = np.full((B, n), -np.inf), np.full((B, n), np.inf)
    fs = np.linspace(0.05, 0.5, B)
    loss = 'soft_l1'
    drv = OuterDriver(method, B, m, n, ctx=ctx)
    rejected = accepted = checks = 0
    try:
        drv.set_loss(loss, fs)
        drv.start(X0, X0, lb, ub, np.ones((B, n)), False, 1e-10, 1e-10, 1e-10, 200)
        X = drv._down(drv.d_x, (B, n))
        drv._up(drv.d_f, fun(X), (B, m))
        drv._up(drv.d_J, jac(X), (B, m, n))
        drv.begin()
        itemJ = m * n * 8
        import ctypes as C
        while drv.propose() > 0:
            # the step just computed was factored from the driver's J: it must be w(f(x)) J_true(x), every problem
            X = drv._down(drv.d_x, (B, n))
            Jd = drv._down(drv.d_J, (B, m, n))
            F, Jt = fun(X), jac(X)
            for b in range(B):
                _check_scaled_J(Jd[b], Jt[b], F[b], H.loss_rho(loss, F[b], fs[b]))
            checks += 1
            Xt = drv._down(drv.d_x_trial, (B, n))
            drv._up(drv.d_f_trial, fun(Xt), (B, m))
            na = drv.judge()
            acc = drv._down(drv.d_accepted, (B,), np.int32)
            st = drv.fetch()
            live = st["status"] == 0
            accepted += int(acc.sum())
            rejected += int(((acc == 0) & live).sum())
            if na > 0:
                X = drv._down(drv.d_x, (B, n))
                Jn = np.ascontiguousarray(jac(X))
                for b in np.nonzero(acc)[0]:                       # the fresh Jacobians only
                    dst = C.c_void_p(drv.d_J.value + int(b) * itemJ)
                    ctx.check(ctx.lib.blsq_memcpy_h2d(ctx.h, dst, Jn[b].ctypes.data_as(C.c_void_p), itemJ), "h2d")
        R = drv.fetch()
    finally:
        drv.close()
    assert checks > 3 and accepted > 0 and rejected > 0
    # ... and the results are those of the host driver, which rescales a freshly evaluated J every tick
    host = least_squares_batch(fun, X0, jac, method=method, loss=loss, f_scale=fs, ftol=1e-10, xtol=1e-10,
                               gtol=1e-10, max_nfev=200)
    for b in range(B):
        assert (R["nfev"][b], R["njev"][b], R["status"][b]) == (host[b].nfev, host[b].njev, host[b].status), b
        np.testing.assert_allclose(R["x"][b], host[b].x, rtol=1e-9, atol=1e-12)


def test_set_loss_after_start_is_an_argument_error(ctx):
    from bounded_lsq import OuterDriver
    from bounded_lsq._abi import BlsqError
    B, m, n = 2, 8, 2
    drv = OuterDriver('trf', B, m, n, ctx=ctx)
    try:
        with pytest.raises(BlsqError):
            drv.set_loss('huber', [1.0, -1.0])                     # f_scale must be positive
        drv.start(np.zeros((B, n)), np.zeros((B, n)), -np.ones((B, n)), np.ones((B, n)), np.ones((B, n)), False,
                  1e-8, 1e-8, 1e-8, 10)
        with pytest.raises(BlsqError):
            drv.set_loss('huber', 1.0)
    finally:
        drv.close()
