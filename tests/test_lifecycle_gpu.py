"""Create / use / destroy, three times over on ONE context, for every kind of plan — the destroy paths with every lazily
allocated buffer group in existence, which no other test reaches.  A plan frees its device memory in its destructor
(csrc/dev_buf.h); what is checked here is that a destroy leaves the context sound: cycle 3 returns the bits of cycle 1.
(No device-memory query: free memory of a shared device moves under other work.  That nothing leaks is the type's
business, checked on the host by tests/test_dev_buf_cpu.py.)"""
import ctypes as C

import numpy as np
import pytest

from bounded_lsq import TrfStepSolver, DogboxStepSolver, _abi, _synth
from bounded_lsq._abi import ptr, vp
from bounded_lsq._outer import OuterDriver

from _model_eval import same_bits

pytestmark = pytest.mark.gpu
CYCLES = 3


@pytest.fixture(scope="module")
def ctx():
    c = _abi.Context(0)
    yield c
    c.close()


def cycles(one):
    """one() -> tuple of arrays; CYCLES times; cycle 1 and cycle 3 bit for bit"""
    outs = [one() for _ in range(CYCLES)]
    assert len(outs[0]) == len(outs[-1])
    for k, (a, b) in enumerate(zip(outs[0], outs[-1])):
        assert same_bits(a, b), ("output %d differs between cycle 1 and cycle %d" % (k, CYCLES))
    return outs[0]


def trf_cycle(ctx, P, Delta):
    B, m, n = P["J"].shape
    sol = TrfStepSolver(B, m, n, ctx=ctx)
    try:
        F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])     # (host pointers: the lazy J / f staging)
        S = sol.step(Delta, np.zeros(B))
    finally:
        sol.close()
    assert sol.h is None
    return (F.g, F.g_norm, F.theta, S.step, S.x_new, S.hits, S.n_iter, S.branch, S.status)


def test_trf_plan(ctx):
    P = _synth.trf_batch(7, 4, 96, 24)
    out = cycles(lambda: trf_cycle(ctx, P, np.array([10.0, 0.5, 10.0, 0.1])))
    assert np.all(np.isfinite(out[3])) and np.all(out[8] == 0)


def test_dogbox_plan(ctx):
    B, m, n = 4, 96, 24
    P = _synth.dogbox_batch(7, B, m, n)

    def one():
        sol = DogboxStepSolver(B, m, n, ctx=ctx)
        try:
            F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
            S = sol.step(np.full(B, 0.02))
        finally:
            sol.close()
        assert sol.h is None
        return (F.g, F.active_set, F.g_norm, S.step, S.x_new, S.on_bound_new, S.status)
    out = cycles(one)
    assert np.all(np.isfinite(out[3])) and np.all(out[6] == 0)


def test_csne_tier_plan(ctx):
    """two ill-conditioned unbounded problems (kappa(J) = 2e3) on the CSNE tier: its recordings and partial sums are
    allocated by the first factor / step call and must go with the plan"""
    B, m, n = 2, 1024, 96
    P = _synth.trf_batch(11, B, m, n, unbounded=True)
    rng = np.random.default_rng(3)
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    for b in range(B):
        P["J"][b] = (P["J"][b] @ (V * np.logspace(0.0, -3.3, n))) @ V.T

    def one():
        ctx.gram_stats(reset=True); ctx.csne_stats(reset=True)
        out = trf_cycle(ctx, P, np.array([10.0, 0.5]))
        assert ctx.gram_stats() == (0, B) and ctx.csne_stats() == (B, B, 0), (ctx.gram_stats(), ctx.csne_stats())
        return out
    out = cycles(one)
    assert np.all(np.isfinite(out[3]))


def cov_cycle(ctx, J, act, scale):
    """one covariance plan: blsq_cov with a mask, then blsq_cov_pinv with a mask and a scale — at destroy the gather, the
    staging, both output groups and the Jacobi group all exist"""
    B, m, n = J.shape
    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "blsq_cov_plan_create")
    try:
        cov, rcond, status = np.empty((B, n, n)), np.empty(B), np.empty(B, np.int32)
        ctx.check(ctx.lib.blsq_cov(h, ptr(J), ptr(act), ptr(cov), ptr(rcond), ptr(status)), "blsq_cov")
        pcov, prcond, pstatus = np.empty((B, n, n)), np.empty(B), np.empty(B, np.int32)
        rank, kept = np.empty(B, np.int32), np.empty(B)
        ctx.check(ctx.lib.blsq_cov_pinv(h, ptr(J), ptr(act), ptr(scale), ptr(pcov), ptr(rank), ptr(prcond), ptr(kept),
                                        ptr(pstatus)), "blsq_cov_pinv")
    finally:
        assert ctx.lib.blsq_cov_plan_destroy(h) == 0
    return (cov, rcond, status, pcov, rank, prcond, kept, pstatus)


def test_cov_plan(ctx):
    B, m, n = 3, 40, 6
    rng = np.random.default_rng(5)
    J = np.ascontiguousarray(rng.standard_normal((B, m, n)))
    act = np.zeros((B, n), np.int64)
    act[0, 1] = 1; act[2, 0] = 1; act[2, 5] = 1
    scale = np.array([1.0, 0.5, 2.0])
    out = cycles(lambda: cov_cycle(ctx, J, act, scale))
    assert np.all(out[2] == 0) and np.all(out[7] == 0)
    assert list(out[4]) == [n - 1, n, n - 2]                 # rank = free variables of a well-conditioned J
    for b in range(B):
        free = act[b] == 0
        Jf = J[b][:, free]
        ref = np.linalg.inv(Jf.T @ Jf)
        assert np.allclose(out[0][b][np.ix_(free, free)], ref, rtol=1e-9, atol=0)
        assert np.allclose(out[3][b][np.ix_(free, free)], scale[b] * ref, rtol=1e-9, atol=0)


def test_fold_plan(ctx):
    """the smallest shape past the tree's merge capacity (m > 1024 with n > 512): the fold's own four buffers"""
    from bounded_lsq import covariance
    B, m, n = 1, 1040, 513
    J = np.random.default_rng(9).standard_normal((B, m, n))
    out = cycles(lambda: covariance(J, ctx=ctx))
    assert out[2][0] == 0 and np.all(np.isfinite(out[0]))


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_outer_driver(ctx, method):
    """a driver that owns a step plan and — after covariance() — a covariance plan, its mask and its output groups"""
    B, m, n = 4, 48, 5
    rng = np.random.default_rng(13)
    A = rng.standard_normal((B, m, n))
    xt = rng.standard_normal((B, n))
    y = np.einsum("bmn,bn->bm", A, xt) + 0.01 * rng.standard_normal((B, m))
    lb = np.full((B, n), -np.inf); ub = np.full((B, n), np.inf)
    ub[:, 0] = xt[:, 0] - 0.5                                 # the fit ends on this bound
    x0 = np.zeros((B, n)); x0[:, 0] = ub[:, 0] - 1.0

    def fun(X):
        return np.einsum("bmn,bn->bm", A, X) - y

    def one():
        drv = OuterDriver(method, B, m, n, ctx=ctx)
        try:
            drv.start(x0, x0, lb, ub, np.ones((B, n)), False, 1e-10, 1e-10, 1e-10, 100)
            R = drv.run_host(fun, lambda X: A)
            cov, rank, rcond, kept, status = drv.covariance(free_only=True, pinv=True)
        finally:
            drv.close()
        assert drv.h is None
        return (R["x"], R["obj"], R["status"], R["nfev"], cov, rank, rcond, kept, status)
    out = cycles(one)
    assert np.all(out[2] > 0), out[2]                         # every problem converged
    assert np.all(out[8] == 0) and np.all(np.isfinite(out[4]))
    if method == "dogbox":                                    # (its mask is exact: x[0] sits on the bound)
        assert np.array_equal(out[0][:, 0], ub[:, 0]) and list(out[5]) == [n - 1] * B
        assert np.all(out[4][:, 0, :] == 0) and np.all(out[4][:, :, 0] == 0)


def test_context_closed_over_open_plans():
    """a context closed while a plan of each kind is open: the plans go first, every handle is dropped, and a fresh
    context works"""
    P = _synth.trf_batch(7, 4, 96, 24)
    Pd = _synth.dogbox_batch(7, 4, 96, 24)
    c = _abi.Context(0)
    trf = TrfStepSolver(4, 96, 24, ctx=c)
    dog = DogboxStepSolver(4, 96, 24, ctx=c)
    drv = OuterDriver("trf", 4, 48, 5, ctx=c)
    trf.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    dog.factor(Pd["J"], Pd["f"], Pd["x"], Pd["lb"], Pd["ub"], Pd["scale"], Pd["on_bound"])
    c.close()
    assert c.h is None and trf.h is None and dog.h is None and drv.h is None
    trf.close(); dog.close(); drv.close(); c.close()          # (idempotent)
    c2 = _abi.Context(0)
    try:
        ref = trf_cycle(c2, P, np.array([10.0, 0.5, 10.0, 0.1]))
        assert np.all(np.isfinite(ref[3])) and np.all(ref[8] == 0)
    finally:
        c2.close()
    assert c2.h is None
