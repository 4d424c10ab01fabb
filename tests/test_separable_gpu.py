"""Separable fits on the GPU: blsq_varpro_expand_dev and blsq_varpro_reduce_dev in isolation against the
np.longdouble definition (``models.varpro_reduce``) on the cases tests/test_separable_cpu.py vets, the structural
promises of the entries, and whole fits with ``separable=True`` against the plain fit.

Cap of the kernel tests (tests/_separable_cases.py): each metric <= 32 kappa_2(Phi_w) eps.  The kernel keeps a problem
of m <= 64 rows (one block) in LDS and streams the blocks of a longer one from global memory in every pass: m = 64 is the
last resident size and m = 65 the first streamed one, and the grid has both, next to 63, 130 and 257 (three and five
blocks), the tiles of the work layout (na + 1 = 2, 12, 49, 62) and nl = 16.  Fits: the
package's margins between two routes, rtol 1e-6 / atol 1e-9 for popt and 1e-6 for the normalised pcov.  The worst
fraction of the cap seen on an MI355X is in DESIGN.md 7v."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

import _model_eval as me
import _separable_cases as sc
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload
ISENT = -77
worst = {}


def reduce_dev(ctx, cs, wform="none", want=("f", "J", "c", "info"), mask=None, G=None, y=None, w=None, **over):
    """blsq_varpro_reduce_dev on a case -> (rc, dict of the outputs asked for), every output pre-filled with a sentinel.
    `G`, `y`, `w`: in place of the case's (their leading axis is B); `over`: arguments replaced by name (B, m, n, nl,
    lin, owner, w_stride, G_ptr, y_ptr)."""
    G = cs.G if G is None else G
    y = cs.y if y is None else y
    B = G.shape[0]
    w = cs.ws[wform] if w is None else w
    a = dict(B=B, m=cs.m, n=cs.n, nl=cs.nl, lin=cs.lin, owner=cs.owner, w_stride=me.w_stride(w, cs.m))
    a.update(over)
    lin, p_lin = me.i32(a["lin"])
    owner, p_owner = me.i32(a["owner"])
    shapes = dict(f=(B, cs.m), J=(B, cs.m, cs.na), c=(B, cs.nl), info=(B,))
    with me.Dev(ctx) as d:
        out = {k: d.up(np.full(shapes[k], ISENT, dtype=np.int32) if k == "info" else np.full(shapes[k], SENTINEL))
               for k in want}
        rc = ctx.lib.blsq_varpro_reduce_dev(
            ctx.h, a["B"], a["m"], a["n"], a["nl"], p_lin, p_owner, over.get("G_ptr", d.up(G)), over.get("y_ptr", d.up(y)),
            d.up(w), a["w_stride"], out.get("f"), out.get("J"), out.get("c"), out.get("info"),
            d.up(None if mask is None else np.asarray(mask, dtype=np.int32)))
        ctx.sync()
        return rc, {k: ctx.to_host(p, shapes[k], np.int32 if k == "info" else np.float64) for k, p in out.items()}


def check(cs, wform, ref, out, problems=None):
    frac = sc.fractions(cs, wform, ref, out.get("f"), out.get("J"), out.get("c"), problems)
    for k, v in frac.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print((cs.m, cs.nl, cs.na), wform, "kappa %.3g" % cs.kappa(wform).max(), frac, "worst so far", worst)
    assert max(frac.values()) <= 1.0, frac


# ---- the kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wform", sc.WFORMS)
@pytest.mark.parametrize("shape", sc.GRID + (sc.ILL + (True,),), ids=str)
def test_reduce_against_longdouble(ctx, shape, wform):
    cs, ref = sc.case(*shape), sc.reference(*shape[:3], wform, *shape[3:])
    rc, out = reduce_dev(ctx, cs, wform)
    assert rc == 0
    assert out["info"].tolist() == [0] * sc.B
    check(cs, wform, ref, out)


@pytest.mark.parametrize("want", [("f",), ("J",), ("c",), ("f", "c"), ("J", "info"), ("f", "J")], ids=str)
def test_reduce_outputs_are_independent(ctx, want):
    cs = sc.case(65, 16, 48)
    rc, full = reduce_dev(ctx, cs, "per_problem")
    rc2, part = reduce_dev(ctx, cs, "per_problem", want=want)
    assert rc == 0 and rc2 == 0 and set(part) == set(want)
    for k in want:
        assert same_bits(part[k], full[k]), k


def test_reduce_masked_problems_are_left_untouched(ctx):
    cs = sc.case(130, 3, 61)
    rc, full = reduce_dev(ctx, cs, "shared")
    G = cs.G.copy()
    G[1] = np.nan                                 # nothing of a masked problem is read either
    rc2, out = reduce_dev(ctx, cs, "shared", mask=[1, 0, 1], G=G)
    assert rc == 0 and rc2 == 0
    for k in ("f", "J", "c"):
        assert same_bits(out[k][1], np.full(out[k][1].shape, SENTINEL)), k
        assert same_bits(out[k][[0, 2]], full[k][[0, 2]]), k
    assert out["info"].tolist() == [0, ISENT, 0]


@pytest.mark.parametrize("shape", [(63, 5, 11), (130, 3, 61), (257, 16, 1)], ids=str)
def test_a_problem_alone_gives_the_bits_it_gives_in_the_batch(ctx, shape):
    cs = sc.case(*shape)
    rc, full = reduce_dev(ctx, cs, "per_problem")
    assert rc == 0
    for b in (0, 2):
        rc, one = reduce_dev(ctx, cs, G=cs.G[b:b + 1], y=cs.y[b:b + 1], w=cs.ws["per_problem"][b:b + 1])
        assert rc == 0
        for k in ("f", "J", "c"):
            assert same_bits(one[k][0], full[k][b]), (k, b)


def test_reduce_rank_deficient(ctx):
    cs = sc.case(63, 5, 11)
    rc, good = reduce_dev(ctx, cs)
    G = cs.G.copy()
    G[1, :, cs.lin[3]] = G[1, :, cs.lin[0]]      # two identical columns
    rc2, out = reduce_dev(ctx, cs, G=G)
    assert rc == 0 and rc2 == 0
    assert out["info"].tolist() == [0, 1, 0]
    for k in ("f", "J", "c"):
        assert np.isnan(out[k][1]).all(), k
        assert same_bits(out[k][[0, 2]], good[k][[0, 2]]), k
    G[2, :, cs.lin[2]] = 0.0                      # and a column of zeros
    rc3, out = reduce_dev(ctx, cs, G=G, want=("c", "info"))
    assert rc3 == 0 and out["info"].tolist() == [0, 1, 1] and np.isnan(out["c"][1:]).all()
    assert models.varpro_reduce(G, cs.y, None, cs.lin, cs.owner)[3].tolist() == [0, 1, 1]


def test_reduce_bad_arguments_launch_nothing(ctx):
    cs = sc.case(63, 5, 11)
    lin, owner = cs.lin, cs.owner
    bad_owner = owner.copy()
    bad_owner[cs.non[0]] = cs.nl
    lin_owner = owner.copy()
    lin_owner[lin[0]] = 0
    cases = [
        (dict(B=0), 2), (dict(m=0), 3), (dict(m=cs.nl), 3), (dict(n=65), 4), (dict(n=1), 4), (dict(nl=0), 5),
        (dict(nl=17), 5), (dict(nl=cs.n), 5), (dict(lin=lin[::-1]), 6), (dict(lin=np.r_[lin[:-1], cs.n]), 6),
        (dict(lin=np.r_[-1, lin[1:]]), 6), (dict(lin=np.r_[lin[:1], lin[:1], lin[2:]]), 6), (dict(owner=bad_owner), 7),
        (dict(owner=lin_owner), 7), (dict(owner=np.where(owner < 0, 0, owner)), 7), (dict(G_ptr=None), 8),
        (dict(y_ptr=None), 9), (dict(w_stride=7), 11), (dict(want=("info",)), 12),
    ]
    for over, index in cases:
        wform = "per_problem" if "w_stride" in over else "none"
        rc, out = reduce_dev(ctx, cs, wform, **over)
        assert rc == -index, (over, rc)
        for k, v in out.items():                  # nothing was launched: every output keeps its sentinel
            assert same_bits(v, np.full(v.shape, ISENT, dtype=np.int32) if k == "info" else np.full(v.shape, SENTINEL))
    assert ctx.lib.blsq_varpro_reduce_dev(None, *([0] * 4), *([None] * 5), 0, *([None] * 5)) == -1
    rc, out = reduce_dev(ctx, cs)                 # and the context is still good
    assert rc == 0 and not np.isnan(out["f"]).any()


@pytest.mark.parametrize("B, n, lin", [(1, 2, [0]), (3, 5, [0, 2, 4]), (7, 64, list(range(0, 64, 4))), (130, 11, [10])])
def test_expand_is_bit_exact(ctx, B, n, lin):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((B, n - len(lin)))
    X[0, 0] = SENTINEL                            # (a payload passes through)
    arr, p_lin = me.i32(lin)
    with me.Dev(ctx) as d:
        d_P = d.up(np.full((B, n), 5.0))
        assert ctx.lib.blsq_varpro_expand_dev(ctx.h, B, n, len(lin), p_lin, d.up(X), d_P) == 0
        P = ctx.to_host(d_P, (B, n), np.float64)
    assert same_bits(P, models.varpro_expand(X, lin, n))


def test_expand_bad_arguments(ctx):
    arr, p_lin = me.i32([0, 2])
    bad, p_bad = me.i32([2, 0])
    with me.Dev(ctx) as d:
        d_X, d_P = d.up(np.zeros((2, 2))), d.up(np.full((2, 4), SENTINEL))
        for args, index in (((0, 4, 2, p_lin, d_X, d_P), 2), ((2, 65, 2, p_lin, d_X, d_P), 3),
                            ((2, 4, 0, p_lin, d_X, d_P), 4), ((2, 4, 17, p_lin, d_X, d_P), 4),
                            ((2, 2, 2, p_lin, d_X, d_P), 4), ((2, 4, 2, None, d_X, d_P), 5),
                            ((2, 4, 2, p_bad, d_X, d_P), 5), ((2, 4, 2, p_lin, None, d_P), 6),
                            ((2, 4, 2, p_lin, d_X, None), 7)):
            assert ctx.lib.blsq_varpro_expand_dev(ctx.h, *args) == -index, (args[:3], index)
        ctx.sync()
        assert same_bits(ctx.to_host(d_P, (2, 4), np.float64), np.full((2, 4), SENTINEL))


def test_worst_fraction_of_the_cap(ctx):
    """Runs last among the kernel tests: the figure DESIGN.md 7v records.  Above one half it is reported, not widened."""
    print("worst fraction of the cap 32 kappa eps:", worst)
    assert worst and max(worst.values()) <= 1.0


# ---- the device stage ------------------------------------------------------------------------------------------------
def test_device_model_stage_matches_the_definition(ctx):
    spec = "gauss*2+lorentz+poly*2"
    M, n, x, P, Y = sc.fit_data(spec)
    lin, owner = models.linear_params(spec)
    non = np.flatnonzero(owner >= 0)
    sigma = np.linspace(0.5, 2.0, sc.FIT_M)
    X = np.ascontiguousarray(1.1 * P[:, non] + 0.02)
    B, m, na = sc.FIT_B, sc.FIT_M, non.size
    with models.DeviceModel(ctx, spec, B, m, n, x, Y, sigma, separable=True) as dm, me.Dev(ctx) as d:
        assert (dm.n, dm.n_model) == (na, n)
        d_X, d_f, d_J = d.up(X), d.up(np.zeros((B, m))), d.up(np.zeros((B, m, na)))
        dm.fun_dev(d_X, d_f, 1)
        dm.jac_dev(d_X, d_J, None)
        c = dm.linear_coefficients(d_X)
        f, J = ctx.to_host(d_f, (B, m), np.float64), ctx.to_host(d_J, (B, m, na), np.float64)
        with pytest.raises(ValueError, match="reps must be 1"):
            dm.fun_dev(d_X, d_f, 2)
    fr, Jr, cr, _ = models.varpro_reduce(M.jac(x, models.varpro_expand(X, lin, n)), Y, 1.0 / sigma, lin, owner)
    np.testing.assert_allclose(f, fr, rtol=0, atol=1e-12)
    np.testing.assert_allclose(J, Jr, rtol=0, atol=1e-10)
    np.testing.assert_allclose(c, cr, rtol=1e-11, atol=1e-12)
    with pytest.raises(ValueError, match="not opened with `separable=True`"):
        with models.DeviceModel(ctx, spec, B, m, n, x, Y) as plain:
            plain.linear_coefficients(None)


# ---- whole fits ------------------------------------------------------------------------------------------------------
def fit(spec, binned=False, **kw):
    M, n, x, P, Y = sc.fit_data(spec, binned)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(spec, x, Y, **sc.TOLS, **({"binned": True} if binned else {}), **kw)


@pytest.fixture(scope="module")
def plain():
    """The plain fit started at the truth, per (spec, method, extras): computed once, shared, left unchanged."""
    cache = {}

    def get(spec, method="trf", binned=False, **kw):
        key = (spec, method, binned, tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in cache:
            cache[key] = fit(spec, binned, p0=sc.fit_data(spec, binned)[3], method=method, driver="device", **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("spec", ["exp*2+poly*1", "gauss*2+lorentz+poly*2", "gauss2d"])
def test_separable_fit_agrees_with_the_plain_fit(plain, spec, method):
    M, n, x, P, Y = sc.fit_data(spec)
    ref = plain(spec, method)
    out = fit(spec, p0=sc.start(spec, P), method=method, driver="device", separable=True)
    assert all(r.success for r in ref[2]) and all(r.success for r in out[2])
    me.agree(ref, out, (spec, method))
    lin, owner = models.linear_params(spec, n)
    non = np.flatnonzero(owner >= 0)
    for b, (r, q) in enumerate(zip(out[2], ref[2])):
        assert r.x.shape == (n,) and np.array_equal(r.x, out[0][b])
        assert r.x_nonlinear.shape == (non.size,) and np.array_equal(r.x_nonlinear, r.x[non])
        assert r.linear_params.tolist() == lin.tolist()
        assert r.active_mask.shape == (n,) and not r.active_mask.any()
        assert r.fun.shape == (sc.FIT_M,) and r.jac.shape == (sc.FIT_M, non.size)
        np.testing.assert_allclose(r.fun, q.fun, rtol=0, atol=1e-8)
        assert r.x_covariance.shape == (n, n) and np.array_equal(r.x_covariance, out[1][b])
        assert r.status > 0 and r.nfev >= 1 and r.optimality >= 0


def test_separable_fit_with_an_active_bound(plain):
    spec = "exp*2+poly*1"
    M, n, x, P, Y = sc.fit_data(spec)
    lb = np.full(n, -np.inf)
    ub = np.full(n, np.inf)
    lb[[1, 3]], ub[3] = 0.0, 2.5                 # the second rate (3.1) is held at 2.5
    p_plain = P.copy()
    p_plain[:, 3] = 2.4
    p0 = sc.start(spec, P)
    p0[:, 3] = 2.4
    for method in ("trf", "dogbox"):
        ref = fit(spec, p0=p_plain, bounds=(lb, ub), method=method, driver="device")
        out = fit(spec, p0=p0, bounds=(lb, ub), method=method, driver="device", separable=True)
        assert all(r.success for r in ref[2]) and all(r.success for r in out[2])
        np.testing.assert_allclose(out[0], ref[0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(out[0][:, 3], 2.5, rtol=1e-9, atol=0)      # (trf stays strictly inside its box)
        if method == "dogbox":
            assert np.all(out[0][:, 3] == 2.5)
        for r, q in zip(out[2], ref[2]):
            assert r.active_mask.tolist() == np.asarray(q.active_mask).tolist() and r.active_mask[3] == 1


def test_separable_fit_with_sigma_per_problem(plain):
    spec = "exp*2+poly*1"
    M, n, x, P, Y = sc.fit_data(spec)
    sigma = np.random.default_rng(2).uniform(0.5, 2.0, Y.shape)
    for absolute in (False, True):
        ref = plain(spec, sigma=sigma, absolute_sigma=absolute)
        out = fit(spec, p0=sc.start(spec, P), driver="device", separable=True, sigma=sigma, absolute_sigma=absolute)
        me.agree(ref, out, ("sigma", absolute))
        np.testing.assert_allclose(np.einsum("bii->bi", out[1]), np.einsum("bii->bi", ref[1]), rtol=1e-5, atol=0)
    for sg in (0.5, sigma[0]):                    # a scalar and one (m,) set shared by all problems
        me.agree(plain(spec, sigma=sg), fit(spec, p0=sc.start(spec, P), driver="device", separable=True, sigma=sg), "sg")


def test_separable_fit_binned(plain):
    spec = "gauss+poly*1"
    M, n, x, P, Y = sc.fit_data(spec, True)
    ref = plain(spec, binned=True)
    out = fit(spec, True, p0=sc.start(spec, P), driver="device", separable=True)
    assert all(r.success for r in out[2])
    me.agree(ref, out, "binned")


def test_separable_fit_host_driver_agrees_with_device(plain):
    spec = "exp*2+poly*1"
    M, n, x, P, Y = sc.fit_data(spec)
    dev = fit(spec, p0=sc.start(spec, P), driver="device", separable=True)
    host = fit(spec, p0=sc.start(spec, P), driver="host", separable=True)
    assert all(r.success for r in host[2])
    me.agree(dev, host, "host")
    me.agree(plain(spec), host, "host against plain")
    for r in host[2]:
        assert r.x_nonlinear.shape == (2,) and r.linear_params.tolist() == [0, 2, 4]


def test_a_rank_deficient_problem_leaves_its_batch_mates_alone():
    spec = "gauss*2+poly*1"
    x = np.linspace(-2.0, 2.0, 90)
    truth = np.array([2.0, -0.6, 0.3, 1.5, 0.7, 0.35, 0.2])
    rng = np.random.default_rng(9)
    P = truth * (1.0 + 0.01 * rng.standard_normal((4, 7)))
    Y = models.resolve(spec).f(x, P) + 0.01 * rng.standard_normal((4, 90))
    p0 = 1.1 * P
    kw = dict(driver="device", separable=True, max_nfev=30, **sc.TOLS)
    good = bounded_lsq.curve_fit_batch(spec, x, Y, p0, **kw)
    assert all(r.success for r in good[2])
    p0[2, [4, 5]] = p0[2, [1, 2]]                 # problem 2 starts with its two peaks on top of each other: Phi has
    with warnings.catch_warnings():               # two identical columns there and the residuals are NaN from the start
        warnings.simplefilter("ignore")
        popt, pcov, res = bounded_lsq.curve_fit_batch(spec, x, Y, p0, **kw)
    assert not res[2].success and np.isnan(popt[2]).all() and np.isnan(pcov[2]).all()
    mates = [0, 1, 3]
    assert same_bits(popt[mates], good[0][mates]) and same_bits(pcov[mates], good[1][mates])
    assert [res[b].nfev for b in mates] == [good[2][b].nfev for b in mates]


def test_without_the_keyword_nothing_changes():
    spec = "gauss*2+lorentz+poly*2"
    M, n, x, P, Y = sc.fit_data(spec)
    for driver in ("device", "host"):
        a = fit(spec, p0=P, driver=driver)
        b = fit(spec, p0=P, driver=driver, separable=False)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
        for r, q in zip(a[2], b[2]):
            assert same_bits(r.fun, q.fun) and r.nfev == q.nfev and not hasattr(r, "x_nonlinear")
