"""Instrument response on the GPU: blsq_response_apply_dev in isolation against numpy.longdouble and, where
the definition promises it, bit for bit; then whole fits through the response across their routes.  The cases are those
tests/test_response_cpu.py vets with scipy alone.

Margins (tests/_response_cases.py has the derivation; they hold for any summation order):
    |f - f_ref| <= gamma_{L+3} |w| (sum |h||g| + |y|)        |J - J_ref| <= gamma_{L+2} |w| sum |h||G|
Poisson: the bound of the transform of DESIGN.md 7m (constants of tests/_poisson_cases.py) plus |c| gamma_{L+1} mu for the
error mu arrives with.  Fits: the package's margins between two routes, rtol 1e-6 / atol 1e-9 for popt, 1e-6 for the
normalised pcov, rtol 1e-4 / atol 1e-7 for finite differences.  The worst fraction of each margin seen on an MI355X is in
DESIGN.md 7s."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _abi, _models, _outer, models

import _model_eval as me
import _poisson_cases as pc
import _response_cases as rc
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

LD = np.longdouble
ENTRY = "blsq_response_apply_dev"
SENTINEL = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload
MS = (1, 63, 64, 65, 130)
LS = (1, 2, 17, 64, 65, 130)
NCS = (1, 4, 17, 64)
worst = {}                                                     # margin name -> worst fraction seen


def note(name, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    worst[name] = max(worst.get(name, 0.0), float(np.max(frac)))
    return float(np.max(frac))


def teardown_module(module):
    print("\nworst fractions of the margins:", {k: round(v, 4) for k, v in worst.items()})


def h_stride(h):
    return h.shape[-1] if h.ndim == 2 else 0


class Staged:
    """A test's arrays on the device, and output buffers that are refilled before every call: `call` runs the entry on
    device pointers and brings back what was asked for."""

    def __init__(self, ctx, Q, B, m, nc):
        self.ctx, self.dev, self.Q, self.B, self.m, self.nc = ctx, me.Dev(ctx), Q, B, m, nc
        self.f_fill, self.J_fill = np.full((Q, m), SENTINEL), np.full((B, m, nc), SENTINEL)
        self.df, self.dJ = self.dev.up(self.f_fill), self.dev.up(self.J_fill)

    def up(self, a):
        return self.dev.up(a)

    def call(self, h, origin, dh, dg, dG, dy=None, dw=None, w_stride=0, est=0, nan=0, want_f=True, want_J=True,
             mask=None, reps=None, B=None, nc=None):
        ctx, lib = self.ctx, self.ctx.lib
        B = self.B if B is None else B
        reps = self.Q // self.B if reps is None else reps
        nc = self.nc if nc is None else nc
        for p, a in ((self.df, self.f_fill), (self.dJ, self.J_fill)):
            ctx.check(lib.blsq_memcpy_h2d(ctx.h, p, _abi.ptr(a), a.nbytes), "refill")
        rc_ = lib.blsq_response_apply_dev(ctx.h, est, nan, B, reps, self.m, nc, h.shape[-1], origin, dh, h_stride(h),
                                          dg, dG, dy, dw, w_stride, self.df if want_f else None,
                                          self.dJ if want_J else None, mask)
        assert rc_ == 0, (rc_, ctx.lib.blsq_last_error(ctx.h))
        return (ctx.to_host(self.df, (B * reps, self.m), np.float64) if want_f else None,
                ctx.to_host(self.dJ, (B, self.m, nc), np.float64) if want_J else None)

    def close(self):
        self.dev.close()


def apply(ctx, g, G, h, origin, y=None, w=None, est=0, nan=0, want_f=True, want_J=True, mask=None, reps=1):
    """The entry on host arrays -> (f (Q, m) or None, J (B, m, nc) or None)."""
    Q, m = g.shape
    B, nc = G.shape[0], G.shape[2]
    st = Staged(ctx, Q, B, m, nc)
    try:
        return st.call(h, origin, st.up(h), st.up(g), st.up(G), st.up(y), st.up(w), me.w_stride(w, m), est, nan,
                       want_f, want_J, st.up(None if mask is None else np.asarray(mask, dtype=np.int32)), reps)
    finally:
        st.close()


def draws(m, nc, B=3, reps=3, seed=0):
    rng = np.random.default_rng([seed, m, nc])
    return dict(g=rng.standard_normal((B * reps, m)), G=rng.standard_normal((B, m, nc)), y=rng.standard_normal((B, m)),
                wm=rng.uniform(0.5, 2.0, m), wB=rng.uniform(0.5, 2.0, (B, m)))


# ---- kernel: the grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_kernel_against_extended_precision(ctx, m):
    """Every L, origin, nc, B, reps, shared and per-problem h, the three forms of w, with and without y.  One draw of
    B = 3 problems, reps = 3 points and nc = 64 columns per m; the smaller batches and widths are its leading problems
    and columns, so one reference serves them all, and a problem alone must give the bits it gives inside the batch."""
    d = draws(m, 64)
    g3 = d["g"].reshape(3, 3, m)
    for L in LS:
        rng = np.random.default_rng([m, L])
        hs = {"shared": rng.standard_normal(L), "per problem": rng.standard_normal((3, L))}
        for origin in sorted({0, L // 2, L - 1}):
            for hname, h in hs.items():
                mu, HG, mu_abs, HG_abs = rc.reference(d["g"], d["G"], h, origin, 3)
                mu, mu_abs = mu.reshape(3, 3, m), mu_abs.reshape(3, 3, m)
                kept = {}
                for B in (3, 1):
                    for nc in NCS[::-1]:                           # (the widest first: the others are compared with it)
                        for reps in (1, 3):
                            if reps == 3 and nc != NCS[-1]:
                                continue                           # (f does not know nc: once per batch size)
                            st = Staged(ctx, B * reps, B, m, nc)
                            try:
                                hb = h if h.ndim == 1 else h[:B]
                                dh = st.up(hb)
                                dg = st.up(g3[:B, :reps].reshape(B * reps, m))
                                dG, dy = st.up(d["G"][:B, :, :nc]), st.up(d["y"][:B])
                                dws = {None: (None, 0), "wm": (st.up(d["wm"]), 0), "wB": (st.up(d["wB"][:B]), m)}
                                for wname, (dw, ws) in dws.items():
                                    w = 1.0 if wname is None else (d["wm"] if wname == "wm" else d["wB"][:B])
                                    wl = np.asarray(w, dtype=LD)
                                    for with_y in (False, True):
                                        what = (m, L, origin, hname, B, nc, reps, wname, with_y)
                                        f, J = st.call(hb, origin, dh, dg, dG, dy if with_y else None, dw, ws,
                                                       want_J=reps == 1)
                                        yl = d["y"][:B].astype(LD) if with_y else np.zeros((B, m), dtype=LD)
                                        wq = wl[:, None, :] if np.ndim(wl) == 2 else wl
                                        f_ref = wq * (mu[:B, :reps] - yl[:, None, :])
                                        f_tol = rc.gamma(L + 3) * np.abs(wq) * (mu_abs[:B, :reps] + np.abs(yl[:, None, :]))
                                        err = np.abs(f.reshape(B, reps, m).astype(LD) - f_ref)
                                        assert np.all(err <= f_tol), (what, note("f", err, f_tol))
                                        note("f / gamma_{L+3}", err, f_tol)
                                        key = (reps, wname, with_y)
                                        if B == 3 and nc == NCS[-1]:
                                            kept[("f",) + key] = f
                                        else:                      # problem 0 alone, or beside a narrower G: the same bits
                                            assert same_bits(f, kept[("f",) + key][:B * reps]), what
                                        if reps != 1:
                                            continue
                                        wj = wl[:, :, None] if np.ndim(wl) == 2 else (wl[:, None] if np.ndim(wl) else wl)
                                        J_ref = wj * HG[:B, :, :nc]
                                        J_tol = rc.gamma(L + 2) * np.abs(wj) * HG_abs[:B, :, :nc]
                                        err = np.abs(J.astype(LD) - J_ref)
                                        assert np.all(err <= J_tol), (what, note("J", err, J_tol))
                                        note("J / gamma_{L+2}", err, J_tol)
                                        if B == 3 and nc == 64:
                                            kept[("J",) + key] = J
                                        elif B == 3:               # a narrower G: the bits of its columns in the wide one
                                            assert same_bits(J, kept[("J",) + key][:, :, :nc]), what
                                        else:
                                            assert same_bits(J, kept[("J",) + key][:1, :, :nc]), what
                            finally:
                                st.close()


def test_a_long_kernel_over_wide_rows_walks_tap_chunks_and_column_tiles(ctx):
    """L = 1024 with nc = 64: sixteen chunks of taps, two column tiles, three row blocks (m = 130), and L > m."""
    m, nc, L, B = 130, 64, 1024, 2
    d = draws(m, nc, B=B, reps=2, seed=5)
    h = np.random.default_rng(6).standard_normal((B, L))
    for origin in (0, 100, L - 1):
        mu, HG, mu_abs, HG_abs = rc.reference(d["g"], d["G"], h, origin, 2)
        f, _ = apply(ctx, d["g"], d["G"], h, origin, d["y"], d["wB"], want_J=False, reps=2)
        _, J = apply(ctx, d["g"][::2], d["G"], h, origin, d["y"], d["wB"], want_f=False)
        wq, yq = np.repeat(d["wB"], 2, axis=0).astype(LD), np.repeat(d["y"], 2, axis=0).astype(LD)
        err, tol = np.abs(f.astype(LD) - wq * (mu - yq)), rc.gamma(L + 3) * wq * (mu_abs + np.abs(yq))
        assert np.all(err <= tol), (origin, note("f", err, tol))
        note("f / gamma_{L+3}", err, tol)
        wj = d["wB"].astype(LD)[:, :, None]
        err, tol = np.abs(J.astype(LD) - wj * HG), rc.gamma(L + 2) * wj * HG_abs
        assert np.all(err <= tol), (origin, note("J", err, tol))
        note("J / gamma_{L+2}", err, tol)


# ---- kernel: bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,nc", [(1, 1), (65, 17), (130, 64)])
def test_the_unit_kernel_is_the_identity_in_every_bit(ctx, m, nc):
    d = draws(m, nc, seed=1)
    h = np.array([1.0])
    g = d["g"][::3]
    for w in (None, d["wm"], d["wB"]):
        for y in (None, d["y"]):
            f, J = apply(ctx, g, d["G"], h, 0, y, w)
            r = g - y if y is not None else g
            assert np.array_equal(f, r if w is None else w * r) and same_bits(f, r if w is None else w * r)
            want_J = d["G"] if w is None else (w[:, None] if w.ndim == 1 else w[:, :, None]) * d["G"]
            assert np.array_equal(J, want_J) and same_bits(J, want_J)


def test_shared_kernel_batch_mates_reps_and_joint_calls_do_not_change_a_bit(ctx):
    m, nc, L, origin = 65, 17, 17, 5
    d = draws(m, nc, seed=2)
    h = np.random.default_rng(2).standard_normal(L)
    g1 = d["g"][::3]
    f_sh, J_sh = apply(ctx, g1, d["G"], h, origin, d["y"], d["wB"])
    f_rep, J_rep = apply(ctx, g1, d["G"], np.ascontiguousarray(np.broadcast_to(h, (3, L))), origin, d["y"], d["wB"])
    assert same_bits(f_sh, f_rep) and same_bits(J_sh, J_rep)                # shared h == h replicated
    f_only, _ = apply(ctx, g1, d["G"], h, origin, d["y"], d["wB"], want_J=False)
    _, J_only = apply(ctx, g1, d["G"], h, origin, d["y"], d["wB"], want_f=False)
    assert same_bits(f_sh, f_only) and same_bits(J_sh, J_only)              # one call == two calls
    f_all, _ = apply(ctx, d["g"], d["G"], h, origin, d["y"], d["wB"], want_J=False, reps=3)
    for p in range(3):                                                      # alone == in the batch == among reps
        sl = slice(p, p + 1)
        f_one, J_one = apply(ctx, g1[sl], d["G"][sl], h, origin, d["y"][sl], d["wB"][sl])
        assert same_bits(f_one, f_sh[sl]) and same_bits(J_one, J_sh[sl])
        assert same_bits(f_all[3 * p], f_sh[p])
        for r in range(3):
            f_r, _ = apply(ctx, d["g"][3 * p + r:3 * p + r + 1], d["G"][sl], h, origin, d["y"][sl], d["wB"][sl],
                           want_J=False)
            assert same_bits(f_r[0], f_all[3 * p + r])


def test_masked_problems_keep_their_sentinel_and_are_not_read(ctx):
    m, nc = 65, 4
    d = draws(m, nc, seed=3)
    h = rc.irf(5, 2.0, 1.0)
    g1 = d["g"][::3]
    _, J_all = apply(ctx, g1, d["G"], h, 2, want_f=False)
    for est, y in ((0, None), (1, np.abs(d["y"]))):
        gp = np.abs(g1) + 1.0 if est else g1
        for mask in ([1, 0, 1], [0, 0, 0], [0, 1, 0]):
            f, J = apply(ctx, gp, d["G"], h, 2, y, est=est, mask=mask)
            ref = apply(ctx, gp, d["G"], h, 2, y, est=est)
            assert same_bits(f, ref[0])                                     # f takes no mask
            for p in range(3):
                assert same_bits(J[p], ref[1][p] if mask[p] else np.full((m, nc), SENTINEL)), (est, mask, p)
    assert same_bits(J_all, apply(ctx, g1, d["G"], h, 2, want_f=False, mask=[1, 1, 1])[1])


def test_non_finite_model_values_propagate_as_in_numpy(ctx):
    m, nc = 40, 3
    d = draws(m, nc, B=1, reps=1, seed=4)
    h = np.array([0.5, 0.0, -1.0, 2.0])                                     # a zero tap: 0 * inf is NaN
    g, G = d["g"].copy(), d["G"].copy()
    g[0, 5], g[0, 20], g[0, 21], g[0, 33] = np.inf, np.inf, np.inf, np.nan
    G[0, 7, 1], G[0, 30, 2], G[0, 39, 0] = -np.inf, np.nan, np.inf
    for origin in (0, 2, 3):
        with np.errstate(invalid="ignore"):
            mu = models.apply_response(g, h, origin)
            HG = np.moveaxis(models.apply_response(np.moveaxis(G, 1, -1), h, origin), -1, 1)
        f, J = apply(ctx, g, G, h, origin)
        for got, ref in ((f, mu), (J, HG)):
            assert np.isnan(ref).any() and np.isinf(ref).any()
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
            assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
            ok = np.isfinite(ref)
            np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("est", [0, 1])
def test_omit_gives_exact_zeros_and_leaves_the_other_rows_alone(ctx, est):
    m, nc, L, origin = 65, 17, 7, 3
    d = draws(m, nc, seed=7)
    h = np.random.default_rng(7).uniform(0.5, 1.5, L)
    g, G = np.abs(d["g"]) + 1.0, d["G"]
    y = np.abs(d["y"]) + 0.5
    w = None if est else d["wB"]
    full = apply(ctx, g, G, h, origin, y, w, est=est, want_J=False, reps=3)[0], apply(ctx, g[::3], G, h, origin, y, w,
                                                                                       est=est, want_f=False)[1]
    yn = y.copy()
    yn[0, [0, 1, 64]], yn[1, 10:30], yn[2, :] = np.nan, np.nan, np.nan
    gone = np.isnan(yn)
    f = apply(ctx, g, G, h, origin, yn, w, est=est, nan=1, want_J=False, reps=3)[0]
    J = apply(ctx, g[::3], G, h, origin, yn, w, est=est, nan=1, want_f=False)[1]
    gq = np.repeat(gone, 3, axis=0)
    assert same_bits(f[gq], np.zeros(gq.sum())) and same_bits(f[~gq], full[0][~gq])
    assert same_bits(J[gone], np.zeros((gone.sum(), nc))) and same_bits(J[~gone], full[1][~gone])
    f2, J2 = apply(ctx, g[::3], G, h, origin, yn, w, est=est, nan=1)        # f and J together
    assert same_bits(f2, f[::3]) and same_bits(J2, J)


@pytest.mark.parametrize("m,nc,L", [(1, 1, 1), (65, 17, 17), (130, 64, 65), (63, 4, 130)])
def test_poisson_epilogue_against_the_transform_in_extended_precision(ctx, m, nc, L):
    """Positive h and g, so that sum |h||g| = mu and the sum does not cancel; y in the mu >= y / 2 range of DESIGN.md 7m
    (0, mu itself, both branches of phi, the next integer above mu).  r and c (H G) against models.poisson_transform in
    longdouble at the longdouble mu: the transform's own bound, 2 eps T_r |r| and 2 eps (T_c + 1) |c HG| with the
    counts of tests/_poisson_cases.py, plus |c| gamma_{L+1} mu (and as much relative to mu for c) for the error mu
    arrives with, plus |c| gamma_{L+1} sum |h||G| for the sum of the column."""
    B, reps = 3, 3
    rng = np.random.default_rng([m, nc, L])
    g = rng.uniform(2.0, 4.0, (B * reps, m))
    G = rng.standard_normal((B, m, nc))
    for h, origin in ((rng.uniform(0.5, 1.5, L), L // 2), (rng.uniform(0.5, 1.5, (B, L)), 0)):
        mu, HG, _, HG_abs = rc.reference(g, G, h, origin, reps)
        mu1 = mu[::reps].astype(float)
        pattern = (np.arange(m)[None, :] + 3 * np.arange(B)[:, None]) % 7
        y = np.choose(pattern, [0 * mu1, mu1, mu1 / 1.2, mu1 / 0.8, mu1 / 1.3, mu1 / 0.7, np.floor(mu1) + 1])
        assert np.all(mu1 >= y / 2)
        yq = np.repeat(y, reps, axis=0).astype(LD)
        r_ref, c_ref = models.poisson_transform(mu, yq)
        pos = yq > 0
        u = np.where(pos, (mu - yq) / np.where(pos, yq, 1), 0).astype(float)
        T_r, T_c = pc.transform_counts(u, pos)
        mu_tol = rc.gamma(L + 1) * mu
        r_tol = np.abs(c_ref) * mu_tol + 2 * pc.EPS * T_r * np.abs(r_ref)
        f = apply(ctx, g, G, h, origin, y, est=1, want_J=False, reps=reps)[0]
        err = np.abs(f.astype(LD) - r_ref)
        assert np.all(err <= r_tol), note("r", err, r_tol)
        note("poisson r", err, r_tol)
        f1, J = apply(ctx, g[::reps], G, h, origin, y, est=1)
        assert same_bits(f1, f[::reps])
        c1, T1 = c_ref[::reps], T_c[::reps]
        J_ref = c1[:, :, None] * HG
        J_tol = np.abs(c1)[:, :, None] * (rc.gamma(L + 1) * HG_abs
                                          + HG_abs * (2 * pc.EPS * (T1 + 1) + rc.gamma(L + 1))[:, :, None])
        err = np.abs(J.astype(LD) - J_ref)
        assert np.all(err <= J_tol), note("cJ", err, J_tol)
        note("poisson c (H G)", err, J_tol)


# ---- kernel: the entry --------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_position(ctx):
    """ctx = 1, est, nan_policy, B, reps, m, nc, L = 8, origin, h, h_stride = 11, g, G, y = 14, w, w_stride = 16,
    f (both outputs NULL) = 17, J (reps != 1) = 18.  The checks come before any launch, so a small buffer stands in."""
    lib = ctx.lib
    with me.Dev(ctx) as d:
        p = d.up(np.ones(64))
        good = dict(est=0, nan=0, B=1, reps=1, m=4, nc=2, L=3, origin=1, h=p, h_stride=0, g=p, G=p, y=p, w=p, w_stride=0,
                    f=p, J=p, mask=None)

        def rc_of(**kw):
            a = dict(good, **kw)
            return lib.blsq_response_apply_dev(ctx.h, *[a[k] for k in good])
        assert rc_of() == 0
        ctx.sync()
        assert lib.blsq_response_apply_dev(None, *good.values()) == -1
        for want, kw in [(2, dict(est=2)), (2, dict(est=-1)), (3, dict(nan=2)), (4, dict(B=0)), (5, dict(reps=0)),
                         (6, dict(m=0)), (7, dict(nc=0)), (8, dict(L=0)), (8, dict(L=1025, origin=0)),
                         (9, dict(origin=3)), (9, dict(origin=-1)), (10, dict(h=None)), (11, dict(h_stride=2)),
                         (12, dict(g=None)), (12, dict(g=None, f=None, est=1, w=None)), (13, dict(G=None)),
                         (14, dict(est=1, y=None, w=None)), (14, dict(nan=1, y=None)), (15, dict(est=1)),
                         (16, dict(w_stride=3)), (17, dict(f=None, J=None)), (18, dict(reps=2)),
                         (2, dict(est=5, B=0)), (4, dict(B=0, L=0))]:        # (the first bad argument is reported)
            assert rc_of(**kw) == -want, (want, kw, rc_of(**kw))
            assert b"invalid argument" in lib.blsq_last_error(ctx.h)
        assert rc_of(h_stride=3) == 0 and rc_of(w_stride=4) == 0             # the other stride of each array
        assert rc_of(g=None, f=None) == 0 and rc_of(G=None, J=None) == 0     # what an output does not need may be NULL
        assert rc_of(y=None) == 0 and rc_of(w=None, w_stride=7) == 0         # (w_stride is not read without w)
        ctx.sync()


def test_one_call_is_one_unit_of_the_model_eval_slot(ctx):
    d = draws(16, 4, B=2, reps=1, seed=8)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        apply(ctx, d["g"], d["G"], rc.irf(5, 2.0, 1.0), 0, d["y"], d["wm"])
        ctx.sync()
        t = ctx.timing_read()
    finally:
        ctx.timing(False)
    assert t["model_eval"][1] == 1 and sum(c for _, c in t.values()) == 1


# ---- fits ---------------------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-13, xtol=1e-13, gtol=1e-13)
_cases, _fits = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = rc.CASES[name]()
    return _cases[name]


def fit(ctx, name, method, route, jac=None, response=True):
    """route A: the numpy model and its Jacobian as callables on the device driver; B: the spec on the device; C: the
    spec with driver='host'.  One fit per key for all the tests that look at it."""
    key = (name, method, route, jac, response)
    if key not in _fits:
        c = case_of(name)
        M = models.compose(c["spec"])
        kw = dict(bounds=c["bounds"], sigma=c["sigma"], method=method, ctx=ctx, **c["kw"], **TOL)
        if response:
            kw.update(response=c["h"], response_origin=c["origin"])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if route == "A":
                _fits[key] = bounded_lsq.curve_fit_batch(M.f, c["x"], c["Y"], c["P0"], jac=M.jac if jac is None else jac,
                                                         driver="device", **kw)
            else:
                _fits[key] = bounded_lsq.curve_fit_batch(c["spec"], c["x"], c["Y"], c["P0"], jac=jac,
                                                         driver="device" if route == "B" else "host", **kw)
    return _fits[key]


def within_six_standard_errors(c, got, what):
    se = np.sqrt(np.einsum("bii->bi", got[1]))
    free = se > 0
    dev = np.abs(got[0] - c["truth"])
    assert np.all(dev[free] <= 6 * se[free]), (what, np.max(dev[free] / se[free]))
    assert np.allclose(dev[~free], 0, atol=1e-9 * np.max(np.abs(c["truth"])))


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_fits_agree_across_their_routes_and_find_the_truth(ctx, name, method):
    """Decay (with sigma, and as counts under the Poisson estimator), the broadened line under 'omit', the tied widths
    (a copy and a ratio) and a kernel per problem: every problem succeeds on every route, the routes agree pairwise,
    and popt lies within 6 standard errors of the truth."""
    c = case_of(name)
    R = {route: fit(ctx, name, method, route) for route in "ABC"}
    for route, got in R.items():
        assert all(r.success for r in got[2]), (name, method, route, [r.status for r in got[2]])
        within_six_standard_errors(c, got, (name, method, route))
    for a, b in ("AB", "AC", "BC"):
        me.agree(R[a], R[b], (name, method, a, b))
    pm, fres, jres = rc.definition(c)
    X = np.stack([r.x_free if pm is not None else r.x for r in R["B"][2]])
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(np.stack([r.fun for r in R["B"][2]]), fres(X), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(np.stack([r.jac for r in R["B"][2]]), jres(X), rtol=1e-9, atol=1e-9)
    if c["kw"].get("nan_policy") == "omit":
        assert all(r.nobs == 56 for r in R["B"][2])


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", rc.FD_CASES)
def test_finite_differences_reach_the_same_optimum(ctx, name, method):
    ref = fit(ctx, name, method, "B")
    for route in "ABC":
        got = fit(ctx, name, method, route, jac="2-point")
        assert all(r.success for r in got[2]), (name, method, route)
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-4, atol=1e-7, err_msg=str((name, method, route)))


@pytest.mark.parametrize("name", ["decay-sigma-exp2", "line-tied-ratio", "decay-per-problem-h"])
def test_evaluate_predicts_the_convolved_model(ctx, name):
    c = case_of(name)
    popt = fit(ctx, name, "trf", "B")[0]
    plain = models.evaluate(c["spec"], c["x"], popt, ctx=ctx)
    got = models.evaluate(c["spec"], c["x"], popt, ctx=ctx, response=c["h"], response_origin=c["origin"])
    L = c["h"].shape[-1]
    ref = models.apply_response(plain.astype(LD), c["h"], c["origin"])
    mag = models.apply_response(np.abs(plain).astype(LD), np.abs(c["h"]), c["origin"])
    err, tol = np.abs(got.astype(LD) - ref), rc.gamma(L + 3) * mag
    assert np.all(err <= tol), note("evaluate", err, tol)
    note("evaluate / gamma_{L+3}", err, tol)


def test_binned_model_through_a_response(ctx):
    """Contiguous bins: bin integrals, then a convolution over the bins; the device route against the host route."""
    c = case_of("decay-sigma-exp+poly")
    m = c["x"].size
    edges = np.arange(m + 1, dtype=float) - 0.5
    kw = dict(bounds=c["bounds"], sigma=c["sigma"], ctx=ctx, binned=True, response=c["h"], absolute_sigma=True, **TOL)
    dev = bounded_lsq.curve_fit_batch(c["spec"], edges, c["Y"], c["P0"], driver="device", **kw)
    host = bounded_lsq.curve_fit_batch(c["spec"], edges, c["Y"], c["P0"], driver="host", **kw)
    assert all(r.success for r in dev[2]) and all(r.success for r in host[2])
    me.agree(dev, host, "binned")
    got = models.evaluate(c["spec"], edges, dev[0], ctx=ctx, binned=True, response=c["h"])
    want = models.apply_response(models.binned(c["spec"]).f(edges, dev[0]), c["h"], 0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


NAMES = tuple(_abi.MODEL_EVAL_ARGS) + ("blsq_linear_eval_dev", ENTRY)


@pytest.mark.parametrize("name", ["decay-counts-exp2", "line-omit", "line-tied-ratio"])
def test_device_route_reaches_the_inner_entry_and_the_response_entry_alone(ctx, name, monkeypatch):
    c = case_of(name)
    ref = fit(ctx, name, "trf", "B")

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    monkeypatch.setattr(_models, "apply_response", boom)
    monkeypatch.setattr(_models, "poisson_transform", boom)
    counts = me.count_entries(ctx, monkeypatch, NAMES)
    kw = dict(bounds=c["bounds"], sigma=c["sigma"], ctx=ctx, driver="device", **c["kw"], **TOL)
    got = bounded_lsq.curve_fit_batch(c["spec"], c["x"], c["Y"], c["P0"], response=c["h"],
                                      response_origin=c["origin"], **kw)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    reached = {k for k, v in counts.items() if v}
    for k in counts:
        counts[k] = 0
    # the inner entry: the one the same fit without the keyword reaches with ydata=None
    M = models.compose(c["spec"])
    tied = c["kw"].get("tied")
    pm = bounded_lsq.ParamMap(M.n, None, tied) if tied else None
    B, m = c["Y"].shape
    with models.DeviceModel(ctx, c["spec"], B, m, M.n, c["x"], param_map=pm, Pfix=c["P0"] if pm else None) as dm:
        with me.Dev(ctx) as d:
            dm.fun_dev(d.up(c["P0"] if pm is None else pm.reduce_x(c["P0"])), d.up(np.zeros((B, m))), 1)
            ctx.sync()
    inner = {k for k, v in counts.items() if v}
    assert len(inner) == 1 and ENTRY not in inner
    assert reached == inner | {ENTRY}, (reached, inner)
    for k in counts:
        counts[k] = 0
    bounded_lsq.curve_fit_batch(c["spec"], c["x"], c["Y"], c["P0"], **kw)    # without the keyword: never
    assert counts[ENTRY] == 0 and sum(counts.values()) > 0
