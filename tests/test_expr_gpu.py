"""Expression models on the GPU (blsq_expr_eval_dev, csrc/expr_kernels.hip) against the truth file and
the numpy definition (tests/_expr_cases.py has the cases, the magnitudes, K_REF and the bound
4 max(K_REF, 1) eps mag), and end to end through curve_fit_batch."""
import ctypes as C
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _abi, models

import _expr_cases as ec
from _model_eval import Dev, agree, ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
SENTINEL = -7.25
worst = {}


def note(key, value):
    worst[key] = max(worst.get(key, 0.0), value)


def ev(ctx, prog, nf, t, X, m=None, npfix=0, Pfix=None, y=None, w=None, reps=1, want_f=True, want_J=False, est=0,
       nan_policy=0, mask=None, fill=np.nan, ncoord=1, raw=None):
    """One call of blsq_expr_eval_dev on host arrays -> (rc, f or None, J or None).  t (m,) / (B, m) — (C, m) /
    (B, C, m) —, X (B * reps, nf); `raw`: positional arguments (by 0-based index behind ctx) replaced as they are."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    m = t.shape[-1] if m is None else m
    B = X.shape[0] // reps
    per_problem = t.ndim == (2 if ncoord == 1 else 3)
    ops = np.ascontiguousarray(prog.ops, dtype=np.uint64)
    consts = np.ascontiguousarray(prog.consts, dtype=np.float64)
    with Dev(ctx) as d:
        f_shape, J_shape = (B * reps, m), (B, m, nf)
        df = d.up(np.full(f_shape, fill)) if want_f else None
        dJ = d.up(np.full(J_shape, fill)) if want_J else None
        a = [est, nan_policy, B, reps, m, nf, npfix, ncoord, len(ops), ops.ctypes.data_as(C.POINTER(C.c_uint64)),
             int(prog.root), len(consts), consts.ctypes.data_as(_abi.c_double_p), d.up(t), ncoord * m if per_problem else 0,
             d.up(y), d.up(w), m if (w is not None and np.ndim(w) == 2) else 0, d.up(X), d.up(Pfix), df, dJ,
             d.up(None if mask is None else np.asarray(mask, dtype=np.int32))]
        for i, v in (raw or {}).items():
            a[i] = v
        rc = ctx.lib.blsq_expr_eval_dev(ctx.h, *a)
        if rc != 0:
            return rc, None, None
        return (0, ctx.to_host(df, f_shape, np.float64) if want_f else None,
                ctx.to_host(dJ, J_shape, np.float64) if want_J else None)


def case(name, m):
    """The model, P, the first m points of t and the truth and magnitudes there."""
    d = ec.truth()[name]
    return ec.model(name), d["P"], d["t"][:m], {k: d[k][:, :m] for k in ("f", "J", "fmag", "Jmag")}


# ---- 1. the seven cases against the truth ----------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", list(ec.CASES))
def test_cases_against_the_truth(ctx, name, m):
    """f (with reps = 3) and J together, f alone, J alone; w absent, (m,) and (B, m); y absent and present: every value
    within 4 max(K_REF, 1) eps mag of the truth (the weights and y are powers of two and small integers times eps-free
    values, applied to truth and magnitude alike)."""
    M, P, t, tr = case(name, m)
    n, bound = M.n, ec.device_bound(name)
    rng = np.random.default_rng(m)
    rc, f, J = ev(ctx, M.program, n, t, P, want_J=True)
    assert rc == 0
    kf, kj = ec.excess(f, tr["f"], tr["fmag"]), ec.excess(J, tr["J"], tr["Jmag"])
    print("%s m=%d: f %.3f J %.3f of %.3g" % (name, m, kf, kj, bound))
    note(name, max(kf, kj) / bound)
    assert kf <= bound and kj <= bound
    # f alone and J alone give the bits of the joint launch; per-problem abscissae too
    assert same_bits(ev(ctx, M.program, n, t, P)[1], f)
    assert same_bits(ev(ctx, M.program, n, np.tile(t, (ec.B, 1)), P, want_f=False, want_J=True)[2], J)
    # reps = 3: the point q = b * reps + r; rows 1 and 2 of every problem are its neighbours' parameters
    X3 = np.stack([P, np.roll(P, 1, axis=0), np.roll(P, 2, axis=0)], axis=1).reshape(3 * ec.B, n)
    f3 = ev(ctx, M.program, n, t, X3, reps=3)[1].reshape(ec.B, 3, m)
    for r in range(3):
        assert same_bits(f3[:, r], np.roll(f, r, axis=0))
    # weights and data: w (v - y) and w J; powers of two scale truth and magnitude exactly
    y = tr["f"] + rng.integers(-3, 4, tr["f"].shape) * 0.25
    for w in (2.0 ** rng.integers(-2, 3, m), 2.0 ** rng.integers(-2, 3, (ec.B, m))):
        rc, fw, Jw = ev(ctx, M.program, n, t, P, y=y, w=w, want_J=True)
        assert rc == 0
        wb = np.broadcast_to(w, (ec.B, m))
        assert ec.excess(fw, wb * (tr["f"] - y), wb * (tr["fmag"] + np.abs(y))) <= bound
        assert same_bits(Jw, wb[:, :, None] * J)
        assert same_bits(ev(ctx, M.program, n, t, P, w=w)[1], wb * f)             # y absent: w v
    assert same_bits(ev(ctx, M.program, n, t, P, y=y, want_J=True)[2], J)          # w absent: the row as it is


# ---- 2. without a library function: the definition's bits ------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", ec.FUNCTION_FREE)
def test_function_free_cases_are_the_definition_bit_for_bit(ctx, name, m):
    M, P, t, _ = case(name, m)
    rc, f, J = ev(ctx, M.program, M.n, t, P, want_J=True)
    assert rc == 0 and same_bits(f, M.f(t, P)) and same_bits(J, M.jac(t, P))
    y, w = np.cos(np.arange(ec.B * m)).reshape(ec.B, m), 1.0 + np.arange(m) / 7.0
    rc, f, J = ev(ctx, M.program, M.n, t, P, y=y, w=w, want_J=True)
    assert same_bits(f, w * (M.f(t, P) - y)) and same_bits(J, w[:, None] * M.jac(t, P))


def test_several_coordinates_and_a_leaf_root(ctx):
    M = models.expression("a*u*u+b*v-w/x+sqrt(u*u+x*x)", ("a", "b"), coords=("u", "v", "w", "x"))
    rng = np.random.default_rng(4)
    P = rng.uniform(0.5, 2, (3, 2))
    for T in (rng.uniform(0.5, 2, (4, 70)), rng.uniform(0.5, 2, (3, 4, 70))):
        rc, f, J = ev(ctx, M.program, 2, T, P, want_J=True, ncoord=4)
        assert rc == 0 and same_bits(f, M.f(T, P)) and same_bits(J, M.jac(T, P))
    assert same_bits(models.evaluate(M, T, P, ctx=ctx), M.f(T, P))
    leaf = models.expression("+a", ("a",))
    assert leaf.program.nops == 0
    rc, f, J = ev(ctx, leaf.program, 1, np.zeros(5), P[:, :1], want_J=True)
    assert rc == 0 and same_bits(f, np.repeat(P[:, :1], 5, axis=1)) and same_bits(J, np.ones((3, 5, 1)))


# ---- 3. the mask -------------------------------------------------------------------------------------------------------
def test_masked_problems_keep_the_sentinel(ctx):
    M, P, t, _ = case("lorentz_root", 130)
    rc, f0, J0 = ev(ctx, M.program, M.n, t, P, want_J=True)
    rc, f, J = ev(ctx, M.program, M.n, t, P, want_J=True, mask=[1, 0, 1], fill=SENTINEL)
    assert rc == 0
    assert np.all(f[1] == SENTINEL) and np.all(J[1] == SENTINEL)
    assert same_bits(f[[0, 2]], f0[[0, 2]]) and same_bits(J[[0, 2]], J0[[0, 2]])


# ---- 4. omission -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (65, 130))
def test_omitted_rows_are_zero_in_every_bit(ctx, m):
    M, P, t, tr = case("decay", m)
    y = tr["f"] + 0.125
    w = np.full((ec.B, m), 2.0)
    rc, f0, J0 = ev(ctx, M.program, M.n, t, P, y=y, w=w, want_J=True)
    hole = np.zeros((ec.B, m), dtype=bool)
    hole[0, ::3] = hole[1, -1] = hole[2, :] = True
    hole[2, 64 % m] = False
    yn, wn, tn = np.where(hole, np.nan, y), np.where(hole, np.nan, w), np.where(hole, np.nan, np.tile(t, (ec.B, 1)))
    rc, f, J = ev(ctx, M.program, M.n, tn, P, y=yn, w=wn, want_J=True, nan_policy=1)
    assert rc == 0
    zero = np.zeros(1).tobytes()
    assert all(v.tobytes() == zero for v in f[hole]) and all(v.tobytes() == zero for v in J[hole].ravel())
    assert same_bits(f[~hole], f0[~hole]) and same_bits(J[~hole], J0[~hole])
    assert same_bits(ev(ctx, M.program, M.n, t, P, y=y, w=w, want_J=True, nan_policy=1)[2], J0)   # no NaN: no change


# ---- 5. Poisson ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("decay", "lorentz_root"))
def test_poisson_against_the_transform_of_the_definition(ctx, name):
    """f = r and J = c J_model of models.poisson_transform at the definition's value, counts with zeros among them.
    The bound is the one tests/_poisson_cases.py derives for the built-in kernels (``transform_counts``: T_r and T_c
    roundings of the transform's own operations, committed once by numpy and once by the device):
        |f - r| <= |c| v_tol + 2 eps T_r |r|        |J - c Jm| <= |c| (Jm_tol + |Jm| (2 eps (T_c + 1) + v_tol / mu))
    with v_tol and Jm_tol what separates the device's model value and row from the definition's: nothing for
    lorentz_root (no library function: the same bits), (4 max(K_REF, 1) + K_REF) eps mag for decay (the device's
    bound and the definition's, both against the truth)."""
    import _poisson_cases as pc
    M, P, t, tr = case(name, 130)
    rng = np.random.default_rng(5)
    mu, Jm = M.f(t, P), M.jac(t, P)
    assert np.all(mu > 0)
    y = rng.poisson(mu).astype(float)
    y[:, ::7] = 0.0
    rc, f, J = ev(ctx, M.program, M.n, t, P, y=y, want_J=True, est=1)
    assert rc == 0
    r, c = models.poisson_transform(mu, y)
    k = 0.0 if name in ec.FUNCTION_FREE else ec.device_bound(name) + ec.K_REF[name]
    v_tol, Jm_tol = k * ec.EPS * tr["fmag"], k * ec.EPS * tr["Jmag"]
    pos = y > 0
    T_r, T_c = pc.transform_counts(np.where(pos, (mu - y) / np.where(pos, y, 1), 0), pos)
    r_tol = np.abs(c) * v_tol + 2 * ec.EPS * T_r * np.abs(r)
    J_tol = np.abs(c)[:, :, None] * (Jm_tol + np.abs(Jm) * (2 * ec.EPS * (T_c + 1) + v_tol / mu)[:, :, None])
    ef, eJ = np.abs(f - r), np.abs(J - c[:, :, None] * Jm)
    note("poisson " + name, max(np.max(ef / r_tol), np.max(eJ / np.where(J_tol > 0, J_tol, 1))))
    assert np.all(ef <= r_tol) and np.all(eJ <= J_tol)
    assert same_bits(ev(ctx, M.program, M.n, t, P, y=y, est=1)[1], f)              # f alone
    assert ev(ctx, M.program, M.n, t, P, est=1)[0] == -17 and ev(ctx, M.program, M.n, t, P, y=y, w=t, est=1)[0] == -18


# ---- 6. the mapped program -----------------------------------------------------------------------------------------------
def test_mapped_program(ctx):
    """f bit-equal to the unmapped launch at the expanded parameters (function-free case); J of the mapped launch within
    the bound of the bound program's magnitudes against reduce_jac of the truth-side definition."""
    M, P, t, _ = case("lorentz_root", 130)
    pm = bounded_lsq.ParamMap(M.n, [3], {5: (2, -2.0, 0.25), 4: 0})
    Bd = M.bind(pm)
    X, full = pm.reduce_x(P), pm.expand_x(pm.reduce_x(P), P)
    rc, f, J = ev(ctx, Bd.program, pm.nf, t, X, npfix=M.n, Pfix=P, want_J=True)
    assert rc == 0
    assert same_bits(f, ev(ctx, M.program, M.n, t, full)[1])
    assert same_bits(f, Bd.f(t, X, P)) and same_bits(J, Bd.jac(t, X, P))          # function-free: the definition's bits
    Jmag = ec.magnitudes(Bd.program, [t], X, P)[1]
    k = ec.excess(J, pm.reduce_jac(M.jac(t, full)), Jmag)
    note("mapped", k / ec.device_bound("lorentz_root"))
    assert k <= ec.device_bound("lorentz_root")
    # with library functions: the decay case, a tie that merges the two exponentials' arguments
    M, P, t, tr = case("decay", 130)
    pm = bounded_lsq.ParamMap(M.n, [4], {3: (2, 4.0, 0.1)})
    Bd = M.bind(pm)
    X = pm.reduce_x(P)
    rc, f, J = ev(ctx, Bd.program, pm.nf, t, X, npfix=M.n, Pfix=P, want_J=True)
    fmag, Jmag = ec.magnitudes(Bd.program, [t], X, P)
    assert rc == 0 and ec.excess(f, Bd.f(t, X, P), fmag) <= ec.device_bound("decay")
    assert ec.excess(J, Bd.jac(t, X, P), Jmag) <= ec.device_bound("decay")
    assert ev(ctx, Bd.program, pm.nf, t, X, npfix=M.n)[0] == -21                   # a PFIX operand without Pfix


# ---- 7. bad arguments ----------------------------------------------------------------------------------------------------
def test_every_bad_argument_returns_its_position(ctx):
    M, P, t, _ = case("decay", 65)
    from bounded_lsq import _expr as E
    n = M.n
    good = dict(prog=M.program, nf=n, t=t, X=P)
    assert ev(ctx, **good)[0] == 0
    y = np.ones((ec.B, 65))
    bad_op = M.program._replace(ops=np.concatenate([M.program.ops[:-1], np.array([14], dtype=np.uint64)]))
    fwd = M.program._replace(ops=np.concatenate([[np.uint64(E.op_word(E.NEG, E.operand(E.TAPE, 3)))], M.program.ops[1:]]))
    for kw, want in [
        (dict(est=2), -2), (dict(est=-1), -2), (dict(nan_policy=2), -3), (dict(raw={2: 0}), -4), (dict(raw={3: 0}), -5),
        (dict(raw={4: 0}), -6), (dict(raw={5: 0}), -7), (dict(raw={5: 65}), -7), (dict(raw={5: n - 1}), -11),
        (dict(raw={6: -1}), -8), (dict(raw={6: 65}), -8), (dict(raw={7: 0}), -9), (dict(raw={7: 5}), -9),
        (dict(raw={8: 65}), -10), (dict(raw={8: -1}), -10), (dict(raw={9: None}), -11), (dict(prog=bad_op), -11),
        (dict(prog=fwd), -11), (dict(raw={10: E.operand(E.TAPE, 11)}), -12), (dict(raw={10: -1}), -12),
        (dict(raw={11: 33}), -13), (dict(raw={11: 0}), -11), (dict(raw={12: None}), -14), (dict(raw={13: None}), -15),
        (dict(raw={14: 64}), -16), (dict(est=1), -17), (dict(nan_policy=1), -17), (dict(est=1, y=y, w=t), -18),
        (dict(w=t, raw={17: 3}), -19), (dict(raw={18: None}), -20), (dict(want_f=False), -22),
        (dict(want_J=True, reps=3, X=np.tile(P, (3, 1))), -23),
    ]:
        args = dict(good)
        args.update(kw)
        rc = ev(ctx, **args)[0]
        assert rc == want, (kw, rc, want)
    with pytest.raises(_abi.BlsqError, match="nf must be"):
        ctx.check(ev(ctx, raw={5: 0}, **good)[0], "blsq_expr_eval_dev")


# ---- 8. end to end -----------------------------------------------------------------------------------------------------
TOL = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)
E2E = "a1*exp(-r1*t)+a2*exp(-r2*t)+c"
E2E_PARAMS = ("a1", "r1", "a2", "r2", "c")


@pytest.fixture(scope="module")
def e2e():
    """B = 8, m = 70: two decays over a constant, Poisson counts, a box around the truth."""
    rng = np.random.default_rng(11)
    Bn, m = 8, 70
    t = np.linspace(0.0, 6.0, m)
    truth = np.column_stack([rng.uniform(300, 600, Bn), rng.uniform(1.5, 2.5, Bn), rng.uniform(150, 300, Bn),
                             rng.uniform(0.3, 0.6, Bn), rng.uniform(20, 40, Bn)])
    M = models.expression(E2E, E2E_PARAMS)
    Y = rng.poisson(M.f(t, truth)).astype(float)
    P0 = truth * rng.uniform(0.9, 1.1, truth.shape)
    bounds = (truth * 0.4, truth * 2.5)
    return dict(M=M, t=t, Y=Y, P0=P0, bounds=bounds, truth=truth)


def fit(ctx, pr, f, driver, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_batch(f, pr["t"], pr["Y"], pr["P0"], bounds=pr["bounds"], estimator="poisson",
                                           driver=driver, ctx=ctx, **TOL, **kw)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_fit_agrees_with_the_composite_and_the_host_driver(ctx, e2e, method):
    """The expression on the device against 'exp*2+poly*1' on the device and against the expression with
    driver='host': popt to rtol 1e-6 / atol 1e-9 and the normalised pcov to 1e-6 (``agree``: the tolerance
    tests/test_composite_gpu.py uses between its routes)."""
    dev = fit(ctx, e2e, e2e["M"], "device", method=method)
    assert all(r.success for r in dev[2]), [r.status for r in dev[2]]
    comp = fit(ctx, e2e, "exp*2+poly*1", "device", method=method)
    host = fit(ctx, e2e, e2e["M"], "host", method=method)
    agree(comp, dev, ("composite", method))
    agree(host, dev, ("host", method))
    lb, ub = e2e["bounds"]
    assert np.all(dev[0] >= lb) and np.all(dev[0] <= ub)
    np.testing.assert_allclose(np.stack([r.fun for r in dev[2]]),
                               models.poisson_transform(e2e["M"].f(e2e["t"], dev[0]), e2e["Y"])[0], rtol=1e-9, atol=1e-9)


def test_fit_through_a_response_and_by_finite_differences(ctx, e2e):
    h = np.array([0.1, 0.4, 0.3, 0.15, 0.05])
    pr = dict(e2e)
    rng = np.random.default_rng(12)
    pr["Y"] = rng.poisson(models.apply_response(e2e["M"].f(e2e["t"], e2e["truth"]), h, 0)).astype(float)
    dev = fit(ctx, pr, e2e["M"], "device", response=h)
    comp = fit(ctx, pr, "exp*2+poly*1", "device", response=h)
    host = fit(ctx, pr, e2e["M"], "host", response=h)
    assert all(r.success for r in dev[2])
    agree(comp, dev, "response, composite")
    agree(host, dev, "response, host")
    an = fit(ctx, e2e, e2e["M"], "device")
    fd = fit(ctx, e2e, e2e["M"], "device", jac="2-point")
    assert all(r.success for r in fd[2])
    np.testing.assert_allclose(fd[0], an[0], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("kw", [
    dict(sigma=np.full(70, 2.0), fixed=[4], tied={3: (1, 0.25, 0.0)}, nan_policy="omit", leverage=True),
    dict(loss="soft_l1", f_scale=3.0, fixed=[4], method="dogbox"),
], ids=["map-sigma-omit-leverage", "loss"])
def test_keywords_against_the_host_driver(ctx, e2e, kw):
    """The keywords an ExprModel takes, each against driver='host' (the numpy definition): least squares on data whose
    second rate is a quarter of the first, with one missing point per problem."""
    M, t = e2e["M"], e2e["t"]
    rng = np.random.default_rng(13)
    truth = e2e["truth"].copy()
    truth[:, 3] = 0.25 * truth[:, 1]
    Y = M.f(t, truth) + 2.0 * rng.standard_normal((8, 70))
    if "nan_policy" in kw:
        Y[:, 5] = np.nan
    P0 = truth * rng.uniform(0.9, 1.1, truth.shape)
    P0[:, 4], P0[:, 3] = truth[:, 4], 0.25 * P0[:, 1]
    common = dict(bounds=(0.4 * truth, 2.5 * truth), ctx=ctx, **TOL, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dev = bounded_lsq.curve_fit_batch(M, t, Y, P0, driver="device", **common)
        host = bounded_lsq.curve_fit_batch(M, t, Y, P0, driver="host", **common)
    assert all(r.success for r in dev[2]) and all(r.success for r in host[2])
    agree(host, dev, sorted(kw))
    assert np.array_equal(dev[0][:, 4], P0[:, 4])
    if "tied" in kw:
        assert np.array_equal(dev[0][:, 3], 0.25 * dev[0][:, 1] + 0.0)
        for a, b in zip(host[2], dev[2]):
            np.testing.assert_allclose(b.leverage, a.leverage, rtol=1e-6, atol=1e-9)
            assert b.nobs == 69


# ---- 9. nothing runs in Python -------------------------------------------------------------------------------------------
def test_device_route_evaluates_nothing_in_python(ctx, e2e, monkeypatch):
    from bounded_lsq import _expr, _outer
    want = fit(ctx, e2e, e2e["M"], "device")

    def boom(*a, **k):
        raise AssertionError("a host evaluation was reached")
    monkeypatch.setattr(_expr.ExprModel, "f", boom)
    monkeypatch.setattr(_expr.ExprModel, "jac", boom)
    monkeypatch.setattr(_expr, "interpret", boom)
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    calls = {}
    lib = ctx.lib

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.endswith("_eval_dev") or "model_eval" in name or name.startswith("blsq_response"):
                def counted(*a):
                    calls[name] = calls.get(name, 0) + 1
                    return fn(*a)
                return counted
            return fn
    monkeypatch.setattr(ctx, "lib", Counting())
    ctx.timing(True, only="model_eval")
    ctx.timing_reset()
    try:
        got = fit(ctx, e2e, e2e["M"], "device")
        ctx.sync()
        timed = ctx.timing_read()["model_eval"][1]
    finally:
        ctx.timing(False)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert set(calls) == {"blsq_expr_eval_dev"} and calls["blsq_expr_eval_dev"] >= 2
    assert timed == calls["blsq_expr_eval_dev"]                                   # every unit of the slot is the new entry


def test_report_margins():
    """Not a check: prints the worst fraction of every margin the tests above used (run with -s to see it)."""
    for k in sorted(worst):
        print("margin %-14s worst fraction %.3g" % (k, worst[k]))
