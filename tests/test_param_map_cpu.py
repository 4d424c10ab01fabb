"""Fixed and tied parameters without a GPU: ``ParamMap`` against formulas written out by hand, its numpy wrappers against
central differences in extended precision, the hand-written reduced models of the end-to-end tests against the wrapped
full models, and what the ``fixed=`` / ``tied=`` keywords of ``curve_fit_batch`` / ``curve_fit`` check and hand on."""
import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models
from bounded_lsq._params import ParamMap

import _model_cases as mc
import _param_map_cases as pc

LD = np.longdouble

# n, fixed, tied, pmap, leaders — written out by hand
MAPS = {
    "fixed_only": (5, [1, 3], None, [0, -1, 1, -1, 2], [0, 2, 4]),
    "fixed_mask": (4, [False, False, True, False], {}, [0, 1, -1, 2], [0, 1, 3]),
    "tied_only": (7, None, {5: 2}, [0, 1, 2, 3, 4, 2, 5], [0, 1, 2, 3, 4, 6]),
    "both": (7, [1, 4], {5: 2}, [0, -1, 1, 2, -1, 1, 3], [0, 2, 3, 6]),
    "three_members": (10, [], {5: 2, 8: 2}, [0, 1, 2, 3, 4, 2, 5, 6, 2, 7], [0, 1, 2, 3, 4, 6, 7, 9]),
    "leader_not_first": (7, [0], {1: 4, 2: 5}, [-1, 1, 2, 0, 1, 2, 3], [3, 4, 5, 6]),    # slots follow the leaders
}


@pytest.mark.parametrize("key", list(MAPS))
def test_param_map_against_hand_written_formulas(key):
    n, fixed, tied, pmap, leaders = MAPS[key]
    pm = ParamMap(n, fixed, tied)
    nf = len(leaders)
    assert pm.n == n and pm.nf == nf and not pm.identity
    assert pm.pmap.dtype == np.int32 and pm.pmap.tolist() == pmap and pm.leaders.tolist() == leaders
    rng = np.random.default_rng(n)
    B, m = 3, 5
    P = rng.standard_normal((B, n))
    for j, i in (tied or {}).items():
        P[:, j] = P[:, i]
    # reduce_x / expand_x: inverse of each other on vectors that satisfy the ties; only fixed columns of Pfix are read
    X = pm.reduce_x(P)
    assert X.shape == (B, nf) and np.array_equal(X, P[:, leaders])
    Pfix = np.where(np.asarray(pmap) < 0, P, np.nan)
    assert np.array_equal(pm.expand_x(X, Pfix), P)
    assert np.array_equal(pm.expand_x(X[1], Pfix[1]), P[1])                    # one vector
    assert np.array_equal(pm.expand_x(np.repeat(X, 2, axis=0).reshape(B, 2, nf), Pfix[:, None, :]),
                          np.repeat(P, 2, axis=0).reshape(B, 2, n))            # broadcast over points
    # reduce_jac: the explicit loop, bit for bit
    J = rng.standard_normal((B, m, n))
    assert np.array_equal(pm.reduce_jac(J), pc.explicit_reduce_jac(J, pmap, nf))
    assert np.array_equal(pm.reduce_jac(J[0]), pc.explicit_reduce_jac(J[0], pmap, nf))
    # expand_cov = T C T^T exactly, with T written out
    T = np.zeros((n, nf))
    for j, k in enumerate(pmap):
        if k >= 0:
            T[j, k] = 1.0
    assert np.array_equal(pm.matrix(), T)
    A = rng.standard_normal((B, nf, nf))
    C = A @ A.transpose(0, 2, 1)
    full = pm.expand_cov(C)
    assert full.shape == (B, n, n) and np.array_equal(full, T @ C @ T.T)
    assert np.array_equal(pm.expand_cov(C[0]), T @ C[0] @ T.T)
    for j, k in enumerate(pmap):
        if k < 0:
            assert not full[:, j, :].any() and not full[:, :, j].any()
        else:
            assert np.array_equal(full[:, j, :], full[:, leaders[k], :])
    assert np.all(np.isinf(pm.expand_cov(np.full((nf, nf), np.inf))[np.ix_(leaders, leaders)]))
    # expand_mask: fixed -> 0, tied -> the leader's
    mask = rng.integers(-1, 2, (B, nf))
    want = np.array([[0 if k < 0 else row[k] for k in pmap] for row in mask])
    assert np.array_equal(pm.expand_mask(mask), want) and np.array_equal(pm.expand_mask(mask[0]), want[0])


def test_reduce_bounds_intersects_the_groups():
    pm = ParamMap(7, [1, 4], {5: 2})                                           # slots: 0, (2, 5), 3, 6
    lb = np.array([-1.0, 5.0, 0.2, -np.inf, 9.0, 0.3, -2.0])
    ub = np.array([1.0, 5.0, 0.9, np.inf, 9.0, 0.8, 2.0])                      # (lb == ub where fixed: ignored)
    lo, hi = pm.reduce_bounds(lb, ub)
    assert lo.tolist() == [-1.0, 0.3, -np.inf, -2.0] and hi.tolist() == [1.0, 0.8, np.inf, 2.0]
    LB, UB = np.stack([lb, lb - 1]), np.stack([ub, ub + 1])
    lo2, hi2 = pm.reduce_bounds(LB, UB)
    assert lo2.shape == (2, 4) and lo2[1].tolist() == [-2.0, -0.7, -np.inf, -3.0] and hi2[1, 1] == 1.8
    ub_bad = ub.copy()
    ub_bad[5] = 0.1                                                            # [0.2, 0.9] and [0.3, 0.1]
    with pytest.raises(ValueError, match=r"\[2, 5\]"):
        pm.reduce_bounds(lb, ub_bad)
    with pytest.raises(ValueError, match="7 entries"):
        pm.reduce_bounds(lb[:6], ub)


def test_identity_and_empty_keywords():
    for fixed, tied in ((None, None), ([], {}), (np.zeros(4, dtype=bool), None), ((), {})):
        pm = ParamMap(4, fixed, tied)
        assert pm.identity and pm.nf == 4 and pm.pmap.tolist() == [0, 1, 2, 3]


def test_every_value_error_names_the_index():
    with pytest.raises(ValueError, match="`fixed` index 5 "):
        ParamMap(5, [5])
    with pytest.raises(ValueError, match="`fixed` index -1 "):
        ParamMap(5, [-1])
    with pytest.raises(ValueError, match="boolean `fixed`"):
        ParamMap(5, [True, False])
    with pytest.raises(ValueError, match="`tied` key 7 "):
        ParamMap(5, None, {7: 1})
    with pytest.raises(ValueError, match="`tied` target 9 "):
        ParamMap(5, None, {1: 9})
    with pytest.raises(ValueError, match="key 2 is also fixed"):
        ParamMap(5, [2], {2: 1})
    with pytest.raises(ValueError, match=r"target 1 \(of parameter 2\) is fixed"):
        ParamMap(5, [1], {2: 1})
    with pytest.raises(ValueError, match=r"target 2 \(of parameter 3\) is itself tied to 1"):
        ParamMap(5, None, {2: 1, 3: 2})
    with pytest.raises(ValueError, match="parameter 3 to itself"):
        ParamMap(5, None, {3: 3})
    with pytest.raises(ValueError, match="nf = 0"):
        ParamMap(3, [0, 1, 2])
    with pytest.raises(ValueError, match="nf = 0"):
        ParamMap(3, np.ones(3, dtype=bool))


# ---- the numpy wrappers ---------------------------------------------------------------------------------------------
WRAP_CASES = [(name, mp) for name in pc.KERNEL_N for mp in pc.kernel_maps(name)]


@pytest.mark.parametrize("name,mp", WRAP_CASES, ids=["%s-%s" % (c[0], c[1][0]) for c in WRAP_CASES])
def test_wrapped_jac_against_central_differences_in_longdouble(name, mp):
    """reduce_jac(model.jac) (float64) against (g(x + h e_k) - g(x - h e_k)) / 2h of the wrapped f in np.longdouble,
    g(X) = f(expand_x(X, Pfix)): the figures of test_numpy_jac_against_central_differences_in_longdouble (h = 1e-6,
    truncation ~1e-11 for third derivatives below 1e2 — a tie of three members triples them at most —, 1e-9 of the
    column's largest entry allowed)."""
    _, fixed, tied = mp
    n = pc.KERNEL_N[name]
    pm = ParamMap(n, fixed, tied)
    B, m = 3, 17
    x, P = mc.case_inputs(name, n, B, m, seed=n)
    M = models.get(name)
    X = pm.reduce_x(P)
    g, dg = pm.wrap_f(M.f, P), pm.wrap_jac(M.jac, P)
    J = dg(x, X)
    assert J.shape == (B, m, pm.nf) and J.dtype == np.float64 and g(x, X).shape == (B, m)
    assert np.array_equal(J, pm.reduce_jac(M.jac(x, pm.expand_x(X, P))))
    gl = pm.wrap_f(M.f, P.astype(LD))
    xl, Xl = x.astype(LD), X.astype(LD)
    assert gl(xl, Xl).dtype == LD
    h = LD(1e-6)
    for k in range(pm.nf):
        Xp, Xm = Xl.copy(), Xl.copy()
        Xp[:, k] += h
        Xm[:, k] -= h
        col = (gl(xl, Xp) - gl(xl, Xm)) / (2 * h)
        err = np.max(np.abs(col - J[:, :, k]))
        assert float(err) <= 1e-9 * max(1.0, float(np.max(np.abs(col)))), (name, mp[0], k, float(err))


@pytest.mark.parametrize("case", pc.E2E_CASES, ids=pc.E2E_IDS)
def test_hand_written_reduced_models_are_the_wrapped_full_models(case):
    """The references of the end-to-end GPU test are independent of ParamMap; here they are held against it: same
    start, same box, f and jac to 1e-12 (they group the operations differently)."""
    label, fixed, tied, red, groups = case
    pr = pc.mapped_problem(label, 33, fixed, tied, groups)
    M = models.get(pr["name"])
    pm = ParamMap(pr["P0"].shape[1], fixed, tied)
    assert pm.nf == len(groups) and [pm.group(k).tolist() for k in range(pm.nf)] == groups
    assert np.array_equal(pm.reduce_x(pr["P0"]), pr["X0"])
    lo, hi = pm.reduce_bounds(*pr["bounds"])
    assert np.array_equal(lo, pr["bounds_red"][0]) and np.array_equal(hi, pr["bounds_red"][1])
    assert np.all((pr["X0"] > lo) & (pr["X0"] < hi))
    f, jac, single = pc.reduced_callables(red, pr["P0"])
    X = pr["X0"]
    np.testing.assert_allclose(f(pr["x"], X), pm.wrap_f(M.f, pr["P0"])(pr["x"], X), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(jac(pr["x"], X), pm.wrap_jac(M.jac, pr["P0"])(pr["x"], X), rtol=1e-12, atol=1e-12)
    fb, jb = single(2)
    np.testing.assert_array_equal(fb(pr["x"], *X[2]), f(pr["x"], X)[2])
    np.testing.assert_array_equal(jb(pr["x"], *X[2]), jac(pr["x"], X)[2])
    for j, i in tied.items():
        assert np.array_equal(pr["truth"][:, j], pr["truth"][:, i])
    assert np.array_equal(pr["P0"][:, fixed], pr["truth"][:, fixed])


# ---- the keywords: checks that need neither the library nor a device ------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from bounded_lsq import _abi, _curve_fit

    def boom(*a, **k):
        raise AssertionError("a library or device call was reached")
    monkeypatch.setattr(_abi, "load", boom)
    monkeypatch.setattr(_abi.Context, "__init__", boom)
    monkeypatch.setattr(_curve_fit, "least_squares_batch", boom)
    monkeypatch.setattr(_curve_fit, "least_squares", boom)


@pytest.mark.parametrize("driver", ["host", "device"])
def test_curve_fit_batch_keyword_errors(no_library, driver):
    t = np.linspace(-2, 2, 12)
    Y = np.zeros((3, 12))
    P0 = np.ones((3, 7))

    def call(**kw):
        return bounded_lsq.curve_fit_batch("gauss_sum", t, Y, P0, driver=driver, **kw)
    with pytest.raises(ValueError, match="`fixed` index 7 "):
        call(fixed=[7])
    with pytest.raises(ValueError, match="key 5 is also fixed"):
        call(fixed=[5], tied={5: 2})
    with pytest.raises(ValueError, match="target 2 .* is fixed"):
        call(fixed=[2], tied={5: 2})
    with pytest.raises(ValueError, match="itself tied"):
        call(tied={5: 2, 2: 1})
    with pytest.raises(ValueError, match="to itself"):
        call(tied={5: 5})
    with pytest.raises(ValueError, match="nf = 0"):
        call(fixed=np.ones(7, dtype=bool))
    lb, ub = np.full(7, -5.0), np.full(7, 5.0)
    lb[2], ub[5] = 1.0, 0.5
    with pytest.raises(ValueError, match=r"\[2, 5\] do not intersect"):
        call(tied={5: 2}, bounds=(lb, ub))
    with pytest.raises(ValueError, match="does not take n"):                   # n is still the model's
        bounded_lsq.curve_fit_batch("gauss_sum", t, Y, np.ones((3, 6)), driver=driver, fixed=[0])


def test_curve_fit_keyword_errors(no_library):
    x = np.linspace(0, 1, 9)

    def f(x, a, b, c):
        return a * x * x + b * x + c
    with pytest.raises(ValueError, match="`p0` is required"):
        bounded_lsq.curve_fit(f, x, x, fixed=[0])
    with pytest.raises(ValueError, match="`p0` is required"):
        bounded_lsq.curve_fit(f, x, x, tied={1: 0})
    with pytest.raises(ValueError, match="`fixed` index 3 "):
        bounded_lsq.curve_fit(f, x, x, p0=[1, 1, 1], fixed=[3])
    with pytest.raises(ValueError, match="nf = 0"):
        bounded_lsq.curve_fit(f, x, x, p0=[1, 1, 1], fixed=[0, 1, 2])
    with pytest.raises(ValueError, match="do not intersect"):
        bounded_lsq.curve_fit(f, x, x, p0=[1, 1, 1], tied={1: 0}, bounds=([0, 2, 0], [1, 3, 1]))


def _capture(monkeypatch, what="least_squares_batch"):
    from bounded_lsq import _curve_fit
    seen = {}

    class Stop(Exception):
        pass

    def fake(fun, x0, jac=None, **kw):
        seen.update(fun=fun, x0=np.asarray(x0), jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, what, fake)
    return seen, Stop


def test_what_the_keywords_hand_to_the_batch_solver(monkeypatch):
    """nf-wide start and bounds; driver='device' with a name: a DeviceFit carrying the map and the template, its `n`
    the number of solver variables; otherwise numpy callables over the nf variables that show the user's function all
    n columns."""
    seen, Stop = _capture(monkeypatch)
    x, P = mc.case_inputs("gauss_sum", 7, 2, 8)
    M = models.get("gauss_sum")
    Y = M.f(x, P) + 0.25
    lb, ub = P - 1.0, P + 1.0
    lb[:, 5] += 0.5
    kw = dict(fixed=[1, 4], tied={5: 2}, bounds=(lb, ub))
    X0 = P[:, [0, 2, 3, 6]]
    Pfull = P.copy()
    Pfull[:, 5] = P[:, 2]
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, sigma=0.5, driver="device", **kw)
    fit = seen["fun"]
    assert isinstance(fit, models.DeviceFit) and seen["jac"] is None
    assert (fit.B, fit.m, fit.n, fit.n_model) == (2, 8, 4, 7)
    assert fit.param_map.pmap.tolist() == [0, -1, 1, 2, -1, 1, 3] and np.array_equal(fit.Pfix, P)
    assert np.array_equal(seen["x0"], X0)
    rlb, rub = seen["kw"]["bounds"]
    assert np.array_equal(rlb, np.stack([lb[:, 0], np.maximum(lb[:, 2], lb[:, 5]), lb[:, 3], lb[:, 6]], axis=1))
    assert np.array_equal(rub, np.stack([ub[:, 0], np.minimum(ub[:, 2], ub[:, 5]), ub[:, 3], ub[:, 6]], axis=1))
    assert seen["kw"]["_variance_scale"] is True
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, jac="3-point", driver="device", **kw)
    assert isinstance(seen["fun"], models.DeviceFit) and seen["jac"] == "3-point" and seen["fun"].n == 4
    # the name on the host driver: the numpy functions, wrapped and weighted
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x, Y, P, sigma=0.5, driver="host", **kw)
    np.testing.assert_array_equal(seen["fun"](X0), 2.0 * (M.f(x, Pfull) - Y))
    J = M.jac(x, Pfull)
    Jr = np.stack([J[:, :, 0], J[:, :, 2] + J[:, :, 5], J[:, :, 3], J[:, :, 6]], axis=2)
    np.testing.assert_array_equal(seen["jac"](X0), 2.0 * Jr)
    # user callables see all n columns
    widths = []

    def uf(xd, Pq):
        widths.append(Pq.shape)
        assert np.array_equal(Pq[:, 5], Pq[:, 2]) and np.array_equal(Pq[:, [1, 4]], P[:, [1, 4]])
        return M.f(xd, Pq)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(uf, x, Y, P, jac=M.jac, **kw)
    np.testing.assert_array_equal(seen["fun"](X0), M.f(x, Pfull) - Y)
    np.testing.assert_array_equal(seen["jac"](X0), Jr)
    assert widths == [(2, 7)] and seen["x0"].shape == (2, 4)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(uf, x, Y, P, **kw)
    assert seen["jac"] == "2-point" and seen["x0"].shape == (2, 4)
    # m <= nf decides the variance factor, not m <= n: m = 8 > nf = 4 above; without the map n = 7 < 8 too, so take
    # six fixed parameters of a problem with m = 5 rows
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x[:5], Y[:, :5], P, driver="device", fixed=[0, 1, 2, 3, 4, 5])
    assert seen["kw"]["_variance_scale"] is True and seen["fun"].n == 1
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch("gauss_sum", x[:5], Y[:, :5], P, driver="device")
    assert seen["kw"]["_variance_scale"] is False


def test_empty_keywords_hand_on_what_no_keywords_hand_on(monkeypatch):
    seen, Stop = _capture(monkeypatch)
    x, P = mc.case_inputs("exp_sum", 5, 2, 8)
    Y = models.get("exp_sum").f(x, P)
    for kw in ({}, dict(fixed=[], tied={}), dict(fixed=None, tied=None), dict(fixed=np.zeros(5, dtype=bool))):
        with pytest.raises(Stop):
            bounded_lsq.curve_fit_batch("exp_sum", x, Y, P, driver="device", **kw)
        fit = seen["fun"]
        assert fit.param_map is None and (fit.n, fit.n_model) == (5, 5) and seen["x0"].shape == (2, 5)
        assert seen["kw"]["bounds"] == (-np.inf, np.inf)


def test_what_the_keywords_hand_to_least_squares(monkeypatch):
    """curve_fit: p0 and bounds of the nf variables; the user's f(xdata, *params) receives all n."""
    seen, Stop = _capture(monkeypatch, "least_squares")
    x = np.linspace(0, 1, 9)
    got = []

    def f(x, a, b, c, d):
        got.append((a, b, c, d))
        return a * x ** 3 + b * x * x + c * x + d
    with pytest.raises(Stop):
        bounded_lsq.curve_fit(f, x, 2 * x, p0=[1.0, 2.0, 3.0, 4.0], fixed=[1], tied={3: 0},
                              bounds=([-5, 0, -6, -4], [5, 0, 6, 7]))
    assert seen["x0"].tolist() == [1.0, 3.0] and seen["jac"] == "2-point"
    assert np.array_equal(seen["kw"]["bounds"][0], [-4.0, -6.0]) and np.array_equal(seen["kw"]["bounds"][1], [5.0, 6.0])
    r = seen["fun"](np.array([0.5, -1.0]))
    assert got[-1] == (0.5, 2.0, -1.0, 0.5)
    np.testing.assert_array_equal(r, 0.5 * x ** 3 + 2.0 * x * x - x + 0.5 - 2 * x)
