"""What the batch and global fit front ends hand on, without a GPU and without the library.

Two parts.  The front-end grid drives ``curve_fit_batch`` and ``curve_fit_global`` over every combination of estimator,
``nan_policy``, `sigma` form, named model or callables and parameter map with ``least_squares_batch`` replaced by a spy,
and holds what the spy receives bit for bit to an explicit composition of the definitions (the methods of ``ParamMap`` /
``GlobalMap``, ``models.poisson_transform``, ``models.omit_residual`` / ``omit_jacobian``, ``1 / sigma``); on the
device route it holds the ``DeviceFit`` and the keywords it was built with.  The ``DeviceModel`` recording builds
``DeviceModel`` on a context that records what is uploaded and what every ``blsq_model_eval*_dev`` entry is called with,
and holds both to the argument lists of include/blsq.h."""
import ctypes

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import GlobalMap, ParamMap, _abi, _curve_fit, models

MODEL = "gauss_sum"                              # a, mu, s, c: positive wherever a, c > 0
N = 4
B, MB = 3, 7                                     # the batch: B problems of MB points
G, S, MG = 3, 2, 6                               # the global fits: G groups of S data sets of MG points
MAPS = {"none": (None, None), "fixed_tied": ([3], {2: 1}), "affine": (None, {2: (1, 2.0, 0.5)})}
SIGMAS = ("none", "scalar", "m", "per")
# estimator, sigma form: under Poisson `sigma` must be None
EST_SIGMA = [("lse", s) for s in SIGMAS] + [("poisson", "none")]


class Stop(Exception):
    pass


@pytest.fixture
def spy(monkeypatch):
    """``least_squares_batch`` and ``DeviceFit`` as `_curve_fit` looks them up: the first records and stops, the second
    records its arguments and builds the real object."""
    seen = {"made": []}

    def solve(fun, x0, jac, **kw):
        seen.update(fun=fun, x0=x0, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, "least_squares_batch", solve)
    real = models.DeviceFit
    monkeypatch.setattr(_curve_fit._models, "DeviceFit", lambda *a, **k: (seen["made"].append((a, k)), real(*a, **k))[1])
    seen["DeviceFit"] = real
    return seen


def _problem(lead, m, omit, sigma_kind):
    """x, Y, P0, bounds and sigma for problems of leading shape `lead`; with `omit` three entries of Y are NaN and a
    per-problem sigma holds NaN there (anything may stand at an omitted point)."""
    rng = np.random.default_rng(11)
    P0 = np.empty(lead + (N,))
    P0[..., 0], P0[..., 1], P0[..., 2], P0[..., 3] = 3.0, rng.uniform(0.3, 0.6, lead), 1.0, 0.5
    Y = rng.uniform(1.0, 4.0, lead + (m,))
    if omit:
        Y[(0,) * len(lead) + (slice(0, 2),)] = np.nan
        Y[(-1,) * len(lead) + (m - 1,)] = np.nan
    sigma = {"none": None, "scalar": 0.5, "m": rng.uniform(0.5, 2.0, m),
             "per": rng.uniform(0.5, 2.0, lead + (m,))}[sigma_kind]
    if omit and sigma_kind == "per":
        sigma[np.isnan(Y)] = np.nan
    return Y, P0, (P0 - 1.0, P0 + 1.0), sigma


def _weights(sigma, sigma_kind, omitted):
    """1 / sigma, with 1 in the place of a per-problem sigma at an omitted point."""
    if sigma is None:
        return None
    s = np.asarray(sigma, dtype=float)
    if sigma_kind == "per" and omitted is not None:
        s = np.where(omitted, 1.0, s)
    return 1.0 / s


def _residual_and_jacobian(mu, Jm, Yrows, w, poisson, omit):
    """The definition, in its order: sigma or the Poisson transform on the mapped model, the omission outermost."""
    if poisson:
        r, c = models.poisson_transform(mu, Yrows)
        J = c[:, :, np.newaxis] * Jm
    else:
        r, J = mu - Yrows, Jm
        if w is not None:
            r, J = w * r, np.broadcast_to(w, Yrows.shape)[:, :, np.newaxis] * J
    if omit:
        r, J = models.omit_residual(lambda: r, Yrows)(), models.omit_jacobian(lambda: J, Yrows)()
    return r, J


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _check_common(seen, driver, X0, bounds_ref, nobs_ref, rows, nv):
    kw = seen["kw"]
    assert _same(seen["x0"], X0)
    assert len(kw["bounds"]) == 2 and _same(kw["bounds"][0], bounds_ref[0]) and _same(kw["bounds"][1], bounds_ref[1])
    if nobs_ref is None:
        assert "_nobs" not in kw
    else:
        assert kw["_nobs"].dtype == np.int32 and np.array_equal(kw["_nobs"], nobs_ref)
    assert kw["_variance_scale"] is (rows > nv)
    assert kw["covariance"] == "pinv" and kw["driver"] == driver and kw["method"] == "trf" and kw["ctx"] is None
    assert kw["max_nfev"] is None
    assert set(kw) - {"_nobs"} == {"bounds", "method", "driver", "ctx", "covariance", "_variance_scale", "max_nfev"}


def _batch_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, est, omit, x):
    M = models.get(MODEL)
    fixed, tied = MAPS[mapkind]
    pm = None if mapkind == "none" else ParamMap(N, fixed, tied)
    X0 = P0 if pm is None else pm.reduce_x(P0)
    P = P0 if pm is None else pm.expand_x(X0, P0)
    Jm = M.jac(x, P) if pm is None else pm.reduce_jac(M.jac(x, P))
    omitted = np.isnan(Y) if omit else None
    r, J = _residual_and_jacobian(M.f(x, P), Jm, Y, _weights(sigma, sigma_kind, omitted), est == "poisson", omit)
    bounds_ref = bounds if pm is None else pm.reduce_bounds(*bounds)
    nobs = np.sum(~np.isnan(Y), axis=1).astype(np.int32) if omit else None
    return pm, X0, r, J, bounds_ref, nobs


def _global_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, shared, est, omit, xs):
    M = models.get(MODEL)
    fixed, tied = MAPS[mapkind]
    gm = GlobalMap(N, S, shared, fixed, tied)
    X0 = gm.reduce_x(P0)
    P = gm.expand_x(X0, P0).reshape(-1, N)
    xrows = np.broadcast_to(xs, (G, S, MG)).reshape(G * S, MG)
    mu = M.f(xrows, P).reshape(G, S * MG)
    Jm = gm.reduce_jac(M.jac(xrows, P).reshape(G, S, MG, N))
    omitted = np.isnan(Y) if omit else None
    w = _weights(sigma, sigma_kind, omitted)
    if w is not None and w.ndim:                 # (m,) / (G, S, m) -> along the S m rows of a group
        w = np.broadcast_to(w, (G, S, MG)).reshape(G, S * MG)
    r, J = _residual_and_jacobian(mu, Jm, Y.reshape(G, S * MG), w, est == "poisson", omit)
    nobs = np.sum(~np.isnan(Y.reshape(G, -1)), axis=1).astype(np.int32) if omit else None
    return gm, X0, r, J, gm.reduce_bounds(*bounds), nobs


def _shared_choices(mapkind):
    """Everything that is free shared (nl = 0), and a mixed choice."""
    fixed, tied = MAPS[mapkind]
    return {"all": [int(j) for j in ParamMap(N, fixed, tied).leaders], "mixed": [1]}


# ---- the front-end grid ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("callables", [False, True], ids=["named", "callable"])
@pytest.mark.parametrize("mapkind", list(MAPS))
@pytest.mark.parametrize("nan_policy", [None, "omit"])
@pytest.mark.parametrize("est,sigma_kind", EST_SIGMA)
def test_batch_host_routes(spy, est, sigma_kind, nan_policy, mapkind, callables):
    omit = nan_policy == "omit"
    x = np.linspace(-2.0, 2.0, MB)
    Y, P0, bounds, sigma = _problem((B,), MB, omit, sigma_kind)
    M = models.get(MODEL)
    fixed, tied = MAPS[mapkind]
    pm, X0, r, J, bounds_ref, nobs = _batch_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, est, omit, x)
    f, jac = (M.f, M.jac) if callables else (MODEL, None)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(f, x, Y, P0, sigma=sigma, bounds=bounds, jac=jac, fixed=fixed, tied=tied,
                                    estimator=est, nan_policy=nan_policy)
    _check_common(spy, "host", X0, bounds_ref, nobs, MB, X0.shape[1])
    assert not spy["made"]
    assert _same(spy["fun"](X0), r) and _same(spy["jac"](X0), J)
    if omit:
        assert not spy["fun"](X0)[np.isnan(Y)].view(np.int64).any()


@pytest.mark.parametrize("callables", [False, True], ids=["named", "callable"])
@pytest.mark.parametrize("mapkind,share", [(k, s) for k in MAPS for s in ("all", "mixed")])
@pytest.mark.parametrize("nan_policy", [None, "omit"])
@pytest.mark.parametrize("est,sigma_kind", EST_SIGMA)
def test_global_host_routes(spy, est, sigma_kind, nan_policy, mapkind, share, callables):
    omit = nan_policy == "omit"
    xs = np.stack([np.linspace(-2.0, 2.0, MG), np.linspace(-1.5, 2.5, MG)])       # one abscissa per data set
    Y, P0, bounds, sigma = _problem((G, S), MG, omit, sigma_kind)
    M = models.get(MODEL)
    fixed, tied = MAPS[mapkind]
    shared = _shared_choices(mapkind)[share]
    gm, X0, r, J, bounds_ref, nobs = _global_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, shared, est, omit, xs)
    assert (gm.nl == 0) == (share == "all")
    f, jac = (M.f, M.jac) if callables else (MODEL, None)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_global(f, xs, Y, P0, shared, sigma=sigma, bounds=bounds, jac=jac, fixed=fixed, tied=tied,
                                     estimator=est, nan_policy=nan_policy)
    _check_common(spy, "host", X0, bounds_ref, nobs, S * MG, gm.nv)
    assert not spy["made"]
    assert _same(spy["fun"](X0), r) and _same(spy["jac"](X0), J)


@pytest.mark.parametrize("front", ["batch", "global"])
def test_variance_scale_flag(spy, front):
    """``_variance_scale`` is ``not absolute_sigma and rows > nv``: off with `absolute_sigma`, off without a degree of
    freedom."""
    if front == "batch":
        def run(m, **kw):
            Y, P0, bounds, _ = _problem((B,), m, False, "none")
            with pytest.raises(Stop):
                bounded_lsq.curve_fit_batch(MODEL, np.linspace(-2.0, 2.0, m), Y, P0, **kw)
        m_small = N                               # m == n
    else:
        def run(m, **kw):
            Y, P0, bounds, _ = _problem((G, S), m, False, "none")
            with pytest.raises(Stop):
                bounded_lsq.curve_fit_global(MODEL, np.linspace(-2.0, 2.0, m), Y, P0, [1], **kw)
        m_small = 3                               # S m = 6 <= nv = 1 + 2 * 3
    run(6)
    assert spy["kw"]["_variance_scale"] is True
    run(6, absolute_sigma=True)
    assert spy["kw"]["_variance_scale"] is False
    run(m_small)
    assert spy["kw"]["_variance_scale"] is False
    run(6, maxfev=17)
    assert spy["kw"]["max_nfev"] == 17 and "maxfev" not in spy["kw"]


# ---- the device route: the DeviceFit and the keywords it was built with ------------------------------------------------
def _check_sigma_handed_on(got, sigma, sigma_kind, omitted):
    """`sigma` as given; at an omitted point of a per-problem `sigma` anything may stand."""
    if sigma is None:
        assert got is None
        return
    got, ref = np.asarray(got, dtype=float), np.asarray(sigma, dtype=float)
    if sigma_kind == "per" and omitted is not None:
        got, ref = np.where(omitted, 1.0, got), np.where(omitted, 1.0, ref)
    assert _same(got, ref)


@pytest.mark.parametrize("mapkind", list(MAPS))
@pytest.mark.parametrize("nan_policy", [None, "omit"])
@pytest.mark.parametrize("est,sigma_kind", EST_SIGMA)
def test_batch_device_route(spy, est, sigma_kind, nan_policy, mapkind):
    omit = nan_policy == "omit"
    x = np.linspace(-2.0, 2.0, MB)
    Y, P0, bounds, sigma = _problem((B,), MB, omit, sigma_kind)
    fixed, tied = MAPS[mapkind]
    pm, X0, _, _, bounds_ref, nobs = _batch_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, est, omit, x)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(MODEL, x, Y, P0, sigma=sigma, bounds=bounds, fixed=fixed, tied=tied, estimator=est,
                                    nan_policy=nan_policy, driver="device")
    _check_common(spy, "device", X0, bounds_ref, nobs, MB, X0.shape[1])
    assert spy["jac"] is None and len(spy["made"]) == 1
    (args, kw), fit = spy["made"][0], spy["fun"]
    omitted = np.isnan(Y) if omit else None
    assert len(args) == 5 and args[:2] == (MODEL, N) and _same(args[2], x) and _same(args[3], Y)
    _check_sigma_handed_on(args[4], sigma, sigma_kind, omitted)
    assert set(kw) == ({"param_map", "Pfix"} | ({"estimator"} if est == "poisson" else set())
                       | ({"nan_policy"} if omit else set()))
    assert kw.get("estimator", "poisson") == "poisson" and kw.get("nan_policy", "omit") == "omit"
    assert isinstance(fit, spy["DeviceFit"]) and fit.model is models.get(MODEL)
    assert (fit.B, fit.m, fit.n, fit.n_model) == (B, MB, X0.shape[1], N)
    assert fit.global_map is None and fit.binned is False
    assert fit.estimator == est and fit.nan_policy == ("omit" if omit else "propagate")
    assert _same(fit.xdata, x) and _same(fit.ydata, Y) and fit.ydata.flags.c_contiguous
    _check_sigma_handed_on(fit.sigma, sigma, sigma_kind, omitted)
    if pm is None:
        assert kw["param_map"] is None and kw["Pfix"] is None and fit.param_map is None and fit.Pfix is None
    else:
        assert fit.param_map is kw["param_map"] and _same(kw["Pfix"], P0) and _same(fit.Pfix, P0)
        assert _same(fit.param_map.pmap, pm.pmap) and _same(fit.param_map.ratio, pm.ratio)
        assert _same(fit.param_map.offset, pm.offset)


def test_batch_device_route_binned(spy):
    Y, P0, bounds, _ = _problem((B,), MB, False, "none")
    edges = np.linspace(-2.0, 2.0, MB + 1)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(MODEL, edges, Y, P0, driver="device", binned=True)
    (args, kw), fit = spy["made"][0], spy["fun"]
    assert set(kw) == {"param_map", "Pfix", "binned"} and kw["binned"] is True and fit.binned is True
    assert _same(args[2], models.bin_rows(edges)) and _same(fit.xdata, models.bin_rows(edges))


@pytest.mark.parametrize("mapkind,share", [(k, s) for k in MAPS for s in ("all", "mixed")])
@pytest.mark.parametrize("nan_policy", [None, "omit"])
@pytest.mark.parametrize("est,sigma_kind", EST_SIGMA)
def test_global_device_route(spy, est, sigma_kind, nan_policy, mapkind, share):
    omit = nan_policy == "omit"
    xs = np.stack([np.linspace(-2.0, 2.0, MG), np.linspace(-1.5, 2.5, MG)])
    Y, P0, bounds, sigma = _problem((G, S), MG, omit, sigma_kind)
    fixed, tied = MAPS[mapkind]
    shared = _shared_choices(mapkind)[share]
    gm, X0, _, _, bounds_ref, nobs = _global_reference(Y, P0, bounds, sigma, sigma_kind, mapkind, shared, est, omit, xs)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_global(MODEL, xs, Y, P0, shared, sigma=sigma, bounds=bounds, fixed=fixed, tied=tied,
                                     estimator=est, nan_policy=nan_policy, driver="device")
    _check_common(spy, "device", X0, bounds_ref, nobs, S * MG, gm.nv)
    assert spy["jac"] is None and len(spy["made"]) == 1
    (args, kw), fit = spy["made"][0], spy["fun"]
    omitted = np.isnan(Y) if omit else None
    assert len(args) == 5 and args[:2] == (MODEL, N) and _same(args[2], xs) and _same(args[3], Y)
    _check_sigma_handed_on(args[4], sigma, sigma_kind, omitted)
    assert set(kw) == ({"global_map", "Pfix"} | ({"estimator"} if est == "poisson" else set())
                       | ({"nan_policy"} if omit else set()))
    assert kw.get("estimator", "poisson") == "poisson" and kw.get("nan_policy", "omit") == "omit"
    assert isinstance(fit, spy["DeviceFit"]) and fit.model is models.get(MODEL)
    assert (fit.B, fit.m, fit.n, fit.n_model) == (G, S * MG, gm.nv, N)
    assert fit.param_map is None and fit.binned is False
    assert fit.estimator == est and fit.nan_policy == ("omit" if omit else "propagate")
    assert _same(fit.xdata, xs) and _same(fit.ydata, Y) and fit.ydata.shape == (G, S, MG)
    _check_sigma_handed_on(fit.sigma, sigma, sigma_kind, omitted)
    assert _same(kw["Pfix"], P0) and _same(fit.Pfix, P0)
    assert fit.global_map is kw["global_map"] and isinstance(fit.global_map, GlobalMap)
    assert _same(fit.global_map.cols, gm.cols) and _same(fit.global_map.pm.pmap, gm.pm.pmap)
    assert _same(fit.global_map.pm.ratio, gm.pm.ratio) and _same(fit.global_map.pm.offset, gm.pm.offset)


# ---- the DeviceModel recording -----------------------------------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("blsq_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class _Token:
    def __init__(self, array):
        self.array = array


class RecordingContext:
    """What ``DeviceModel`` needs of a context: uploads become tokens that keep a copy of the array."""

    def __init__(self):
        self.h, self.lib = object(), _Lib()
        self.tokens, self.freed, self.adopted, self.checked = [], [], [], []

    def to_device(self, a):
        a = np.asarray(a)
        assert a.flags.c_contiguous
        self.tokens.append(_Token(a.copy()))
        return self.tokens[-1]

    def free(self, p):
        self.freed.append(p)

    def adopt(self, obj):
        self.adopted.append(obj)

    def check(self, rc, what=""):
        self.checked.append((rc, what))
        assert rc == 0


def _host_array(p, ctype, count):
    """The `count` numbers behind a host pointer argument."""
    assert p is not None
    return np.array(ctypes.cast(p, ctypes.POINTER(ctype))[:count])


# the argument runs of the entries (include/blsq.h): the number of flags (est, sampling, nan_policy) in front, then the
# model id, the component table (ncomp, fam, cnt), the run of S (S, shared, t_sstride), nf / pmap / Pfix, the tie pair
LAYOUT = {
    "blsq_model_eval_dev": dict(flags=0, model=True, table=False, S=False, mapped=False, tie=False),
    "blsq_model_eval_map_dev": dict(flags=0, model=True, table=False, S=False, mapped=True, tie=False),
    "blsq_model_eval_comp_dev": dict(flags=0, model=False, table=True, S=False, mapped=True, tie=False),
    "blsq_model_eval_est_dev": dict(flags=1, model=True, table=True, S=False, mapped=True, tie=False),
    "blsq_model_eval_bin_dev": dict(flags=2, model=True, table=True, S=False, mapped=True, tie=False),
    "blsq_model_eval_nan_dev": dict(flags=3, model=True, table=True, S=False, mapped=True, tie=False),
    "blsq_model_eval_global_dev": dict(flags=3, model=True, table=True, S=True, mapped=True, tie=False),
    "blsq_model_eval_tie_dev": dict(flags=3, model=True, table=True, S=True, mapped=True, tie=True),
}


def _case(name, entry, model=MODEL, m=6, x="m", sigma="none", fixed=None, tied=None, estimator="lse", binned=False,
          omit=False, shared=None, pfix=True):
    return pytest.param(dict(entry=entry, model=model, m=m, x=x, sigma=sigma, fixed=fixed, tied=tied,
                             estimator=estimator, binned=binned, omit=omit, shared=shared, pfix=pfix), id=name)


CASES = [
    _case("plain", "blsq_model_eval_dev", sigma="scalar"),
    _case("plain_per_problem", "blsq_model_eval_dev", m=7, x="per", sigma="per"),
    _case("mapped", "blsq_model_eval_map_dev", m=7, x="per", sigma="m", fixed=[3], tied={2: 1}),
    _case("mapped_tie_only_no_Pfix", "blsq_model_eval_map_dev", tied={2: 1}, pfix=False),
    _case("composite", "blsq_model_eval_comp_dev", model="gauss+poly*1", m=8, sigma="per"),
    _case("composite_mapped", "blsq_model_eval_comp_dev", model="gauss+poly*1", fixed=[0]),
    _case("poisson", "blsq_model_eval_est_dev", m=9, estimator="poisson"),
    _case("poisson_composite_mapped", "blsq_model_eval_est_dev", model="gauss+poly*1", estimator="poisson", fixed=[3]),
    _case("binned_edges", "blsq_model_eval_bin_dev", x="edges", binned=True, sigma="m"),
    _case("binned_rows_poisson", "blsq_model_eval_bin_dev", m=7, x="rows_per", binned=True, estimator="poisson"),
    _case("omit", "blsq_model_eval_nan_dev", m=9, sigma="per", omit=True),
    _case("omit_binned_poisson_mapped", "blsq_model_eval_nan_dev", x="edges", binned=True, estimator="poisson",
          omit=True, fixed=[3]),
    _case("global_m", "blsq_model_eval_global_dev", x="m", sigma="m", shared=[1, 2]),
    _case("global_Sm", "blsq_model_eval_global_dev", x="set", sigma="set", shared=[1], fixed=[3], tied={2: 1}, omit=True),
    _case("global_GSm", "blsq_model_eval_global_dev", x="per", sigma="per", shared=[0, 1, 2, 3], omit=True,
          pfix=False),
    _case("global_scalar_poisson", "blsq_model_eval_global_dev", model="gauss+poly*1", shared=[1, 2],
          estimator="poisson"),
    _case("affine_batch", "blsq_model_eval_tie_dev", m=7, x="per", sigma="scalar", tied={2: (1, 2.0, 0.5)}),
    _case("affine_batch_all_flags", "blsq_model_eval_tie_dev", model="gauss+poly*1", x="edges", binned=True,
          estimator="poisson", omit=True, fixed=[3], tied={2: (1, -2.0)}),
    _case("affine_global", "blsq_model_eval_tie_dev", x="set", sigma="per", shared=[1],
          tied={2: (1, 2.0, 0.5)}, omit=True),
]


@pytest.mark.parametrize("c", CASES)
def test_device_model_uploads_and_arguments(c):
    glob = c["shared"] is not None
    lead = (G, S) if glob else (B,)
    nprob, sets, m = lead[0], (S if glob else 1), c["m"]
    rng = np.random.default_rng(5)
    model = models.resolve(c["model"])
    comp = isinstance(model, models.CompositeModel)
    coords = model.coords
    # ---- the inputs and, next to each, what must reach the device
    grid = np.linspace(-2.0, 2.0, m)
    if c["x"] == "m":
        x, t_ref, t_stride, t_sstride = grid, grid, 0, 0
    elif c["x"] == "set":                        # (S, m): global only
        x = np.stack([grid + 0.25 * s for s in range(S)])
        t_ref, t_stride, t_sstride = x, 0, m
    elif c["x"] == "per":
        x = grid + 0.25 * rng.uniform(size=lead + (m,))
        t_ref, t_stride, t_sstride = x, sets * m, (m if glob else 0)
    elif c["x"] == "edges":
        x = np.linspace(-2.0, 2.0, m + 1)
        t_ref, t_stride, t_sstride = np.stack([x[:-1], x[1:]]), 0, 0
    else:                                        # rows (B, 2, m) of bins with gaps
        lo = grid + 0.25 * rng.uniform(size=(B, m))
        x = np.stack([lo, lo + 0.1], axis=1)
        t_ref, t_stride, t_sstride = x, 2 * coords * m, 0
    Y = rng.uniform(1.0, 4.0, lead + (m,))
    if c["omit"]:
        Y[(0,) * len(lead) + (slice(0, 2),)] = np.nan
        Y[(-1,) * len(lead) + (m - 1,)] = np.nan
    omitted = np.isnan(Y)
    if c["sigma"] == "none":
        sigma, w_ref, w_stride = None, None, 0
    elif c["sigma"] == "scalar":
        sigma, w_ref, w_stride = 0.5, np.full(m, 1.0 / 0.5), 0
    elif c["sigma"] == "m":
        sigma = rng.uniform(0.5, 2.0, m)
        w_ref, w_stride = 1.0 / sigma, 0
    else:                                        # per problem: (S, m) or lead + (m,); anything at an omitted point
        sigma = rng.uniform(0.5, 2.0, (S, m) if c["sigma"] == "set" else lead + (m,))
        filled = np.where(omitted, 1.0, np.broadcast_to(sigma, lead + (m,)))
        if c["sigma"] == "per" and c["omit"]:
            sigma[omitted] = np.nan
        w_ref, w_stride = (1.0 / filled).reshape(nprob, sets * m), sets * m
    P0 = rng.uniform(0.5, 1.5, lead + (N,))
    pm = ParamMap(N, c["fixed"], c["tied"]) if (c["fixed"] or c["tied"] or glob) else None
    gm = GlobalMap(N, S, c["shared"], c["fixed"], c["tied"]) if glob else None
    width = gm.nv if glob else (N if pm is None else pm.nf)
    # ---- build it
    ctx = RecordingContext()
    kw = dict(estimator=c["estimator"], binned=c["binned"], nan_policy="omit" if c["omit"] else "propagate")
    Pfix = P0 if (pm is not None and c["pfix"]) else None
    if glob:
        dm = models.DeviceModel(ctx, c["model"], G, m, N, x, Y, sigma, None, Pfix, global_map=gm, **kw)
    else:
        dm = models.DeviceModel(ctx, c["model"], B, m, N, x, Y, sigma, pm, Pfix, **kw)
    assert ctx.adopted == [dm]
    assert (dm.B, dm.m, dm.n, dm.n_model) == (nprob, sets * m, width, N)
    assert dm.param_map is (None if glob else pm) and dm.global_map is gm
    assert (dm.estimator, dm.binned, dm.nan_policy) == (kw["estimator"], kw["binned"], kw["nan_policy"])
    uploads = [t_ref, Y.reshape(nprob, sets * m)] + ([w_ref] if w_ref is not None else [])
    uploads += [P0] if Pfix is not None else []
    assert len(ctx.tokens) == len(uploads)
    for tok, ref in zip(ctx.tokens, uploads):
        assert tok.array.dtype == np.float64 and _same(tok.array, np.asarray(ref, dtype=np.float64))
    d_t, d_y = ctx.tokens[0], ctx.tokens[1]
    d_w = ctx.tokens[2] if w_ref is not None else None
    d_Pfix = ctx.tokens[-1] if Pfix is not None else None
    lb, ub = dm.set_bounds(-1.0, np.arange(1.0, width + 1.0))
    assert dm.bounds_dev == (lb, ub) and ctx.tokens[-2:] == [lb, ub]
    assert _same(lb.array, np.full((nprob, width), -1.0))
    assert _same(ub.array, np.broadcast_to(np.arange(1.0, width + 1.0), (nprob, width)))
    # ---- the two callbacks
    d_x, d_f, d_J, d_mask = object(), object(), object(), object()
    dm.fun_dev(d_x, d_f, 3)
    dm.jac_dev(d_x, d_J, d_mask)
    dm.jac_dev(d_x, d_J)
    dm.fun_dev(d_x, d_f)
    L = LAYOUT[c["entry"]]
    tails = [(3, d_f, None, None), (1, None, d_J, d_mask), (1, None, d_J, None), (1, d_f, None, None)]
    assert [name for name, _ in ctx.lib.calls] == [c["entry"]] * 4
    assert ctx.checked == [(0, c["entry"])] * 4
    for (name, args), (reps, f_ptr, J_ptr, mask_ptr) in zip(ctx.lib.calls, tails):
        assert len(args) - 1 == len(_abi.SIGNATURES[name][1]) - 1        # every argument behind ctx
        a = list(args)
        assert a.pop(0) is ctx.h
        flags = [models.ESTIMATORS.index(c["estimator"]), int(c["binned"]), int(c["omit"])]
        for k in range(L["flags"]):
            assert a.pop(0) == flags[k]
        assert flags[L["flags"]:] == [0] * (3 - L["flags"])          # a flag the entry does not take is not set
        if L["model"]:
            assert a.pop(0) == (-1 if comp else model.id)
        else:
            assert comp
        if L["table"]:
            ncomp, fam, cnt = a.pop(0), a.pop(0), a.pop(0)
            if comp:
                assert ncomp == len(model.components)
                assert _host_array(fam, ctypes.c_int32, ncomp).tolist() == model.fam_ids.tolist()
                assert _host_array(cnt, ctypes.c_int32, ncomp).tolist() == model.counts.tolist()
            else:
                assert (ncomp, fam, cnt) == (0, None, None)
        else:
            assert not comp
        if L["S"]:
            s_arg, shared_arg, sstride_arg = a.pop(0), a.pop(0), a.pop(0)
            if glob:
                assert s_arg == S and sstride_arg == t_sstride
                assert _host_array(shared_arg, ctypes.c_int32, gm.nf).tolist() == gm.slot_shared.astype(int).tolist()
            else:
                assert (s_arg, shared_arg, sstride_arg) == (0, None, 0)
        else:
            assert not glob
        assert [a.pop(0) for _ in range(4)] == [nprob, reps, m, N]               # B (G), reps, m per data set, n
        if L["mapped"]:
            nf_arg, pmap_arg = a.pop(0), a.pop(0)
            if pm is None:
                assert (nf_arg, pmap_arg) == (N, None)
            else:
                assert nf_arg == pm.nf and _host_array(pmap_arg, ctypes.c_int32, N).tolist() == pm.pmap.tolist()
        else:
            assert pm is None
        if L["tie"]:
            assert _host_array(a.pop(0), ctypes.c_double, N).tolist() == pm.ratio.tolist()
            assert _host_array(a.pop(0), ctypes.c_double, N).tolist() == pm.offset.tolist()
        else:
            assert pm is None or not pm.affine
        assert a.pop(0) is d_t and a.pop(0) == t_stride
        assert a.pop(0) is d_y and a.pop(0) is d_w and a.pop(0) == w_stride
        assert a.pop(0) is d_x
        if L["mapped"]:
            assert a.pop(0) is d_Pfix
        assert a == [f_ptr, J_ptr, mask_ptr]
        for v in args[1:]:                                                # scalars are Python ints
            assert v is None or not isinstance(v, (float, np.generic))
    # ---- close() frees every buffer once
    dm.close()
    assert len(ctx.freed) == len(ctx.tokens) and {id(p) for p in ctx.freed} == {id(p) for p in ctx.tokens}
    dm.close()
    assert len(ctx.freed) == len(ctx.tokens) and dm.bounds_dev is None


def test_device_model_prediction_has_no_y_and_no_weights():
    """y = None, sigma = None (``models.evaluate``): one upload, NULL for y and w."""
    ctx = RecordingContext()
    x = np.linspace(-2.0, 2.0, 6)
    dm = models.DeviceModel(ctx, MODEL, B, 6, N, x)
    d_x, d_f = object(), object()
    dm.fun_dev(d_x, d_f, 1)
    (name, args), = ctx.lib.calls
    assert name == "blsq_model_eval_dev" and len(ctx.tokens) == 1 and _same(ctx.tokens[0].array, x)
    assert list(args[1:]) == [models.get(MODEL).id, B, 1, 6, N, ctx.tokens[0], 0, None, None, 0, d_x, d_f, None, None]


def test_device_fit_opens_the_same_device_model():
    """``DeviceFit.open_device``: the model the front end described, with the bounds uploaded (B, n)."""
    x = np.linspace(-2.0, 2.0, MG)
    Y, P0, _, sigma = _problem((G, S), MG, True, "per")
    gm = GlobalMap(N, S, [1], [3], {2: (1, 2.0, 0.5)})
    fit = models.DeviceFit(MODEL, N, x, Y, sigma, Pfix=P0, global_map=gm, nan_policy="omit")
    ctx = RecordingContext()
    dm = fit.open_device(ctx, -np.ones(gm.nv), np.ones((G, gm.nv)))
    assert (dm.B, dm.m, dm.n, dm.n_model, dm.nan_policy) == (G, S * MG, gm.nv, N, "omit")
    assert [t.array.shape for t in ctx.tokens] == [(MG,), (G, S * MG), (G, S * MG), (G, S, N), (G, gm.nv), (G, gm.nv)]
    assert _same(ctx.tokens[2].array, (1.0 / np.where(np.isnan(Y), 1.0, sigma)).reshape(G, S * MG))
    dm.fun_dev(None, None, 2)
    assert ctx.lib.calls[0][0] == "blsq_model_eval_tie_dev"
    Yb, P0b, _, sb = _problem((B,), MB, False, "m")
    pm = ParamMap(N, [3], {2: 1})
    fit = models.DeviceFit(MODEL, N, np.linspace(-2.0, 2.0, MB), Yb, sb, param_map=pm, Pfix=P0b, estimator="lse")
    ctx = RecordingContext()
    dm = fit.open_device(ctx, -1.0, 1.0)
    assert (dm.B, dm.m, dm.n, dm.n_model, dm.param_map) == (B, MB, pm.nf, N, pm)
    assert [t.array.shape for t in ctx.tokens] == [(MB,), (B, MB), (MB,), (B, N), (B, pm.nf), (B, pm.nf)]
    dm.jac_dev(None, None)
    assert ctx.lib.calls[0][0] == "blsq_model_eval_map_dev"
