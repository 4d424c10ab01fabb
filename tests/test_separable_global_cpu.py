"""Separable global fits without a GPU: the layout and the rejections, the gradient identity of Kaufman's
Jacobian of a group against central differences in np.longdouble, ``separable_global_cov`` against the dense inverse of
the full group's J^T J built by explicit loops in np.longdouble (cap 64 kappa_2(J^T J) eps relative to the block's largest
entry), the front end with the solve stubbed, and scipy's convergence on every fit case of the GPU tests."""
import types
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _curve_fit, models
from bounded_lsq._varpro import _HostGlobalStage

import _separable_global_cases as gc

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def small(spec, S, shared, m=16, G=2, seed=0, with_sigma=False, dtype=np.float64):
    """(x, Y (G, S, m), sigma, X (G, nv), gm, lin, owner, non, n) of a small group near a sensible point."""
    truth = {"exp*2+poly*1": [3.0, 0.7, 1.5, 3.1, 0.2], "gauss+poly*1": [2.0, 0.2, 0.4, 0.3]}[spec]
    rng = np.random.default_rng(seed)
    n = len(truth)
    x = np.linspace(0.0, 3.0, m) if spec.startswith("exp") else np.linspace(-1.5, 1.5, m)
    P = np.tile(np.array(truth), (G, S, 1))
    lin, owner = models.linear_params(spec, n)
    P[..., lin] *= 1.0 + 0.3 * rng.uniform(-1, 1, (G, S, lin.size))
    Y = models.resolve(spec).f(x, P.reshape(G * S, n)).reshape(G, S, m) + 0.05 * rng.standard_normal((G, S, m))
    sigma = rng.uniform(0.5, 2.0, (G, S, m)) if with_sigma else None
    gm, lin, owner, non = models.separable_global_map(spec, n, S, shared)
    X = gm.reduce_x(1.05 * P[..., non] + 0.02 * rng.standard_normal((G, S, non.size)))
    cast = lambda a: None if a is None else a.astype(dtype)                   # noqa: E731
    return cast(x), cast(Y), cast(sigma), cast(X), gm, lin, owner, non, n


# ---- the layout ------------------------------------------------------------------------------------------------------
def test_the_layout_is_a_global_map_over_the_non_linear_parameters():
    gm, lin, owner, non = models.separable_global_map("exp*2+poly*1", 5, 300, [1, 3])
    assert isinstance(gm, bounded_lsq.GlobalMap) and (gm.n, gm.S, gm.ns, gm.nl, gm.nv) == (2, 300, 2, 0, 2)
    assert lin.tolist() == [0, 2, 4] and non.tolist() == [1, 3]
    gm, lin, owner, non = models.separable_global_map("gauss+poly*1", 4, 5, np.array([False, False, True, False]))
    assert (gm.ns, gm.nl, gm.nv) == (1, 1, 6) and gm.cols.tolist() == [[1 + s, 0] for s in range(5)]
    with pytest.raises(ValueError, match="`shared` index 0 is a linear parameter"):
        models.separable_global_map("gauss+poly*1", 4, 5, [0, 2])
    with pytest.raises(ValueError, match="`shared` index 9 is outside"):
        models.separable_global_map("gauss+poly*1", 4, 5, [9])
    with pytest.raises(ValueError, match="`shared` is empty"):
        models.separable_global_map("gauss+poly*1", 4, 5, [])
    with pytest.raises(ValueError, match="use `lsq_linear`"):
        models.separable_global_map("poly*3", 3, 5, [0])


@pytest.mark.parametrize("with_sigma", [False, True])
def test_the_definition_is_varpro_reduce_per_data_set(with_sigma):
    spec = "gauss+poly*1"
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, 3, [2], with_sigma=with_sigma)
    G, S, m = Y.shape
    f = models.separable_global_residual(spec, Y, [2], sigma)(x, X)
    J = models.separable_global_jacobian(spec, Y, [2], sigma)(x, X)
    c = models.separable_global_coefficients(spec, Y, [2], sigma)(x, X)
    assert f.shape == (G, S * m) and J.shape == (G, S * m, gm.nv) and c.shape == (G, S, lin.size)
    M = models.resolve(spec)
    for g in range(G):
        for s in range(S):
            alpha = X[g, gm.cols[s]]
            Graw = M.jac(x, models.varpro_expand(alpha[None], lin, n))
            w = None if sigma is None else 1.0 / sigma[g, s][None]
            fr, Jr, cr, info = models.varpro_reduce(Graw, Y[g, s][None], w, lin, owner)
            rows = slice(s * m, (s + 1) * m)
            assert np.array_equal(f[g, rows], fr[0]) and np.array_equal(c[g, s], cr[0])
            assert np.array_equal(J[g, rows][:, gm.cols[s]], Jr[0])
            other = np.setdiff1d(np.arange(gm.nv), gm.cols[s])
            assert np.all(J[g, rows][:, other].view(np.int64) == 0)          # +0.0


@pytest.mark.parametrize("with_sigma", [False, True])
@pytest.mark.parametrize("spec, shared", [("gauss+poly*1", [2]), ("exp*2+poly*1", [1]), ("exp*2+poly*1", [1, 3])])
def test_kaufmans_gradient_of_a_group_against_central_differences(spec, shared, with_sigma):
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, 3, shared, with_sigma=with_sigma, dtype=LD)
    stage = _HostGlobalStage(spec, Y, shared, sigma, n)
    f, J = stage(x, X)[:2]
    assert f.dtype == LD
    grad = np.einsum("gik,gi->gk", J, f)
    h = LD(1e-7)
    for v in range(gm.nv):
        Xp, Xm = X.copy(), X.copy()
        Xp[:, v] += h
        Xm[:, v] -= h
        fp, fm = stage(x, Xp)[0], stage(x, Xm)[0]
        fd = (np.sum(fp * fp, axis=1) - np.sum(fm * fm, axis=1)) / (4 * h)
        scale = np.linalg.norm(J[:, :, v], axis=1) * np.linalg.norm(f, axis=1)
        assert np.all(np.abs(fd - grad[:, v]) <= 1e-9 * scale), (v, fd, grad[:, v])


# ---- the covariance --------------------------------------------------------------------------------------------------
def dense_blocks(spec, x, Y, sigma, popt, shared):
    """The (S, n, n) blocks of the inverse of the full group's J^T J, the matrix built by explicit loops in longdouble:
    column of parameter j of data set s is GlobalMap(n, S, shared).column(j, s).  Also kappa_2(J^T J)."""
    M = models.resolve(spec)
    S, m = Y.shape
    n = popt.shape[1]
    gfull = bounded_lsq.GlobalMap(n, S, shared)
    Jm = M.jac(x.astype(LD), popt.astype(LD))
    A = np.zeros((gfull.nv, gfull.nv), dtype=LD)
    for s in range(S):
        for i in range(m):
            w = LD(1) if sigma is None else LD(1) / LD(sigma[s, i])
            for j in range(n):
                for k in range(n):
                    A[gfull.column(j, s), gfull.column(k, s)] += (w * Jm[s, i, j]) * (w * Jm[s, i, k])
    C = np.linalg.inv(A.astype(np.float64)).astype(LD)
    for _ in range(3):                            # Newton-Schulz in longdouble: C <- C (2 I - A C)
        C = C @ (2 * np.eye(gfull.nv, dtype=LD) - A @ C)
    return np.stack([C[np.ix_(gfull.cols[s], gfull.cols[s])] for s in range(S)]), np.linalg.cond(A.astype(np.float64))


@pytest.mark.parametrize("spec, S, shared, with_sigma", [
    ("exp*2+poly*1", 1, [1, 3], False), ("exp*2+poly*1", 3, [1, 3], False), ("gauss+poly*1", 1, [1, 2], False),
    ("gauss+poly*1", 3, [1, 2], True), ("gauss+poly*1", 3, [2], False), ("exp*2+poly*1", 3, [3], True)], ids=str)
def test_cov_blocks_against_the_dense_inverse(spec, S, shared, with_sigma):
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, S, shared, G=1, with_sigma=with_sigma)
    f, J, c, info, Sinv, TD = _HostGlobalStage(spec, Y, shared, sigma, n)(x, X)
    assert not info.any()
    C = np.linalg.inv(J[0].T @ J[0])
    blocks = models.separable_global_cov(C[None], Sinv, TD, gm, np.array([2.5]), lin)[0]
    assert blocks.shape == (S, n, n) and np.array_equal(blocks, np.swapaxes(blocks, 1, 2))
    popt = models.varpro_expand(gm.split_x(X[0]), lin, n)
    popt[:, lin] = c[0]
    want, kappa = dense_blocks(spec, x, Y[0], None if sigma is None else sigma[0], popt, shared)
    err = np.max(np.abs(blocks.astype(LD) / LD(2.5) - want), axis=(1, 2)) / np.max(np.abs(want), axis=(1, 2))
    print(spec, S, shared, "kappa_2(J^T J) = %.3g" % kappa, "worst fraction of 64 kappa eps: %.3g"
          % float(np.max(err) / (64 * kappa * EPS)))
    assert np.all(err <= 64 * kappa * EPS)
    with pytest.raises(ValueError, match="`lin` is required"):
        models.separable_global_cov(C[None], Sinv, TD, gm)
    with pytest.raises(ValueError, match="`C` must have shape"):
        models.separable_global_cov(C[None, :1], Sinv, TD, gm, None, lin)


# ---- the front end, the solve stubbed ------------------------------------------------------------------------------------
class Stub:
    """In the place of ``least_squares_batch``: the start point is the solution; f, J and the unscaled covariance there."""

    def __init__(self):
        self.calls = []

    def __call__(self, fun, x0, jac, **kw):
        self.calls.append((x0.copy(), kw))
        f, J = fun(x0), jac(x0)
        out = []
        for g in range(x0.shape[0]):
            out.append(types.SimpleNamespace(x=x0[g].copy(), success=True, status=1, fun=f[g], jac=J[g], nfev=1, njev=1,
                                             obj_value=float(f[g] @ f[g]), active_mask=np.zeros(x0.shape[1], dtype=int),
                                             x_covariance=np.linalg.inv(J[g].T @ J[g]), optimality=0.0))
        return out


def front(monkeypatch, spec, x, Y, p0, shared, **kw):
    stub = Stub()
    monkeypatch.setattr(_curve_fit, "least_squares_batch", stub)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, separable=True, driver="host", ctx=object(), **kw)
    return out, stub


@pytest.mark.parametrize("absolute", [False, True])
def test_front_end_shapes_bounds_and_the_variance_factor(monkeypatch, absolute):
    spec, shared = "gauss+poly*1", [2]
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, 3, shared, with_sigma=True)
    G, S, m = Y.shape
    p0 = np.full((G, S, n), np.nan)
    p0[..., non] = gm.split_x(X)
    lb, ub = np.full((G, S, n), -np.inf), np.full((G, S, n), np.inf)
    lb[:, 0, 2], lb[:, 1, 2], ub[:, 2, 2] = 0.1, 0.2, 0.9          # the shared width: the box is the intersection
    ub[0, 1, 1] = 5.0                                               # a local position
    (popt, pcov, res), stub = front(monkeypatch, spec, x, Y, p0, shared, sigma=sigma, bounds=(lb, ub),
                                    absolute_sigma=absolute)
    x0, kw = stub.calls[0]
    assert x0.shape == (G, gm.nv) and np.array_equal(x0, X)
    assert kw["covariance"] == "pinv" and kw["_variance_scale"] is False
    lo, hi = kw["bounds"]
    assert lo.shape == (G, gm.nv) and np.all(lo[:, 0] == 0.2) and np.all(hi[:, 0] == 0.9)
    assert hi[0, gm.column(0, 1)] == 5.0 and np.isinf(hi[1]).sum() == gm.nv - 1
    assert popt.shape == (G, S, n) and pcov.shape == (G, S, n, n) and len(res) == G
    f, J, c, info, Sinv, TD = _HostGlobalStage(spec, Y, shared, sigma, n)(x, X)
    for g, r in enumerate(res):
        factor = 1.0 if absolute else float(f[g] @ f[g]) / (S * m - gm.nv - S * lin.size)
        C = np.linalg.inv(J[g].T @ J[g])
        want = models.separable_global_cov(C, Sinv[g], TD[g], gm, None, lin) * factor
        np.testing.assert_allclose(pcov[g], want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r.x_covariance, C * factor, rtol=1e-12, atol=0)
        assert np.array_equal(popt[g][:, lin], c[g]) and np.array_equal(popt[g][:, non], gm.split_x(X[g]))
        assert r.popt.shape == (S, n) and r.linear_coefficients.shape == (S, lin.size)
        assert r.linear_params.tolist() == lin.tolist() and r.global_map.nv == gm.nv
        assert r.fun.shape == (S * m,) and r.jac.shape == (S * m, gm.nv)
    (p1, c1, r1), _ = front(monkeypatch, spec, x, Y[0], p0[0], shared, sigma=sigma[0], absolute_sigma=absolute)
    assert p1.shape == (S, n) and c1.shape == (S, n, n) and np.array_equal(p1, popt[0])


def test_front_end_without_a_degree_of_freedom(monkeypatch):
    spec, shared = "gauss+poly*1", [1, 2]
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, 2, shared, m=3)          # S m - nv - S nl = 6 - 2 - 4 = 0
    p0 = np.zeros(Y.shape[:2] + (n,))
    p0[..., non] = gm.split_x(X)
    stub = Stub()
    monkeypatch.setattr(_curve_fit, "least_squares_batch", stub)
    with pytest.warns(bounded_lsq.OptimizeWarning if hasattr(bounded_lsq, "OptimizeWarning") else Warning):
        popt, pcov, res = bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, separable=True, driver="host", ctx=object())
    assert np.isinf(pcov).all() and np.isfinite(popt).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pcov = bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, separable=True, driver="host", ctx=object(),
                                            absolute_sigma=True)[1]
    assert np.isfinite(pcov).all()


def test_rejections(monkeypatch):
    spec, shared = "gauss+poly*1", [1, 2]
    x, Y, sigma, X, gm, lin, owner, non, n = small(spec, 3, shared)
    p0 = np.ones(Y.shape[:2] + (n,))
    monkeypatch.setattr(_curve_fit, "least_squares_batch", Stub())

    def go(f=spec, shared=shared, Y=Y, p0=p0, x=x, **kw):
        return bounded_lsq.curve_fit_global(f, x, Y, p0, shared, separable=True, driver="host", ctx=object(), **kw)
    lb = np.full(n, -np.inf)
    lb[0] = 0.0
    for kw, text in ((dict(f=lambda t, P: P[:, :1] * t), "needs a built-in model"),
                     (dict(f=models.expression("a*exp(-t/tau)+c", ("a", "tau", "c")), p0=np.ones(Y.shape[:2] + (3,))),
                      "expression model"),
                     (dict(jac="2-point"), "`jac` must be None"), (dict(loss="huber"), "`loss` must be 'linear'"),
                     (dict(estimator="poisson"), "estimator='poisson' is not yet supported"),
                     (dict(nan_policy="omit"), "nan_policy='omit' is not yet supported"),
                     (dict(fixed=[1]), "`fixed` / `tied` are not yet supported"),
                     (dict(tied={2: 1}), "`fixed` / `tied` are not yet supported"),
                     (dict(leverage=True), "leverage=True is not yet supported"),
                     (dict(Y=Y[:, :, :2], x=x[:2]), "needs more points than linear parameters: m = 2, nl = 2"),
                     (dict(f="poly*3", p0=np.ones(Y.shape[:2] + (3,)), shared=[0]), "use `lsq_linear`"),
                     (dict(shared=[0, 1]), "`shared` index 0 is a linear parameter"),
                     (dict(bounds=(lb, np.inf)), "parameter 0.*is linear and is projected out"),
                     (dict(separable=1), None)):
        if text is None:
            with pytest.raises(ValueError, match="`separable` must be False or True"):
                bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, separable=1)
            continue
        with pytest.raises(ValueError, match=text):
            go(**kw)
    gml, *_ = models.separable_global_map("gauss+poly*1", 4, 128, [2])                # nv = 1 + 128 = 129: fine
    assert gml.nv == 129
    big = np.ones((1, 300, 16))
    with pytest.raises(ValueError, match=r"nv = nsh \+ S nloc = 1 \+ 300 \* 1 = 301 non-linear variables, more than 256"):
        go(Y=big, p0=np.ones((1, 300, n)), shared=[2], x=np.linspace(-1, 1, 16))
    with pytest.raises(ValueError, match="GlobalMap over the 2 non-linear parameters"):
        models.DeviceFit(spec, n, x, Y, separable=True, global_map=bounded_lsq.GlobalMap(n, 3, shared))


def test_the_abi_declares_the_new_entries():
    import re
    from bounded_lsq import _abi
    src = open(_abi.__file__.replace("bounded_lsq/_abi.py", "../include/blsq.h")).read()
    for name, nargs in (("blsq_varpro_expand_global_dev", 9), ("blsq_varpro_reduce_global_dev", 20),
                        ("blsq_varpro_cov_blocks_dev", 14)):
        assert len(_abi.SIGNATURES[name][1]) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, src).group(1)
        assert decl.count(",") + 1 == nargs


# ---- the fit cases of the GPU tests are solvable ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.FITS))
def test_scipy_converges_on_the_reduced_residual_of_every_fit_case(name):
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data(name)
    lin, owner = models.linear_params(spec, n)
    assert np.isnan(p0_sep[..., lin]).all() and np.isfinite(p0_sep[..., owner >= 0]).all()
    for g in range(Y.shape[0]):
        popt, res = gc.scipy_reference(name, g)
        print(name, g, "nfev", res.nfev, "cost %.3g" % res.cost, "optimality %.3g" % res.optimality)
        # (scipy differences the Jacobian: its gradient carries sqrt(eps) |J| |f|, about 1e-7 here)
        assert res.success and res.optimality < 1e-6 and res.nfev < 40
        np.testing.assert_allclose(popt[:, list(shared)], P[g][:, list(shared)], rtol=0.05)
