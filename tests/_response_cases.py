"""Inputs shared by tests/test_response_cpu.py and tests/test_response_gpu.py: the kernels, the
extended-precision reference and error bounds of the kernel-level comparison, and the seeded end-to-end fits with their
numpy definition.  Not collected as a test.

Bounds.  A sum of L terms h[k] g[.], each product rounded once and added in any order (fused or not), is off its exact
value by at most gamma_L sum |h||g|, gamma_k = k eps / (1 - k eps), eps = 2^-52 (the device fuses, which is tighter).
The residual w (mu - y) adds a subtraction and a product: three more roundings over (sum |h||g| + |y|) |w|.  A Jacobian
entry w HG adds the product: two more over |w| sum |h||G|."""
import numpy as np

from bounded_lsq import models, ParamMap

LD = np.longdouble
EPS = 2.0 ** -52


def gamma(k):
    return k * EPS / (1 - k * EPS)


def irf(L=24, centre=8.0, sigma=2.5):
    """A Gaussian instrument response of `sigma` channels centred at tap `centre`, L taps, normalised to sum 1."""
    h = np.exp(-0.5 * ((np.arange(L) - centre) / sigma) ** 2)
    return h / h.sum()


def loop_reference(g, h, origin):
    """apply_response by the explicit double loop of its definition, one problem: g (m,), h (L,)."""
    m, L = len(g), len(h)
    out = np.zeros(m, dtype=np.result_type(g.dtype, h.dtype))
    for i in range(m):
        for k in range(L):
            j = i + origin - k
            if 0 <= j < m:
                out[i] += h[k] * g[j]
    return out


def reference(g, G, h, origin, reps):
    """-> mu (Q, m), HG (B, m, nc), and the magnitudes sum |h||g|, sum |h||G|, all in np.longdouble.  g (Q, m) with
    Q = B reps, G (B, m, nc), h (L,) or (B, L)."""
    hl = np.asarray(h, dtype=LD)
    hq = np.repeat(hl, reps, axis=0) if hl.ndim == 2 else hl
    gl, Gl = np.asarray(g, dtype=LD), np.moveaxis(np.asarray(G, dtype=LD), 1, -1)
    with np.errstate(invalid="ignore"):
        mu = models.apply_response(gl, hq, origin)
        HG = np.moveaxis(models.apply_response(Gl, hl, origin), -1, 1)
        mu_abs = models.apply_response(np.abs(gl), np.abs(hq), origin)
        HG_abs = np.moveaxis(models.apply_response(np.abs(Gl), np.abs(hl), origin), -1, 1)
    return mu, HG, mu_abs, HG_abs


def per_point(a, reps):
    """(B, m) weights or data as (Q, m); (m,) and None as they are."""
    return a if a is None or np.ndim(a) == 1 else np.repeat(a, reps, axis=0)


# ---- end to end ------------------------------------------------------------------------------------------------------
B = 8


def _decay(spec, counts, per_problem_h=False, seed=0):
    """A decay through the response of a detector: m = 130 channels, rates 0.5 and 0.05 per channel, a Gaussian IRF of
    2.5 channels centred at tap 8 (L = 24, sum 1), origin 0.  counts: Poisson draws at a peak of about 1000 for
    estimator='poisson'; otherwise Gaussian noise of a known `sigma`.  per_problem_h: every problem has an IRF of its
    own width and delay."""
    rng = np.random.default_rng([11, seed, int(counts), len(spec)])
    m = 130
    x = np.arange(m, dtype=float)
    scale = 1000.0 if counts else 100.0
    if spec == "exp*2":
        base = np.array([0.9 * scale, 0.5, 0.45 * scale, 0.05])
        lb, ub = [0.0, 0.2, 0.0, 0.005], [50 * scale, 2.0, 50 * scale, 0.15]
    else:                                              # exp+poly*1
        base = np.array([0.6 * scale, 0.05, 0.02 * scale])
        lb, ub = [0.0, 0.005, 1e-3], [50 * scale, 1.0, scale]
    truth = base * (1 + 0.05 * rng.uniform(-1, 1, (B, len(base))))
    if per_problem_h:
        h = np.stack([irf(24, 8.0 + 0.2 * (b - 3.5), 2.0 + 0.15 * b) for b in range(B)])
    else:
        h = irf()
    mu = models.apply_response(models.compose(spec).f(x, truth), h, 0)
    sigma = None
    if counts:
        Y = rng.poisson(mu).astype(float)
    else:
        sigma = np.broadcast_to(0.5 + 0.02 * np.sqrt(np.abs(mu)), mu.shape).copy()
        Y = mu + sigma * rng.standard_normal(mu.shape)
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    return dict(spec=spec, x=x, Y=Y, P0=P0, truth=truth, h=h, origin=0, sigma=sigma,
                bounds=(np.broadcast_to(lb, truth.shape).copy(), np.broadcast_to(ub, truth.shape).copy()),
                kw=dict(estimator="poisson", absolute_sigma=True) if counts else dict(absolute_sigma=True))


def _line(two=False, tied=None, seed=0):
    """A line broadened by the resolution of a spectrometer: m = 70 channels, a centred Gaussian kernel of 2 channels
    (L = 15, origin 7), over a baseline.  The 7 points at each end are NaN for nan_policy='omit': they would see the
    zero padding of the convolution.  two: a second line whose width is tied to the first's (`tied`)."""
    rng = np.random.default_rng([12, seed, int(two)])
    m = 70
    x = np.arange(m, dtype=float)
    base = [100.0, 28.0, 4.0, 60.0, 45.0, 4.0, 10.0] if two else [100.0, 33.0, 4.0, 10.0]
    n = len(base)
    truth = np.array(base) * (1 + 0.04 * rng.uniform(-1, 1, (B, n)))
    pm = None
    if tied:
        pm = ParamMap(n, None, tied)
        truth = pm.expand_x(pm.reduce_x(truth), truth)
    spec = "gauss*2+poly*1" if two else "gauss+poly*1"
    h = irf(15, 7.0, 2.0)
    mu = models.apply_response(models.compose(spec).f(x, truth), h, 7)
    sigma = 1.0
    Y = mu + sigma * rng.standard_normal(mu.shape)
    Y[:, :7] = np.nan
    Y[:, -7:] = np.nan
    P0 = truth * (1 + 0.08 * rng.choice([-1.0, 1.0], truth.shape))
    if pm is not None:
        P0 = pm.expand_x(pm.reduce_x(P0), P0)
    lb = np.broadcast_to([0.0, 5.0, 1.0] * (n // 3) + [0.0], truth.shape).copy()
    ub = np.broadcast_to([1e4, 65.0, 15.0] * (n // 3) + [100.0], truth.shape).copy()
    kw = dict(nan_policy="omit", absolute_sigma=True)
    if tied:
        kw["tied"] = tied
    return dict(spec=spec, x=x, Y=Y, P0=P0, truth=truth, h=h, origin=7, sigma=sigma, bounds=(lb, ub), kw=kw)


CASES = {
    "decay-sigma-exp+poly": lambda: _decay("exp+poly*1", False),
    "decay-sigma-exp2": lambda: _decay("exp*2", False),
    "decay-counts-exp+poly": lambda: _decay("exp+poly*1", True),
    "decay-counts-exp2": lambda: _decay("exp*2", True),
    "line-omit": lambda: _line(),
    "line-tied-width": lambda: _line(True, {5: 2}),
    "line-tied-ratio": lambda: _line(True, {5: (2, 1.25)}, seed=1),
    "decay-per-problem-h": lambda: _decay("exp+poly*1", False, per_problem_h=True, seed=2),
}
FD_CASES = ("decay-sigma-exp+poly", "decay-counts-exp2")        # jac='2-point' on case 1


def definition(case, with_response=True):
    """The numpy definition of a case's residual and Jacobian over the SOLVER's variables, for all problems at once:
    -> (pm or None, fres(X) -> (B, m), jres(X) -> (B, m, nf)).  with_response=False: the same data against the
    unconvolved model."""
    M = models.compose(case["spec"])
    kw = case["kw"]
    pm = ParamMap(M.n, None, kw["tied"]) if kw.get("tied") else None
    f, jac = M.f, M.jac
    if pm is not None:
        f, jac = pm.wrap_f(f, case["P0"]), pm.wrap_jac(jac, case["P0"])
    if with_response:
        f, jac = (models.response_residual(f, case["h"], case["origin"]),
                  models.response_jacobian(jac, case["h"], case["origin"]))
    x, Y = case["x"], case["Y"]
    if kw.get("estimator") == "poisson":
        fr, jr = models.poisson_residual(f, Y), models.poisson_jacobian(f, jac, Y)
        fres, jres = (lambda X: fr(x, X)), (lambda X: jr(x, X))
    else:
        w = 1.0 / np.asarray(case["sigma"], dtype=float)
        fres = lambda X: w * (f(x, X) - Y)                                          # noqa: E731
        jres = lambda X: (w[..., np.newaxis] if np.ndim(w) else w) * jac(x, X)     # noqa: E731
    if kw.get("nan_policy") == "omit":
        fres, jres = models.omit_residual(fres, Y), models.omit_jacobian(jres, Y)
    return pm, fres, jres


def scipy_fit(case, b, with_response=True):
    """Problem b alone by scipy.optimize.least_squares on the definition -> (x (nf,), standard errors (nf,), lb, ub,
    truth (nf,)), absolute_sigma=True throughout."""
    from scipy.optimize import least_squares
    pm, fres, jres = definition(case, with_response)
    lb, ub = case["bounds"]
    X0, T = case["P0"], case["truth"]
    if pm is not None:
        lb, ub = pm.reduce_bounds(lb, ub)
        X0, T = pm.reduce_x(X0), pm.reduce_x(T)
    template = X0.copy()

    def at(v):
        X = template.copy()
        X[b] = v
        return X
    res = least_squares(lambda v: fres(at(v))[b], X0[b], jac=lambda v: jres(at(v))[b], bounds=(lb[b], ub[b]),
                        method="trf", ftol=1e-13, xtol=1e-13, gtol=1e-13)
    se = np.sqrt(np.diag(np.linalg.pinv(res.jac.T @ res.jac)))
    return res.x, se, lb[b], ub[b], T[b]
