"""Cases of the missing-data tests (nan_policy='omit'): the kernel instances, their inputs and NaN
patterns for tests/test_nan_policy_gpu.py, and the fit problems with their per-problem patterns, which
tests/test_nan_policy_cpu.py vets on the host (every problem keeps more points than it has free parameters)."""
import functools

import numpy as np

from bounded_lsq import models

import _model_cases as mc

ROWS = [1, 63, 64, 65, 130]                       # the edges of the 64-row tile
SENTINEL = 1234.5                                 # what f and J hold before a launch

# label -> (name or spec, n, fixed, tied)
INSTANCES = {
    "gauss_sum": ("gauss_sum", 4, None, None),
    "poly": ("poly", 3, None, None),
    "gauss2d": ("gauss2d", 5, None, None),
    "composite": ("gauss*2+lorentz+pvoigt+poly*3", 16, None, None),
    "wide": ("pvoigt*15+poly*4", 64, None, None),             # n = 64: one wave per workgroup
    "mapped": ("gauss_sum", 7, [6], {5: 2}),                  # nf = 5 < n = 7
}
PATTERNS = ["none", "first", "last", "seam", "alternate", "tile", "problem"]


model_of = functools.partial(mc.model_of, INSTANCES)
map_of = functools.partial(mc.map_of, INSTANCES)


def _roles(label):
    name, n = INSTANCES[label][:2]
    M = model_of(label)
    if isinstance(M, models.CompositeModel):
        out = []
        for fam, K in M.components:
            T = models.TERMS[fam]
            out += ["c"] * K if T.params is None else list(T.params) * K
        return out
    if name == "poly":
        return ["c"] * n
    if name == "gauss2d":
        return ["a", "mu", "mu", "s2", "c"]
    return ["a", "mu", "s"] * ((n - 1) // 3) + ["c"]


_DRAW = {"a": (1.0, 3.0), "mu": (2.0, 8.0), "s": (0.5, 2.0), "s2": (1.0, 3.0), "eta": (0.2, 0.8), "c": (0.2, 1.0)}


def kernel_inputs(label, m, B, reps, per_problem, sampling, seed=0):
    """Finite inputs of one launch, every model value positive (so both estimators take them): dict(t, ts, y, w1 (m,),
    w2 (B, m), X [B reps][nc], Pfix [B][n] or None, nc).  t: the points (sampling 0) or the bin rows (1), (.., m) per
    coordinate, shared or per problem; ts its stride."""
    rng = np.random.default_rng([seed, m, B, reps, int(per_problem), sampling, sorted(INSTANCES).index(label)])
    M, pm = model_of(label), map_of(label)
    n = INSTANCES[label][1]
    P = np.stack([rng.uniform(*_DRAW[r], B * reps) for r in _roles(label)], axis=1)
    lead = (B,) if per_problem else ()
    rows = []
    for c in range(M.coords):
        lo = np.sort(rng.uniform(0.0, 10.0, lead + (m,)), axis=-1)
        rows.append(lo)
        if sampling:
            rows.append(lo + rng.uniform(0.05, 0.3, lead + (m,)))
    t = np.ascontiguousarray(np.stack(rows, axis=-2) if len(rows) > 1 else rows[0])
    ts = len(rows) * m if per_problem else 0
    out = dict(t=t, ts=ts, y=rng.uniform(0.5, 20.0, (B, m)), w1=rng.uniform(0.5, 2.0, m),
               w2=rng.uniform(0.5, 2.0, (B, m)), nc=n if pm is None else pm.nf, Pfix=None, X=P)
    if pm is not None:
        out["X"], out["Pfix"] = np.ascontiguousarray(pm.reduce_x(P)), np.ascontiguousarray(P[::reps])
    return out


def nan_pattern(pattern, B, m):
    """The omitted points (B, m) of `pattern`, or None where the shape has no such pattern: 'first' row 0, 'last' row
    m - 1, 'seam' rows 63 and 64 (those that exist), 'alternate' every second row (problem b starts at row b % 2), 'tile'
    the whole of one 64-row tile of a longer problem (the last complete one), 'problem' all rows of problem 1 of 3."""
    om = np.zeros((B, m), dtype=bool)
    if pattern == "first":
        om[:, 0] = True
    elif pattern == "last":
        om[:, m - 1] = True
    elif pattern == "seam":
        if m < 64:
            return None
        om[:, 63:65] = True
    elif pattern == "alternate":
        for b in range(B):
            om[b, b % 2::2] = True
    elif pattern == "tile":
        if m <= 64:
            return None
        k = m // 64 - 1
        om[:, 64 * k:64 * (k + 1)] = True
    elif pattern == "problem":
        if B < 3:
            return None
        om[1, :] = True
    return om


# ---- fit problems ----------------------------------------------------------------------------------------------------
SPEC = "gauss+poly*1"
TRUTH = [1.5, -1.0, 0.4, 0.2]                     # a, mu, s, c: the peak lies where the longest ragged tail leaves it
NF = 4
SIGMA = 0.01
FIT_ROWS = [33, 70]
FIT_PATTERNS = ["none", "tail", "random", "flank"]


def fit_problem(m, B=8, seed=0):
    """B data sets of 'gauss+poly*1' on [-2, 2], as _composite_cases.fit_problem: the truth perturbed by 5 % per problem,
    noise of sigma = 0.01, p0 10 % off the truth (the sign drawn per parameter) and a box of +-(0.4 |p| + 0.2) around
    the truth.  -> dict(spec, x, Y, P0, bounds, truth)"""
    rng = np.random.default_rng([seed, m, 77])
    truth = np.asarray(TRUTH) * (1 + 0.05 * rng.uniform(-1, 1, (B, len(TRUTH))))
    x = np.linspace(-2.0, 2.0, m)
    Y = models.compose(SPEC).f(x, truth) + SIGMA * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    return dict(spec=SPEC, x=x, Y=Y, P0=P0, bounds=(truth - half, truth + half), truth=truth)


def fit_omitted(pr, seed=0):
    """The omitted points (B, m) of a fit problem, pattern b % 4 for problem b: none; a ragged tail of 5 to 20 points;
    10 % at random (fixed seed); a blanked window on the upper flank of the peak, mu + 0.3 s .. mu + 1.3 s."""
    B, m = pr["Y"].shape
    rng = np.random.default_rng([seed, m, 78])
    om = np.zeros((B, m), dtype=bool)
    for b in range(B):
        kind = FIT_PATTERNS[b % 4]
        if kind == "tail":
            om[b, m - int(rng.integers(5, 21)):] = True
        elif kind == "random":
            om[b, rng.choice(m, size=max(1, m // 10), replace=False)] = True
        elif kind == "flank":
            mu, s = pr["truth"][b, 1], pr["truth"][b, 2]
            om[b] = (pr["x"] >= mu + 0.3 * s) & (pr["x"] <= mu + 1.3 * s)
    return om


def blanked(Y, omitted):
    return np.where(omitted, np.nan, Y)


def histogram_problem(m=40, B=6, seed=0):
    """B histograms of 'gauss+poly*1' read as a density over m contiguous bins on [-2, 2]: Poisson counts of a peak of
    about 40 counts over 4 per channel; dead channels: problem b loses channels b, b + 7, b + 14, ... (none for b = 0).
    -> dict(spec, edges, Y (counts), omitted, P0, bounds, truth)"""
    rng = np.random.default_rng([seed, m, 79])
    truth = np.asarray([400.0, 0.1, 0.5, 40.0]) * (1 + 0.05 * rng.uniform(-1, 1, (B, 4)))
    edges = np.linspace(-2.0, 2.0, m + 1)
    mu = models.binned(SPEC).f(edges, truth)
    Y = rng.poisson(mu).astype(float)
    om = np.zeros((B, m), dtype=bool)
    for b in range(1, B):
        om[b, b::7] = True
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    lb, ub = truth - half, truth + half
    return dict(spec=SPEC, edges=edges, Y=Y, omitted=om, P0=P0, bounds=(lb, ub), truth=truth)


def ragged_scans(seed=0):
    """Three scans of 'gauss+poly*1' of lengths 40, 64 and 70 on [-2, 2] (each its own grid).
    -> dict(xs, ys, P0 (3, 4), bounds, truth)"""
    rng = np.random.default_rng([seed, 80])
    truth = np.asarray(TRUTH) * (1 + 0.05 * rng.uniform(-1, 1, (3, 4)))
    xs = [np.linspace(-2.0, 2.0, k) for k in (40, 64, 70)]
    ys = [models.compose(SPEC).f(x, truth[b:b + 1])[0] + SIGMA * rng.standard_normal(x.size) for b, x in enumerate(xs)]
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    return dict(xs=xs, ys=ys, P0=P0, bounds=(truth - half, truth + half), truth=truth)
