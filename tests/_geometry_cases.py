"""Step-solve inputs over the bound geometries `bounded_lsq/_synth.py` never draws, per factorisation route, and the
screen that admits a draw on the CPU reference alone.  No GPU code: tools/make_geometry_cases.py screens the draws and
writes tests/golden/geometry_cases.json, tests/test_geometry_cpu.py holds the conditions the inputs must meet,
tests/test_geometry_gpu.py runs the admitted cases.

A problem is `_synth.trf_problem(seed, m, n)` / `_synth.dogbox_problem(seed, m, n, 0.0)` with its bounds, scale and
on_bound redrawn from `default_rng(seed + CLASS_SEED[class])`.  A case is a problem with one trust radius (TRF: and one
initial alpha).

Why a screen: with x within 10^U(-12,-1) of its bounds the reference's OWN step moves by up to 1e-9 when every entry
of J moves by one ulp (trf.py:264-274: gesdd of the augmented matrix whose Coleman-Li block spans six decades and
more), above the project's 1e-10 bar — such an input says nothing about a kernel.  `screen` runs the oracle on J and on
J with every entry moved one ulp by random sign patterns; a case is admitted iff the step moves by at most SCREEN_RTOL
and no mask, branch or count changes.  It never sees the code under test.
"""
import numpy as np

from bounded_lsq import _synth
from oracle import blsq_oracle as orc

SCREEN_RTOL = 1e-12                    # the 1e-10 bar with a factor of 100 to spare
TRF_CLASSES = ("one_sided", "mixed", "far", "near6", "near12", "jac_scale")
CSNE_CLASSES = ("one_sided", "unbounded")
DOG_CLASSES = ("upper", "both_signs", "one_sided_box", "far", "inward", "one_free", "all_active")
CLASS_SEED = {c: 0x6E0 + 0x101 * k for k, c in enumerate(
    ("one_sided", "mixed", "far", "near6", "near12", "jac_scale", "unbounded",
     "upper", "both_signs", "one_sided_box", "inward", "one_free", "all_active"))}
TRF_PAIRS = ((0.05, 0.0), (1.0, 0.3), (30.0, 0.0), (0.5, "warm"))     # (Delta, alpha0); warm: alpha of the second pair
DOG_DELTAS = (0.01, 0.3, 30.0)
CSNE_KAPPA = 2e4
# Decades either side of 1 of the given scale on the csne route.  The tier takes a problem only if the reference's rank
# test holds by its PROVEN bound (csne_kernels.hip); measured on the MI355X: at two decades that gate hands 7 of 16
# unbounded draws to CholeskyQR2 instead, at one decade and below none.
CSNE_SCALE_SPAN = 1.0
SCALE_GIVEN, SCALE_JAC_INIT, SCALE_JAC_UPDATE = 0, 1, 2

# route -> (library switches, shapes per solver).  Each shape is the smallest that reaches the route.
ROUTES = {
    "reg":   dict(opts={},                 trf=((60, 16), (130, 79)), dogbox=((60, 16), (130, 79))),
    "rl":    dict(opts={},                 trf=((160, 96),),          dogbox=((160, 96),)),
    "tree":  dict(opts={"gram": 0},        trf=((160, 96), (90, 33)), dogbox=((160, 96), (90, 33))),
    "svd":   dict(opts={"no_svdfree": 1},  trf=((90, 33),),           dogbox=((90, 33),)),
    "wide":  dict(opts={},                 trf=((300, 272),),         dogbox=((300, 272), (640, 600))),
    "short": dict(opts={},                 trf=((40, 60),),           dogbox=((40, 60),)),
    "csne":  dict(opts={},                 trf=((1024, 96),),         dogbox=()),
}


def seeds_for(n):
    return 16 if n < 272 else 8


def classes_for(solver, route):
    if solver == "dogbox":
        return DOG_CLASSES
    return CSNE_CLASSES if route == "csne" else TRF_CLASSES


def base_seed(solver, route, m, n, cls):
    """Disjoint seed ranges per (solver, route, shape, class): no two groups share a `_synth` problem."""
    k = sorted(ROUTES).index(route) * 16 + sorted(CLASS_SEED).index(cls)
    return (500000 if solver == "trf" else 900000) + 1000 * k + 7 * (m % 97) + n


def _logspaced(rng, m, n, kappa):
    """The construction of tests/test_csne_gpu.logspaced: singular values log-spaced over [1/kappa, 1] sqrt(m)."""
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * np.logspace(0, -np.log10(kappa), n)) @ V.T * np.sqrt(m)


def _jac_scale(J, given, mode):
    """trf.py:216-219, 239-242 (scaling='jac') on the host: the scale the oracle is fed while screening."""
    norms = np.linalg.norm(J, axis=0)
    norms[norms == 0] = 1.0
    inv = 1.0 / norms
    return inv if mode == SCALE_JAC_INIT else np.minimum(given, inv)


def trf_problem(route, m, n, cls, seed, mode=SCALE_GIVEN):
    """-> dict(J, f, x, lb, ub, scale, scale_in, mode).  `scale` is what the oracle is fed; `scale_in` and `mode` what the
    device's factor call is given (class jac_scale: mode 1 ignores scale_in, mode 2 takes min(scale_in, 1 / ||J_j||))."""
    P = _synth.trf_problem(seed, m, n)
    rng = np.random.default_rng(int(seed) + CLASS_SEED[cls])
    x = P["x"]
    if route == "csne":
        P["J"] = _logspaced(rng, m, n, CSNE_KAPPA)
    span = CSNE_SCALE_SPAN if route == "csne" else 2.0
    scale = 10.0 ** rng.uniform(-span, span, n)
    inf = np.full(n, np.inf)
    if cls == "one_sided":
        up = np.ones(n, bool) if route == "csne" else rng.random(n) < 0.5
        dist = rng.uniform(1e-3, 0.5, n)
        P["lb"] = np.where(up, -inf, x - dist)
        P["ub"] = np.where(up, x + dist, inf)
    elif cls == "unbounded":
        P["lb"], P["ub"] = -inf, inf
    elif cls == "mixed":
        kind = rng.integers(0, 4, n)                           # free, lower only, upper only, both
        lo, hi = rng.uniform(1e-3, 0.5, n), rng.uniform(1e-3, 0.5, n)
        P["lb"] = np.where((kind == 1) | (kind == 3), x - lo, -inf)
        P["ub"] = np.where((kind == 2) | (kind == 3), x + hi, inf)
    elif cls == "far":
        P["lb"], P["ub"] = x - rng.uniform(5.0, 50.0, n), x + rng.uniform(5.0, 50.0, n)
    elif cls == "near6":
        P["lb"], P["ub"] = x - 10.0 ** rng.uniform(-6.0, -1.0, n), x + 10.0 ** rng.uniform(-6.0, -1.0, n)
    elif cls == "near12":
        # every second variable (by a coin) keeps the `_synth` box: with ALL variables at 10^U(-12,-1) the screen
        # rejected 45 of 64 draws at 160 x 96, above the class's cap of 2 in 3
        lo, hi = 10.0 ** rng.uniform(-12.0, -1.0, n), 10.0 ** rng.uniform(-12.0, -1.0, n)
        near = rng.random(n) < 0.5
        P["lb"], P["ub"] = np.where(near, x - lo, P["lb"]), np.where(near, x + hi, P["ub"])
    elif cls == "jac_scale":                                   # the `_synth` box
        given = rng.uniform(0.5, 2.0, n) / np.linalg.norm(P["J"], axis=0)
        P["scale_in"] = np.ones(n) if mode == SCALE_JAC_INIT else given
        scale = _jac_scale(P["J"], given, mode)
    else:
        raise ValueError(cls)
    P["scale"] = scale
    P.setdefault("scale_in", scale)
    P["mode"] = mode
    return P


def dogbox_problem(route, m, n, cls, seed):
    """-> dict(J, f, x, lb, ub, scale, on_bound): about n/5 variables placed exactly on a bound (dogbox.py:152-154)."""
    P = _synth.dogbox_problem(seed, m, n, 0.0)
    rng = np.random.default_rng(int(seed) + CLASS_SEED[cls])
    x = P["x"]
    P["scale"] = 10.0 ** rng.uniform(-2.0, 2.0, n)
    inf = np.full(n, np.inf)
    w = (5.0, 50.0) if cls == "far" else (1e-3, 0.5)
    lb, ub = x - rng.uniform(w[0], w[1], n), x + rng.uniform(w[0], w[1], n)
    g = P["J"].T.dot(P["f"])
    k = max(1, int(round(n / 5.0)))
    idx = rng.choice(n, size=k, replace=False)
    if cls == "upper":
        sign = np.ones(k, np.int64)
    elif cls in ("both_signs", "far"):
        sign = np.where(rng.random(k) < 0.5, -1, 1).astype(np.int64)
    elif cls == "one_sided_box":
        up = rng.random(n) < 0.5
        lb, ub = np.where(up, -inf, lb), np.where(up, ub, inf)
        sign = np.where(up[idx], 1, -1).astype(np.int64)       # on the bound that is finite
    elif cls == "inward":                                      # on_bound g >= 0: flagged, yet free (dogbox.py:172)
        sign = np.where(g[idx] >= 0, 1, -1).astype(np.int64)
    elif cls in ("one_free", "all_active"):                    # on_bound g < 0: active
        idx = np.arange(n) if cls == "all_active" else np.delete(np.arange(n), int(rng.integers(0, n)))
        sign = np.where(g[idx] < 0, 1, -1).astype(np.int64)
    else:
        raise ValueError(cls)
    x = x.copy()
    x[idx] = np.where(sign > 0, ub[idx], lb[idx])
    ob = np.zeros(n, np.int64)
    ob[idx] = sign
    P.update(x=x, lb=lb, ub=ub, on_bound=ob)
    return P


def problem(solver, route, m, n, cls, seed, mode=SCALE_GIVEN):
    if solver == "trf":
        return trf_problem(route, m, n, cls, seed, mode)
    return dogbox_problem(route, m, n, cls, seed)


def modes_for(cls):
    return (SCALE_JAC_INIT, SCALE_JAC_UPDATE) if cls == "jac_scale" else (SCALE_GIVEN,)


# ---- the oracle on a problem and on its one-ulp neighbours -----------------------------------------------------
def one_ulp(J, pattern):
    """J with EVERY entry moved one ulp, up or down by the sign pattern of seed `pattern`."""
    rng = np.random.default_rng(0x9E3779B9 + int(pattern))
    return np.nextafter(J, np.where(rng.random(J.shape) < 0.5, -np.inf, np.inf))


def trf_solve(P, J, pairs):
    """The oracle's steps of one factorisation for all (Delta, alpha0) pairs."""
    F = orc.trf_factor(J, P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    out = []
    for (D, a) in pairs:
        try:
            out.append(orc.trf_step(F, float(D), float(a)))
        except ValueError:                                     # trust_region.py:28-29, 34-35: the reference raises
            out.append(RAISED)
    return out


def warm_alpha(P):
    """alpha the oracle returns for the second pair (Delta = 1.0, alpha0 = 0.3) on the problem as drawn: the warm
    start of the fourth (trf.py:283-331: the inner loop carries alpha to the next, smaller radius)."""
    D, a = TRF_PAIRS[1]
    S = trf_solve(P, P["J"], [(D, a)])[0]
    return 0.0 if S is RAISED else S.alpha


def resolve_pairs(P):
    w = None
    out = []
    for (D, a) in TRF_PAIRS:
        if a == "warm":
            w = warm_alpha(P) if w is None else w
            a = w
        out.append((D, float(a)))
    return out


def dog_solve(P, J, deltas):
    F = orc.dogbox_factor(J, P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    if F.all_active:
        return [None for _ in deltas]
    return [orc.dogbox_step(F, float(D), P["on_bound"]) for D in deltas]


RAISED = "raised"                      # the reference's own ValueError: never a parity case


def _rel(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (den if den > 0 else 1.0))


def trf_same(S, T):
    if S is RAISED or T is RAISED:
        return False
    return (np.array_equal(S.hits, T.hits) and S.branch == T.branch and S.choice == T.choice
            and S.n_iter == T.n_iter)


def dog_same(S, T):
    if S is None or T is None:
        return S is None and T is None
    return (np.array_equal(S.on_bound_new, T.on_bound_new) and S.tr_hit == T.tr_hit and S.fallback == T.fallback)


def screen_problem(solver, P, radii, patterns):
    """-> [(admitted, movement, S)] per entry of `radii` (TRF: (Delta, alpha0) pairs; dogbox: Deltas), S the oracle's
    step on J as drawn (None: every variable active).  One factorisation per pattern serves all radii."""
    solve = trf_solve if solver == "trf" else dog_solve
    same = trf_same if solver == "trf" else dog_same
    base = solve(P, P["J"], radii)
    move = [0.0] * len(radii)
    ok = [True] * len(radii)
    for pat in patterns:
        Jp = one_ulp(P["J"], pat)
        Pp = P
        if solver == "trf" and P["mode"] != SCALE_GIVEN:       # 'jac' scaling follows J
            Pp = dict(P, scale=_jac_scale(Jp, P["scale_in"], P["mode"]))
        got = solve(Pp, Jp, radii)
        for k, (S, T) in enumerate(zip(base, got)):
            if not same(S, T):
                ok[k] = False
                move[k] = float("inf")
            elif S is not None:
                move[k] = max(move[k], _rel(T.step, S.step))
    return [(ok[k] and move[k] <= SCREEN_RTOL, move[k], base[k]) for k in range(len(radii))]


def screen(case, patterns):
    """case: dict(solver, route, m, n, cls, seed, mode, Delta, alpha0) -> (admitted, movement, S)."""
    P = problem(case["solver"], case["route"], case["m"], case["n"], case["cls"], case["seed"], case.get("mode", 0))
    radii = [(case["Delta"], case["alpha0"])] if case["solver"] == "trf" else [case["Delta"]]
    return screen_problem(case["solver"], P, radii, patterns)[0]


def summary(solver, S):
    """What the fixture records of the oracle's step beside its movement."""
    if solver == "trf":
        return [-1, -1] if S is RAISED else [int(S.branch), int(S.choice)]
    if S is None:
        return [-1, 0, 0]
    clip = int(np.any(S.on_bound_free != 0))                   # the box clips the dogleg (dogbox.py:38-75)
    return [int(S.tr_hit), int(S.fallback), clip]


# ---- the fixture -----------------------------------------------------------------------------------------------
def groups():
    """Every (solver, route, m, n, class, mode) the tool draws, in the fixture's order."""
    for solver in ("trf", "dogbox"):
        for route in ("reg", "rl", "tree", "svd", "wide", "short", "csne"):
            for (m, n) in ROUTES[route][solver]:
                for cls in classes_for(solver, route):
                    for mode in (modes_for(cls) if solver == "trf" else (SCALE_GIVEN,)):
                        yield solver, route, m, n, cls, mode


def group_seeds(solver, route, m, n, cls):
    s0 = base_seed(solver, route, m, n, cls)
    return [s0 + 11 * k for k in range(seeds_for(n))]


def load_fixture(path=None):
    import json
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_cases.json")
    with open(path) as fh:
        return json.load(fh)


def cases_of(fix, solver=None, route=None):
    """The admitted cases of the fixture as dicts (see `screen`), with `move` and `info` (see `summary`)."""
    out = []
    for G in fix["groups"]:
        if (solver and G["solver"] != solver) or (route and G["route"] != route):
            continue
        for row in G["admitted"]:
            c = dict(solver=G["solver"], route=G["route"], m=G["m"], n=G["n"], cls=G["cls"], mode=G["mode"],
                     seed=row[0], Delta=row[1], move=row[-2], info=row[-1])
            if G["solver"] == "trf":
                c["alpha0"] = row[2]
            out.append(c)
    return out
