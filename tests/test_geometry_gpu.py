"""Step parity per factorisation route over the bound geometries `_synth.py` never draws: one-sided and mixed bounds,
wide boxes (Coleman-Li scaling active, step interior), x within 1e-6 / 1e-12 of its bounds, on_bound = +1, a given
scale != 1, 'jac' scaling and a warm-started alpha — crossed with the register Cholesky (N <= 80), the right-looking
Cholesky (N > 80), the Householder tree, the Jacobi SVD, the widths past the front end, m < n and the CSNE tier.

The cases are the rows of tests/golden/geometry_cases.json: draws of tests/_geometry_cases.py that the screen admitted on
the CPU oracle alone (the oracle's own step moves by at most 2.5e-13 under one-ulp changes of J; masks, branch, choice
and iteration count stable).  So there is no excuse mechanism here: every case is held to the project's bars
(tests/test_csne_gpu.check) — step within 1e-10 relative, hits / active_new / on_bound_new bit-exact, branch, choice,
n_iter, tr_hit, fallback equal, alpha and predicted_reduction within 1e-9 relative, status 0.

All admitted cases of a (route, shape) run as ONE batch through the host-pointer API (class jac_scale as a batch of its
own: the scale mode is an argument of the factor call — SCALE_JAC_INIT, then SCALE_JAC_UPDATE on the same plan; dogbox:
each problem once, its three radii as successive step calls on the one factor, which keeps the 640 x 600 batch at 56
Jacobi SVDs), and each test proves its route by the counters the suite already uses.

x_new: TRF strictly inside the box.  dogbox returns x + step (dogbox.py:220; setting flagged variables ON their bound is
the driver's, dogbox.py:257-261): a variable flagged in on_bound_new lies within the three roundings of
x + (c + t d) of its bound, an active variable has not moved a bit, every other one is inside the box.
"""
import numpy as np
import pytest

import _geometry_cases as gc
from oracle import blsq_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SCAL_RTOL = 1e-9
EPS = float(np.finfo(float).eps)
ENV = {"gram": "BLSQ_GRAM", "no_svdfree": "BLSQ_NO_SVDFREE"}


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def close(a, b, rtol):
    return abs(a - b) <= rtol * abs(b)


@pytest.fixture(scope="module")
def fix():
    return gc.load_fixture()


@pytest.fixture(scope="module")
def bl():
    import bounded_lsq
    return bounded_lsq


@pytest.fixture
def route_ctx(blsq_opt):
    """route -> a fresh context with the route's switches (and the defaults for the two the routes use)."""
    made = []

    def make(route):
        from bounded_lsq import _abi
        opts = dict(gram=1, no_svdfree=0)
        opts.update(gc.ROUTES[route]["opts"])
        for k, v in opts.items():
            blsq_opt(ENV[k], str(v))
        ctx = _abi.Context(0)
        made.append(ctx)
        return ctx
    yield make
    for c in made:
        c.close()


class Tally:
    def __init__(self, solver, route):
        self.solver, self.route = solver, route
        self.bad, self.worst, self.count = [], {}, {}

    def check(self, ok, case, what, value=None):
        if not ok:
            self.bad.append((case["m"], case["n"], case["cls"], case["mode"], case["seed"], case["Delta"], what, value))

    def step_error(self, case, e):
        k = (case["m"], case["n"], case["cls"])
        self.worst[k] = max(self.worst.get(k, 0.0), e)
        self.count[k] = self.count.get(k, 0) + 1

    def report(self):
        for (m, n, cls), w in sorted(self.worst.items()):
            print("geometry %-6s %-5s %4dx%-3d %-13s %3d cases, worst step error %.2e"
                  % (self.solver, self.route, m, n, cls, self.count[(m, n, cls)], w))


def _most_sweeps(fast, sweeps):
    """debug_sweeps is written by the Jacobi SVD only: read it where debug_fast says the SVD ran."""
    return int(sweeps[fast == 0].max()) if np.any(fast == 0) else 0


def _stack(problems, keys):
    return {k: np.stack([np.asarray(P[k]) for P in problems]) for k in keys}


def _problems(cases):
    """One problem per (class, seed, mode), shared by the radii drawn on it."""
    cache = {}
    out = []
    for c in cases:
        key = (c["cls"], c["seed"], c["mode"])
        if key not in cache:
            cache[key] = gc.problem(c["solver"], c["route"], c["m"], c["n"], c["cls"], c["seed"], c["mode"])
        out.append(cache[key])
    return out


# ---- TRF ------------------------------------------------------------------------------------------------------
def check_trf(T, case, P, scale, S, D, b, Fo_cache):
    key = (case["cls"], case["seed"], case["mode"])
    if key not in Fo_cache:
        Fo_cache.clear()                                       # (cases come grouped by problem: keep one factor)
        Fo_cache[key] = orc.trf_factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], scale)
    So = orc.trf_step(Fo_cache[key], float(case["Delta"]), float(case["alpha0"]))
    lb, ub = P["lb"], P["ub"]
    e = rel(S.step[b], So.step)
    T.step_error(case, e)
    T.check(e < RTOL, case, "step", e)
    T.check(np.array_equal(S.hits[b], So.hits), case, "hits")
    T.check(np.array_equal(S.active_new[b], orc.active_constraints(So.x_new, lb, ub, rtol=1e-8)), case, "active_new")
    T.check(int(S.branch[b]) == So.branch, case, "branch", (int(S.branch[b]), So.branch))
    T.check(int(D.choice[b]) == So.choice, case, "choice", (int(D.choice[b]), So.choice))
    T.check(int(S.n_iter[b]) == So.n_iter, case, "n_iter", (int(S.n_iter[b]), So.n_iter))
    T.check(close(S.alpha[b], So.alpha, SCAL_RTOL), case, "alpha", (S.alpha[b], So.alpha))
    T.check(close(S.predicted_reduction[b], So.predicted_reduction, SCAL_RTOL), case, "predicted_reduction",
            (S.predicted_reduction[b], So.predicted_reduction))
    T.check(np.all(S.x_new[b] > lb) and np.all(S.x_new[b] < ub), case, "x_new not strictly inside")
    T.check(int(S.status[b]) == 0, case, "status", int(S.status[b]))
    T.check([So.branch, So.choice] == case["info"], case, "the oracle's branch / choice is not the recorded one")
    return So


def trf_route_proof(T, route, case, ctx_stats, fast, sweeps, on_tier, B, n):
    gram, csne, cqr2 = ctx_stats
    if route in ("reg", "rl"):
        T.check(gram == (B, 0), case, "gram_stats", gram)
    elif route == "csne":
        # the tier is for what the conditioning certificate keeps off the normal equations, per problem by the problem's
        # own numbers: EVERY rejected problem is routed to it and delivered by it — none declined, none left for
        # CholeskyQR2 or the tree.  (test_trf_route holds the classes to their share on the tier.)
        k = 0 if on_tier is None else int(on_tier.sum())
        T.check(gram == (B - k, k), case, "gram_stats", (gram, k))
        T.check(csne == (k, k, 0) and cqr2 == 0, case, "csne_stats / cqr2_stats", (csne, cqr2, k))
    elif route == "svd":
        T.check(gram == (B, 0), case, "gram_stats", gram)
        T.check(np.all(fast == 0) and np.all(sweeps > 0), case, "debug_fast / debug_sweeps on the forced route",
                (fast.tolist(), sweeps.tolist()))
    else:                                                      # tree, wide, short: no normal equations
        T.check(gram == (0, 0), case, "gram_stats", gram)
        if route == "short" or (route == "tree" and 16 < n < 48):      # m < n fails the rank gate; the Jacobi band
            T.check(np.all(fast == 0) and np.all(sweeps > 0), case, "debug_fast / debug_sweeps",
                    (fast.tolist(), sweeps.tolist()))


def trf_solve(bl, ctx, A, Delta, alpha0, scale_in, mode, sol=None):
    B, m, n = A["J"].shape
    if sol is None:
        sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    ctx.gram_stats(reset=True); ctx.csne_stats(reset=True); ctx.cqr2_stats(reset=True)
    F = sol.factor(A["J"], A["f"], A["x"], A["lb"], A["ub"], scale_in, mode)
    fast, sweeps = sol.debug_fast(), sol.debug_sweeps()
    S = sol.step(Delta, np.array(alpha0, float))
    D = sol.fetch_step()
    on_tier = sol.debug_csne()[0] if ctx.csne_stats()[0] else None
    stats = (ctx.gram_stats(), ctx.csne_stats(), ctx.cqr2_stats())
    return sol, F, S, D, stats, fast, sweeps, on_tier


def run_trf_shape(bl, ctx, T, route, cases):
    """The cases of one shape: those with a given scale as one batch, class jac_scale as a second; -> the first batch
    (for the bits check) and the (branch, choice) pairs it reached."""
    m, n = cases[0]["m"], cases[0]["n"]
    plain = [c for c in cases if c["mode"] == gc.SCALE_GIVEN]
    Ps = _problems(plain)
    A = _stack(Ps, ("J", "f", "x", "lb", "ub", "scale"))
    Delta = np.array([c["Delta"] for c in plain]); alpha0 = np.array([c["alpha0"] for c in plain])
    sol, F, S, D, stats, fast, sweeps, on_tier = trf_solve(bl, ctx, A, Delta, alpha0, A["scale"], gc.SCALE_GIVEN)
    sol.close()
    trf_route_proof(T, route, plain[0], stats, fast, sweeps, on_tier, len(plain), n)
    print("geometry trf %-5s %dx%d: %d cases, gram %s csne %s, SVD-free %d, most sweeps %d"
          % (route, m, n, len(plain), stats[0], stats[1], int(fast.sum()), _most_sweeps(fast, sweeps)))
    cache = {}
    seen = set()
    tier = {}                                                  # class -> [cases on the tier, reflective, warm-started]
    for b, (c, P) in enumerate(zip(plain, Ps)):
        So = check_trf(T, c, P, P["scale"], S, D, b, cache)
        seen.add((So.branch, So.choice))
        if on_tier is not None and on_tier[b] == 1:
            t = tier.setdefault(c["cls"], [0, 0, 0])
            t[0] += 1; t[1] += int(So.branch == 1); t[2] += int(c["Delta"] == 0.5 and c["alpha0"] > 0)
    if route == "csne":
        # the unbounded draws all reach the tier (kappa^2 = 4e8 against the certificate's 2.5e5); of the bounded ones the
        # certificate itself accepts some (the Coleman-Li block regularises: measured 5 of 16 draws) — at least half are
        # on the tier, and the reflective branch and the warm start are both taken there
        count = {cls: sum(1 for c in plain if c["cls"] == cls) for cls in gc.CSNE_CLASSES}
        print("geometry trf csne on the tier [cases, reflective, warm]:", tier, "of", count)
        T.check(tier.get("unbounded", [0])[0] == count["unbounded"], plain[0], "unbounded cases off the tier", tier)
        t = tier.get("one_sided", [0, 0, 0])
        T.check(2 * t[0] >= count["one_sided"] and t[1] >= 3 and t[2] >= 3, plain[0], "one_sided cases on the tier", tier)
        T.check(tier.get("unbounded", [0, 0, 0])[2] >= 3, plain[0], "warm-started unbounded cases on the tier", tier)
    # class jac_scale: SCALE_JAC_INIT, then SCALE_JAC_UPDATE with a given vector, on one plan
    jac = [c for c in cases if c["mode"] != gc.SCALE_GIVEN]
    if jac:
        entries = sorted({(c["seed"], c["Delta"]) for c in jac})
        at = {e: k for k, e in enumerate(entries)}
        B = len(entries)
        sol = None
        for mode in (gc.SCALE_JAC_INIT, gc.SCALE_JAC_UPDATE):
            mine = {(c["seed"], c["Delta"]): c for c in jac if c["mode"] == mode}
            proto = dict(jac[0], mode=mode)
            jPs = _problems([dict(proto, seed=s) for (s, _) in entries])
            A = _stack(jPs, ("J", "f", "x", "lb", "ub", "scale_in"))
            Delta = np.array([d for (_, d) in entries])
            alpha0 = np.array([mine[e]["alpha0"] if e in mine else 0.0 for e in entries])
            sol, F, S, D, stats, fast, sweeps, on_tier = trf_solve(bl, ctx, A, Delta, alpha0, A["scale_in"], mode, sol)
            trf_route_proof(T, route, proto, stats, fast, sweeps, on_tier, B, n)
            cache = {}
            for e, c in sorted(mine.items()):
                b = at[e]
                P = jPs[b]
                # the device's scale against numpy column norms (test_jac_scaling_modes), then fed to the oracle
                inv = 1.0 / np.linalg.norm(P["J"], axis=0)
                want = inv if mode == gc.SCALE_JAC_INIT else np.minimum(P["scale_in"], inv)
                T.check(np.allclose(F.scale[b], want, rtol=1e-13, atol=0.0), c, "scale", rel(F.scale[b], want))
                cache.clear()
                check_trf(T, c, P, F.scale[b], S, D, b, cache)
        sol.close()
    return plain, Ps, seen


def trf_bits(bl, ctx, T, plain, Ps, picks):
    """The problem alone in its plan gives the bits it gave in the mixed batch."""
    A = _stack(Ps, ("J", "f", "x", "lb", "ub", "scale"))
    Delta = np.array([c["Delta"] for c in plain]); alpha0 = np.array([c["alpha0"] for c in plain])
    sol, F, S, D, *_ = trf_solve(bl, ctx, A, Delta, alpha0, A["scale"], gc.SCALE_GIVEN)
    sol.close()
    for b in picks:
        one = {k: v[b:b + 1] for k, v in A.items()}
        s1, F1, S1, D1, *_ = trf_solve(bl, ctx, one, Delta[b:b + 1], alpha0[b:b + 1], one["scale"], gc.SCALE_GIVEN)
        s1.close()
        for name in ("step", "x_new", "hits", "active_new", "alpha", "predicted_reduction", "n_iter", "branch"):
            T.check(np.array_equal(np.asarray(getattr(S1, name))[0], np.asarray(getattr(S, name))[b]), plain[b],
                    "bits alone vs in the batch: " + name)
        T.check(np.array_equal(F1.g[0], F.g[b]), plain[b], "bits alone vs in the batch: g")


@pytest.mark.parametrize("route", ["reg", "rl", "tree", "svd", "wide", "short", "csne"])
def test_trf_route(bl, fix, route_ctx, route):
    ctx = route_ctx(route)
    T = Tally("trf", route)
    seen = set()
    first = None
    for (m, n) in gc.ROUTES[route]["trf"]:
        cases = [c for c in gc.cases_of(fix, "trf", route) if (c["m"], c["n"]) == (m, n)]
        assert cases, (route, m, n)
        plain, Ps, s = run_trf_shape(bl, ctx, T, route, cases)
        seen |= s
        if first is None:
            first = (plain, Ps)
    plain, Ps = first
    trf_bits(bl, ctx, T, plain, Ps, (0, len(plain) // 2, len(plain) - 1))
    T.report()
    print("geometry trf %-5s (branch, choice) reached: %s" % (route, sorted(seen)))
    assert not T.bad, T.bad[:20]


# ---- dogbox ---------------------------------------------------------------------------------------------------
def check_dogbox(T, case, P, F, S, b, cache):
    key = (case["cls"], case["seed"])
    if key not in cache:
        cache.clear()
        cache[key] = orc.dogbox_factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    Fo = cache[key]
    x, lb, ub, ob = P["x"], P["lb"], P["ub"], P["on_bound"]
    T.check(np.array_equal(F.active_set[b], Fo.active.astype(np.uint8)), case, "active_set")
    T.check(int(F.all_active[b]) == int(Fo.all_active), case, "all_active", int(F.all_active[b]))
    T.check(int(S.status[b]) == 0, case, "status", int(S.status[b]))
    if Fo.all_active:                                          # no step: x stays, the mask stays (dogbox.py:176-178)
        T.check(case["info"][0] == -1, case, "the oracle's all_active is not the recorded one")
        T.check(not np.any(S.step[b]) and np.array_equal(S.x_new[b], x) and np.array_equal(S.on_bound_new[b], ob),
                case, "all active: step / x_new / on_bound_new")
        T.check(int(S.tr_hit[b]) == 0 and int(S.fallback[b]) == 0 and S.predicted_reduction[b] == 0.0, case,
                "all active: tr_hit / fallback / predicted_reduction")
        T.step_error(case, 0.0)
        return None
    So = orc.dogbox_step(Fo, float(case["Delta"]), ob)
    e = rel(S.step[b], So.step)
    T.step_error(case, e)
    T.check(e < RTOL, case, "step", e)
    T.check(np.array_equal(S.on_bound_new[b], So.on_bound_new), case, "on_bound_new")
    T.check(int(S.tr_hit[b]) == int(So.tr_hit), case, "tr_hit", (int(S.tr_hit[b]), int(So.tr_hit)))
    T.check(int(S.fallback[b]) == int(So.fallback), case, "fallback", (int(S.fallback[b]), int(So.fallback)))
    T.check(close(S.predicted_reduction[b], So.predicted_reduction, SCAL_RTOL), case, "predicted_reduction",
            (S.predicted_reduction[b], So.predicted_reduction))
    xn, st, obn = S.x_new[b], S.step[b], S.on_bound_new[b]
    T.check(np.array_equal(xn, x + st), case, "x_new is not x + step")
    T.check(np.array_equal(xn[Fo.active], x[Fo.active]), case, "an active variable moved")
    free = Fo.free
    slack = 4.0 * EPS * (np.abs(x) + np.abs(st))               # three roundings of x + (c + t d)
    lo, up = free & (obn < 0), free & (obn > 0)
    T.check(np.all(np.abs(xn[lo] - lb[lo]) <= slack[lo]) and np.all(np.abs(xn[up] - ub[up]) <= slack[up]), case,
            "a flagged variable is not on its bound")
    rest = free & (obn == 0)
    T.check(np.all(xn[rest] >= lb[rest]) and np.all(xn[rest] <= ub[rest]), case, "x_new outside the box")
    T.check(gc.summary("dogbox", So) == case["info"], case, "the oracle's tr_hit / fallback / clip is not the recorded one")
    return So


def _dogbox_factors(cases, Ps):
    """The oracle's factor of every problem of a batch.  gelsd on the free block takes 0.08 s at 640 x 600 and hardly
    threads: with threadpoolctl at hand the problems are factored side by side on one BLAS thread each (LAPACK releases
    the interpreter lock; 56 problems: 4.6 s -> 0.7 s on eight cores), otherwise one after the other."""
    todo = {}
    for c, P in zip(cases, Ps):
        todo.setdefault((c["cls"], c["seed"]), P)

    def factor(P):
        return orc.dogbox_factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        return {k: factor(P) for k, P in todo.items()}
    from concurrent.futures import ThreadPoolExecutor
    with threadpool_limits(1), ThreadPoolExecutor(8) as ex:
        return dict(zip(todo, ex.map(factor, todo.values())))


def dog_solve(bl, ctx, A, Deltas):
    """One factor call, one step call per entry of `Deltas` on that factor (dogbox.py:203-220 runs inside the loop that
    shrinks Delta on the same J)."""
    B, m, n = A["J"].shape
    sol = bl.DogboxStepSolver(B, m, n, ctx=ctx)
    ctx.gram_stats(reset=True)
    F = sol.factor(A["J"], A["f"], A["x"], A["lb"], A["ub"], A["scale"], A["on_bound"])
    fast, sweeps = sol.debug_fast(), sol.debug_sweeps()
    steps = [sol.step(D) for D in Deltas]
    stats = ctx.gram_stats()
    sol.close()
    return F, steps, stats, fast, sweeps


@pytest.mark.parametrize("route", ["reg", "rl", "tree", "svd", "wide", "short"])
def test_dogbox_route(bl, fix, route_ctx, route):
    """Every problem of a (route, shape) once in ONE batch; its radii are successive step calls on the one factor."""
    ctx = route_ctx(route)
    T = Tally("dogbox", route)
    tr_hits, signs, clips = set(), set(), 0
    first = None
    for (m, n) in gc.ROUTES[route]["dogbox"]:
        cases = [c for c in gc.cases_of(fix, "dogbox", route) if (c["m"], c["n"]) == (m, n)]
        assert cases, (route, m, n)
        at = {}                                                # problem -> its row in the batch
        for c in cases:
            at.setdefault((c["cls"], c["seed"]), len(at))
        heads = [next(c for c in cases if (c["cls"], c["seed"]) == k) for k in at]
        Ps = _problems(heads)
        A = _stack(Ps, ("J", "f", "x", "lb", "ub", "scale", "on_bound"))
        B = len(Ps)
        radii = sorted({c["Delta"] for c in cases})
        own = [{c["Delta"] for c in cases if (c["cls"], c["seed"]) == k} for k in at]
        # (a problem without an admitted case at a radius runs there at one of its own: the call is per batch)
        Deltas = [np.array([D if D in own[b] else min(own[b]) for b in range(B)]) for D in radii]
        F, steps, stats, fast, sweeps = dog_solve(bl, ctx, A, Deltas)
        stepping = np.array([c["cls"] != "all_active" for c in heads])
        print("geometry dogbox %-5s %dx%d: %d problems, %d cases, gram %s, fast %d, most sweeps %d"
              % (route, m, n, B, len(cases), stats, int(fast.sum()),
                 _most_sweeps(np.where(stepping, fast, 1), sweeps)))
        if route in ("reg", "rl", "svd"):
            T.check(stats == (B, 0), cases[0], "gram_stats", stats)
        else:
            T.check(stats == (0, 0), cases[0], "gram_stats", stats)
        if route == "svd":
            T.check(np.all(fast[stepping] == 0) and np.all(sweeps[stepping] > 0), cases[0],
                    "debug_fast / debug_sweeps on the forced route", (fast.tolist(), sweeps.tolist()))
        cache = _dogbox_factors(heads, Ps)
        for c in cases:
            b = at[(c["cls"], c["seed"])]
            So = check_dogbox(T, c, Ps[b], F, steps[radii.index(c["Delta"])], b, cache)
            if So is not None:
                tr_hits.add(int(So.tr_hit)); clips += int(np.any(So.on_bound_free != 0))
                signs |= set(int(v) for v in np.unique(Ps[b]["on_bound"]))
        if first is None:
            first = (heads, A, Deltas, F, steps)
    heads, A, Deltas, F, steps = first
    for b in (0, len(heads) // 2, len(heads) - 1):             # alone in its plan: the bits of the mixed batch
        one = {k: v[b:b + 1] for k, v in A.items()}
        F1, steps1, *_ = dog_solve(bl, ctx, one, [D[b:b + 1] for D in Deltas])
        for S, S1 in zip(steps, steps1):
            for name in ("step", "x_new", "on_bound_new", "tr_hit", "fallback", "predicted_reduction"):
                T.check(np.array_equal(np.asarray(getattr(S1, name))[0], np.asarray(getattr(S, name))[b]), heads[b],
                        "bits alone vs in the batch: " + name)
        T.check(np.array_equal(F1.g[0], F.g[b]), heads[b], "bits alone vs in the batch: g")
    T.report()
    assert not T.bad, T.bad[:20]
    assert tr_hits == {0, 1} and signs >= {-1, 1} and clips > 0, (tr_hits, signs, clips)
