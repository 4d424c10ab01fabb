"""Cases of the tests of BVLS / NNLS with a sum constraint (tests/test_fcls_cpu.py vets them without a GPU,
tests/test_fcls_gpu.py runs them).  Not collected as a test.

The constructed cases are built BACKWARDS as ``_linear_cases.fit_case`` builds its own: choose x* inside the box with a
prescribed active set, multipliers in [1, 2] on the bound variables and a multiplier lambda* of the equality; the
gradient at x* must then be g* = -(multipliers on) - lambda* e (so that (g* + lambda* e) on = -multipliers: no bound
variable wants to leave), and b = A x* - r* with A^T r* = g*.  kappa(A) = 30 (``lc.matrix``), m = n + 12, B = 3, d = e^T x*.
The exact x*, active set and lambda* are known.

The brute-force search solves the KKT system of EVERY active set (3^n of them) in numpy.longdouble and keeps the feasible
candidate of least cost: the minimiser is a candidate with its own active set, and no feasible point costs less.
"""
import itertools

import numpy as np

import _bvls_cases as bc
import _linear_cases as lc

EPS = np.finfo(np.float64).eps
L = np.longdouble


# ---- constructed cases ----------------------------------------------------------------------------------------------
_made = {}


def fit_case(m, n, B, shared, seed, sigma=False, simplex=False):
    """dict(A (m, n) or (B, m, n), b (B, m), lb, ub (B, n), e (n,), d (B,), xstar (B, n), active (B, n), lam (B,),
    sigma None or (m,)).  n == 1: the variable is free and pinned by the equality; else max(1, n // 4) variables are on
    a bound.  simplex: lb = 0, ub = inf, e = 1 and x* scaled to sum to 1."""
    rng = np.random.default_rng(seed)
    A = lc.matrix(rng, m, n) if shared else np.stack([lc.matrix(rng, m, n) for _ in range(B)])
    sg = rng.uniform(0.5, 2.0, m) if sigma else None
    k = 0 if n == 1 else max(1, n // 4)
    if simplex:
        lb, ub = np.zeros((B, n)), np.full((B, n), np.inf)
        e = np.ones(n)
        xstar = rng.uniform(0.3, 0.7, (B, n))
    else:
        lb = -1.0 + 0.2 * rng.uniform(-1, 1, (B, n))
        ub = 1.0 + 0.2 * rng.uniform(-1, 1, (B, n))
        e = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.5, 2.0, n)
        xstar = lb + (ub - lb) * rng.uniform(0.3, 0.7, (B, n))
    active = np.zeros((B, n), dtype=int)
    lam = rng.uniform(-1.5, 1.5, B)
    b = np.empty((B, m))
    for p in range(B):
        S = rng.choice(n, size=k, replace=False)
        side = -np.ones(k, dtype=int) if simplex else rng.choice([-1, 1], size=k)
        active[p, S] = side
        xstar[p, S] = np.where(side < 0, lb[p, S], ub[p, S])
        if simplex:
            xstar[p] /= xstar[p].sum()
        g = -lam[p] * e
        g[S] += -side * rng.uniform(1.0, 2.0, k)
        Ap = A if shared else A[p]
        Aw = Ap if sg is None else Ap / sg[:, None]
        Q, R = np.linalg.qr(Aw)
        r = Q @ np.linalg.solve(R.T, g)
        z = rng.standard_normal(m)
        z -= Q @ (Q.T @ z)
        r = r + 0.05 * z / np.linalg.norm(z)
        bw = Aw @ xstar[p] - r
        b[p] = bw if sg is None else bw * sg
    d = xstar @ e
    return dict(A=A, b=b, lb=lb, ub=ub, e=e, d=d, xstar=xstar, active=active, lam=lam, sigma=sg, m=m, n=n, B=B,
                shared=shared)


def _frozen(key, make):
    if key not in _made:
        case = make()
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _made[key] = case
    return _made[key]


def gram_case(n):
    """The constructed case of width n (B = 3, one shared matrix of n + 12 rows) with its moments in numpy."""
    def make():
        case = fit_case(n + 12, n, 3, True, 9000 + n)
        case["G"] = case["A"].T @ case["A"]
        case["c"] = case["b"] @ case["A"]
        return case
    return _frozen(("gram", n), make)


# whole-path cases: A shared and per problem, sigma (m,); the (B, m) form of sigma is the same values replicated
WHOLE = {"18x6-shared": dict(m=18, n=6, B=3, shared=True, seed=9101),
         "29x17-own": dict(m=29, n=17, B=3, shared=False, seed=9102),
         "77x65-shared-sigma": dict(m=77, n=65, B=3, shared=True, seed=9103, sigma=True),
         "18x6-own-sigma": dict(m=18, n=6, B=3, shared=False, seed=9104, sigma=True),
         "140x128-shared": dict(m=140, n=128, B=3, shared=True, seed=9105)}


def whole_case(name):
    return _frozen(("whole", name), lambda: fit_case(**WHOLE[name]))


def simplex_case(seed=11):
    """Unmixing against the library of ``lc.nnls_case`` (5 non-negative columns, two components absent) with abundances
    that sum to one: x* = (0.5, 0.3, 0.2, 0, 0), multipliers 1.5 and 2 on the absent ones, lambda* = 0.7."""
    def make():
        rng = np.random.default_rng(seed)
        A = lc.nnls_case()["A"]
        m, n = A.shape
        xstar = np.array([0.5, 0.3, 0.2, 0.0, 0.0])
        lam = 0.7
        g = -lam * np.ones(n) + np.array([0.0, 0.0, 0.0, 1.5, 2.0])
        Q, R = np.linalg.qr(A)
        z = rng.standard_normal(m)
        z -= Q @ (Q.T @ z)
        r = Q @ np.linalg.solve(R.T, g) + 0.05 * z / np.linalg.norm(z)
        return dict(A=A, b=A @ xstar - r, xstar=xstar, lam=lam, m=m, n=n, kappa=float(np.linalg.cond(A)),
                    active=np.array([0, 0, 0, -1, -1]))
    return _frozen(("simplex", seed), make)


# ---- brute force ----------------------------------------------------------------------------------------------------
def _solve_ld(M, r):
    """Gaussian elimination with partial pivoting in numpy.longdouble (numpy's solvers are double only)."""
    M, r = np.array(M, dtype=L), np.array(r, dtype=L)
    k = len(r)
    for i in range(k):
        p = i + int(np.argmax(np.abs(M[i:, i])))
        if M[p, i] == 0:
            return None
        if p != i:
            M[[i, p]], r[[i, p]] = M[[p, i]], r[[p, i]]
        for q in range(i + 1, k):
            f = M[q, i] / M[i, i]
            M[q, i:] -= f * M[i, i:]
            r[q] -= f * r[i]
    out = np.zeros(k, dtype=L)
    for i in range(k - 1, -1, -1):
        out[i] = (r[i] - M[i, i + 1:] @ out[i + 1:]) / M[i, i]
    return out


def kkt_on_active_set(G, c, lb, ub, e, d, on):
    """The stationary point of the equality-constrained problem with the variables of `on` != 0 held on their bounds,
    in numpy.longdouble -> (x, lambda); lambda is None with no free variable; None: a bound is infinite."""
    n = len(c)
    Gl, cl, el = np.asarray(G, dtype=L), np.asarray(c, dtype=L), np.asarray(e, dtype=L)
    x = np.zeros(n, dtype=L)
    F, Bd = np.flatnonzero(on == 0), np.flatnonzero(on != 0)
    x[Bd] = np.where(on[Bd] < 0, lb[Bd], ub[Bd])
    if not np.all(np.isfinite(x)):
        return None
    if F.size == 0:
        return x, None
    k = F.size
    M = np.zeros((k + 1, k + 1), dtype=L)
    M[:k, :k] = Gl[np.ix_(F, F)]
    M[:k, k] = M[k, :k] = el[F]
    rhs = np.concatenate([cl[F] - Gl[np.ix_(F, Bd)] @ x[Bd], [L(d) - el[Bd] @ x[Bd]]])
    sol = _solve_ld(M, rhs)
    if sol is None:
        return None
    x[F] = sol[:k]
    return x, sol[k]


def kkt_from_matrix(A, b, lb, ub, e, d, on, sweeps=4):
    """``kkt_on_active_set`` for min 1/2 |A x - b|^2 at a conditioning the Gram matrix squares: the longdouble solve of
    the KKT system, then `sweeps` steps of iterative refinement whose residual A_F^T (b - A x) - lambda e_F is formed
    from A itself in longdouble, so that the answer carries kappa(A) and not kappa(A)^2 -> (x, lambda)."""
    Al, bl, el = np.asarray(A, dtype=L), np.asarray(b, dtype=L), np.asarray(e, dtype=L)
    G, c = Al.T @ Al, Al.T @ bl
    x, lam = kkt_on_active_set(G, c, lb, ub, e, d, on)
    F = np.flatnonzero(on == 0)
    if F.size == 0:
        return x, lam
    k = F.size
    M = np.zeros((k + 1, k + 1), dtype=L)
    M[:k, :k] = G[np.ix_(F, F)]
    M[:k, k] = M[k, :k] = el[F]
    for _ in range(sweeps):
        res = np.concatenate([Al[:, F].T @ (bl - Al @ x) - lam * el[F], [L(d) - el @ x]])
        step = _solve_ld(M, res)
        x[F] += step[:k]
        lam = lam + step[k]
    return x, lam


def lam_tolerance(G, n, xstar, e, kappa=bc.KAPPA):
    """|lambda - lambda*|: the multiplier is a weighted mean of -g_j / e_j over the free set and g moves by G dx, so an
    x within ``bc.x_tolerance`` of x* puts lambda within |G|_inf x_tolerance / min |e_j| of lambda*."""
    return float(np.max(np.sum(np.abs(G), axis=1))) * bc.x_tolerance(n, xstar, kappa) / float(np.min(np.abs(e)))


def brute_force(G, c, lb, ub, e, d, feas=1e-12):
    """The minimiser by a search over all 3^n active sets -> (x, cost) in longdouble, or None: infeasible."""
    n = len(c)
    Gl, cl = np.asarray(G, dtype=L), np.asarray(c, dtype=L)
    scale = max(1.0, abs(d), float(np.max(np.abs(e))))
    best = None
    for on in itertools.product((-1, 0, 1), repeat=n):
        on = np.array(on)
        cand = kkt_on_active_set(G, c, lb, ub, e, d, on)
        if cand is None:
            continue
        x = cand[0]
        slack = feas * max(scale, float(np.max(np.abs(x))))
        if np.any(x < lb - slack) or np.any(x > ub + slack) or abs(float(np.asarray(e, dtype=L) @ x - d)) > slack * n:
            continue
        cost = 0.5 * x @ (Gl @ x) - cl @ x
        if best is None or cost < best[1]:
            best = (x, cost)
    return best


KINDS = ("simplex", "box", "signed")
BRUTE_DRAWS = 110                               # per kind: 330 draws in all


def brute_draw(kind, seed):
    """A small problem of one of the three kinds -> G, c, lb, ub, e, d (n in 1 .. 5, kappa(A) = 30)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 6))
    A = lc.matrix(rng, n + int(rng.integers(1, 8)), n) / lc.SIGMA_MIN
    b = A @ rng.uniform(-1.0, 1.0, n) + 0.3 * rng.standard_normal(A.shape[0])
    if kind == "simplex":
        lb, ub, e, d = np.zeros(n), np.full(n, np.inf), np.ones(n), 1.0
    elif kind == "box":
        w = rng.uniform(0.1, 1.0, n)
        lb, ub, e = -w, w, np.ones(n)
        d = float(rng.uniform(-1.2, 1.2) * w.sum())              # beyond +-sum(w): infeasible
    else:
        lb = -rng.uniform(0.1, 1.0, n)
        ub = rng.uniform(0.1, 1.0, n)
        lb[rng.random(n) < 0.2] = -np.inf
        ub[rng.random(n) < 0.2] = np.inf
        e = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-1.0, 1.0, n)
        d = float(rng.uniform(-1.0, 1.0) * np.sum(np.abs(e)) * 0.6)
    return A.T @ A, A.T @ b, lb, ub, e, d


def feasible(lb, ub, e, d):
    """Whether e^T x = d has a solution in the box (the range of e^T x over the box, exactly enough for the draws)."""
    lo = np.sum(np.where(e > 0, e * lb, e * ub))
    hi = np.sum(np.where(e > 0, e * ub, e * lb))
    return lo <= d <= hi


# ---- the certificate ------------------------------------------------------------------------------------------------
def multiplier_ld(g, on, e):
    """The reported multiplier recomputed in longdouble from a gradient: least squares over the free set; with no free
    variable the midpoint of the admissible interval (its finite end when only one is)."""
    g, e = np.asarray(g, dtype=L), np.asarray(e, dtype=L)
    F = on == 0
    if F.any():
        return -(e[F] @ g[F]) / (e[F] @ e[F])
    q = -g / e
    up = on * e > 0
    hi = np.min(q[up]) if up.any() else np.inf
    lo = np.max(q[~up]) if (~up).any() else -np.inf
    if np.isfinite(lo) and np.isfinite(hi):
        return (lo + hi) / 2
    return lo if np.isfinite(lo) else (hi if np.isfinite(hi) else L(0))


def optimality_ld(g, on, e, lam):
    r = np.asarray(g, dtype=L) + lam * np.asarray(e, dtype=L)
    return max(float(np.max(np.where(on == 0, np.abs(r), r * on))), 0.0)


def kkt_bound(G, c, x, e, lam, tol=1e-10):
    """``bc.kkt_bound`` with |lambda| |e| added to its scale term: the reduced gradient g + lambda e has one more term
    to round."""
    n = len(c)
    return tol + 16.0 * n * EPS * float(np.max(np.abs(G) @ np.abs(x) + np.abs(c) + abs(float(lam)) * np.abs(e)))


def sum_bound(e, x):
    """|e^T x - d| <= 4 n eps sum |e_j x_j|"""
    return 4.0 * len(x) * EPS * float(np.sum(np.abs(e * x)))


def conditioning_case(draw):
    """A draw of ``bc.CONDITIONING`` with e = 1 and d = e^T clip(x_ls) -> A, b, d."""
    kappa, m, n, seed = draw
    A, b = bc.draw(m, n, kappa, seed)
    xls = np.linalg.lstsq(A, b, rcond=None)[0]
    return A, b, float(np.sum(np.clip(xls, -bc.BOX, bc.BOX)))
