"""Cases of the BVLS tests (tests/test_bvls_cpu.py vets them without a GPU, tests/test_bvls_gpu.py runs them).  Not
collected as a test.

The constructed cases are those of tests/_linear_cases.py (built backwards from x*, kappa(A) = 30, multipliers in
[1, 2]) and more of the same construction at the widths the solve kernel changes its shape at.  The sweep is random:
A with prescribed singular values in [1, kappa], b = A x_t + noise with x_t uniform in [-1, 1]^n and the box
[-0.5, 0.5]^n, so that about half the variables end on a bound.  scipy's BVLS stops when a step lowers the cost by less
than tol * cost, which at kappa >= 1e5 happens before its active set is final on a few draws in a hundred (its cost is
then ABOVE the one reached here: draws 76 and 87 from seed 1000, draw 57 from seed 2000); from the seed below scipy's own
iteration runs to its end on every draw.
"""
import numpy as np

import _linear_cases as lc

EPS = np.finfo(np.float64).eps
KAPPA = 30.0                                   # of every constructed matrix (lc.SIGMA_MAX / lc.SIGMA_MIN)


def x_tolerance(n, xstar, kappa=KAPPA):
    """|x - x*|_inf <= 8 n eps kappa(A) max(1, |x*|_inf): the bound the GPU results are held to; the numpy definition
    is held to 1 / 8 of it."""
    return 8.0 * n * EPS * kappa * max(1.0, float(np.max(np.abs(xstar))))


# the widths of the solve kernel: one entry per lane, both entries, the wave boundary, the largest n
GRAM_NS = (1, 2, 6, 17, 63, 64, 65, 100, 128)
_gram = {}


def gram_case(n):
    """A constructed case of width n (B = 3 problems, one shared matrix of n + 12 rows) with its moments in numpy:
    the dict of ``lc.fit_case`` plus G (n, n) and c (B, n)."""
    if n not in _gram:
        case = lc.fit_case(n + 12, n, 3, True, 7000 + n)
        A = case["A"]
        case["G"] = A.T @ A
        case["c"] = case["b"] @ A
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _gram[n] = case
    return _gram[n]


def weighted_case():
    return lc.fit_case(40, 6, 4, False, 301, sigma=True)


SWEEP_KAPPAS = (30.0, 1e3, 1e5, 1e6)
SWEEP_SHAPES = ((40, 6), (130, 17), (200, 64), (300, 128))
SWEEP_DRAWS = 6
SWEEP_SEED = 3000
OTHER_SWEEP_SEEDS = (1000, 2000)                # kept as drawn: scipy's mask differs on draws 76 and 87, and on draw 57
BOX = 0.5


def draw(m, n, kappa, seed):
    """-> A (m, n) with singular values log-spaced over [1, kappa], b (m,)."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (U * np.logspace(np.log10(kappa), 0.0, n)) @ V.T
    xt = rng.uniform(-1.0, 1.0, n)
    return A, A @ xt + 0.1 * rng.standard_normal(m)


def sweep(base=None):
    """(kappa, m, n, seed) of the 96 draws from `base` (None: SWEEP_SEED)."""
    base = SWEEP_SEED if base is None else base
    k = 0
    for kappa in SWEEP_KAPPAS:
        for (m, n) in SWEEP_SHAPES:
            for _ in range(SWEEP_DRAWS):
                k += 1
                yield kappa, m, n, base + k


# the two draws of the conditioning test: (130, 17) at kappa = 1e5
CONDITIONING = ((1e5, 130, 17, 5001), (1e5, 130, 17, 5002))


# Narrow boxes: a released variable can cross its whole interval and land on the OPPOSITE bound, the first one dropped
# in its own pass, after a step of positive length.  n in 2 .. 7, m up to n + 11, kappa in 25 .. 140, box half-width
# in 0.01 .. 0.2, every seed of a range kept.
NARROW_SEEDS = range(1000)
_narrow = {}


def narrow(seed):
    """-> A (m, n), b (m,), the half-width of the box."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 8))
    m = n + int(rng.integers(2, 12))
    kappa, box = 10.0 ** rng.uniform(1.4, 2.15), 10.0 ** rng.uniform(-2.0, -0.7)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (U * np.logspace(np.log10(kappa), 0.0, n)) @ V.T
    return A, A @ rng.uniform(-1.0, 1.0, n) + 0.1 * rng.standard_normal(m), box


def narrow_with_scipy(seed):
    """``narrow(seed)`` and scipy's BVLS on it (tol = 1e-14), solved once per process: A, b, box, scipy's result."""
    if seed not in _narrow:
        from scipy import optimize
        A, b, box = narrow(seed)
        _narrow[seed] = (A, b, box, optimize.lsq_linear(A, b, (-box, box), method="bvls", tol=1e-14))
    return _narrow[seed]


def kkt_optimality(g, on):
    """max(max over free |g_j|, max over bound g_j on_j, 0): scipy's compute_kkt_optimality."""
    return max(float(np.max(np.where(on == 0, np.abs(g), g * on))), 0.0)


def kkt_bound(G, c, x, tol=1e-10):
    """What the optimality of a point the iteration calls optimal may be, from g = G x - c: `tol` on the bound
    variables, and on the free ones the residual of a backward-stable Cholesky solve plus the rounding of the gradient
    itself, 16 n eps max_j (|G||x| + |c|)_j (the constant covers the factor, two substitutions and the product)."""
    n = len(c)
    return tol + 16.0 * n * EPS * float(np.max(np.abs(G) @ np.abs(x) + np.abs(c)))


def agrees_with_scipy(A, b, x, on, s):
    """The masks are equal, or the cost at x is not above scipy's (it stops on a small relative gain, or on its
    iteration count, before its active set is final on a few draws in a thousand)."""
    cost = 0.5 * float(np.sum((A @ x - b) ** 2))
    return np.array_equal(on, s.active_mask) or cost <= s.cost * (1.0 + 64 * EPS)


def singular_case():
    """G = A^T A of a matrix with a duplicated column, in small integers so that every product, sum, square root and
    quotient of its factorisation is exact in any order: the second pivot is exactly 0.  -> G (3, 3), c (3, 3) for
    B = 3 problems, lb, ub."""
    A = np.array([[2.0, 2.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    b = np.array([[1.0, 2.0, 3.0, 0.5], [-1.0, 0.0, 1.0, 0.0], [4.0, -2.0, 0.0, 1.0]])
    return A.T @ A, b @ A, -1.0, 1.0


def csne_finish(A, b, x, on, lb, ub):
    """The finish of the whole path in numpy: one corrected-semi-normal-equations step on the free variables,
    x_F += (A_F^T A_F)^-1 A_F^T (b - A x), with the Cholesky factor of the Gram block, then the clamp."""
    F = np.flatnonzero(on == 0)
    x = np.array(x, dtype=np.float64)
    if F.size:
        L = np.linalg.cholesky(A[:, F].T @ A[:, F])
        t = A[:, F].T @ (b - A @ x)
        x[F] += np.linalg.solve(L.T, np.linalg.solve(L, t))
        x = np.clip(x, lb, ub)
    return x


def moments_reference(A, y, w):
    """G and c in numpy.longdouble with the magnitudes their error bounds are relative to: A (m, n) or (B, m, n),
    y (B, m), w None, (m,) or (B, m) -> G, |A|^T W^2 |A| (n, n) or (B, n, n), c, |A|^T W^2 |y| (B, n).  G has no batch
    axis iff A is shared and w is not per problem."""
    L = np.longdouble
    Al, yl = np.asarray(A, dtype=L), np.asarray(y, dtype=L)
    B = yl.shape[0]
    w2 = None if w is None else np.asarray(w, dtype=L) ** 2
    per = Al.ndim == 3 or (w2 is not None and w2.ndim == 2)
    if per:
        A3 = np.broadcast_to(Al if Al.ndim == 3 else Al[None], (B,) + Al.shape[-2:])
        W = np.ones((B, A3.shape[1]), dtype=L) if w2 is None else np.broadcast_to(w2, (B, A3.shape[1]))
        WA = W[:, :, None] * A3
        G = np.einsum("bij,bik->bjk", WA, A3)
        Gm = np.einsum("bij,bik->bjk", np.abs(WA), np.abs(A3))
        c = np.einsum("bij,bi->bj", WA, yl)
        cm = np.einsum("bij,bi->bj", np.abs(WA), np.abs(yl))
    else:
        WA = Al if w2 is None else w2[:, None] * Al
        G, Gm = WA.T @ Al, np.abs(WA).T @ np.abs(Al)
        c, cm = yl @ WA, np.abs(yl) @ np.abs(WA)
    return G, Gm, c, cm
