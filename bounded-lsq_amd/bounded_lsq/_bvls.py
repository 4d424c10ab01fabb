"""`bvls_batch`, `bvls`, `nnls_batch`, `fcls_batch`, `bvls_gram_batch`: bounded-variable least squares by an exact
active-set method, a whole batch in two calls of the library, optionally under one linear equality
``e^T x = d`` (``equality=(e, d)``).

``min 1/2 |W (A x - b)|^2, lb <= x <= ub`` is a strictly convex quadratic programme in the moments ``G = A^T W^2 A``
and ``c = A^T W^2 b``.  The iteration of Stark and Parker (Lawson and Hanson's NNLS is its ``(0, inf)`` case) reaches the
exact minimiser and the exact active set in finitely many steps: a variable on a bound holds ``lb`` or ``ub`` bit for
bit.  One call forms the moments (blsq_bvls_moments_dev), one launch runs every problem's whole iteration in a
workgroup of its own (blsq_bvls_solve_dev) and, where `A` is given, corrects the answer once against `A` itself, which
takes back the conditioning the normal equations squared.  Nothing crosses to the host in between.

``bvls_reference`` is the numpy definition of the iteration.  There is no host route.
"""
import numpy as np

from . import _abi
from ._batch import _bounds_2d
from ._linear import _checked_problem

__all__ = ['bvls_batch', 'bvls', 'nnls_batch', 'fcls_batch', 'bvls_gram_batch', 'bvls_reference', 'BvlsResult',
           'BVLS_MAX_N']

BVLS_MAX_N = 128                               # BLSQ_BVLS_MAX_N of include/blsq.h

MESSAGES = {1: "No variable on a bound wants to leave it, and the free ones solve their normal equations.",
            0: "The maximum number of release passes is exceeded.",
            -1: "A free block is not positive definite in floating point, or a value is not finite.",
            -2: "The equality constraint cannot be met inside the bounds."}


def _cholesky(M):
    """Lower Cholesky factor of M column by column, or None when a pivot is <= 0 or not finite."""
    k = M.shape[0]
    L = np.zeros((k, k))
    for j in range(k):
        col = M[j:, j] - L[j:, :j] @ L[j, :j]
        d = col[0]
        if not (d > 0.0 and np.isfinite(d)):
            return None
        L[j:, j] = col / np.sqrt(d)
    return L


def _tri_solve(L, r):
    """(L L^T)^-1 r by the two substitutions the kernel runs."""
    k = len(r)
    y = np.array(r, dtype=np.float64)
    for t in range(k):
        y[t] /= L[t, t]
        y[t + 1:] -= L[t + 1:, t] * y[t]
    for t in range(k - 1, -1, -1):
        y[t] /= L[t, t]
        y[:t] -= L[t, :t] * y[t]
    return y


def bvls_reference(G, c, lb, ub, tol=1e-10, max_iter=None, equality=None):
    """The iteration on one problem, in numpy, decision for decision: G (n, n) symmetric, c, lb, ub (n,).

    State: x and on_bound in {-1, 0, 1}.  (1) Clip-in start: all variables free; solve on the free set F; every free
    variable whose solution lies outside its bounds goes to that bound exactly and leaves F; repeat until a solve
    violates nothing or F is empty.  (2) Release pass: g = G x - c; of the variables on a bound that are not barred take
    the largest g_j on_bound_j (lowest index on ties); not > tol: status 1; else free it.  (3) Drop loop: solve on F; z
    inside the bounds: x_F = z, bars cleared, the pass ends; else the smallest alpha_i = (bound_i - x_i) / (z_i - x_i)
    over the violators (lowest index on ties, clamped to [0, 1]) moves x_F, its variable goes to its bound exactly and
    the rest of x_F is clamped into the box.  The released variable, when it is the first one dropped in its own pass, is
    barred from release until a pass ends with an accepted z; when it fell back with alpha = 0 onto the bound it left,
    x and F are those before the pass, which ends there (a further solve would accept and clear the bar at once).  When
    no other variable wants to leave its bound the bars are cleared and the barred ones are asked again: status 1 is
    returned only when no variable on a bound wants to leave it.

    Every loop is bounded: the start by n + 1 solves, the passes by `max_iter` (None: 5 n), the drop loop by n + 1
    rounds.  Status 1: KKT holds; 0: `max_iter` passes used; -1: a pivot <= 0 or not finite, or a value not finite (x is
    then the last feasible iterate).
    -> dict(x, on_bound, status, nit (release passes), nfact (factorisations), g (= G x - c at the end)).

    equality : None, or a pair (e, d): the iteration under ``e^T x = d`` as well (`_reference_eq` below has its rules);
    the dict then also holds ``multiplier`` and ``optimality``."""
    G = np.asarray(G, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[0]
    lb = np.broadcast_to(np.asarray(lb, dtype=np.float64), (n,))
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (n,))
    max_iter = 5 * n if max_iter is None else int(max_iter)
    if equality is not None:
        e = np.broadcast_to(np.asarray(equality[0], dtype=np.float64), (n,))
        return _reference_eq(G, c, lb, ub, e, float(equality[1]), tol, max_iter)
    x = np.clip(np.zeros(n), lb, ub)
    on = np.zeros(n, dtype=np.int32)
    barred = np.zeros(n, dtype=bool)
    count = dict(nit=0, nfact=0)

    def solve():
        """z over the free set (full length; bound entries are x), or None."""
        F = np.flatnonzero(on == 0)
        Bd = np.flatnonzero(on != 0)
        z = x.copy()
        if F.size == 0:
            return z
        count["nfact"] += 1
        L = _cholesky(G[np.ix_(F, F)])
        if L is None:
            return None
        zF = _tri_solve(L, c[F] - G[np.ix_(F, Bd)] @ x[Bd])
        if not np.all(np.isfinite(zF)):
            return None
        z[F] = zF
        return z

    def to_bound(j, side):
        on[j] = side
        x[j] = lb[j] if side < 0 else ub[j]

    def finish(status):
        return dict(x=x, on_bound=on, status=status, nit=count["nit"], nfact=count["nfact"], g=G @ x - c)

    for _ in range(n + 1):                                           # (1) clip-in start
        z = solve()
        if z is None:
            return finish(-1)
        low, high = (on == 0) & (z < lb), (on == 0) & (z > ub)
        keep = (on == 0) & ~low & ~high
        x[keep] = z[keep]
        for j in np.flatnonzero(low | high):
            to_bound(j, -1 if low[j] else 1)
        if not np.any(low | high):
            break
    while True:                                                      # (2) release passes
        g = G @ x - c
        if not np.all(np.isfinite(g)):
            return finish(-1)
        cand = np.flatnonzero((on != 0) & ~barred)
        if not (cand.size and np.max(g[cand] * on[cand]) > tol) and barred.any():
            barred[:] = False                                        # nothing else wants to leave: the barred ones are
            cand = np.flatnonzero(on != 0)                           # asked again, so that status 1 means KKT holds
        if cand.size == 0:
            return finish(1)
        v = g[cand] * on[cand]
        j = cand[int(np.argmax(v))]                                  # (argmax: the first of equal values)
        if not g[j] * on[j] > tol:
            return finish(1)
        if count["nit"] >= max_iter:
            return finish(0)
        count["nit"] += 1
        left = on[j]
        on[j] = 0
        first = True
        for _ in range(n + 1):                                       # (3) drop loop
            z = solve()
            if z is None:
                return finish(-1)
            free = on == 0
            low, high = free & (z < lb), free & (z > ub)
            viol = np.flatnonzero(low | high)
            if viol.size == 0:
                x[free] = z[free]
                barred[:] = False
                break
            bound = np.where(low, lb, ub)
            alpha = (bound[viol] - x[viol]) / (z[viol] - x[viol])
            i = viol[int(np.argmin(alpha))]
            a = min(max(alpha.min(), 0.0), 1.0)
            x[free] = np.clip(x[free] + a * (z[free] - x[free]), lb[free], ub[free])
            to_bound(i, -1 if low[i] else 1)
            if first and i == j:
                barred[j] = True
                if a == 0.0 and on[j] == left:                       # back where the pass began: nothing to solve again
                    break
            first = False
        else:
            return finish(-1)                                        # (unreachable: every round removes a variable)


def _feasible_start(lb, ub, e, d):
    """x = clip(0, lb, ub); the gap d - e^T x (ascending j) is walked off in ascending j: a variable takes the whole of
    what is left, gap / e_j, when its room towards the bound on that side allows it (clamped into the box against the
    rounding of x_j + step), and else goes to that bound exactly.  -> x, 2; or the clipped start and -1 (e with a zero,
    e, d or a step not finite) or -2 (the gap cannot be absorbed)."""
    n = len(lb)
    x0 = np.clip(np.zeros(n), lb, ub)
    if not (np.all(np.isfinite(e)) and np.all(e != 0.0) and np.isfinite(d)):
        return x0, -1
    x = x0.copy()
    gap = d
    for j in range(n):
        gap = gap - e[j] * x[j]
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(n):
            if gap == 0.0:
                break
            step = gap / e[j]
            if not (np.isfinite(gap) and np.isfinite(step)):
                return x0, -1
            bound = ub[j] if step > 0.0 else lb[j]
            room = bound - x[j]
            if abs(step) <= abs(room):
                x[j] = min(max(x[j] + step, lb[j]), ub[j])
                gap = 0.0
                break
            x[j] = bound
            gap = gap - e[j] * room
    if not np.isfinite(gap):
        return x0, -1
    return (x, 2) if gap == 0.0 else (x0, -2)


def _lambda_interval(g, on, e):
    """With every variable on a bound the multipliers that satisfy (g_j + lambda e_j) on_j <= 0 for all j are the
    interval [lo, hi]: hi the minimum of -g_j / e_j over on_j e_j > 0, lo the maximum over the others."""
    q = -g / e
    up = on * e > 0.0
    hi = float(np.min(q[up])) if up.any() else np.inf
    lo = float(np.max(q[~up])) if (~up).any() else -np.inf
    return lo, hi


def _multiplier(g, on, e):
    """The multiplier reported: least squares over the free set, -e_F^T g_F / e_F^T e_F; with no free variable the
    midpoint of `_lambda_interval`, its finite end when only one is, 0 when neither is."""
    F = on == 0
    if F.any():
        return float(-(e[F] @ g[F]) / (e[F] @ e[F]))
    lo, hi = _lambda_interval(g, on, e)
    if np.isfinite(lo) and np.isfinite(hi):
        return 0.5 * (lo + hi)
    return lo if np.isfinite(lo) else (hi if np.isfinite(hi) else 0.0)


def _reference_eq(G, c, lb, ub, e, d, tol, max_iter):
    """``bvls_reference`` under one equality e^T x = d (every e_j finite and not zero).

    (1) `_feasible_start`; on_bound_j = -1 where x_j == lb_j, +1 where x_j == ub_j, else 0.  (2) A solve on the free set
    F with the bound set B: u = G_FF^-1 (c_F - G_FB x_B), v = G_FF^-1 e_F, lambda = (e_F^T u - (d - e_B^T x_B)) /
    (e_F^T v), z_F = u - lambda v; e_F^T v not positive or not finite: status -1.  A free set of ONE variable j is pinned by
    the equality: its z is (d - e_B^T x_B) / e_j, one rounding from the sum, clamped into the box (it can leave it by
    rounding only), so that solve is always accepted; lambda is still the one above.
    (3) The first pass is a drop loop with no release; then release passes as in ``bvls_reference``, the release test
    reading (g_j + lambda e_j) on_bound_j with the lambda of the last accepted solve.  With F empty lambda comes from
    `_lambda_interval`: lo <= hi + tol is status 1, else lambda is the midpoint.  A drop loop that empties F clears the
    bars, as it does without the equality.  (An accepted solve is the only way a drop loop ends with F not empty and x
    changed, so the stored lambda always belongs to the current F and x.)
    -> the dict of ``bvls_reference`` plus multiplier (`_multiplier` of the final g) and optimality =
    max(max_F |g_j + multiplier e_j|, max_B (g_j + multiplier e_j) on_bound_j, 0).  Status -2: the equality cannot be met
    inside the box; x is then the clipped start."""
    n = c.shape[0]
    x, start = _feasible_start(lb, ub, e, d)
    on = np.where(x == lb, -1, np.where(x == ub, 1, 0)).astype(np.int32)
    barred = np.zeros(n, dtype=bool)
    count = dict(nit=0, nfact=0)
    lam = [0.0]

    def finish(status):
        with np.errstate(all="ignore"):
            g = G @ x - c
            mult = _multiplier(g, on, e)
            r = g + mult * e
            opt = max(float(np.max(np.where(on == 0, np.abs(r), r * on))), 0.0) if np.all(np.isfinite(r)) else np.nan
        return dict(x=x, on_bound=on, status=status, nit=count["nit"], nfact=count["nfact"], g=g, multiplier=mult,
                    optimality=opt)

    def solve():
        """(z over the free set (full length; bound entries are x), lambda), or None."""
        F = np.flatnonzero(on == 0)
        Bd = np.flatnonzero(on != 0)
        count["nfact"] += 1
        L = _cholesky(G[np.ix_(F, F)])
        if L is None:
            return None
        u = _tri_solve(L, c[F] - G[np.ix_(F, Bd)] @ x[Bd])
        v = _tri_solve(L, e[F])
        ev = e[F] @ v
        if not (ev > 0.0 and np.isfinite(ev)):
            return None
        dF = d - e[Bd] @ x[Bd]
        l = (e[F] @ u - dF) / ev
        zF = u - l * v
        if not (np.all(np.isfinite(zF)) and np.isfinite(l)):
            return None
        z = x.copy()
        z[F] = np.clip(dF / e[F], lb[F], ub[F]) if F.size == 1 else zF
        return z, l

    def to_bound(j, side):
        on[j] = side
        x[j] = lb[j] if side < 0 else ub[j]

    def drop_loop(j, left):
        """The drop loop of a pass that released j from the side `left` (j < 0: nothing released) -> False: status -1."""
        first = j >= 0
        for _ in range(n + 1):
            if not np.any(on == 0):
                barred[:] = False
                return True
            s = solve()
            if s is None:
                return False
            z, l = s
            free = on == 0
            low, high = free & (z < lb), free & (z > ub)
            viol = np.flatnonzero(low | high)
            if viol.size == 0:
                x[free] = z[free]
                barred[:] = False
                lam[0] = l
                return True
            bound = np.where(low, lb, ub)
            alpha = (bound[viol] - x[viol]) / (z[viol] - x[viol])
            i = viol[int(np.argmin(alpha))]
            a = min(max(alpha.min(), 0.0), 1.0)
            x[free] = np.clip(x[free] + a * (z[free] - x[free]), lb[free], ub[free])
            to_bound(i, -1 if low[i] else 1)
            if first and i == j:
                barred[j] = True
                if a == 0.0 and on[j] == left:
                    return True
            first = False
        return False                                                 # (unreachable: every round removes a variable)

    if start != 2:
        return finish(start)
    if not drop_loop(-1, 0):
        return finish(-1)
    while True:
        g = G @ x - c
        if not np.all(np.isfinite(g)):
            return finish(-1)
        if np.any(on == 0):
            l = lam[0]
        else:
            lo, hi = _lambda_interval(g, on, e)
            if lo <= hi + tol:
                return finish(1)
            l = 0.5 * (lo + hi)
        r = (g + l * e) * on
        cand = np.flatnonzero((on != 0) & ~barred)
        if not (cand.size and np.max(r[cand]) > tol) and barred.any():
            barred[:] = False
            cand = np.flatnonzero(on != 0)
        if cand.size == 0:
            return finish(1)
        j = cand[int(np.argmax(r[cand]))]
        if not r[j] > tol:
            return finish(1)
        if count["nit"] >= max_iter:
            return finish(0)
        count["nit"] += 1
        left = on[j]
        on[j] = 0
        if not drop_loop(j, left):
            return finish(-1)


class BvlsResult:
    """The results of a batch as arrays over the problems (a batch is 1e5 to 1e6 problems: not a list of objects):
    x (B, n), cost (B,) = 0.5 fun @ fun, fun (B, m) = w (A x - b) or None, optimality (B,), active_mask (B, n) in
    {-1, 0, 1}, nit (B,) the release passes, nfact (B,) the factorisations, status (B,), success (B,), multiplier (B,)
    the multiplier of the equality (None without ``equality=``; `optimality` is then of g + multiplier e).  ``res[p]``
    is problem p with scipy's names (and ``message``).

    ``cost``: with `fun`, ``0.5 * numpy.dot(fun[p], fun[p])`` of the returned residuals, scipy's definition in numpy's
    own summation order, formed on first use; without (``fun=False``) the kernel's sum of the same squares in its own
    order (``device_cost``, always there), within 2 gamma_m of the other."""
    FIELDS = ('x', 'cost', 'fun', 'optimality', 'active_mask', 'nit', 'nfact', 'status', 'success', 'multiplier')

    def __init__(self, device_cost=None, cost=None, **kw):
        self.device_cost, self._cost = device_cost, cost
        for k in self.FIELDS:
            if k != 'cost':
                setattr(self, k, kw.get(k))

    @property
    def cost(self):
        if self._cost is None and self.fun is not None:
            self._cost = np.array([0.5 * np.dot(f, f) for f in self.fun])
        return self.device_cost if self._cost is None else self._cost

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, p):
        p = int(p)
        if not -len(self) <= p < len(self):
            raise IndexError(p)
        one = _OneResult()
        for k in self.FIELDS:
            if k == 'cost':
                continue
            v = getattr(self, k)
            setattr(one, k, None if v is None else v[p])
        if self.fun is not None and self._cost is None:
            one.cost = 0.5 * np.dot(self.fun[p], self.fun[p])
        else:
            one.cost = None if self.cost is None else self.cost[p]
        one.message = MESSAGES[int(one.status)]
        return one


class _OneResult:
    def __repr__(self):
        return "\n".join("%12s: %r" % kv for kv in vars(self).items())


def _checked_size(n):
    if not 1 <= n <= BVLS_MAX_N:
        raise ValueError("`bvls_batch` takes 1 <= n <= %d variables (got %d): use `lsq_linear_batch`." % (BVLS_MAX_N, n))


def _checked_bounds(bounds, B, n):
    try:
        return _bounds_2d(bounds, B, n)
    except ValueError as e:
        if "bound" in str(e):
            raise
        raise ValueError("Inconsistent shapes between bounds and the problem.")


def _checked_iter(tol, max_iter, n):
    max_iter = 5 * n if max_iter is None else int(max_iter)
    if max_iter < 0:
        raise ValueError("`max_iter` must not be negative.")
    return float(tol), max_iter


class _Buffers:
    """The device memory of one call: ONE allocation of `capacity` bytes, carved in 256-byte steps and freed on exit (an
    allocation and its release cost more than the launches of a small batch)."""
    ALIGN = 256

    @classmethod
    def need(cls, *items):
        """The capacity for `items`: byte counts, arrays to upload, or None (nothing)."""
        sizes = (int(getattr(it, "nbytes", it)) for it in items if it is not None)
        return sum((max(sz, 8) + cls.ALIGN - 1) // cls.ALIGN * cls.ALIGN for sz in sizes)

    def __init__(self, ctx, capacity):
        self.ctx, self.capacity, self.used = ctx, int(capacity), 0
        self.base = ctx.malloc(max(self.capacity, 8))

    def new(self, nbytes):
        p = _abi.vp(self.base.value + self.used)
        self.used += self.need(nbytes)
        if self.used > self.capacity:
            raise _abi.BlsqError("device buffers of a bvls call exceed their allocation")
        return p

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        p = self.new(a.nbytes)
        self.ctx.check(self.ctx.lib.blsq_memcpy_h2d(self.ctx.h, p, _abi.ptr(a), a.nbytes), "blsq_memcpy_h2d")
        return p

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.free(self.base)


def _output_bytes(B, m, n, fun):
    """x, on_bound, fun, grad, optimality and cost, stat"""
    return (8 * B * n, 4 * B * n, 8 * B * m if fun else None, 8 * B * n, 16 * B, 12 * B)


def _context(ctx):
    if ctx is not None:
        return ctx
    from ._hip_step import default_context
    return default_context()


def _checked_equality(equality, B, n):
    """None, or (e (n,) or (B, n), d (B,)) of ``equality=(e, d)``: e a scalar, (n,) or (B, n), d a scalar or (B,)."""
    if equality is None:
        return None
    try:
        e, d = equality
        e = np.asarray(e, dtype=np.float64)
        d = np.asarray(d, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("`equality` must be a pair (e, d).")
    try:
        e = np.broadcast_to(e, (B, n) if e.ndim == 2 else (n,))
        d = np.broadcast_to(d, (B,))
    except ValueError:
        raise ValueError("Inconsistent shapes between `equality` and the problem: e is a scalar, (n,) or (B, n), d a "
                         "scalar or (B,).")
    if not np.all(np.isfinite(e)) or np.any(e == 0.0):
        raise ValueError("Every entry of the `e` of `equality` must be finite and not zero.")
    if not np.all(np.isfinite(d)):
        raise ValueError("The `d` of `equality` must be finite.")
    return np.ascontiguousarray(e), np.ascontiguousarray(d)


def _equality_bytes(eq, B):
    """e, d and the multiplier"""
    return (None, None, None) if eq is None else (eq[0], eq[1], 8 * B)


def _solve(ctx, buf, B, m, n, d_G, G_stride, d_c, lb, ub, tol, max_iter, d_A, A_stride, d_y, d_w, w_stride, fun,
           eq=None):
    """blsq_bvls_solve_dev (with `eq`: blsq_bvls_solve_eq_dev) and the read-back -> BvlsResult."""
    whole = d_A is not None
    d_x, d_on = buf.new(8 * B * n), buf.new(4 * B * n)
    d_fun = buf.new(8 * B * m) if (whole and fun) else None
    d_grad, d_opt, d_stat = buf.new(8 * B * n), buf.new(8 * B * 2), buf.new(4 * B * 3)
    args = (ctx.h, B, m, n, d_G, G_stride, d_c, buf.up(lb), buf.up(ub), tol, max_iter, d_A, A_stride, d_y, d_w,
            w_stride, d_x, d_on, d_fun, d_grad, d_opt, d_stat)
    d_mult = None
    if eq is None:
        ctx.check(ctx.lib.blsq_bvls_solve_dev(*args), "blsq_bvls_solve_dev")
    else:
        d_mult = buf.new(8 * B)
        ctx.check(ctx.lib.blsq_bvls_solve_eq_dev(*args, buf.up(eq[0]), n if eq[0].ndim == 2 else 0, buf.up(eq[1]),
                                                 d_mult), "blsq_bvls_solve_eq_dev")
    stat = ctx.to_host(d_stat, (B, 3), np.int32)
    opt = ctx.to_host(d_opt, (B, 2), np.float64)
    return BvlsResult(x=ctx.to_host(d_x, (B, n), np.float64), device_cost=opt[:, 1].copy() if whole else None,
                      fun=ctx.to_host(d_fun, (B, m), np.float64) if d_fun is not None else None,
                      optimality=opt[:, 0].copy(), active_mask=ctx.to_host(d_on, (B, n), np.int32),
                      nit=stat[:, 1].copy(), nfact=stat[:, 2].copy(), status=stat[:, 0].copy(),
                      success=stat[:, 0] > 0,
                      multiplier=None if d_mult is None else ctx.to_host(d_mult, (B,), np.float64))


def bvls_batch(A, b, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True,
               equality=None):
    """Solve B problems ``min 1/2 |w (A x - b)|^2``, ``lb <= x <= ub`` exactly (scipy's ``lsq_linear(method='bvls')``),
    in two calls of the library: the moments, then every problem's whole active-set iteration and its correction against `A`.

    A : (m, n), one matrix shared by all problems, or (B, m, n);  b : (B, m), or (m,) for one problem;  n <= 128.
    bounds : pair broadcastable to (B, n), every lb < ub, infinities allowed on either side.
    tol : a variable on a bound is released when the gradient pushes it inwards by more than `tol`.
    max_iter : the most release passes per problem (None: 5 n).
    sigma : None, a scalar, (m,) or (B, m): rows are weighted by w = 1 / sigma.
    fun : False: the residuals (B, m) are neither written nor returned; ``fun`` of the result is None.
    equality : None, or a pair (e, d): the problem under ``e^T x = d`` as well.  e : a scalar, (n,) or
        (B, n), every entry finite and not zero;  d : a scalar or (B,).  The sum holds to rounding, bound variables
        still hold their bounds bit for bit, ``multiplier`` of the result is the multiplier of the equality and
        ``optimality`` is taken from ``grad + multiplier e``.  One equality only; rank-deficient free blocks stay
        status -1.
    -> BvlsResult.  ``status`` 1: the optimality conditions hold; 0: `max_iter` passes used; -1: a free block was not
    positive definite (rank-deficient problems are not handled) or a value was not finite; -2 (with `equality` only):
    the equality cannot be met inside the bounds.  ``cost`` and ``optimality`` are taken from `A` at the returned x,
    whatever the status."""
    A, b, w = _checked_problem(A, b, sigma)
    B, m = b.shape
    n = A.shape[-1]
    _checked_size(n)
    lb, ub = _checked_bounds(bounds, B, n)
    tol, max_iter = _checked_iter(tol, max_iter, n)
    eq = _checked_equality(equality, B, n)
    ctx = _context(ctx)
    A_stride = m * n if A.ndim == 3 else 0
    w_stride = m if (w is not None and w.ndim == 2) else 0
    G_stride = n * n if (A_stride or w_stride) else 0
    with _Buffers(ctx, _Buffers.need(A, b, w, 8 * n * n * (B if G_stride else 1), 8 * B * n, lb, ub,
                                     *_output_bytes(B, m, n, fun), *_equality_bytes(eq, B))) as buf:
        d_A, d_y, d_w = buf.up(A), buf.up(b), buf.up(w)
        d_G, d_c = buf.new(8 * n * n * (B if G_stride else 1)), buf.new(8 * B * n)
        ctx.check(ctx.lib.blsq_bvls_moments_dev(ctx.h, B, m, n, d_A, A_stride, d_y, d_w, w_stride, d_G, G_stride, d_c),
                  "blsq_bvls_moments_dev")
        return _solve(ctx, buf, B, m, n, d_G, G_stride, d_c, lb, ub, tol, max_iter, d_A, A_stride, d_y, d_w, w_stride,
                      fun, eq)


def bvls(A, b, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True, equality=None):
    """``bvls_batch`` for one problem: A (m, n), b (m,).  Returns the one result, with scipy's names."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if A.ndim != 2 or b.ndim != 1:
        raise ValueError("`A` must have shape (m, n) and `b` shape (m,): use `bvls_batch` for a batch.")
    return bvls_batch(A, b, bounds, tol, max_iter, sigma, ctx, fun, equality)[0]


def nnls_batch(A, b, tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True, equality=None):
    """Non-negative least squares (``scipy.optimize.nnls``) for a batch: ``bvls_batch`` with ``bounds=(0, inf)``."""
    return bvls_batch(A, b, (0.0, np.inf), tol, max_iter, sigma, ctx, fun, equality)


def fcls_batch(A, b, sigma=None, tol=1e-10, max_iter=None, ctx=None, fun=True):
    """Fully constrained least squares (Heinz and Chang) for a batch: abundances that are non-negative and sum to one,
    ``nnls_batch(..., equality=(1.0, 1.0))``.  ``multiplier`` of the result is the multiplier of the sum."""
    return nnls_batch(A, b, tol, max_iter, sigma, ctx, fun, equality=(1.0, 1.0))


def bvls_gram_batch(G, c, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, ctx=None, equality=None):
    """The same iteration for callers who hold normal equations: ``min 1/2 x^T G x - c^T x``, ``lb <= x <= ub``.

    G : (n, n), shared, or (B, n, n), symmetric positive definite (both triangles are read);  c : (B, n), or (n,).
    equality : as in ``bvls_batch``.
    -> BvlsResult without ``fun`` and ``cost``; ``optimality`` is taken from ``g = G x - c``.  No correction against a
    matrix: the answer carries the conditioning of G."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or c.size == 0:
        raise ValueError("`c` must have shape (n,) or (B, n).")
    B, n = c.shape
    if G.ndim not in (2, 3) or G.shape[-2:] != (n, n):
        raise ValueError("`G` must have shape (n, n) or (B, n, n) with the n of `c`.")
    if G.ndim == 3 and G.shape[0] != B:
        raise ValueError("`G` of shape (B, n, n) needs `c` of shape (B, n) with the same B.")
    _checked_size(n)
    lb, ub = _checked_bounds(bounds, B, n)
    tol, max_iter = _checked_iter(tol, max_iter, n)
    eq = _checked_equality(equality, B, n)
    ctx = _context(ctx)
    with _Buffers(ctx, _Buffers.need(G, c, lb, ub, *_output_bytes(B, 0, n, False), *_equality_bytes(eq, B))) as buf:
        return _solve(ctx, buf, B, 0, n, buf.up(G), n * n if G.ndim == 3 else 0, buf.up(c), lb, ub, tol, max_iter,
                      None, 0, None, None, 0, False, eq)
