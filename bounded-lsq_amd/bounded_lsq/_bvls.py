"""`bvls_batch`, `bvls`, `nnls_batch`, `bvls_gram_batch`: bounded-variable least squares by an exact active-set method,
a whole batch in two calls of the library.

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

__all__ = ['bvls_batch', 'bvls', 'nnls_batch', 'bvls_gram_batch', 'bvls_reference', 'BvlsResult', 'BVLS_MAX_N']

BVLS_MAX_N = 128                               # BLSQ_BVLS_MAX_N of include/blsq.h

MESSAGES = {1: "No variable on a bound wants to leave it, and the free ones solve their normal equations.",
            0: "The maximum number of release passes is exceeded.",
            -1: "A free block is not positive definite in floating point, or a value is not finite."}


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


def bvls_reference(G, c, lb, ub, tol=1e-10, max_iter=None):
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
    -> dict(x, on_bound, status, nit (release passes), nfact (factorisations), g (= G x - c at the end))."""
    G = np.asarray(G, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[0]
    lb = np.broadcast_to(np.asarray(lb, dtype=np.float64), (n,))
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (n,))
    max_iter = 5 * n if max_iter is None else int(max_iter)
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


class BvlsResult:
    """The results of a batch as arrays over the problems (a batch is 1e5 to 1e6 problems: not a list of objects):
    x (B, n), cost (B,) = 0.5 fun @ fun, fun (B, m) = w (A x - b) or None, optimality (B,), active_mask (B, n) in
    {-1, 0, 1}, nit (B,) the release passes, nfact (B,) the factorisations, status (B,), success (B,).  ``res[p]`` is
    problem p with scipy's names (and ``message``).

    ``cost``: with `fun`, ``0.5 * numpy.dot(fun[p], fun[p])`` of the returned residuals, scipy's definition in numpy's
    own summation order, formed on first use; without (``fun=False``) the kernel's sum of the same squares in its own
    order (``device_cost``, always there), within 2 gamma_m of the other."""
    FIELDS = ('x', 'cost', 'fun', 'optimality', 'active_mask', 'nit', 'nfact', 'status', 'success')

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


def _solve(ctx, buf, B, m, n, d_G, G_stride, d_c, lb, ub, tol, max_iter, d_A, A_stride, d_y, d_w, w_stride, fun):
    """blsq_bvls_solve_dev and the read-back -> BvlsResult."""
    whole = d_A is not None
    d_x, d_on = buf.new(8 * B * n), buf.new(4 * B * n)
    d_fun = buf.new(8 * B * m) if (whole and fun) else None
    d_grad, d_opt, d_stat = buf.new(8 * B * n), buf.new(8 * B * 2), buf.new(4 * B * 3)
    ctx.check(ctx.lib.blsq_bvls_solve_dev(ctx.h, B, m, n, d_G, G_stride, d_c, buf.up(lb), buf.up(ub), tol, max_iter,
                                          d_A, A_stride, d_y, d_w, w_stride, d_x, d_on, d_fun, d_grad, d_opt, d_stat),
              "blsq_bvls_solve_dev")
    stat = ctx.to_host(d_stat, (B, 3), np.int32)
    opt = ctx.to_host(d_opt, (B, 2), np.float64)
    return BvlsResult(x=ctx.to_host(d_x, (B, n), np.float64), device_cost=opt[:, 1].copy() if whole else None,
                      fun=ctx.to_host(d_fun, (B, m), np.float64) if d_fun is not None else None,
                      optimality=opt[:, 0].copy(), active_mask=ctx.to_host(d_on, (B, n), np.int32),
                      nit=stat[:, 1].copy(), nfact=stat[:, 2].copy(), status=stat[:, 0].copy(),
                      success=stat[:, 0] > 0)


def bvls_batch(A, b, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True):
    """Solve B problems ``min 1/2 |w (A x - b)|^2``, ``lb <= x <= ub`` exactly (scipy's ``lsq_linear(method='bvls')``),
    in two calls of the library: the moments, then every problem's whole active-set iteration and its correction against `A`.

    A : (m, n), one matrix shared by all problems, or (B, m, n);  b : (B, m), or (m,) for one problem;  n <= 128.
    bounds : pair broadcastable to (B, n), every lb < ub, infinities allowed on either side.
    tol : a variable on a bound is released when the gradient pushes it inwards by more than `tol`.
    max_iter : the most release passes per problem (None: 5 n).
    sigma : None, a scalar, (m,) or (B, m): rows are weighted by w = 1 / sigma.
    fun : False: the residuals (B, m) are neither written nor returned; ``fun`` of the result is None.
    -> BvlsResult.  ``status`` 1: the optimality conditions hold; 0: `max_iter` passes used; -1: a free block was not
    positive definite (rank-deficient problems are not handled) or a value was not finite.  ``cost`` and ``optimality``
    are taken from `A` at the returned x, whatever the status."""
    A, b, w = _checked_problem(A, b, sigma)
    B, m = b.shape
    n = A.shape[-1]
    _checked_size(n)
    lb, ub = _checked_bounds(bounds, B, n)
    tol, max_iter = _checked_iter(tol, max_iter, n)
    ctx = _context(ctx)
    A_stride = m * n if A.ndim == 3 else 0
    w_stride = m if (w is not None and w.ndim == 2) else 0
    G_stride = n * n if (A_stride or w_stride) else 0
    with _Buffers(ctx, _Buffers.need(A, b, w, 8 * n * n * (B if G_stride else 1), 8 * B * n, lb, ub,
                                     *_output_bytes(B, m, n, fun))) as buf:
        d_A, d_y, d_w = buf.up(A), buf.up(b), buf.up(w)
        d_G, d_c = buf.new(8 * n * n * (B if G_stride else 1)), buf.new(8 * B * n)
        ctx.check(ctx.lib.blsq_bvls_moments_dev(ctx.h, B, m, n, d_A, A_stride, d_y, d_w, w_stride, d_G, G_stride, d_c),
                  "blsq_bvls_moments_dev")
        return _solve(ctx, buf, B, m, n, d_G, G_stride, d_c, lb, ub, tol, max_iter, d_A, A_stride, d_y, d_w, w_stride,
                      fun)


def bvls(A, b, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True):
    """``bvls_batch`` for one problem: A (m, n), b (m,).  Returns the one result, with scipy's names."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if A.ndim != 2 or b.ndim != 1:
        raise ValueError("`A` must have shape (m, n) and `b` shape (m,): use `bvls_batch` for a batch.")
    return bvls_batch(A, b, bounds, tol, max_iter, sigma, ctx, fun)[0]


def nnls_batch(A, b, tol=1e-10, max_iter=None, sigma=None, ctx=None, fun=True):
    """Non-negative least squares (``scipy.optimize.nnls``) for a batch: ``bvls_batch`` with ``bounds=(0, inf)``."""
    return bvls_batch(A, b, (0.0, np.inf), tol, max_iter, sigma, ctx, fun)


def bvls_gram_batch(G, c, bounds=(-np.inf, np.inf), tol=1e-10, max_iter=None, ctx=None):
    """The same iteration for callers who hold normal equations: ``min 1/2 x^T G x - c^T x``, ``lb <= x <= ub``.

    G : (n, n), shared, or (B, n, n), symmetric positive definite (both triangles are read);  c : (B, n), or (n,).
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
    ctx = _context(ctx)
    with _Buffers(ctx, _Buffers.need(G, c, lb, ub, *_output_bytes(B, 0, n, False))) as buf:
        return _solve(ctx, buf, B, 0, n, buf.up(G), n * n if G.ndim == 3 else 0, buf.up(c), lb, ub, tol, max_iter,
                      None, 0, None, None, 0, False)
