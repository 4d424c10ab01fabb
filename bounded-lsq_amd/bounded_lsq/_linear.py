"""`lsq_linear` and `lsq_linear_batch`: bounded linear least squares, ``min 1/2 |A x - b|^2`` with ``lb <= x <= ub``, on
this package's solvers.

A linear residual is one more producer of f and J for the device-resident outer driver: ``LinearDeviceModel`` keeps A, b
and 1 / sigma on the GPU and evaluates ``f = w (A x - b)`` and ``J = diag(w) A`` there (blsq_linear_eval_dev), so a whole
batch — typically many right-hand sides against ONE matrix — is solved without f, J or x crossing the boundary.
``numpy_callbacks`` is the definition, and the ``driver='host'`` route.  Nothing here knows that J is constant: every
iteration factors it again, as for any other residual ("Not built").
"""
import numpy as np

from . import _abi
from ._batch import least_squares_batch, _bounds_2d
from ._cov import check_covariance, check_leverage, attach as _attach_covariance
from ._hostmath import EPS, _initialize_feasible, active_mask
from ._models import sigma_weights

__all__ = ['lsq_linear', 'lsq_linear_batch', 'LinearFit', 'LinearDeviceModel', 'numpy_callbacks']

METHODS = ('trf', 'dogbox')


def _checked_problem(A, b, sigma=None):
    """-> (A (m, n) or (B, m, n), b (B, m), w None / (m,) / (B, m), all float64 and contiguous).  A 1-D `b` is a batch
    of one.  ValueError for anything else (before any GPU is touched)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim not in (2, 3):
        raise ValueError("`A` must have shape (m, n) or (B, m, n).")
    b = np.ascontiguousarray(b, dtype=np.float64)
    if b.ndim == 1:
        b = b[None]
    if b.ndim != 2:
        raise ValueError("`b` must have shape (m,) or (B, m).")
    if A.size == 0 or b.size == 0:
        raise ValueError("`A` and `b` must not be empty.")
    B, m = b.shape
    if A.shape[-2] != m:
        raise ValueError("Inconsistent shapes between `A` and `b`.")
    if A.ndim == 3 and A.shape[0] != B:
        raise ValueError("`A` of shape (B, m, n) needs `b` of shape (B, m) with the same B.")
    w = None
    if sigma is not None:
        w, per_problem = sigma_weights(sigma, (B,), m)
        w = np.ascontiguousarray(w if per_problem else np.broadcast_to(w, (m,)), dtype=np.float64)
    return A, b, w


def numpy_callbacks(A, b, sigma=None):
    """The numpy ``(fun, jac)`` of the problem, vectorised over the batch as ``least_squares_batch`` takes them:
    ``fun(X) = w * (A @ x - b)`` of shape (B, m) and ``jac(X) = w[:, None] * A`` of shape (B, m, n) for X (B, n), with
    w = 1 / sigma (None: 1).  The definition of what the device evaluates, and the callbacks of ``driver='host'``."""
    A, b, w = _checked_problem(A, b, sigma)
    B, m = b.shape
    Jw = A if w is None else w[..., :, None] * A
    Jw = np.broadcast_to(Jw, (B, m, A.shape[-1]))

    def fun(X):
        r = (A @ np.asarray(X, dtype=np.float64)[:, :, None])[..., 0] - b
        return r if w is None else w * r

    def jac(X):
        return np.array(Jw, order='C')                                # a fresh array: the host driver keeps and rescales it
    return fun, jac


class LinearDeviceModel:
    """A, b and 1 / sigma resident on the GPU: the device callbacks of ``OuterDriver.run_device`` for a linear residual,
    the counterpart of ``models.DeviceModel``.

    A: (m, n), ONE matrix for all problems (uploaded once, read by every problem through a zero stride), or (B, m, n);
    b: (B, m), or (m,) for one problem; sigma: None, a scalar, (m,) or (B, m).  ``fun_dev(x_ptr, f_ptr, reps)`` and
    ``jac_dev(x_ptr, J_ptr, mask_ptr)`` launch on the context's stream, the stream of every driver on that context.
    ``jac_dev`` copies diag(w) A into the driver's J on EVERY call: the driver scales J in place under a robust loss,
    and the copy is one pass over J next to a Gram that reads it anyway.  ``bounds_dev`` is the (lb_ptr, ub_ptr) pair
    the finite-difference route asks for, after ``set_bounds(lb, ub)``.  ``close()`` frees the buffers (also run when the
    context closes)."""

    def __init__(self, ctx, A, b, sigma=None):
        A, b, w = _checked_problem(A, b, sigma)
        self.B, self.m = b.shape
        self.n = A.shape[-1]
        self.A_stride = self.m * self.n if A.ndim == 3 else 0
        self.w_stride = self.m if (w is not None and w.ndim == 2) else 0
        self.ctx = ctx
        self._bufs = []
        self.d_A, self.d_y, self.d_w = self._upload(A), self._upload(b), self._upload(w)
        self.bounds_dev = None
        ctx.adopt(self)

    def _upload(self, a):
        if a is None:
            return None
        p = self.ctx.to_device(a)
        self._bufs.append(p)
        return p

    def set_bounds(self, lb, ub):
        self.bounds_dev = tuple(self._upload(np.ascontiguousarray(np.broadcast_to(a, (self.B, self.n)), dtype=np.float64))
                                for a in (lb, ub))
        return self.bounds_dev

    def _eval(self, x_ptr, reps, f_ptr, J_ptr, mask_ptr):
        ctx = self.ctx
        ctx.check(ctx.lib.blsq_linear_eval_dev(ctx.h, self.B, int(reps), self.m, self.n, self.d_A, self.A_stride, self.d_y,
                                               self.d_w, self.w_stride, x_ptr, f_ptr, J_ptr, mask_ptr),
                  "blsq_linear_eval_dev")

    def fun_dev(self, x_ptr, f_ptr, reps=1):
        self._eval(x_ptr, reps, f_ptr, None, None)

    def jac_dev(self, x_ptr, J_ptr, mask_ptr=None):
        self._eval(x_ptr, 1, None, J_ptr, mask_ptr)

    def close(self):
        bufs, self._bufs = getattr(self, "_bufs", []), []
        ctx = self.ctx
        if ctx is not None and getattr(ctx, "h", None):
            for p in bufs:
                ctx.free(p)
        self.bounds_dev = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class LinearFit:
    """What ``least_squares_batch(fun=...)`` takes in place of a callable for a linear residual evaluated on the device:
    the checked (A, b, sigma) that opens a ``LinearDeviceModel`` on the driver's context (driver='device'; `jac` None,
    '2-point' or '3-point').  Built by ``lsq_linear_batch``; the counterpart of ``models.DeviceFit``."""

    def __init__(self, A, b, sigma=None):
        self.A, self.b, w = _checked_problem(A, b, sigma)
        self.sigma = sigma
        self.B, self.m = self.b.shape
        self.n = self.A.shape[-1]

    def open_device(self, ctx, lb, ub):
        dm = LinearDeviceModel(ctx, self.A, self.b, self.sigma)
        dm.set_bounds(lb, ub)
        return dm


def lsq_linear_batch(A, b, bounds=(-np.inf, np.inf), method='trf', tol=1e-10, max_iter=None, x0=None, sigma=None,
                     driver='device', ctx=None, covariance=False, leverage=False):
    """Solve B bounded linear least-squares problems ``min 1/2 |A x - b|^2``, ``lb <= x <= ub`` (scipy's ``lsq_linear``,
    and NNLS with ``bounds=(0, inf)``), together.

    A : (m, n), one matrix shared by all problems, or (B, m, n);  b : (B, m), or (m,) for one problem.
    bounds : pair broadcastable to (B, n), every lb < ub.
    method : 'trf' or 'dogbox', this package's solvers ('bvls' is not built).
    tol : the gradient and the cost tolerance (``gtol = ftol = tol``; the step tolerance is machine epsilon).
    max_iter : the most residual evaluations per problem (None: 100 n).
    x0 : (B, n) or broadcastable to it, inside the bounds; None: 1, or the middle of / one unit inside the finite bounds.
    sigma : None, a scalar, (m,) or (B, m): rows are weighted by 1 / sigma.
    driver : 'device' — A, b and the weights stay on the GPU and f and J are evaluated there (``LinearFit``); 'host' —
             the numpy callbacks of ``numpy_callbacks`` around batched step calls.
    covariance : False, or a mode of ``least_squares_batch``.  True means 'free' here: the covariance
             ``(A_F^T A_F)^-1`` over the variables off their bounds with zeros elsewhere — what
             ``bounded_lsq.covariance(A, active_mask)`` gives —, because the inverse over all variables belongs to the
             problem without bounds.  leverage : True (needs `covariance`) adds the leverages of the rows.
    Returns the list of B results of ``least_squares_batch`` with scipy's names added: ``x``, ``cost``
    (= 0.5 * fun @ fun), ``fun`` (= A x - b, times 1 / sigma), ``optimality``, ``active_mask`` ('trf': scipy's
    ``find_active_constraints(x, lb, ub, rtol=tol)``, since TRF ends strictly inside the box; 'dogbox': its own
    on_bound), ``nit`` (= nfev - 1: the steps tried), ``nfev``, ``status``, ``message``, ``success``, and
    ``x_covariance`` / ``leverage`` (``_cov.attach`` on the final Jacobians, after the masks) where asked for.
    """
    if method not in METHODS:
        raise ValueError("`method` must be 'trf' or 'dogbox' (got %r%s)."
                         % (method, ": 'bvls' is not built" if method == 'bvls' else ""))
    if driver not in ('host', 'device'):
        raise ValueError("`driver` must be 'host' or 'device'.")
    covariance = check_covariance(covariance)
    leverage = check_leverage(leverage, covariance)
    if covariance is True:
        covariance = 'free'
    fit = LinearFit(A, b, sigma)
    B, n = fit.B, fit.n
    try:
        lb, ub = _bounds_2d(bounds, B, n)
    except ValueError as e:
        if "bound" in str(e):
            raise
        raise ValueError("Inconsistent shapes between bounds and `A`.")
    if x0 is None:
        X0 = _initialize_feasible(lb, ub)
    else:
        try:
            X0 = np.broadcast_to(np.asarray(x0, dtype=np.float64), (B, n)).copy()
        except ValueError:
            raise ValueError("`x0` must have shape (n,) or (B, n).")
    tol = float(tol)
    kw = dict(bounds=(lb, ub), method=method, ftol=tol, xtol=EPS, gtol=tol, max_nfev=max_iter, scaling=1.0, ctx=ctx,
              driver=driver)
    if driver == 'device':
        results = least_squares_batch(fit, X0, None, **kw)
    else:
        fun, jac = numpy_callbacks(fit.A, fit.b, sigma)
        results = least_squares_batch(fun, X0, jac, **kw)
    for p, r in enumerate(results):
        r.cost = 0.5 * float(np.dot(r.fun, r.fun))
        r.nit = r.nfev - 1
        if method == 'trf':
            # TRF ends strictly inside the box; the solver's own mask uses rtol = xtol = machine epsilon and would name
            # nothing.  scipy's lsq_linear (trf_linear) reports find_active_constraints(x, lb, ub, rtol=tol): so here.
            r.active_mask = active_mask(r.x, lb[p], ub[p], rtol=tol)
    if covariance:
        # after the masks, so that 'free' holds exactly the variables `active_mask` names (for 'trf' the driver's own
        # covariance call would use the solver's mask); from the final Jacobians the results carry
        _attach_covariance(results, covariance, ctx=ctx, leverage=leverage)
    return results


def lsq_linear(A, b, bounds=(-np.inf, np.inf), method='trf', tol=1e-10, max_iter=None, x0=None, sigma=None,
               driver='device', ctx=None, covariance=False, leverage=False):
    """``lsq_linear_batch`` for one problem: A (m, n), b (m,), bounds and x0 broadcastable to (n,).  Returns the one
    result."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if A.ndim != 2 or b.ndim != 1:
        raise ValueError("`A` must have shape (m, n) and `b` shape (m,): use `lsq_linear_batch` for a batch.")
    return lsq_linear_batch(A, b, bounds, method, tol, max_iter, x0, sigma, driver, ctx, covariance, leverage)[0]
