"""Tiny n-vector helpers the host drivers need OUTSIDE the per-iteration path
(initial interior shift, final active mask, Coleman-Li v for Delta_0).  Inside
the iteration the same quantities are produced on the GPU."""
import numpy as np


def in_bounds(x, lb, ub):
    """bounds.py:19-21."""
    return bool(np.all((x >= lb) & (x <= ub)))


def prepare_bounds(bounds, x0):
    """bounds.py:7-16: scalar bounds are broadcast to x0's shape."""
    lb, ub = (np.asarray(b, dtype=float) for b in bounds)
    if lb.ndim == 0:
        lb = np.resize(lb, x0.shape)
    if ub.ndim == 0:
        ub = np.resize(ub, x0.shape)
    return lb, ub


def _initialize_feasible(lb, ub):
    """scipy's start point when p0 is None: 1, or the middle of / one unit inside the finite bounds."""
    p0 = np.ones_like(lb)
    lo, hi = np.isfinite(lb), np.isfinite(ub)
    both = lo & hi
    p0[both] = 0.5 * (lb[both] + ub[both])
    p0[lo & ~hi] = lb[lo & ~hi] + 1
    p0[~lo & hi] = ub[~lo & hi] - 1
    return p0


def shift_into_interior(x, lb, ub, rstep=0.0):
    """bounds.py:79-103 (make_strictly_feasible)."""
    out = np.array(x, dtype=float, copy=True)
    low = x <= lb
    up = x >= ub
    if rstep == 0:
        out[low] = np.nextafter(lb[low], ub[low])
        out[up] = np.nextafter(ub[up], lb[up])
    else:
        out[low] = lb[low] + rstep * (1 + np.abs(lb[low]))
        out[up] = ub[up] - rstep * (1 + np.abs(ub[up]))
    return out


def active_mask(x, lb, ub, rtol=1e-12):
    """bounds.py:51-76 (find_active_constraints)."""
    mask = np.zeros(np.shape(x), dtype=int)
    dl = x - lb
    du = ub - x
    lower_nearer = dl < du
    with np.errstate(invalid="ignore"):
        on_l = dl < rtol * np.maximum(1, np.abs(lb))
        on_u = du < rtol * np.maximum(1, np.abs(ub))
    mask[lower_nearer & on_l] = -1
    mask[~lower_nearer & on_u] = 1
    return mask


def cl_vector(x, g, lb, ub):
    """bounds.py:106-149 (scaling_vector), v only."""
    v = np.ones_like(x)
    sel = (g < 0) & np.isfinite(ub)
    v[sel] = ub[sel] - x[sel]
    sel = (g > 0) & np.isfinite(lb)
    v[sel] = x[sel] - lb[sel]
    return v


def cl_optimality(x, g, lb, ub):
    """bounds.py:152-156 (CL_optimality)."""
    lb = np.resize(lb, np.shape(x))
    ub = np.resize(ub, np.shape(x))
    return float(np.linalg.norm(cl_vector(np.asarray(x, float), g, lb, ub) * g, ord=np.inf))


# ---- robust loss functions (scipy.optimize.least_squares `loss=` / `f_scale=`) --------------------------------------
# The reference minimises sum f^2.  Its successor scipy (1.15.3) adds a robust loss on top of the same drivers by
# transforming the step's inputs (_lsq/common.py scale_for_robust_loss_function); restated here for the host drivers
# (one operation per scipy operation: the same bits).  The device path is loss_kernels.hip.
LOSSES = ('linear', 'huber', 'soft_l1', 'cauchy', 'arctan')     # scipy's IMPLEMENTED_LOSSES order = BLSQ_LOSS_*
EPS = np.finfo(float).eps


def loss_message():
    return "`loss` must be one of {0} or a callable.".format(dict.fromkeys(LOSSES).keys())


def _rho_builtin(name, z):
    """(rho0, rho1, rho2) of z for a named loss, before the f_scale factors."""
    r = np.empty((3,) + z.shape)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if name == 'linear':                    # rho(z) = z
            r[0] = z
            r[1] = 1.0
            r[2] = 0.0
        elif name == 'huber':                   # z for z <= 1, 2 sqrt(z) - 1 above
            lin = z <= 1
            far = ~lin
            zf = z[far]
            r[0][lin] = z[lin]
            r[1][lin] = 1
            r[2][lin] = 0
            r[0][far] = 2 * zf ** 0.5 - 1
            r[1][far] = zf ** -0.5
            r[2][far] = -0.5 * zf ** -1.5
        elif name == 'soft_l1':                 # 2 (sqrt(1 + z) - 1)
            t = 1 + z
            r[0] = 2 * (t ** 0.5 - 1)
            r[1] = t ** -0.5
            r[2] = -0.5 * t ** -1.5
        elif name == 'cauchy':                  # log(1 + z)
            t = 1 + z
            r[0] = np.log1p(z)
            r[1] = 1 / t
            r[2] = -1 / t ** 2
        elif name == 'arctan':                  # arctan(z)
            t = 1 + z ** 2
            r[0] = np.arctan(z)
            r[1] = 1 / t
            r[2] = -2 * z / t ** 2
        else:
            raise ValueError(loss_message())
    return r


def loss_rho(loss, f, f_scale):
    """rho (3, m) at the residuals f: scipy's construct_loss_function(m, loss, f_scale)(f) (rho0 *= f_scale^2,
    rho2 /= f_scale^2).  `loss` is a name of LOSSES or a callable z -> (3, m)."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        z = (f / f_scale) ** 2
        rho = np.array(loss(z), dtype=float) if callable(loss) else _rho_builtin(loss, z)
        rho[0] *= f_scale ** 2
        rho[2] /= f_scale ** 2
    return rho


def loss_cost(loss, f, f_scale):
    """The objective f_scale^2 * sum rho0((f / f_scale)^2): the library's convention (no 1/2, so 'linear' with
    f_scale = 1 is ||f||^2); twice scipy's cost_only value, bit for bit."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        z = (f / f_scale) ** 2
        rho0 = np.asarray(loss(z), dtype=float)[0] if callable(loss) else _rho_builtin(loss, z)[0]
        return f_scale ** 2 * np.sum(rho0)


def loss_scale(J, f, rho):
    """scipy's scale_for_robust_loss_function without the in-place updates: -> (diag(w) J, f * (rho1 / w)),
    w = sqrt(max(rho1 + 2 rho2 f^2, EPS)) (NaN stays NaN).  J (m, n) and f (m,) are not modified."""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        w = rho[1] + 2 * rho[2] * f ** 2
        w[w < EPS] = EPS
        w **= 0.5
        return J * w[:, np.newaxis], f * (rho[1] / w)


def check_loss(loss, f_scale):
    """Argument checks of `least_squares` (the message of scipy for `loss`; scipy does not check `f_scale`)."""
    if not callable(loss) and not (isinstance(loss, str) and loss in LOSSES):
        raise ValueError(loss_message())
    fs = np.asarray(f_scale, dtype=float)
    with np.errstate(invalid='ignore'):
        if fs.size == 0 or not np.all(fs > 0) or not np.all(np.isfinite(fs)):
            raise ValueError("`f_scale` must be positive.")
