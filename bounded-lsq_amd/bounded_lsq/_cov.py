"""Parameter covariance from the final Jacobian (blsq_cov* of include/blsq.h).

The reference documents ``x_covariance`` as the inverse of ``J^T J`` at the solution (least_squares.py:248-252) and
fills it only through its MINPACK bridge.  Here it is computed on the GPU from a Householder triangle of J:

  ``covariance=True``    C = (J^T J)^-1 over all n variables (scipy ``curve_fit``'s ``pcov`` with
                         ``absolute_sigma=True`` whenever J has full rank);
  ``covariance='free'``  F = {j : active_mask[j] == 0}; C[F, F] = (J_F^T J_F)^-1 and every row and column of an
                         active variable exactly 0.0: the covariance with the variables on a bound held fixed.

  ``covariance='pinv'``  the Moore-Penrose covariance ``V diag(1/s^2) V^T`` over the singular values of J above
                         ``eps * max(m, n) * s_max``: scipy ``curve_fit``'s ``pcov`` (``absolute_sigma=True``) for
                         any rank (blsq_cov_pinv*).  ``x_covariance_rank`` is the number kept;
  ``covariance='free-pinv'``  the same over the free variables, zeros in the rows and columns of the others.

For the two pinv modes ``x_covariance_rcond`` is ``s_min / s_max`` over all singular values (0 for a rank-deficient
J), NOT the 1-norm figure of the other two modes, and ``x_covariance`` is None only where J is not finite (scipy's
``svd`` raises there) or the SVD did not converge.

For True / 'free': a problem whose triangle has a zero or non-finite pivot, or whose ``rcond_1 = 1 / (||R||_1 ||R^-1||_1)`` is below
``eps * max(m, |F|)``, is singular: its ``x_covariance`` is None (as the reference's docstring prescribes), its rcond
is still reported.  No residual-variance scaling is applied: multiply by ``obj_value / (m - n)`` for ``curve_fit``'s
default (``absolute_sigma=False``).
"""
import ctypes as C

import numpy as np

from ._abi import vp, ptr


MODES = ('free', 'pinv', 'free-pinv')


def check_covariance(covariance):
    """-> False, True, 'free', 'pinv' or 'free-pinv'; ValueError for anything else (before any GPU is touched)."""
    if isinstance(covariance, (bool, np.bool_)):
        return bool(covariance)
    if isinstance(covariance, str) and covariance in MODES:
        return covariance
    raise ValueError("`covariance` must be False, True or 'free', or 'pinv' or 'free-pinv'.")


def is_pinv(mode):
    return mode in ('pinv', 'free-pinv')


def is_free(mode):
    return mode in ('free', 'free-pinv')


def checked_inputs(J, active_mask, pinv, scale):
    """The argument checks of `covariance` (ValueError, before any GPU is touched) -> (Jb (B, m, n) contiguous,
    act (B, n) int64 or None, sc (B,) or None, single)."""
    if not isinstance(pinv, (bool, np.bool_)):
        raise ValueError("`pinv` must be False or True.")
    J = np.asarray(J, dtype=np.float64)
    if J.ndim not in (2, 3):
        raise ValueError("`J` must have shape (m, n) or (B, m, n).")
    single = J.ndim == 2
    Jb = np.ascontiguousarray(J[None] if single else J)
    B, m, n = Jb.shape
    if B == 0 or m == 0 or n == 0:
        raise ValueError("`J` must not be empty.")
    act = None
    if active_mask is not None:
        act = np.asarray(active_mask)
        if single and act.ndim == 1:
            act = act[None]
        if act.shape != (B, n):
            raise ValueError("`active_mask` must have shape (n,) or (B, n) matching `J`.")
        act = np.ascontiguousarray(act != 0, dtype=np.int64)
    sc = None
    if scale is not None:
        try:
            sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,)))
        except ValueError:
            raise ValueError("`scale` must be a scalar or have shape (B,).")
    return Jb, act, sc, single


def plan_rows(ctx, h, B, rows, A=None, scale=None):
    """blsq_cov_rows on the plan `h` after its covariance call: (B, rows) row forms of `A` (B, rows, n; None: the J that
    call staged) through the factor it left, times `scale` (B,) or None."""
    out = np.empty((B, rows))
    ctx.check(ctx.lib.blsq_cov_rows(h, int(rows), ptr(A), ptr(scale), ptr(out)), "blsq_cov_rows")
    return out


def plan_call(Jb, act, sc, pinv, ctx=None, after=None):
    """One plan, one H2D of `Jb`, blsq_cov or blsq_cov_pinv -> (the call's batched outputs, after(ctx, h) or None):
    `after` runs on the live plan, whose factor blsq_cov_rows reads."""
    B, m, n = Jb.shape
    if ctx is None:
        from ._hip_step import default_context
        ctx = default_context()
    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "blsq_cov_plan_create")
    try:
        cov = np.empty((B, n, n))
        rcond = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        if pinv:
            rank = np.empty(B, dtype=np.int32)
            kept = np.empty(B)
            ctx.check(ctx.lib.blsq_cov_pinv(h, ptr(Jb), ptr(act), ptr(sc), ptr(cov), ptr(rank), ptr(rcond), ptr(kept),
                                            ptr(status)), "blsq_cov_pinv")
            out = (cov, rank, rcond, kept, status)
        else:
            ctx.check(ctx.lib.blsq_cov(h, ptr(Jb), ptr(act), ptr(cov), ptr(rcond), ptr(status)), "blsq_cov")
            out = (cov, rcond, status)
        extra = after(ctx, h) if after is not None else None
    finally:
        ctx.lib.blsq_cov_plan_destroy(h)
    return out, extra


def covariance(J, active_mask=None, ctx=None, pinv=False, scale=None):
    """Covariance of one (m, n) Jacobian or of a batch (B, m, n).

    active_mask : None (all variables), or integers of shape (n,) / (B, n): non-zero marks a variable on a bound.
    Returns ``(cov, rcond, status)``: cov (n, n) or (B, n, n) — NaN everywhere for a singular problem —, rcond and
    status (0 regular, 1 singular) scalars or (B,).

    pinv=True : the pseudo-inverse covariance (module docstring); returns ``(cov, rank, rcond, kept_rcond, status)``
    with rcond = s_min / s_max, kept_rcond = (smallest kept singular value) / s_max, status 0, 1 (J not finite: cov
    NaN) or 2 (SVD not converged: cov NaN).  scale (pinv only): None, a scalar or (B,): cov[b] is multiplied by it
    on the GPU (the residual variance ``obj_value / (m - n)`` of ``curve_fit``'s ``absolute_sigma=False``).
    """
    if not isinstance(pinv, (bool, np.bool_)):
        raise ValueError("`pinv` must be False or True.")
    if scale is not None and not pinv:
        raise ValueError("`scale` needs pinv=True.")
    Jb, act, sc, single = checked_inputs(J, active_mask, pinv, scale)
    out, _ = plan_call(Jb, act, sc, bool(pinv), ctx)
    if pinv:
        cov, rank, rcond, kept, status = out
        if single:
            return cov[0], int(rank[0]), float(rcond[0]), float(kept[0]), int(status[0])
        return cov, rank, rcond, kept, status
    cov, rcond, status = out
    if single:
        return cov[0], float(rcond[0]), int(status[0])
    return cov, rcond, status


def fill_results(results, mode, cov, *rest):
    """x_covariance (None where singular / not finite), x_covariance_rcond and, for the pinv modes,
    x_covariance_rank of each result from one batched call's outputs (`rest`: rcond, status, or rank, rcond,
    kept_rcond, status)."""
    if is_pinv(mode):
        rank, rcond, kept, status = rest
    else:
        rcond, status = rest
    for b, r in enumerate(results):
        r.x_covariance = None if int(status[b]) != 0 else cov[b].copy()
        r.x_covariance_rcond = float(rcond[b])
        if is_pinv(mode):
            r.x_covariance_rank = int(rank[b])
    return results


def variance_scales(results, nobs=None):
    """obj_value / (m - n) of each result (curve_fit: "s_sq = cost / (ysize - p0.size)"); needs m > n.  nobs (B,): the
    points each problem kept (``nan_policy='omit'``): obj_value / (nobs[b] - n), and inf where nobs[b] <= n."""
    if nobs is None:
        return np.array([r.obj_value / (r.jac.shape[0] - r.jac.shape[1]) for r in results])
    nobs = np.asarray(nobs)
    if nobs.shape != (len(results),):
        raise ValueError("`nobs` must have shape (B,).")
    dof = [int(k) - r.jac.shape[1] for k, r in zip(nobs, results)]
    return np.array([r.obj_value / d if d > 0 else np.inf for d, r in zip(dof, results)])


def fill_leverage(results, h):
    """``leverage`` of each result from the (B, m) leverages of the same plan call: None wherever x_covariance is."""
    for b, r in enumerate(results):
        r.leverage = None if r.x_covariance is None else h[b].copy()
    return results


def check_leverage(leverage, covariance):
    """-> bool; ValueError for a non-boolean, or for leverage=True without a covariance mode."""
    if not isinstance(leverage, (bool, np.bool_)):
        raise ValueError("`leverage` must be False or True.")
    if leverage and not covariance:
        raise ValueError("`leverage=True` needs a `covariance` mode: the leverages come from its factor.")
    return bool(leverage)


def attach(results, mode, ctx=None, variance_scale=False, leverage=False, nobs=None):
    """One batched covariance call on the stacked final Jacobians of `results` (`mode`: as check_covariance returns
    it).  variance_scale (pinv modes): multiply problem b by obj_value / (m - n) on the GPU.  leverage: the leverages
    of the rows of each Jacobian from the same plan call (blsq_cov_rows on the staged J; never scaled).  nobs: the
    points each problem kept, for the variance factor (``variance_scales``)."""
    J = np.stack([r.jac for r in results])
    act = np.stack([np.asarray(r.active_mask) for r in results]) if is_free(mode) else None
    scale = variance_scales(results, nobs) if (variance_scale and is_pinv(mode)) else None
    Jb, act, sc, _ = checked_inputs(J, act, is_pinv(mode), scale)
    after = (lambda c, h: plan_rows(c, h, Jb.shape[0], Jb.shape[1])) if leverage else None
    out, lev = plan_call(Jb, act, sc, is_pinv(mode), ctx, after)
    fill_results(results, mode, *out)
    if leverage:
        fill_leverage(results, lev)
    return results
