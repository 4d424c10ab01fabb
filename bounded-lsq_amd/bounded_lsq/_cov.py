"""Parameter covariance from the final Jacobian (blsq_cov* of include/blsq.h).

The reference documents ``x_covariance`` as the inverse of ``J^T J`` at the solution (least_squares.py:248-252) and
fills it only through its MINPACK bridge.  Here it is computed on the GPU from a Householder triangle of J:

  ``covariance=True``    C = (J^T J)^-1 over all n variables (scipy ``curve_fit``'s ``pcov`` with
                         ``absolute_sigma=True`` whenever J has full rank);
  ``covariance='free'``  F = {j : active_mask[j] == 0}; C[F, F] = (J_F^T J_F)^-1 and every row and column of an
                         active variable exactly 0.0: the covariance with the variables on a bound held fixed.

A problem whose triangle has a zero or non-finite pivot, or whose ``rcond_1 = 1 / (||R||_1 ||R^-1||_1)`` is below
``eps * max(m, |F|)``, is singular: its ``x_covariance`` is None (as the reference's docstring prescribes), its rcond
is still reported.  No residual-variance scaling is applied: multiply by ``obj_value / (m - n)`` for ``curve_fit``'s
default (``absolute_sigma=False``).
"""
import ctypes as C

import numpy as np

from ._abi import vp, ptr


def check_covariance(covariance):
    """-> False, True or 'free'; ValueError for anything else (before any GPU is touched)."""
    if isinstance(covariance, (bool, np.bool_)):
        return bool(covariance)
    if isinstance(covariance, str) and covariance == 'free':
        return 'free'
    raise ValueError("`covariance` must be False, True or 'free'.")


def covariance(J, active_mask=None, ctx=None):
    """Covariance of one (m, n) Jacobian or of a batch (B, m, n).

    active_mask : None (all variables), or integers of shape (n,) / (B, n): non-zero marks a variable on a bound.
    Returns ``(cov, rcond, status)``: cov (n, n) or (B, n, n) — NaN everywhere for a singular problem —, rcond and
    status (0 regular, 1 singular) scalars or (B,).
    """
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
    if ctx is None:
        from ._hip_step import default_context
        ctx = default_context()
    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "blsq_cov_plan_create")
    try:
        cov = np.empty((B, n, n))
        rcond = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        ctx.check(ctx.lib.blsq_cov(h, ptr(Jb), ptr(act), ptr(cov), ptr(rcond), ptr(status)), "blsq_cov")
    finally:
        ctx.lib.blsq_cov_plan_destroy(h)
    if single:
        return cov[0], float(rcond[0]), int(status[0])
    return cov, rcond, status


def fill_results(results, mode, cov, rcond, status):
    """x_covariance (None where singular) and x_covariance_rcond of each result from one batched call's outputs."""
    for b, r in enumerate(results):
        r.x_covariance = None if int(status[b]) != 0 else cov[b].copy()
        r.x_covariance_rcond = float(rcond[b])
    return results


def attach(results, mode, ctx=None):
    """One batched covariance call on the stacked final Jacobians of `results` (`mode`: True or 'free')."""
    J = np.stack([r.jac for r in results])
    act = np.stack([np.asarray(r.active_mask) for r in results]) if mode == 'free' else None
    cov, rcond, status = covariance(J, act, ctx=ctx)
    return fill_results(results, mode, cov, rcond, status)
