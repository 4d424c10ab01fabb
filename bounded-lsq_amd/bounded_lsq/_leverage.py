"""Leverages, prediction variances and influence measures (blsq_cov_rows* of include/blsq.h).

Both GPU quantities are one computation: the row-wise quadratic form ``a_i C a_i^T`` of a matrix A through the
covariance ``C`` of a fit with Jacobian J,

  ``leverage``             A = J:      h_i = (J C J^T)_ii, the diagonal of the hat matrix;
  ``prediction_variance``  A = J_new:  the variance of the fitted curve at new points, diag(J_new C J_new^T).

They are not evaluated through C.  C = X X^T with X = R^-1 (R the Householder triangle of J) has squared the
conditioning once more than needed: the GPU computes ``||a_i X||^2`` from the X the covariance plan has just formed —
for A = J a row of the orthogonal factor Q = J R^-1 — and on the pseudo-inverse route ``sum_k (v_k . a_i)^2 / s_k^2``
over the kept singular directions of the plan's Jacobi SVD.  Neither J nor C crosses back to the host.

``influence`` turns leverages and residuals into studentised residuals and Cook's distances on the host.
"""
import numpy as np

from ._cov import checked_inputs, plan_call, plan_rows


def _effective_count(act, n, B, pinv, out):
    """free variables per problem, or the rank on the pinv route"""
    if pinv:
        return np.asarray(out[1], dtype=np.int64).copy()
    if act is None:
        return np.full(B, n, dtype=np.int64)
    return (n - np.count_nonzero(act, axis=1)).astype(np.int64)


def leverage(J, active_mask=None, ctx=None, pinv=False):
    """Leverages of the rows of one (m, n) Jacobian or of a batch (B, m, n).

    active_mask : as ``covariance``: None, or integers (n,) / (B, n), non-zero = variable held fixed (its column of J
                  is ignored).
    pinv        : False — through X = R^-1 of ``covariance(J, active_mask)``; a singular problem (status 1) has no
                  leverages.  True — through the kept singular directions of ``covariance(..., pinv=True)``: any rank.
    Returns ``(h, p, status)``: h (m,) or (B, m), NaN where status != 0; p the effective parameter count (the number
    of free variables, or the rank for pinv; sum(h) = p up to rounding), an int or (B,); status as ``covariance``.
    One plan and one copy of J to the GPU: blsq_cov[_pinv], then blsq_cov_rows on the staged J.
    """
    Jb, act, _, single = checked_inputs(J, active_mask, pinv, None)
    B, m, n = Jb.shape
    out, h = plan_call(Jb, act, None, bool(pinv), ctx, lambda c, hd: plan_rows(c, hd, B, m))
    status = out[-1]
    p = _effective_count(act, n, B, bool(pinv), out)
    if single:
        return h[0], int(p[0]), int(status[0])
    return h, p, status


def prediction_variance(J, J_new, active_mask=None, ctx=None, pinv=False, scale=None):
    """``var[i] = scale * a_i C a_i^T`` for the rows a_i of J_new, C the covariance that
    ``covariance(J, active_mask, pinv=pinv)`` would return (never formed here).

    J      : (m, n) or (B, m, n), the Jacobian of the fit;  J_new : (m_new, n) or (B, m_new, n) — a 2-D J_new with a
             batch J serves every problem.  Columns of J_new that belong to active variables are never read: those
             parameters are held fixed.
    scale  : None, a scalar or (B,), applied on the GPU (on either route).
    Returns ``(var, status)``: var (m_new,) or (B, m_new), NaN where status != 0.

    A confidence band after ``popt, pcov, info, _, _ = curve_fit(f, x, y, full_output=True)``: with
    ``J = jac(x, *popt)`` (times 1 / sigma if sigma was given), ``J_new = jac(x_new, *popt)`` the model Jacobian at
    popt on the new abscissae and ``scale = sum(info['fvec']**2) / (m - n)`` (curve_fit's residual variance,
    obj_value / (m - n); 1 with absolute_sigma), ``f(x_new, *popt) +- t * sqrt(var)`` is the band.
    """
    Jb, act, sc, single = checked_inputs(J, active_mask, pinv, scale)
    B, m, n = Jb.shape
    A = np.asarray(J_new, dtype=np.float64)
    if A.ndim not in (2, 3) or (single and A.ndim != 2):
        raise ValueError("`J_new` must have shape (m_new, n) or (B, m_new, n) matching `J`.")
    if A.ndim == 2:
        A = np.broadcast_to(A, (B,) + A.shape)
    if A.shape[0] != B or A.shape[2] != n:
        raise ValueError("`J_new` must have shape (m_new, n) or (B, m_new, n) matching `J`.")
    if A.shape[1] == 0:
        raise ValueError("`J_new` must not be empty.")
    A = np.ascontiguousarray(A)
    rows = A.shape[1]
    out, var = plan_call(Jb, act, None, bool(pinv), ctx, lambda c, hd: plan_rows(c, hd, B, rows, A, sc))
    status = out[-1]
    if single:
        return var[0], int(status[0])
    return var, status


def influence(h, f, p):
    """Studentised residuals and Cook's distances from leverages h, residuals f (both (m,) or (B, m)) and the
    effective parameter count p (scalar or (B,)) -> ``(student, cook)``:

        s^2 = sum(f^2) / (m - p),  student_i = f_i / (s sqrt(1 - h_i)),  cook_i = student_i^2 h_i / (p (1 - h_i)).

    Pure numpy on the host, evaluated under ``np.errstate(divide='ignore', invalid='ignore')``: at h_i = 1 (a point the
    fit passes through exactly), at m = p or at p = 0 the result is whatever IEEE arithmetic gives (inf or NaN), with
    no warning and no exception.
    """
    h = np.asarray(h, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    if h.shape != f.shape or h.ndim not in (1, 2):
        raise ValueError("`h` and `f` must both have shape (m,) or (B, m).")
    p = np.asarray(p, dtype=np.float64)
    if p.shape not in ((), h.shape[:-1]):
        raise ValueError("`p` must be a scalar or have shape (B,).")
    m = f.shape[-1]
    pe = p[..., None] if p.ndim else p
    with np.errstate(divide='ignore', invalid='ignore'):
        s2 = np.sum(f * f, axis=-1, keepdims=True) / (m - pe)
        student = f / np.sqrt(s2 * (1.0 - h))
        cook = student * student * h / (pe * (1.0 - h))
    return student, cook
