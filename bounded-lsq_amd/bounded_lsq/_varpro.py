"""Separable fits: variable projection of the linear parameters (``separable=True``, DESIGN.md 7v;
blsq_varpro_expand_dev, blsq_varpro_reduce_dev of include/blsq.h, csrc/varpro_kernels.hip).

A model ``model(t; p) = sum_k c_k phi_k(t; alpha)`` is linear in some of its parameters: the amplitudes of its peaks and
decays, the coefficients of its polynomial, its offset.  For given non-linear parameters alpha the best linear ones
c(alpha) solve a small linear least-squares problem, so the solver needs to see alpha alone (Golub and Pereyra), with
Kaufman's Jacobian.  With

    lin    the ascending indices of the nl linear parameters, `non` the ascending indices of the na = n - nl others,
    G      (m, n) the raw Jacobian of the model with every linear parameter set to 1 and the others to alpha:
           G[:, lin] = Phi, and column j of `non` is d model / d alpha_j for a unit amplitude of the term it belongs to,
    owner  (n,): owner[j] the position in `lin` of that amplitude, -1 for a linear column,
    Phi_w = w * Phi,   A_w = [w * G[:, non] | w * y],   S = Phi_w^T Phi_w,

the scheme is

    T  = S^-1 Phi_w^T A_w       E  = A_w - Phi_w T              (project)
    T2 = S^-1 Phi_w^T E         E <- E - Phi_w T2,  T <- T + T2  (one correction against Phi_w itself)
    c  = T[:, last]             f  = -E[:, last]                 ( = w (Phi c - y) )
    J_K[:, i] = c[owner[non[i]]] * E[:, i]                       (Kaufman: P_perp (d Phi / d alpha_j) c)

``J_K^T f`` is the exact gradient of 1/2 |f|^2 because f is orthogonal to range(Phi_w).  The correction is what keeps
the answer from carrying the squared conditioning of the normal equations: the error of f, c and J_K is a small multiple
of kappa(Phi_w) eps with it, kappa^2 eps without.

S^-1 is applied through the Cholesky factor of the symmetrically scaled matrix D S D, D = diag(S)^-1/2 (unit diagonal),
which makes the pivots relative quantities: a pivot that is not above ``VARPRO_PIVOT_TOL`` = 64 eps — not positive beyond
the rounding noise of its own computation, kappa(Phi_w) of about 1e7 and more — or a diagonal entry of S that is not a
positive finite number, marks Phi as rank deficient: ``info = 1`` and NaN in f, J_K and c of that problem.

``varpro_reduce`` below IS the definition; the kernel follows the scheme (not its summation order).  The functions keep
the dtype of their inputs: np.longdouble in gives a longdouble reference.
"""
import numpy as np

VARPRO_MAX_NL = 16                           # BLSQ_VARPRO_MAX_NL
VARPRO_PIVOT_TOL = 64.0                      # ... in units of eps of the working precision

__all__ = ['VARPRO_MAX_NL', 'VARPRO_PIVOT_TOL', 'linear_params', 'varpro_reduce', 'varpro_expand',
           'separable_residual', 'separable_jacobian', 'separable_coefficients', 'separable_global_map',
           'separable_global_residual', 'separable_global_jacobian', 'separable_global_coefficients',
           'separable_global_cov']

_USE_LINEAR = ("model '%s' has no non-linear parameter left: it is a linear least-squares problem, use `lsq_linear`.")


def _components(model, n):
    """((family, K), ...) of a Model with n parameters, a CompositeModel or the binned form of either; None: gauss2d."""
    from . import _models
    if isinstance(model, _models.BinnedModel):
        model = model.base
    if isinstance(model, _models.ExprModel):
        raise ValueError("the expression model '%s' cannot be separated: the structure of a formula is not known. "
                         "Fit it without `separable=True`." % model.name)
    if isinstance(model, _models.CompositeModel):
        if n is not None:
            model.terms(n)
        return model.components, model.n
    if n is None:
        if model.n_per_term != 0:
            raise ValueError("model '%s' needs `n`: its number of terms is not fixed by its name." % model.name)
        n = model.n_base
    model.terms(n)
    if model.name == 'gauss2d':
        return None, n
    if model.name == 'poly':
        return (('poly', n),), n
    fam = _models._FAMILY_TERM[model.name]
    return ((fam, (n - 1) // _models.TERMS[fam].n_per_term), ('poly', 1)), n


def linear_params(model, n=None):
    """``(lin, owner)`` of a name, a composite spec, a ``Model``, a ``CompositeModel`` or a ``BinnedModel``: `lin` the
    ascending int32 indices of the parameters the model is linear in, `owner` (n,) int32 with, for a non-linear
    parameter, the position in `lin` of the amplitude of its term, and -1 for a linear one.  `n` is needed where the
    name does not fix it ('exp_sum', 'gauss_sum', 'lorentz_sum').

    Linear are: ``a`` of every gauss / lorentz / pvoigt / exp term, every coefficient of a ``poly*d``, ``a_k`` and ``c``
    of 'exp_sum' / 'gauss_sum' / 'lorentz_sum', ``a`` and ``c`` of 'gauss2d'.  ValueError for an ``ExprModel`` (its
    structure is unknown), for a model with nothing non-linear left ('poly', 'poly*3': use ``lsq_linear``) and for more
    than ``VARPRO_MAX_NL`` linear parameters."""
    from . import _models
    if not isinstance(model, (_models.Model, _models.CompositeModel, _models.BinnedModel, _models.ExprModel)):
        model = _models.resolve(model)
    comps, n = _components(model, n)
    owner = np.full(n, -1, dtype=np.int32)
    lin = []
    if comps is None:                            # gauss2d: (a, u0, v0, s, c)
        lin, owner[1:4] = [0, 4], 0
    else:
        o = 0
        for fam, K in comps:
            T = _models.TERMS[fam]
            if T.params is None:                 # poly*K: K coefficients
                lin += list(range(o, o + K))
                o += K
                continue
            for k in range(K):
                owner[o + 1:o + T.n_per_term] = len(lin)
                lin.append(o)
                o += T.n_per_term
    if len(lin) == n:
        raise ValueError(_USE_LINEAR % model.name)
    if len(lin) > VARPRO_MAX_NL:
        raise ValueError("model '%s' has %d linear parameters, more than VARPRO_MAX_NL = %d: fit it without "
                         "`separable=True`." % (model.name, len(lin), VARPRO_MAX_NL))
    return np.asarray(lin, dtype=np.int32), owner


def check_structure(lin, owner, n=None):
    """`lin` and `owner` as int arrays after the checks the device entries make: `lin` ascending within 0 .. n - 1,
    1 <= nl <= VARPRO_MAX_NL, at least one other parameter, ``owner[j] == -1`` exactly on `lin` and a position in `lin`
    elsewhere.  Returns (lin, owner, non)."""
    lin = np.asarray(lin, dtype=np.int64).reshape(-1)
    owner = np.asarray(owner, dtype=np.int64).reshape(-1)
    n = owner.size if n is None else int(n)
    nl = lin.size
    if owner.size != n:
        raise ValueError("`owner` must have one entry per parameter.")
    if not 1 <= nl <= VARPRO_MAX_NL:
        raise ValueError("the number of linear parameters must be in 1 .. %d, not %d." % (VARPRO_MAX_NL, nl))
    if nl >= n:
        raise ValueError("no non-linear parameter is left: use `lsq_linear`.")
    if lin[0] < 0 or lin[-1] >= n or np.any(np.diff(lin) <= 0):
        raise ValueError("`lin` must be ascending indices in 0 .. n - 1.")
    is_lin = np.zeros(n, dtype=bool)
    is_lin[lin] = True
    if np.any((owner == -1) != is_lin) or np.any(owner < -1) or np.any(owner >= nl):
        raise ValueError("`owner` must be -1 on `lin` and a position 0 .. nl - 1 in `lin` elsewhere.")
    return lin, owner, np.nonzero(~is_lin)[0]


def varpro_expand(X, lin, n):
    """The model parameters P (..., n) of the solver variables X (..., n - nl): 1.0 in the slots `lin`, X in the others
    in ascending order."""
    X = np.asarray(X)
    lin = np.asarray(lin, dtype=np.int64).reshape(-1)
    n = int(n)
    if X.shape[-1] != n - lin.size:
        raise ValueError("`X` must have n - nl = %d entries per problem, not %d." % (n - lin.size, X.shape[-1]))
    dt = np.result_type(X.dtype, np.float64)
    P = np.ones(X.shape[:-1] + (n,), dtype=dt)
    keep = np.ones(n, dtype=bool)
    keep[lin] = False
    P[..., keep] = X
    return P


def _solve_factor(S, eps):
    """D = diag(S)^-1/2, the upper Cholesky factor R of D S D (unit diagonal) by its own loops, and bad (B,): a diagonal
    entry of S that is not positive and finite, or a pivot not above VARPRO_PIVOT_TOL eps.  S: (B, nl, nl)."""
    B, nl, _ = S.shape
    dt = S.dtype
    one = dt.type(1)
    diag = np.einsum('bkk->bk', S)
    with np.errstate(all='ignore'):
        bad = ~np.all(np.isfinite(diag) & (diag > 0), axis=1)
        d = one / np.sqrt(np.where(bad[:, None], one, diag))
        A = S * d[:, :, None] * d[:, None, :]
        R = np.zeros_like(A)
        tol = dt.type(VARPRO_PIVOT_TOL) * dt.type(eps)
        for k in range(nl):
            piv = A[:, k, k] - np.einsum('bp,bp->b', R[:, :k, k], R[:, :k, k])
            bad |= ~(piv > tol)
            r = np.sqrt(np.where(bad, one, piv))
            R[:, k, k] = r
            for j in range(k + 1, nl):
                R[:, k, j] = (A[:, k, j] - np.einsum('bp,bp->b', R[:, :k, k], R[:, :k, j])) / r
    return d, R, bad


def _solve(d, R, M):
    """S^-1 M through S = D^-1 R^T R D^-1: forward and back substitution by loops.  M: (B, nl, q)."""
    nl = R.shape[1]
    Z = M * d[:, :, None]
    for k in range(nl):                          # R^T z = D M
        for p in range(k):
            Z[:, k] = Z[:, k] - R[:, p, k, None] * Z[:, p]
        Z[:, k] = Z[:, k] / R[:, k, k, None]
    for k in range(nl - 1, -1, -1):              # R t = z
        for p in range(k + 1, nl):
            Z[:, k] = Z[:, k] - R[:, k, p, None] * Z[:, p]
        Z[:, k] = Z[:, k] / R[:, k, k, None]
    return Z * d[:, :, None]


def varpro_reduce(G, y, w, lin, owner):
    """The reduced residual, Kaufman's Jacobian and the linear parameters of a batch: ``(f, J_K, c, info)`` of shapes
    (B, m), (B, m, n - nl), (B, nl) and (B,) int32, by the scheme of the module docstring.  `G`: (B, m, n) raw Jacobians
    at unit linear parameters; `y`: (B, m); `w`: None (1), (m,) or (B, m) weights 1 / sigma; `lin`, `owner`: as
    ``linear_params`` returns them.  ``info[b] = 1``, and NaN in f, J_K and c of problem b, where Phi is rank deficient
    (two identical peaks, a column of zeros).  The result has the common floating dtype of G, y and w."""
    return _reduce_full(G, y, w, lin, owner)[:4]


def _reduce_full(G, y, w, lin, owner):
    """``varpro_reduce`` and the two small matrices a separable global fit finishes its covariance with:
    ``(f, J_K, c, info, Sinv, TD)`` with ``Sinv = (Phi_w^T Phi_w)^-1`` (B, nl, nl) through the same factor and
    ``TD[:, :, i] = c[owner[non[i]]] (T + T2)[:, :, i]`` (B, nl, n - nl), computed from T after one more correction
    whose residual is formed in np.longdouble; NaN where info is 1."""
    G, y = np.asarray(G), np.asarray(y)
    if G.ndim != 3 or y.shape != G.shape[:2]:
        raise ValueError("`G` must have shape (B, m, n) and `y` (B, m).")
    B, m, n = G.shape
    lin, owner, non = check_structure(lin, owner, n)
    nl = lin.size
    if m <= nl:
        raise ValueError("m = %d points cannot determine nl = %d linear parameters and a residual." % (m, nl))
    dt = np.result_type(G.dtype, y.dtype, np.float64) if w is None else np.result_type(
        G.dtype, y.dtype, np.asarray(w).dtype, np.float64)
    G, y = G.astype(dt, copy=False), y.astype(dt, copy=False)
    if w is None:
        wy, Gw = y, G
    else:
        w = np.asarray(w).astype(dt, copy=False)
        if w.shape not in ((m,), (B, m)):
            raise ValueError("`w` must be None or have shape (m,) or (B, m).")
        w = np.broadcast_to(w, (B, m))
        wy, Gw = w * y, w[:, :, None] * G
    Pw = Gw[:, :, lin]
    Aw = np.concatenate([Gw[:, :, non], wy[:, :, None]], axis=2)
    with np.errstate(all='ignore'):
        S = np.einsum('bip,biq->bpq', Pw, Pw)
        d, R, bad = _solve_factor(S, np.finfo(dt).eps)
        T = _solve(d, R, np.einsum('bip,biq->bpq', Pw, Aw))
        E = Aw - np.einsum('bip,bpq->biq', Pw, T)
        T2 = _solve(d, R, np.einsum('bip,biq->bpq', Pw, E))
        E = E - np.einsum('bip,bpq->biq', Pw, T2)
        T = T + T2
        c = T[:, :, -1].copy()
        f = -E[:, :, -1]
        J = c[:, owner[non]][:, None, :] * E[:, :, :-1]
        Sinv = _solve(d, R, np.broadcast_to(np.eye(nl, dtype=dt), (B, nl, nl)).copy())
        Sinv = (Sinv + np.swapaxes(Sinv, 1, 2)) / dt.type(2)
        # TD needs T beyond kappa eps |T| (a column of T solves for a column of G, with a residual as large as the
        # column): one more correction with the residual in extended precision, on the unrounded w G
        xt = np.longdouble
        wx = None if w is None else w.astype(xt)
        Px = G[:, :, lin].astype(xt) if w is None else wx[:, :, None] * G[:, :, lin].astype(xt)
        Ax = np.concatenate([G[:, :, non].astype(xt), y.astype(xt)[:, :, None]], axis=2)
        if w is not None:
            Ax = wx[:, :, None] * Ax
        r = np.einsum('bip,biq->bpq', Px, Ax - np.einsum('bip,bpq->biq', Px, T.astype(xt)))
        T3 = T + _solve(d, R, r.astype(dt))
        TD = T3[:, :, -1][:, owner[non]][:, None, :] * T3[:, :, :-1]
    nan = dt.type(np.nan)
    f[bad], J[bad], c[bad], Sinv[bad], TD[bad] = nan, nan, nan, nan, nan
    return f, J, c, bad.astype(np.int32), Sinv, TD


class _HostStage:
    """The ``driver='host'`` route: the raw Jacobian of the model's numpy definition at unit linear parameters, reduced
    by ``varpro_reduce`` with the data and the weights applied inside.  One evaluation is remembered, because the solver
    asks for f and J at the same point."""

    def __init__(self, model, ydata, sigma=None, n=None, binned=False):
        from . import _models
        if not isinstance(model, (_models.Model, _models.CompositeModel, _models.BinnedModel)):
            model = _models.resolve(model)
        self.lin, self.owner = linear_params(model, n)
        self.n = self.owner.size
        self.jac_of = (_models.binned(model) if binned else model).jac
        self.y = np.asarray(ydata)
        if self.y.ndim != 2:
            raise ValueError("`ydata` must have shape (B, m).")
        B, m = self.y.shape
        self.w = None
        if sigma is not None:
            self.w = np.asarray(_models.sigma_weights(sigma, (B,), m)[0])
            if self.w.ndim == 0:
                self.w = np.broadcast_to(self.w, (m,))
        self._at = self._out = None

    def __call__(self, xdata, X):
        X = np.asarray(X)
        if self._at is None or self._at.shape != X.shape or not np.array_equal(self._at, X, equal_nan=True):
            G = self.jac_of(xdata, varpro_expand(X, self.lin, self.n))
            self._out = varpro_reduce(G, self.y, self.w, self.lin, self.owner)
            self._at = X.copy()
        return self._out


def separable_residual(model, ydata, sigma=None, n=None, binned=False, _stage=None):
    """``f(xdata, X) -> (B, m)`` over the n - nl solver variables X (B, n - nl): the reduced residual
    ``w (Phi c(X) - y)`` of `model` (a name, a spec, a ``Model`` or a ``CompositeModel``; `n` where the name does not
    fix it) against `ydata` (B, m) with weights 1 / `sigma` (None, a scalar, (m,) or (B, m)), from ``model.jac`` — or,
    with ``binned=True``, ``binned(model).jac`` — through ``varpro_reduce``.  NaN for a problem whose Phi is rank
    deficient at X."""
    stage = _stage or _HostStage(model, ydata, sigma, n, binned)
    return lambda xdata, X: stage(xdata, X)[0]


def separable_jacobian(model, ydata, sigma=None, n=None, binned=False, _stage=None):
    """``jac(xdata, X) -> (B, m, n - nl)``: Kaufman's Jacobian of ``separable_residual`` (same arguments)."""
    stage = _stage or _HostStage(model, ydata, sigma, n, binned)
    return lambda xdata, X: stage(xdata, X)[1]


def separable_coefficients(model, ydata, sigma=None, n=None, binned=False, _stage=None):
    """``coef(xdata, X) -> (B, nl)``: the linear parameters c(X) that ``separable_residual`` projects out."""
    stage = _stage or _HostStage(model, ydata, sigma, n, binned)
    return lambda xdata, X: stage(xdata, X)[2]


# ---- separable global fits ----------------------------------------------------------------------------
def separable_global_map(model, n, S, shared):
    """``(gmap, lin, owner, non)`` of a separable global fit: `gmap` the ``GlobalMap(na, S, positions of `shared` within
    non)`` over the na non-linear parameters — THE layout of the group's nv = nsh + S nloc solver variables, the shared
    ones first, then the window of data set 0, 1, ...  `shared`: a boolean mask (n,) or indices of MODEL parameters.
    ValueError for a shared linear parameter (it would couple the projections of the data sets), naming it."""
    from ._params import GlobalMap
    lin, owner = linear_params(model, n)
    n = owner.size
    a = np.asarray(shared)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError("a boolean `shared` must have shape (n,) = (%d,), not %s." % (n, a.shape))
        idx = np.flatnonzero(a).tolist()
    else:
        idx = []
        for j in np.atleast_1d(a).ravel().tolist() if a.size else []:
            if int(j) != j or not 0 <= int(j) < n:
                raise ValueError("`shared` index %r is outside 0 .. %d." % (j, n - 1))
            idx.append(int(j))
    non = np.flatnonzero(owner >= 0)
    pos = {int(j): i for i, j in enumerate(non)}
    for j in idx:
        if j not in pos:
            raise ValueError("`shared` index %d is a linear parameter: with `separable=True` it is projected out per "
                             "data set and cannot be shared (sharing it would couple the projections); fit without "
                             "`separable=True` to share it." % j)
    return GlobalMap(non.size, S, [pos[j] for j in idx]), lin, owner, non


class _HostGlobalStage:
    """The ``driver='host'`` route of a separable global fit, and its definition: every data set of every group reduced
    by ``varpro_reduce`` at its own alpha (the shared values and its window), f concatenated and Kaufman's Jacobians
    laid out by ``GlobalMap.reduce_jac``.  One evaluation is remembered."""

    def __init__(self, model, ydata, shared, sigma=None, n=None):
        from . import _models
        if not isinstance(model, (_models.Model, _models.CompositeModel)):
            model = _models.resolve(model)
        self.y = np.asarray(ydata)
        if self.y.ndim != 3:
            raise ValueError("`ydata` must have shape (G, S, m).")
        G, S, m = self.y.shape
        self.gmap, self.lin, self.owner, self.non = separable_global_map(model, n, S, shared)
        self.n = self.owner.size
        self.jac_of = model.jac
        self.w = None
        if sigma is not None:
            w, per_set = _models.sigma_weights(sigma, (G, S), m)
            self.w = np.asarray(w).reshape(G * S, m) if per_set else np.broadcast_to(w, (m,))
        self._at = self._out = None

    def __call__(self, xdata, X):
        X = np.asarray(X)
        if self._at is None or self._at.shape != X.shape or not np.array_equal(self._at, X, equal_nan=True):
            gm = self.gmap
            G, S, m = self.y.shape
            if X.shape != (G, gm.nv):
                raise ValueError("`X` must have shape (G, nv) = (%d, %d), not %s." % (G, gm.nv, X.shape))
            alpha = gm.split_x(X).reshape(G * S, gm.n)
            x = np.asarray(xdata)
            if x.ndim > 1:
                x = np.broadcast_to(x, (G, S, m)).reshape(G * S, m)
            Graw = self.jac_of(x, varpro_expand(alpha, self.lin, self.n))
            f, J, c, info, Sinv, TD = _reduce_full(Graw, self.y.reshape(G * S, m), self.w, self.lin, self.owner)
            nl = self.lin.size
            self._out = (f.reshape(G, S * m), gm.reduce_jac(J.reshape(G, S, m, gm.n)), c.reshape(G, S, nl),
                         info.reshape(G, S), Sinv.reshape(G, S, nl, nl), TD.reshape(G, S, nl, gm.n))
            self._at = X.copy()
        return self._out


def separable_global_residual(model, ydata, shared, sigma=None, n=None, _stage=None):
    """``f(xdata, X) -> (G, S m)`` over the nv solver variables X (G, nv) of ``separable_global_map``: the reduced
    residuals of the S data sets of every group, concatenated.  `ydata` (G, S, m); `sigma` None, a scalar, (m,),
    (S, m) or (G, S, m); `xdata` (m,), (S, m) or (G, S, m).  NaN in the rows of a data set whose Phi is rank deficient."""
    stage = _stage or _HostGlobalStage(model, ydata, shared, sigma, n)
    return lambda xdata, X: stage(xdata, X)[0]


def separable_global_jacobian(model, ydata, shared, sigma=None, n=None, _stage=None):
    """``jac(xdata, X) -> (G, S m, nv)``: ``GlobalMap.reduce_jac`` of Kaufman's Jacobians of the data sets, +0.0 outside
    a data set's columns (same arguments as ``separable_global_residual``)."""
    stage = _stage or _HostGlobalStage(model, ydata, shared, sigma, n)
    return lambda xdata, X: stage(xdata, X)[1]


def separable_global_coefficients(model, ydata, shared, sigma=None, n=None, _stage=None):
    """``coef(xdata, X) -> (G, S, nl)``: the linear parameters of every data set at X."""
    stage = _stage or _HostGlobalStage(model, ydata, shared, sigma, n)
    return lambda xdata, X: stage(xdata, X)[2]


def _mirror(A):
    """The upper triangle of (..., k, k) and its mirror image."""
    U = np.triu(A)
    return U + np.swapaxes(np.triu(A, 1), -1, -2)


def separable_global_cov(C, Sinv, TD, gmap, scale=None, lin=None):
    """The per-data-set blocks of the covariance of a separable global fit: (..., S, n, n) from the covariance `C`
    (..., nv, nv) of the reduced group, ``Sinv`` (..., S, nl, nl) and ``TD`` (..., S, nl, na) of every data set
    (``_reduce_full``), the layout `gmap` and `lin`, the ascending model indices of the nl linear parameters
    (n = na + nl).  Kaufman's ``J_K^T J_K`` is the Schur complement of the full Gauss-Newton matrix onto the non-linear
    variables, so C is the exact alpha-alpha block of the full covariance, and with C_s its restriction to the na
    columns of data set s

        alpha-alpha = C_s,   c-alpha = -TD_s C_s,   c-c = Sinv_s + TD_s C_s TD_s^T

    are the other blocks of data set s.  Everything is multiplied by ``scale`` (...,) where given.  The terms between
    two data sets are not formed.  Of C_s and of the c-c block the upper triangle is taken and mirrored, as the kernel
    does: the blocks are exactly symmetric."""
    if lin is None:
        raise ValueError("`lin` is required: the model indices of the linear parameters.")
    C, Sinv, TD = np.asarray(C), np.asarray(Sinv), np.asarray(TD)
    lin = np.asarray(lin, dtype=np.int64).reshape(-1)
    na, nl, S = gmap.n, lin.size, gmap.S
    n = na + nl
    if C.shape[-2:] != (gmap.nv, gmap.nv):
        raise ValueError("`C` must have shape (..., nv, nv) = (..., %d, %d), not %s." % (gmap.nv, gmap.nv, C.shape))
    lead = C.shape[:-2]
    if Sinv.shape != lead + (S, nl, nl) or TD.shape != lead + (S, nl, na):
        raise ValueError("`Sinv` and `TD` must have shapes (..., S, nl, nl) and (..., S, nl, na).")
    keep = np.ones(n, dtype=bool)
    keep[lin] = False
    non = np.flatnonzero(keep)
    dt = np.result_type(C.dtype, Sinv.dtype, TD.dtype, np.float64)
    out = np.zeros(lead + (S, n, n), dtype=dt)
    for s in range(S):
        cols = gmap.cols[s]
        Cs = _mirror(C[..., cols[:, None], cols[None, :]].astype(dt))
        W = np.einsum('...pi,...ia->...pa', TD[..., s, :, :], Cs)
        cc = _mirror(Sinv[..., s, :, :] + np.einsum('...pa,...qa->...pq', W, TD[..., s, :, :]))
        blk = out[..., s, :, :]
        blk[..., non[:, None], non[None, :]] = Cs
        blk[..., lin[:, None], non[None, :]] = -W
        blk[..., non[:, None], lin[None, :]] = -np.swapaxes(W, -1, -2)
        blk[..., lin[:, None], lin[None, :]] = cc
    if scale is not None:
        out *= np.asarray(scale, dtype=dt)[..., None, None, None]
    return out
