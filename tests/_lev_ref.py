"""Extended-precision references for the leverage / prediction-variance tests (tests/test_leverage_cpu.py,
tests/test_leverage_gpu.py), in the convention of tests/_cov_ref.py: every reference is checked against a SECOND
evaluation before it is used.

  small (m <= 512, n <= 64)   h* = diag(A (J^T J)^-1 A^T) in mpmath at 50 digits with G = J^T J formed exactly from
                              the doubles (integer arithmetic); the second evaluation is the same at 100 digits.
  large (A = J only)          a longdouble Householder triangle R, X = R^-1 by back substitution, Q = J X, row sums
                              of squares.  The second evaluation is a different algorithm: Gram-Schmidt in longdouble,
                              every column orthogonalised and then re-orthogonalised twice, h = row sums of Q^2.

`reference(J, A, recipe)` asserts that the reference is at least 100x closer to its second evaluation than the float64
recipe — the arithmetic a user would do on the host — and returns it with the bound the GPU result must meet on
max_i |h_i - h*_i|:  max(4 x the recipe's error against the reference, 8 n eps), the rule `_cov_ref.reference` uses.

The float64 recipes (both from ``scipy.linalg.svd(J, full_matrices=False)``, singular values above curve_fit's
threshold kept):
  recipe_regular(J)      row sums of U_kept^2: the regular route's yardstick;
  recipe_rows(J, A)      row sums of (A @ (VT_kept.T / s_kept))^2: the pinv route's and prediction_variance's — the
                         recipe has to match the route's arithmetic (against the regular recipe the pinv arithmetic
                         would exceed the bound at kappa >= 1e6 with column scales).
"""
import numpy as np

from _cov_ref import make_jacobian, ld_triangle, EPS, LD  # noqa: F401  (re-exported for the tests)


# ---- float64 recipes ---------------------------------------------------------------------------------
def _kept_svd(J):
    from scipy.linalg import svd
    U, s, VT = svd(np.asarray(J, dtype=float), full_matrices=False)
    k = int(np.count_nonzero(s > EPS * max(J.shape) * s[0]))
    return U[:, :k], s[:k], VT[:k]


def recipe_regular(J):
    U, _, _ = _kept_svd(J)
    return np.sum(U * U, axis=1)


def recipe_rows(J, A):
    _, s, VT = _kept_svd(J)
    Y = np.asarray(A, dtype=float) @ (VT.T / s)
    return np.sum(Y * Y, axis=1)


# ---- exact integers and mpmath -------------------------------------------------------------------------
def _to_ints(A):
    """float64 array -> (object array of Python ints Z, e) with A = Z * 2^e exactly."""
    A = np.asarray(A, dtype=float)
    mant, ex = np.frexp(A)
    mi = np.ldexp(mant, 53).astype(np.int64)                      # exact: |mant| < 1 carries 53 bits
    nz = A != 0
    e = int(ex[nz].min()) - 53 if np.any(nz) else 0
    sh = np.where(nz, ex - 53 - e, 0)
    assert int(sh.max()) < 4000, "exponent range too wide for the integer reference"
    Z = np.array([int(a) << int(s) for a, s in zip(mi.ravel(), sh.ravel())], dtype=object).reshape(A.shape)
    return Z, e


def mp_rows(J, A=None, dps=50):
    """diag(A (J^T J)^-1 A^T) -> list of mpmath numbers (held at 120 digits).  G is exact integer arithmetic, rounded
    once to `dps` digits; the inverse is mpmath's at `dps` digits; the quadratic forms are exact integer arithmetic
    again on the inverse rounded to a fixed-point grid 8 bits finer than `dps` digits of its largest entry."""
    import mpmath as mp
    J = np.asarray(J, dtype=float)
    A = J if A is None else np.asarray(A, dtype=float)
    n = J.shape[1]
    Ji, ej = _to_ints(J)
    Gi = Ji.T.dot(Ji)                                               # G = Gi * 2^(2 ej)
    mp.mp.dps = dps
    G = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            G[i, j] = mp.mpf(int(Gi[i, j]))
    C = mp.inverse(G)                                               # (J^T J)^-1 = C * 2^(-2 ej)
    cmax = max(abs(C[i, j]) for i in range(n) for j in range(n))
    K = mp.mp.prec + 8 - int(mp.ceil(mp.log(cmax, 2)))
    Ci = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            Ci[i, j] = int(mp.nint(mp.ldexp(C[i, j], K)))
    Ai, ea = _to_ints(A)
    T = Ai.dot(Ci)
    hi = [int(v) for v in np.sum(T * Ai, axis=1)]
    mp.mp.dps = 120
    return [mp.ldexp(mp.mpf(v), 2 * ea - K - 2 * ej) for v in hi]


def _mp_max_diff(h, hmp):
    """max_i |h_i - h*_i| for a float / longdouble array against mpmath numbers, evaluated in mpmath."""
    import mpmath as mp
    mp.mp.dps = 120
    worst = mp.mpf(0)
    for v, r in zip(h, hmp):
        if not isinstance(v, mp.mpf):
            v = LD(v)
            hi = float(v)
            v = mp.mpf(hi) + mp.mpf(float(v - LD(hi)))
        worst = max(worst, abs(v - r))
    return float(worst)


def _mp_to_ld(hmp):
    import mpmath as mp
    out = np.empty(len(hmp), dtype=LD)
    for i, v in enumerate(hmp):
        hi = float(v)
        out[i] = LD(hi) + LD(float(v - mp.mpf(hi)))
    return out


# ---- longdouble ------------------------------------------------------------------------------------------
def ld_rows(J):
    """Leverages of J: Householder R in longdouble, X = R^-1 by back substitution, row sums of (J X)^2."""
    R = ld_triangle(J)
    n = R.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for c in range(n):
        X[c, c] = 1 / R[c, c]
        for i in range(c - 1, -1, -1):
            X[i, c] = -np.dot(R[i, i + 1:c + 1], X[i + 1:c + 1, c]) / R[i, i]
    Q = np.asarray(J, dtype=LD) @ X
    return np.sum(Q * Q, axis=1)


def ld_rows_gram_schmidt(J):
    """Leverages of J by a different algorithm: Gram-Schmidt in longdouble, every column orthogonalised against its
    predecessors and then re-orthogonalised twice; row sums of Q^2."""
    A = np.array(J, dtype=LD)
    m, n = A.shape
    Q = np.zeros((m, n), dtype=LD)
    for k in range(n):
        v = A[:, k].copy()
        for _ in range(3):
            if k:
                v -= Q[:, :k] @ (Q[:, :k].T @ v)
        Q[:, k] = v / np.sqrt(np.dot(v, v))
    return np.sum(Q * Q, axis=1)


# ---- the checked reference -------------------------------------------------------------------------------
def reference(J, A=None, recipe=None, force=None, base=None, n_floor=None):
    """h* = diag(A (J^T J)^-1 A^T) (A = J: the leverages) -> dict(h (longdouble), kind, err_reference, err_recipe,
    bound, second).  `recipe`: the float64 recipe's values for the same rows (default recipe_regular(J), A = J only) —
    it may come from another matrix with the same h* (a rank-deficient J with duplicated columns has the leverages of
    its independent columns; n_floor is then the width of that matrix, for the floor 8 n eps).  `base`: an earlier
    record of the same J and A, whose two evaluations are used again (another recipe, another bound).

    Asserts err(reference vs second evaluation) * 100 <= err(recipe vs second evaluation)."""
    J = np.ascontiguousarray(J, dtype=float)
    m, n = J.shape
    if recipe is None:
        assert A is None, "give the recipe that matches the route"
        recipe = recipe_regular(J)
    rows = m if A is None else np.asarray(A).shape[0]
    assert np.shape(recipe) == (rows,)
    small = m <= 512 and n <= 64
    kind = force or ("mpmath" if small else "longdouble")
    if base is not None:
        kind, h, second, err_ref = base["kind"], base["h"], base["second"], base["err_reference"]
        assert len(h) == rows
    elif kind == "mpmath":
        second = mp_rows(J, A, 100)
        h50 = mp_rows(J, A, 50)
        err_ref = _mp_max_diff(h50, second)
        h = _mp_to_ld(h50)
    else:
        assert A is None, "the longdouble reference serves A = J only"
        h = ld_rows(J)
        second = ld_rows_gram_schmidt(J)
        err_ref = float(np.max(np.abs(h - second)))
    if kind == "mpmath":
        err_rec2 = _mp_max_diff(recipe, second)
    else:
        err_rec2 = float(np.max(np.abs(np.asarray(recipe, dtype=LD) - second)))
    assert err_ref * 100 <= err_rec2, ("reference not 100x finer than the float64 recipe", kind, (m, n), err_ref,
                                       err_rec2)
    err_rec = float(np.max(np.abs(np.asarray(recipe, dtype=LD) - h)))
    return dict(h=h, kind=kind, second=second, err_reference=err_ref, err_recipe=err_rec,
                bound=max(4 * err_rec, 8 * (n_floor or n) * EPS))


def lev_error(h, href):
    """max_i |h_i - h*_i|, evaluated in longdouble."""
    return float(np.max(np.abs(np.asarray(h, dtype=LD) - np.asarray(href, dtype=LD))))
