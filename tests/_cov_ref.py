"""Extended-precision references for the covariance tests (tests/test_cov_cpu.py, tests/test_cov_gpu.py).

Two references, each checked against a SECOND evaluation of higher precision before it is used:

  small (m <= 512, n <= 64)   mpmath at 50 digits: G = J^T J formed exactly from the doubles, inverted; the second
                              evaluation is the same at 100 digits.  numpy.longdouble is only ~2000x finer than double
                              and sits on its own error beyond kappa ~ 1e2, so it is not used here.
  large (kappa_2 <= 1e2)      a longdouble Householder triangle R, X = R^-1 by back substitution, C = X X^T.  The
                              second evaluation is one Newton-Schulz step C1 = C0 + C0 (I - G C0) whose residual is
                              EXACT: the large cases are drawn on a fixed-point grid (`quantise`), so G = J^T J and
                              G C0 are sums of float64 matrix products of short integer chunks, each exact, added up in
                              Python integers.  C1's error is the square of C0's (plus one longdouble rounding).

`reference(J)` asserts that the reference is at least 100x closer to the second evaluation than scipy's float64 SVD
recipe (curve_fit's lines, `svd_recipe`) is, and returns the reference with the bound the GPU result must meet:
4x the recipe's error against the reference, with a floor of 8 n eps.
"""
import numpy as np

EPS = np.finfo(float).eps
LD = np.longdouble
GRID_BITS = 24                      # large cases: entries are multiples of 2^-24, |entry| < 2^4


def cov_error(C, Cref):
    """max_ij |C - C*|_ij / sqrt(C*_ii C*_jj), evaluated in longdouble."""
    Cref = np.asarray(Cref, dtype=LD)
    d = np.sqrt(np.diag(Cref))
    return float(np.max(np.abs(np.asarray(C, dtype=LD) - Cref) / np.outer(d, d)))


def svd_recipe(J):
    """scipy.optimize.curve_fit's covariance from the final Jacobian (scipy 1.15.3 _minpack_py.py, restated)."""
    from scipy.linalg import svd
    _, s, VT = svd(J, full_matrices=False)
    threshold = EPS * max(J.shape) * s[0]
    s = s[s > threshold]
    VT = VT[:s.size]
    return np.dot(VT.T / s ** 2, VT)


def make_jacobian(rng, m, n, kappa, column_scales=False, grid=False):
    """J = U diag(s) V^T with s log-spaced over [1/kappa, 1], optionally with column scales e^U(-2, 2), optionally
    rounded to the fixed-point grid of the large cases (which moves kappa by a relative 1e-7 at most)."""
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    J = (U * s) @ V.T
    if column_scales:
        J = J * np.exp(rng.uniform(-2.0, 2.0, n))
    if grid:
        J = quantise(J * np.sqrt(m))              # entries of order one
    return np.ascontiguousarray(J)


def quantise(J):
    J = np.round(np.asarray(J, dtype=float) * 2.0 ** GRID_BITS) / 2.0 ** GRID_BITS
    assert np.max(np.abs(J)) < 16.0
    return J


# ---- mpmath --------------------------------------------------------------------------------------
def _mp_gram(J, dps):
    import mpmath as mp
    mp.mp.dps = dps
    m, n = J.shape
    cols = [[mp.mpf(float(v)) for v in J[:, j]] for j in range(n)]
    G = mp.zeros(n, n)
    for i in range(n):
        for j in range(i, n):
            G[i, j] = G[j, i] = mp.fdot(cols[i], cols[j])
    return G


def mp_covariance(J, dps=50):
    """inv(J^T J) with G exact from the doubles -> mpmath matrix (at `dps` digits)."""
    import mpmath as mp
    G = _mp_gram(np.asarray(J, dtype=float), dps)
    mp.mp.dps = dps
    return mp.inverse(G)


def _mp_error(C, Cmp, dps):
    """cov_error of a float / longdouble array against an mpmath matrix, evaluated in mpmath."""
    import mpmath as mp
    mp.mp.dps = dps
    n = Cmp.rows
    d = [mp.sqrt(Cmp[i, i]) for i in range(n)]
    worst = mp.mpf(0)
    for i in range(n):
        for j in range(n):
            c = C[i, j]
            c = mp.mpf(c) if isinstance(c, mp.mpf) else _ld_to_mp(c)
            e = abs(c - Cmp[i, j]) / (d[i] * d[j])
            if e > worst:
                worst = e
    return float(worst)


def _ld_to_mp(v):
    import mpmath as mp
    v = LD(v)
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def _mp_to_ld(Cmp):
    import mpmath as mp
    n = Cmp.rows
    out = np.empty((n, n), dtype=LD)
    for i in range(n):
        for j in range(n):
            hi = float(Cmp[i, j])
            out[i, j] = LD(hi) + LD(float(Cmp[i, j] - mp.mpf(hi)))
    return out


# ---- longdouble Householder ----------------------------------------------------------------------
def ld_triangle(J):
    """Householder R (n x n, longdouble) of J (m >= n)."""
    A = np.array(J, dtype=LD)
    m, n = A.shape
    for k in range(n):
        x = A[k:, k]
        nx = np.sqrt(np.dot(x, x))
        if nx == 0:
            continue
        v = x.copy()
        v[0] += nx if x[0] >= 0 else -nx
        v /= np.sqrt(np.dot(v, v))
        A[k:, k:] -= 2.0 * np.outer(v, v @ A[k:, k:])
    return np.triu(A[:n])


def ld_covariance(J):
    R = ld_triangle(J)
    n = R.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for c in range(n):                              # R x = e_c, back substitution
        X[c, c] = 1 / R[c, c]
        for i in range(c - 1, -1, -1):
            X[i, c] = -np.dot(R[i, i + 1:c + 1], X[i + 1:c + 1, c]) / R[i, i]
    C = X @ X.T
    return (C + C.T) / 2


def _chunks(Aint_obj, bits, count):
    """A (object array of Python ints) = sum_k chunk_k * 2^(bits k), |chunk_k| < 2^bits, as float64 arrays."""
    out = []
    rest = Aint_obj
    base = 1 << bits
    for _ in range(count):
        low = np.vectorize(lambda v: ((v + (base >> 1)) % base) - (base >> 1), otypes=[object])(rest)
        out.append(low.astype(np.float64))
        rest = np.vectorize(lambda a, b: (a - b) >> bits, otypes=[object])(rest, low)
    assert not np.any(rest != 0), "chunks do not cover the integers"
    return out


def _exact_product(Aint, Bint, abits, acount, bbits, bcount):
    """A @ B of two object arrays of Python ints, exactly: float64 products of short chunks, summed as integers."""
    inner = Aint.shape[1]
    assert abits + bbits + int(np.ceil(np.log2(inner))) + 1 <= 53
    Ac, Bc = _chunks(Aint, abits, acount), _chunks(Bint, bbits, bcount)
    total = np.zeros((Aint.shape[0], Bint.shape[1]), dtype=object)
    for ka, a in enumerate(Ac):
        for kb, b in enumerate(Bc):
            P = (a @ b)
            assert np.max(np.abs(P)) < 2.0 ** 53
            total = total + (P.astype(np.int64).astype(object) << (abits * ka + bbits * kb))
    return total


def _to_int(A, shift):
    """A * 2^shift as Python integers (A float64 or longdouble, exactly representable after the shift)."""
    A = np.asarray(A, dtype=LD)
    hi = np.floor(np.ldexp(A, shift - 40))                            # upper part, in units of 2^(40 - shift)
    lo = np.ldexp(A, shift) - np.ldexp(hi, 40)
    assert np.all(lo == np.floor(lo)), "not on the grid"
    f = np.vectorize(lambda h, l: (int(h) << 40) + int(l), otypes=[object])
    return f(hi.astype(np.float64), lo.astype(np.float64))


def newton_refined(J, C0):
    """-> (C0q, corr): C1 = C0q + corr, one Newton-Schulz step from C0 with an exact residual (J on the grid).
    C0q is C0 rounded to a fixed-point grid (any approximate inverse serves as the starting point)."""
    m, n = J.shape
    Jint = _to_int(J, GRID_BITS)                                       # < 2^28
    G = _exact_product(Jint.T.copy(), Jint, 14, 3, 14, 3)               # exact J^T J * 2^48
    cmax = float(np.max(np.abs(C0)))
    xs = 70 - int(np.ceil(np.log2(cmax)))                               # C0q = integer * 2^-xs, 70 bits below the max
    C0q = np.ldexp(np.round(np.ldexp(np.asarray(C0, dtype=LD), xs)), -xs)
    Xint = _to_int(C0q, xs)
    gbits = max(int(v).bit_length() for v in G.ravel())
    GX = _exact_product(G, Xint, 14, (gbits + 14) // 14 + 1, 14, 7)      # exact G C0q * 2^(48 + xs)
    one = 1 << (2 * GRID_BITS + xs)
    Rint = -GX
    for i in range(n):
        Rint[i, i] += one
    scale = LD(2.0) ** (-(2 * GRID_BITS + xs))
    Rm = np.vectorize(lambda v: LD(v), otypes=[LD])(Rint) * scale       # I - G C0q: tiny, so longdouble keeps it
    corr = C0q @ Rm
    return C0q, (corr + corr.T) / 2


# ---- the checked reference -----------------------------------------------------------------------
def reference(J, force=None):
    """-> dict(C: reference covariance (longdouble), kind, err_reference, err_recipe, bound).

    Asserts err(reference vs second evaluation) * 100 <= err(float64 SVD recipe vs second evaluation)."""
    J = np.ascontiguousarray(J, dtype=float)
    m, n = J.shape
    Crec = svd_recipe(J)
    assert Crec.shape == (n, n)
    small = m <= 512 and n <= 64
    kind = force or ("mpmath" if small else "longdouble")
    if kind == "mpmath":
        C50 = mp_covariance(J, 50)
        C100 = mp_covariance(J, 100)
        err_ref = _mp_error(C50, C100, 100)
        err_rec2 = _mp_error(Crec, C100, 100)
        C = _mp_to_ld(C50)
    else:
        C = ld_covariance(J)
        if small:                                                       # the second evaluation is affordable in mpmath
            C2 = mp_covariance(J, 60)
            err_ref = _mp_error(C, C2, 60)
            err_rec2 = _mp_error(Crec, C2, 60)
        else:
            C0q, corr = newton_refined(J, C)
            d = np.sqrt(np.diag(C0q + corr))
            dd = np.outer(d, d)
            err_ref = float(np.max(np.abs((C - C0q) - corr) / dd))
            err_rec2 = float(np.max(np.abs((np.asarray(Crec, dtype=LD) - C0q) - corr) / dd))
            # the step has converged: its error is second order in its correction, at most kappa(G) <= 1e4 times
            # the correction squared (1e-20 here), which is below the longdouble rounding of C0q + corr itself
            assert float(np.max(np.abs(corr) / dd)) < 1e-12
    assert err_ref * 100 <= err_rec2, ("reference not 100x finer than the float64 recipe", kind, (m, n), err_ref, err_rec2)
    err_rec = cov_error(Crec, C)
    return dict(C=C, kind=kind, err_reference=err_ref, err_recipe=err_rec, bound=max(4 * err_rec, 8 * n * EPS))
