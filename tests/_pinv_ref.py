"""Extended-precision references for the pseudo-inverse covariance (tests/test_pinv_cpu.py, tests/test_pinv_gpu.py).

The quantity: C* = sum over the singular values s_k of J above thr * s_max of v_k v_k^T / s_k^2, thr = eps * max(m, n)
(scipy.optimize.curve_fit's lines, `_cov_ref.svd_recipe`).

  small (n <= 32)    mpmath at 50 digits: G = J^T J exact from the doubles (`_cov_ref._mp_gram`), `mp.eigsy`, the sum
                     over the eigenvalues lambda_k > thr^2 lambda_max.  Second evaluation: the same at 100 digits.
                     Asserted: the reference is at least 100x closer to the second evaluation than the float64 recipe.
  doubled (large)    J = [A A] under a column permutation, A of full rank (kappa_2 = 50, on the fixed-point grid):
                     J^T J = K^T (A^T A) K with K = [I I], K^+ = K^T / 2, so C* = 1/4 [[C_A, C_A], [C_A, C_A]] EXACTLY,
                     with C_A = inv(A^T A) from the checked `_cov_ref.reference(A)`.

Gap condition, asserted by both: no singular value within a factor 100 of the threshold (there the answer is decided by
rounding noise in any implementation, scipy's included).

Metric and bound are the project's: `cov_error` = max |C - C*|_ij / sqrt(C*_ii C*_jj) <= max(4 x the recipe's error
against the same reference, 8 n eps).  An exactly zero column makes C*_jj = 0: `check` asserts that those rows and
columns of C are exactly 0.0 and applies the metric to the remaining block.
"""
import numpy as np

import _cov_ref as ref
from _cov_ref import EPS, LD, cov_error, svd_recipe

GAP = 100.0


class GapError(AssertionError):
    pass


def assert_gap(s_rel, thr, what=""):
    """s_rel: singular values over the largest.  None may lie in [thr / GAP, thr * GAP]."""
    s_rel = np.asarray(s_rel, dtype=float)
    near = (s_rel >= thr / GAP) & (s_rel <= thr * GAP)
    if np.any(near):
        raise GapError("singular value within a factor %g of the threshold %.3g: %s %s"
                       % (GAP, thr, s_rel[near], what))


def _mp_pinv(J, dps):
    """-> (C as an mpmath matrix, relative singular values as floats, rank) at `dps` digits."""
    import mpmath as mp
    J = np.asarray(J, dtype=float)
    m, n = J.shape
    G = ref._mp_gram(J, dps)
    mp.mp.dps = dps
    lam, Q = mp.eigsy(G)
    lmax = max(lam)
    C = mp.zeros(n, n)
    if lmax <= 0:
        return C, np.zeros(n), 0
    thr = mp.mpf(EPS) * max(m, n)
    rel = []
    rank = 0
    for k in range(n):
        lk = lam[k] if lam[k] > 0 else mp.mpf(0)
        rel.append(float(mp.sqrt(lk / lmax)))
        if lk > thr * thr * lmax:
            rank += 1
            q = Q[:, k]
            C += (q * q.T) / lk
    return C, np.array(rel), rank


def _mp_err(C, Cmp, keep, dps):
    """cov_error over the index set `keep` of an array (float / longdouble) or mpmath matrix against an mpmath one."""
    import mpmath as mp
    mp.mp.dps = dps
    d = {i: mp.sqrt(Cmp[i, i]) for i in keep}
    worst = mp.mpf(0)
    for i in keep:
        for j in keep:
            c = C[i, j]
            c = c if isinstance(c, mp.mpf) else ref._ld_to_mp(c)
            e = abs(c - Cmp[i, j]) / (d[i] * d[j])
            if e > worst:
                worst = e
    return float(worst)


def reference_small(J):
    """-> dict(C longdouble (n, n), rank, zero (indices with C*_jj = 0), rel (s / s_max), err_reference, err_recipe,
    bound).  mpmath; n <= 32."""
    J = np.ascontiguousarray(J, dtype=float)
    m, n = J.shape
    assert n <= 32, "mpmath eigen-decompositions beyond n = 32 take too long for the suite"
    thr = EPS * max(m, n)
    C50, rel, rank = _mp_pinv(J, 50)
    assert_gap(rel, thr, "(%d x %d)" % (m, n))
    C100, rel100, rank100 = _mp_pinv(J, 100)
    assert rank == rank100
    zero = [j for j in range(n) if not np.any(J[:, j])]
    keep = [j for j in range(n) if j not in zero]
    Crec = svd_recipe(J)
    err_ref = _mp_err(C50, C100, keep, 100)
    err_rec2 = _mp_err(Crec, C100, keep, 100)
    assert err_ref * 100 <= err_rec2, ("reference not 100x finer than the float64 recipe", (m, n), err_ref, err_rec2)
    C = ref._mp_to_ld(C50)
    for j in zero:                                   # (exact: a zero column is a null vector e_j of G)
        C[j, :] = 0
        C[:, j] = 0
    err_rec = _block_error(Crec, C, keep)
    return dict(C=C, rank=rank, zero=zero, rel=rel, err_reference=err_ref, err_recipe=err_rec,
                bound=max(4 * err_rec, 8 * n * EPS), kind="mpmath")


def _block_error(C, Cref, keep):
    if not keep:
        return 0.0
    ix = np.ix_(keep, keep)
    return cov_error(np.asarray(C)[ix], np.asarray(Cref)[ix])


def doubled_case(seed, m, na, kappa=50.0):
    """J = [A A] P (m x 2 na, rank na) and its reference record (as reference_small's)."""
    rng = np.random.default_rng(seed)
    A = ref.make_jacobian(rng, m, na, kappa, grid=True)
    rA = ref.reference(A)
    n = 2 * na
    perm = rng.permutation(n)
    J = np.ascontiguousarray(np.hstack([A, A])[:, perm])
    CA = np.asarray(rA["C"], dtype=LD)
    C = (np.block([[CA, CA], [CA, CA]]) / 4)[np.ix_(perm, perm)]
    s = np.linalg.svd(J, compute_uv=False)
    thr = EPS * max(m, n)
    assert_gap(s / s[0], thr, "(doubled %d x %d)" % (m, n))
    assert int(np.sum(s > thr * s[0])) == na
    err_rec = cov_error(svd_recipe(J), C)
    return J, dict(C=C, rank=na, zero=[], rel=s / s[0], err_reference=rA["err_reference"], err_recipe=err_rec,
                   bound=max(4 * err_rec, 8 * n * EPS), kind="doubled")


def full_rank(J):
    """The record of a full-rank J from the checked `_cov_ref.reference` (inverse = pseudo-inverse), gap asserted."""
    J = np.asarray(J, dtype=float)
    m, n = J.shape
    r = dict(ref.reference(J))
    s = np.linalg.svd(J, compute_uv=False)
    assert_gap(s / s[0], EPS * max(m, n), "(full rank %d x %d)" % (m, n))
    r.update(rank=n, zero=[], rel=s / s[0])
    return r


def check(C, r, label=""):
    """C against a record: exactly symmetric, exact zeros where C* has a zero diagonal, the metric on the rest within
    the bound.  Prints and returns the error."""
    C = np.asarray(C)
    n = C.shape[0]
    assert np.array_equal(C, C.T), (label, "not exactly symmetric")
    for j in r["zero"]:
        assert np.all(C[j] == 0.0) and np.all(C[:, j] == 0.0), (label, "zero column", j)
    keep = [j for j in range(n) if j not in r["zero"]]
    err = _block_error(C, r["C"], keep)
    print("%s: rank %d, error %.3g, bound %.3g (recipe %.3g, reference %.3g, %s), ratio to bound %.3g"
          % (label, r["rank"], err, r["bound"], r["err_recipe"], r["err_reference"], r["kind"], err / r["bound"]))
    assert err <= r["bound"], (label, err, r["bound"])
    return err


# ---- the small inputs the tests share ------------------------------------------------------------
def duplicated_column(seed, m, n, kappa=10.0):
    """A well-conditioned (m, n) matrix whose last column repeats its first (rank n - 1; n >= 2)."""
    rng = np.random.default_rng(seed)
    J = ref.make_jacobian(rng, m, n - 1, kappa)
    return np.ascontiguousarray(np.hstack([J, J[:, :1]]))


def dependent_column(seed, m=300, n=18, kappa=1e3):
    """kappa = 1e3 over n - 1 columns plus their rounded sum-like combination (rank n - 1 up to rounding)."""
    rng = np.random.default_rng(seed)
    J = ref.make_jacobian(rng, m, n - 1, kappa)
    c = J @ rng.standard_normal(n - 1)
    return np.ascontiguousarray(np.hstack([J, c[:, None]]))


def wide(seed, m=6, n=10):
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((m, n)))


def zero_column(seed, m=40, n=5, col=2):
    J = ref.make_jacobian(np.random.default_rng(seed), m, n, 10.0)
    J[:, col] = 0.0
    return J
