"""Bin-integrated fit models without a GPU: the numpy definition ``models.binned`` against 40-digit
quadrature of the point-sampled terms, its identities, the argument checks of ``curve_fit_batch(..., binned=True)`` and
the host-route fit that pins why the feature exists."""
import mpmath as mp
import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

import _binned_cases as bc

EPS = bc.EPS
TERMS_1D = ["gauss", "lorentz", "pvoigt", "exp", "poly"]


def spec_of(term):
    return "poly*4" if term == "poly" else term + "*1"


def definition_at(term, P, lo, hi):
    """Value (G,) and columns (G, n) of the binned term: one problem per grid point, one bin each."""
    M = models.binned(spec_of(term))
    x = np.stack([lo, hi], axis=1)[:, :, np.newaxis]                       # (G, 2, 1)
    return M.f(x, P)[:, 0], M.jac(x, P)[:, 0, :]


@pytest.fixture(scope="module")
def references():
    """The quadrature references, computed once: term -> (P, lo, hi, value) on the full grid and (P, lo, hi, value,
    columns) on the sub-grid."""
    out = {}
    for term in TERMS_1D:
        P, lo, hi = bc.definition_grid(term)
        Ps, los, his = bc.definition_grid(term, sub=True)
        out[term] = ((P, lo, hi, bc.quad_reference(term, P, lo, hi, False)[0]),
                     (Ps, los, his) + bc.quad_reference(term, Ps, los, his, True))
    return out


@pytest.mark.parametrize("term", TERMS_1D)
def test_definition_against_quadrature(references, term):
    """``models.binned`` in float64 against mp.quad of the point-sampled term at 40 digits (values over the whole grid of
    ``_binned_cases.definition_grid``; columns, by mp.diff of the quadrature, over every second zl and width): the worst
    |error| / (eps * magnitude * conditioning) of the term stays below twice ``_binned_cases.MEASURED``, the figure
    measured here (the comment there defines magnitude and conditioning)."""
    (P, lo, hi, ref), (Ps, los, his, refs, Jrefs) = references[term]
    val, _ = definition_at(term, P, lo, hi)
    mag, _, cond = bc.term_magnitudes(term, P, lo, hi)
    worst = float(bc.err_over(val, ref, mag * cond).max())
    vals, Js = definition_at(term, Ps, los, his)
    mags, Jmags, conds = bc.term_magnitudes(term, Ps, los, his)
    per_col = bc.err_over(Js, Jrefs, Jmags * conds[:, np.newaxis]).max(axis=0)
    worst_all = max(worst, float(per_col.max()))
    print("binned %s: worst error / (eps magnitude conditioning)  value %.2f  columns %s" %
          (term, worst, np.array2string(per_col, precision=2)))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(Js))
    assert worst_all <= 2 * bc.MEASURED[term], (term, worst_all)


@pytest.mark.parametrize("term", TERMS_1D)
def test_no_point_loses_more_than_its_cancellation_explains(references, term):
    """The relative error of the value at every grid point is below LOSS_CAP eps times the cancellation factor
    (|E_h| + |E_l|) / |E_h - E_l| of the form used times the conditioning of a tail, 1 + z^2.  The plain difference of two
    erf values does not pass: with both edges in one tail it loses every digit, and this check sees it."""
    P, lo, hi, ref = references[term][0]
    val, _ = definition_at(term, P, lo, hi)
    mag, _, cond = bc.term_magnitudes(term, P, lo, hi)
    ratio = bc.err_over(val, ref, mag * cond)
    assert float(ratio.max()) <= bc.LOSS_CAP, (term, float(ratio.max()))
    if term == "gauss":
        from scipy import special
        a, mu, s = P[:, 0], P[:, 1], P[:, 2]
        zl, zh = (lo - mu) / s, (hi - mu) / s
        plain = a * (s * models.SQRT_PI_2) * (special.erf(zh * models.SQRT_HALF) - special.erf(zl * models.SQRT_HALF))
        bad = bc.err_over(plain, ref, mag * cond)
        assert float(bad.max()) > 1e6 * bc.LOSS_CAP


def test_gauss2d_against_quadrature():
    """The pixel-integrated gauss2d against the product of the two 40-digit quadratures of its separable peak plus
    c w_u w_v, and its columns by mp.diff of that; magnitudes: the products of the 1-D magnitudes, as the four columns are
    the products of the 1-D forms (value: |a| I_u I_v + |c| w_u w_v); conditioning 1 + the largest z^2 of the four
    edges; the column of c is w_u w_v exactly."""
    mp.mp.dps = 40
    P, px = bc.gauss2d_grid()
    M = models.binned("gauss2d")
    x = px.T[np.newaxis, :, :]                                            # (1, 4, G)
    val, J = M.f(x, P[np.newaxis])[0], M.jac(x, P[np.newaxis])[0]
    worst = 0.0
    for g in range(px.shape[0]):
        e = [mp.mpf(float(v)) for v in px[g]]

        def I(p):
            gu = mp.quad(lambda t: mp.exp(-((t - p[1]) / p[3]) ** 2 / 2), [e[0], e[1]])
            gv = mp.quad(lambda t: mp.exp(-((t - p[2]) / p[3]) ** 2 / 2), [e[2], e[3]])
            return p[0] * gu * gv + p[4] * (e[1] - e[0]) * (e[3] - e[2])
        p = [mp.mpf(float(v)) for v in P]
        one = np.ones(1)
        Tu, Cu, cu = bc.term_magnitudes("gauss", np.array([[1.0, P[1], P[3]]]), px[g, 0] * one, px[g, 1] * one)
        Tv, Cv, cv = bc.term_magnitudes("gauss", np.array([[1.0, P[2], P[3]]]), px[g, 2] * one, px[g, 3] * one)
        (Iu, mu_u, s_u), (Iv, mu_v, s_v) = Cu[0], Cv[0]                    # magnitudes of the 1-D value and columns
        ww = (px[g, 1] - px[g, 0]) * (px[g, 3] - px[g, 2])
        cond = max(cu[0], cv[0])
        worst = max(worst, float(abs(mp.mpf(float(val[g])) - I(p)) / (mp.mpf(EPS) * (abs(P[0]) * Iu * Iv + abs(P[4]) * ww)
                                                                       * cond)))
        scales = [Iu * Iv, abs(P[0]) * mu_u * Iv, abs(P[0]) * Iu * mu_v, abs(P[0]) * (s_u * Iv + Iu * s_v)]
        for j in range(4):
            ref = mp.diff(lambda v: I(p[:j] + [v] + p[j + 1:]), p[j])
            worst = max(worst, float(abs(mp.mpf(float(J[g, j])) - ref) / (mp.mpf(EPS) * scales[j] * cond)))
        assert J[g, 4] == ww
    print("binned gauss2d: worst error / (eps magnitude conditioning) %.2f" % worst)
    assert worst <= 2 * bc.MEASURED["gauss2d"]


# ---- identities ------------------------------------------------------------------------------------------------------
SPEC_ALL = "gauss+lorentz+pvoigt+exp+poly*3"
P_ALL = np.array([[2.0, 0.3, 1.1, 3.0, -0.5, 0.7, 1.5, 0.2, 0.9, 0.4, 2.0, 0.3, 1.0, 0.5, -0.2],
                  [1.0, -0.4, 0.6, 2.0, 0.8, 1.3, 2.5, -0.1, 0.5, 0.7, 1.0, -0.2, 0.3, -0.1, 0.05]])


def test_contiguous_bins_telescope():
    """sum_i mu_i over m contiguous bins equals the one-bin integral over [e_0, e_m].  Bound: every bin value is a
    difference F(hi) - F(lo) of antiderivative-like quantities computed within a few eps of the term magnitudes T_i
    (the sum of absolute values the definition test uses), and the m - 1 additions add eps each on the running sum:
    |sum - whole| <= eps [16 sum_i T_i + 16 T_whole + m sum_i |mu_i|]."""
    M = models.binned(SPEC_ALL)
    m = 37
    edges = np.sort(np.random.default_rng(3).uniform(-3.0, 4.0, m + 1))
    parts = M.f(edges, P_ALL)
    whole = M.f(edges[[0, -1]], P_ALL)[:, 0]

    def magnitude(e):
        lo, hi = e[:-1], e[1:]
        T, o = np.zeros((P_ALL.shape[0], lo.size)), 0
        for fam, K in models.compose(SPEC_ALL).components:
            w = K * models.TERMS[fam].n_per_term
            for b in range(P_ALL.shape[0]):
                T[b] += bc.term_magnitudes(fam, np.tile(P_ALL[b, o:o + w], (lo.size, 1)), lo, hi)[0]
            o += w
        return T
    bound = EPS * (16 * magnitude(edges).sum(axis=1) + 16 * magnitude(edges[[0, -1]])[:, 0]
                   + m * np.abs(parts).sum(axis=1))
    assert np.all(np.abs(parts.sum(axis=1) - whole) <= bound), (np.abs(parts.sum(axis=1) - whole), bound)


def test_narrow_bins_tend_to_the_point_model_quadratically():
    """mu_i / w - model(centre) = w^2 model''(centre) / 24 + O(w^4): halving w divides it by 4, within 10 %."""
    Mb, Mp = models.binned(SPEC_ALL), models.compose(SPEC_ALL)
    centres = np.array([-1.3, -0.2, 0.45, 1.7])
    diffs = []
    for w in (0.08, 0.04, 0.02):
        x = np.stack([centres - w / 2, centres + w / 2])
        diffs.append(Mb.f(x, P_ALL) / w - Mp.f(centres, P_ALL))
    for coarse, fine in zip(diffs, diffs[1:]):
        np.testing.assert_allclose(coarse / fine, 4.0, rtol=0.1)


@pytest.mark.parametrize("name,spec,n", [("gauss_sum", "gauss*3+poly*1", 10), ("lorentz_sum", "lorentz*2+poly*1", 7),
                                         ("exp_sum", "exp*2+poly*1", 5), ("poly", "poly*5", 5)])
def test_named_families_are_their_composites_bit_for_bit(name, spec, n):
    rng = np.random.default_rng(5)
    P = rng.uniform(0.5, 1.5, (4, n))
    edges = np.sort(rng.uniform(-2.0, 2.0, 20))
    A, C = models.binned(name), models.binned(spec)
    assert np.array_equal(A.f(edges, P), C.f(edges, P)) and np.array_equal(A.jac(edges, P), C.jac(edges, P))
    assert np.all(A.jac(edges, P)[:, :, 0 if name == "poly" else -1] == edges[1:] - edges[:-1])     # w exactly


def test_edge_forms_give_identical_bits():
    """(m + 1,) edges, (2, m) rows, (B, m + 1) and (B, 2, m) through ``check_xdata``, and ``bin_rows``."""
    M = models.binned(SPEC_ALL)
    B, m = P_ALL.shape[0], 9
    edges = np.sort(np.random.default_rng(8).uniform(-2.0, 2.0, m + 1))
    rows = np.stack([edges[:-1], edges[1:]])
    ref_f, ref_J = M.f(edges, P_ALL), M.jac(edges, P_ALL)
    for form in (rows, np.tile(edges, (B, 1)), np.tile(rows, (B, 1, 1))):
        x, per_problem = M.check_xdata(form, B, m)
        assert x.shape[-2:] == (2, m) and per_problem == (x.ndim == 3)
        assert np.array_equal(M.f(x, P_ALL), ref_f) and np.array_equal(M.jac(x, P_ALL), ref_J)
    assert np.array_equal(models.bin_rows(edges), rows)
    assert M.n == 15 and M.name == models.compose(SPEC_ALL).name and len(M.param_names) == 15 and M.terms(15) == 7
    assert M.f(edges, P_ALL.astype(np.float32)).dtype == np.float64
    assert M.f(edges.astype(np.longdouble), P_ALL).dtype == np.longdouble


def test_the_exponential_passes_through_r_zero():
    """r = 0 and |r w| tiny: the value is a w and d / dr is -a w (lo + hi) / 2, finite and accurate."""
    M = models.binned("exp*1")
    x = np.array([[0.5], [2.0]])
    for r in (0.0, 1e-300, -1e-12, 1e-9):
        P = np.array([[3.0, r]])
        assert M.f(x, P)[0, 0] == pytest.approx(3.0 * 1.5 * (1 - r * 1.25), rel=1e-15)
        assert M.jac(x, P)[0, 0, 1] == pytest.approx(-3.0 * 1.5 * 1.25, rel=1e-8)
        assert M.jac(x, P)[0, 0, 0] == pytest.approx(1.5, rel=1e-8)


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_argument():
    B, m = 3, 6
    Y = np.ones((B, m))
    P0 = np.tile([1.0, 0.0, 1.0, 0.5], (B, 1))
    edges = np.linspace(-1.0, 1.0, m + 1)

    def fit(x, f="gauss_sum", **kw):
        return bounded_lsq.curve_fit_batch(f, x, Y, P0, binned=True, **kw)
    for bad in (np.zeros(m), np.zeros(m + 2), np.zeros((B, m)), np.zeros((3, m)), np.zeros((B + 1, m + 1)),
                np.zeros((B, 3, m)), np.zeros((4, m)), np.zeros((B, 2, m + 1))):
        with pytest.raises(ValueError, match="`xdata` of binned model 'gauss_sum' must have shape"):
            fit(bad)
    with pytest.raises(ValueError, match=r"`xdata` of binned model 'gauss2d' must have shape \(4, m\)"):
        bounded_lsq.curve_fit_batch("gauss2d", np.zeros((2, m)), Y, np.ones((B, 5)), binned=True)
    e = edges.copy()
    e[3] = e[2]
    with pytest.raises(ValueError, match="`xdata` of binned model 'gauss_sum': bin 2 has lo = .* lo < hi"):
        fit(e)
    rows = np.tile(np.stack([edges[:-1], edges[1:]]), (B, 1, 1))
    rows[1, 1, 4] = rows[1, 0, 4] - 0.1
    with pytest.raises(ValueError, match="bin 4 of problem 1 has lo"):
        fit(rows)
    e = edges.copy()
    e[5] = np.nan
    with pytest.raises(ValueError, match="bin 4 has lo = .*nan"):
        fit(e)
    e[5] = np.inf
    with pytest.raises(ValueError, match="bin 4 has lo"):
        fit(e)
    px = np.stack([np.arange(m), np.arange(m) + 1.0, np.zeros(m), np.ones(m)])
    px[3, 2] = 0.0
    with pytest.raises(ValueError, match=r"bin 2 \(coordinate 1\) has lo"):
        bounded_lsq.curve_fit_batch("gauss2d", px, Y, np.ones((B, 5)), binned=True)
    with pytest.raises(ValueError, match="`binned=True` needs a built-in model"):
        fit(edges, f=lambda x, P: np.ones((B, m)))
    with pytest.raises(ValueError, match="`sigma` must be None with estimator='poisson'"):
        fit(edges, estimator="poisson", sigma=np.ones(m))
    with pytest.raises(ValueError, match="`driver` must be"):
        fit(edges, driver="gpu")
    with pytest.raises(ValueError, match="bin edges must have shape"):
        models.bin_rows(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="unknown model"):
        models.binned("gauss_prod")


# ---- the host route --------------------------------------------------------------------------------------------------
def test_host_route_functions_recover_the_truth_where_point_sampling_is_biased():
    """The problem of the table in DESIGN.md 7n at bins 1.5 s wide (noise-free bin integrals of gauss + constant, a = 200,
    mu = 0.3, s = 1, c = 5, 24 contiguous bins, the peak 0.37 off centre), solved to 1e-13 with the numpy functions that
    ``driver='host', binned=True`` hands to the solver.  Every solver of this package steps on the GPU, so here scipy's
    least_squares drives them (tests/test_binned_gpu.py runs ``curve_fit_batch(driver='host', binned=True)`` itself on
    the same problem and asks the same): all four parameters are recovered to 1e-9; the same data fitted point-sampled
    at the bin centres against y / w has |s / s_true - 1| > 0.05 (measured: 0.094, the s^2 + w^2 / 12 of the table)."""
    from scipy.optimize import least_squares
    pr = bc.table_problem()
    Mb, Mp = models.binned(pr["name"]), models.get(pr["name"])
    lb, ub = pr["bounds"][0][0], pr["bounds"][1][0]

    def solve(M, x, y):
        return least_squares(lambda p: M.f(x, p[np.newaxis])[0] - y, pr["P0"][0], jac=lambda p: M.jac(x, p[np.newaxis])[0],
                             bounds=(lb, ub), x_scale="jac", **bc.TOL)
    got = solve(Mb, pr["edges"], pr["Y"][0])
    rel = np.abs(got.x / pr["truth"][0] - 1)
    print("binned fit: worst relative error %.2e" % rel.max())
    assert got.success and np.all(rel < 1e-9)
    pt = solve(Mp, pr["centres"], pr["Y"][0] / pr["width"])
    bias = abs(pt.x[2] / pr["truth"][0, 2] - 1)
    print("point-sampled fit of the same data: |s / s_true - 1| = %.4f, a = %.1f" % (bias, pt.x[0]))
    assert pt.success and bias > 0.05
    assert bias == pytest.approx(np.sqrt(1 + 1.5 ** 2 / 12) - 1, rel=0.1)
