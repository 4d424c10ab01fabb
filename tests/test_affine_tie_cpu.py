"""Affine ties without a GPU: every ``ParamMap`` method against a dense T and d built by explicit loops,
trivial tuple ties against the int form, the ValueErrors, ``GlobalMap`` against the dense group matrix, the screening of
the fit cases by scipy, and the declaration of the new entry."""
import itertools
import os
import re

import numpy as np
import pytest

from bounded_lsq import GlobalMap, ParamMap, _abi, models

import _affine_tie_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, fixed, tied)
MAPS = {
    "doublet": (7, None, ac.DOUBLET_TIED),
    "key_below": (4, None, {0: (3, 2.0)}),
    "negative": (5, None, {2: (0, -0.5, 0.25), 4: (1, -3.0)}),
    "three_ratios": (10, None, {3: (0, 2.0 / 3.0), 6: (0, 1.0 / 3.0), 5: 2, 8: (2, 1.0, 0.0)}),
    "fixed_next": (7, [2, 6], {3: (0, 0.5, 0.1), 1: (5, 1.0, -0.3)}),
}


def dense(n, fixed, tied):
    """By explicit loops: T (n, nf), d (n,), the slot of every parameter (-1: fixed) and the leaders."""
    fixed = set(fixed or ())
    tie = {}
    for j, v in tied.items():
        v = v if isinstance(v, tuple) else (v,)
        tie[j] = (v[0], v[1] if len(v) > 1 else 1.0, v[2] if len(v) > 2 else 0.0)
    leaders = [j for j in range(n) if j not in fixed and j not in tie]
    T, d, slot = np.zeros((n, len(leaders))), np.zeros(n), [-1] * n
    for j in range(n):
        if j in fixed:
            continue
        i, r, o = tie.get(j, (j, 1.0, 0.0))
        slot[j] = leaders.index(i)
        T[j, slot[j]], d[j] = r, o
    return T, d, slot, leaders


@pytest.fixture(params=list(MAPS))
def mapped(request):
    n, fixed, tied = MAPS[request.param]
    return ParamMap(n, fixed, tied), dense(n, fixed, tied), (n, fixed, tied)


def test_attributes(mapped):
    pm, (T, d, slot, leaders), (n, fixed, tied) = mapped
    assert pm.affine and pm.nf == len(leaders) and pm.pmap.tolist() == slot and pm.leaders.tolist() == leaders
    assert np.array_equal(pm.ratio, np.where(T.any(axis=1), T.sum(axis=1), 1.0)) and np.array_equal(pm.offset, d)
    assert pm.tied == {j: (v[0] if isinstance(v, tuple) else v) for j, v in tied.items()}
    assert all(isinstance(k, int) and isinstance(v, int) for k, v in pm.tied.items())
    assert np.array_equal(pm.matrix(), T)


def test_expand_x_is_T_x_plus_d_bit_for_bit(mapped):
    pm, (T, d, slot, leaders), (n, fixed, tied) = mapped
    rng = np.random.default_rng(3)
    X, Pfix = rng.standard_normal((2, 3, pm.nf)), rng.standard_normal((2, 3, n))
    got = pm.expand_x(X, Pfix)
    for idx in itertools.product(range(2), range(3)):
        for j in range(n):
            want = Pfix[idx][j] if slot[j] < 0 else T[j, slot[j]] * X[idx][slot[j]] + d[j]   # one product, one sum
            assert got[idx][j].tobytes() == np.float64(want).tobytes()
    assert np.array_equal(pm.reduce_x(got), X)


def test_reduce_jac_is_the_sequential_sum_bit_for_bit(mapped):
    pm, (T, d, slot, leaders), (n, fixed, tied) = mapped
    J = np.random.default_rng(4).standard_normal((3, 5, n))
    got = pm.reduce_jac(J)
    for b, i, k in itertools.product(range(3), range(5), range(pm.nf)):
        acc = None
        for j in range(n):                                  # ascending j; a key below its leader arrives first
            if slot[j] == k:
                term = T[j, k] * J[b, i, j]
                acc = term if acc is None else acc + term
        assert got[b, i, k].tobytes() == np.float64(acc).tobytes()


def test_expand_cov_is_T_C_Tt(mapped):
    pm, (T, d, slot, leaders), _ = mapped
    A = np.random.default_rng(5).standard_normal((2, pm.nf, pm.nf))
    C = A @ A.transpose(0, 2, 1)
    got = pm.expand_cov(C)
    np.testing.assert_allclose(got, T @ C @ T.T, rtol=4e-16, atol=0)      # two products per entry against a dot
    for j, l in itertools.product(range(pm.n), repeat=2):
        if slot[j] >= 0 and slot[l] >= 0:
            assert np.array_equal(got[:, j, l], pm.ratio[j] * pm.ratio[l] * C[:, slot[j], slot[l]])
        else:
            assert not got[:, j, l].any()


def test_expand_mask_carries_the_sign_of_the_ratio(mapped):
    pm, (T, d, slot, leaders), _ = mapped
    mask = np.random.default_rng(6).integers(-1, 2, (4, pm.nf))
    got = pm.expand_mask(mask)
    for b, j in itertools.product(range(4), range(pm.n)):
        assert got[b, j] == (0 if slot[j] < 0 else int(np.sign(T[j, slot[j]])) * mask[b, slot[j]])
    assert got.dtype == mask.dtype


def brute_box(lb, ub, T, d, slot, k, grid):
    """The feasible x of slot k on `grid`, by scanning: every member's value r x + d inside its own box."""
    ok = np.ones(grid.shape, dtype=bool)
    for j in range(len(slot)):
        if slot[j] == k:
            v = T[j, k] * grid + d[j]
            ok &= (v >= lb[j]) & (v <= ub[j])
    return grid[ok]


def test_reduce_bounds_against_a_scan(mapped):
    pm, (T, d, slot, leaders), (n, fixed, tied) = mapped
    rng = np.random.default_rng(7)
    grid = np.linspace(-40.0, 40.0, 160001)                 # step 5e-4
    for trial in range(6):
        lb, ub = -rng.uniform(1.0, 3.0, n), rng.uniform(1.0, 3.0, n)
        lb[rng.random(n) < 0.3], ub[rng.random(n) < 0.3] = -np.inf, np.inf
        lo, hi = pm.reduce_bounds(lb, ub)
        for k in range(pm.nf):
            feas = brute_box(lb, ub, T, d, slot, k, grid)
            assert feas.size
            if np.isfinite(lo[k]):
                assert abs(feas[0] - lo[k]) <= 5e-4
            else:
                assert lo[k] == -np.inf and feas[0] == grid[0]
            if np.isfinite(hi[k]):
                assert abs(feas[-1] - hi[k]) <= 5e-4
            else:
                assert hi[k] == np.inf and feas[-1] == grid[-1]
    # batched bounds give the rows
    LB, UB = -rng.uniform(1.0, 3.0, (3, n)), rng.uniform(1.0, 3.0, (3, n))
    lo, hi = pm.reduce_bounds(LB, UB)
    for b in range(3):
        l1, h1 = pm.reduce_bounds(LB[b], UB[b])
        assert np.array_equal(lo[b], l1) and np.array_equal(hi[b], h1)


def test_reduce_bounds_negative_ratio_infinite_ends_and_empty_intersection():
    pm = ParamMap(3, None, {1: (0, -2.0, 1.0)})             # p1 = -2 p0 + 1
    lo, hi = pm.reduce_bounds([-np.inf, -3.0, 0.0], [np.inf, np.inf, 1.0])      # p1 >= -3  <=>  p0 <= 2
    assert lo.tolist() == [-np.inf, 0.0] and hi.tolist() == [2.0, 1.0]
    lo, hi = pm.reduce_bounds([0.0, -np.inf, 0.0], [5.0, 0.0, 1.0])             # p1 <= 0  <=>  p0 >= 0.5
    assert lo.tolist() == [0.5, 0.0] and hi.tolist() == [5.0, 1.0]
    with pytest.raises(ValueError, match=re.escape("the bounds of the tied parameters [0, 1] do not intersect.")):
        pm.reduce_bounds([1.0, 0.0, 0.0], [2.0, 5.0, 1.0])                      # p1 in [0, 5]  <=>  p0 in [-2, 0.5]


def test_wrap_jac_against_central_differences_of_wrap_f(mapped):
    pm, (T, d, slot, leaders), (n, fixed, tied) = mapped
    rng = np.random.default_rng(8)
    A = rng.standard_normal((6, n))

    def f(x, P):
        return np.sin(P @ A.T) + x

    def jac(x, P):
        return np.cos(P @ A.T)[..., :, None] * A
    Pfix = rng.standard_normal((2, n))
    g, gj = pm.wrap_f(f, Pfix), pm.wrap_jac(jac, Pfix)
    X = rng.standard_normal((2, pm.nf))
    J = gj(0.5, X)
    assert J.shape == (2, 6, pm.nf)
    h = 1e-6
    for k in range(pm.nf):
        E = np.zeros(pm.nf)
        E[k] = h
        np.testing.assert_allclose(J[..., k], (g(0.5, X + E) - g(0.5, X - E)) / (2 * h), rtol=0, atol=1e-8)


# ---- trivial ties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [lambda i: (i,), lambda i: (i, 1.0), lambda i: (i, 1.0, 0.0), lambda i: [i, 1]])
def test_trivial_tuple_ties_equal_the_int_form(form):
    n, fixed, tied = 8, [6], {3: 0, 5: 2, 1: 4}
    a, b = ParamMap(n, fixed, tied), ParamMap(n, fixed, {j: form(i) for j, i in tied.items()})
    assert not b.affine and b.tied == a.tied and np.array_equal(a.pmap, b.pmap)
    assert np.array_equal(b.ratio, np.ones(n)) and np.array_equal(b.offset, np.zeros(n))
    rng = np.random.default_rng(9)
    X, Pfix = rng.standard_normal((3, a.nf)), rng.standard_normal((3, n))
    X[0, 0] = X[1, 2] = -0.0
    ea, eb = a.expand_x(X, Pfix), b.expand_x(X, Pfix)
    assert np.array_equal(ea, eb) and np.array_equal(np.signbit(ea), np.signbit(eb)) and np.signbit(eb[0, 3])
    J = rng.standard_normal((3, 4, n))
    C = rng.standard_normal((3, a.nf, a.nf))
    lb, ub = -rng.uniform(1, 2, (3, n)), rng.uniform(1, 2, (3, n))
    mask = rng.integers(-1, 2, (3, a.nf))
    assert np.array_equal(a.reduce_jac(J), b.reduce_jac(J)) and np.array_equal(a.expand_cov(C), b.expand_cov(C))
    assert all(np.array_equal(p, q) for p, q in zip(a.reduce_bounds(lb, ub), b.reduce_bounds(lb, ub)))
    assert np.array_equal(a.expand_mask(mask), b.expand_mask(mask)) and np.array_equal(a.matrix(), b.matrix())
    assert np.array_equal(a.reduce_x(Pfix), b.reduce_x(Pfix))
    ga, gb = GlobalMap(n, 2, [0, 3], fixed, tied), GlobalMap(n, 2, [0, 3], fixed, {j: form(i) for j, i in tied.items()})
    Xg, Pg = rng.standard_normal((ga.nv,)), rng.standard_normal((2, n))
    assert np.array_equal(ga.expand_x(Xg, Pg), gb.expand_x(Xg, Pg)) and np.array_equal(ga.matrix(), gb.matrix())


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied, text", [
    ({2: (0, 0.0)}, "`tied` ratio 0.0 of key 2 must be finite and not 0."),
    ({2: (0, -0.0)}, "`tied` ratio -0.0 of key 2 must be finite and not 0."),
    ({2: (0, np.inf)}, "`tied` ratio inf of key 2 must be finite and not 0."),
    ({2: (0, np.nan, 1.0)}, "`tied` ratio nan of key 2 must be finite and not 0."),
    ({1: (0, 2.0, np.inf)}, "`tied` offset inf of key 1 must be finite."),
    ({1: (0, 2.0, np.nan)}, "`tied` offset nan of key 1 must be finite."),
    ({1: ()}, "`tied` value of key 1 must be i, (i, ratio) or (i, ratio, offset), not 0 entries."),
    ({1: (0, 1.0, 0.0, 2.0)}, "`tied` value of key 1 must be i, (i, ratio) or (i, ratio, offset), not 4 entries."),
    # the old ones keep their texts, in either form
    ({9: 0}, "`tied` key 9 is outside 0 .. 3."),
    ({1: (7, 2.0)}, "`tied` target 7 is outside 0 .. 3."),
    ({1: (1, 2.0)}, "`tied` ties parameter 1 to itself."),
    ({3: (0, 2.0)}, "`tied` key 3 is also fixed."),
    ({1: (3, 2.0)}, "`tied` target 3 (of parameter 1) is fixed."),
    ({1: (2, 2.0), 2: 0}, "`tied` target 2 (of parameter 1) is itself tied to 0."),
])
def test_value_errors(tied, text):
    with pytest.raises(ValueError, match=re.escape(text)):
        ParamMap(4, [3], tied)


def test_old_errors_outside_tied_keep_their_texts():
    with pytest.raises(ValueError, match=re.escape("every parameter is fixed: nothing is left to fit (nf = 0).")):
        ParamMap(2, [0], {1: (0, 2.0)}) if False else ParamMap(2, [0, 1])
    with pytest.raises(ValueError, match=re.escape("`shared` index 1 is tied to parameter 0, which is not shared.")):
        GlobalMap(3, 2, [1], None, {1: (0, 2.0)})


# ---- GlobalMap -------------------------------------------------------------------------------------------------------
def test_global_map_against_the_dense_group_matrix():
    """An affine tie in a shared slot (p4 = 2 p1 - 0.5) and another in a local slot (p3 = -0.5 p0 + 1)."""
    n, S, fixed, tied, shared = 6, 3, [5], {4: (1, 2.0, -0.5), 3: (0, -0.5, 1.0)}, [1, 4]
    gm = GlobalMap(n, S, shared, fixed, tied)
    T1, d1, slot, leaders = dense(n, fixed, tied)
    sh = [k for k, j in enumerate(leaders) if j in shared]
    lo = [k for k, j in enumerate(leaders) if j not in shared]
    nv = len(sh) + S * len(lo)
    Tg, dg = np.zeros((S * n, nv)), np.zeros(S * n)
    for s in range(S):
        for j in range(n):
            if slot[j] >= 0:
                k = slot[j]
                col = sh.index(k) if k in sh else len(sh) + s * len(lo) + lo.index(k)
                Tg[s * n + j, col], dg[s * n + j] = T1[j, k], d1[j]
    assert gm.nv == nv and np.array_equal(gm.matrix(), Tg)
    rng = np.random.default_rng(10)
    X, Pfix = rng.standard_normal((2, nv)), rng.standard_normal((2, S, n))
    want = (X @ Tg.T + dg).reshape(2, S, n)
    want[..., 5] = Pfix[..., 5]
    got = gm.expand_x(X, Pfix)
    np.testing.assert_allclose(got, want, rtol=0, atol=0)   # one product and one sum per entry (the rest adds 0.0)
    m = 4
    J = rng.standard_normal((2, S, m, n))
    Jg = gm.reduce_jac(J)
    for s in range(S):
        blk = np.zeros((2, m, nv))
        for j in range(n):                                  # ascending j
            if slot[j] >= 0:
                c = int(np.flatnonzero(Tg[s * n + j])[0])
                blk[..., c] = blk[..., c] + Tg[s * n + j, c] * J[:, s, :, j]
        assert np.array_equal(Jg[:, s * m:(s + 1) * m], blk)
    A = rng.standard_normal((nv, nv))
    C = A @ A.T
    full = Tg @ C @ Tg.T
    for s in range(S):
        np.testing.assert_allclose(gm.expand_cov(C)[s], full[s * n:(s + 1) * n, s * n:(s + 1) * n], rtol=4e-16, atol=0)
    mask = rng.integers(-1, 2, (nv,))
    assert np.array_equal(gm.expand_mask(mask).reshape(-1), (np.sign(Tg) @ mask).astype(mask.dtype))
    lb, ub = np.full((S, n), -1.0), np.full((S, n), 1.0)
    ub[1, 4] = 0.0                                          # p4 = 2 p1 - 0.5 <= 0 in data set 1: p1 <= 0.25 for all
    lo_v, hi_v = gm.reduce_bounds(lb, ub)
    assert hi_v[gm.column(gm.pm.pmap[1], 0)] == 0.25 and lo_v[gm.column(gm.pm.pmap[1], 0)] == -0.25
    assert (lo_v[gm.column(gm.pm.pmap[0], 2)], hi_v[gm.column(gm.pm.pmap[0], 2)]) == (0.0, 1.0)     # p3 = 1 - p0 / 2


# ---- the fit cases: screened by scipy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.FIT_CASES)
def test_scipy_converges_from_every_start(name):
    """The independent reference converges from the case's p0 for every problem, and it is converged where the fits
    are compared with it: the Gauss-Newton step that remains at its solution (over the variables off their bounds), which
    estimates its own distance from the minimum, is below a hundredth of the margin rtol 1e-6 / atol 1e-9 of the GPU
    tests, so the reference uses up at most 1 % of any comparison (scipy does not get closer under the Poisson deviance
    with every tolerance at 1e-15 and restarts: its remaining steps there are up to 2e-3 of the margin).  The reference keeps the constraint by construction."""
    case = ac.fit_case(name)
    popt, pcov, results, ok = ac.reference(name)
    assert ok and all(r.status > 0 for r in results)
    for r in results:
        free = r.active_mask == 0
        step = np.linalg.lstsq(r.jac[:, free], -r.fun, rcond=None)[0]
        assert np.all(np.abs(step) <= 1e-2 * (1e-9 + 1e-6 * np.abs(r.x[free])))
    assert np.array_equal(popt[..., 3], ac.RATIO * popt[..., 0]) and np.array_equal(popt[..., 4], popt[..., 1] + ac.SPLIT)
    np.testing.assert_allclose(pcov[..., 3, 3], 0.25 * pcov[..., 0, 0], rtol=1e-12)
    if name == "bound":
        assert np.all(np.abs(popt[:, 4] - case["bounds"][1][:, 4]) <= 2 * np.finfo(float).eps)      # (ub - d) + d
        assert all(list(r.active_mask) == [0, 1, 0, 0] for r in results)
    pm = ParamMap(case["n"], None, case["tied"])
    assert pm.nf == 4 and np.array_equal(pm.expand_x(pm.reduce_x(popt), popt), popt)


def test_host_callables_of_the_doublet_are_the_hand_written_ones():
    """``wrap_f`` / ``wrap_jac`` (what callables and driver='host' go through) against the residual and Jacobian the
    reference is written from."""
    case = ac.fit_case("lse")
    M = models.compose(ac.DOUBLET)
    pm = ParamMap(case["n"], None, case["tied"])
    z = case["z0"]
    assert np.array_equal(pm.expand_x(z, case["P0"]), ac.full(z))
    assert np.array_equal(pm.wrap_f(M.f, case["P0"])(case["x"], z), M.f(case["x"], ac.full(z)))
    assert np.array_equal(pm.wrap_jac(M.jac, case["P0"])(case["x"], z), ac.chain(M.jac(case["x"], ac.full(z))))


# ---- the declaration -------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_with_the_tie_pair_behind_pmap():
    code = open(os.path.join(ROOT, "include", "blsq.h")).read()
    tie = re.search(r"int\s+blsq_model_eval_tie_dev\s*\(([^)]*)\)", code)
    glo = re.search(r"int\s+blsq_model_eval_global_dev\s*\(([^)]*)\)", code)
    assert tie and glo
    names = lambda d: [re.sub(r"\s+", " ", a).strip() for a in d.group(1).split(",")]       # noqa: E731
    t, g = names(tie), names(glo)
    at = g.index("const int32_t* pmap") + 1
    assert t == g[:at] + ["const double* tie_ratio", "const double* tie_offset"] + g[at:]
    restype, argtypes = _abi.SIGNATURES["blsq_model_eval_tie_dev"]
    gtypes = _abi.SIGNATURES["blsq_model_eval_global_dev"][1]
    assert len(argtypes) == len(t) == 29
    assert argtypes == gtypes[:at] + [_abi.c_double_p, _abi.c_double_p] + gtypes[at:]
