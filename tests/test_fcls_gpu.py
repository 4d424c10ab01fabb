"""BVLS / NNLS with a sum constraint on the GPU: the solve kernel under one equality e^T x = d against
``bvls_reference(..., equality=)`` decision for decision, the certificate of every status-1 result, the whole path
(``bvls_batch(..., equality=)``, ``fcls_batch``) against the constructed solutions, conditioning, independence of the
batch mates, failure handling, the argument checks of blsq_bvls_solve_eq_dev, and the unchanged path without
``equality``.  The cases are those tests/test_fcls_cpu.py vets without a GPU.

Margins (gamma_k = k eps / (1 - k eps)):
  x           |x - x*|_inf <= 8 n eps kappa(A) max(1, |x*|_inf) (``bc.x_tolerance``), kappa = 30 by construction.
  sum         |e^T x - d| <= 4 n eps sum |e_j x_j|.
  KKT         optimality <= tol + 16 n eps max_j (|G||x| + |c| + |lambda||e|)_j (``fc.kkt_bound``), lambda recomputed in
              numpy.longdouble from g = G x - c; the reported multiplier is a weighted mean of -g_j / e_j over the free
              set, so it is within (that bound - tol) / min |e_j| of the recomputed one.
  fun, cost   those of tests/test_bvls_gpu.py::_check_whole.
  optimality  (whole path) below gamma_{m+n} max_j (|A|^T W^2 (|A||x| + |b|) + |lambda||e|)_j: the rounding of the
              reduced gradient itself.
"""
import numpy as np
import pytest

import bounded_lsq

import _bvls_cases as bc
import _fcls_cases as fc
import _linear_cases as lc
import _model_eval as me
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)
from test_bvls_gpu import moments

pytestmark = pytest.mark.gpu

BYTES = ("x", "active_mask", "optimality", "nit", "nfact", "status", "multiplier")
worst = {}


def note(name, frac):
    worst[name] = max(worst.get(name, 0.0), float(frac))


def raw_solve(ctx, entry, G, c, lb, ub, e=None, d=None, tol=1e-10, max_pass=None):
    """`entry` (blsq_bvls_solve_dev, or blsq_bvls_solve_eq_dev with e and d) on (G, c) alone, nothing checked on the
    host -> (rc, dict of x, on_bound, grad, optimality, status, nit, nfact, multiplier)."""
    B, n = c.shape
    lb, ub = np.broadcast_to(lb, (B, n)), np.broadcast_to(ub, (B, n))
    with me.Dev(ctx) as dv:
        dx, dgrad = dv.up(np.full((B, n), np.nan)), dv.up(np.full((B, n), np.nan))
        don, dstat = dv.up(np.zeros((B, n), dtype=np.int32)), dv.up(np.zeros((B, 3), dtype=np.int32))
        dopt, dmult = dv.up(np.full((B, 2), np.nan)), dv.up(np.full(B, np.nan))
        args = [ctx.h, B, 0, n, dv.up(G), n * n if G.ndim == 3 else 0, dv.up(c), dv.up(lb), dv.up(ub), tol,
                5 * n if max_pass is None else max_pass, None, 0, None, None, 0, dx, don, None, dgrad, dopt, dstat]
        if e is not None:
            e = np.asarray(e, dtype=np.float64)
            args += [dv.up(e), n if e.ndim == 2 else 0, dv.up(np.broadcast_to(np.asarray(d, dtype=np.float64), (B,))),
                     dmult]
        rc = getattr(ctx.lib, entry)(*args)
        if rc != 0:
            return rc, None
        stat = ctx.to_host(dstat, (B, 3), np.int32)
        return 0, dict(x=ctx.to_host(dx, (B, n), np.float64), on_bound=ctx.to_host(don, (B, n), np.int32),
                       grad=ctx.to_host(dgrad, (B, n), np.float64), optimality=ctx.to_host(dopt, (B, 2), np.float64)[:, 0],
                       status=stat[:, 0], nit=stat[:, 1], nfact=stat[:, 2],
                       multiplier=ctx.to_host(dmult, (B,), np.float64))


def certificate(res, p, G, c, lb, ub, e, d, what):
    """What a status-1 result carries: the box, the bounds bit for bit, the sum, and the KKT conditions with the
    multiplier recomputed in numpy.longdouble."""
    x, on = res.x[p], res.active_mask[p]
    n = len(x)
    assert np.all((x >= lb) & (x <= ub)), what
    assert same_bits(x[on < 0], lb[on < 0]) and same_bits(x[on > 0], ub[on > 0]), what
    gap, bound = abs(float(np.asarray(e, dtype=fc.L) @ np.asarray(x, dtype=fc.L) - d)), fc.sum_bound(e, x)
    print("%s: |e^T x - d| = %.3g (bound %.3g)" % (what, gap, bound))
    assert gap <= bound, (what, gap, bound)
    note("sum", gap / bound)
    g = np.asarray(G, dtype=fc.L) @ np.asarray(x, dtype=fc.L) - np.asarray(c, dtype=fc.L)
    lam = fc.multiplier_ld(g, on, e)
    kkt = fc.kkt_bound(G, c, x, e, lam)
    opt = fc.optimality_ld(g, on, e, lam)
    print("%s: optimality %.3g, recomputed %.3g (bound %.3g)" % (what, res.optimality[p], opt, kkt))
    assert opt <= kkt and res.optimality[p] <= kkt, (what, opt, res.optimality[p], kkt)
    note("KKT", max(opt, res.optimality[p]) / kkt)
    if np.any(on == 0):                                               # (F empty: any point of the interval serves)
        lam_tol = (kkt - 1e-10) / float(np.min(np.abs(e)))
        assert abs(res.multiplier[p] - float(lam)) <= lam_tol, (what, res.multiplier[p], float(lam), lam_tol)
        note("multiplier", abs(res.multiplier[p] - float(lam)) / lam_tol)


def against_reference(res, G, c, lb, ub, e, d, n, **kw):
    """Status, mask, passes and factorisations equal those of the numpy definition; x within the tolerance."""
    for p in range(c.shape[0]):
        ep = e if np.ndim(e) == 1 else e[p]
        r = bounded_lsq.bvls_reference(G if G.ndim == 2 else G[p], c[p], lb[p], ub[p], equality=(ep, d[p]), **kw)
        assert np.array_equal(res.active_mask[p], r["on_bound"]), (n, p)
        assert (res.status[p], res.nit[p], res.nfact[p]) == (r["status"], r["nit"], r["nfact"]), (n, p)
        tol = bc.x_tolerance(n, r["x"])
        err = np.max(np.abs(res.x[p] - r["x"]))
        assert err <= tol, (n, p, err, tol)
        note("gram x (vs definition)", err / tol)


# ---- the solve on (G, c) alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.GRAM_NS)
def test_gram_solve_against_the_definition(ctx, n):
    case = fc.gram_case(n)
    G, c, lb, ub, e, d = case["G"], case["c"], case["lb"], case["ub"], case["e"], case["d"]
    res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, d))
    assert res.fun is None and res.cost is None and res.multiplier.shape == (case["B"],)
    assert np.all(res.status == 1) and np.array_equal(res.active_mask, case["active"])
    against_reference(res, G, c, lb, ub, e, d, n)
    for p in range(case["B"]):
        tol = bc.x_tolerance(n, case["xstar"][p])
        err = np.max(np.abs(res.x[p] - case["xstar"][p]))
        assert err <= tol, (n, p, err, tol)
        note("gram x", err / tol)
        certificate(res, p, G, c[p], lb[p], ub[p], e, d[p], "gram n=%d p=%d" % (n, p))
        assert abs(res.multiplier[p] - case["lam"][p]) <= fc.lam_tolerance(G, n, case["xstar"][p], e), (n, p)
    # one-sided (the inactive side at infinity): the same solution, multipliers and decisions of the definition
    lo, hi = np.where(case["active"] < 0, lb, -np.inf), np.where(case["active"] > 0, ub, np.inf)
    one = bounded_lsq.bvls_gram_batch(G, c, (lo, hi), ctx=ctx, equality=(e, d))
    assert np.all(one.status == 1) and np.array_equal(one.active_mask, case["active"])
    against_reference(one, G, c, lo, hi, e, d, n)
    for p in range(case["B"]):
        assert np.max(np.abs(one.x[p] - case["xstar"][p])) <= bc.x_tolerance(n, case["xstar"][p]), (n, p)
        certificate(one, p, G, c[p], lo[p], hi[p], e, d[p], "gram one-sided n=%d p=%d" % (n, p))


def test_gram_solve_with_a_matrix_and_an_e_per_problem(ctx):
    case = fc.whole_case("29x17-own")
    G = np.einsum("bij,bik->bjk", case["A"], case["A"])
    c = np.einsum("bij,bi->bj", case["A"], case["b"])
    rng = np.random.default_rng(5)
    e = case["e"] * rng.uniform(0.5, 2.0, (case["B"], 1))            # the same constraint, scaled per problem
    d = np.einsum("bj,bj->b", e, case["xstar"])
    res = bounded_lsq.bvls_gram_batch(G, c, (case["lb"], case["ub"]), ctx=ctx, equality=(e, d))
    assert np.all(res.status == 1) and np.array_equal(res.active_mask, case["active"])
    against_reference(res, G, c, case["lb"], case["ub"], e, d, 17)
    for p in range(case["B"]):
        certificate(res, p, G[p], c[p], case["lb"][p], case["ub"][p], e[p], d[p], "own p=%d" % p)


def test_every_variable_on_a_bound_and_the_singleton_free_set(ctx):
    """The box [0, 0.5]^n with sum 1: the walk ends with every variable on a bound, the multiplier comes from the
    interval, and the first release frees ONE variable, which the equality pins.  At the midpoint of the interval its
    two ends violate by |e_j| (lo - hi) / 2 each, equal for e = 1, so WHICH end is released first is decided by rounding
    and the passes of the kernel and of the definition may differ: the minimiser is unique, so x, the status and the
    certificate are held, not the decisions."""
    for n in (3, 6, 65):
        case = fc.gram_case(n)
        G, c = case["G"], case["c"]
        lb, ub = np.zeros_like(c), np.full_like(c, 0.5)
        e, d = np.ones(n), np.ones(case["B"])
        res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, d))
        for p in range(case["B"]):
            r = bounded_lsq.bvls_reference(G, c[p], lb[p], ub[p], equality=(e, d[p]))
            assert res.status[p] == 1 and r["status"] == 1 and 1 <= res.nit[p] <= 5 * n, (n, p)
            tol = bc.x_tolerance(n, r["x"])
            err = np.max(np.abs(res.x[p] - r["x"]))
            assert err <= tol, (n, p, err, tol)
            note("x (vertex start)", err / tol)
            certificate(res, p, G, c[p], lb[p], ub[p], e, d[p], "vertex start n=%d p=%d" % (n, p))


# ---- the whole path -------------------------------------------------------------------------------------------------
def check_whole(res, case, name, sigma):
    """The margins of tests/test_bvls_gpu.py::_check_whole, with the reduced gradient in the optimality."""
    n, m, e = case["n"], case["m"], case["e"]
    w = None if sigma is None else 1.0 / np.broadcast_to(sigma, (case["B"], m))
    assert np.all(res.status == 1) and np.all(res.success), (name, res.status)
    assert np.array_equal(res.active_mask, case["active"]), name
    for p in range(case["B"]):
        A = lc.problem_matrix(case, p)
        x, on = res.x[p], res.active_mask[p]
        wv = np.ones(m) if w is None else w[p]
        tol = bc.x_tolerance(n, case["xstar"][p])
        err = np.max(np.abs(x - case["xstar"][p]))
        assert err <= tol, (name, p, err, tol)
        note("x", err / tol)
        Aw, bw = A * wv[:, None], case["b"][p] * wv
        certificate(res, p, Aw.T @ Aw, Aw.T @ bw, case["lb"][p], case["ub"][p], e, case["d"][p], "%s p=%d" % (name, p))
        ref, mag = lc.residual_reference(A, x[None, None, :], case["b"][p][None], None if w is None else wv)
        ef = np.abs(res.fun[p] - ref[0, 0]).astype(np.float64)
        bf = (lc.gamma(n + 1) * mag[0, 0]).astype(np.float64)
        assert np.all(ef <= bf), (name, p)
        note("fun", np.max(ef / np.maximum(bf, 1e-300)))
        cost = 0.5 * (res.fun[p] @ res.fun[p])
        assert res.cost[p] == cost and res[p].cost == cost, (name, p)
        assert abs(res.device_cost[p] - cost) <= 2.0 * lc.gamma(m) * cost, (name, p)
        lam = res.multiplier[p]
        bound = lc.gamma(m + n) * np.max(np.abs(A).T @ (wv * wv * (np.abs(A) @ np.abs(x) + np.abs(case["b"][p])))
                                         + abs(lam) * np.abs(e))
        print("%s p=%d: optimality %.3g (bound %.3g)" % (name, p, res.optimality[p], bound))
        assert 0.0 <= res.optimality[p] <= bound, (name, p, res.optimality[p], bound)
        note("optimality", res.optimality[p] / bound)
        assert abs(lam - case["lam"][p]) <= fc.lam_tolerance(Aw.T @ Aw, n, case["xstar"][p], e), (name, p)


@pytest.mark.parametrize("name", list(fc.WHOLE))
def test_whole_path_on_the_constructed_cases(ctx, name):
    case = fc.whole_case(name)
    kw = dict(bounds=(case["lb"], case["ub"]), ctx=ctx, equality=(case["e"], case["d"]))
    res = bounded_lsq.bvls_batch(case["A"], case["b"], sigma=case["sigma"], **kw)
    assert res.x.shape == (case["B"], case["n"]) and res.fun.shape == (case["B"], case["m"])
    check_whole(res, case, name, case["sigma"])
    one = res[0]
    assert one.status == 1 and one.success and one.multiplier == res.multiplier[0] and one.message
    if case["sigma"] is not None:                                     # sigma as (B, m): weights per problem
        per = np.tile(case["sigma"], (case["B"], 1))
        res2 = bounded_lsq.bvls_batch(case["A"], case["b"], sigma=per, **kw)
        check_whole(res2, case, name + " sigma (B, m)", per)
    single = bounded_lsq.bvls(lc.problem_matrix(case, 0), case["b"][0], (case["lb"][0], case["ub"][0]),
                              sigma=case["sigma"], ctx=ctx, equality=(case["e"], case["d"][0]))
    assert same_bits(np.asarray(single.x), res.x[0]) and single.multiplier == res.multiplier[0]


def test_fcls_on_the_simplex_case(ctx):
    """Unmixing with abundances that sum to one, A shared and per problem, with and without sigma."""
    s = fc.simplex_case()
    A, n, m = s["A"], s["n"], s["m"]
    rng = np.random.default_rng(3)
    b = np.stack([s["b"], s["b"] + 0.01 * rng.standard_normal(m), s["b"] + 0.01 * rng.standard_normal(m)])
    tol = bc.x_tolerance(n, s["xstar"], s["kappa"])
    for A_in in (A, np.tile(A, (3, 1, 1))):
        for sigma in (None, np.ones(m), np.ones((3, m))):
            res = bounded_lsq.fcls_batch(A_in, b, sigma=sigma, ctx=ctx)
            assert np.all(res.status == 1) and np.array_equal(res.active_mask[0], s["active"])
            assert np.max(np.abs(res.x[0] - s["xstar"])) <= tol
            assert abs(res.multiplier[0] - s["lam"]) <= fc.lam_tolerance(A.T @ A, n, s["xstar"], np.ones(n), s["kappa"])
            for p in range(3):
                assert np.all(res.x[p] >= 0.0) and same_bits(res.x[p][res.active_mask[p] < 0],
                                                              np.zeros(int(np.sum(res.active_mask[p] < 0))))
                certificate(res, p, A.T @ A, A.T @ b[p], np.zeros(n), np.full(n, np.inf), np.ones(n), 1.0,
                            "simplex p=%d" % p)
                r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b[p], 0.0, np.inf, equality=(1.0, 1.0))
                assert np.array_equal(res.active_mask[p], r["on_bound"]) and np.max(np.abs(res.x[p] - r["x"])) <= tol
    nn = bounded_lsq.nnls_batch(A, b, ctx=ctx, equality=(1.0, 1.0))
    for k in BYTES + ("fun",):
        assert same_bits(getattr(nn, k), getattr(bounded_lsq.fcls_batch(A, b, ctx=ctx), k)), k


def test_two_launches_in_the_model_eval_slot_with_an_equality(ctx):
    case = fc.whole_case("18x6-shared")
    ctx.timing(True)
    ctx.timing_reset()
    bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx, equality=(case["e"], case["d"]))
    ctx.sync()
    T = ctx.timing_read()
    ctx.timing(False)
    assert T["model_eval"][1] == 2, T["model_eval"]
    assert all(cnt == 0 for slot, (ms, cnt) in T.items() if slot != "model_eval"), T


# ---- conditioning ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", bc.CONDITIONING)
def test_the_projected_correction_takes_back_the_conditioning(ctx, draw):
    """kappa = 1e5, e = 1, d = e^T clip(x_ls): x with the finish is closer than the Gram-domain x (same moments) to the
    KKT solution on the final active set, solved in numpy.longdouble and refined against A.  Only the ordering is
    asserted; both distances are printed (DESIGN.md 7w records them)."""
    A, b, d = fc.conditioning_case(draw)
    n = A.shape[1]
    rc, G, c = moments(ctx, A, b[None])
    assert rc == 0
    kw = dict(ctx=ctx, equality=(1.0, d))
    gram = bounded_lsq.bvls_gram_batch(G, c, (-bc.BOX, bc.BOX), **kw)
    whole = bounded_lsq.bvls_batch(A, b, (-bc.BOX, bc.BOX), **kw)
    assert gram.status[0] == 1 and whole.status[0] == 1
    assert np.array_equal(gram.active_mask[0], whole.active_mask[0])
    x, lam = fc.kkt_from_matrix(A, b, np.full(n, -bc.BOX), np.full(n, bc.BOX), np.ones(n), d, whole.active_mask[0])
    x = x.astype(np.float64)
    e_gram, e_whole = np.max(np.abs(gram.x[0] - x)), np.max(np.abs(whole.x[0] - x))
    s_gram, s_whole = abs(gram.x[0].sum() - d), abs(whole.x[0].sum() - d)
    print("kappa %.0e seed %d: |x - x_kkt| Gram domain %.3g, after the correction %.3g; |sum - d| %.3g, %.3g"
          % (draw[0], draw[3], e_gram, e_whole, s_gram, s_whole))
    assert e_whole < e_gram
    assert s_whole <= fc.sum_bound(np.ones(n), whole.x[0])


# ---- independence ---------------------------------------------------------------------------------------------------
def test_a_result_does_not_depend_on_its_batch_mates(ctx):
    for n in (17, 100):
        case = fc.gram_case(n)
        G, c, lb, ub, e, d = case["G"], case["c"], case["lb"], case["ub"], case["e"], case["d"]
        batch = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, d))
        repl = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(np.tile(e, (case["B"], 1)), d))
        for k in BYTES:
            assert same_bits(getattr(batch, k), getattr(repl, k)), (n, k)     # a shared e and the same e replicated
        for p in range(case["B"]):
            alone = bounded_lsq.bvls_gram_batch(G, c[p:p + 1], (lb[p:p + 1], ub[p:p + 1]), ctx=ctx,
                                                equality=(e, d[p:p + 1]))
            for k in BYTES:
                assert same_bits(getattr(alone, k)[0], getattr(batch, k)[p]), (n, p, k)
    case = fc.whole_case("18x6-own-sigma")
    kw = dict(ctx=ctx, sigma=case["sigma"])
    batch = bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), equality=(case["e"], case["d"]), **kw)
    for p in range(case["B"]):
        alone = bounded_lsq.bvls_batch(case["A"][p:p + 1], case["b"][p:p + 1], (case["lb"][p:p + 1], case["ub"][p:p + 1]),
                                       equality=(case["e"], case["d"][p:p + 1]), **kw)
        for k in BYTES + ("fun",):
            assert same_bits(getattr(alone, k)[0], getattr(batch, k)[p]), (p, k)


# ---- failure handling -----------------------------------------------------------------------------------------------
def test_a_nan_or_an_infeasible_box_ends_one_problem_and_leaves_its_batch_mates_alone(ctx):
    case = fc.gram_case(17)
    G, c, lb, ub, e, d = case["G"], case["c"], case["lb"], case["ub"], case["e"], case["d"]
    clean = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, d))

    def others_untouched(res, get):
        for p in (0, 2):
            for k in BYTES:
                assert same_bits(get(res, k)[p], getattr(clean, k)[p]), (p, k)

    free = int(np.flatnonzero(case["active"][1] == 0)[0])             # a variable the iteration has to solve for
    bad = c.copy()
    bad[1, free] = np.nan
    res = bounded_lsq.bvls_gram_batch(G, bad, (lb, ub), ctx=ctx, equality=(e, d))
    assert res.status[1] == -1 and not res.success[1]
    assert np.all((res.x[1] >= lb[1]) & (res.x[1] <= ub[1]))
    others_untouched(res, getattr)
    r = bounded_lsq.bvls_reference(G, bad[1], lb[1], ub[1], equality=(e, d[1]))
    assert (r["status"], r["nit"], r["nfact"]) == (res.status[1], res.nit[1], res.nfact[1])
    # a NaN, and a zero, in one problem's e: the host refuses them, so through the entry itself
    names = dict(active_mask="on_bound")
    for poison in (np.nan, 0.0):
        e3 = np.tile(e, (3, 1))
        e3[1, 4] = poison
        rc, raw = raw_solve(ctx, "blsq_bvls_solve_eq_dev", G, c, lb, ub, e3, d)
        assert rc == 0 and raw["status"][1] == -1 and raw["nit"][1] == 0 and raw["nfact"][1] == 0
        assert same_bits(raw["x"][1], np.clip(np.zeros(17), lb[1], ub[1]))
        others_untouched(raw, lambda res, k: res[names.get(k, k)])
    # the sum out of the box's reach for one problem: -2 for it alone, x the clipped start
    reach = np.sum(np.where(e > 0, e * ub[1], e * lb[1]))
    far = d.copy()
    far[1] = reach + 1.0
    res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, far))
    assert res.status[1] == -2 and not res.success[1] and res.nit[1] == 0 and res.nfact[1] == 0
    assert same_bits(res.x[1], np.clip(np.zeros(17), lb[1], ub[1])) and "equality" in res[1].message
    others_untouched(res, getattr)
    whole = fc.whole_case("18x6-shared")
    far = whole["d"].copy()
    far[0] = -100.0
    res = bounded_lsq.bvls_batch(whole["A"], whole["b"], (whole["lb"], whole["ub"]), ctx=ctx, equality=(whole["e"], far))
    assert list(res.status) == [-2, 1, 1] and np.all(np.isfinite(res.fun)) and np.all(np.isfinite(res.cost))
    assert same_bits(res.x[0], np.clip(np.zeros(6), whole["lb"][0], whole["ub"][0]))


# ---- limits and arguments -------------------------------------------------------------------------------------------
def test_max_iter_zero_and_one(ctx):
    case = fc.gram_case(17)
    G, c, lb, ub, e, d = case["G"], case["c"], case["lb"], case["ub"], case["e"], case["d"]
    for max_iter in (0, 1):
        res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), max_iter=max_iter, ctx=ctx, equality=(e, d))
        against_reference(res, G, c, lb, ub, e, d, 17, max_iter=max_iter)
        assert np.all((res.status == 0) | (res.status == 1)) and np.all(res.nit <= max_iter)
        for p in range(case["B"]):
            assert np.all((res.x[p] >= lb[p]) & (res.x[p] <= ub[p]))
            assert abs(e @ res.x[p] - d[p]) <= fc.sum_bound(e, res.x[p])
    assert np.any(res.status == 0)                                  # (vetted on the CPU: a problem needs two passes)


def test_bad_arguments_return_their_position(ctx):
    B, m, n = 2, 5, 3
    with me.Dev(ctx) as dv:
        P = dv.up(np.ones(B * m * n + B * n * n))                     # one buffer large enough for every role
        I = dv.up(np.zeros(B * n + 3 * B, dtype=np.int32))
        lib, h = ctx.lib, ctx.h
        good = dict(B=B, m=m, n=n, G=P, G_stride=0, c=P, lb=P, ub=P, tol=1e-10, max_pass=5, A=P, A_stride=0, y=P,
                    w=None, w_stride=0, x=P, on_bound=I, fun=P, grad=P, optimality=P, stat=I, e=P, e_stride=0, d=P,
                    multiplier=P)

        def sol(**kw):
            a = dict(good, **kw)
            return lib.blsq_bvls_solve_eq_dev(h, *[a[k] for k in good])
        assert sol(B=0) == -2 and sol(m=0) == -3 and sol(m=-1, A=None, fun=None) == -3
        assert sol(n=0) == -4 and sol(n=129) == -4 and sol(G=None) == -5 and sol(G_stride=4) == -6
        assert sol(c=None) == -7 and sol(lb=None) == -8 and sol(ub=None) == -9 and sol(tol=float("nan")) == -10
        assert sol(max_pass=-1) == -11 and sol(A_stride=9) == -13 and sol(y=None) == -14
        assert sol(w=P, w_stride=2) == -16 and sol(x=None) == -17 and sol(on_bound=None) == -18
        assert sol(A=None) == -19 and sol(grad=None) == -20 and sol(optimality=None) == -21 and sol(stat=None) == -22
        assert sol(e=None) == -23 and sol(e_stride=2) == -24 and sol(e_stride=-3) == -24
        assert b"e_stride" in lib.blsq_last_error(h)
        assert sol(d=None) == -25 and sol(multiplier=None) == -26
        ctx.sync()


# ---- the unchanged path ---------------------------------------------------------------------------------------------
def test_without_an_equality_nothing_changes(ctx, monkeypatch):
    fields = ("x", "fun", "active_mask", "device_cost", "optimality", "nit", "nfact", "status")
    counts = me.count_entries(ctx, monkeypatch, ("blsq_bvls_solve_dev", "blsq_bvls_solve_eq_dev"))
    for name in ("40x6-shared", "130x17-own"):
        case = lc.get(name)
        plain = bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx)
        none = bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx, equality=None)
        assert plain.multiplier is None and none.multiplier is None
        for k in fields:
            assert same_bits(getattr(plain, k), getattr(none, k)), (name, k)
    assert counts == {"blsq_bvls_solve_dev": 4, "blsq_bvls_solve_eq_dev": 0}
    # blsq_bvls_solve_dev itself on one Gram case: the bytes bvls_gram_batch returns, with and without the keyword
    case = bc.gram_case(65)
    G, c, lb, ub = case["G"], case["c"], case["lb"], case["ub"]
    rc, raw = raw_solve(ctx, "blsq_bvls_solve_dev", G, c, lb, ub)
    assert rc == 0 and np.all(raw["status"] == 1) and np.array_equal(raw["on_bound"], case["active"])
    for res in (bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx),
                bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=None)):
        for k, r in (("x", "x"), ("active_mask", "on_bound"), ("optimality", "optimality"), ("nit", "nit"),
                     ("nfact", "nfact"), ("status", "status")):
            assert same_bits(getattr(res, k), raw[r]), k
    # an equality that binds nothing it would not hold anyway: the constrained solve at d = e^T x_plain reaches x_plain
    plain = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx)
    e = np.ones(65)
    tied = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx, equality=(e, plain.x @ e))
    assert np.all(tied.status == 1) and np.array_equal(tied.active_mask, plain.active_mask)
    for p in range(case["B"]):
        assert np.max(np.abs(tied.x[p] - plain.x[p])) <= bc.x_tolerance(65, plain.x[p])
        assert abs(tied.multiplier[p]) <= fc.kkt_bound(G, c[p], tied.x[p], e, 0.0)


def test_report_margins():
    """Not a check: prints the worst fraction of every margin the tests above used (run with -s to see it)."""
    for k in sorted(worst):
        print("margin %-28s worst fraction %.3g" % (k, worst[k]))
