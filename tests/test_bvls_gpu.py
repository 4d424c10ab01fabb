"""BVLS / NNLS on the GPU: the moments kernel against numpy.longdouble, the solve kernel on (G, c) alone
against ``bvls_reference`` decision for decision, the whole path against the constructed solutions, scipy's BVLS and
NNLS, and the argument checks of the two entries.  The cases are those tests/test_bvls_cpu.py vets without a GPU.

Margins (gamma_k = k eps / (1 - k eps), tests/_linear_cases.py):
  moments   |G - G_ref| <= gamma_{m+2} |A|^T W^2 |A|,  |c - c_ref| <= gamma_{m+2} |A|^T W^2 |y|: each term is two
            roundings for the weights and one fused multiply-add; references in numpy.longdouble.
  x         |x - x*|_inf <= 8 n eps kappa(A) max(1, |x*|_inf), kappa = 30 by construction; the numpy definition is held
            to 1 / 8 of it without a GPU.
  fun       gamma_{n+1} w (|A||x| + |b|), the bound of ``residual_reference``.
  cost      with `fun`: equal to 0.5 * fun @ fun.  With fun=False the cost is the kernel's sum of the same squares in its
            own order: both are sums of m non-negative terms, each within gamma_m of the exact sum, so they are within
            2 gamma_m cost of each other.
  KKT       on the narrow-box draws the optimality of a status-1 result stays under ``kkt_bound`` (tests/_bvls_cases.py).
  optimality  below gamma_{m+n} max_j (|A|^T W (|A||x| + |b|))_j: the rounding of the gradient itself.
The worst fraction of each margin seen on an MI355X is in DESIGN.md 7t.
"""
import numpy as np
import pytest
from scipy import optimize

import bounded_lsq
from bounded_lsq import _bvls

import _bvls_cases as bc
import _linear_cases as lc
import _model_eval as me
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

ENTRIES = ("blsq_bvls_moments_dev", "blsq_bvls_solve_dev")
worst = {}                                                     # margin name -> worst fraction seen (printed at the end)


def note(name, frac):
    worst[name] = max(worst.get(name, 0.0), float(frac))


def w_stride(w, m):
    return m if (w is not None and np.ndim(w) == 2) else 0


def moments(ctx, A, y, w=None, G_stride=None):
    """blsq_bvls_moments_dev on host arrays -> (rc, G (n, n) or (B, n, n), c (B, n))."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, n = A.shape[-2:]
    B = y.shape[0]
    per = A.ndim == 3 or w_stride(w, m) != 0
    if G_stride is None:
        G_stride = n * n if per else 0
    with me.Dev(ctx) as d:
        dG = d.up(np.full((B, n, n) if G_stride else (n, n), np.nan))
        dc = d.up(np.full((B, n), np.nan))
        rc = ctx.lib.blsq_bvls_moments_dev(ctx.h, B, m, n, d.up(A), m * n if A.ndim == 3 else 0, d.up(y), d.up(w),
                                           w_stride(w, m), dG, G_stride, dc)
        if rc != 0:
            return rc, None, None
        return 0, ctx.to_host(dG, (B, n, n) if G_stride else (n, n), np.float64), ctx.to_host(dc, (B, n), np.float64)


# ---- moments --------------------------------------------------------------------------------------------------------
MOM_MS = (1, 3, 4, 5, 63, 64, 65, 130)
MOM_NS = (1, 2, 15, 16, 17, 33, 128)
MOM_BS = (1, 3, 17, 33)


@pytest.mark.parametrize("m", MOM_MS)
def test_moments_against_extended_precision(ctx, m):
    """Every n and B, shared and per-problem A, the three forms of w: the MFMA tile of 16, the K-step of 4 and the row
    block of 16 straddled.  The references are computed once for 33 problems; a smaller batch is their first B."""
    g = lc.gamma(m + 2)
    for n in MOM_NS:
        rng = np.random.default_rng(100 * m + n)
        Bmax = max(MOM_BS)
        A_own, y = rng.standard_normal((Bmax, m, n)), rng.standard_normal((Bmax, m))
        ws = {"none": None, "m": rng.uniform(0.5, 2.0, m), "per": rng.uniform(0.5, 2.0, (Bmax, m))}
        for shared in (True, False):
            A = A_own[0] if shared else A_own
            for wname, w in ws.items():
                Gr, Gm, cr, cm = bc.moments_reference(A, y, w)
                per = Gr.ndim == 3
                for B in MOM_BS:
                    what = (m, n, B, shared, wname)
                    rc, G, c = moments(ctx, A if shared else A[:B], y[:B], w if wname != "per" else w[:B])
                    assert rc == 0, what
                    assert G.shape == ((B, n, n) if per else (n, n)), what
                    eG = np.abs(G - (Gr[:B] if per else Gr)).astype(np.float64)
                    bG = (g * (Gm[:B] if per else Gm)).astype(np.float64)
                    ec = np.abs(c - cr[:B]).astype(np.float64)
                    bnd_c = (g * cm[:B]).astype(np.float64)
                    assert np.all(eG <= bG), what
                    assert np.all(ec <= bnd_c), what
                    note("moments G", np.max(eG / bG))
                    note("moments c", np.max(ec / bnd_c))
                    assert same_bits(G, np.swapaxes(G, -1, -2)), what          # symmetric in every bit


@pytest.mark.parametrize("shared", [True, False])
def test_a_problem_s_c_does_not_depend_on_its_batch_mates(ctx, shared):
    """c of a problem alone equals its c inside a batch in every bit: in the first row of the first tile, in the first
    row of the second, and in the last, incomplete one."""
    rng = np.random.default_rng(17)
    for (m, n) in ((5, 2), (65, 17), (130, 33)):
        B = 33
        A, y, w = rng.standard_normal((B, m, n)), rng.standard_normal((B, m)), rng.uniform(0.5, 2.0, m)
        rc, G, c = moments(ctx, A[0] if shared else A, y, w)
        assert rc == 0
        for p in (0, 5, 16, 32):
            rc, G1, c1 = moments(ctx, A[0] if shared else A[p:p + 1], y[p:p + 1], w)
            assert rc == 0 and same_bits(c1[0], c[p]), (m, n, p)
            assert same_bits(G1 if shared else G1[0], G if shared else G[p]), (m, n, p)


# ---- the solve on (G, c) alone --------------------------------------------------------------------------------------
def _against_reference(res, G, c, lb, ub, n, xstar=None, **kw):
    lb, ub = np.broadcast_to(lb, c.shape), np.broadcast_to(ub, c.shape)
    for p in range(c.shape[0]):
        Gp = G if G.ndim == 2 else G[p]
        r = bounded_lsq.bvls_reference(Gp, c[p], lb[p], ub[p], **kw)
        assert np.array_equal(res.active_mask[p], r["on_bound"]), (n, p)
        assert (res.status[p], res.nit[p], res.nfact[p]) == (r["status"], r["nit"], r["nfact"]), (n, p)
        ref = r["x"] if xstar is None else xstar[p]
        tol = bc.x_tolerance(n, ref)
        err = np.max(np.abs(res.x[p] - r["x"]))
        assert err <= tol, (n, p, err, tol)
        note("gram x", err / tol)
        on = res.active_mask[p]
        assert same_bits(res.x[p][on < 0], lb[p][on < 0]) and same_bits(res.x[p][on > 0], ub[p][on > 0]), (n, p)
        assert np.all((res.x[p] >= lb[p]) & (res.x[p] <= ub[p]))


@pytest.mark.parametrize("n", bc.GRAM_NS)
def test_gram_solve_against_the_definition(ctx, n):
    """on_bound, status, passes and factorisations equal those of ``bvls_reference`` on the constructed cases
    (multipliers >= 1: no decision is near a tie); x within the tolerance; bounds held bit for bit.  With the box as
    constructed, one-sided (the inactive side at infinity), wide open but finite, and all-infinite (against solve)."""
    case = bc.gram_case(n)
    G, c, lb, ub, act = case["G"], case["c"], case["lb"], case["ub"], case["active"]
    res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx)
    assert res.fun is None and res.cost is None
    assert np.all(res.status == 1) and np.array_equal(res.active_mask, act)
    _against_reference(res, G, c, lb, ub, n)
    for p in range(case["B"]):
        assert np.max(np.abs(res.x[p] - case["xstar"][p])) <= bc.x_tolerance(n, case["xstar"][p])
    # one-sided: the solution and its multipliers are the same
    lo, hi = np.where(act < 0, lb, -np.inf), np.where(act > 0, ub, np.inf)
    one = bounded_lsq.bvls_gram_batch(G, c, (lo, hi), ctx=ctx)
    assert np.all(one.status == 1) and np.array_equal(one.active_mask, act)
    _against_reference(one, G, c, lo, hi, n)
    # wide open, finite and infinite: the unconstrained solution
    x_free = np.linalg.solve(G, c.T).T
    for box in ((-1e3, 1e3), (-np.inf, np.inf)):
        free = bounded_lsq.bvls_gram_batch(G, c, box, ctx=ctx)
        assert np.all(free.status == 1) and not free.active_mask.any() and np.all(free.nit == 0)
        assert np.all(free.nfact == 1)
        for p in range(case["B"]):
            tol = bc.x_tolerance(n, x_free[p])
            assert np.max(np.abs(free.x[p] - x_free[p])) <= tol, (n, p)
            note("gram x (free)", np.max(np.abs(free.x[p] - x_free[p])) / tol)


def test_gram_solve_with_a_matrix_per_problem(ctx):
    case = lc.get("130x17-own")
    G = np.einsum("bij,bik->bjk", case["A"], case["A"])
    c = np.einsum("bij,bi->bj", case["A"], case["b"])
    res = bounded_lsq.bvls_gram_batch(G, c, (case["lb"], case["ub"]), ctx=ctx)
    assert np.all(res.status == 1) and np.array_equal(res.active_mask, case["active"])
    _against_reference(res, G, c, case["lb"], case["ub"], 17)


def test_max_iter_one_is_status_zero_and_feasible(ctx):
    kappa, m, n, seed = 30.0, 130, 17, bc.SWEEP_SEED + 7             # (vetted on the CPU: needs two passes or more)
    A, b = bc.draw(m, n, kappa, seed)
    G, c = A.T @ A, (A.T @ b)[None]
    res = bounded_lsq.bvls_gram_batch(G, c, (-bc.BOX, bc.BOX), max_iter=1, ctx=ctx)
    assert res.status[0] == 0 and res.nit[0] == 1 and not res.success[0]
    assert np.all(np.abs(res.x[0]) <= bc.BOX)
    r = bounded_lsq.bvls_reference(G, c[0], -bc.BOX, bc.BOX, max_iter=1)
    assert np.array_equal(res.active_mask[0], r["on_bound"]) and res.nfact[0] == r["nfact"]
    full = bounded_lsq.bvls_gram_batch(G, c, (-bc.BOX, bc.BOX), ctx=ctx)
    assert full.status[0] == 1 and full.nit[0] >= 2


def test_a_nan_ends_one_problem_and_leaves_its_batch_mates_alone(ctx):
    """Guaranteed to end by the loop bounds: the first solve of the poisoned problem returns a value that is not finite
    and the problem stops with status -1 after that one factorisation."""
    case = bc.gram_case(17)
    G, c, lb, ub = case["G"], case["c"], case["lb"], case["ub"]
    clean = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx)
    bad = c.copy()
    bad[1, 3] = np.nan
    res = bounded_lsq.bvls_gram_batch(G, bad, (lb, ub), ctx=ctx)
    assert res.status[1] == -1 and res.nit[1] == 0 and res.nfact[1] == 1 and not res.success[1]
    assert np.all((res.x[1] >= lb[1]) & (res.x[1] <= ub[1]))
    for p in (0, 2):
        for k in ("x", "active_mask", "optimality", "nit", "nfact", "status"):
            assert same_bits(getattr(res, k)[p], getattr(clean, k)[p]), (p, k)


def test_a_singular_gram_matrix_is_status_minus_one(ctx):
    G, c, lb, ub = bc.singular_case()
    res = bounded_lsq.bvls_gram_batch(G, c, (lb, ub), ctx=ctx)
    assert np.all(res.status == -1) and np.all(res.nit == 0) and np.all(res.nfact == 1)
    assert np.all((res.x >= lb) & (res.x <= ub))


# ---- narrow boxes: a released variable crosses to its opposite bound -------------------------------------------------
def _narrow_groups(key):
    groups = {}
    for seed in bc.NARROW_SEEDS:
        A, b, box, s = bc.narrow_with_scipy(seed)
        groups.setdefault(key(A), []).append((seed, A, b, box, s))
    return groups


def test_narrow_boxes_on_the_gram_solve(ctx):
    """The thousand draws of the CPU test, one launch per n with a G per problem: status 1 on every draw, the optimality
    from g = G x - c under its bound, the decisions of the definition, and scipy's mask (or a cost not above scipy's)."""
    for n, grp in sorted(_narrow_groups(lambda A: A.shape[1]).items()):
        G = np.stack([A.T @ A for _, A, _, _, _ in grp])
        c = np.stack([A.T @ b for _, A, b, _, _ in grp])
        box = np.array([g[3] for g in grp])[:, None] * np.ones((1, n))
        res = bounded_lsq.bvls_gram_batch(G, c, (-box, box), ctx=ctx)
        for p, (seed, A, b, _, s) in enumerate(grp):
            assert res.status[p] == 1, seed
            g = G[p] @ res.x[p] - c[p]
            opt, bound = bc.kkt_optimality(g, res.active_mask[p]), bc.kkt_bound(G[p], c[p], res.x[p])
            assert opt <= bound and res.optimality[p] <= bound, (seed, opt, res.optimality[p], bound)
            note("KKT (narrow, gram)", max(opt, res.optimality[p]) / bound)
            assert bc.agrees_with_scipy(A, b, res.x[p], res.active_mask[p], s), seed
            r = bounded_lsq.bvls_reference(G[p], c[p], -box[p], box[p])
            assert np.array_equal(res.active_mask[p], r["on_bound"]), seed
            assert (res.nit[p], res.nfact[p]) == (r["nit"], r["nfact"]), seed


def test_narrow_boxes_on_the_whole_path(ctx):
    """The same draws through bvls_batch, one call per shape: status 1, scipy's mask or a lower cost, and the optimality
    from the true gradient under the same bound."""
    for (m, n), grp in sorted(_narrow_groups(lambda A: A.shape).items()):
        A3 = np.stack([g[1] for g in grp])
        b = np.stack([g[2] for g in grp])
        box = np.array([g[3] for g in grp])[:, None] * np.ones((1, n))
        res = bounded_lsq.bvls_batch(A3, b, (-box, box), ctx=ctx)
        for p, (seed, A, bp, _, s) in enumerate(grp):
            assert res.status[p] == 1 and res.success[p], seed
            assert bc.agrees_with_scipy(A, bp, res.x[p], res.active_mask[p], s), seed
            bound = bc.kkt_bound(A.T @ A, A.T @ bp, res.x[p])
            assert res.optimality[p] <= bound, (seed, res.optimality[p], bound)
            note("KKT (narrow, whole path)", res.optimality[p] / bound)


# ---- the whole path -------------------------------------------------------------------------------------------------
def _check_whole(res, case, name):
    n, m = case["n"], case["m"]
    sg = case["sigma"]
    w = None if sg is None else 1.0 / sg
    assert np.all(res.status == 1) and np.all(res.success), name
    assert np.array_equal(res.active_mask, case["active"]), name
    for p in range(case["B"]):
        A = lc.problem_matrix(case, p)
        x, on = res.x[p], res.active_mask[p]
        assert same_bits(x[on < 0], case["lb"][p][on < 0]) and same_bits(x[on > 0], case["ub"][p][on > 0]), (name, p)
        tol = bc.x_tolerance(n, case["xstar"][p])
        err = np.max(np.abs(x - case["xstar"][p]))
        assert err <= tol, (name, p, err, tol)
        note("x", err / tol)
        ref, mag = lc.residual_reference(A, x[None, None, :], case["b"][p][None], w)
        ef = np.abs(res.fun[p] - ref[0, 0]).astype(np.float64)
        bf = (lc.gamma(n + 1) * mag[0, 0]).astype(np.float64)
        assert np.all(ef <= bf), (name, p)
        note("fun", np.max(ef / np.maximum(bf, 1e-300)))
        cost = 0.5 * (res.fun[p] @ res.fun[p])
        assert res.cost[p] == cost and res[p].cost == cost, (name, p)
        assert abs(res.device_cost[p] - cost) <= 2.0 * lc.gamma(m) * cost, (name, p)
        note("cost (fun=False)", abs(res.device_cost[p] - cost) / (2.0 * lc.gamma(m) * cost))
        wv = np.ones(m) if w is None else w
        bound = lc.gamma(m + n) * np.max(np.abs(A).T @ (wv * wv * (np.abs(A) @ np.abs(x) + np.abs(case["b"][p]))))
        assert 0.0 <= res.optimality[p] <= bound, (name, p, res.optimality[p], bound)
        note("optimality", res.optimality[p] / bound)


@pytest.mark.parametrize("name", list(lc.FIT_CASES) + ["weighted"])
def test_whole_path_on_the_constructed_cases(ctx, name):
    case = bc.weighted_case() if name == "weighted" else lc.get(name)
    res = bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), sigma=case["sigma"], ctx=ctx)
    assert res.x.shape == (case["B"], case["n"]) and res.fun.shape == (case["B"], case["m"])
    _check_whole(res, case, name)
    assert np.all(res.nit <= 1.5 * case["n"])
    one = res[0]
    assert one.status == 1 and one.success and np.array_equal(one.x, res.x[0]) and one.message


@pytest.mark.parametrize("name", ["40x6-shared", "130x17-shared", "300x100-shared"])
def test_shared_against_replicated(ctx, name):
    case = lc.get(name)
    kw = dict(bounds=(case["lb"], case["ub"]), ctx=ctx)
    shared = bounded_lsq.bvls_batch(case["A"], case["b"], **kw)
    repl = bounded_lsq.bvls_batch(np.tile(case["A"], (case["B"], 1, 1)), case["b"], **kw)
    assert np.array_equal(shared.active_mask, repl.active_mask) and np.array_equal(shared.status, repl.status)
    for p in range(case["B"]):
        tol = bc.x_tolerance(case["n"], case["xstar"][p])
        assert np.max(np.abs(shared.x[p] - repl.x[p])) <= tol
        note("x (shared vs replicated)", np.max(np.abs(shared.x[p] - repl.x[p])) / tol)


def test_bvls_is_the_first_row_of_its_batch(ctx):
    case = lc.get("130x17-shared")
    batch = bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx)
    one = bounded_lsq.bvls(case["A"], case["b"][0], (case["lb"][0], case["ub"][0]), ctx=ctx)
    for k in ("x", "fun", "active_mask", "cost", "optimality", "nit", "nfact", "status"):
        assert same_bits(np.asarray(getattr(one, k)), np.asarray(getattr(batch, k)[0])), k
    assert one.success and one.message


def test_nnls_against_scipy(ctx):
    c = lc.nnls_case()
    rng = np.random.default_rng(3)
    b = np.stack([c["b"], c["b"] + 0.01 * rng.standard_normal(c["m"]), -c["b"]])     # the last: x = 0
    res = bounded_lsq.nnls_batch(c["A"], b, ctx=ctx)
    assert np.all(res.status == 1)
    tol = bc.x_tolerance(c["n"], c["xstar"])
    assert np.array_equal(res.active_mask[0], [0, 0, 0, -1, -1]) and np.max(np.abs(res.x[0] - c["xstar"])) <= tol
    for p in range(3):
        xs = optimize.nnls(c["A"], b[p])[0]
        assert np.array_equal(res.x[p] == 0.0, xs == 0.0) and np.array_equal(res.active_mask[p] != 0, xs == 0.0)
        assert np.max(np.abs(res.x[p] - xs)) <= tol, p
        note("x (nnls)", np.max(np.abs(res.x[p] - xs)) / tol)
    assert same_bits(res.x[2], np.zeros(c["n"]))


def test_fun_false_returns_none(ctx):
    case = lc.get("40x6-shared")
    kw = dict(bounds=(case["lb"], case["ub"]), ctx=ctx)
    with_fun = bounded_lsq.bvls_batch(case["A"], case["b"], **kw)
    without = bounded_lsq.bvls_batch(case["A"], case["b"], fun=False, **kw)
    assert without.fun is None and without[0].fun is None
    for k in ("x", "device_cost", "optimality", "active_mask", "nit", "nfact", "status"):
        assert same_bits(getattr(without, k), getattr(with_fun, k)), k
    assert same_bits(without.cost, without.device_cost) and without[1].cost == without.device_cost[1]
    assert np.all(np.abs(without.cost - with_fun.cost) <= 2.0 * lc.gamma(case["m"]) * with_fun.cost)


# ---- launches and routes --------------------------------------------------------------------------------------------
def test_two_launches_in_the_model_eval_slot_and_nothing_else(ctx):
    case = lc.get("40x6-shared")
    ctx.timing(True)
    ctx.timing_reset()
    bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx)
    ctx.sync()
    T = ctx.timing_read()
    ctx.timing(False)
    assert T["model_eval"][1] == 2, T["model_eval"]
    assert all(cnt == 0 for slot, (ms, cnt) in T.items() if slot != "model_eval"), T


def test_the_entries_each_route_reaches(ctx, monkeypatch):
    case = lc.get("40x6-shared")
    counts = me.count_entries(ctx, monkeypatch, ENTRIES + ("blsq_linear_eval_dev",))
    bounded_lsq.lsq_linear_batch(case["A"], case["b"], bounds=(case["lb"], case["ub"]), x0=case["x0"], ctx=ctx)
    assert counts["blsq_bvls_moments_dev"] == 0 and counts["blsq_bvls_solve_dev"] == 0
    assert counts["blsq_linear_eval_dev"] > 0
    counts["blsq_linear_eval_dev"] = 0
    bounded_lsq.bvls_batch(case["A"], case["b"], (case["lb"], case["ub"]), ctx=ctx)
    assert counts == {"blsq_bvls_moments_dev": 1, "blsq_bvls_solve_dev": 1, "blsq_linear_eval_dev": 0}
    bounded_lsq.bvls_gram_batch(case["A"].T @ case["A"], case["b"] @ case["A"], (case["lb"], case["ub"]), ctx=ctx)
    assert counts == {"blsq_bvls_moments_dev": 1, "blsq_bvls_solve_dev": 2, "blsq_linear_eval_dev": 0}


# ---- conditioning ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", bc.CONDITIONING)
def test_the_correction_against_A_takes_back_the_conditioning(ctx, draw):
    """kappa = 1e5: x with the finish is closer to scipy's BVLS than the Gram-domain x on the same moments; equal
    masks.  Only the ordering is asserted; both errors are printed (DESIGN.md 7t records them)."""
    kappa, m, n, seed = draw
    A, b = bc.draw(m, n, kappa, seed)
    s = optimize.lsq_linear(A, b, (-bc.BOX, bc.BOX), method="bvls", tol=1e-14)
    rc, G, c = moments(ctx, A, b[None])
    assert rc == 0
    gram = bounded_lsq.bvls_gram_batch(G, c, (-bc.BOX, bc.BOX), ctx=ctx)
    whole = bounded_lsq.bvls_batch(A, b, (-bc.BOX, bc.BOX), ctx=ctx)
    assert gram.status[0] == 1 and whole.status[0] == 1
    assert np.array_equal(gram.active_mask[0], s.active_mask) and np.array_equal(whole.active_mask[0], s.active_mask)
    e_gram, e_whole = np.max(np.abs(gram.x[0] - s.x)), np.max(np.abs(whole.x[0] - s.x))
    print("kappa %.0e seed %d: |x - x_scipy| Gram domain %.3g, after the correction %.3g" % (kappa, seed, e_gram, e_whole))
    assert e_whole < e_gram


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_position(ctx):
    B, m, n = 2, 5, 3
    with me.Dev(ctx) as d:
        P = d.up(np.ones(B * m * n + B * n * n))                      # one buffer large enough for every role
        I = d.up(np.zeros(B * n + 3 * B, dtype=np.int32))
        lib, h = ctx.lib, ctx.h
        good = dict(B=B, m=m, n=n, A=P, A_stride=0, y=P, w=None, w_stride=0, G=P, G_stride=0, c=P)

        def mom(**kw):
            a = dict(good, **kw)
            return lib.blsq_bvls_moments_dev(h, *[a[k] for k in good])
        assert mom(B=0) == -2 and mom(m=0) == -3 and mom(n=0) == -4 and mom(n=129) == -4
        assert mom(A=None) == -5 and mom(A_stride=7) == -6 and mom(y=None) == -7 and mom(w=P, w_stride=3) == -9
        assert mom(G=None) == -10 and mom(G_stride=5) == -11 and mom(A_stride=m * n) == -11
        assert mom(c=None) == -12 and mom(w=P, w_stride=m) == -11
        assert b"G_stride" in lib.blsq_last_error(h)
        sgood = dict(B=B, m=m, n=n, G=P, G_stride=0, c=P, lb=P, ub=P, tol=1e-10, max_pass=5, A=P, A_stride=0, y=P,
                     w=None, w_stride=0, x=P, on_bound=I, fun=P, grad=P, optimality=P, stat=I)

        def sol(**kw):
            a = dict(sgood, **kw)
            return lib.blsq_bvls_solve_dev(h, *[a[k] for k in sgood])
        assert sol(B=0) == -2 and sol(m=0) == -3 and sol(m=-1, A=None, fun=None) == -3
        assert sol(n=0) == -4 and sol(n=129) == -4 and sol(G=None) == -5 and sol(G_stride=4) == -6
        assert sol(c=None) == -7 and sol(lb=None) == -8 and sol(ub=None) == -9 and sol(tol=float("nan")) == -10
        assert sol(max_pass=-1) == -11 and sol(A_stride=9) == -13 and sol(y=None) == -14
        assert sol(w=P, w_stride=2) == -16 and sol(x=None) == -17 and sol(on_bound=None) == -18
        assert sol(A=None) == -19 and sol(grad=None) == -20 and sol(optimality=None) == -21 and sol(stat=None) == -22
        ctx.sync()


def test_report_margins():
    """Not a check: prints the worst fraction of every margin the tests above used (run with -s to see it)."""
    for k in sorted(worst):
        print("margin %-28s worst fraction %.3g" % (k, worst[k]))
