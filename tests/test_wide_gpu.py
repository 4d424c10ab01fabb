"""Parity at the widths past the normal-equations front end: n = 272 ... 512 (TRF and dogbox) and n = 513 ... 1023
(dogbox, m <= 1024).  There gram_supported is false, and with it the certificate, the CSNE tier and CholeskyQR2: every
problem goes through the Householder tree (merge groups of 3 and 2 triangles), the stacked-QR staging up to its
1024-row limit, the jacobi_rows_kernel<34> / <68> instantiations (row blocks of 16 and 8 streamed through LDS) and the
n >= 128 variants of the step kernels.

Every case goes through the C-ABI against oracle.blsq_oracle, on the project's own bars: step, x_new, p_h_tr within
1e-10 relative; hits / active_new / on_bound_new / active_set bit-exact; n_iter, branch, tr_hit, fallback equal; alpha
to 1e-9, predicted_reduction to 1e-10; x_new inside the box (strictly for TRF; dogbox leaves variables ON a bound by
design, dogbox.py:38-75); g and g_norm within 1e-12 of J.T @ f accumulated in np.longdouble.  Each case runs on the
SVD-free route and with the Jacobi SVD forced; on the forced route debug_fast() == 0, the sweep count is positive and
below the cap of 40, and (TRF: the dogbox plan keeps no singular values to fetch) the singular values match the
reference's to 1e-12.  No case is skipped, excused or pinned by name.

The case lists were fixed after running every problem of this file through the oracle and `oracle_sensitivity` on the
CPU (tests/test_fuzz_gpu.py; three sign patterns per problem, masks stable throughout).  Largest movement of the oracle's
own step under one-ulp changes of J: 1.8e-14 (TRF width sweep), 6.6e-15 (dogbox width sweep), 1.3e-13 / 5.2e-14
(columns scaled by 10^+-3), 4.5e-15 (rank-deficient batches), 8.5e-14 at kappa = 1e3 and 5.1e-12 (TRF) / 6.2e-12
(dogbox) at kappa = 1e5 -- the largest found, 16 times under the bar.  Two cases were replaced by a neighbour (WIDE_ROWS
below: p_h_tr beside a pole) and one was changed (the zero-column TRF problem keeps its box: rankdef_cases).
"""
import numpy as np
import pytest

from oracle import blsq_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAX_SWEEPS = 40                                                # ja.max_sweeps of both plans
WIDTHS = (272, 273, 288, 320, 336, 337, 400, 496, 497, 511, 512)
DOG_ONLY_WIDTHS = (513, 700, 1008, 1023)                       # single leaf: m <= 1024


# TRF rows of the wide (m < n) case of a width, where not n - 40.  A bounded m < n problem whose Gauss-Newton step
# lies inside Delta sends the reference's Newton iteration to NEGATIVE alpha (full_rank is forced False,
# trust_region.py:108-112), ten iterations, and p_h_tr = -V (s uf / (s^2 + alpha)) then sits beside a pole: at
# 360 x 400 and 472 x 512 the oracle's own p_h_tr moves by 1.4e-11 and 3.2e-11 under one-ulp changes of J (its step,
# the gradient step there, by 4e-16).  Their neighbours two rows down move by 5e-13.
WIDE_ROWS = {400: 358, 512: 470}


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    den = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (den if den > 0 else 1.0)


# ---- the cases (plain functions: the CPU sensitivity check imports them) -----------------------------------------
def trf_sweep_cases():
    """-> [(tag, P, Delta)]: every width against one leaf (wide, square), two leaves, ragged leaves, four or more
    leaves; one deep tree (several merge levels at three triangles per workgroup)."""
    from bounded_lsq import _synth
    shapes = [(m, n) for n in WIDTHS for m in (WIDE_ROWS.get(n, n - 40), n, 1024, 1025, 2049, 4096)] + [(20000, 320)]
    for i, (m, n) in enumerate(shapes):
        B = 2 + (m + n) % 2
        Delta = np.array([(10.0, 0.5, 0.05)[(i + b) % 3] for b in range(B)])
        yield "trf_%dx%d" % (m, n), (lambda i=i, B=B, m=m, n=n: _synth.trf_batch(9000 + 4 * i, B, m, n)), Delta


def dogbox_sweep_cases():
    from bounded_lsq import _synth
    shapes = [(m, n) for n in WIDTHS for m in (n - 40, n, 1024, 1025, 2049, 4096)]
    shapes += [(m, n) for n in DOG_ONLY_WIDTHS for m in (n - 30, n, 1024)]
    for i, (m, n) in enumerate(shapes):
        B = 2 + (m + n) % 2
        Delta = np.array([(5e-3, 5e-4, 2e-2)[(i + b) % 3] for b in range(B)])
        yield "dog_%dx%d" % (m, n), (lambda i=i, B=B, m=m, n=n: _synth.dogbox_batch(12000 + 4 * i, B, m, n)), Delta


def _unbounded(P):
    P["lb"][:] = -np.inf
    P["ub"][:] = np.inf
    return P


def _batch(kind, seed, B, m, n, unbounded=False):
    from bounded_lsq import _synth
    if kind == "trf":
        return _synth.trf_batch(seed, B, m, n, unbounded=unbounded)
    P = _synth.dogbox_batch(seed, B, m, n, frac_on_bound=0.0 if unbounded else 0.10)
    return _unbounded(P) if unbounded else P


def spectrum_cases(kind):
    """Prescribed log-spaced spectra (the construction of test_fuzz_gpu.draw_case), unbounded, kappa 1e3 and 1e5,
    one problem per Delta of (0.3, 30, 1e9): Newton rounds active / the plain Gauss-Newton step."""
    for (m, n) in ((2000, 400), (1024, 512)):
        for lk in (3, 5):
            def make(m=m, n=n, lk=lk):
                P = _batch(kind, 31000 + n + lk, 3, m, n, unbounded=True)
                rng = np.random.default_rng(7 * n + lk)
                for b in range(3):
                    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
                    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
                    P["J"][b] = (U * np.logspace(0, -lk, n)) @ V.T * np.sqrt(m)
                return P
            yield "%s_spec_%dx%d_k1e%d" % (kind, m, n, lk), make, np.array([0.3, 30.0, 1e9])


RANKDEF_FAST = [1, 0, 1, 0, 0]                                 # full rank, duplicated, full rank, zero, dependent


def rankdef_cases(kind):
    """A batch mixing full-rank problems with a duplicated, a zero and a dependent column (unbounded, but see below): both
    trust-region routes in one launch.  The rank-deficient TRF problems get a Delta inside their min-norm step (beyond
    it the reference's answer is LAPACK null-space noise: KNIFE_EDGE of tests/test_hip_parity.py)."""
    for (m, n) in ((1500, 400), (1100, 512)):
        def make(m=m, n=n):
            P = _batch(kind, 41000 + n, 5, m, n, unbounded=True)
            P["J"][1, :, n - 7] = P["J"][1, :, 3]
            P["J"][3, :, n // 2] = 0.0
            P["J"][4, :, n - 1] = P["J"][4, :, 0] + P["J"][4, :, n // 3]
            if kind == "trf":
                # the zero-column problem keeps its box: unbounded, hits = sign(p) for EVERY variable, and the
                # reference's own sign of p at the zero column flips when that column moves by one ulp
                Pb = _batch(kind, 41000 + n, 5, m, n)
                P["lb"][3], P["ub"][3] = Pb["lb"][3], Pb["ub"][3]
            return P
        if kind == "trf":
            P = make()
            Delta = np.array([0.3 * np.linalg.norm(np.linalg.lstsq(P["J"][b], -P["f"][b], rcond=None)[0])
                              for b in range(5)])
            Delta[2] = 10.0 * Delta[2] / 0.3                   # a full-rank problem on the plain Gauss-Newton step
        else:
            Delta = np.array([0.02, 0.02, 5.0, 0.02, 5.0])
        yield "%s_rankdef_%dx%d" % (kind, m, n), make, Delta


def colscale_cases(kind):
    for (m, n) in ((2000, 400), (1300, 512)):
        def make(m=m, n=n):
            P = _batch(kind, 51000 + n, 3, m, n)
            rng = np.random.default_rng(n)
            P["J"] = P["J"] * 10.0 ** rng.uniform(-3, 3, size=(3, 1, n))
            return P
        yield ("%s_colscale_%dx%d" % (kind, m, n), make,
               np.array([10.0, 0.5, 0.05]) if kind == "trf" else np.array([5e-3, 5e-4, 2e-2]))


def hard_cases(kind):
    for gen in (spectrum_cases, rankdef_cases, colscale_cases):
        for c in gen(kind):
            yield c


# ---- running one batch against the oracle -------------------------------------------------------------------------
_ORACLE = {}                                                   # (tag, b) -> (Fo, So): shared by the two routes


def oracle_of(kind, tag, P, b, Delta):
    """(factor quantities the checks need, step) of the oracle; the big arrays of its factor are not kept."""
    from types import SimpleNamespace
    key = (tag, b)
    if key not in _ORACLE:
        if kind == "trf":
            Fo, So = orc.trf_step_solve(P["J"][b], P["f"][b], P["x"][b], P["lb"][b], P["ub"][b],
                                        P["scale"][b], float(Delta[b]), 0.0)
            _ORACLE[key] = SimpleNamespace(v=Fo.v, s=Fo.s), So
        else:
            Fo, So = orc.dogbox_step_solve(P["J"][b], P["f"][b], P["x"][b], P["lb"][b], P["ub"][b],
                                           P["scale"][b], P["on_bound"][b], float(Delta[b]))
            _ORACLE[key] = SimpleNamespace(free=Fo.free, active=Fo.active), So
    return _ORACLE[key]


def _g_longdouble(P, b):
    return np.asarray(P["J"][b].T.astype(np.longdouble) @ P["f"][b].astype(np.longdouble))


class Tally:
    """What a sweep reached (asserted at its end) and what it found wrong."""

    def __init__(self):
        self.bad, self.worst, self.nprob = [], 0.0, 0
        self.branch, self.tr_hit, self.fast = set(), set(), set()
        self.max_n_iter, self.max_sweeps = 0, 0

    def check(self, ok, tag, b, what, value=None):
        if not ok:
            self.bad.append((tag, b, what, value))


def run_trf(bl, ctx, tag, P, Delta, forced, T, expect_fast=None):
    B, m, n = P["J"].shape
    ctx.gram_stats(reset=True)
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    fast = sol.debug_fast()
    sweeps = sol.debug_sweeps()
    _, sing = sol.fetch_factor(want_singular=True)
    S = sol.step(Delta, np.zeros(B))
    D = sol.fetch_step()
    sol.close()
    T.check(ctx.gram_stats() == (0, 0), tag, -1, "gram_stats", ctx.gram_stats())
    if expect_fast is not None and not forced:
        T.check(list(fast) == list(expect_fast), tag, -1, "debug_fast", list(fast))
    for b in range(B):
        Fo, So = oracle_of("trf", tag, P, b, Delta)
        lb, ub = P["lb"][b], P["ub"][b]
        g = _g_longdouble(P, b)
        g_norm = float(np.max(np.abs(g * Fo.v)))
        T.check(rel(F.g[b], g.astype(float)) < 1e-12, tag, b, "g", rel(F.g[b], g.astype(float)))
        T.check(abs(F.g_norm[b] - g_norm) <= 1e-12 * max(1.0, g_norm), tag, b, "g_norm", F.g_norm[b] - g_norm)
        if forced:
            T.check(int(fast[b]) == 0, tag, b, "debug_fast on the forced route", int(fast[b]))
            T.check(0 < int(sweeps[b]) < MAX_SWEEPS, tag, b, "sweeps", int(sweeps[b]))
            T.max_sweeps = max(T.max_sweeps, int(sweeps[b]))
        if not fast[b]:                                        # singular values exist only on the SVD route
            es = rel(np.sort(sing[b])[::-1], Fo.s)
            T.check(es < 1e-12, tag, b, "singular values", es)
        else:                                                  # the gate must never pass a rank-deficient problem
            T.check(m >= n and Fo.s[-1] > 1e3 * np.finfo(float).eps * m * Fo.s[0], tag, b, "gate passed rank-deficient")
        e = rel(S.step[b], So.step)
        T.worst = max(T.worst, e); T.nprob += 1
        T.check(e < RTOL, tag, b, "step", e)
        T.check(rel(S.x_new[b], So.x_new) < RTOL, tag, b, "x_new", rel(S.x_new[b], So.x_new))
        T.check(rel(D.p_h_tr[b], So.p_h_tr) < RTOL, tag, b, "p_h_tr", rel(D.p_h_tr[b], So.p_h_tr))
        T.check(np.array_equal(S.hits[b], So.hits), tag, b, "hits")
        T.check(np.array_equal(S.active_new[b], orc.active_constraints(So.x_new, lb, ub, rtol=1e-8)), tag, b,
                "active_new")
        T.check(int(S.n_iter[b]) == So.n_iter, tag, b, "n_iter", (int(S.n_iter[b]), So.n_iter))
        T.check(int(S.branch[b]) == So.branch, tag, b, "branch", (int(S.branch[b]), So.branch))
        T.check(abs(S.alpha[b] - So.alpha) <= 1e-9 * max(abs(So.alpha), 1e-300), tag, b, "alpha",
                (S.alpha[b], So.alpha))
        pr = So.predicted_reduction
        T.check(abs(S.predicted_reduction[b] - pr) <= 1e-10 * abs(pr), tag, b, "predicted_reduction",
                (S.predicted_reduction[b], pr))
        T.check(np.all(S.x_new[b] > lb) and np.all(S.x_new[b] < ub), tag, b, "x_new not strictly inside")
        T.check(int(S.status[b]) == 0, tag, b, "status", int(S.status[b]))
        T.branch.add(So.branch); T.max_n_iter = max(T.max_n_iter, So.n_iter); T.fast.add(int(fast[b]))
    return S


def run_dogbox(bl, ctx, tag, P, Delta, forced, T, expect_fast=None):
    B, m, n = P["J"].shape
    ctx.gram_stats(reset=True)
    sol = bl.DogboxStepSolver(B, m, n, ctx=ctx)
    F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    fast = sol.debug_fast()
    sweeps = sol.debug_sweeps()
    S = sol.step(Delta)
    sol.close()
    T.check(ctx.gram_stats() == (0, 0), tag, -1, "gram_stats", ctx.gram_stats())
    if expect_fast is not None and not forced:
        T.check(list(fast) == list(expect_fast), tag, -1, "debug_fast", list(fast))
    for b in range(B):
        Fo, So = oracle_of("dogbox", tag, P, b, Delta)
        assert So is not None, (tag, b, "every variable active: not a case")
        lb, ub = P["lb"][b], P["ub"][b]
        g = _g_longdouble(P, b)
        g_norm = float(np.max(np.abs(g[Fo.free])))
        T.check(rel(F.g[b], g.astype(float)) < 1e-12, tag, b, "g", rel(F.g[b], g.astype(float)))
        T.check(abs(F.g_norm[b] - g_norm) <= 1e-12 * max(1.0, g_norm), tag, b, "g_norm", F.g_norm[b] - g_norm)
        T.check(np.array_equal(F.active_set[b], Fo.active.astype(np.uint8)), tag, b, "active_set")
        if forced:
            T.check(int(fast[b]) == 0, tag, b, "debug_fast on the forced route", int(fast[b]))
            T.check(0 < int(sweeps[b]) < MAX_SWEEPS, tag, b, "sweeps", int(sweeps[b]))
            T.max_sweeps = max(T.max_sweeps, int(sweeps[b]))
        e = rel(S.step[b], So.step)
        T.worst = max(T.worst, e); T.nprob += 1
        T.check(e < RTOL, tag, b, "step", e)
        T.check(rel(S.x_new[b], So.x_new) < RTOL, tag, b, "x_new", rel(S.x_new[b], So.x_new))
        T.check(np.array_equal(S.on_bound_new[b], So.on_bound_new), tag, b, "on_bound_new")
        T.check(int(S.tr_hit[b]) == int(So.tr_hit), tag, b, "tr_hit", (int(S.tr_hit[b]), int(So.tr_hit)))
        T.check(int(S.fallback[b]) == int(So.fallback), tag, b, "fallback")
        pr = So.predicted_reduction
        T.check(abs(S.predicted_reduction[b] - pr) <= 1e-10 * abs(pr), tag, b, "predicted_reduction",
                (S.predicted_reduction[b], pr))
        T.check(np.all(S.x_new[b] >= lb) and np.all(S.x_new[b] <= ub), tag, b, "x_new outside the box")
        T.check(int(S.status[b]) == 0, tag, b, "status", int(S.status[b]))
        T.tr_hit.add(int(So.tr_hit)); T.fast.add(int(fast[b]))
    return S


RUN = {"trf": run_trf, "dogbox": run_dogbox}


# ---- fixtures -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bl():
    import bounded_lsq
    return bounded_lsq


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["svd_free", "svd_only"])
def tr_path(request, blsq_opt, ctx):
    """Both trust-region routes (the fixture of tests/test_hip_parity.py, on this module's context)."""
    blsq_opt("BLSQ_NO_SVDFREE", "1" if request.param == "svd_only" else "0", ctx=ctx)
    blsq_opt("BLSQ_SVDFREE_MIN_N", "0", ctx=ctx)
    return request.param


# ---- the width sweeps ---------------------------------------------------------------------------------------------
def test_width_sweep_trf(bl, ctx, tr_path):
    forced = tr_path == "svd_only"
    T = Tally()
    for tag, make, Delta in trf_sweep_cases():
        run_trf(bl, ctx, tag, make(), Delta, forced, T)
    print("wide TRF sweep (%s): %d problems, worst step error %.2e, most sweeps %d"
          % (tr_path, T.nprob, T.worst, T.max_sweeps))
    assert not T.bad, T.bad
    assert T.branch == {0, 1} and T.max_n_iter >= 2, (T.branch, T.max_n_iter)
    assert T.fast == ({0} if forced else {0, 1}), T.fast       # (m < n never passes the full-rank gate)


def test_width_sweep_dogbox(bl, ctx, tr_path):
    forced = tr_path == "svd_only"
    T = Tally()
    for tag, make, Delta in dogbox_sweep_cases():
        run_dogbox(bl, ctx, tag, make(), Delta, forced, T)
    print("wide dogbox sweep (%s): %d problems, worst step error %.2e, most sweeps %d"
          % (tr_path, T.nprob, T.worst, T.max_sweeps))
    assert not T.bad, T.bad
    assert T.tr_hit == {0, 1}, T.tr_hit
    assert T.fast == ({0} if forced else {0, 1}), T.fast


# ---- hard inputs at n = 400 and n = 512 ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trf", "dogbox"])
def test_hard_inputs_at_wide_n(bl, ctx, tr_path, kind):
    """Spectra up to kappa = 1e5 at the bar of 1e-10 (no excuse: the oracle's own step moves by at most 6e-12 there
    under one-ulp changes of J), rank-deficient columns with the debug_fast() pattern, columns scaled by 10^+-3."""
    forced = tr_path == "svd_only"
    T = Tally()
    n_iters = set()
    for tag, make, Delta in hard_cases(kind):
        P = make()
        S = RUN[kind](bl, ctx, tag, P, Delta, forced, T,
                      expect_fast=RANKDEF_FAST if "rankdef" in tag else None)
        if kind == "trf" and "spec" in tag:
            n_iters.update(int(v) for v in S.n_iter)
    print("hard inputs (%s, %s): %d problems, worst step error %.2e" % (kind, tr_path, T.nprob, T.worst))
    assert not T.bad, T.bad
    if kind == "trf":                                          # the Gauss-Newton step and Newton rounds both taken
        assert 0 in n_iters and max(n_iters) >= 2, n_iters
    assert T.fast == ({0} if forced else {0, 1}), T.fast


# ---- 'jac' scaling: the column norms come from the tree's R -------------------------------------------------------
def test_jac_scaling_at_n400(bl, ctx):
    from bounded_lsq import _synth, SCALE_JAC_INIT, SCALE_JAC_UPDATE
    B, m, n = 3, 1500, 400
    P = _synth.trf_batch(77, B, m, n)
    P["J"][1, :, 333] = 0.0                                    # zero column -> scale 1 at init
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], np.ones((B, n)), SCALE_JAC_INIT)
    ref = np.linalg.norm(P["J"], axis=1)
    ref[ref == 0] = 1.0
    np.testing.assert_allclose(F.scale, 1.0 / ref, rtol=1e-13)
    big = np.full((B, n), 1e-3)                                # min(scale, 1/norm) keeps the smaller
    F2 = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], big, SCALE_JAC_UPDATE)
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(F2.scale, np.minimum(big, 1.0 / np.linalg.norm(P["J"], axis=1)), rtol=1e-13)
    sol.close()
    dog = bl.DogboxStepSolver(B, m, n, ctx=ctx)
    Pd = _synth.dogbox_batch(78, B, m, n)
    Pd["J"][2, :, 5] = 0.0
    Fd = dog.factor(Pd["J"], Pd["f"], Pd["x"], Pd["lb"], Pd["ub"], np.ones((B, n)), Pd["on_bound"], SCALE_JAC_INIT)
    ref = np.linalg.norm(Pd["J"], axis=1)
    ref[ref == 0] = 1.0
    np.testing.assert_allclose(Fd.scale, 1.0 / ref, rtol=1e-13)
    dog.close()


# ---- bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trf", "dogbox"])
def test_bits_alone_in_a_batch_of_64_and_repeated(bl, ctx, kind):
    """1500 x 400: a problem's bits do not depend on its batch neighbours or on the run."""
    B, m, n = 64, 1500, 400
    P = _batch(kind, 6100, B, m, n)
    Delta = np.where(np.arange(B) % 2 == 0, 10.0, 0.5) if kind == "trf" else \
        np.where(np.arange(B) % 2 == 0, 5e-3, 5e-4)

    def solve(sol, sl):
        if kind == "trf":
            sol.factor(P["J"][sl], P["f"][sl], P["x"][sl], P["lb"][sl], P["ub"][sl], P["scale"][sl])
            S = sol.step(Delta[sl], np.zeros(len(Delta[sl])))
            return [np.copy(v) for v in (S.step, S.alpha, S.n_iter, S.hits, S.active_new, S.x_new)]
        sol.factor(P["J"][sl], P["f"][sl], P["x"][sl], P["lb"][sl], P["ub"][sl], P["scale"][sl], P["on_bound"][sl])
        S = sol.step(Delta[sl])
        return [np.copy(v) for v in (S.step, S.tr_hit, S.on_bound_new, S.x_new, S.predicted_reduction)]

    cls = bl.TrfStepSolver if kind == "trf" else bl.DogboxStepSolver
    sol = cls(B, m, n, ctx=ctx)
    runs = [solve(sol, slice(0, B)) for _ in range(3)]
    sol.close()
    for r in runs[1:]:
        for a, c in zip(runs[0], r):
            np.testing.assert_array_equal(a, c)
    if kind == "trf":
        assert set(int(v) for v in runs[0][2]) >= {0, 2}, set(runs[0][2])   # both the plain step and Newton rounds
    one = cls(1, m, n, ctx=ctx)
    for b in (5, 40):
        for a, c in zip(runs[0], solve(one, slice(b, b + 1))):
            np.testing.assert_array_equal(a[b], c[0])
    one.close()


# ---- end to end ---------------------------------------------------------------------------------------------------
def _linear_family(B=2, m=1200, n=300):
    """fun(x) = A x - y_b with the box [-0.05, 0.05]^n: about a third of the variables end on a bound."""
    rng = np.random.default_rng(2024)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    xt = rng.uniform(-0.08, 0.08, (B, n))
    Y = xt @ A.T + 1e-3 * rng.standard_normal((B, m))
    return A, Y


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_end_to_end_n300_all_drivers(bl, method):
    from scipy.optimize import lsq_linear
    B, m, n = 2, 1200, 300
    A, Y = _linear_family(B, m, n)
    lo, hi = np.full(n, -0.05), np.full(n, 0.05)
    X0 = np.zeros((B, n))

    def fun(X):
        X = np.atleast_2d(X)
        return X @ A.T - Y[:X.shape[0]]

    def jac(X):
        X = np.atleast_2d(X)
        return np.broadcast_to(A, (X.shape[0], m, n)).copy()
    kw = dict(bounds=(lo, hi), method=method, ftol=1e-14, xtol=1e-14, gtol=1e-14)
    host = bl.least_squares_batch(fun, X0, jac, driver='host', **kw)
    dev = bl.least_squares_batch(fun, X0, jac, driver='device', **kw)
    for b in range(B):
        seq = bl.least_squares(lambda x, b=b: A @ x - Y[b], X0[b], lambda x: A.copy(), **kw)
        ref = lsq_linear(A, Y[b], bounds=(lo, hi), method='bvls', tol=1e-14)
        on = int(np.sum(ref.active_mask != 0))
        assert 30 <= on <= n - 30, on                          # some variables end on a bound, some inside
        assert seq.status > 0
        for r, lvl in ((host[b], dict(rtol=1e-9, atol=1e-12)), (dev[b], dict(rtol=1e-9, atol=1e-12))):
            assert (r.nfev, r.njev, r.status) == (seq.nfev, seq.njev, seq.status), (b, method)
            np.testing.assert_allclose(r.x, seq.x, **lvl)
        np.testing.assert_allclose(seq.x, ref.x, rtol=1e-6)
