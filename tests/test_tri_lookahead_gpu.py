"""The look-ahead schedule of the blocked triangular solves (tri_solve_upper_pf_la / tri_solve_upper_t_pf_la, tri_ops.h:
wave 0 substitutes the next diagonal block while the other waves update, one barrier per block step) against the
three-barrier reference schedule (Context.tri_reference(True): blsq_debug_tri_reference), bit for bit.

Both schedules give every entry of the solution the same operations in the same order, so every output of a step-solve
must be the same bits through every kernel that calls the solves: lm_start / lm_update (TRF), the one-pass and the
four-pass form of the certificate's stage 0 (gram_cert0_kernel; the latter with both comparison-matrix solves),
lm_gate_kernel's inverse iteration (Householder path), dog_gate_solve_kernel (gathered sub-matrices: widths that are no
multiple of 16), and the CSNE tier's recording and correction.  The factor kernel is the same in both runs, so the
certificate's proven bound (debug_cond) compares too.

Widths: 81 (the last block holds one column), 96 (whole blocks), 97, 209 (the first width whose bulk update has more than
192 rows: a thread of waves 1 .. 3 gets a second row), 240 / 241, 255 / 256."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (81, 96, 97, 209, 240, 241, 255, 256)


@pytest.fixture(scope="module")
def bl():
    import bounded_lsq
    return bounded_lsq


def _trf_outputs(bl, P, Deltas, ref, stats=None):
    from bounded_lsq import _abi
    B, m, n = P["J"].shape
    ctx = _abi.Context(0)
    ctx.tri_reference(ref)
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    if stats is not None:
        ctx.csne_stats(reset=True)
    sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    got = []
    for D in Deltas:
        S = sol.step(D, np.zeros(B))
        got += [S.step.copy(), np.asarray(S.alpha).copy(), S.predicted_reduction.copy(), np.asarray(S.n_iter).copy()]
    got.append(sol.debug_cond().copy())
    if stats is not None:
        stats.append(ctx.csne_stats())
    sol.close(); ctx.close()
    return got


def _dogbox_outputs(bl, P, Deltas, ref):
    from bounded_lsq import _abi
    B, m, n = P["J"].shape
    ctx = _abi.Context(0)
    ctx.tri_reference(ref)
    sol = bl.DogboxStepSolver(B, m, n, ctx=ctx)
    sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    got = []
    for D in Deltas:
        S = sol.step(D)
        got += [S.step.copy(), S.predicted_reduction.copy(), S.on_bound_new.copy()]
    sol.close(); ctx.close()
    return got


def _same(outs):
    """every run's outputs equal the first run's, bit for bit"""
    ref = outs[0]
    for got in outs[1:]:
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(ref, got)):
            assert np.array_equal(a, b, equal_nan=True), k


def _both_routes(run):
    """run(ref): the three-barrier reference first, then the look-ahead"""
    outs = [run(True), run(False)]
    _same(outs)
    return outs


@pytest.mark.parametrize("n", NS)
def test_trf_bounded_matches_the_three_barrier_solves(bl, n):
    """Radii spread over three decades inside one batch (different round counts, a problem that accepts the Gauss-Newton
    step beside ones that iterate), then all 0.3, then all 50."""
    from bounded_lsq import _synth
    B, m = 6, max(2 * n, 300)
    P = _synth.trf_batch(1500 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 10.0, B), np.full(B, 0.3), np.full(B, 50.0)]
    _both_routes(lambda ref: _trf_outputs(bl, P, Deltas, ref))


@pytest.mark.parametrize("n", NS)
def test_trf_unbounded_matches_the_three_barrier_solves(bl, n):
    from bounded_lsq import _synth
    B, m = 4, max(2 * n, 300)
    P = _synth.trf_batch(1600 + n, B, m, n, unbounded=True)
    Deltas = [np.geomspace(0.05, 5.0, B)]
    _both_routes(lambda ref: _trf_outputs(bl, P, Deltas, ref))


@pytest.mark.parametrize("n", NS)
def test_four_pass_certificate_matches_the_three_barrier_solves(bl, blsq_opt, n):
    """BLSQ_CHOL_RL = 0: the left-looking factor kernel leaves all of stage 0 to the certificate, which then runs both
    comparison-matrix solves (the CMP instantiations of the two routines)."""
    from bounded_lsq import _synth
    B, m = 5, max(2 * n, 300)
    P = _synth.trf_batch(1700 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 10.0, B)]
    blsq_opt("BLSQ_CHOL_RL", "0")
    _both_routes(lambda ref: _trf_outputs(bl, P, Deltas, ref))


@pytest.mark.parametrize("n", (97, 256))
def test_householder_path_matches_the_three_barrier_solves(bl, blsq_opt, n):
    """BLSQ_GRAM = 0: R_aug from the stacked QR, and lm_gate_kernel's inverse iteration."""
    from bounded_lsq import _synth
    B, m = 4, max(2 * n, 300)
    P = _synth.trf_batch(1800 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 10.0, B), np.full(B, 0.3)]
    blsq_opt("BLSQ_GRAM", "0")
    _both_routes(lambda ref: _trf_outputs(bl, P, Deltas, ref))


@pytest.mark.parametrize("n", NS)
def test_dogbox_matches_the_three_barrier_solves(bl, n):
    """Gathered principal sub-matrices: the widths nf of the solves are whatever the free sets are."""
    from bounded_lsq import _synth
    B, m = 5, max(2 * n, 300)
    P = _synth.dogbox_batch(1900 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 1.0, B), np.full(B, 0.05)]
    _both_routes(lambda ref: _dogbox_outputs(bl, P, Deltas, ref))


@pytest.mark.parametrize("m,n", [(1024, 96), (4096, 256)])
def test_csne_tier_matches_the_three_barrier_solves(bl, m, n):
    """Unbounded problems with kappa(J) = 3e3 (as tests/test_csne_gpu.py builds them): the certificate rejects them, the
    tier records four extra solves per evaluation and csne_fix_kernel solves once more."""
    from bounded_lsq import _synth
    B = 4
    rng = np.random.default_rng(2000 + n)
    P = _synth.trf_batch(77, B, m, n, unbounded=True)
    for b in range(B):
        U, _ = np.linalg.qr(rng.standard_normal((m, n)))
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        P["J"][b] = (U * np.logspace(0, -np.log10(3e3), n)) @ V.T * np.sqrt(m)
    Deltas = [np.array([10.0, 0.5, 0.05, 1e6])]
    stats = []
    _both_routes(lambda ref: _trf_outputs(bl, P, Deltas, ref, stats))
    assert all(s[0] == B for s in stats), stats              # (every problem was routed to the tier, in both runs)


def test_more_problems_than_resident_workgroups(bl):
    """B = 520 at n = 96: more workgroups than a launch keeps resident.  Four problems also against the oracle: the
    normal-equations path loses kappa_2(C) eps with kappa_2(C) <= 2.5e5 proven by the certificate, 5.6e-11; 1e-10 is
    the bound __graft_entry__.smoke() holds this path to."""
    from bounded_lsq import _synth
    from oracle import blsq_oracle as orc
    B, m, n = 520, 200, 96
    P = _synth.trf_batch(2100, B, m, n)
    Delta = np.geomspace(0.01, 10.0, B)
    outs = _both_routes(lambda ref: _trf_outputs(bl, P, [Delta], ref))
    step, n_iter = outs[1][0], outs[1][3]
    for b in (0, 173, 346, 519):
        _, So = orc.trf_step_solve(P["J"][b], P["f"][b], P["x"][b], P["lb"][b], P["ub"][b], P["scale"][b], Delta[b], 0.0)
        err = np.linalg.norm(step[b] - So.step) / np.linalg.norm(So.step)
        print("problem", b, "step error", err)
        assert err < 1e-10, (b, err)
        assert int(n_iter[b]) == So.n_iter, (b, n_iter[b], So.n_iter)


def test_look_ahead_gives_the_same_bits_on_every_run(bl):
    """Each shape is solved five times with the look-ahead against one run of the three-barrier reference."""
    from bounded_lsq import _synth
    for (B, m, n, kind) in [(2, 600, 256, "trf"), (3, 500, 255, "trf"), (40, 400, 120, "dogbox")]:
        P = _synth.trf_batch(2200 + n, B, m, n) if kind == "trf" else _synth.dogbox_batch(2200 + n, B, m, n)
        Deltas = [np.geomspace(0.02, 2.0, B)]
        outs = []
        for ref in [True] + [False] * 5:
            outs.append(_trf_outputs(bl, P, Deltas, ref) if kind == "trf" else _dogbox_outputs(bl, P, Deltas, ref))
        _same(outs)
