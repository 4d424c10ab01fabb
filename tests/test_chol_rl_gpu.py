"""The flag-driven N > 80 Cholesky (gram_chol_rl2_kernel, chol_rl.hip: wave 0 runs the 16 x 16 chains, fifteen worker
waves hold the tiles) against the left-looking reference kernel (BLSQ_CHOL_RL = 0), bit for bit.

Both kernels apply the same operands in the same order, so every output of a step-solve must be the same bits:
the factor with the certificate's share of stage 0 (the first factor of a TRF plan), the alpha-shifted systems of the
Newton rounds, the gathered principal sub-matrices of dogbox, and batches whose problems leave the Newton rounds at
different times (the rounds then factor a shrinking list of problems)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (81, 120, 200, 255, 256)          # N = n + 1 = 82 ... 257: 6 ... 17 tile columns, 1 ... 2 LDS-resident tile slots


@pytest.fixture(scope="module")
def bl():
    import bounded_lsq
    return bounded_lsq


def _trf_outputs(bl, P, B, m, n, Deltas):
    from bounded_lsq import _abi
    ctx = _abi.Context(0)
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    got = []
    for D in Deltas:
        S = sol.step(D, np.zeros(B))
        got += [S.step.copy(), np.asarray(S.alpha).copy(), S.predicted_reduction.copy(), np.asarray(S.n_iter).copy()]
    # the bound that the certificate proved, last: the factor kernel's share of stage 0 is the flag-driven kernel's
    # alone (the left-looking one leaves all of stage 0 to the certificate), so only runs of one kernel compare it
    got.append(sol.debug_cond().copy())
    sol.close(); ctx.close()
    return got


def _dogbox_outputs(bl, P, B, m, n, Deltas):
    from bounded_lsq import _abi
    ctx = _abi.Context(0)
    sol = bl.DogboxStepSolver(B, m, n, ctx=ctx)
    sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"], P["on_bound"])
    got = []
    for D in Deltas:
        S = sol.step(D)
        got += [S.step.copy(), S.predicted_reduction.copy(), S.on_bound_new.copy()]
    sol.close(); ctx.close()
    return got


def _same(outs, last=True):
    """every run's outputs equal the first run's, bit for bit (last = False: all but the last output)"""
    ref = outs[0]
    for got in outs[1:]:
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(ref, got)):
            if k < len(ref) - 1 or last:
                assert np.array_equal(a, b, equal_nan=True), k


@pytest.mark.parametrize("n", NS)
def test_trf_factor_and_newton_rounds_match_the_left_looking_kernel(bl, blsq_opt, n):
    """TRF: the certificate-sharing factor and the alpha-shifted Newton-round factors.  The trust radii are spread
    over three decades inside one batch, so the problems need different numbers of Newton rounds."""
    from bounded_lsq import _synth
    B, m = 6, max(2 * n, 300)
    P = _synth.trf_batch(500 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 10.0, B), np.full(B, 0.3), np.full(B, 50.0)]
    outs = []
    for rl in ("0", "1"):
        blsq_opt("BLSQ_CHOL_RL", rl)
        outs.append(_trf_outputs(bl, P, B, m, n, Deltas))
    _same(outs, last=False)


@pytest.mark.parametrize("n", NS)
def test_unbounded_trf_matches_the_left_looking_kernel(bl, blsq_opt, n):
    """Unbounded problems: H = J^T J without the diagonal term (the first factor is the plain Gram's)."""
    from bounded_lsq import _synth
    B, m = 4, max(2 * n, 300)
    P = _synth.trf_batch(600 + n, B, m, n, unbounded=True)
    Deltas = [np.geomspace(0.05, 5.0, B)]
    outs = []
    for rl in ("0", "1"):
        blsq_opt("BLSQ_CHOL_RL", rl)
        outs.append(_trf_outputs(bl, P, B, m, n, Deltas))
    _same(outs, last=False)


@pytest.mark.parametrize("n", NS)
def test_dogbox_gathered_submatrices_match_the_left_looking_kernel(bl, blsq_opt, n):
    """dogbox: the factor of the gathered free columns (a principal sub-matrix of the kept Gram)."""
    from bounded_lsq import _synth
    B, m = 5, max(2 * n, 300)
    P = _synth.dogbox_batch(700 + n, B, m, n)
    Deltas = [np.geomspace(0.01, 1.0, B), np.full(B, 0.05)]
    outs = []
    for rl in ("0", "1"):
        blsq_opt("BLSQ_CHOL_RL", rl)
        outs.append(_dogbox_outputs(bl, P, B, m, n, Deltas))
    _same(outs)


def test_sixteen_wave_flag_protocol_is_race_free_under_repetition(bl, blsq_opt):
    """The hand-overs between wave 0 and the fifteen workers (and the LDS-resident tile slots) must give the same bits
    on every run: each shape — the largest factor, two LDS slots with the certificate, more problems than CUs, a
    gathered sub-matrix — is solved ten times against one run of the left-looking kernel."""
    from bounded_lsq import _synth
    for (B, m, n, kind) in [(2, 600, 256, "trf"), (3, 500, 255, "trf"), (300, 300, 200, "trf"), (40, 400, 120, "dogbox")]:
        P = _synth.trf_batch(800 + n, B, m, n) if kind == "trf" else _synth.dogbox_batch(800 + n, B, m, n)
        Deltas = [np.geomspace(0.02, 2.0, B)]
        outs = []
        for rl in ["0"] + ["1"] * 10:
            blsq_opt("BLSQ_CHOL_RL", rl)
            if kind == "trf":
                outs.append(_trf_outputs(bl, P, B, m, n, Deltas))
            else:
                outs.append(_dogbox_outputs(bl, P, B, m, n, Deltas))
        _same(outs, last=kind != "trf")                 # every run against the left-looking kernel ...
        if kind == "trf":
            _same(outs[1:])                             # ... and the certificate's bound against the first run
