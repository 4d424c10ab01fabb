"""The LDS-DMA staging of the 16-tile Gram kernel (gram16_kernel<true, PAIR, true>, n = 256) against the register staging
it replaces on the default route (Context.gram_regstage(True): blsq_debug_gram_regstage), bit for bit.

Both stagings put the same rows into the same LDS buffers, every tile sees the same k-steps in the same order, and the
rhs column J^T f / f^T f is the same chain of fma calls per wave (from LDS instead of from the staging registers), so
every output of a factor and a step call must be the same bits.

Row counts.  The kernel streams 32-row chunks through two LDS buffers; a chunk's rows are requested while the chunk
before it is multiplied.  The cases are the ones where that can go wrong: a single chunk (nothing is ever requested
ahead), two chunks (each buffer used once), a ragged last chunk of 8 and of 2 rows (clamped requests, the owning wave
clears its rows), the 2048-row boundary between two workgroups' row chunks, and the same boundary inside ONE workgroup
(PAIR: 256 problems; the first chunk's sums are parked and read back).

m = 32, 64, 40 and 34 are below n = 256: such problems never reach a Gram kernel (gram_supported: m < n fails the gate
by construction), so these four cases pass through the Householder tree on both settings of the switch and
gram_stats() counts nothing — they are kept as row counts the switch must not disturb.  Their chunk structure is repeated at the smallest
row counts the normal-equations path takes: m = 256 (whole chunks, an even number), 288 (an odd number: the pass ends
in the other buffer), 264 and 258 (ragged by 8 and by 2).  Small batches run the 16-tile kernel only with one workgroup
per row chunk and without the one-tile-per-wave kernel: BLSQ_GRAM_TILE_GROUPS = 1, BLSQ_GRAM1 = 0."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 256
DELTA = 0.7


@pytest.fixture(scope="module")
def bl():
    import bounded_lsq
    return bounded_lsq


def _problems(B, m, seed):
    """B problems of m x 256; more than 8: copies of 8 base problems with f scaled per problem"""
    from bounded_lsq import _synth
    if B <= 8:
        return _synth.trf_batch(seed, B, m, N)
    base = _synth.trf_batch(seed, 8, m, N)
    P = {k: np.concatenate([v] * ((B + 7) // 8))[:B].copy() for k, v in base.items()}
    P["f"] = P["f"] * (1.0 + 0.01 * np.arange(B))[:, None]
    return P


def _solve(bl, P, regstage):
    """-> (g, step, alpha, gram_stats) of one factor + step through the host-pointer entries"""
    from bounded_lsq import _abi
    B, m, n = P["J"].shape
    ctx = _abi.Context(0)
    ctx.gram_regstage(regstage)
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    ctx.gram_stats(reset=True)
    sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    stats = ctx.gram_stats()
    S = sol.step(np.full(B, DELTA), np.zeros(B))
    out = (sol.fetch_factor().g.copy(), S.step.copy(), np.asarray(S.alpha).copy(), stats)
    sol.close(); ctx.close()
    return out


def _small_batch_route(blsq_opt):
    blsq_opt("BLSQ_GRAM_TILE_GROUPS", "1")
    blsq_opt("BLSQ_GRAM1", "0")


def _both(bl, P):
    ref = _solve(bl, P, True)                  # the register staging
    got = _solve(bl, P, False)                 # LDS-DMA where the launch qualifies
    B, m, n = P["J"].shape
    for k, name in enumerate(("g", "step", "alpha")):
        print((B, m), name, "differing entries:", int(np.sum(ref[k] != got[k])))
        assert np.array_equal(ref[k], got[k]), ((B, m), name)
    want = (B, 0) if m >= n else (0, 0)        # (m < n: the plan has no Gram front end, nothing is counted)
    assert ref[3] == want and got[3] == want, ((B, m), ref[3], got[3])
    return ref, got


@pytest.mark.parametrize("B,m", [(2, 32), (3, 64), (2, 40), (2, 34),        # (m < n: see the module docstring)
                                 (2, 256), (3, 288), (2, 264), (2, 258),
                                 (2, 2080), (2, 2050)])
def test_dma_staging_matches_register_staging_one_workgroup_per_row_chunk(bl, blsq_opt, B, m):
    """One workgroup per row chunk of at most 2048 rows (no PAIR).  m = 2080: the second workgroup's pass is a single
    chunk; m = 2050: a single ragged chunk of 2 rows — its prologue clears 30 rows."""
    _small_batch_route(blsq_opt)
    _both(bl, _problems(B, m, 3100 + m))


@pytest.mark.parametrize("B,m", [(256, 2080), (256, 2050)])
def test_dma_staging_matches_register_staging_chunk_pairs(bl, B, m):
    """256 problems of two row chunks on the default route: one workgroup takes both (PAIR), parks the first chunk's
    tiles and rhs sums at row 2048 and adds them back at the end."""
    _both(bl, _problems(B, m, 3300 + m))


def _solve_dev(bl, P, regstage, j_offset):
    """As _solve through the device-pointer entries; J at `j_offset` bytes inside a larger allocation."""
    from bounded_lsq import _abi
    B, m, n = P["J"].shape
    ctx = _abi.Context(0)
    ctx.gram_regstage(regstage)
    sol = bl.TrfStepSolver(B, m, n, ctx=ctx)
    J = np.ascontiguousarray(P["J"])
    raw = ctx.malloc(J.nbytes + 16)
    dJ = C.c_void_p(raw.value + j_offset)
    ctx.check(ctx.lib.blsq_memcpy_h2d(ctx.h, dJ, J.ctypes.data_as(C.c_void_p), J.nbytes), "blsq_memcpy_h2d")
    d = {k: ctx.to_device(P[k]) for k in ("f", "x", "lb", "ub", "scale")}
    dD, dA = ctx.to_device(np.full(B, DELTA)), ctx.to_device(np.zeros(B))
    ctx.gram_stats(reset=True)
    sol.factor_dev(dJ, d["f"], d["x"], d["lb"], d["ub"], d["scale"])
    sol.step_dev(dD, dA)
    S = sol.fetch_step()
    out = (sol.fetch_factor().g.copy(), S.step.copy(), np.asarray(S.alpha).copy(), ctx.gram_stats())
    for v in list(d.values()) + [dD, dA, raw]:
        ctx.free(v)
    sol.close(); ctx.close()
    return out


def test_misaligned_jacobian_takes_the_register_staging(bl, blsq_opt):
    """A J whose base is 8 bytes past a 16-byte boundary cannot be requested 16 bytes at a time: launch_gram keeps the
    register staging for it, so the default setting gives the bits the forced register route gives for an aligned copy
    of the same numbers (and the aligned copy on the default setting — the DMA staging — the same again)."""
    _small_batch_route(blsq_opt)
    B, m = 2, 264
    P = _problems(B, m, 3500)
    ref = _solve_dev(bl, P, True, 0)
    for got in (_solve_dev(bl, P, False, 8), _solve_dev(bl, P, False, 0)):
        for k, name in enumerate(("g", "step", "alpha")):
            assert np.array_equal(ref[k], got[k]), name
        assert ref[3] == (B, 0) and got[3] == (B, 0), (ref[3], got[3])


def test_nan_in_the_last_row_of_a_ragged_chunk(bl, blsq_opt):
    """Problem 0 has a NaN in its last row, the only valid row pair of a ragged chunk (m = 258): the clamped requests
    of rows >= m fetch that row again.  Both stagings must leave the same g, byte for byte.  (Non-finite input fails
    the gate by construction: problem 0 is handed on, problem 1 stays on the normal-equations path.)"""
    _small_batch_route(blsq_opt)
    B, m = 2, 258
    P = _problems(B, m, 3600)
    P["J"][0, m - 1, 5] = np.nan
    ref = _solve(bl, P, True)
    got = _solve(bl, P, False)
    assert ref[0].tobytes() == got[0].tobytes()
    assert np.array_equal(ref[1][1], got[1][1]) and np.array_equal(ref[2][1], got[2][1])
    assert ref[3] == (B - 1, 1) and got[3] == (B - 1, 1), (ref[3], got[3])
