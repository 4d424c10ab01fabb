"""Separable global fits on the GPU: blsq_varpro_expand_global_dev, blsq_varpro_reduce_global_dev and
blsq_varpro_cov_blocks_dev in isolation — exact, bit for bit, against the existing blsq_varpro_reduce_dev passed through
``GlobalMap.reduce_jac``; Sinv and TD against np.longdouble under the caps of tests/_separable_global_cases.py; the
covariance blocks against the numpy definition under a summation bound — and whole fits with
``curve_fit_global(separable=True)`` on both drivers against the plain (dense) global fit, with the package's margins
between two routes: popt rtol 1e-6 / atol 1e-9, pcov atol 1e-6 after dividing by the reference's standard deviations.

The large-S fit (S = 300, two shared rates: nv = 2, the plain route would need 902 > 256 columns) fails without the
feature.  The worst fractions of the caps seen on an MI355X are in DESIGN.md 7x."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import models

import _model_eval as me
import _separable_cases as sc
import _separable_global_cases as gc
from _model_eval import ctx, same_bits  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload
ISENT = -77
OUTPUTS = ("f", "J", "c", "info", "Sinv", "TD")
worst = {}


def group_w(cs, wform):
    """The weights of a case as the global entry takes them: None, (m,) or (G, S m); and their stride."""
    w = cs.ws[wform]
    if wform == "per_problem":
        return w.reshape(cs.G, cs.S * cs.m), cs.S * cs.m
    return w, 0


def reduce_global(ctx, cs, wform="none", want=OUTPUTS, mask=None, Graw=None, **over):
    """blsq_varpro_reduce_global_dev on a case -> (rc, dict of the outputs asked for), each pre-filled with a sentinel."""
    G, S, m, n, nl, na, nv = cs.G, cs.S, cs.m, cs.n, cs.nl, cs.na, cs.nv
    w, stride = group_w(cs, wform)
    a = dict(G=G, S=S, m=m, n=n, nl=nl, lin=cs.lin, owner=cs.owner, shared=cs.shared, w_stride=stride)
    a.update(over)
    lin, p_lin = me.i32(a["lin"])
    owner, p_owner = me.i32(a["owner"])
    shared, p_shared = me.i32(a["shared"])
    shapes = dict(f=(G, S * m), J=(G, S * m, nv), c=(G * S, nl), info=(G * S,), Sinv=(G * S, nl, nl), TD=(G * S, nl, na))
    with me.Dev(ctx) as d:
        out = {k: d.up(np.full(shapes[k], ISENT, dtype=np.int32) if k == "info" else np.full(shapes[k], SENTINEL))
               for k in want}
        rc = ctx.lib.blsq_varpro_reduce_global_dev(
            ctx.h, a["G"], a["S"], a["m"], a["n"], a["nl"], p_lin, p_owner, p_shared,
            over.get("G_ptr", d.up(cs.Graw if Graw is None else Graw)), over.get("y_ptr", d.up(cs.y)), d.up(w),
            a["w_stride"], *(out.get(k) for k in OUTPUTS),
            d.up(None if mask is None else np.asarray(mask, dtype=np.int32)))
        ctx.sync()
        return rc, {k: ctx.to_host(p, shapes[k], np.int32 if k == "info" else np.float64) for k, p in out.items()}


def reduce_plain(ctx, cs, wform="none", Graw=None):
    """The existing blsq_varpro_reduce_dev on the G S data sets, passed through reshape / ``GlobalMap.reduce_jac``."""
    B, m, n, nl, na = cs.G * cs.S, cs.m, cs.n, cs.nl, cs.na
    w = cs.ws[wform]
    lin, p_lin = me.i32(cs.lin)
    owner, p_owner = me.i32(cs.owner)
    with me.Dev(ctx) as d:
        d_f, d_J, d_c = d.up(np.full((B, m), SENTINEL)), d.up(np.full((B, m, na), SENTINEL)), d.up(np.full((B, nl), SENTINEL))
        d_info = d.up(np.full(B, ISENT, dtype=np.int32))
        assert ctx.lib.blsq_varpro_reduce_dev(ctx.h, B, m, n, nl, p_lin, p_owner, d.up(cs.Graw if Graw is None else Graw),
                                              d.up(cs.y), d.up(w), me.w_stride(w, m), d_f, d_J, d_c, d_info, None) == 0
        ctx.sync()
        f, J = ctx.to_host(d_f, (B, m), np.float64), ctx.to_host(d_J, (B, m, na), np.float64)
        c, info = ctx.to_host(d_c, (B, nl), np.float64), ctx.to_host(d_info, (B,), np.int32)
    return dict(f=f.reshape(cs.G, cs.S * m), J=cs.gm.reduce_jac(J.reshape(cs.G, cs.S, m, na)), c=c, info=info)


def foreign(cs):
    """(G, S m, nv) bool: the elements of J outside the columns of the row's data set."""
    out = np.ones((cs.G, cs.S, cs.m, cs.nv), dtype=bool)
    for s in range(cs.S):
        out[:, s][..., cs.gm.cols[s]] = False
    return out.reshape(cs.G, cs.S * cs.m, cs.nv)


# ---- the kernels, exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", gc.GROUPS)
@pytest.mark.parametrize("shape", gc.GRID, ids=str)
def test_expand_global_is_the_definition(ctx, shape, G):
    cs = gc.group_case(*shape, G)
    X = cs.X.copy()
    X[0, 0] = SENTINEL                            # (a payload passes through)
    lin, p_lin = me.i32(cs.lin)
    shared, p_shared = me.i32(cs.shared)
    with me.Dev(ctx) as d:
        d_P = d.up(np.full((G * cs.S, cs.n), 5.0))
        assert ctx.lib.blsq_varpro_expand_global_dev(ctx.h, G, cs.S, cs.n, cs.nl, p_lin, p_shared, d.up(X), d_P) == 0
        P = ctx.to_host(d_P, (G * cs.S, cs.n), np.float64)
    assert same_bits(P, gc.expand_definition(cs, X))


@pytest.mark.parametrize("wform", sc.WFORMS)
@pytest.mark.parametrize("G", gc.GROUPS)
@pytest.mark.parametrize("shape", gc.GRID, ids=str)
def test_reduce_global_has_the_bits_of_the_existing_entry(ctx, shape, G, wform):
    cs = gc.group_case(*shape, G)
    assert cs.nv <= 256
    rc, out = reduce_global(ctx, cs, wform)
    ref = reduce_plain(ctx, cs, wform)
    assert rc == 0 and out["info"].tolist() == [0] * (G * cs.S)
    for k in ("f", "J", "c", "info"):
        assert same_bits(out[k], ref[k]), k
    away = foreign(cs)
    assert np.all(me.bits(out["J"])[away] == 0)   # the all-zero pattern: +0.0, written by the kernel over the sentinel
    assert not np.isnan(out["Sinv"]).any() and not np.isnan(out["TD"]).any()
    assert same_bits(out["Sinv"], np.swapaxes(out["Sinv"], 1, 2))


def test_one_data_set_with_everything_shared_is_the_existing_entry(ctx):
    base = gc.group_case(65, 16, 48, 1, 48, 3)
    rc, out = reduce_global(ctx, base, "per_problem", want=("f", "J", "c", "info"))
    ref = reduce_plain(ctx, base, "per_problem")
    assert rc == 0 and base.nv == base.na
    B = base.G
    lin, p_lin = me.i32(base.lin)
    owner, p_owner = me.i32(base.owner)
    with me.Dev(ctx) as d:                        # and the raw layout [B][m][na] itself, without reduce_jac
        d_J = d.up(np.full((B, base.m, base.na), SENTINEL))
        assert ctx.lib.blsq_varpro_reduce_dev(ctx.h, B, base.m, base.n, base.nl, p_lin, p_owner, d.up(base.Graw),
                                              d.up(base.y), d.up(base.ws["per_problem"]), base.m, None, d_J, None, None,
                                              None) == 0
        ctx.sync()
        assert same_bits(ctx.to_host(d_J, (B, base.m, base.na), np.float64), out["J"])
    for k in ("f", "J", "c", "info"):
        assert same_bits(out[k], ref[k]), k


def test_reduce_global_outputs_are_independent(ctx):
    cs = gc.group_case(65, 16, 48, 3, 40, 3)
    rc, full = reduce_global(ctx, cs, "per_problem")
    assert rc == 0
    for want in (("f",), ("J",), ("c", "info"), ("Sinv",), ("TD",), ("f", "TD")):
        rc, part = reduce_global(ctx, cs, "per_problem", want=want)
        assert rc == 0 and set(part) == set(want)
        for k in want:
            assert same_bits(part[k], full[k]), k


def test_a_rank_deficient_data_set_keeps_to_itself(ctx):
    cs = gc.group_case(63, 5, 11, 4, 6, 3)
    rc, good = reduce_global(ctx, cs)
    Graw = cs.Graw.copy()
    b = 1 * cs.S + 2                              # data set 2 of group 1
    Graw[b, :, cs.lin[3]] = Graw[b, :, cs.lin[0]]                    # two identical Phi columns
    rc2, out = reduce_global(ctx, cs, Graw=Graw)
    assert rc == 0 and rc2 == 0
    info = np.zeros(cs.G * cs.S, dtype=int)
    info[b] = 1
    assert out["info"].tolist() == info.tolist()
    m, rows = cs.m, slice(2 * cs.m, 3 * cs.m)
    own = cs.gm.cols[2]
    assert np.isnan(out["f"][1, rows]).all() and np.isnan(out["J"][1, rows][:, own]).all()
    assert np.isnan(out["c"][b]).all() and np.isnan(out["Sinv"][b]).all() and np.isnan(out["TD"][b]).all()
    other = np.setdiff1d(np.arange(cs.nv), own)
    assert np.all(me.bits(out["J"][1, rows][:, other]) == 0)        # its other columns are still +0.0
    for k in OUTPUTS:                             # everything else keeps its bits
        a, g = out[k].copy(), good[k].copy()
        if k in ("f", "J"):
            a[1, rows], g[1, rows] = 0, 0
        else:
            a[b], g[b] = 0, 0
        assert same_bits(a, g), k


def test_a_masked_group_keeps_its_sentinel(ctx):
    cs = gc.group_case(130, 3, 61, 2, 30, 3)
    rc, full = reduce_global(ctx, cs, "shared")
    Graw = cs.Graw.copy()
    Graw[cs.S:2 * cs.S] = np.nan                  # nothing of a masked group is read either
    rc2, out = reduce_global(ctx, cs, "shared", mask=[1, 0, 1], Graw=Graw)
    assert rc == 0 and rc2 == 0
    for k in ("f", "J"):
        assert same_bits(out[k][1], np.full(out[k][1].shape, SENTINEL)), k
        assert same_bits(out[k][[0, 2]], full[k][[0, 2]]), k
    sets = np.arange(cs.S, 2 * cs.S)
    rest = np.setdiff1d(np.arange(cs.G * cs.S), sets)
    for k in ("c", "Sinv", "TD"):
        assert same_bits(out[k][sets], np.full(out[k][sets].shape, SENTINEL)), k
        assert same_bits(out[k][rest], full[k][rest]), k
    assert out["info"][sets].tolist() == [ISENT] * cs.S and out["info"][rest].tolist() == [0] * rest.size


@pytest.mark.parametrize("shape", [(63, 5, 11, 4, 6), (130, 3, 61, 2, 30), (257, 16, 1, 7, 1)], ids=str)
def test_the_bits_of_a_group_do_not_depend_on_G(ctx, shape):
    cs = gc.group_case(*shape, 3)
    rc, full = reduce_global(ctx, cs, "per_problem")
    assert rc == 0
    for g in (0, 2):
        rc, one = reduce_global(ctx, cs.only(g), "per_problem")
        assert rc == 0
        sets = slice(g * cs.S, (g + 1) * cs.S)
        for k in OUTPUTS:
            assert same_bits(one[k], full[k][g:g + 1] if k in ("f", "J") else full[k][sets]), (k, g)


def test_bad_arguments_return_their_positions_and_launch_nothing(ctx):
    cs = gc.group_case(63, 5, 11, 4, 6, 3)
    lin, owner, shared = cs.lin, cs.owner, cs.shared
    on_lin = shared.copy()
    on_lin[lin[0]] = 1
    two = shared.copy()
    two[cs.non[0]] = 2
    bad_owner = owner.copy()
    bad_owner[cs.non[0]] = cs.nl
    local = np.zeros_like(shared)                 # nothing shared: nv = 52 * 11 > 256 with S = 52
    cases = [
        (dict(G=0), 2), (dict(S=0), 3), (dict(S=52, shared=local), 3), (dict(m=0), 4), (dict(m=cs.nl), 4),
        (dict(n=65), 5), (dict(n=1), 5), (dict(nl=0), 6), (dict(nl=17), 6), (dict(lin=lin[::-1]), 7),
        (dict(owner=bad_owner), 8), (dict(shared=on_lin), 9), (dict(shared=two), 9), (dict(G_ptr=None), 10),
        (dict(y_ptr=None), 11), (dict(w_stride=cs.m), 13), (dict(w_stride=7), 13), (dict(want=("info",)), 14),
    ]
    for over, index in cases:
        wform = "per_problem" if "w_stride" in over else "none"
        if over.get("S") == 52:                   # (the buffers of the case are smaller: nothing may be launched)
            rc = reduce_global_rc_only(ctx, cs, **over)
        else:
            rc, out = reduce_global(ctx, cs, wform, **over)
            for k, v in out.items():
                assert same_bits(v, np.full(v.shape, ISENT, dtype=np.int32) if k == "info" else np.full(v.shape, SENTINEL))
        assert rc == -index, (over, rc)
    arr, p_lin = me.i32(lin)
    sh, p_shared = me.i32(shared)
    ol, p_on_lin = me.i32(on_lin)
    with me.Dev(ctx) as d:
        d_X, d_P = d.up(cs.X), d.up(np.full((cs.G * cs.S, cs.n), SENTINEL))
        ok = (cs.G, cs.S, cs.n, cs.nl, p_lin, p_shared, d_X, d_P)
        for at, value, index in ((0, 0, 2), (1, 0, 3), (2, 65, 4), (3, 17, 5), (4, None, 6), (5, None, 7),
                                 (5, p_on_lin, 7), (6, None, 8), (7, None, 9)):
            args = list(ok)
            args[at] = value
            assert ctx.lib.blsq_varpro_expand_global_dev(ctx.h, *args) == -index, (at, index)
        ctx.sync()
        assert same_bits(ctx.to_host(d_P, (cs.G * cs.S, cs.n), np.float64), np.full((cs.G * cs.S, cs.n), SENTINEL))
        d_cov = d.up(np.full((cs.G * cs.S, cs.n, cs.n), SENTINEL))
        d_C, d_S, d_T = d.up(np.zeros((cs.G, cs.nv, cs.nv))), d.up(np.zeros((cs.G * cs.S, cs.nl, cs.nl))), d.up(
            np.zeros((cs.G * cs.S, cs.nl, cs.na)))
        ok = (cs.G, cs.S, cs.n, cs.nl, p_lin, p_shared, d_C, d_S, d_T, None, None, None, d_cov)
        for at, value, index in ((0, 0, 2), (1, 0, 3), (2, 1, 4), (3, 0, 5), (4, None, 6), (5, p_on_lin, 7), (6, None, 8),
                                 (7, None, 9), (8, None, 10), (12, None, 14)):
            args = list(ok)
            args[at] = value
            assert ctx.lib.blsq_varpro_cov_blocks_dev(ctx.h, *args) == -index, (at, index)
        ctx.sync()
        assert same_bits(ctx.to_host(d_cov, (cs.G * cs.S, cs.n, cs.n), np.float64),
                         np.full((cs.G * cs.S, cs.n, cs.n), SENTINEL))
    assert ctx.lib.blsq_varpro_reduce_global_dev(None, *([0] * 5), *([None] * 6), 0, *([None] * 7)) == -1
    rc, out = reduce_global(ctx, cs)              # and the context is still good
    assert rc == 0 and not np.isnan(out["f"]).any()


def reduce_global_rc_only(ctx, cs, **over):
    """The return code of an entry call whose sizes do not fit the case's buffers: it must refuse before any launch, and
    every pointer it is given is a valid device buffer of the case all the same."""
    a = dict(G=cs.G, S=cs.S, m=cs.m, n=cs.n, nl=cs.nl, lin=cs.lin, owner=cs.owner, shared=cs.shared, w_stride=0)
    a.update(over)
    lin, p_lin = me.i32(a["lin"])
    owner, p_owner = me.i32(a["owner"])
    shared, p_shared = me.i32(a["shared"])
    with me.Dev(ctx) as d:
        d_f = d.up(np.full((cs.G, cs.S * cs.m), SENTINEL))
        rc = ctx.lib.blsq_varpro_reduce_global_dev(ctx.h, a["G"], a["S"], a["m"], a["n"], a["nl"], p_lin, p_owner,
                                                   p_shared, d.up(cs.Graw), d.up(cs.y), None, 0, d_f, None, None, None,
                                                   None, None, None)
        ctx.sync()
        assert same_bits(ctx.to_host(d_f, (cs.G, cs.S * cs.m), np.float64), np.full((cs.G, cs.S * cs.m), SENTINEL))
    return rc


# ---- Sinv and TD against np.longdouble, the covariance blocks against the definition -------------------------------------
def vetted_group(shape, wform, as_sets):
    """A vetted case of tests/_separable_cases.py (B = 3 data sets) as one group of three data sets or three groups of
    one, with random shared flags -> an object ``reduce_global`` takes."""
    cs = sc.case(*shape)
    g = object.__new__(gc.GroupCase)
    G, S = (1, sc.B) if as_sets else (sc.B, 1)
    rng = np.random.default_rng(cs.m)
    nsh = max(1, cs.na // 2)                       # (nv = nsh + S (na - nsh) <= 3 * 61 < 256)
    pos = np.sort(rng.choice(cs.na, nsh, replace=False))
    shared = np.zeros(cs.n, dtype=np.int32)
    shared[cs.non[pos]] = 1
    gm = bounded_lsq.GlobalMap(cs.na, S, pos)
    g.__dict__.update(m=cs.m, nl=cs.nl, na=cs.na, n=cs.n, S=S, G=G, lin=cs.lin, owner=cs.owner, non=cs.non, shared=shared,
                      gm=gm, nv=gm.nv, Graw=cs.G, y=cs.y, ws=cs.ws, X=None)
    return cs, g


def full_fractions(ctx, shape, wform):
    cs, g = vetted_group(shape, wform, as_sets=(shape[0] % 2 == 1))
    ref = gc.reference_full(*shape[:3], wform, *shape[3:])
    rc, out = reduce_global(ctx, g, wform, want=("Sinv", "TD", "c", "info"))
    assert rc == 0 and out["info"].tolist() == [0] * sc.B
    frac = gc.fractions_full(cs, wform, ref, out["Sinv"], out["TD"])
    print(shape, wform, "kappa %.3g" % cs.kappa(wform).max(), frac)
    return frac


@pytest.mark.parametrize("wform", sc.WFORMS)
@pytest.mark.parametrize("shape", sc.GRID + (sc.ILL + (True,),), ids=str)
def test_sinv_against_longdouble(ctx, shape, wform):
    frac = full_fractions(ctx, shape, wform)["Sinv"]
    worst["Sinv"] = max(worst.get("Sinv", 0.0), frac)
    assert frac <= 1.0


@pytest.mark.parametrize("wform", sc.WFORMS)
@pytest.mark.parametrize("shape", sc.GRID + (sc.ILL + (True,),), ids=str)
def test_td_against_longdouble(ctx, shape, wform):
    """The ill-conditioned case (kappa = 2e5) is what the extra correction of TD in double-double arithmetic is for:
    without it the kernel is at 31 to 57 times the cap there (tests/_separable_global_cases.py)."""
    frac = full_fractions(ctx, shape, wform)["TD"]
    worst["TD"] = max(worst.get("TD", 0.0), frac)
    assert frac <= 1.0


@pytest.mark.parametrize("G", gc.GROUPS)
@pytest.mark.parametrize("shape", gc.GRID, ids=str)
def test_cov_blocks_against_the_definition(ctx, shape, G):
    cs = gc.group_case(*shape, G)
    rc, out = reduce_global(ctx, cs, "per_problem", want=("Sinv", "TD", "info"))
    assert rc == 0
    rng = np.random.default_rng(cs.nv)
    A = rng.standard_normal((G, cs.nv + 3, cs.nv))
    C = np.einsum("gik,gil->gkl", A, A) / (cs.nv + 3)          # a covariance: symmetric positive definite
    C = np.triu(C) + np.swapaxes(np.triu(C, 1), 1, 2)
    scale = rng.uniform(0.5, 2.0, G)
    lin, p_lin = me.i32(cs.lin)
    shared, p_shared = me.i32(cs.shared)
    GS, n = G * cs.S, cs.n
    info = np.zeros(GS, dtype=np.int32)
    info[GS - 1] = 1
    status = np.zeros(G, dtype=np.int32)
    with me.Dev(ctx) as d:
        d_C, d_S, d_T, d_cov = d.up(C), d.up(out["Sinv"]), d.up(out["TD"]), d.up(np.full((GS, n, n), SENTINEL))
        head = (ctx.h, G, cs.S, n, cs.nl, p_lin, p_shared, d_C, d_S, d_T)
        assert ctx.lib.blsq_varpro_cov_blocks_dev(*head, d.up(scale), None, None, d_cov) == 0
        cov = ctx.to_host(d_cov, (G, cs.S, n, n), np.float64)
        assert ctx.lib.blsq_varpro_cov_blocks_dev(*head, None, d.up(info), d.up(status), d_cov) == 0
        flagged = ctx.to_host(d_cov, (GS, n, n), np.float64)
        status[0] = 3
        assert ctx.lib.blsq_varpro_cov_blocks_dev(*head, None, None, d.up(status), d_cov) == 0
        failed = ctx.to_host(d_cov, (G, cs.S, n, n), np.float64)
    Sinv, TD = out["Sinv"].reshape(G, cs.S, cs.nl, cs.nl), out["TD"].reshape(G, cs.S, cs.nl, cs.na)
    want = models.separable_global_cov(C.astype(gc.LD), Sinv.astype(gc.LD), TD.astype(gc.LD), cs.gm, scale.astype(gc.LD),
                                       cs.lin)
    bound = gc.cov_bound(C, Sinv, TD, cs.gm, cs.lin, scale)
    frac = float(np.max(np.abs(cov.astype(gc.LD) - want) / np.where(bound > 0, bound, 1.0)))
    worst["cov"] = max(worst.get("cov", 0.0), frac)
    print(shape, G, "cov-blocks: worst fraction of the summation bound %.3g" % frac)
    assert np.all(np.abs(cov.astype(gc.LD) - want) <= bound)
    assert same_bits(cov, np.swapaxes(cov, 2, 3))              # exactly symmetric
    assert np.isnan(flagged[GS - 1]).all() and not np.isnan(flagged[:GS - 1]).any()
    plain = models.separable_global_cov(C, Sinv, TD, cs.gm, None, cs.lin).reshape(GS, n, n)
    assert np.all(np.abs(flagged[:GS - 1] - plain[:GS - 1]) <= gc.cov_bound(C, Sinv, TD, cs.gm, cs.lin, None).reshape(
        GS, n, n)[:GS - 1])
    assert np.isnan(failed[0]).all() and not np.isnan(failed[1:]).any()


def test_worst_fractions_of_the_caps(ctx):
    """Runs last among the kernel tests: the figures DESIGN.md 7x records."""
    print("worst fractions (TD: 32 kappa eps, Sinv: 32 kappa^2 eps, cov: the summation bound):", worst)
    assert worst and max(worst.values()) <= 1.0


# ---- the device stage ------------------------------------------------------------------------------------------------
def test_device_model_stage_matches_the_definition(ctx):
    spec, n, shared, x, P, Y, sigma, p0, _ = gc.fit_data("local")
    G, S, m = Y.shape
    gm, lin, owner, non = models.separable_global_map(spec, n, S, shared)
    X = np.ascontiguousarray(gm.reduce_x(p0[..., non]))
    from bounded_lsq._varpro import _HostGlobalStage
    f_r, J_r, c_r, info_r, Sinv_r, TD_r = _HostGlobalStage(spec, Y, shared, sigma, n)(x, X)
    with models.DeviceModel(ctx, spec, G, m, n, x, Y, sigma, separable=True, global_map=gm) as dm, me.Dev(ctx) as d:
        assert (dm.B, dm.m, dm.n, dm.n_model) == (G, S * m, gm.nv, n)
        d_X, d_f, d_J = d.up(X), d.up(np.full((G, S * m), SENTINEL)), d.up(np.full((G, S * m, gm.nv), SENTINEL))
        dm.fun_dev(d_X, d_f, 1)
        dm.jac_dev(d_X, d_J, None)
        c, info = dm.linear_coefficients(d_X, with_info=True)
        f, J = ctx.to_host(d_f, (G, S * m), np.float64), ctx.to_host(d_J, (G, S * m, gm.nv), np.float64)
        C = np.linalg.inv(np.einsum("gik,gil->gkl", J_r, J_r))
        cov, c2, _ = dm.covariance_blocks(d_X, d.up(C), np.full(G, 2.0))
        with pytest.raises(ValueError, match="reps must be 1"):
            dm.fun_dev(d_X, d_f, 2)
    np.testing.assert_allclose(f, f_r, rtol=0, atol=1e-12)
    np.testing.assert_allclose(J, J_r, rtol=0, atol=1e-10)
    assert np.all(me.bits(J)[J_r == 0] == 0)
    np.testing.assert_allclose(c, c_r, rtol=1e-11, atol=1e-12)
    assert same_bits(c, c2) and not info.any()
    np.testing.assert_allclose(cov, models.separable_global_cov(C, Sinv_r, TD_r, gm, np.full(G, 2.0), lin), rtol=1e-9,
                               atol=1e-14)
    with pytest.raises(ValueError, match="GlobalMap over the 2 non-linear parameters"):
        models.DeviceModel(ctx, spec, G, m, n, x, Y, separable=True, global_map=bounded_lsq.GlobalMap(n, S, shared))


# ---- whole fits ------------------------------------------------------------------------------------------------------
def fit(name, separable, **kw):
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_global(spec, x, Y, p0_sep if separable else p0, shared, sigma=sigma, **gc.TOLS,
                                            **({"separable": True} if separable else {}), **kw)


@pytest.fixture(scope="module")
def plain():
    """The plain (dense) global fit per (name, method): computed once, shared, left unchanged."""
    cache = {}

    def get(name, method="trf", **kw):
        key = (name, method, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = fit(name, False, method=method, driver="device", **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", ["exp", "gauss", "local"])
def test_separable_global_fit_agrees_with_the_dense_route(plain, name, method):
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data(name)
    G, S, m = Y.shape
    ref = plain(name, method)
    assert ref[2][0].x.shape == (bounded_lsq.GlobalMap(n, S, shared).nv,) and all(r.success for r in ref[2])
    dev = fit(name, True, method=method, driver="device")
    host = fit(name, True, method=method, driver="host")
    assert all(r.success for r in dev[2]) and all(r.success for r in host[2])
    gc.agree_with_reference(ref, dev, (name, method, "device against dense"))
    gc.agree_with_reference(ref, host, (name, method, "host against dense"))
    gc.agree_with_reference(dev, host, (name, method, "host against device"))
    gm, lin, owner, non = models.separable_global_map(spec, n, S, shared)
    for g, r in enumerate(dev[2]):
        assert r.x.shape == (gm.nv,) and r.x_covariance.shape == (gm.nv, gm.nv)
        assert r.popt.shape == (S, n) and np.array_equal(r.popt, dev[0][g])
        assert r.linear_coefficients.shape == (S, lin.size) and np.array_equal(r.linear_coefficients, r.popt[:, lin])
        assert r.linear_params.tolist() == lin.tolist() and r.global_map.nv == gm.nv
        assert r.fun.shape == (S * m,) and r.jac.shape == (S * m, gm.nv)
        for s in range(S):                        # the reduced covariance IS the alpha-alpha block of the full one
            np.testing.assert_array_equal(dev[1][g, s][np.ix_(non, non)], r.x_covariance[np.ix_(gm.cols[s], gm.cols[s])])
        for j in shared:
            assert np.all(dev[0][g, :, j] == dev[0][g, 0, j])


def test_absolute_sigma_and_bounds(plain):
    name = "local"
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data(name)
    ref = plain(name, absolute_sigma=True)
    out = fit(name, True, driver="device", absolute_sigma=True)
    gc.agree_with_reference(ref, out, "absolute_sigma")
    lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    lb[2] = 0.43                                  # the shared width (0.4, started at 0.45) is held at its bound
    ref = fit(name, False, driver="device", method="dogbox", bounds=(lb, ub))
    out = fit(name, True, driver="device", method="dogbox", bounds=(lb, ub))
    assert all(r.success for r in out[2]) and np.all(out[0][..., 2] == 0.43)
    np.testing.assert_allclose(out[0], ref[0], rtol=1e-6, atol=1e-9)


def test_large_S_fits_where_the_dense_route_cannot(ctx):
    name = "large"
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data(name)
    G, S, m = Y.shape
    assert (G, S, m) == (2, 300, 16)
    with pytest.raises(ValueError, match=r"nv = ns \+ S nl = 2 \+ 300 \* 3 = 902 variables, more than 256"):
        bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, driver="device")
    popt, pcov, res = fit(name, True, driver="device")
    assert all(r.success for r in res) and res[0].x.shape == (2,) and res[0].jac.shape == (S * m, 2)
    which = [0, 149, 299]
    for g in range(G):
        ref, sres = gc.scipy_reference(name, g)
        assert sres.success
        np.testing.assert_allclose(popt[g], ref, rtol=1e-6, atol=1e-9)
        blocks = gc.full_blocks(name, g, popt[g], which)
        d = np.sqrt(np.einsum("sii->si", blocks))
        norm = d[:, :, None] * d[:, None, :]
        np.testing.assert_allclose(pcov[g, which] / norm, blocks / norm, rtol=0, atol=1e-6)
    host = fit(name, True, driver="host")
    gc.agree_with_reference((popt, pcov), host, "large S, host against device")


def test_routes_are_isolated(ctx, monkeypatch):
    new = ("blsq_varpro_expand_global_dev", "blsq_varpro_reduce_global_dev", "blsq_varpro_cov_blocks_dev")
    old = ("blsq_varpro_expand_dev", "blsq_varpro_reduce_dev", "blsq_model_eval_global_dev")
    counts = me.count_entries(ctx, monkeypatch, new + old)
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data("exp")

    def no_numpy(*a, **k):
        raise AssertionError("the device route reached a numpy model function")
    M = models.resolve(spec)
    with monkeypatch.context() as mp:
        for fn in ("f", "jac"):
            mp.setattr(type(M), fn, no_numpy)
        mp.setattr(models, "varpro_reduce", no_numpy)
        mp.setattr(bounded_lsq._varpro, "_reduce_full", no_numpy)
        out = bounded_lsq.curve_fit_global(spec, x, Y, p0_sep, shared, driver="device", separable=True, ctx=ctx, **gc.TOLS)
    assert all(r.success for r in out[2])
    assert counts["blsq_varpro_reduce_global_dev"] > 0 and counts["blsq_varpro_cov_blocks_dev"] == 1
    assert counts["blsq_varpro_expand_global_dev"] == counts["blsq_varpro_reduce_global_dev"]
    assert [counts[k] for k in old] == [0, 0, 0]
    for k in counts:
        counts[k] = 0
    bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, driver="device", ctx=ctx, **gc.TOLS)
    G, S, m = Y.shape
    bounded_lsq.curve_fit_batch(spec, x, Y[0], p0_sep[0], driver="device", separable=True, ctx=ctx, **gc.TOLS)
    assert [counts[k] for k in new] == [0, 0, 0]
    assert counts["blsq_model_eval_global_dev"] > 0 and counts["blsq_varpro_reduce_dev"] > 0


def test_separable_false_is_the_default_path():
    spec, n, shared, x, P, Y, sigma, p0, p0_sep = gc.fit_data("gauss")
    for driver in ("device", "host"):
        a = bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, driver=driver, **gc.TOLS)
        b = bounded_lsq.curve_fit_global(spec, x, Y, p0, shared, driver=driver, separable=False, **gc.TOLS)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for r, q in zip(a[2], b[2]):
            assert np.array_equal(r.fun, q.fun) and r.nfev == q.nfev and not hasattr(r, "linear_coefficients")
