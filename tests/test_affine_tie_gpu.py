"""Affine ties on the GPU: blsq_model_eval_tie_dev bit for bit against ``ParamMap`` / ``GlobalMap`` applied
to the output of blsq_model_eval_nan_dev without a map, and the doublet fits of tests/_affine_tie_cases.py across their
routes against the independent scipy reference.

The exact reference.  f is the f of blsq_model_eval_nan_dev (no map) at ``expand_x(X, Pfix)``.  Under BLSQ_EST_LSE J is
``reduce_jac`` of that entry's J (for S >= 1 scattered by ``GlobalMap.reduce_jac``).  Under BLSQ_EST_POISSON the kernel
multiplies a slot by c = dr / dmu AFTER its sum, as it does for a plain map (include/blsq.h: "the columns are summed
first and the slot is multiplied by c"), so ``reduce_jac`` of the unmapped Poisson J, which sums columns that each
carry c already, is not the same bits where a slot has several members.  The exact reference there is c times
``reduce_jac`` of the unweighted columns, every factor in the device's own bits: the columns from the unmapped
least-squares instance with w = NULL, and c from the unmapped Poisson instance of 'poly' with n = 1 evaluated at the
model value (its one column is c * 1.0).  The unmapped Poisson J, reduced, is checked too: to 8 eps of the sum of the
magnitudes of a slot's terms (two roundings per term and their sum)."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import GlobalMap, ParamMap, models

import _affine_tie_cases as ac
import _model_eval as me
from _model_eval import bits, ctx, same_bits  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

LSE, POISSON = 0, 1                                      # BLSQ_EST_*
POINT, BIN = 0, 1                                        # BLSQ_SAMPLE_*
PROPAGATE, OMIT = 0, 1                                   # BLSQ_NAN_*
FLAGS = [(LSE, PROPAGATE), (LSE, OMIT), (POISSON, PROPAGATE), (POISSON, OMIT)]
SENTINEL = -77.25
EPS = np.finfo(float).eps


def rows_of(case, sampling):
    """t as rows per abscissa set: (..., rows, m) with rows = coords (points) or 2 coords (bins lo, hi per coordinate)."""
    t = case["t"] if case["coords"] == 2 else case["t"][..., None, :]
    if sampling == POINT:
        return t
    lo, hi = t - 0.04, t + 0.05
    return np.stack([lo, hi], axis=-2).reshape(t.shape[:-2] + (2 * case["coords"], case["m"]))


def maps(case):
    pm = ParamMap(case["n"], case["fixed"], case["tied"])
    gm = GlobalMap(case["n"], case["S"], case["shared"], case["fixed"], case["tied"]) if case["S"] else None
    return pm, gm


def points(case, reps, seed=1):
    """X (B reps, nv): the case's parameters reduced, every further rep a perturbed copy."""
    pm, gm = maps(case)
    X0 = gm.reduce_x(case["P"]) if gm is not None else pm.reduce_x(case["P"][:, 0])
    X = np.repeat(X0[:, None, :], reps, axis=1)
    rng = np.random.default_rng(seed)
    X[:, 1:] *= 1.0 + 0.01 * rng.uniform(-1.0, 1.0, X[:, 1:].shape)
    return np.ascontiguousarray(X.reshape(-1, X.shape[-1]))


ENTRIES = {"tie": "blsq_model_eval_tie_dev", "global": "blsq_model_eval_global_dev", "nan": "blsq_model_eval_nan_dev",
           "map": "blsq_model_eval_map_dev"}


def run_tie(ctx, case, est, policy, reps, X, sampling=POINT, want_f=True, want_J=False, mask=None, fill=np.nan,
            ties="map", entry="tie", **bad):
    """blsq_model_eval_tie_dev on the case -> (rc, f, J).  ties: 'map' (the map's ratio and offset), 'null' (both NULL).
    entry: 'tie', or 'global' / 'nan' / 'map' for the existing entry with the same arguments less the tie pair (and,
    for 'nan' / 'map', the run of S).  Under POISSON w is NULL; y holds NaN at the omitted points under OMIT only.
    `bad` overrides arguments by name (G: the header's name of B)."""
    pm, gm = maps(case)
    B, S, m, n = case["B"], case["S"], case["m"], case["n"]
    Se = max(S, 1)
    w = None if est == POISSON else case["w"]
    t = rows_of(case, sampling)
    rows = t.shape[-2]
    if S:
        tg, ts = {2: (0, 0), 3: (0, m), 4: (S * m, m)}[t.ndim]
    else:
        tg, ts = (rows * m if t.ndim == 4 else 0), 0
    nv = gm.nv if gm is not None else pm.nf
    a = dict(est=est, sampling=sampling, nan_policy=policy, **me.model_args(models.resolve(case["spec"])), S=S,
             shared=gm.slot_shared if gm is not None else None, t_sstride=ts, B=B, reps=reps, m=m, n=n, nf=pm.nf,
             pmap=pm.pmap, tie_ratio=pm.ratio if ties == "map" else None,
             tie_offset=pm.offset if ties == "map" else None, t=t, t_stride=tg,
             y=np.where(case["omitted"], np.nan, case["y"]) if policy == OMIT else case["y"], w=w,
             w_stride=0 if w is None or w.ndim == 1 else Se * m, X=X, Pfix=case["P"], mask=mask)
    if "G" in bad:
        bad["B"] = bad.pop("G")
    a.update(bad)
    return me.run(ctx, ENTRIES[entry], (B * reps, Se * m), (B, Se * m, nv), want_f, want_J, fill, strict=entry == "tie",
                  **a)


def unmapped(ctx, M, est, sampling, policy, Bt, reps, m, n, t, t_stride, y, w, w_stride, P, want_J):
    """blsq_model_eval_nan_dev without a map on Bt problems -> f (Bt reps, m), J (Bt, m, n) or None."""
    rc, f, J = me.run(ctx, "blsq_model_eval_nan_dev", (Bt * reps, m), (Bt, m, n), True, want_J, strict=True, est=est,
                      sampling=sampling, nan_policy=policy, **me.model_args(M), B=Bt, reps=reps, m=m, n=n, nf=n, pmap=None,
                      t=t, t_stride=t_stride, y=y, w=w, w_stride=w_stride, X=P, Pfix=None, mask=None)
    assert rc == 0, rc
    return f, J


def reference(ctx, case, est, policy, reps, X, sampling=POINT, want_J=False):
    """(f, J, J_literal): the exact reference of the module docstring; J_literal is ``reduce_jac`` of the unmapped
    entry's own J and its bound (under LSE: J itself, bound 0)."""
    pm, gm = maps(case)
    M = models.resolve(case["spec"])
    B, S, m, n = case["B"], case["S"], case["m"], case["n"]
    Se, Bt = max(S, 1), case["B"] * max(S, 1)
    y = (np.where(case["omitted"], np.nan, case["y"]) if policy == OMIT else case["y"]).reshape(Bt, m)
    w = None if est == POISSON else case["w"]
    w_stride = 0
    if w is not None and w.ndim > 1:
        w, w_stride = w.reshape(Bt, m), m
    t = rows_of(case, sampling)
    rows = t.shape[-2]
    t_stride = 0
    if t.ndim > 2:
        t, t_stride = np.broadcast_to(t, (B, Se, rows, m)).reshape(Bt, rows * m), rows * m
    Xr = X.reshape(B, reps, -1)
    if gm is not None:                                      # (B, reps, S, n) -> problem (b, s), rep r
        Pf = gm.expand_x(Xr, case["P"][:, None]).transpose(0, 2, 1, 3)
    else:
        Pf = pm.expand_x(Xr, case["P"][:, 0][:, None, :])[:, None]
    Pf = np.ascontiguousarray(Pf.reshape(Bt * reps, n))
    f, Jl = unmapped(ctx, M, est, sampling, policy, Bt, reps, m, n, t, t_stride, y, w, w_stride, Pf, want_J)
    f = np.ascontiguousarray(f.reshape(B, Se, reps, m).transpose(0, 2, 1, 3)).reshape(B * reps, Se * m)
    if not want_J:
        return f, None, None
    scatter = GlobalMap(pm.nf, S, np.flatnonzero(gm.slot_shared)) if gm is not None else None

    def shape(Jr):                                          # (Bt, m, nf) -> the entry's J
        return scatter.reduce_jac(Jr.reshape(B, S, m, pm.nf)) if scatter is not None else Jr
    literal = shape(pm.reduce_jac(Jl))
    if est == LSE:
        return f, literal, (literal, np.zeros_like(literal))
    bound = 8 * EPS * shape(ParamMap(n, case["fixed"], ac.plain(case["tied"])).reduce_jac(np.abs(Jl * pm.ratio)))
    v, cols = unmapped(ctx, M, LSE, sampling, PROPAGATE, Bt, 1, m, n, t, t_stride, None, None, 0, Pf, True)
    poly = models.resolve("poly")
    yc = np.where(np.isnan(y), 1.0, y).reshape(Bt * m, 1)
    _, c = unmapped(ctx, poly, POISSON, POINT, PROPAGATE, Bt * m, 1, 1, 1, np.zeros(1), 0, yc, None, 0,
                    np.ascontiguousarray(v.reshape(Bt * m, 1)), True)
    Jr = c.reshape(Bt, m, 1) * pm.reduce_jac(cols)
    Jr[np.isnan(y)] = 0.0                                   # (NaN in y under OMIT only)
    return f, shape(Jr), (literal, bound)


# ---- the kernel: exact -----------------------------------------------------------------------------------------------
def check_kernel(ctx, case, est, policy, sampling):
    X = points(case, 1)
    rc, f, J = run_tie(ctx, case, est, policy, 1, X, sampling, want_f=True, want_J=True)
    assert rc == 0
    f_ref, J_ref, (lit, bound) = reference(ctx, case, est, policy, 1, X, sampling, want_J=True)
    assert same_bits(f, f_ref)
    assert same_bits(J, J_ref)
    assert np.all(np.abs(J - lit) <= bound)
    assert np.isfinite(J).all() and np.isfinite(f).all()
    if policy == OMIT and case["omitted"].any():            # an omitted row: zeros in f and in every column
        om = case["omitted"].reshape(case["B"], -1)
        assert not bits(f[om]).any() and not bits(J[om]).any()
    X3 = points(case, 3)
    rc, f3, _ = run_tie(ctx, case, est, policy, 3, X3, sampling)
    assert rc == 0
    assert same_bits(f3, reference(ctx, case, est, policy, 3, X3, sampling)[0])
    assert same_bits(f3[0::3], f)                           # rep 0 is the point above


@pytest.mark.parametrize("est, policy", FLAGS)
@pytest.mark.parametrize("label", list(ac.KERNEL_CASES))
def test_kernel_is_the_map_of_the_unmapped_entry(ctx, label, est, policy):
    """f and J (reps 1) and f (reps 3) of the new entry, bit for bit against the reference of the module docstring, over
    m in {1, 63, 64, 65, 130}, B in {1, 3}, S in {0, 1, 2, 3}, the three forms of t and of w and every map of the list."""
    check_kernel(ctx, ac.kernel_case(label), est, policy, POINT)


@pytest.mark.parametrize("est, policy", FLAGS)
@pytest.mark.parametrize("label", [k for k, v in ac.KERNEL_CASES.items() if v[5] == 0])
def test_binned_kernel_is_the_map_of_the_unmapped_entry(ctx, label, est, policy):
    """The same with BLSQ_SAMPLE_BIN for the plain batches (S = 0), gauss2d's pixels included."""
    check_kernel(ctx, ac.kernel_case(label), est, policy, BIN)


def test_the_cases_cover_what_they_are_there_for():
    cs = ac.KERNEL_CASES.values()
    assert {c[7] for c in cs} == {1, 63, 64, 65, 130} and {c[6] for c in cs} == {1, 3} and {c[5] for c in cs} == {0, 1, 2, 3}
    assert {c[8] for c in cs} == {"shared", "set", "group"} and {c[9] for c in cs} == {None, "shared", "group"}
    nf = {k: ParamMap(c[1], c[2], c[3]).nf for k, c in ac.KERNEL_CASES.items()}
    assert nf["big_odd"] == 63 and nf["big_even"] == 62
    pm = ParamMap(10, None, ac.KERNEL_CASES["three_ratios"][3])
    assert len(set(pm.ratio[pm.group(0)])) == 3


@pytest.mark.parametrize("label", ac.TRIVIAL_CASES)
def test_trivial_ties_give_the_bits_of_the_existing_entries(ctx, label):
    """All ties (i, 1, 0): with the pair given and with both NULL the entry gives the bits of blsq_model_eval_map_dev
    (S = 0; a composite: blsq_model_eval_nan_dev with the pmap, which a composite's map goes through) and of
    blsq_model_eval_global_dev (S >= 1)."""
    case = ac.kernel_case(label, trivial_ties=True)
    assert not maps(case)[0].affine
    X = points(case, 1)
    comp = isinstance(models.resolve(case["spec"]), models.CompositeModel)
    entry = "global" if case["S"] else ("nan" if comp else "map")
    rc0, f0, J0 = run_tie(ctx, case, LSE, PROPAGATE, 1, X, want_f=True, want_J=True, entry=entry)
    assert rc0 == 0
    for ties in ("map", "null"):
        rc, f, J = run_tie(ctx, case, LSE, PROPAGATE, 1, X, want_f=True, want_J=True, ties=ties)
        assert rc == 0 and same_bits(f, f0) and same_bits(J, J0)
    if entry != "map":                                      # ... and under the other flags
        rc0, f0, J0 = run_tie(ctx, case, POISSON, OMIT, 1, X, want_f=True, want_J=True, entry=entry)
        rc, f, J = run_tie(ctx, case, POISSON, OMIT, 1, X, want_f=True, want_J=True)
        assert rc0 == 0 and rc == 0 and same_bits(f, f0) and same_bits(J, J0)


def test_minus_zero_passes_a_trivial_member_unchanged(ctx):
    """x = -0.0 in a slot with a trivial and an affine member: the residual is that of the unmapped entry at
    expand_x, whose trivial member is -0.0 and whose affine member is r * -0.0 + d."""
    case = ac.kernel_case("negative")
    pm, _ = maps(case)
    X = points(case, 1)
    X[:, 1] = -0.0                                          # mu1; mu2 = -1.0 * mu1 + 0.0 = +0.0
    Pf = pm.expand_x(X, case["P"][:, 0])
    assert np.signbit(Pf[:, 1]).all() and not np.signbit(Pf[:, 4]).any()
    rc, f, J = run_tie(ctx, case, LSE, PROPAGATE, 1, X, want_f=True, want_J=True)
    f_ref, J_ref, _ = reference(ctx, case, LSE, PROPAGATE, 1, X, want_J=True)
    assert rc == 0 and same_bits(f, f_ref) and same_bits(J, J_ref)


@pytest.mark.parametrize("label, est, policy", [("doublet", LSE, PROPAGATE), ("doublet_s2", POISSON, OMIT)])
def test_a_masked_problem_keeps_its_sentinel(ctx, label, est, policy):
    case = ac.kernel_case(label)
    X = points(case, 1)
    rc, f, J = run_tie(ctx, case, est, policy, 1, X, want_f=True, want_J=True, mask=[1, 0, 1], fill=SENTINEL)
    f_ref, J_ref, _ = reference(ctx, case, est, policy, 1, X, want_J=True)
    assert rc == 0
    assert np.all(f[1] == SENTINEL) and np.all(J[1] == SENTINEL)
    for b in (0, 2):
        assert same_bits(f[b], f_ref[b]) and same_bits(J[b], J_ref[b])


def test_bad_arguments_return_their_positions(ctx):
    """Every refusal by the position of its argument (ctx = 1); nothing is launched."""
    case = ac.kernel_case("doublet_s2")
    pm, gm = maps(case)
    X = points(case, 1)
    n, nf, S, m = case["n"], pm.nf, case["S"], case["m"]

    def rc(reps=1, want_f=True, want_J=False, est=LSE, **bad):
        return run_tie(ctx, case, est, PROPAGATE, reps, bad.pop("X", X), want_f=want_f, want_J=want_J, **bad)[0]
    assert rc() == 0
    assert rc(est=2) == -2
    assert rc(sampling=1) == -3                             # BLSQ_SAMPLE_BIN with S >= 1
    assert rc(sampling=2) == -3
    assert rc(nan_policy=2) == -4
    assert rc(model=5) == -5
    assert rc(model=4, ncomp=0) == -5                       # gauss2d with S >= 1
    assert rc(ncomp=0) == -6 and rc(ncomp=9) == -6
    assert rc(fam=None) == -7 and rc(cnt=None) == -8
    assert rc(S=-1) == -9
    assert (gm.ns, gm.nl) == (2, 2) and rc(S=128) == -9     # nv = 2 + 128 * 2 = 258 > BLSQ_GLOBAL_MAX_NV
    assert rc(shared=None) == -10
    assert rc(shared=[2] + [0] * (nf - 1)) == -10
    assert rc(t_sstride=m + 1) == -11
    assert rc(G=0) == -12 and rc(reps=0) == -13 and rc(m=0) == -14 and rc(n=n + 1) == -15
    assert rc(nf=0) == -16 and rc(nf=n + 1) == -16
    assert rc(pmap=None) == -17
    assert rc(tie_ratio=None) == -18 and rc(tie_offset=None) == -19     # exactly one NULL: the NULL one
    assert rc(t=None) == -20 and rc(t_stride=7) == -21
    assert rc(est=POISSON, y=None) == -22
    assert rc(nan_policy=OMIT, y=None) == -22
    assert rc(w_stride=m) == -24                            # per group is S m
    assert rc(X=None) == -25
    assert rc(want_f=False) == -27
    assert rc(reps=3, want_J=True) == -28
    p = pm.pmap.copy()
    p[0] = nf
    assert rc(pmap=p) == -30
    p = pm.pmap.copy()
    p[p == nf - 1] = 0
    assert rc(pmap=p) == -31
    for bad_ratio in (0.0, -0.0, np.inf, -np.inf, np.nan):
        r = pm.ratio.copy()
        r[3] = bad_ratio
        assert rc(tie_ratio=r) == -32
    for bad_offset in (np.inf, -np.inf, np.nan):
        o = pm.offset.copy()
        o[4] = bad_offset
        assert rc(tie_offset=o) == -33
    # S == 0: a plain batch; shared is ignored, t_sstride must be 0; entries at fixed parameters are not read
    case = ac.kernel_case("fixed_next")
    pm, _ = maps(case)
    X = points(case, 1)

    def rc0(**bad):
        return run_tie(ctx, case, LSE, PROPAGATE, 1, X, **bad)[0]
    assert rc0() == 0 and rc0(shared=[7, 7, 7]) == 0
    assert rc0(t_sstride=case["m"]) == -11
    assert rc0(Pfix=None) == -26
    r, o = pm.ratio.copy(), pm.offset.copy()
    r[2], o[6] = 0.0, np.nan                                # parameters 2 and 6 are fixed
    assert rc0(tie_ratio=r, tie_offset=o) == 0
    r[3] = np.nan
    assert rc0(tie_ratio=r) == -32


# ---- fits ------------------------------------------------------------------------------------------------------------
def fit(ctx, case, driver, method="trf", tied=None, **kw):
    lb, ub = case["bounds"]
    tied = case["tied"] if tied is None else tied
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if case["shared"] is not None:
            return bounded_lsq.curve_fit_global(case["spec"], case["x"], case["Y"], case["P0"], case["shared"],
                                                bounds=(lb, ub), method=method, driver=driver, ctx=ctx, tied=tied,
                                                **dict(ac.TOL, **case["kw"], **kw))
        return bounded_lsq.curve_fit_batch(case["spec"], case["x"], case["Y"], case["P0"], bounds=(lb, ub),
                                           method=method, driver=driver, ctx=ctx, tied=tied,
                                           **dict(ac.TOL, **case["kw"], **kw))


@pytest.fixture(scope="module")
def worst():
    return {}


def against(popt, pcov, ref_popt, ref_pcov, what, worst):
    """popt rtol 1e-6 / atol 1e-9; pcov atol 1e-6 after normalising by the REFERENCE's standard deviations."""
    popt, pcov = np.asarray(popt).reshape(ref_popt.shape), np.asarray(pcov).reshape(ref_pcov.shape)
    d = np.sqrt(np.einsum("...ii->...i", ref_pcov))
    a = pcov / (d[..., :, None] * d[..., None, :])
    b = ref_pcov / (d[..., :, None] * d[..., None, :])
    ep = float(np.max(np.abs(popt - ref_popt) / (1e-9 + 1e-6 * np.abs(ref_popt))))
    ec = float(np.max(np.abs(a - b)) / 1e-6)
    worst[what] = (ep, ec)
    print("affine fit %-34s fraction of the popt margin %.3g   of the pcov margin %.3g" % (what, ep, ec))
    np.testing.assert_allclose(popt, ref_popt, rtol=1e-6, atol=1e-9, err_msg=str(what))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=str(what))


def ties_hold(popt, pcov):
    """The constraint in the results: exact for the copies and the power-of-two ratio, one rounding for the offset."""
    assert np.array_equal(popt[..., 3], ac.RATIO * popt[..., 0]) and np.array_equal(popt[..., 5], popt[..., 2])
    assert np.array_equal(popt[..., 4], popt[..., 1] + ac.SPLIT)
    assert np.array_equal(pcov[..., 3, 3], 0.25 * pcov[..., 0, 0])        # a dropped ratio in expand_cov fails here
    assert np.array_equal(pcov[..., 3, 1], ac.RATIO * pcov[..., 0, 1])
    assert np.array_equal(pcov[..., 4, 4], pcov[..., 1, 1]) and np.all(pcov[..., 0, 0] > 0)


@pytest.mark.parametrize("method", ["trf", "dogbox"])
def test_doublet_device_host_and_reference(ctx, method, worst):
    """B = 8 doublets, m = 80, mu2 = mu1 + 0.6, a2 = 0.5 a1, s2 = s1 (nf = 4 of n = 7): the device route against the host
    route, and both against scipy on the hand-written constrained residual."""
    case = ac.fit_case("lse")
    ref_popt, ref_pcov, _, ok = ac.reference("lse")
    assert ok
    D, H = fit(ctx, case, "device", method), fit(ctx, case, "host", method)
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    r = D[2][0]
    assert r.x.shape == (7,) and r.x_free.shape == (4,) and r.jac.shape == (80, 4) and r.x_covariance.shape == (7, 7)
    ties_hold(D[0], D[1])
    ties_hold(H[0], H[1])
    for b, r in enumerate(D[2]):
        assert np.array_equal(r.x, D[0][b])
    against(D[0], D[1], ref_popt, ref_pcov, ("lse", method, "device"), worst)
    against(H[0], H[1], ref_popt, ref_pcov, ("lse", method, "host"), worst)
    against(D[0], D[1], H[0], H[1], ("lse", method, "device-host"), worst)


@pytest.mark.parametrize("name", ["poisson", "omit", "bound", "global"])
def test_doublet_variants_against_the_reference(ctx, name, worst):
    """estimator='poisson' with absolute_sigma=True; nan_policy='omit' on padded data; a bound on mu2 alone that is
    active at the solution (the transformed box and the expanded mask); curve_fit_global with S = 3 and the width
    shared."""
    case = ac.fit_case(name)
    ref_popt, ref_pcov, _, ok = ac.reference(name)
    assert ok
    D, H = fit(ctx, case, "device"), fit(ctx, case, "host")
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    ties_hold(D[0], D[1])
    ties_hold(H[0], H[1])
    if name == "omit":
        assert [r.nobs for r in D[2]] == [72 + b for b in range(ac.B_FIT)]
    if name == "bound":
        ub4 = case["bounds"][1][:, 4]
        for R in (D, H):
            assert np.all(R[0][:, 4] <= ub4) and np.all(np.abs(R[0][:, 4] - ub4) <= 1e-9)
            for r in R[2]:
                assert list(r.active_mask) == [0, 1, 0, 0, 1, 0, 0]
    if name == "global":
        assert D[0].shape == (2, 3, 7) and np.all(D[0][:, :, 2] == D[0][:, :1, 2])
        assert D[2][0].x.shape == (10,)
    against(D[0], D[1], ref_popt, ref_pcov, (name, "device"), worst)
    against(H[0], H[1], ref_popt, ref_pcov, (name, "host"), worst)
    against(D[0], D[1], H[0], H[1], (name, "device-host"), worst)


def test_doublet_with_three_point_differences(ctx, worst):
    """jac='3-point': device finite differences over the nf variables, through fun_dev with reps."""
    case = ac.fit_case("lse")
    ref_popt, ref_pcov, _, _ = ac.reference("lse")
    D = fit(ctx, case, "device", jac="3-point")
    assert all(r.success for r in D[2])
    ties_hold(D[0], D[1])
    against(D[0], D[1], ref_popt, ref_pcov, ("lse", "3-point", "device"), worst)


def test_one_data_set_through_curve_fit(ctx, worst):
    """``curve_fit`` with a callable over all seven parameters and its Jacobian, through ParamMap's expansion."""
    case = ac.fit_case("single")
    ref_popt, ref_pcov, _, ok = ac.reference("single")
    assert ok
    M = models.compose(ac.DOUBLET)
    lb, ub = case["bounds"]
    popt, pcov = bounded_lsq.curve_fit(lambda t, *p: M.f(t, np.asarray(p)[None])[0], case["x"], case["Y"][0],
                                       p0=case["P0"][0], sigma=np.full(case["m"], 0.05), bounds=(lb[0], ub[0]),
                                       jac=lambda t, *p: M.jac(t, np.asarray(p)[None])[0], tied=case["tied"], **ac.TOL)
    ties_hold(popt, pcov)
    against(popt, pcov, ref_popt[0], ref_pcov[0], ("single", "curve_fit"), worst)


def test_device_route_goes_through_the_new_entry_alone(ctx, monkeypatch):
    """The device route reaches no numpy model function and no blsq_model_eval* entry but the new one; a fit without
    tuple ties does not reach the new entry."""
    from bounded_lsq import _models, _outer
    case = ac.fit_case("lse")
    before = fit(ctx, case, "device")

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    entries = me.count_entries(ctx, monkeypatch)
    got = fit(ctx, case, "device")
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1])
    assert set(entries) == {"blsq_model_eval_tie_dev"}
    entries.clear()
    fit(ctx, ac.fit_case("poisson"), "device")
    fit(ctx, ac.fit_case("omit"), "device", jac="2-point")
    fit(ctx, ac.fit_case("global"), "device")
    assert set(entries) == {"blsq_model_eval_tie_dev"}
    entries.clear()
    fit(ctx, case, "device", tied=ac.plain(case["tied"]))
    fit(ctx, case, "device", tied=ac.trivial(case["tied"]))
    assert set(entries) == {"blsq_model_eval_comp_dev"}
    entries.clear()
    fit(ctx, ac.fit_case("global"), "device", tied=ac.plain(case["tied"]))
    assert set(entries) == {"blsq_model_eval_global_dev"}
