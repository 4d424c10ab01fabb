"""Global fits on the GPU: blsq_model_eval_global_dev bit for bit against ``GlobalMap`` applied to the
output of blsq_model_eval_nan_dev on the G S data sets, and ``curve_fit_global`` across its routes against the
independent scipy reference of tests/_global_cases.py."""
import warnings

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import GlobalMap, models

import _global_cases as gc
import _model_eval as me
from _model_eval import bits, ctx, same_bits  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

LSE, POISSON = 0, 1                                      # BLSQ_EST_*
PROPAGATE, OMIT = 0, 1                                   # BLSQ_NAN_*
FLAGS = [(LSE, PROPAGATE), (LSE, OMIT), (POISSON, PROPAGATE), (POISSON, OMIT)]
SENTINEL = -77.25


def setup(case):
    """The map, the model and the data of a kernel case as both entries take them."""
    gm = GlobalMap(case["n"], case["S"], case["shared"], case["fixed"], case["tied"])
    M = models.resolve(case["spec"])
    G, S, m = case["G"], case["S"], case["m"]
    t = case["t"]
    strides = {1: (0, 0), 2: (0, m), 3: (S * m, m)}[t.ndim]                     # group stride, data-set stride
    return gm, M, G, S, m, t, strides


def run_global(ctx, case, est, policy, reps, X, want_f=True, want_J=False, mask=None, fill=np.nan, **bad):
    """blsq_model_eval_global_dev on the case -> (rc, f (G reps, S m) or None, J (G, S m, nv) or None).  Under POISSON w is
    NULL; under OMIT y holds NaN at the case's omitted points (under PROPAGATE as well: they pass through).  `bad`
    overrides arguments by name (G: the header's name of B)."""
    gm, M, G, S, m, t, (tg, ts) = setup(case)
    w = None if est == POISSON else case["w"]
    a = dict(est=est, sampling=0, nan_policy=policy, **me.model_args(M), S=S, shared=gm.slot_shared, t_sstride=ts, B=G,
             reps=reps, m=m, n=case["n"], nf=gm.nf, pmap=gm.pm.pmap, t=t, t_stride=tg,
             y=np.where(case["omitted"], np.nan, case["y"]), w=w, w_stride=0 if w is None or w.ndim == 1 else S * m, X=X,
             Pfix=case["P"], mask=mask)
    if "G" in bad:
        bad["B"] = bad.pop("G")
    a.update(bad)
    return me.run(ctx, "blsq_model_eval_global_dev", (G * reps, S * m), (G, S * m, gm.nv), want_f, want_J, fill,
                  strict=True, **a)


def run_sets(ctx, case, est, policy, reps, X, want_f=True, want_J=False, entry="nan"):
    """The reference: the G S data sets as G S problems of the existing entry (blsq_model_eval_nan_dev; entry='map':
    blsq_model_eval_map_dev) at expand_x(X), brought into the group's shape by reshape / ``GlobalMap.reduce_jac``."""
    gm, M, G, S, m, t, (tg, ts) = setup(case)
    B, nf = G * S, gm.nf
    w = None if est == POISSON else case["w"]
    if w is not None and w.ndim == 2:
        w = w.reshape(B, m)
    # the points of problem (g, s): its own nf variables of every rep
    Xs = gm.split_x(X.reshape(G, reps, gm.nv)).transpose(0, 2, 1, 3).reshape(B * reps, nf)
    rc, f, J = me.run(ctx, "blsq_model_eval_%s_dev" % entry, (B * reps, m), (B, m, nf), want_f, want_J, est=est,
                      sampling=0, nan_policy=policy, **me.model_args(M), B=B, reps=reps, m=m, n=case["n"], nf=nf,
                      pmap=gm.pm.pmap, t=t if t.ndim == 1 else np.broadcast_to(t, (G, S, m)).reshape(B, m),
                      t_stride=0 if t.ndim == 1 else m, y=np.where(case["omitted"], np.nan, case["y"]).reshape(B, m), w=w,
                      w_stride=0 if w is None or w.ndim == 1 else m, X=Xs, Pfix=case["P"].reshape(B, -1), mask=None)
    assert rc == 0, rc
    if want_f:
        f = np.ascontiguousarray(f.reshape(G, S, reps, m).transpose(0, 2, 1, 3)).reshape(G * reps, S * m)
    if want_J:                                              # a pure scatter: the identity map over the nf slots
        J = GlobalMap(nf, S, np.flatnonzero(gm.slot_shared)).reduce_jac(J.reshape(G, S, m, nf))
    return f, J


def points(case, reps, seed=1):
    """X (G reps, nv): the case's parameters reduced, every further rep a perturbed copy."""
    gm = GlobalMap(case["n"], case["S"], case["shared"], case["fixed"], case["tied"])
    X = np.repeat(gm.reduce_x(case["P"])[:, None, :], reps, axis=1)
    rng = np.random.default_rng(seed)
    X[:, 1:] *= 1.0 + 0.01 * rng.uniform(-1.0, 1.0, X[:, 1:].shape)
    return gm, np.ascontiguousarray(X.reshape(-1, gm.nv))


# ---- the kernel: exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est, policy", FLAGS)
@pytest.mark.parametrize("label", list(gc.KERNEL_CASES))
def test_kernel_is_the_map_of_the_existing_entry(ctx, label, est, policy):
    """f and J (reps 1) and f (reps 3) of the new entry, bit for bit: the existing entry on the G S data sets at
    expand_x(X), reshaped and scattered by ``GlobalMap.reduce_jac``; and every column outside a data set's own holds the
    all-zero bit pattern, also where the Poisson model value is negative (case poly_neg) and c is NaN."""
    case = gc.kernel_case(label)
    gm, X = points(case, 1)
    rc, f, J = run_global(ctx, case, est, policy, 1, X, want_f=True, want_J=True)
    assert rc == 0
    f_ref, J_ref = run_sets(ctx, case, est, policy, 1, X, want_f=True, want_J=True)
    assert same_bits(f, f_ref) and same_bits(J, J_ref)
    S, m = case["S"], case["m"]
    for s in range(S):
        other = np.setdiff1d(np.arange(gm.nv), gm.cols[s])
        assert not bits(J[:, s * m:(s + 1) * m][:, :, other]).any()
    if policy == OMIT:                                     # an omitted row: zeros in f and in all nv columns
        om = case["omitted"].reshape(case["G"], S * m)
        assert not bits(f[om]).any() and not bits(J[om]).any()
    if label == "poly_neg" and est == POISSON:             # (the case does what it is there for)
        assert np.isnan(J[:, m:2 * m][:, :, gm.cols[1]]).any()
    gm, X3 = points(case, 3)
    rc, f3, _ = run_global(ctx, case, est, policy, 3, X3)
    assert rc == 0
    assert same_bits(f3, run_sets(ctx, case, est, policy, 3, X3)[0])
    assert same_bits(f3[0::3], f)                          # rep 0 is the point above


def test_one_data_set_gives_the_bits_of_the_mapped_entry(ctx):
    """S = 1 with every slot shared: the outputs of blsq_model_eval_map_dev."""
    case = gc.kernel_case("one_set")
    gm, X = points(case, 1)
    assert gm.S == 1 and gm.nl == 0
    rc, f, J = run_global(ctx, case, LSE, PROPAGATE, 1, X, want_f=True, want_J=True)
    f_map, J_map = run_sets(ctx, case, LSE, PROPAGATE, 1, X, want_f=True, want_J=True, entry="map")
    assert rc == 0 and same_bits(f, f_map) and same_bits(J, J_map)


@pytest.mark.parametrize("est, policy", [(LSE, PROPAGATE), (POISSON, OMIT)])
def test_a_masked_group_keeps_its_sentinel(ctx, est, policy):
    case = gc.kernel_case("mixed")
    gm, X = points(case, 1)
    rc, f, J = run_global(ctx, case, est, policy, 1, X, want_f=True, want_J=True, mask=[1, 0, 1], fill=SENTINEL)
    f_ref, J_ref = run_sets(ctx, case, est, policy, 1, X, want_f=True, want_J=True)
    assert rc == 0
    assert np.all(f[1] == SENTINEL) and np.all(J[1] == SENTINEL)
    for g in (0, 2):
        assert same_bits(f[g], f_ref[g]) and same_bits(J[g], J_ref[g])


def test_bad_arguments_return_their_positions(ctx):
    """Every refusal by the position of its argument (ctx = 1); nothing is launched."""
    case = gc.kernel_case("mixed")
    gm, X = points(case, 1)
    n, nf, S, m = case["n"], gm.nf, case["S"], case["m"]

    def rc(reps=1, want_f=True, want_J=False, est=LSE, **bad):
        return run_global(ctx, case, est, PROPAGATE, reps, bad.pop("X", X), want_f=want_f, want_J=want_J, **bad)[0]
    assert rc(est=2) == -2
    assert rc(sampling=1) == -3                             # BLSQ_SAMPLE_BIN: out of scope
    assert rc(sampling=2) == -3
    assert rc(nan_policy=2) == -4
    assert rc(model=5) == -5
    assert rc(model=4, ncomp=0) == -5                       # gauss2d: two coordinates
    assert rc(ncomp=0) == -6 and rc(ncomp=9) == -6
    assert rc(fam=None) == -7 and rc(cnt=None) == -8
    assert rc(S=0) == -9
    assert (gm.ns, gm.nl) == (4, 10) and rc(S=26) == -9     # nv = 4 + 26 * 10 = 264 > BLSQ_GLOBAL_MAX_NV
    assert rc(shared=None) == -10
    assert rc(shared=[2] + [0] * (nf - 1)) == -10
    assert rc(t_sstride=m + 1) == -11
    assert rc(G=0) == -12 and rc(reps=0) == -13 and rc(m=0) == -14 and rc(n=n + 1) == -15
    assert rc(nf=0) == -16 and rc(nf=n + 1) == -16
    assert rc(pmap=None) == -17
    assert rc(t=None) == -18 and rc(t_stride=7) == -19
    assert rc(est=POISSON, y=None) == -20
    assert rc(nan_policy=OMIT, y=None) == -20
    assert rc(w_stride=m) == -22                            # per group is S m
    assert rc(X=None) == -23 and rc(Pfix=None) == -24
    assert rc(want_f=False) == -25
    assert rc(reps=3, want_J=True) == -26
    pm = gm.pm.pmap.copy()
    pm[0] = nf
    assert rc(pmap=pm) == -28
    pm = gm.pm.pmap.copy()
    pm[pm == nf - 1] = 0
    assert rc(pmap=pm) == -29


# ---- fits ------------------------------------------------------------------------------------------------------------
def fit(ctx, case, driver, method="trf", f=None, **kw):
    lb, ub = case["bounds"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return bounded_lsq.curve_fit_global(case["spec"] if f is None else f, case["x"], case["Y"], case["P0"],
                                            case["shared"], bounds=(lb, ub), method=method, driver=driver, ctx=ctx,
                                            fixed=case["fixed"], tied=case["tied"], **dict(gc.TOL, **case["kw"], **kw))


def against(got, ref_popt, ref_pcov, case, what, worst):
    """popt rtol 1e-6 / atol 1e-9; pcov atol 1e-6 after normalising by the REFERENCE's standard deviations (a wrong
    M - nv shows); rows and columns of fixed parameters are exactly 0 on both sides."""
    popt, pcov = got[0].reshape(ref_popt.shape), got[1].reshape(ref_pcov.shape)
    free = np.array([j for j in range(case["n"]) if j not in (case["fixed"] or ())])
    d = np.sqrt(np.einsum("gsii->gsi", ref_pcov)[:, :, free])
    a = pcov[:, :, free[:, None], free[None, :]] / (d[..., :, None] * d[..., None, :])
    b = ref_pcov[:, :, free[:, None], free[None, :]] / (d[..., :, None] * d[..., None, :])
    ep = float(np.max(np.abs(popt - ref_popt) / (1e-9 + 1e-6 * np.abs(ref_popt))))
    ec = float(np.max(np.abs(a - b)))
    worst[what] = (ep, ec)
    print("global fit %-28s popt error / margin %.3g   normalised pcov error %.3g" % (what, ep, ec))
    np.testing.assert_allclose(popt, ref_popt, rtol=1e-6, atol=1e-9, err_msg=str(what))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=str(what))
    for j in case["fixed"] or ():
        assert not pcov[:, :, j, :].any() and not pcov[:, :, :, j].any()


@pytest.fixture(scope="module")
def worst():
    return {}


@pytest.mark.parametrize("method", ["trf", "dogbox"])
@pytest.mark.parametrize("name", ["lse33", "lse70"])
def test_fit_device_host_and_reference(ctx, name, method, worst):
    """G = 4 groups of S = 5 data sets of gauss+poly*1 with shared position and width: the device route against the host
    route, and both against scipy on the hand-written concatenated residual."""
    case = gc.fit_case(name)
    ref_popt, ref_pcov, _, nv = gc.reference(name)
    D, H = fit(ctx, case, "device", method), fit(ctx, case, "host", method)
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    r = D[2][0]
    M = case["S"] * case["m"]
    assert r.x.shape == (nv,) and r.x_covariance.shape == (nv, nv) and r.popt.shape == (case["S"], case["n"])
    assert r.fun.shape == (M,) and r.jac.shape == (M, nv)
    for j in case["shared"]:                               # equal in all S rows
        assert np.all(D[0][:, :, j] == D[0][:, :1, j])
    against(D, ref_popt, ref_pcov, case, (name, method, "device"), worst)
    against(H, ref_popt, ref_pcov, case, (name, method, "host"), worst)
    against(D, H[0], H[1], case, (name, method, "device-host"), worst)


@pytest.mark.parametrize("name", ["poisson", "ragged", "soft_l1", "fixtied"])
def test_fit_variants_against_the_reference(ctx, name, worst):
    """estimator='poisson' with absolute_sigma=True; three data sets of 40, 64 and 70 points through pad_ragged and
    nan_policy='omit' against the reference on the compressed data; loss='soft_l1'; fixed= / tied=."""
    case = gc.fit_case(name)
    ref_popt, ref_pcov, _, nv = gc.reference(name)
    D, H = fit(ctx, case, "device"), fit(ctx, case, "host")
    assert all(r.success for r in D[2]) and all(r.success for r in H[2])
    if name == "ragged":
        assert D[0].shape == (1, 3, 4) and D[2][0].nobs == 40 + 64 + 70 and D[2][0].omitted.shape == (3, 70)
    if name == "poisson":
        assert abs(D[2][0].deviance - D[2][0].obj_value) <= 1e-9 * D[2][0].deviance
    against(D, ref_popt, ref_pcov, case, (name, "device"), worst)
    against(H, ref_popt, ref_pcov, case, (name, "host"), worst)
    against(D, H[0].reshape(ref_popt.shape), H[1].reshape(ref_pcov.shape), case, (name, "device-host"), worst)


def test_fit_with_three_point_differences(ctx, worst):
    """jac='3-point': device finite differences over the nv variables, through fun_dev with reps."""
    case = gc.fit_case("lse33")
    ref_popt, ref_pcov, _, nv = gc.reference("lse33")
    D = fit(ctx, case, "device", jac="3-point")
    assert all(r.success for r in D[2])
    against(D, ref_popt, ref_pcov, case, ("lse33", "3-point", "device"), worst)


def test_leverages_agree_and_sum_to_the_rank(ctx):
    case = gc.fit_case("lse33")
    nv = gc.reference("lse33")[3]
    D, H = fit(ctx, case, "device", leverage=True), fit(ctx, case, "host", leverage=True)
    for rd, rh in zip(D[2], H[2]):
        assert rd.leverage.shape == (case["S"] * case["m"],)
        np.testing.assert_allclose(rd.leverage, rh.leverage, rtol=1e-6, atol=1e-9)
        assert abs(rd.leverage.sum() - nv) < 1e-6          # trace of the hat matrix = rank = nv


def test_one_data_set_equals_curve_fit_batch(ctx):
    """S = 1: popt and pcov array_equal to curve_fit_batch(..., fixed=, tied=) on both drivers."""
    case = gc.fit_case("fixtied")
    G, S, m, n = case["G"], case["S"], case["m"], case["n"]
    Y, P0 = case["Y"].reshape(G * S, 1, m), case["P0"].reshape(G * S, 1, n)
    lb, ub = (b.reshape(G * S, 1, n) for b in case["bounds"])
    leaders = [0, 1, 2, 3, 4]                              # every free parameter: the variables keep ParamMap's order
    for driver in ("device", "host"):
        kw = dict(sigma=0.05, driver=driver, ctx=ctx, fixed=case["fixed"], tied=case["tied"], **gc.TOL)
        g = bounded_lsq.curve_fit_global(case["spec"], case["x"], Y, P0, leaders, bounds=(lb, ub), **kw)
        b = bounded_lsq.curve_fit_batch(case["spec"], case["x"], Y[:, 0], P0[:, 0], bounds=(lb[:, 0], ub[:, 0]), **kw)
        assert all(r.success for r in b[2])
        assert np.array_equal(g[0][:, 0], b[0]) and np.array_equal(g[1][:, 0], b[1])


def test_device_route_goes_through_the_new_entry_alone(ctx, monkeypatch):
    """The device route reaches no numpy model function and no blsq_model_eval* entry but the new one; and
    curve_fit_batch still does not call it."""
    from bounded_lsq import _models, _outer
    case = gc.fit_case("lse33")
    before = fit(ctx, case, "device")

    def boom(*a, **k):
        raise AssertionError("a host callback was reached")
    monkeypatch.setattr(_outer.OuterDriver, "run_host", boom)
    monkeypatch.setattr(_models.CompositeModel, "f", boom)
    monkeypatch.setattr(_models.CompositeModel, "jac", boom)
    entries = me.count_entries(ctx, monkeypatch)
    got = fit(ctx, case, "device")
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1])
    assert set(entries) == {"blsq_model_eval_global_dev"}
    entries.clear()
    fit(ctx, gc.fit_case("poisson"), "device")
    fit(ctx, gc.fit_case("ragged"), "device", jac="2-point")
    assert set(entries) == {"blsq_model_eval_global_dev"}
    entries.clear()
    G, S, m, n = case["G"], case["S"], case["m"], case["n"]
    bounded_lsq.curve_fit_batch(case["spec"], case["x"], case["Y"].reshape(G * S, m), case["P0"].reshape(G * S, n),
                                sigma=0.05, ctx=ctx, driver="device", **gc.TOL)
    assert set(entries) == {"blsq_model_eval_comp_dev"}
