"""The conditions the inputs of tests/test_geometry_gpu.py must meet themselves (no GPU; tests/_geometry_cases.py):
the screen rejects no more than its cap of a class's draws, what it admits still spans every branch the raw draws
reached, and the committed fixture is what the screen admits today."""
import numpy as np
import pytest

import _geometry_cases as gc

CAP = {"near12": 2.0 / 3.0}                                    # every other class: 1 in 4
TRF_BRANCHES = ("0,0", "1,0", "1,1", "1,2")                    # (branch, choice)


@pytest.fixture(scope="module")
def fix():
    return gc.load_fixture()


def test_fixture_lists_every_group_the_generator_draws(fix):
    want = list(gc.groups())
    got = [(G["solver"], G["route"], G["m"], G["n"], G["cls"], G["mode"]) for G in fix["groups"]]
    assert got == want
    assert fix["screen_rtol"] == gc.SCREEN_RTOL == 1e-12 and fix["patterns"] == 8
    for G in fix["groups"]:
        per_seed = len(gc.TRF_PAIRS) if G["solver"] == "trf" else len(gc.DOG_DELTAS)
        seeds = gc.group_seeds(G["solver"], G["route"], G["m"], G["n"], G["cls"])
        assert len(seeds) == (16 if G["n"] < 272 else 8)
        assert G["drawn"] == per_seed * len(seeds) == sum(G["raw"].values())
        assert len(G["admitted"]) == G["drawn"] - G["rejected"] - G["dropped"]
        assert {row[0] for row in G["admitted"]} <= set(seeds)
        assert all(row[-2] <= gc.SCREEN_RTOL / fix["margin"] for row in G["admitted"])


def test_screen_rejects_no_more_than_its_cap(fix):
    """Per (solver, route, shape, class) — the shapes of a route are held to the cap one by one.  `rejected` is the
    screen's tally under its eight patterns; what the tool drops on top of it (sixteen further patterns and a margin of
    four under the screen's bound, tools/make_geometry_cases.py) may not thin a group below a quarter of its draws:
    at least 16 cases (8 at n >= 272) of every group reach the GPU."""
    over, thin = [], []
    for G in fix["groups"]:
        cap = CAP.get(G["cls"], 0.25)
        tag = (G["solver"], G["route"], G["m"], G["n"], G["cls"], G["rejected"], G["dropped"], G["drawn"])
        if G["rejected"] > cap * G["drawn"]:
            over.append(tag)
        if 4 * len(G["admitted"]) < G["drawn"]:
            thin.append(tag)
    assert not over, over
    assert not thin, thin
    for G in fix["groups"]:                                    # (measured: no dogbox draw moves its oracle beyond 8.5e-14)
        if G["solver"] == "dogbox":
            assert G["rejected"] == 0 and G["dropped"] == 0, G["cls"]


def test_admitted_trf_cases_span_the_branches_of_the_raw_draws(fix):
    seen_all = set()
    for route in gc.ROUTES:
        raw, adm = {}, set()
        for G in fix["groups"]:
            if G["solver"] == "trf" and G["route"] == route:
                for k, v in G["raw"].items():
                    raw[k] = raw.get(k, 0) + v
                adm |= {",".join(str(v) for v in row[-1]) for row in G["admitted"]}
        for bc in TRF_BRANCHES:
            if raw.get(bc, 0) >= 2:
                assert bc in adm, (route, bc, raw)
        seen_all |= adm
    assert seen_all >= set(TRF_BRANCHES), seen_all


def test_admitted_dogbox_cases_span_tr_hit_on_bound_signs_and_a_clipped_dogleg(fix):
    for route in gc.ROUTES:
        if not gc.ROUTES[route]["dogbox"]:
            continue
        cases = gc.cases_of(fix, "dogbox", route)
        assert {c["info"][0] for c in cases} >= {0, 1}, route                   # tr_hit
        assert any(c["info"][2] == 1 for c in cases), route                     # the box clips the dogleg
        signs = set()
        seen = set()
        for c in cases:
            key = (c["m"], c["n"], c["cls"], c["seed"])
            if key in seen or c["cls"] not in ("both_signs", "one_sided_box", "upper"):
                continue
            seen.add(key)
            signs |= set(np.unique(gc.problem("dogbox", route, c["m"], c["n"], c["cls"], c["seed"])["on_bound"]))
        assert signs >= {-1, 1}, (route, signs)
        assert any(c["info"][0] == -1 for c in cases if c["cls"] == "all_active"), route


def test_generator_draws_what_its_classes_promise():
    """One problem per class at 60 x 16: the redrawn bounds, scale and on_bound are the geometry the class names."""
    m, n = 60, 16
    for cls in gc.TRF_CLASSES:
        for mode in gc.modes_for(cls):
            P = gc.trf_problem("reg", m, n, cls, 4242, mode)
            x, lb, ub = P["x"], P["lb"], P["ub"]
            assert np.all(lb < x) and np.all(x < ub)
            fl, fu = np.isfinite(lb), np.isfinite(ub)
            if cls == "one_sided":
                assert np.all(fl ^ fu) and fl.any() and fu.any()
            elif cls == "mixed":
                assert len({(a, b) for a, b in zip(fl, fu)}) == 4
            elif cls == "far":
                assert np.all(x - lb >= 5) and np.all(ub - x >= 5)
            elif cls == "near6":
                assert np.all(ub - x < 0.11) and (ub - x).min() < 1e-3
            elif cls == "near12":
                assert min((ub - x).min(), (x - lb).min()) < 1e-8
            if cls == "jac_scale":
                inv = 1.0 / np.linalg.norm(P["J"], axis=0)
                want = inv if mode == gc.SCALE_JAC_INIT else np.minimum(P["scale_in"], inv)
                np.testing.assert_array_equal(P["scale"], want)
                if mode == gc.SCALE_JAC_UPDATE:
                    assert (P["scale_in"] < inv).any() and (P["scale_in"] > inv).any()
            else:
                assert P["scale"].min() < 0.1 and P["scale"].max() > 10 and P["mode"] == gc.SCALE_GIVEN
    for cls in gc.DOG_CLASSES:
        P = gc.dogbox_problem("reg", m, n, cls, 4242)
        x, lb, ub, ob = P["x"], P["lb"], P["ub"], P["on_bound"]
        g = P["J"].T @ P["f"]
        assert np.all(x[ob > 0] == ub[ob > 0]) and np.all(x[ob < 0] == lb[ob < 0])
        assert np.all((x[ob == 0] > lb[ob == 0]) & (x[ob == 0] < ub[ob == 0]))
        assert np.all(np.isfinite(x))
        active = ob * g < 0
        if cls == "upper":
            assert (ob > 0).sum() == 3 and not (ob < 0).any()
        elif cls == "inward":
            assert (ob != 0).sum() == 3 and not active.any()
        elif cls == "one_free":
            assert active.sum() == n - 1
        elif cls == "all_active":
            assert active.all()
        elif cls == "one_sided_box":
            assert np.all(np.isfinite(lb) ^ np.isfinite(ub))
        elif cls == "far":
            assert np.all(ub - lb >= 5)


def test_fixture_is_what_the_screen_admits_today(fix):
    """Every admitted case with n <= 96, and one in four of the others, screened again under two fresh sign patterns
    (the tool used patterns 0 .. 7); and the recorded branch / choice / tr_hit are the oracle's on this host."""
    fresh = (101, 102)
    bad, count = [], 0
    for G in fix["groups"]:
        solver = G["solver"]
        by_seed = {}
        for row in G["admitted"]:
            by_seed.setdefault(row[0], []).append(row)
        seeds = sorted(by_seed)
        if G["n"] > 96:
            seeds = seeds[::4]
        for seed in seeds:
            P = gc.problem(solver, G["route"], G["m"], G["n"], G["cls"], seed, G["mode"])
            rows = by_seed[seed]
            radii = [(r[1], r[2]) for r in rows] if solver == "trf" else [r[1] for r in rows]
            for row, (ok, move, S) in zip(rows, gc.screen_problem(solver, P, radii, fresh)):
                count += 1
                if not ok or gc.summary(solver, S) != row[-1]:
                    bad.append((solver, G["route"], G["m"], G["n"], G["cls"], seed, row[1], move))
    print("re-screened", count, "cases")
    assert not bad, bad
