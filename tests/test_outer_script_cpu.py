"""The scripted shadow of the reference's outer loops (tests/_outer_shadow.py), run alone on every configuration that
test_outer_script_gpu.py plays against the device driver.  What is asserted here is a condition on the INPUTS: every
branch is visited, and every decision is taken with a margin that no rounding difference between a device reduction and
numpy's can bridge.  With that, a disagreement on the GPU is a finding and not noise."""
import math

import numpy as np
import pytest

import _outer_shadow as sh

NAMES = sorted(sh.CONFIGS)
_runs = {}


CYCLE_NAMES = [n for n in NAMES if sh.route_of(n) in ('tier', 'cqr2')]
SCREEN_NAMES = CYCLE_NAMES + [n for n in NAMES if sh.route_of(n) == 'short']      # (m < n: see _route_bounds)
SCREEN_CAP = 1e-10                     # of ||step||: a tenth of the bound test_outer_script_gpu.play holds x_trial to


def played(name):
    """One run of each configuration, shared by the tests of this module (the conditioning cycles with the one-ulp
    screen of every trial switched on: it adds records to the log and changes nothing else)."""
    if name not in _runs:
        sb = sh.CONFIGS[name]()
        if name in SCREEN_NAMES:
            sb.screen = 3
        sb.run_alone()
        _runs[name] = sb
    return _runs[name]


def _apart(lhs, rhs):
    return lhs != rhs and (lhs >= 2 * rhs or rhs >= 2 * lhs)


@pytest.mark.parametrize("name", NAMES)
def test_decision_margins(name):
    sb = played(name)
    trf = sb.method == 'trf'
    for b, log in enumerate(sb.log):
        move = None
        for rec in log:
            where = (name, b, move, rec.get('ratio'))
            if rec['kind'] == 'move':
                move = rec['move']
                continue
            for what, lhs, rhs in rec.get('cmp', ()):
                if math.isnan(lhs):                       # a NaN compares false in every implementation
                    continue
                if what == 'ftol' and move == "same":     # the one deliberately exact case: |0| < ftol obj
                    assert lhs == 0.0
                    continue
                assert _apart(lhs, rhs), (where, what, lhs, rhs)
            if rec['kind'] != 'trial':
                continue
            ratio = rec['ratio']
            if not math.isnan(ratio):
                assert abs(ratio - 0.25) >= 0.05 and abs(ratio - 0.75) >= 0.05, where
                if isinstance(move, (int, float)) and not rec.get('fallback'):
                    # the realised ratio is the scripted one, up to the rounding of obj - f_trial.f_trial over pred
                    assert abs(ratio - move) < 1e-6 + (sb.m + 8) * sh.EPS * rec['obj'] / rec['pred'], where
            if not trf:
                continue
            if ratio > 0.75:
                assert abs(rec['shn'] / rec['Delta'] - 0.95) >= 0.01, (where, rec['shn'] / rec['Delta'])
            assert abs(rec['to_bound'] - 1.0) >= 1e-6, (where, rec['to_bound'])
            if rec['branch'] == 1:
                qp, k = rec['qp'], rec['choice']
                for j in range(len(qp)):
                    if j != k and not np.array_equal(rec['steps_h'][j], rec['steps_h'][k]):
                        assert qp[j] - qp[k] >= 1e-6 * abs(qp[k]), (where, qp)


@pytest.mark.parametrize("method", ['trf', 'dogbox'])
def test_every_branch_is_visited(method):
    seen = {}
    for name in NAMES:
        if sh.method_of(name) == method:
            for t, c in played(name).branch_counts().items():
                seen[t] = seen.get(t, 0) + c
    wanted = sh.TAGS_BOTH + (sh.TAGS_DOGBOX if method == 'dogbox' else [])
    missing = [t for t in wanted if not seen.get(t)]
    assert not missing, (missing, seen)
    if method == 'trf':                                   # both step branches of the oracle: feasible and reflective
        br = {rec['branch'] for name in NAMES if sh.method_of(name) == 'trf' for log in played(name).log
              for rec in log if rec['kind'] == 'trial'}
        assert br == {0, 1}


@pytest.mark.parametrize("method", ['trf', 'dogbox'])
def test_decision_table_rotates_the_branches(method):
    """In the decision table different problems sit in different branches in the same round, several rejections follow
    one another (the carried alpha), and the 'jac' scale update both changes and keeps entries."""
    for scaling in ('given', 'jac'):
        sb = played('decision-%s-%s' % (method, scaling))
        per_round = {}
        streak = 0
        for log in sb.log:
            r, run = 0, 0
            for rec in log:
                if rec['kind'] != 'trial':
                    continue
                per_round.setdefault(r, set()).add(frozenset(rec['tags'] - {'pending-on-reject'}))
                r += 1
                run = run + 1 if ('reject' in rec['tags'] and 'shrink' in rec['tags']) else 0
                streak = max(streak, run)
        assert sum(len(v) >= 3 for v in per_round.values()) >= 8, {k: len(v) for k, v in per_round.items()}
        assert streak >= 2
        assert sb.rounds == 13
        fin = sb.final()
        assert (fin['status'] == 0).all() and (fin['nfev'] == 14).all()
        if scaling == 'jac':
            ups = [rec for log in sb.log for rec in log[1:] if rec['kind'] == 'scale']
            assert any(u['changed'] and u['kept'] for u in ups)


@pytest.mark.parametrize("method", ['trf', 'dogbox'])
def test_termination_table_is_what_it_says(method):
    def run(case):
        sb = played('termination-%s-%s' % (method, case))
        return sb, sb.final(), sb.branch_counts()
    sb, fin, c = run('ftol')
    assert (fin['status'] == 2).all() and c.get('shrink', 0) > 0       # ratios < 0.25 were played and did not stop
    sb, fin, c = run('xtol')
    assert (fin['status'] == 3).all() and c.get('pending-on-reject', 0) >= 4
    assert (fin['njev'] == 1).any() and (fin['njev'] == 2).any() and (fin['nfev'] == 2).all()
    sb, fin, c = run('both')
    assert set(fin['status']) == {3, 4}
    sb, fin, c = run('xtol_arm')
    arms = {rec['xtol_arm'] for log in sb.log for rec in log
            if rec['kind'] == 'trial' and rec['cmp'][1][1] < rec['cmp'][1][2]}
    assert arms == {'eps', 'x'}, arms
    assert (fin['status'][0::3] == 3).sum() >= 2 and (fin['status'][2::3] == 3).sum() >= 2
    assert (fin['status'][1::3] == 0).all()               # ||x0|| = 1: three evaluations never get the step that small
    sb, fin, c = run('orth')
    assert (fin['status'] == 1).all() and (fin['nfev'] < 14).all()
    sb, fin, c = run('lost')
    assert c.get('status-lost-to-max_nfev', 0) >= 2 and c.get('status2', 0) >= 2
    assert (fin['nfev'][fin['status'] == 0] == 4).all()
    sb, fin, c = run('nfev1')
    assert sb.rounds == 0 and (fin['nfev'] == 1).all() and (fin['status'] == 0).all()


def test_dogbox_starts_are_what_they_say():
    sb = played('starts-dogbox')
    fin = sb.final()
    assert (fin['status'][:4] == 1).all() and (fin['nfev'][:4] == 1).all() and (fin['optimality'][:4] == 0).all()
    first = [log[0] for log in sb.log]
    assert all('all-active' in t['tags'] for t in first[:4])
    assert all((t['start_on_bound'] == 1).any() for t in first)
    mixed = [t for t in first[4:] if (t['active'] & (t['start_on_bound'] == 1)).any()
             and (~t['active'] & (t['start_on_bound'] != 0)).any()]
    assert len(mixed) >= 3
    c = sb.branch_counts()
    assert c.get('tr_hit', 0) >= 2 and c.get('good-but-inside', 0) >= 2 and c.get('snap', 0) >= 1


@pytest.mark.parametrize("name", ['shape-trf-3x300x257', 'shape-dogbox-3x300x257', 'shape-trf-300x6x3',
                                  'shape-trf-4x1x1', 'shape-dogbox-4x1x1'])
def test_shape_edges_walk_accepts_and_rejects(name):
    c = played(name).branch_counts()
    assert c.get('shrink', 0) and c.get('reject', 0) and c.get('exact-zero', 0) and (c.get('double', 0)
                                                                                     or c.get('keep', 0))


# ---- the route configurations: conditions on the inputs of test_outer_route_gpu.py -----------------------------
def test_route_table_is_complete():
    """Every route for both methods, B = 6 (n = 256: 3), max_nfev <= 12, accepts and rejects in every round."""
    for method in ('trf', 'dogbox'):
        for route, (_, shapes, _) in sh.ROUTES.items():
            for (m, n) in shapes:
                sb = played('route-%s-%s-%dx%d' % (method, route, m, n))
                assert (sb.m, sb.n) == (m, n) and sb.B == (3 if n >= 256 else 6) and sb.max_nfev <= 12
                assert sb.rounds == sb.max_nfev - 1
                c = sb.branch_counts()
                assert c.get('reject', 0) and c.get('shrink', 0) and (c.get('double', 0) or c.get('keep', 0)), c
                mixed = 0                                       # rounds r with accepts (a refresh for r + 1) and rejects
                for r in range(sb.rounds - 1):
                    fresh = {b for (q, b, _, _) in sb.refreshes if q == r + 1}
                    mixed += int(0 < len(fresh) < sb.B)
                assert mixed == sb.rounds - 1 if sb.B >= 6 else mixed >= 6, (method, route, mixed)


def _same(a, b):
    """Bit-for-bit equality of two log records / snapshots (dicts, sequences, arrays, floats with NaN == NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def _trace(sb):
    """Everything the shadow hands to the device test, round by round."""
    sb.start()
    out = [dict(F0=sb.F0.copy(), J0=sb.J0.copy())]
    while True:
        act, xt, sn = sb.propose()
        out.append(dict(act=act, xt=xt, sn=sn, x=sb.current_x()))
        if not act.any():
            break
        ft = sb.f_trials()
        acc, exp, fresh = sb.judge(ft)
        out.append(dict(ft=ft, acc=acc, exp=exp, fresh=fresh))
    out.append(sb.final())
    return out


def _row(v, k):
    if isinstance(v, dict) and all(isinstance(q, (int, np.integer)) for q in v):      # fresh: {b: J}
        return {0: v[k]} if k in v else {}
    if isinstance(v, dict):
        return {q: _row(w, k) for q, w in v.items()}
    return v[k:k + 1]


@pytest.mark.parametrize("name", ['route-trf-rl-160x96', 'route-dogbox-tier-600x96', 'decision-trf-jac'])
def test_a_problem_played_alone_is_its_row_of_the_batch(name):
    """ShadowBatch(..., ids=[b]): the same streams, so the same log, trial points, f_trials, snapshots and fresh
    Jacobians as row b of the batch, bit for bit (what the history-independence test on the device rests on)."""
    if sh.route_of(name):
        make = sh.CONFIGS[name]
    else:                                                       # (a configuration from before `ids`: through its batch)
        def make(ids=None):
            full = sh.CONFIGS[name]()
            return sh.ShadowBatch(full.method, full.m, full.X0, full.lb, full.ub,
                                  None if full.jac_scaling else full.scale, (full.ftol, full.xtol, full.gtol),
                                  full.max_nfev, full.scripts, full.seed, full.J0_mod, full.J0_class, ids=ids)
    batch = make()
    whole = _trace(batch)
    for b in (0, batch.B // 2, batch.B - 1):
        lone = make(ids=[b])
        alone = _trace(lone)
        assert lone.B == 1 and lone.ids == [b]
        assert _same(lone.log[0], batch.log[b]), (name, b)
        assert len(alone) == len(whole)
        for r, (one, all_) in enumerate(zip(alone, whole)):
            assert _same(one, _row(all_, b)), (name, b, r)
        assert lone.refreshes == [e for e in batch.refreshes if e[1] == b]
        assert lone.classes == [{b: c[b]} if b in c else {} for c in batch.classes]


def test_short_trf_steps_are_determined():
    """m < n under trf: every factor's augmented matrix (trf.py:264-268) has full column rank by a wide margin, so no
    step is decided by a null space (there the reference's own step is rounding noise).  The reference's
    sub-problem solver still takes its not-full-rank branch (m < n) and may end on a negative alpha after ten
    iterations: deterministic, and the screen below holds it to 1e-10 like every other step."""
    sb = played('route-trf-short-40x60')
    trials = [rec for log in sb.log for rec in log if rec['kind'] == 'trial']
    assert len(trials) == sb.B * sb.rounds
    assert min(rec['s_ratio'] for rec in trials) >= 1e-4, min(rec['s_ratio'] for rec in trials)
    assert all(not np.isfinite(sb.lb[b]).all() or not np.isfinite(sb.ub[b]).all() for b in range(sb.B))
    assert all(np.isfinite(sb.lb[b]).all() or np.isfinite(sb.ub[b]).all() for b in range(sb.B))


@pytest.mark.parametrize("name", SCREEN_NAMES)
def test_conditioning_cycle_passes_the_one_ulp_screen(name):
    """The oracle alone: with every entry of J moved one ulp (three sign patterns) the step of EVERY trial moves by at
    most 1e-10 of its norm and no mask, branch, choice or iteration count changes.  A condition on the draw — a seed
    that fails it is replaced, the cap stays."""
    sb = played(name)
    worst, count = 0.0, 0
    for b, log in enumerate(sb.log):
        for rec in log:
            if rec['kind'] != 'trial':
                continue
            move, same = rec['screen']
            assert same, (name, b, rec['Delta'])
            assert move <= SCREEN_CAP, (name, b, rec['Delta'], move)
            worst, count = max(worst, move), count + 1
    assert count == sb.B * sb.rounds
    print("\n[outer-route] %s: %d trials screened, worst oracle movement %.3g of ||step||" % (name, count, worst))


@pytest.mark.parametrize("name", CYCLE_NAMES)
def test_conditioning_cycle_covers_the_masked_branches(name):
    """What the masked factor calls of these configurations meet, from sb.refreshes and sb.classes (round r: the round
    whose propose() factors the Jacobians accepted in round r - 1; a problem counts in a round it is active in)."""
    sb = played(name)
    assert sorted(set(sb.J0_class)) == ['beyond', 'tier', 'well']
    proper = kept_tier = relist = 0
    trans = {}
    for r in range(1, sb.rounds):
        active = sb.classes[r]
        fresh = {b: new for (q, b, old, new) in sb.refreshes if q == r and b in active}
        for (q, b, old, new) in sb.refreshes:
            if q == r and b in active:
                assert active[b] == new
                trans[(old, new)] = trans.get((old, new), 0) + 1
        kept = [b for b in active if b not in fresh and active[b] == 'tier']      # rejected: steps again on its factor
        proper += int(0 < len(fresh) < len(active))
        kept_tier += int(bool(fresh) and bool(kept))
        # no refreshed problem fails the certificate while the tier keeps a problem: the relist branch
        relist += int(bool(fresh) and bool(kept) and all(c == 'well' for c in fresh.values()))
    print("\n[outer-route] %s: proper subsets %d, tier problem kept beside a refresh %d, relist rounds %d, transitions %s"
          % (name, proper, kept_tier, relist, sorted(trans.items())))
    assert proper >= 6 and kept_tier >= 3 and relist >= 1
    for t in (('well', 'tier'), ('tier', 'beyond'), ('beyond', 'well')):
        assert trans.get(t, 0) >= 2, (t, trans)
    assert set(trans) == {('well', 'tier'), ('tier', 'beyond'), ('beyond', 'well')}
