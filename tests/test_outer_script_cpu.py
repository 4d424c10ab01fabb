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


def played(name):
    """One run of each configuration, shared by the tests of this module."""
    if name not in _runs:
        sb = sh.CONFIGS[name]()
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
