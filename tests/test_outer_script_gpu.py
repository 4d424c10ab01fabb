"""The device outer driver (outer_kernels.hip and the sequencing of blsq_outer.hip) against the scripted shadow of the
reference's loops (tests/_outer_shadow.py), branch by branch.

The test owns the callbacks of the raw protocol (start / begin / propose / judge / fetch): every f_trial and every fresh
J is what the script says, so each branch of the accept / radius / termination logic is entered on purpose, in every
round by different problems of the batch.  Delta and alpha are not fetchable; they are seen through the next x_trial (a
wrong Delta is off by 2 or 4, a wrong carried alpha moves the step at the 1e-2 level).  test_outer_script_cpu.py holds
the margins that make every decision here safe from rounding."""
import ctypes as C
import time

import numpy as np
import pytest

import _outer_shadow as sh

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
FIELDS = ('x', 'f', 'obj', 'optimality', 'on_bound', 'nfev', 'njev', 'status')


@pytest.fixture(scope="module")
def ctx():
    from bounded_lsq import _abi
    c = _abi.Context(0)
    yield c
    c.close()


def _bits(R, b):
    return tuple(np.ascontiguousarray(R[k][b]).tobytes() for k in FIELDS)


def _check_fetch(name, sb, R, exp, x_allow, frozen, live):
    """One fetch against what the shadow says it must show; `x_allow`: 1e-9 times the norm of the step that led to each
    x (the bound on x after an accept is the bound on its x_trial; `play(..., carry=True)`: plus the difference of the
    two x measured before that step); `live`: the problems judged in this round."""
    B = sb.B
    for k in ('nfev', 'njev', 'status'):
        assert np.array_equal(R[k], exp[k]), (name, k, R[k], exp[k])
    assert np.array_equal(R['on_bound'], exp['on_bound']), (name, 'on_bound')
    assert np.array_equal(R['f'], exp['f']), (name, 'f')                  # an accepted f_trial, bit for bit
    np.testing.assert_allclose(R['obj'], exp['obj'], rtol=1e-12, atol=0, err_msg=name)
    for b in range(B):
        bound = x_allow[b] + 4 * EPS * np.linalg.norm(exp['x'][b])
        err = np.linalg.norm(R['x'][b] - exp['x'][b])
        assert err <= bound, (name, 'x', b, err, bound)
        if exp['status'][b] == 1:
            assert R['optimality'][b] < sb.gtol and exp['optimality'][b] < sb.gtol, (name, b)
        else:
            np.testing.assert_allclose(R['optimality'][b], exp['optimality'][b], rtol=1e-9, atol=0,
                                       err_msg='%s optimality %d' % (name, b))
        if b in frozen:                                                    # nothing of a frozen problem is written
            assert _bits(R, b) == frozen[b], (name, 'frozen problem written', b)
        elif not live[b]:
            frozen[b] = _bits(R, b)
    if sb.method == 'dogbox':                                              # dogbox.py:258-261: exactly on the bound
        ob = R['on_bound']
        assert np.array_equal(R['x'][ob == -1], sb.lb[ob == -1]) and np.array_equal(R['x'][ob == 1], sb.ub[ob == 1])


def play(ctx, name, sb=None, make_driver=None, observe=None, carry=False):
    """Drive OuterDriver and the shadow in lock-step; returns (rounds, branch counts, worst x_trial error / bound).
    `carry`: for Jacobians on which a step of the library and of the oracle agree to 1e-12 .. 1e-11 of its norm instead
    of 1e-15.  x is the sum of the accepted steps, so there the two x differ by that much of a LARGE step accepted
    earlier, and a later trial at a radius shrunk by 4^-5 inherits a difference above 1e-9 of its own small step without
    any new error.  With carry=True the inherited difference ||x_device - x_oracle|| is MEASURED at every propose and
    nothing is allowed for it beyond what was measured: x_trial is held, by the same 1e-9 ||step|| + 4 eps ||x||, to the
    oracle's step added to the DEVICE's x; x after an accept to that bound plus the difference measured before the
    step; and x may change in an accept only -- at every propose it is, byte for byte, the x of the last fetch, and a
    rejected trial leaves it byte for byte.  The third value returned is then the worst error of x_trial against
    (device x + oracle step) over the bound, and 'final' is observed with `literal`, the worst error of x_trial
    against the oracle's x_trial over the same bound.
    `ctx`: the context the driver lives on (its route switches are the caller's); `sb`: the shadow to play instead of
    ``CONFIGS[name]()``; `make_driver(sb, ctx)`: the driver instead of an OuterDriver of the shadow's shape;
    `observe(event, sb, **what)`: called with 'begin' (before begin()), 'proposed' (round, act, x_trial), 'judged'
    (round, accepted, fetch) and 'final' (fetch) -- what it sees is what the assertions here have seen."""
    from bounded_lsq import OuterDriver
    sb = sh.CONFIGS[name]() if sb is None else sb
    sb.start()
    B, m, n = sb.B, sb.m, sb.n
    itemJ = m * n * 8
    worst = literal = 0.0
    frozen = {}
    x_allow = np.zeros(B)                                  # 1e-9 x the norm of the last ACCEPTED step of each problem
    x_last = sb.Xs.copy()                                  # (carry) the device's x as last seen
    drv = OuterDriver(sb.method, B, m, n, ctx=ctx) if make_driver is None else make_driver(sb, ctx)
    try:
        drv.start(sb.X0, sb.Xs, sb.lb, sb.ub, sb.scale, sb.jac_scaling, sb.ftol, sb.xtol, sb.gtol, sb.max_nfev)
        drv._up(drv.d_f, sb.F0, (B, m))
        drv._up(drv.d_J, sb.J0, (B, m, n))
        if observe:
            observe('begin', sb)
        drv.begin()
        while True:
            act, xt_ref, sn = sb.propose()
            x_ref = sb.current_x()
            n_active = drv.propose()
            assert n_active == int(act.sum()), (name, sb.rounds, n_active, act)
            xt = drv._down(drv.d_x_trial, (B, n))
            xd = drv._down(drv.d_x, (B, n))
            inherited = np.linalg.norm(xd - x_ref, axis=1)                 # (carry) measured, never assumed
            if carry:
                assert xd.tobytes() == x_last.tobytes(), (name, 'x changed between a fetch and the next propose', sb.rounds)
            for b in range(B):
                if act[b]:
                    bound = 1e-9 * sn[b] + 4 * EPS * np.linalg.norm(x_ref[b])
                    err = np.linalg.norm(xt[b] - xt_ref[b])
                    literal = max(literal, err / bound)
                    if carry:                                              # against the oracle's step from the device's x
                        err = np.linalg.norm(xt[b] - (xd[b] + (xt_ref[b] - x_ref[b])))
                    worst = max(worst, err / bound)
                    assert err <= bound, (name, 'x_trial', sb.rounds, b, err, bound)
                else:                                                      # frozen: the trial point is x itself
                    assert xt[b].tobytes() == xd[b].tobytes(), (name, 'x_trial of a frozen problem', b)
            if observe:
                observe('proposed', sb, round=sb.rounds, act=act, x_trial=xt)
            if n_active == 0:
                break
            ft = sb.f_trials()                                             # NaN rows for the problems that are done
            drv._up(drv.d_f_trial, ft, (B, m))
            n_accepted = drv.judge()
            acc_ref, exp, fresh = sb.judge(ft)
            acc = drv._down(drv.d_accepted, (B,), np.int32)
            assert np.array_equal(acc != 0, acc_ref), (name, sb.rounds, acc, acc_ref)
            assert n_accepted == int(acc_ref.sum()), (name, sb.rounds, n_accepted)
            x_allow[acc_ref] = 1e-9 * sn[acc_ref] + (inherited[acc_ref] if carry else 0.0)
            R = drv.fetch()
            _check_fetch(name, sb, R, exp, x_allow, frozen, act)
            if carry:
                kept = ~acc_ref
                assert R['x'][kept].tobytes() == xd[kept].tobytes(), (name, 'x of a problem without an accept changed', sb.rounds)
                x_last = R['x'].copy()
            if observe:
                observe('judged', sb, round=sb.rounds - 1, accepted=acc, fetch=R)
            for b, Jb in fresh.items():                                    # the accepted problems' Jacobians only
                dst = C.c_void_p(drv.d_J.value + int(b) * itemJ)
                ctx.check(ctx.lib.blsq_memcpy_h2d(ctx.h, dst, Jb.ctypes.data_as(C.c_void_p), itemJ), "h2d")
        R = drv.fetch()
        _check_fetch(name, sb, R, sb.final(), x_allow, frozen, np.zeros(B, dtype=bool))
        if observe:
            observe('final', sb, fetch=R, literal=literal)
    finally:
        drv.close()
    return sb.rounds, sb.branch_counts(), worst


# (the 'route-*' configurations are played by test_outer_route_gpu.py, each on a context with its route's switches)
@pytest.mark.parametrize("name", [n for n in sorted(sh.CONFIGS) if sh.route_of(n) is None])
def test_device_driver_follows_the_script(ctx, name):
    t0 = time.perf_counter()
    rounds, counts, worst = play(ctx, name)
    print("\n[outer-script] %s rounds=%d worst_x_trial/bound=%.3g wall=%.2fs branches=%s"
          % (name, rounds, worst, time.perf_counter() - t0, sorted(counts.items())))
