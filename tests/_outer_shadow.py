"""A scripted float64 shadow of the reference's outer loops, per problem (trf.py:201-358, dogbox.py:148-272).

The loops below are the reference's own, line for line, written as generators: where the reference calls ``fun`` or
``jac`` the generator yields and receives the value, so the CALLER decides every f_trial and every fresh J.  The steps
come from the committed CPU oracle (``oracle/blsq_oracle.py``).  Nothing here is written from ``outer_kernels.hip``.

``ShadowBatch`` plays B such generators in lock-step from a script (one move per trial evaluation and problem):

    r (a number)      target ratio: ``obj_target = obj - (correction + r pred)`` (dogbox: ``obj - r pred``), then
                      ``f_trial = u sqrt(obj_target / u.u)`` for a fresh seeded direction u
    "same"            f_trial = f bit for bit (actual_reduction == 0 exactly)
    "nan"             f with one NaN
    (r, "orth")       as r; if the trial is accepted the fresh J is projected so that J^T f = 0 (status 1 next top)
    (r, "cols")       as r; the fresh J has its columns rescaled by 10^+-1 (the 'jac' scale update changes some
                      entries and keeps others)
    (r, "kappa", c)   as r; the fresh J is of conditioning class c (below), or of the class after the problem's
                      current one in KAPPA_CYCLE if c is "next"; composes with "cols"

After an accept the fresh J is seeded: J and f need not come from any function, so a 1e-10 difference in x between two
implementations cannot steer the trajectory; only decisions can.

Conditioning classes of a problem's current J (KAPPA): "well" is a Gaussian matrix; "tier" and "beyond" have singular
values log-spaced over [1 / kappa, 1] sqrt(m) with kappa = 2e4 and 1.5e5 (the construction of
``_geometry_cases._logspaced``), drawn from the problem's own stream.  ``J0_class[b]`` is the class of the first J, a
"kappa" modifier sets the class of a fresh one; a J without either is "well".  ``sb.refreshes`` holds one entry
(round, b, old class, new class) per fresh J, `round` being the round whose propose() factors it (the masked factor call
of the device driver: always >= 1), and ``sb.classes[r]`` the class each problem active in round r steps on.  There is
no rank-deficient class: the reference's step is determined by rounding noise there (tests/test_cqr2_gpu.py leaves such
problems out of its parity check for that reason), so no implementation can be held to it.

``ids``: ``ShadowBatch(..., ids=[b])`` is problem b of the batch the other arguments describe, played alone: its random
stream is ``default_rng([seed, b])`` and its script, x0, bounds, scale and classes are row b of the batch's, so its log
and every snapshot equal the batch's row b bit for bit (test_outer_script_cpu.py).

``screen``: with ``sb.screen = k`` set before start(), every trial's step is computed again by the oracle on k copies of
the current J with EVERY entry moved one ulp (``_geometry_cases.one_ulp``); the trial's log record gets
``screen = (largest ||step' - step|| / ||step||, all masks / branch / choice / n_iter unchanged)``.

To add a move: give it a branch in ``ShadowBatch._f_trial`` (what f_trial is) or ``_fresh_J`` (what the next J is), a
tag in the loops' ``tags`` if it opens a new branch, and a case in ``CONFIGS`` whose script plays it;
``test_outer_script_cpu.py`` then has to see its tag and its decision margins.
"""
import math

import numpy as np
from numpy.linalg import norm

from oracle import blsq_oracle as orc

EPS = orc.EPS

# every branch a trial or a top can take; test_outer_script_cpu.py asserts each is visited per method where it applies
TAGS_BOTH = ["shrink", "keep", "double", "good-but-inside", "reject", "exact-zero", "nan", "status0", "status1",
             "status2", "status3", "status4", "pending-on-reject", "status-lost-to-max_nfev"]
TAGS_DOGBOX = ["snap", "all-active", "tr_hit"]

# conditioning classes of a scripted J: kappa_2(J).  "tier": the CSNE tier's own (_geometry_cases.CSNE_KAPPA); "beyond":
# past the tier's measured bound (test_csne_gpu.py: 1.5e5 is declined) and still a decade inside what the oracle's own
# step tolerates under one-ulp changes of J (at 1e6 numpy's Gauss-Newton step moves by 1e-10 of its norm)
KAPPA = {"tier": 2e4, "beyond": 1.5e5}
KAPPA_CYCLE = ["well", "tier", "beyond"]


class Trial:
    """What the loop hands out where the reference calls fun(x_new)."""

    def __init__(self, x_new, step, pred, corr, obj, f, x):
        self.x_new, self.step, self.pred, self.corr, self.obj, self.f, self.x = x_new, step, pred, corr, obj, f, x


def _snapshot(x, f, obj, g_norm, nfev, njev, on_bound, accepted):
    return dict(x=x.copy(), f=f.copy(), obj=float(obj), optimality=float(g_norm), nfev=int(nfev), njev=int(njev),
                on_bound=on_bound.copy(), status=0, accepted=bool(accepted))


def trf_loop(x0, lb, ub, ftol, xtol, gtol, max_nfev, scale, log, probe=None):
    """trf.py:201-358.  `scale`: the reference's ``1 / scaling`` (n,), or None for scaling='jac'.  Yields
    ('fun', x) / ('jac', x) / ('trial', Trial) and expects f / J / f_new back; ('judged', snapshot) after every
    trial (what a fetch must show then).  Returns the result dict.  Appends one record per trial and per top to `log`."""
    jac_scaling = scale is None
    x = orc.nudge_inside(x0, lb, ub, rstep=1e-10)
    f = yield ('fun', x)
    nfev = 1
    J = yield ('jac', x)
    njev = 1
    g = J.T.dot(f)
    m, n = J.shape
    if jac_scaling:
        J_norm = norm(J, axis=0)
        J_norm[J_norm == 0] = 1
        scale = 1 / J_norm
    v, jv = orc.cl_scaling(x, g, lb, ub)
    Delta = norm(x0 / (scale * v ** 0.5))
    if Delta == 0:
        Delta = 1.0
    obj_value = np.dot(f, f)
    alpha = 0.0
    g_norm = 0.0                       # (the reference leaves it unset when max_nfev == 1; the library reports 0)
    zeros = np.zeros(n, dtype=np.int64)
    termination_status = None
    while nfev < max_nfev:
        if jac_scaling:
            J_norm = norm(J, axis=0)
            with np.errstate(divide='ignore'):
                new_scale = np.minimum(scale, 1 / J_norm)
            log.append(dict(kind='scale', changed=int(np.sum(new_scale != scale)),
                            kept=int(np.sum(new_scale == scale))))
            scale = new_scale
        F = orc.trf_factor(J, f, x, lb, ub, scale)
        g_norm = F.g_norm
        if g_norm < gtol:
            termination_status = 1
        log.append(dict(kind='top', cmp=[('gtol', g_norm, gtol)], tags=set()))
        if termination_status is not None:
            log[-1]['tags'].add('status%d' % termination_status)
            return dict(x=x, f=f, obj=float(obj_value), optimality=float(g_norm), nfev=nfev, njev=njev,
                        on_bound=zeros, status=termination_status)
        actual_reduction = -1
        while actual_reduction <= 0 and nfev < max_nfev:
            S = orc.trf_step(F, Delta, alpha)
            screened = probe(S, J, f, x, scale, Delta, alpha, None) if probe else None
            alpha = S.alpha
            step_h, step, x_new = S.step_h, S.step, S.x_new
            predicted_reduction = S.predicted_reduction
            correction = np.dot(step_h * F.diag_h, step_h)
            f_new = yield ('trial', Trial(x_new, step, predicted_reduction, correction, obj_value, f, x))
            nfev += 1
            obj_value_new = np.dot(f_new, f_new)
            actual_reduction = obj_value - obj_value_new
            if predicted_reduction > 0:
                ratio = (actual_reduction - correction) / predicted_reduction
            else:
                ratio = 0
            tags = set()
            rec = dict(kind='trial', ratio=float(ratio), tags=tags, Delta=float(Delta), shn=float(norm(step_h)),
                       pred=float(predicted_reduction), obj=float(obj_value),
                       branch=S.branch, to_bound=S.to_bound, qp=np.array(S.qp), steps_h=S.steps_h, choice=S.choice,
                       alpha=float(S.alpha), n_iter=int(S.n_iter), s_ratio=float(F.s[-1] / F.s[0]))
            if screened is not None:
                rec['screen'] = screened
            if ratio < 0.25:
                Delta_new = 0.25 * norm(step_h)
                alpha *= Delta / Delta_new
                Delta = Delta_new
                tags.add('shrink')
            elif ratio > 0.75 and norm(step_h) > 0.95 * Delta:
                Delta *= 2.0
                alpha *= 0.5
                tags.add('double')
            elif ratio > 0.75:
                tags.add('good-but-inside')
            elif ratio >= 0.25:
                tags.add('keep')
            ftol_satisfied = (abs(actual_reduction) < ftol * obj_value and ratio > 0.25)
            xtol_rhs = xtol * max(EPS ** 0.5, norm(x))
            xtol_satisfied = norm(step) < xtol_rhs
            rec['cmp'] = [('ftol', abs(actual_reduction), ftol * obj_value), ('xtol', norm(step), xtol_rhs)]
            rec['xtol_arm'] = 'eps' if EPS ** 0.5 > norm(x) else 'x'
            if ftol_satisfied and xtol_satisfied:
                termination_status = 4
            elif ftol_satisfied:
                termination_status = 2
            elif xtol_satisfied:
                termination_status = 3
            if math.isnan(actual_reduction):
                tags.add('nan')
            elif actual_reduction == 0:
                tags.add('exact-zero')
            if not actual_reduction > 0:
                if not math.isnan(actual_reduction):
                    tags.add('reject')
                if termination_status is not None:
                    tags.add('pending-on-reject')
                log.append(rec)
                yield ('judged', _snapshot(x, f, obj_value, g_norm, nfev, njev, zeros, False))
            else:
                log.append(rec)
            if termination_status is not None:
                break
        if actual_reduction > 0:
            x = x_new
            f = f_new
            obj_value = obj_value_new
            yield ('judged', _snapshot(x, f, obj_value, g_norm, nfev, njev + 1, zeros, True))
            J = yield ('jac', x)
            njev += 1
    log.append(dict(kind='end', tags={'status0'} | ({'status-lost-to-max_nfev'} if termination_status is not None
                                                      else set())))
    return dict(x=x, f=f, obj=float(obj_value), optimality=float(g_norm), nfev=nfev, njev=njev, on_bound=zeros,
                status=0)


def dogbox_loop(x0, lb, ub, ftol, xtol, gtol, max_nfev, scale, log, probe=None):
    """dogbox.py:131-272; same protocol as `trf_loop`."""
    jac_scaling = scale is None
    f = yield ('fun', x0.copy())
    nfev = 1
    J = yield ('jac', x0.copy())
    njev = 1
    if jac_scaling:
        J_norm = norm(J, axis=0)
        J_norm[J_norm == 0] = 1
        scale = 1 / J_norm
    Delta = norm(x0 / scale, ord=np.inf)
    if Delta == 0:
        Delta = 1.0
    on_bound = np.zeros(x0.shape, dtype=np.int64)
    on_bound[np.equal(x0, lb)] = -1
    on_bound[np.equal(x0, ub)] = 1
    x = x0.copy()
    obj_value = np.dot(f, f)
    g_norm = 0.0
    termination_status = None
    while nfev < max_nfev:
        if jac_scaling:
            J_norm = norm(J, axis=0)
            with np.errstate(divide='ignore'):
                new_scale = np.minimum(scale, 1 / J_norm)
            log.append(dict(kind='scale', changed=int(np.sum(new_scale != scale)),
                            kept=int(np.sum(new_scale == scale))))
            scale = new_scale
        F = orc.dogbox_factor(J, f, x, lb, ub, scale, on_bound)
        top = dict(kind='top', cmp=[], tags=set(), start_on_bound=on_bound.copy(), active=F.active.copy())
        if F.all_active:
            g_norm = 0.0
            termination_status = 1
            top['tags'].add('all-active')
        else:
            g_norm = F.g_norm
            top['cmp'].append(('gtol', g_norm, gtol))
            if g_norm < gtol:
                termination_status = 1
        log.append(top)
        if termination_status is not None:
            top['tags'].add('status%d' % termination_status)
            return dict(x=x, f=f, obj=float(obj_value), optimality=float(g_norm), nfev=nfev, njev=njev,
                        on_bound=on_bound, status=termination_status)
        actual_reduction = -1.0
        while actual_reduction <= 0 and nfev < max_nfev:
            S = orc.dogbox_step(F, Delta, on_bound)
            screened = probe(S, J, f, x, scale, Delta, None, on_bound) if probe else None
            step, x_new, tr_hit = S.step, S.x_new, S.tr_hit
            predicted_reduction = S.predicted_reduction
            f_new = yield ('trial', Trial(x_new, step, predicted_reduction, 0.0, obj_value, f, x))
            nfev += 1
            obj_value_new = np.dot(f_new, f_new)
            actual_reduction = obj_value - obj_value_new
            if predicted_reduction > 0:
                ratio = actual_reduction / predicted_reduction
            else:
                ratio = 0
            tags = set()
            rec = dict(kind='trial', ratio=float(ratio), tags=tags, Delta=float(Delta), fallback=S.fallback,
                       pred=float(predicted_reduction), obj=float(obj_value))
            if screened is not None:
                rec['screen'] = screened
            if ratio < 0.25:
                Delta = 0.25 * norm(step / scale, ord=np.inf)
                tags.add('shrink')
            elif ratio > 0.75 and tr_hit:
                Delta *= 2.0
                tags.update(('double', 'tr_hit'))
            elif ratio > 0.75:
                tags.add('good-but-inside')
            elif ratio >= 0.25:
                tags.add('keep')
            ftol_satisfied = (abs(actual_reduction) < ftol * obj_value and ratio > 0.25)
            xn = norm(x / scale, ord=np.inf)
            xtol_rhs = xtol * max(EPS ** 0.5, xn)
            xtol_satisfied = Delta < xtol_rhs
            rec['cmp'] = [('ftol', abs(actual_reduction), ftol * obj_value), ('xtol', Delta, xtol_rhs)]
            rec['xtol_arm'] = 'eps' if EPS ** 0.5 > xn else 'x'
            if ftol_satisfied and xtol_satisfied:
                termination_status = 4
            elif ftol_satisfied:
                termination_status = 2
            elif xtol_satisfied:
                termination_status = 3
            if math.isnan(actual_reduction):
                tags.add('nan')
            elif actual_reduction == 0:
                tags.add('exact-zero')
            log.append(rec)
            if not actual_reduction > 0:
                if not math.isnan(actual_reduction):
                    tags.add('reject')
                if termination_status is not None:
                    tags.add('pending-on-reject')
                yield ('judged', _snapshot(x, f, obj_value, g_norm, nfev, njev, on_bound, False))
            if termination_status is not None:
                break
        if actual_reduction > 0:
            on_bound = S.on_bound_new.copy()
            x = x_new.copy()
            mask = on_bound == -1
            if np.any(mask & (x != lb)) or np.any((on_bound == 1) & (x != ub)):
                rec['tags'].add('snap')                 # the snap moved x (by an ulp or more)
            rec['on_bound_hit'] = bool(np.any(on_bound != 0))
            x[mask] = lb[mask]
            mask = on_bound == 1
            x[mask] = ub[mask]
            f = f_new
            obj_value = obj_value_new
            yield ('judged', _snapshot(x, f, obj_value, g_norm, nfev, njev + 1, on_bound, True))
            J = yield ('jac', x)
            njev += 1
    log.append(dict(kind='end', tags={'status0'} | ({'status-lost-to-max_nfev'} if termination_status is not None
                                                      else set())))
    return dict(x=x, f=f, obj=float(obj_value), optimality=float(g_norm), nfev=nfev, njev=njev, on_bound=on_bound,
                status=0)


class ShadowBatch:
    """B scripted problems in lock-step.  The protocol mirrors OuterDriver's:

        sb.start()                    -> sb.F0 (B, m), sb.J0 (B, m, n) to upload before begin()
        sb.propose()                  -> (active (B,) bool, x_trial (B, n), step_norm (B,))
        sb.f_trials()                 -> (B, m) scripted f_trial, NaN rows for problems that are done
        sb.judge(f_trial)             -> (accepted (B,) bool, expected fetch (dict of arrays), fresh J {b: (m, n)})
    """

    def __init__(self, method, m, X0, lb, ub, scale, tols, max_nfev, scripts, seed, J0_mod=None, J0_class=None,
                 ids=None):
        self.method = method
        X0, lb, ub = np.array(X0, dtype=float), np.array(lb, dtype=float), np.array(ub, dtype=float)
        scale = None if scale is None else np.array(scale, dtype=float)
        J0_mod = J0_mod or {}
        J0_class = list(J0_class) if J0_class is not None else ["well"] * len(X0)
        self.ids = list(range(len(X0))) if ids is None else [int(i) for i in ids]
        if ids is not None:                          # the rows `ids` of the batch, with the streams they have there
            X0, lb, ub = X0[self.ids], lb[self.ids], ub[self.ids]
            scale = None if scale is None else scale[self.ids]
            scripts = [scripts[i] for i in self.ids]
            J0_mod = {k: J0_mod[i] for k, i in enumerate(self.ids) if i in J0_mod}
            J0_class = [J0_class[i] for i in self.ids]
        self.X0 = X0
        self.B, self.n = self.X0.shape
        self.m = m
        self.lb, self.ub = lb, ub
        self.jac_scaling = scale is None
        self.scale = np.ones((self.B, self.n)) if scale is None else scale
        self.ftol, self.xtol, self.gtol = tols
        self.max_nfev = max_nfev
        self.scripts = scripts
        self.seed = seed
        self.J0_mod = J0_mod
        self.J0_class = J0_class
        self.screen = 0
        self.trf = method == 'trf'
        if self.trf:
            self.Xs = np.stack([orc.nudge_inside(self.X0[b], self.lb[b], self.ub[b], rstep=1e-10)
                                for b in range(self.B)])
        else:
            self.Xs = self.X0.copy()

    # ---- the scripted callbacks --------------------------------------------------------------------
    def _f_trial(self, b, t):
        move = self.scripts[b][self.pos[b] % len(self.scripts[b])]
        self.pos[b] += 1
        self.mods[b] = ()
        if isinstance(move, tuple):
            move, self.mods[b] = move[0], move[1:]
        self.moves[b] = move
        if move == "same":
            return t.f.copy()
        if move == "nan":
            ft = t.f.copy()
            ft[int(self.rng[b].integers(self.m))] = np.nan
            return ft
        r = float(move)
        assert t.pred > 0, (b, t.pred)
        target = t.obj - (t.corr + r * t.pred)
        assert target > 0, (b, r, target)
        u = self.rng[b].standard_normal(self.m)
        return u * math.sqrt(target / np.dot(u, u))

    def _class_J(self, b, cls):
        """A J of conditioning class `cls` from the problem's own stream ("well": the Gaussian draw)."""
        rng, m, n = self.rng[b], self.m, self.n
        if cls == "well":
            return rng.standard_normal((m, n))
        U, _ = np.linalg.qr(rng.standard_normal((m, n)))      # (_geometry_cases._logspaced)
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return (U * np.logspace(0, -np.log10(KAPPA[cls]), n)) @ V.T * np.sqrt(m)

    def _fresh_J(self, b, f):
        mods = self.mods[b]
        new = "well"
        if "kappa" in mods:
            new = mods[mods.index("kappa") + 1]
            if new == "next":
                new = KAPPA_CYCLE[(KAPPA_CYCLE.index(self.cls[b]) + 1) % len(KAPPA_CYCLE)]
        self.refreshes.append((self.rounds, self.ids[b], self.cls[b], new))
        self.cls[b] = new
        J = self._class_J(b, new)
        if "cols" in mods:
            J = J * 10.0 ** self.rng[b].choice([-1.0, 1.0], size=self.n)
        if "orth" in mods:
            J = J - np.outer(f, f.dot(J)) / np.dot(f, f)
        return np.ascontiguousarray(J)

    def _probe(self, b):
        """The sensitivity screen of one trial (see the module's docstring); None when the screen is off."""
        if not self.screen:
            return None
        import _geometry_cases as gc

        def probe(S, J, f, x, scale, Delta, alpha, on_bound):
            move, same = 0.0, True
            for pat in range(self.screen):
                Jp = gc.one_ulp(J, pat)
                if self.trf:
                    T = orc.trf_step(orc.trf_factor(Jp, f, x, self.lb[b], self.ub[b], scale), Delta, alpha)
                    same = same and gc.trf_same(S, T)
                else:
                    T = orc.dogbox_step(orc.dogbox_factor(Jp, f, x, self.lb[b], self.ub[b], scale, on_bound), Delta,
                                        on_bound)
                    same = same and gc.dog_same(S, T)
                move = max(move, float(norm(T.step - S.step) / norm(S.step)))
            return move, same
        return probe

    def _first_J(self, b, f, x0):
        J = self._class_J(b, self.cls[b])
        mod = self.J0_mod.get(b)
        if mod is not None:                      # wanted sign of the gradient per variable (0: leave)
            g = J.T.dot(f)
            flip = (np.sign(g) * mod) < 0
            J[:, flip] *= -1
        return np.ascontiguousarray(J)

    # ---- generator plumbing ------------------------------------------------------------------------
    def _advance(self, b, value):
        """send `value`, run to the next trial; returns the ('judged', snapshot) met on the way, if any"""
        snap = None
        fresh = None
        try:
            ev = self.gen[b].send(value)
            while ev[0] != 'trial':
                if ev[0] == 'judged':
                    snap = ev[1]
                    ev = self.gen[b].send(None)
                elif ev[0] == 'jac':
                    fresh = self._fresh_J(b, self.cur_f[b])
                    ev = self.gen[b].send(fresh)
                else:
                    raise AssertionError(ev[0])
            self.trial[b] = ev[1]
        except StopIteration as stop:
            self.trial[b] = None
            self.result[b] = dict(stop.value, accepted=False)
        return snap, fresh

    def start(self):
        B, m, n = self.B, self.m, self.n
        loop = trf_loop if self.trf else dogbox_loop
        self.log = [[] for _ in range(B)]
        self.rng = [np.random.default_rng([self.seed, i]) for i in self.ids]
        self.cls = list(self.J0_class)
        self.refreshes = []
        self.classes = []
        self.pos = [0] * B
        self.mods = [()] * B
        self.moves = [None] * B
        self.trial = [None] * B
        self.result = [None] * B
        self.cur_f = [None] * B
        self.gen = []
        self.F0 = np.empty((B, m))
        self.J0 = np.empty((B, m, n))
        self.rounds = 0
        for b in range(B):
            sc = None if self.jac_scaling else self.scale[b]
            g = loop(self.X0[b], self.lb[b], self.ub[b], self.ftol, self.xtol, self.gtol, self.max_nfev, sc,
                     self.log[b], self._probe(b))
            self.gen.append(g)
            ev = next(g)
            assert ev[0] == 'fun'
            self.F0[b] = self.rng[b].standard_normal(m)
            self.cur_f[b] = self.F0[b]
            ev = g.send(self.F0[b].copy())
            assert ev[0] == 'jac'
            self.J0[b] = self._first_J(b, self.F0[b], self.X0[b])
            self._advance(b, self.J0[b].copy())

    def done(self):
        return np.array([t is None for t in self.trial])

    def propose(self):
        act = ~self.done()
        xt = np.stack([self.trial[b].x_new if act[b] else self.result[b]['x'] for b in range(self.B)])
        sn = np.array([norm(self.trial[b].step) if act[b] else 0.0 for b in range(self.B)])
        return act, xt, sn

    def current_x(self):
        return np.stack([self.trial[b].x if self.trial[b] is not None else self.result[b]['x']
                         for b in range(self.B)])

    def f_trials(self):
        ft = np.full((self.B, self.m), np.nan)
        for b in range(self.B):
            if self.trial[b] is not None:
                ft[b] = self._f_trial(b, self.trial[b])
        return ft

    def judge(self, ft):
        B = self.B
        self.classes.append({self.ids[b]: self.cls[b] for b in range(B) if self.trial[b] is not None})
        self.rounds += 1
        states, fresh = [None] * B, {}
        for b in range(B):
            if self.trial[b] is None:
                states[b] = self.result[b]
                continue
            self.cur_f[b] = ft[b]
            self.log[b].append(dict(kind='move', move=self.moves[b]))
            snap, J = self._advance(b, ft[b].copy())
            assert snap is not None
            states[b] = snap
            if J is not None:
                fresh[b] = J
        exp = {k: np.array([s[k] for s in states]) for k in ('x', 'f', 'obj', 'optimality', 'nfev', 'njev',
                                                             'on_bound', 'status')}
        acc = np.array([s['accepted'] for s in states])
        return acc, exp, fresh

    def final(self):
        assert self.done().all()
        return {k: np.array([r[k] for r in self.result]) for k in ('x', 'f', 'obj', 'optimality', 'nfev', 'njev',
                                                                   'on_bound', 'status')}

    def branch_counts(self):
        """how often each branch tag was taken, over all problems"""
        counts = {}
        for log in self.log:
            for rec in log:
                for t in rec.get('tags', ()):
                    counts[t] = counts.get(t, 0) + 1
        return counts

    def run_alone(self):
        """The whole script without a device (test_outer_script_cpu.py)."""
        self.start()
        while True:
            act, _, _ = self.propose()
            if not act.any():
                break
            self.judge(self.f_trials())
        return self.final()


# ---- the configurations the GPU test runs (and the CPU test vets) --------------------------------------
OFF = 0.0                      # a tolerance that never fires: `a < 0` is false for every norm
HUGE = 1e30
BASE = [0.9, 0.5, 0.1, -0.5, "same", 0.1, 0.9, "nan", 0.9, 0.6, 0.95]


def _rot(base, b):
    k = b % len(base)
    return base[k:] + base[:k]


def _mixed_bounds(rng, B, n, x0_mag=None, kinds=(0, 1, 2, 3, 4, 5)):
    """The batch mix of the decision table, by kinds[b % len(kinds)]: 0 unbounded; 1 lower bounds only; 2 upper bounds
    only; 3 two-sided with x0[0] ON its lower and x0[1] ON its upper bound; 4 x0 = 0 two-sided; 5 two-sided."""
    X0 = rng.standard_normal((B, n))
    if x0_mag is not None:
        X0 = X0 / norm(X0, axis=1)[:, None] * np.asarray(x0_mag)[:, None]
    lo, hi = rng.uniform(0.01, 2.0, (B, n)), rng.uniform(0.01, 2.0, (B, n))
    lb, ub = X0 - lo, X0 + hi
    for b in range(B):
        k = kinds[b % len(kinds)]
        if k == 0:
            lb[b], ub[b] = -np.inf, np.inf
        elif k == 1:
            ub[b] = np.inf
        elif k == 2:
            lb[b] = -np.inf
        elif k == 3:
            lb[b, 0] = X0[b, 0]
            if n > 1:
                ub[b, 1] = X0[b, 1]
        elif k == 4:
            X0[b] = 0.0
            lb[b], ub[b] = -lo[b], hi[b]
    return X0, lb, ub


def _decision(method, scaling, seed):
    B, m, n = 12, 9, 4
    rng = np.random.default_rng([seed, 1])
    X0, lb, ub = _mixed_bounds(rng, B, n)
    scale = None if scaling == 'jac' else 10.0 ** rng.uniform(-2, 2, (B, n))
    base = BASE if scaling != 'jac' else [(0.9, "cols"), 0.5, (0.1, "cols"), -0.5, "same", 0.1, (0.9, "cols"), "nan",
                                          0.9, (0.6, "cols"), 0.95]
    return ShadowBatch(method, m, X0, lb, ub, scale, (OFF, OFF, OFF), 14, [_rot(base, b) for b in range(B)], seed)


def _termination(method, case, seed):
    B, m, n = 12, 9, 4
    rng = np.random.default_rng([seed, 2])
    mag = None
    max_nfev = 14
    if case == 'ftol':                  # status 2 on the first ratio > 0.25; a ratio < 0.25 must not terminate
        tols, base = (HUGE, OFF, OFF), [0.1, -0.5, "same", 0.5, 0.9]
    elif case == 'xtol':                # status 3, also on a rejected step (pending, x unchanged, nfev counted)
        tols, base = (OFF, HUGE, OFF), [-0.5, 0.5, "nan", "same", 0.1, 0.9]
    elif case == 'both':                # status 4 where the ratio allows ftol, else 3
        tols, base = (HUGE, HUGE, OFF), [0.5, 0.9, 0.1, -0.5]
    elif case == 'xtol_arm':            # max(sqrt(eps), ||x||): ||x0|| = 1e-12 (eps arm), 1 (never fires), 1e6 (x arm)
        tols, base, max_nfev = (OFF, 1e-2, OFF), [0.5, 0.1, 0.9, 0.5], 4
        mag = np.array([1e-12, 1.0, 1e6])[np.arange(B) % 3]
    elif case == 'orth':                # J^T f = 0 after the refresh: status 1 at the next top
        tols, base = (OFF, OFF, 1e-8), [-0.5, 0.1, (0.5, "orth"), 0.9]
    elif case == 'lost':                # the status-producing move falls on evaluation number max_nfev: status 0
        tols, base, max_nfev = (HUGE, OFF, OFF), [0.1, -0.5, 0.5, 0.1], 4
    elif case == 'nfev1':               # n_active == 0 at the first propose
        tols, base, max_nfev = (OFF, OFF, OFF), [0.5], 1
    else:
        raise KeyError(case)
    X0, lb, ub = _mixed_bounds(rng, B, n, mag)
    if case == 'xtol_arm':              # keep the three magnitudes (the mix's x0 = 0 rows would lose theirs)
        for b in range(B):
            if b % 6 == 4:
                X0[b] = mag[b] * np.eye(n)[0]
                lb[b], ub[b] = X0[b] - 1.0, X0[b] + 1.0
    return ShadowBatch(method, m, X0, lb, ub, np.ones((B, n)), tols, max_nfev, [_rot(base, b) for b in range(B)], seed)


def _dogbox_starts(seed):
    """Every variable on a bound with the gradient pointing outward (status 1 at nfev 1, b < 4); starts with
    on_bound = +1 and -1 mixed, some of them active and some free (b >= 4); ratios > 0.75 with and without tr_hit."""
    B, m, n = 12, 9, 4
    rng = np.random.default_rng([seed, 3])
    X0 = rng.standard_normal((B, n))
    lb, ub = X0 - rng.uniform(0.5, 2.0, (B, n)), X0 + rng.uniform(0.5, 2.0, (B, n))
    J0_mod = {}
    for b in range(B):
        side = rng.choice([-1, 1], size=n)                   # which bound x0[j] sits on
        if b >= 4:
            side[rng.integers(n)] = 0                        # one variable strictly inside
            side[(b + 1) % n] = 1 if side[(b + 1) % n] != 0 else 0
        lb[b][side == -1] = X0[b][side == -1]
        ub[b][side == 1] = X0[b][side == 1]
        want = -side.astype(float)                           # outward: on_bound * g < 0
        if b >= 4:
            inward = rng.integers(n)
            want[inward] = -want[inward]
        J0_mod[b] = want
    base = [0.9, 0.95, 0.9, 0.5, 0.9, 0.1, 0.9, 0.9]
    return ShadowBatch('dogbox', m, X0, lb, ub, np.ones((B, n)), (OFF, OFF, 1e-8), 10,
                       [_rot(base, b) for b in range(B)], seed, J0_mod)


def _shape(method, B, m, n, seed, max_nfev=14, base=BASE, kinds=(0, 1, 2, 3, 4, 5)):
    rng = np.random.default_rng([seed, 4])
    X0, lb, ub = _mixed_bounds(rng, B, n, kinds=kinds)
    return ShadowBatch(method, m, X0, lb, ub, np.ones((B, n)), (OFF, OFF, OFF), max_nfev,
                       [_rot(base, b) for b in range(B)], seed)


# 300 problems are 300 chances of a near-tie: no start a relative 1e-10 off a bound (there the reflected and the
# gradient step of trf nearly coincide) and no ratio > 0.75 (an interior step has any ||step_h|| / Delta)
BASE_300 = [0.5, 0.1, -0.5, "same", 0.6, "nan", 0.35]


TERMINATION_CASES = ['ftol', 'xtol', 'both', 'xtol_arm', 'orth', 'lost', 'nfev1']

CONFIGS = {}
for _m in ('trf', 'dogbox'):
    for _s in ('given', 'jac'):
        CONFIGS['decision-%s-%s' % (_m, _s)] = (lambda _m=_m, _s=_s: _decision(_m, _s, 11))
    for _c in TERMINATION_CASES:
        CONFIGS['termination-%s-%s' % (_m, _c)] = (lambda _m=_m, _c=_c: _termination(_m, _c, 21))
    CONFIGS['shape-%s-3x300x257' % _m] = (lambda _m=_m: _shape(_m, 3, 300, 257, 31))
    CONFIGS['shape-%s-4x1x1' % _m] = (lambda _m=_m: _shape(_m, 4, 1, 1, 34))


# ---- one configuration per factorisation route a masked factor call can take (test_outer_route_gpu.py) -------------
# route -> (library switches, shapes, whether the conditioning cycle is played)
ROUTES = {
    "rl":    ({},                ((160, 96), (300, 256)), False),
    "tree":  ({"gram": 0},       ((160, 96),),            False),
    "svd":   ({"no_svdfree": 1}, ((90, 33),),             False),
    "short": ({},                ((40, 60),),             False),
    "tier":  ({},                ((600, 96),),            True),
    "cqr2":  ({"csne": 0},       ((600, 96),),            True),
}
ROUTE_NFEV = 12
# the cycle's scripts: every move that can be accepted advances the problem's class.  Rotation and first class per
# problem were searched (on the accept pattern of BASE alone, no numbers involved) for the coverage that
# test_outer_script_cpu.py::test_conditioning_cycle_covers_the_masked_branches asserts.
CYCLE_BASE = [(mv, "kappa", "next") if isinstance(mv, float) else mv for mv in BASE]
CYCLE_ROT = (1, 3, 4, 6, 8, 9)
CYCLE_START = ("beyond", "beyond", "tier", "well", "tier", "beyond")


def _route_bounds(method, route, rng, B, n):
    cycle = ROUTES[route][2]
    if not cycle:
        if method == 'trf' and route == 'short':
            # m < n: without bounds the augmented matrix of trf.py:264-268 has rank m and, with Delta beyond the
            # minimum-norm step, the reference's own step is decided by LAPACK's null-space outputs (noise,
            # not a parity case); with two-sided bounds and a carried alpha its sub-problem solver leaves the bracket
            # and raises (trust_region.py:28-35, cf. _geometry_cases.RAISED).  One-sided bounds: about half the
            # variables are regularised by the Coleman-Li block, the matrix has full column rank
            # (test_outer_script_cpu.py::test_short_trf_steps_are_determined holds every trial to that)
            return _mixed_bounds(rng, B, n, kinds=(1, 2))
        return _mixed_bounds(rng, B, n, kinds=(0, 1, 2, 3, 4, 5) if B >= 6 else (0, 1, 2))
    if method == 'trf':                         # the bound kinds the tier takes: unbounded and upper bounds only
        return _mixed_bounds(rng, B, n, kinds=(0, 2))
    # dogbox: unbounded, and wide two-sided bounds with a tenth of the variables sitting on the lower one
    X0 = rng.standard_normal((B, n))
    lb, ub = X0 - rng.uniform(50.0, 500.0, (B, n)), X0 + rng.uniform(50.0, 500.0, (B, n))
    for b in range(B):
        if b % 2 == 0:
            lb[b], ub[b] = -np.inf, np.inf
        else:
            idx = rng.choice(n, n // 10, replace=False)
            X0[b, idx] = lb[b, idx]
    return X0, lb, ub


def _route(method, route, m, n, seed, ids=None):
    cycle = ROUTES[route][2]
    B = 3 if n >= 256 else 6
    rng = np.random.default_rng([seed, 5])
    X0, lb, ub = _route_bounds(method, route, rng, B, n)
    if cycle:
        scripts = [_rot(CYCLE_BASE, CYCLE_ROT[b]) for b in range(B)]
        start = CYCLE_START[:B]
    else:                                       # (B = 6: rotations that leave accepts AND rejects in every round)
        scripts = [_rot(BASE, k) for k in ((0, 1, 2, 3, 4, 6) if B >= 6 else (0, 3, 6))]
        start = None
    return ShadowBatch(method, m, X0, lb, ub, np.ones((B, n)), (OFF, OFF, OFF), ROUTE_NFEV, scripts, seed,
                       J0_class=start, ids=ids)


ROUTE_SEED = 51
for _m in ('trf', 'dogbox'):
    for _r, (_o, _shapes, _c) in ROUTES.items():
        for (_mm, _nn) in _shapes:
            CONFIGS['route-%s-%s-%dx%d' % (_m, _r, _mm, _nn)] = (
                lambda ids=None, _m=_m, _r=_r, _mm=_mm, _nn=_nn: _route(_m, _r, _mm, _nn, ROUTE_SEED, ids))
CONFIGS['shape-trf-300x6x3'] = lambda: _shape('trf', 300, 6, 3, 32, max_nfev=8, base=BASE_300, kinds=(0, 1, 2, 4, 5))
CONFIGS['starts-dogbox'] = lambda: _dogbox_starts(41)


def method_of(name):
    return 'dogbox' if 'dogbox' in name else 'trf'


def route_of(name):
    """The route of a 'route-<method>-<route>-<m>x<n>' configuration (None for the others)."""
    parts = name.split('-')
    return parts[2] if parts[0] == 'route' else None
