"""Inputs shared by tests/test_param_map_cpu.py and tests/test_param_map_gpu.py: the maps of the kernel-level
comparisons, and the end-to-end fit problems with fixed and tied parameters together with their reduced models written
out by hand (no ParamMap, no bounded_lsq.models: an independent statement of what a user would write today)."""
import numpy as np

from bounded_lsq import models

import _model_cases as mc

# ---- kernel level: name -> n, and the maps (id, fixed, tied) ---------------------------------------------------------
KERNEL_N = {"poly": 7, "exp_sum": 7, "gauss_sum": 10, "lorentz_sum": 10, "gauss2d": 5}


def kernel_maps(name):
    """first parameter fixed; last (offset) fixed; all but one fixed (nf = 1); one tie; a three-member tie; fixed and
    tied mixed; a tie across terms; a tie whose key lies before its target (the slot's first column is then not its
    leader's); for gauss2d the centres fixed."""
    n = KERNEL_N[name]
    maps = [("first_fixed", [0], {}), ("last_fixed", [n - 1], {}),
            ("all_but_one", [j for j in range(n) if j != 1], {})]
    if name == "gauss2d":
        maps += [("tie", [], {2: 1}), ("tie3", [], {2: 1, 3: 1}), ("mixed", [4], {2: 1}), ("key_first", [0], {1: 3}),
                 ("centres_fixed", [1, 2], {})]
    elif name in ("gauss_sum", "lorentz_sum"):
        maps += [("tie_in_term", [], {2: 1}), ("tie_across", [], {5: 2}), ("tie3", [], {5: 2, 8: 2}),
                 ("mixed", [1, 4, 9], {5: 2, 8: 2, 6: 0}), ("key_first", [3], {1: 7, 4: 7})]
    else:                                            # poly, exp_sum: n = 7
        maps += [("tie", [], {3: 1}), ("tie3", [], {3: 1, 5: 1}), ("mixed", [0, 6], {4: 2, 5: 3}),
                 ("key_first", [2], {0: 4, 1: 4})]
    return maps


def edge_map(nf, n=64):
    """gauss_sum at n = 64 with nf variables: nf = 63 by one tie, otherwise n - nf parameters fixed, spread over the
    terms by the bijection j -> 37 j mod 64."""
    if nf == n - 1:
        return [], {5: 2}
    return [j for j in range(n) if (37 * j) % n < n - nf], {}


def explicit_reduce_jac(J_full, pmap, nf):
    """The definition of J_map as three nested loops over plain floats."""
    J_full = np.asarray(J_full)
    lead = J_full.shape[:-1]
    Jf = J_full.reshape(-1, J_full.shape[-1])
    out = np.zeros((Jf.shape[0], nf), dtype=J_full.dtype)
    for r in range(Jf.shape[0]):
        for k in range(nf):
            first = True
            for j in range(len(pmap)):
                if pmap[j] == k:
                    out[r, k] = Jf[r, j] if first else out[r, k] + Jf[r, j]
                    first = False
    return out.reshape(lead + (nf,))


# ---- end to end: the reduced models by hand -------------------------------------------------------------------------
def _c(A, k):
    return A[:, k, np.newaxis]


def _gauss(t, a, mu, s):
    """term, d/da, d/dmu, d/ds of a exp(-((t - mu) / s)^2 / 2)"""
    z = (t - mu) / s
    e = np.exp(-0.5 * z * z)
    return a * e, e, a * e * z / s, a * e * z * z / s


def _lorentz(t, a, mu, s):
    z = (t - mu) / s
    e = 1.0 / (1.0 + z * z)
    return a * e, e, 2 * a * e * e * z / s, 2 * a * e * e * z * z / s


def _stack(t, cols):
    return np.stack([c + 0 * t for c in cols], axis=-1)


def red_poly4_fix0(t, X, F):                     # X = (p1, p2, p3); p0 = F[:, 0]
    f = _c(F, 0) + _c(X, 0) * t + _c(X, 1) * t ** 2 + _c(X, 2) * t ** 3
    return f, _stack(f, [t, t ** 2, t ** 3])


def red_exp1_fix1(t, X, F):                      # X = (a, c); r = F[:, 1]
    e = np.exp(-_c(F, 1) * t)
    f = _c(X, 0) * e + _c(X, 1)
    return f, _stack(f, [e, 1.0])


def red_exp2_fix4(t, X, F):                      # X = (a1, r1, a2, r2); c = F[:, 4]
    e1, e2 = np.exp(-_c(X, 1) * t), np.exp(-_c(X, 3) * t)
    f = _c(X, 0) * e1 + _c(X, 2) * e2 + _c(F, 4)
    return f, _stack(f, [e1, -t * _c(X, 0) * e1, e2, -t * _c(X, 2) * e2])


def red_gauss1_fix2(t, X, F):                    # X = (a, mu, c); s = F[:, 2]
    g, da, dmu, ds = _gauss(t, _c(X, 0), _c(X, 1), _c(F, 2))
    f = g + _c(X, 2)
    return f, _stack(f, [da, dmu, 1.0])


def red_gauss2_tie52(t, X, F):                   # X = (a1, mu1, s, a2, mu2, c): one width for both peaks
    g1, da1, dmu1, ds1 = _gauss(t, _c(X, 0), _c(X, 1), _c(X, 2))
    g2, da2, dmu2, ds2 = _gauss(t, _c(X, 3), _c(X, 4), _c(X, 2))
    f = g1 + g2 + _c(X, 5)
    return f, _stack(f, [da1, dmu1, ds1 + ds2, da2, dmu2, 1.0])


def red_gauss2_fix14_tie52(t, X, F):             # X = (a1, s, a2, c); mu1 = F[:, 1], mu2 = F[:, 4]
    g1, da1, dmu1, ds1 = _gauss(t, _c(X, 0), _c(F, 1), _c(X, 1))
    g2, da2, dmu2, ds2 = _gauss(t, _c(X, 2), _c(F, 4), _c(X, 1))
    f = g1 + g2 + _c(X, 3)
    return f, _stack(f, [da1, ds1 + ds2, da2, 1.0])


def red_gauss2_fix_peaks(t, X, F):               # X = (c,): both peaks known
    g1 = _gauss(t, _c(F, 0), _c(F, 1), _c(F, 2))[0]
    g2 = _gauss(t, _c(F, 3), _c(F, 4), _c(F, 5))[0]
    f = g1 + g2 + _c(X, 0)
    return f, _stack(f, [1.0])


def red_lorentz1_fix3(t, X, F):                  # X = (a, mu, s); c = F[:, 3]
    g, da, dmu, ds = _lorentz(t, _c(X, 0), _c(X, 1), _c(X, 2))
    f = g + _c(F, 3)
    return f, _stack(f, [da, dmu, ds])


def _spot(x, a, u0, v0, s):
    du, dv = x[..., 0, :] - u0, x[..., 1, :] - v0
    r2 = du * du + dv * dv
    e = np.exp(-0.5 * r2 / (s * s))
    return a * e, e, a * e * du / (s * s), a * e * dv / (s * s), a * e * r2 / s ** 3


def red_gauss2d_fix4(x, X, F):                   # X = (a, u0, v0, s); c = F[:, 4]
    g, da, du0, dv0, ds = _spot(x, _c(X, 0), _c(X, 1), _c(X, 2), _c(X, 3))
    f = g + _c(F, 4)
    return f, _stack(f, [da, du0, dv0, ds])


def red_gauss2d_fix12(x, X, F):                  # X = (a, s, c); centre = F[:, 1:3]
    g, da, du0, dv0, ds = _spot(x, _c(X, 0), _c(F, 1), _c(F, 2), _c(X, 1))
    f = g + _c(X, 2)
    return f, _stack(f, [da, ds, 1.0])


# label, fixed, tied, the reduced model, and the solver variables as lists of the full parameters that share each
# (written out, not derived: the first of a list carries the start value)
E2E_CASES = [
    ("poly4", [0], {}, red_poly4_fix0, [[1], [2], [3]]),
    ("exp1", [1], {}, red_exp1_fix1, [[0], [2]]),
    ("exp2", [4], {}, red_exp2_fix4, [[0], [1], [2], [3]]),
    ("gauss1", [2], {}, red_gauss1_fix2, [[0], [1], [3]]),
    ("gauss2", [], {5: 2}, red_gauss2_tie52, [[0], [1], [2, 5], [3], [4], [6]]),
    ("gauss2", [1, 4], {5: 2}, red_gauss2_fix14_tie52, [[0], [2, 5], [3], [6]]),
    ("gauss2", [0, 1, 2, 3, 4, 5], {}, red_gauss2_fix_peaks, [[6]]),
    ("lorentz1", [3], {}, red_lorentz1_fix3, [[0], [1], [2]]),
    ("gauss2d", [4], {}, red_gauss2d_fix4, [[0], [1], [2], [3]]),
    ("gauss2d", [1, 2], {}, red_gauss2d_fix12, [[0], [3], [4]]),
]
E2E_IDS = ["%s-fixed%s-tied%s" % (c[0], "".join(map(str, c[1])) or "none",
                                  "".join("%d%d" % kv for kv in c[2].items()) or "none") for c in E2E_CASES]


def mapped_problem(label, m, fixed, tied, groups, B=8):
    """`_model_cases.fit_problem(label, m)` with the truth made to satisfy the ties, Y regenerated from it as
    model.f(x, truth) + 0.01 N(0, 1) (seeded) and P0 at the truth in the fixed columns.  Adds the reduced start X0 and
    the reduced box (the intersection over each group, written as max / min over its columns)."""
    pr = mc.fit_problem(label, m, B=B)
    truth = pr["truth"].copy()
    for j, i in tied.items():
        truth[:, j] = truth[:, i]
    rng = np.random.default_rng([7, m, len(fixed), len(tied)])
    pr["truth"] = truth
    pr["Y"] = models.get(pr["name"]).f(pr["x"], truth) + mc.SIGMA * rng.standard_normal((B, m))
    P0 = pr["P0"].copy()
    P0[:, fixed] = truth[:, fixed]
    pr["P0"] = P0
    lb, ub = pr["bounds"]
    pr["X0"] = np.stack([P0[:, g[0]] for g in groups], axis=1)
    pr["bounds_red"] = (np.stack([lb[:, g].max(axis=1) for g in groups], axis=1),
                        np.stack([ub[:, g].min(axis=1) for g in groups], axis=1))
    return pr


def reduced_callables(red, F):
    """Batch callables f(x, X) -> (B, m), jac(x, X) -> (B, m, nf) of a hand-written reduced model, the fixed values
    taken from F (B, n); and per-problem ones for scipy."""
    def f(x, X):
        return red(x, X, F)[0]

    def jac(x, X):
        return red(x, X, F)[1]

    def single(b):
        Fb = F[b:b + 1]
        return (lambda x, *p: red(x, np.asarray(p)[np.newaxis], Fb)[0][0],
                lambda x, *p: red(x, np.asarray(p)[np.newaxis], Fb)[1][0])
    return f, jac, single
