"""Writes tests/golden/expr_truth.npz: the truth the expression-model tests are held to.

For every case of tests/_expr_cases.py: the model value and its derivatives from sympy's symbolic differentiation of
the formula, evaluated by mpmath at 50 digits at the float64 inputs (taken exactly) and rounded to float64; and the
magnitudes of ``_expr_cases.magnitudes`` rounded to float32.  Needs sympy and mpmath; nothing of the library.

    python tools/make_expr_truth.py              write the file
    python tools/make_expr_truth.py --measure    print K_ref per case: max |numpy definition - truth| / (eps mag)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bounded-lsq_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIGITS = 50


def true_values(name, P, t, rows=None):
    """(f (B, m), J (B, m, n)) of case `name` at P (B, n) and t (m,), rounded to float64; `rows`: the indices of t to
    evaluate (default: all)."""
    import mpmath
    import sympy
    import _expr_cases as ec
    params, text, _ = ec.CASES[name]
    names = params.split()
    syms = {nm: sympy.Symbol(nm, real=True) for nm in names + ["t"]}
    expr = sympy.sympify(text, locals=dict(syms, pi=sympy.pi))
    funcs = [expr] + [sympy.diff(expr, syms[nm]) for nm in names]
    call = sympy.lambdify([syms[nm] for nm in names] + [syms["t"]], funcs, modules="mpmath")
    rows = range(len(t)) if rows is None else rows
    f = np.empty((P.shape[0], len(rows)))
    J = np.empty((P.shape[0], len(rows), len(names)))
    with mpmath.workdps(DIGITS):
        for b in range(P.shape[0]):
            args = [mpmath.mpf(float(v)) for v in P[b]]
            for c, i in enumerate(rows):
                out = call(*args, mpmath.mpf(float(t[i])))
                f[b, c] = float(out[0])
                J[b, c] = [float(v) for v in out[1:]]
    return f, J


def generate(names=None):
    """{'case.key': array} for the golden file."""
    import _expr_cases as ec
    out = {}
    for name in (ec.CASES if names is None else names):
        P, t = ec.draw(name)
        f, J = true_values(name, P, t)
        fmag, Jmag = ec.magnitudes(ec.model(name).program, [t], P)
        for k, a in (("P", P), ("t", t), ("f", f), ("J", J), ("fmag", fmag.astype(np.float32)),
                     ("Jmag", Jmag.astype(np.float32))):
            out["%s.%s" % (name, k)] = a
    return out


def measure():
    import _expr_cases as ec
    tr = ec.truth()
    for name in ec.CASES:
        d, M = tr[name], ec.model(name)
        kf = ec.excess(M.f(d["t"], d["P"]), d["f"], d["fmag"])
        kj = ec.excess(M.jac(d["t"], d["P"]), d["J"], d["Jmag"])
        print("%-14s nops %2d  K_ref f %.3f  J %.3f  -> %.3f" % (name, M.program.nops, kf, kj, max(kf, kj)))


if __name__ == "__main__":
    import _expr_cases as ec
    if "--measure" in sys.argv[1:]:
        measure()
    else:
        np.savez_compressed(ec.GOLDEN, **generate())
        print("%s: %d bytes" % (ec.GOLDEN, os.path.getsize(ec.GOLDEN)))
