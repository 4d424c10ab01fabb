"""The cases, the magnitudes and the tolerance of the expression-model tests, shared by
tests/test_expr_cpu.py, tests/test_expr_gpu.py and tools/make_expr_truth.py.

Truth.  tests/golden/expr_truth.npz (written by tools/make_expr_truth.py: sympy's symbolic derivatives evaluated by
mpmath at 50 digits) holds, per case, P (3, n), t (130,), the true f (3, 130) and J (3, 130, n) rounded to float64 and
the magnitudes fmag, Jmag as float32.

Magnitudes.  ``magnitudes(prog, T, X)`` runs the forward and the reverse sweep of the definition with absolute values at
every leaf, sum and contribution, as a first-order running bound on the rounding error: nothing cancels, and the error
an argument already carries passes through a function with the function's slope.  E is the forward magnitude (of a
leaf: |x|), v the value, G the adjoint magnitude; a push adds the absolute value it is given:
    forward   ADD, SUB  Ea + Eb       MUL  Ea Eb       DIV  (Ea / |vb|) (Eb / |vb|)       NEG  Ea
              a function h  |v| + |h'(va)| Ea   (EXP |v| (1 + Ea); LOG |v| + Ea / |va|; SQRT |v| + Ea / (2 |v|);
              SIN |v| + |cos va| Ea; COS |v| + |sin va| Ea; ATAN |v| + Ea / (1 + va^2); ERF, ERFC |v| + C exp(-va^2) Ea;
              POWC |v| + |c| |va|^(c-1) Ea)
    reverse   seed 1;  ADD, SUB  G, G     MUL  G Eb, G Ea     DIV  (G / |vb|) (Eb / |vb|),  (G E / |vb|) (Eb / |vb|)
              NEG G     EXP G E     LOG (G / |va|) (Ea / |va|)     SQRT (G / (2 |v|)) (E / |v|)
              SIN G (|cos va| + |sin va| Ea)     COS G (|sin va| + |cos va| Ea)
              ATAN (G / (1 + va^2)) (1 + 2 |va| Ea / (1 + va^2))     ERF, ERFC  G C exp(-va^2) (1 + 2 |va| Ea)
              POWC G |c| (|va|^(c-1) + |c - 1| |va|^(c-2) Ea)
fmag is E of the root and Jmag the row the pushes leave.  A deterministic function of (program, t, P) in float64; the
file keeps it rounded to float32, which is what both tests use (eight digits of a bound are plenty).

Tolerance.  K_REF[case] is the measured max |numpy definition - truth| / (eps mag) over f and J of the case, rounded
up: the reference arithmetic against the truth.  The CPU test holds the definition to it; the GPU test holds the device
to 4 max(K_REF, 1) eps mag against the same truth, the factor 4 because the device runs the definition's operations and
differs only in the last bits of exp, log, sin, cos, atan, erf, erfc and pow.
"""
import os

import numpy as np

from bounded_lsq import _expr, models

EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expr_truth.npz")
B, POINTS, T_LO, T_HI = 3, 130, -1.0, 3.0

# name -> (params, text, (lo, hi) of each parameter's uniform draw)
CASES = {
    "gauss2_line": ("a1 m1 s1 a2 m2 s2 c0 c1", "a1*exp(-((t-m1)/s1)**2/2)+a2*exp(-((t-m2)/s2)**2/2)+c0+c1*t",
                    [(1, 3), (-0.5, 0.5), (0.2, 0.6), (1, 3), (1.5, 2.5), (0.3, 0.8), (0.1, 1), (-0.3, 0.3)]),
    "decay": ("a f1 tau1 tau2 bg", "a*(f1*exp(-t/tau1)+(1-f1)*exp(-t/tau2))+bg",
              [(1, 5), (0.2, 0.8), (0.3, 0.8), (1.5, 4), (0.1, 1)]),
    "emg": ("a m s tau c", "a*0.5*erfc((m-t)/(s*sqrt(2)))*exp(-(t-m)/tau)+c",
            [(1, 5), (-0.2, 0.8), (0.1, 0.4), (0.5, 2), (0.1, 1)]),
    "damped_sine": ("a f ph T2 c", "a*sin(2*pi*f*t+ph)*exp(-t/T2)+c",
                    [(1, 5), (0.5, 3), (-1, 1), (0.8, 3), (0.1, 1)]),
    "stretched": ("a m w b k", "a/(1+((t-m)/w)**2)**1.5+b*log(1+t*t)+atan(k*t)",
                  [(1, 5), (0, 2), (0.2, 0.9), (0.2, 2), (0.5, 3)]),
    # the two without a library function: the device must give the definition's bits
    "lorentz_root": ("a m w c0 c1 b", "a/(1+((t-m)/w)**2)+c0+c1*t+sqrt(b*b+t*t)",
                     [(1, 5), (0, 2), (0.2, 0.9), (0.1, 1), (-0.3, 0.3), (0.3, 2)]),
    "sum64": (" ".join("p%d" % i for i in range(64)), "t*(" + "+".join("p%d" % i for i in range(64)) + ")",
              [(-1, 1)] * 64),
}
FUNCTION_FREE = ("lorentz_root", "sum64")

# Measured on the CPU by tools/make_expr_truth.py --measure (max over f and J; rounded up to two digits).
K_REF = {"gauss2_line": 1.6, "decay": 1.4, "emg": 0.77, "damped_sine": 0.91, "stretched": 0.94, "lorentz_root": 2.7,
         "sum64": 0.25}


def model(name):
    params, text, _ = CASES[name]
    return models.expression(text, tuple(params.split()))


def draw(name):
    """P (B, n) and t (POINTS,) of a case: a fixed draw per case (the golden file stores both)."""
    ranges = CASES[name][2]
    rng = np.random.default_rng(list(CASES).index(name) + 20260)
    P = np.column_stack([rng.uniform(lo, hi, B) for lo, hi in ranges])
    return P, np.linspace(T_LO, T_HI, POINTS)


def magnitudes(prog, T, X, Pfix=None):
    """(fmag (B, m), Jmag (B, m, nf)) of the program at the coordinates T (a list of arrays), in float64."""
    E = _expr
    X = np.asarray(X, dtype=np.float64)
    T = [np.asarray(t, dtype=np.float64) for t in T]
    Bn, m, nf = X.shape[0], T[0].shape[-1], X.shape[1]
    ops = prog.decode()
    val, mag = [None] * len(ops), [None] * len(ops)

    def leaf(o):
        kind, i = o >> 8, o & 0xff
        if kind == E.VAR:
            return X[:, i, np.newaxis]
        if kind == E.PFIX:
            return np.asarray(Pfix, dtype=np.float64)[:, i, np.newaxis]
        if kind == E.CONST:
            return prog.consts[i]
        return T[i]

    def value(o):
        return val[o & 0xff] if o >> 8 == E.TAPE else leaf(o)

    def size(o):
        return mag[o & 0xff] if o >> 8 == E.TAPE else np.abs(leaf(o))

    unary = {E.EXP: np.exp, E.LOG: np.log, E.SQRT: np.sqrt, E.SIN: np.sin, E.COS: np.cos, E.ATAN: np.arctan,
             E.ERF: lambda x: E._erf(x, False), E.ERFC: lambda x: E._erf(x, True)}
    C = E.TWO_BY_SQRT_PI

    def slope(opc, va, v, c):
        """|h'(va)| of the function ops, and |h''(va)| / |h'(va)| (the relative slope of the reverse factor)."""
        ava = np.abs(va)
        if opc == E.EXP:
            return np.abs(v), 1.0
        if opc == E.LOG:
            return 1.0 / ava, 1.0 / ava
        if opc == E.SQRT:
            return 0.5 / np.abs(v), 0.5 / ava
        if opc == E.SIN:
            return np.abs(np.cos(va)), None
        if opc == E.COS:
            return np.abs(np.sin(va)), None
        if opc == E.ATAN:
            return 1.0 / (1 + va * va), 2 * ava / (1 + va * va)
        if opc in (E.ERF, E.ERFC):
            return C * np.exp(-(va * va)), 2 * ava
        return np.abs(c) * np.power(ava, c - 1), np.abs(c - 1) / ava          # POWC

    with np.errstate(all='ignore'):
        for k, (opc, a, b) in enumerate(ops):
            va, ma = value(a), size(a)
            if opc in (E.ADD, E.SUB):
                val[k] = va + value(b) if opc == E.ADD else va - value(b)
                mag[k] = ma + size(b)
            elif opc == E.MUL:
                val[k], mag[k] = va * value(b), ma * size(b)
            elif opc == E.DIV:
                vb = value(b)
                val[k], mag[k] = va / vb, (ma / np.abs(vb)) * (size(b) / np.abs(vb))
            elif opc == E.NEG:
                val[k], mag[k] = -va, ma
            else:
                c = value(b) if opc == E.POWC else None
                val[k] = np.power(va, c) if opc == E.POWC else unary[opc](va)
                mag[k] = np.abs(val[k]) + slope(opc, va, val[k], c)[0] * ma
        fmag = np.array(np.broadcast_to(size(prog.root), (Bn, m)))
        act = prog.active()
        Jmag = np.zeros((Bn, m, nf))
        adj = [np.zeros((Bn, m)) if act[k] else None for k in range(len(ops))]

        def push(o, c):
            kind, i = o >> 8, o & 0xff
            if kind == E.TAPE and act[i]:
                adj[i] = adj[i] + np.abs(c)
            elif kind == E.VAR:
                Jmag[:, :, i] = Jmag[:, :, i] + np.abs(c)

        push(prog.root, 1.0)
        for k in range(len(ops) - 1, -1, -1):
            if not act[k]:
                continue
            opc, a, b = ops[k]
            g, va, ma = adj[k], value(a), size(a)
            if opc in (E.ADD, E.SUB):
                push(a, g)
                push(b, g)
            elif opc == E.MUL:
                push(a, g * size(b))
                push(b, g * ma)
            elif opc == E.DIV:
                vb = np.abs(value(b))
                push(a, (g / vb) * (size(b) / vb))
                push(b, ((g * mag[k]) / vb) * (size(b) / vb))
            elif opc == E.NEG:
                push(a, g)
            elif opc == E.EXP:
                push(a, g * mag[k])
            elif opc == E.SQRT:
                push(a, ((0.5 * g) / np.abs(val[k])) * (mag[k] / np.abs(val[k])))
            elif opc == E.SIN:
                push(a, g * (np.abs(np.cos(va)) + np.abs(np.sin(va)) * ma))
            elif opc == E.COS:
                push(a, g * (np.abs(np.sin(va)) + np.abs(np.cos(va)) * ma))
            elif opc == E.LOG:
                push(a, (g / np.abs(va)) * (ma / np.abs(va)))
            else:                                            # ATAN, ERF, ERFC, POWC: |h'| (1 + (|h''| / |h'|) Ea)
                h1, rel = slope(opc, va, val[k], value(b) if opc == E.POWC else None)
                push(a, g * h1 * (1 + rel * ma))
    return fmag, Jmag


_truth = None


def truth():
    """{case: dict(P, t, f, J, fmag, Jmag)} of the golden file (read once; the arrays are read-only), the magnitudes
    as float64 values of the stored float32."""
    global _truth
    if _truth is None:
        out = {}
        with np.load(GOLDEN) as z:
            for name in CASES:
                d = {k: z["%s.%s" % (name, k)] for k in ("P", "t", "f", "J", "fmag", "Jmag")}
                d["fmag"], d["Jmag"] = d["fmag"].astype(np.float64), d["Jmag"].astype(np.float64)
                for a in d.values():
                    a.setflags(write=False)
                out[name] = d
        _truth = out
    return _truth


def excess(got, want, mag):
    """max |got - want| / (eps mag): the error in units of the tolerance's yardstick; inf where got is not finite or a
    row with mag == 0 is not met exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = np.abs(got - want)
    with np.errstate(all='ignore'):
        r = np.where(d == 0, 0.0, d / (EPS * mag))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


def device_bound(name):
    """The GPU tests' bound in units of eps mag: 4 max(K_REF, 1)."""
    return 4.0 * max(K_REF[name], 1.0)
