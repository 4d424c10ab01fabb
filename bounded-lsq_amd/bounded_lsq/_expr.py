"""Expression models (``models.expression``): a formula written by the user, compiled on the host into a
short straight-line program that the GPU interprets per row (blsq_expr_eval_dev of include/blsq.h,
csrc/expr_kernels.hip); a reverse sweep over the program's tape gives the exact Jacobian row.  Nothing is compiled at
run time, by Python or for the device.

The language.  ``expression(text, params, coords=('t',))``: `text` is parsed with ``ast.parse(text, mode='eval')`` and
walked; it is never evaluated.  Accepted: int and float literals; the names in `params` and `coords`, and ``pi``; binary
``+ - * /`` and unary ``+ -``; ``**`` with a constant exponent; one-argument calls of ``exp log sqrt sin cos atan erf
erfc``.  Anything else is a ValueError naming the construct.

The compile rules (the text is the definition, so they are fixed).  Ops are emitted in post-order, the left operand
first.  Common subexpressions are merged on the key (opcode, a, b).  An op on two constants is folded in float64 and so
is a minus sign on a constant (a function of a constant is an op like any other).  ``x**2`` is ``mul(x, x)``, integer
exponents 3 to 8 repeated ``mul`` from the left (``(x*x)*x``), exponent 1 is ``x``, exponent 0 the constant 1, any
other constant exponent ``POWC``.  Constants are merged on their bits.

The program.  ``Program(ops, consts, root)``: at most MAX_OPS ops and MAX_CONST constants.  An operand is 16 bits, the
kind (``KINDS``) in the high byte and an index in the low one: ``TAPE k`` the result of the earlier op k, ``VAR k``
solver variable k, ``PFIX j`` model parameter j held per problem, ``CONST i`` entry i of `consts`, ``COORD r``
coordinate r.  An op is one 64-bit word: the opcode (``OPCODES``) in bits 0-7, operand a in bits 8-23, operand b in
bits 24-39 (0 for a one-operand op; the b of ``POWC`` is a ``CONST``).  `root` is an operand and may be a leaf.

The definition.  ``interpret`` below IS the model; the kernel follows it operation by operation.
Forward: val[k] for k ascending; the model value is the value of `root`.
Reverse: the adjoints and the row start at +0.0; 1 is pushed to `root`; then k descending with g = adj[k], operand a
pushed before b.  A push is ``dst = dst + contribution``: dst is adj[.] for a ``TAPE`` operand whose op depends on a
variable, column k of the row for ``VAR k``; a push to anything else is dropped.  An op that depends on no variable is
skipped (``Program.active``; derived, not part of the program).  The contributions:

    ADD   g            g               EXP   g*v                     ATAN  g/(1+va*va)
    SUB   g            -g              LOG   g/va                    ERF   g*(C*exp(-(va*va)))   C = 2/sqrt(pi)
    MUL   g*vb         g*va            SQRT  (0.5*g)/v               ERFC  -(g*(C*exp(-(va*va))))
    DIV   g/vb         -((g*v)/vb)     SIN   g*cos(va)               POWC  g*(c*pow(va, c-1))
    NEG   -g                           COS   -(g*sin(va))

A fit then forms f = w (v - y) and multiplies the row by w as a whole, after the sweep (under Poisson: r and c of
``models.poisson_transform``).  The built-in terms weight each column before they sum; nobody should look for bit
equality between the two.
"""
import ast
import math
import re
import struct
from collections import namedtuple

import numpy as np

MAX_OPS = 64                                 # BLSQ_EXPR_MAX_OPS
MAX_CONST = 32                               # BLSQ_EXPR_MAX_CONST
MAX_COORD = 4                                # BLSQ_EXPR_MAX_COORD
MAX_N = 64                                   # BLSQ_MODEL_MAX_N: parameters, and solver variables
OPCODES = ('ADD', 'SUB', 'MUL', 'DIV', 'NEG', 'EXP', 'LOG', 'SQRT', 'SIN', 'COS', 'ATAN', 'ERF', 'ERFC', 'POWC')
KINDS = ('TAPE', 'VAR', 'PFIX', 'CONST', 'COORD')
ADD, SUB, MUL, DIV, NEG, EXP, LOG, SQRT, SIN, COS, ATAN, ERF, ERFC, POWC = range(14)
TAPE, VAR, PFIX, CONST, COORD = range(5)
TWO_BY_SQRT_PI = 1.1283791670955126          # C of the erf and erfc contributions
FUNCTIONS = {'exp': EXP, 'log': LOG, 'sqrt': SQRT, 'sin': SIN, 'cos': COS, 'atan': ATAN, 'erf': ERF, 'erfc': ERFC}
_BINARY = (ADD, SUB, MUL, DIV, POWC)

__all__ = ['expression', 'ExprModel', 'BoundExpr', 'Program', 'interpret', 'OPCODES', 'KINDS', 'MAX_OPS', 'MAX_CONST',
           'MAX_COORD']


def operand(kind, index):
    return (kind << 8) | index


def op_word(opcode, a, b=0):
    return opcode | (a << 8) | (b << 24)


def _bits(c):
    return struct.unpack('<q', struct.pack('<d', c))[0]


class Program(namedtuple('Program', 'ops consts root')):
    """``ops`` (nops,) uint64, ``consts`` (nconst,) float64, ``root`` an operand (module docstring)."""
    __slots__ = ()

    @property
    def nops(self):
        return len(self.ops)

    def decode(self):
        """[(opcode, a, b)] of the ops, as ints."""
        return [(int(w) & 0xff, (int(w) >> 8) & 0xffff, (int(w) >> 24) & 0xffff) for w in self.ops]

    def active(self):
        """(nops,) bool: the ops that depend on a solver variable (an operand that is a VAR, or an earlier such op)."""
        act = np.zeros(self.nops, dtype=bool)
        for k, (opc, a, b) in enumerate(self.decode()):
            for o in ((a, b) if opc in _BINARY else (a,)):
                if o >> 8 == VAR or (o >> 8 == TAPE and act[o & 0xff]):
                    act[k] = True
        return act

    def __repr__(self):
        def show(o):
            return "%s %d" % (KINDS[o >> 8], o & 0xff)
        lines = ["%2d %s %s%s" % (k, OPCODES[opc], show(a), ", " + show(b) if opc in _BINARY else "")
                 for k, (opc, a, b) in enumerate(self.decode())]
        return "Program(%d ops, consts %s, root %s)\n  " % (self.nops, self.consts.tolist(), show(self.root)) \
            + "\n  ".join(lines)


class _Emitter:
    """The ops, constants and merge table of a program under construction.  A value is ``('c', float)`` while it is a
    constant nobody has used as an operand, or ``('o', operand)``."""

    def __init__(self, what):
        self.what, self.ops, self.consts, self.seen, self.cbits = what, [], [], {}, {}

    def const(self, c):
        c = float(c)
        key = _bits(c)
        if key not in self.cbits:
            self.cbits[key] = len(self.consts)
            self.consts.append(c)
        return operand(CONST, self.cbits[key])

    def use(self, v):
        return self.const(v[1]) if v[0] == 'c' else v[1]

    def emit(self, opcode, a, b=0):
        key = (opcode, a, b)
        if key not in self.seen:
            self.seen[key] = len(self.ops)
            self.ops.append(op_word(opcode, a, b))
        return ('o', operand(TAPE, self.seen[key]))

    def binary(self, opcode, x, y):
        if x[0] == 'c' and y[0] == 'c':                      # folded in float64, as the interpreter would compute it
            fold = {ADD: np.add, SUB: np.subtract, MUL: np.multiply, DIV: np.divide}[opcode]
            with np.errstate(all='ignore'):
                return ('c', float(fold(np.float64(x[1]), np.float64(y[1]))))
        return self.emit(opcode, self.use(x), self.use(y))

    def power(self, x, c):
        if x[0] == 'c':
            with np.errstate(all='ignore'):
                return ('c', float(np.power(np.float64(x[1]), np.float64(c))))
        if c == 0:
            return ('c', 1.0)
        if c == 1:
            return x
        if 2 <= c <= 8 and c == int(c):
            a = self.use(x)
            acc = self.emit(MUL, a, a)
            for _ in range(int(c) - 2):
                acc = self.emit(MUL, acc[1], a)
            return acc
        return self.emit(POWC, self.use(x), self.const(c))

    def finish(self, root):
        root = self.use(root)
        if len(self.ops) > MAX_OPS:                          # (an operand past its byte never leaves this function)
            raise ValueError("%s compiles to %d ops, more than %d." % (self.what, len(self.ops), MAX_OPS))
        if len(self.consts) > MAX_CONST:
            raise ValueError("%s needs %d constants, more than %d." % (self.what, len(self.consts), MAX_CONST))
        return Program(np.array(self.ops, dtype=np.uint64), np.array(self.consts, dtype=np.float64), root)


def _src(text, node):
    seg = ast.get_source_segment(text, node)
    return seg if seg else type(node).__name__


def _compile(text, params, coords):
    what = "expression %r" % text
    text = text.strip()                                      # (leading blanks would read as an indent)
    try:
        tree = ast.parse(text, mode='eval')
    except SyntaxError as e:
        raise ValueError("%s does not parse: %s." % (what, e.msg)) from None
    em = _Emitter(what)
    leaves = {name: operand(VAR, j) for j, name in enumerate(params)}
    leaves.update({name: operand(COORD, r) for r, name in enumerate(coords)})
    used = set()
    binops = {ast.Add: ADD, ast.Sub: SUB, ast.Mult: MUL, ast.Div: DIV}

    def walk(node):
        if isinstance(node, ast.Constant):
            if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
                raise ValueError("%s: the literal %s is not an int or a float." % (what, _src(text, node)))
            return ('c', float(node.value))
        if isinstance(node, ast.Name):
            if node.id in leaves:
                used.add(node.id)
                return ('o', leaves[node.id])
            if node.id == 'pi':
                return ('c', math.pi)
            raise ValueError("%s: unknown name %r (parameters: %s; coordinates: %s; the constant pi)."
                             % (what, node.id, ", ".join(params), ", ".join(coords)))
        if isinstance(node, ast.UnaryOp):
            if isinstance(node.op, ast.UAdd):
                return walk(node.operand)
            if isinstance(node.op, ast.USub):
                x = walk(node.operand)
                return ('c', -x[1]) if x[0] == 'c' else em.emit(NEG, x[1])
            raise ValueError("%s: the unary operator in %s is not supported (+ and - are)." % (what, _src(text, node)))
        if isinstance(node, ast.BinOp):
            if isinstance(node.op, ast.Pow):
                x, e = walk(node.left), walk(node.right)
                if e[0] != 'c':
                    raise ValueError("%s: the exponent of %s is not a constant." % (what, _src(text, node)))
                return em.power(x, e[1])
            if type(node.op) not in binops:
                raise ValueError("%s: the operator in %s is not supported (+ - * / ** are)." % (what, _src(text, node)))
            x = walk(node.left)
            return em.binary(binops[type(node.op)], x, walk(node.right))
        if isinstance(node, ast.Call):
            if not isinstance(node.func, ast.Name) or node.func.id not in FUNCTIONS:
                raise ValueError("%s: %s is not a call of a known function (%s)."
                                 % (what, _src(text, node), ", ".join(FUNCTIONS)))
            if node.keywords:
                raise ValueError("%s: the call %s has a keyword argument." % (what, _src(text, node)))
            if len(node.args) != 1 or isinstance(node.args[0], ast.Starred):
                raise ValueError("%s: the call %s must have one argument." % (what, _src(text, node)))
            return em.emit(FUNCTIONS[node.func.id], em.use(walk(node.args[0])))
        kind = {ast.Attribute: "attribute", ast.Subscript: "subscript", ast.Compare: "comparison",
                ast.BoolOp: "boolean operator", ast.IfExp: "conditional", ast.Lambda: "lambda", ast.Tuple: "tuple",
                ast.List: "list"}.get(type(node), type(node).__name__)
        raise ValueError("%s: the %s %s is not part of the language." % (what, kind, _src(text, node)))

    prog = em.finish(walk(tree.body))
    missing = [p for p in params if p not in used]
    if missing:
        raise ValueError("%s: parameter %r never appears." % (what, missing[0]))
    return prog


# ---- the definition --------------------------------------------------------------------------------------------------
def _erf(x, complement):
    """scipy.special's float64 erf / erfc; another dtype is computed in float64 and cast back (as ``models.erf_diff``)."""
    from scipy import special
    x = np.asarray(x)
    return (special.erfc if complement else special.erf)(x.astype(np.float64)).astype(x.dtype, copy=False)


_UNARY = {EXP: np.exp, LOG: np.log, SQRT: np.sqrt, SIN: np.sin, COS: np.cos, ATAN: np.arctan,
          ERF: lambda x: _erf(x, False), ERFC: lambda x: _erf(x, True)}


def interpret(prog, T, X, Pfix=None, want_f=True, want_J=False):
    """The definition (module docstring).  `T`: the coordinates, a sequence of arrays (m,) or (B, m); `X` (B, nf);
    `Pfix` (B, n) or None.  Returns ``(v (B, m) or None, J (B, m, nf) or None)`` in the common floating dtype."""
    X = np.asarray(X)
    T = [np.asarray(t) for t in T]
    dt = np.result_type(X.dtype, np.float64, *[t.dtype for t in T], *([] if Pfix is None else [np.asarray(Pfix).dtype]))
    X = X.astype(dt, copy=False)
    T = [t.astype(dt, copy=False) for t in T]
    Pfix = None if Pfix is None else np.asarray(Pfix).astype(dt, copy=False)
    consts = prog.consts.astype(dt)
    B, m = X.shape[0], T[0].shape[-1]
    ops = prog.decode()
    val = [None] * len(ops)

    def fetch(o):
        kind, i = o >> 8, o & 0xff
        if kind == TAPE:
            return val[i]
        if kind == VAR:
            return X[:, i, np.newaxis]
        if kind == PFIX:
            return Pfix[:, i, np.newaxis]
        if kind == CONST:
            return consts[i]
        return T[i]

    with np.errstate(all='ignore'):
        for k, (opc, a, b) in enumerate(ops):
            va = fetch(a)
            if opc == ADD:
                v = va + fetch(b)
            elif opc == SUB:
                v = va - fetch(b)
            elif opc == MUL:
                v = va * fetch(b)
            elif opc == DIV:
                v = va / fetch(b)
            elif opc == NEG:
                v = -va
            elif opc == POWC:
                v = np.power(va, fetch(b))
            else:
                v = _UNARY[opc](va)
            val[k] = v
        v_root = np.array(np.broadcast_to(fetch(prog.root), (B, m))) if want_f else None
        if not want_J:
            return v_root, None
        act = prog.active()
        nf = X.shape[1]
        J = np.zeros((B, m, nf), dtype=dt)
        adj = [np.zeros((B, m), dtype=dt) if act[k] else None for k in range(len(ops))]

        def push(o, c):
            kind, i = o >> 8, o & 0xff
            if kind == TAPE and act[i]:
                adj[i] = adj[i] + c
            elif kind == VAR:
                J[:, :, i] = J[:, :, i] + c

        push(prog.root, dt.type(1))
        for k in range(len(ops) - 1, -1, -1):
            if not act[k]:
                continue
            opc, a, b = ops[k]
            g, v, va = adj[k], val[k], fetch(a)
            if opc == ADD:
                push(a, g)
                push(b, g)
            elif opc == SUB:
                push(a, g)
                push(b, -g)
            elif opc == MUL:
                vb = fetch(b)
                push(a, g * vb)
                push(b, g * va)
            elif opc == DIV:
                vb = fetch(b)
                push(a, g / vb)
                push(b, -((g * v) / vb))
            elif opc == NEG:
                push(a, -g)
            elif opc == EXP:
                push(a, g * v)
            elif opc == LOG:
                push(a, g / va)
            elif opc == SQRT:
                push(a, (0.5 * g) / v)
            elif opc == SIN:
                push(a, g * np.cos(va))
            elif opc == COS:
                push(a, -(g * np.sin(va)))
            elif opc == ATAN:
                push(a, g / (1 + va * va))
            elif opc == ERF:
                push(a, g * (dt.type(TWO_BY_SQRT_PI) * np.exp(-(va * va))))
            elif opc == ERFC:
                push(a, -(g * (dt.type(TWO_BY_SQRT_PI) * np.exp(-(va * va)))))
            else:                                            # POWC
                c = fetch(b)
                push(a, g * (c * np.power(va, c - 1)))
    return v_root, J


def _coordinates(xdata, ncoord):
    """xdata (m,) / (B, m) — (C, m) / (B, C, m) for C > 1 coordinates — as the list of its coordinates."""
    x = np.asarray(xdata)
    return [x] if ncoord == 1 else [x[..., r, :] for r in range(ncoord)]


class BoundExpr:
    """The program of an ``ExprModel`` behind a ``ParamMap`` (``ExprModel.bind``): ``program`` reads the nf solver
    variables (``VAR``) and the parameters the map holds fixed (``PFIX j``: column j of the template); ``n`` model
    parameters, ``nf`` variables.  ``f(xdata, X, Pfix)`` and ``jac(xdata, X, Pfix)`` interpret it."""

    def __init__(self, model, program, nf):
        self.model, self.program, self.n, self.nf, self.coords = model, program, model.n, int(nf), model.coords

    def f(self, xdata, X, Pfix=None):
        return interpret(self.program, _coordinates(xdata, self.coords), X, Pfix)[0]

    def jac(self, xdata, X, Pfix=None):
        return interpret(self.program, _coordinates(xdata, self.coords), X, Pfix, want_f=False, want_J=True)[1]


class ExprModel:
    """A model given as a formula (``expression``; the module docstring has the language and the definition).  Offers
    what a ``CompositeModel`` offers its callers: ``name`` (the text without whitespace), ``coords`` (the number of
    coordinates; their names are ``coord_names``), ``n``, ``param_names``, ``terms``, ``check_xdata``, the numpy
    ``f(xdata, P) -> (B, m)`` / ``jac(xdata, P) -> (B, m, n)`` — and ``program`` and ``bind``."""

    def __init__(self, text, params, coords=('t',)):
        if not isinstance(text, str):
            raise ValueError("an expression model is given as a string such as 'a*exp(-t/tau)+c', not %r." % (text,))
        params = (params,) if isinstance(params, str) else tuple(params)
        coords = (coords,) if isinstance(coords, str) else tuple(coords)
        names = params + coords
        for nm in names:
            if not isinstance(nm, str) or not nm.isidentifier():
                raise ValueError("%r is not a name a parameter or a coordinate can have." % (nm,))
            if nm == 'pi' or nm in FUNCTIONS:
                raise ValueError("the name %r is taken by the language." % nm)
        if len(set(names)) != len(names):
            raise ValueError("the names of parameters and coordinates must differ: %s." % ", ".join(names))
        if not 1 <= len(params) <= MAX_N:
            raise ValueError("an expression model takes 1 to %d parameters, not %d." % (MAX_N, len(params)))
        if not 1 <= len(coords) <= MAX_COORD:
            raise ValueError("an expression model takes 1 to %d coordinates, not %d." % (MAX_COORD, len(coords)))
        self.text, self.name = text, re.sub(r"\s+", "", text)
        self.param_names, self.coord_names = params, coords
        self.n, self.coords = len(params), len(coords)
        self.program = _compile(text, params, coords)

    def terms(self, n):
        """1; ValueError unless n is the number of parameters."""
        if int(n) != self.n:
            raise ValueError("model '%s' does not take n = %d parameters (n = %d)." % (self.name, int(n), self.n))
        return 1

    def rule(self):
        return "n = %d" % self.n

    def check_xdata(self, xdata, B, m):
        """xdata as a float64 array of shape (m,) / (B, m) — (C, m) / (B, C, m) for C > 1 coordinates; ValueError
        otherwise.  Returns (array, per_problem)."""
        x = np.asarray(xdata, dtype=np.float64)
        shared = (m,) if self.coords == 1 else (self.coords, m)
        if x.shape == (B,) + shared:
            return np.ascontiguousarray(x), True
        if x.shape == shared:
            return np.ascontiguousarray(x), False
        raise ValueError("`xdata` of model '%s' must have shape %s or %s, not %s."
                         % (self.name, shared, (B,) + shared, x.shape))

    def _P(self, P):
        P = np.asarray(P)
        if P.ndim != 2 or P.shape[1] != self.n:
            raise ValueError("model '%s' takes P of shape (B, %d), not %s." % (self.name, self.n, P.shape))
        return P

    def f(self, xdata, P):
        return interpret(self.program, _coordinates(xdata, self.coords), self._P(P))[0]

    def jac(self, xdata, P):
        return interpret(self.program, _coordinates(xdata, self.coords), self._P(P), want_f=False, want_J=True)[1]

    def bind(self, param_map=None):
        """The program behind a ``ParamMap`` (None: the identity), as a ``BoundExpr``.  Only leaves are rewritten:
        parameter j with ``pmap[j] < 0`` becomes ``PFIX j``; with (ratio, offset) == (1, 0) ``VAR pmap[j]``; otherwise
        ``ADD(MUL(CONST ratio, VAR k), CONST offset)``, the product first as in ``ParamMap.expand_x``, emitted where
        the parameter is first used and computed once (the ops are merged as the compiler merges them).  The columns of
        tied parameters then accumulate in the reverse sweep by themselves.

        ``f`` of the bound program at X equals ``self.f(xdata, pm.expand_x(X, Pfix))`` bit for bit.  ``jac`` equals
        ``pm.reduce_jac(self.jac(...))`` to rounding only: the sweep adds the contributions of a slot in the order it
        meets them, ``reduce_jac`` the finished columns in ascending j.  ValueError if the ties push the program past
        its limits."""
        pm = param_map
        if pm is None:
            return BoundExpr(self, self.program, self.n)
        if pm.n != self.n:
            raise ValueError("`param_map` is for %d parameters, the model has %d." % (pm.n, self.n))
        em = _Emitter("expression %r with its ties" % self.text)
        old = self.program
        for c in old.consts:                                 # the constants keep their indices
            em.const(c)
        tape = {}

        def leaf(o):
            kind, i = o >> 8, o & 0xff
            if kind == TAPE:
                return tape[i]
            if kind != VAR:
                return o
            k = int(pm.pmap[i])
            if k < 0:
                return operand(PFIX, i)
            r, d = float(pm.ratio[i]), float(pm.offset[i])
            if (r, d) == (1.0, 0.0):
                return operand(VAR, k)
            prod = em.emit(MUL, em.const(r), operand(VAR, k))
            return em.emit(ADD, prod[1], em.const(d))[1]

        for k, (opc, a, b) in enumerate(old.decode()):
            a2 = leaf(a)
            b2 = leaf(b) if opc in _BINARY else 0
            tape[k] = em.emit(opc, a2, b2)[1]
        return BoundExpr(self, em.finish(('o', leaf(old.root))), pm.nf)

    def __repr__(self):
        return "ExprModel(%r, params=%r, coords=%r)" % (self.text, self.param_names, self.coord_names)


def expression(text, params, coords=('t',)):
    """The ``ExprModel`` of the formula `text` over the parameters `params` (an ordered tuple of names: the column order
    of p0, popt, pcov and bounds) and the coordinates `coords` (1 to 4 names; xdata is (m,) / (B, m) for one, (C, m) /
    (B, C, m) otherwise).  ValueError naming the construct for anything outside the language, a parameter that never
    appears, or a program past 64 ops or 32 constants (with the count)."""
    return ExprModel(text, params, coords)
