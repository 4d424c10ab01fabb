"""Expression models without a GPU: the exports, the two entries against header and binding,
blsq_expr_check and the NULL context, the language and its errors, the compile rules, the numpy definition against the
truth file (tests/_expr_cases.py: the cases, the magnitudes and K_REF), the truth file against a regeneration, the map
of fixed and tied parameters, the refusals, and what driver='host' hands the solver."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _abi, _expr, models

import _expr_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _expr
DECAY = "a*(f1*exp(-t/tau1)+(1-f1)*exp(-t/tau2))+bg"
DECAY_PARAMS = ("a", "f1", "tau1", "tau2", "bg")


def op(name, a, b=0):
    return E.op_word(E.OPCODES.index(name), a, b)


def opd(kind, i):
    return E.operand(E.KINDS.index(kind), i)


def decoded(prog):
    return [(E.OPCODES[o], (E.KINDS[a >> 8], a & 0xff), (E.KINDS[b >> 8], b & 0xff)) for o, a, b in prog.decode()]


# ---- exports, header, binding ------------------------------------------------------------------------------------------
def test_exports():
    assert models.expression is _expr.expression and models.ExprModel is _expr.ExprModel
    assert "expression" in models.__all__ and "ExprModel" in models.__all__
    assert bounded_lsq.models.expression("a*t", ("a",)).n == 1
    M = models.expression(" a * exp( -t / tau ) + c ", ("a", "tau", "c"))
    assert M.name == "a*exp(-t/tau)+c" and M.param_names == ("a", "tau", "c") and M.coords == 1 and M.n == 3
    assert M.terms(3) == 1 and models.resolve(M) is M
    with pytest.raises(ValueError, match="does not take n = 4"):
        M.terms(4)
    x, per = M.check_xdata(np.zeros((2, 7)), 2, 7)
    assert per and x.shape == (2, 7) and not M.check_xdata(np.zeros(7), 2, 7)[1]
    with pytest.raises(ValueError, match="`xdata` of model"):
        M.check_xdata(np.zeros(6), 2, 7)
    M2 = models.expression("a*u+v", ("a",), coords=("u", "v"))
    assert M2.coords == 2 and M2.check_xdata(np.zeros((3, 2, 5)), 3, 5)[1]
    np.testing.assert_array_equal(M2.f(np.array([[1.0, 2.0], [10.0, 20.0]]), np.array([[3.0]])), [[13.0, 26.0]])


def test_header_signatures_and_library_agree():
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    for k, v in (("BLSQ_EXPR_MAX_OPS", E.MAX_OPS), ("BLSQ_EXPR_MAX_CONST", E.MAX_CONST),
                 ("BLSQ_EXPR_MAX_COORD", E.MAX_COORD)):
        assert re.search(r"#define %s %d\b" % (k, v), src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    enums = [re.findall(r"BLSQ_EXPR_([A-Z]+)", body) for body in re.findall(r"enum\s*\{([^}]*BLSQ_EXPR_[^}]*)\}", code)]
    assert enums == [list(E.OPCODES), list(E.KINDS)]
    for name, nargs in (("blsq_expr_check", 7), ("blsq_expr_eval_dev", 24)):
        assert not re.fullmatch(r"blsq_model_eval.*_dev", name)
        decl = re.search(r"int %s\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == nargs == len(_abi.SIGNATURES[name][1])
        assert hasattr(_abi.load(), name)
    types = [a.strip().rsplit(" ", 1)[0] for a in re.search(r"int blsq_expr_eval_dev\(([^)]*)\)", code).group(1).split(",")]
    want = {"int": C.c_int, "long": C.c_long, "const uint64_t*": C.POINTER(C.c_uint64), "const double*": None,
            "double*": _abi.vp, "const int32_t*": _abi.vp, "blsq_ctx*": _abi.vp}
    for ty, got in zip(types, _abi.SIGNATURES["blsq_expr_eval_dev"][1]):
        assert want[ty] is got or (want[ty] is None and got in (_abi.vp, _abi.c_double_p)), (ty, got)
    assert len(models.TERMS) == 5 and len(models.MODELS) == 5 and len(_abi.MODEL_EVAL_ARGS) == 8


# ---- blsq_expr_check ---------------------------------------------------------------------------------------------------
def check(ops, root, nconst=1, nf=2, npfix=2, ncoord=1, nops=None, null=False):
    ops = np.ascontiguousarray(ops, dtype=np.uint64)
    p = None if null else ops.ctypes.data_as(C.POINTER(C.c_uint64))
    return _abi.load().blsq_expr_check(len(ops) if nops is None else nops, p, root, nconst, nf, npfix, ncoord)


def test_expr_check_good_programs():
    lib = _abi.load()
    for name in ec.CASES:
        M = ec.model(name)
        p = M.program
        assert check(p.ops, p.root, len(p.consts), M.n, M.n, 1) == 0, name
        pm = bounded_lsq.ParamMap(M.n, [0], {2: 1} if name == "sum64" else {2: (1, -2.0, 0.5)})
        q = M.bind(pm).program
        assert check(q.ops, q.root, len(q.consts), pm.nf, M.n, 1) == 0, name
    assert lib.blsq_expr_check(0, None, opd("VAR", 0), 0, 1, 0, 1) == 0          # a leaf as the whole program
    assert check([op("POWC", opd("VAR", 1), opd("CONST", 0))], opd("TAPE", 0)) == 0
    assert check([op("NEG", opd("COORD", 3))], opd("TAPE", 0), ncoord=4) == 0


@pytest.mark.parametrize("kw, want", [
    (dict(ops=[], root=opd("VAR", 0), nops=-1), -1),
    (dict(ops=[], root=opd("VAR", 0), nops=65), -1),
    (dict(ops=[0], root=opd("VAR", 0), null=True), -2),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), nconst=-1), -4),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), nconst=33), -4),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), nf=0), -5),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), nf=65), -5),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), npfix=-1), -6),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), npfix=65), -6),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), ncoord=0), -7),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 0), ncoord=5), -7),
    (dict(ops=[14 | (opd("VAR", 0) << 8)], root=opd("TAPE", 0)), -2),                         # an unknown opcode
    (dict(ops=[op("NEG", opd("VAR", 0)) | (1 << 40)], root=opd("TAPE", 0)), -2),              # bits past the operands
    (dict(ops=[op("NEG", opd("TAPE", 0))], root=opd("TAPE", 0)), -2),                         # its own result
    (dict(ops=[op("NEG", opd("VAR", 0)), op("ADD", opd("TAPE", 0), opd("TAPE", 1))], root=opd("TAPE", 1)), -2),
    (dict(ops=[op("NEG", opd("VAR", 2))], root=opd("TAPE", 0)), -2),                          # VAR >= nf
    (dict(ops=[op("NEG", opd("PFIX", 2))], root=opd("TAPE", 0)), -2),                         # PFIX >= npfix
    (dict(ops=[op("NEG", opd("CONST", 1))], root=opd("TAPE", 0)), -2),                        # CONST >= nconst
    (dict(ops=[op("NEG", opd("COORD", 1))], root=opd("TAPE", 0)), -2),                        # COORD >= ncoord
    (dict(ops=[op("NEG", (5 << 8))], root=opd("TAPE", 0)), -2),                               # an unknown kind
    (dict(ops=[op("MUL", opd("VAR", 0), opd("VAR", 2))], root=opd("TAPE", 0)), -2),           # the b operand
    (dict(ops=[op("POWC", opd("VAR", 0), opd("VAR", 1))], root=opd("TAPE", 0)), -2),          # POWC's b is no CONST
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("TAPE", 1)), -3),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=opd("VAR", 2)), -3),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=-1), -3),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=0x10000), -3),
    (dict(ops=[op("NEG", opd("VAR", 0))], root=(5 << 8)), -3),
])
def test_expr_check_names_the_first_bad_argument(kw, want):
    assert check(**kw) == want
    # the b operand of a one-operand op is not read
    assert check([op("NEG", opd("VAR", 0), 0xffff)], opd("TAPE", 0)) == 0


def test_null_context():
    lib = _abi.load()
    assert lib.blsq_expr_eval_dev(None, 0, 0, 1, 1, 1, 1, 0, 1, 0, None, opd("VAR", 0), 0, None, None, 0, None, None, 0,
                                  None, None, None, None, None) == -1


# ---- the language ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, match", [
    ("a.real+b", "attribute a.real"), ("a[0]+b", "subscript a\\[0\\]"), ("(a<b)+b", "comparison"),
    ("exp(a, b)", "one argument"), ("exp(x=a)+b", "keyword"), ("a*cosh(b)", "cosh\\(b\\) is not a call of a known"),
    ("a.f(b)", "not a call of a known"), ("a**b", "exponent of a\\*\\*b is not a constant"),
    ("a**t+b", "not a constant"), ("a+b+q", "unknown name 'q'"), ("a if b else 1", "conditional"),
    ("a and b", "boolean operator"), ("a+b+'s'", "literal"), ("a+b+True", "literal"), ("a+b+1j", "literal"),
    ("a+b+", "does not parse"), ("a//b", "operator in a//b"), ("a%b", "operator"), ("~a+b", "unary operator"),
    ("[a, b]", "list"), ("(a, b)", "tuple"), ("lambda: a", "lambda"), ("a", "parameter 'b' never appears"),
    ("a*exp(*b)", "one argument"),
])
def test_language_errors_name_the_construct(text, match):
    with pytest.raises(ValueError, match=match):
        models.expression(text, ("a", "b"))


def test_names_and_limits():
    with pytest.raises(ValueError, match="not a string|given as a string"):
        models.expression(3, ("a",))
    with pytest.raises(ValueError, match="taken by the language"):
        models.expression("pi", ("pi",))
    with pytest.raises(ValueError, match="taken by the language"):
        models.expression("exp+t", ("exp",))
    with pytest.raises(ValueError, match="must differ"):
        models.expression("a+t", ("a", "t"))
    with pytest.raises(ValueError, match="not a name"):
        models.expression("a+t", ("a b",))
    with pytest.raises(ValueError, match="1 to 64 parameters, not 0"):
        models.expression("t", ())
    with pytest.raises(ValueError, match="1 to 64 parameters, not 65"):
        models.expression("t", tuple("p%d" % i for i in range(65)))
    with pytest.raises(ValueError, match="1 to 4 coordinates, not 5"):
        models.expression("a", ("a",), coords=("u", "v", "w", "x", "y"))
    with pytest.raises(ValueError, match="1 to 4 coordinates, not 0"):
        models.expression("a", ("a",), coords=())
    assert ec.model("sum64").program.nops == 64                                   # the limit itself compiles
    with pytest.raises(ValueError, match="compiles to 65 ops, more than 64"):
        models.expression("t*t*(" + "+".join("p%d" % i for i in range(64)) + ")", tuple("p%d" % i for i in range(64)))
    assert len(models.expression("a" + "".join("*%d.5" % i for i in range(32)), ("a",)).program.consts) == 32
    with pytest.raises(ValueError, match="needs 33 constants, more than 32"):
        models.expression("a" + "".join("*%d.5" % i for i in range(33)), ("a",))
    # the ties of a map count too
    M = ec.model("sum64")
    with pytest.raises(ValueError, match="more than 64"):
        M.bind(bounded_lsq.ParamMap(64, None, {1: (0, 2.0)}))


# ---- the compile rules -------------------------------------------------------------------------------------------------
def test_post_order_and_merging():
    p = models.expression("exp(-t/tau)*a+exp(-t/tau)", ("a", "tau")).program
    assert decoded(p) == [("NEG", ("COORD", 0), ("TAPE", 0)), ("DIV", ("TAPE", 0), ("VAR", 1)),
                          ("EXP", ("TAPE", 1), ("TAPE", 0)), ("MUL", ("TAPE", 2), ("VAR", 0)),
                          ("ADD", ("TAPE", 3), ("TAPE", 2))]
    assert p.root == opd("TAPE", 4) and len(p.consts) == 0
    # the key is (opcode, a, b): a*t and t*a are two ops
    assert models.expression("a*t+t*a", ("a",)).program.nops == 3
    assert models.expression("a*t+a*t", ("a",)).program.nops == 2
    # a leaf as root, and a program without ops
    q = models.expression("+a", ("a",)).program
    assert q.nops == 0 and q.root == opd("VAR", 0)


def test_folding():
    p = models.expression("2*pi*a+(1+2)/4-(-3)", ("a",)).program
    assert p.consts.tolist() == [2 * np.pi, 0.75, -3.0] and [d[0] for d in decoded(p)] == ["MUL", "ADD", "SUB"]
    p = models.expression("a*(2*3)+-(4)", ("a",)).program
    assert p.consts.tolist() == [6.0, -4.0] and [d[0] for d in decoded(p)] == ["MUL", "ADD"]
    # a function of a constant is an op like any other; a constant is stored once
    p = models.expression("a*sqrt(2)+2", ("a",)).program
    assert [d[0] for d in decoded(p)] == ["SQRT", "MUL", "ADD"] and p.consts.tolist() == [2.0]
    assert p.active().tolist() == [False, True, True]
    assert models.expression("a+2**0.5", ("a",)).program.consts.tolist() == [2 ** 0.5]
    assert models.expression("a+0.0+-0.0", ("a",)).program.consts.tolist() == [0.0, -0.0]   # merged on their bits


def test_powers():
    x = ("VAR", 0)
    assert decoded(models.expression("a**2", ("a",)).program) == [("MUL", x, x)]
    assert decoded(models.expression("a**3", ("a",)).program) == [("MUL", x, x), ("MUL", ("TAPE", 0), x)]
    p = models.expression("a**8", ("a",)).program
    assert p.nops == 7 and all(d == ("MUL", ("TAPE", k - 1), x) for k, d in enumerate(decoded(p)) if k)
    p = models.expression("a**1+t", ("a",)).program
    assert decoded(p) == [("ADD", x, ("COORD", 0))]
    p = models.expression("a**0+a", ("a",)).program
    assert decoded(p) == [("ADD", ("CONST", 0), x)] and p.consts.tolist() == [1.0]
    for text, c in (("a**9", 9.0), ("a**1.5", 1.5), ("a**-2", -2.0), ("a**(1/2)", 0.5), ("a**2.0000001", 2.0000001)):
        p = models.expression(text, ("a",)).program
        assert decoded(p) == [("POWC", x, ("CONST", 0))] and p.consts.tolist() == [c], text
    assert decoded(models.expression("a**2.0", ("a",)).program) == [("MUL", x, x)]
    assert decoded(models.expression("(a+t)**2", ("a",)).program)[1] == ("MUL", ("TAPE", 0), ("TAPE", 0))


# ---- the definition ----------------------------------------------------------------------------------------------------
def test_case_programs_have_the_documented_sizes():
    sizes = {name: (ec.model(name).program.nops, len(ec.model(name).program.consts)) for name in ec.CASES}
    assert sizes == {"gauss2_line": (18, 1), "decay": (11, 1), "emg": (13, 2), "damped_sine": (10, 1),
                     "stretched": (14, 2), "lorentz_root": (13, 1), "sum64": (64, 0)}
    assert os.path.getsize(ec.GOLDEN) < 200 * 1024


@pytest.mark.parametrize("name", list(ec.CASES))
def test_definition_against_the_truth(name):
    """max |numpy definition - truth| / (eps mag) <= K_REF, for f and for J."""
    d, M = ec.truth()[name], ec.model(name)
    P, t = ec.draw(name)
    assert np.array_equal(P, d["P"]) and np.array_equal(t, d["t"])
    kf = ec.excess(M.f(t, P), d["f"], d["fmag"])
    kj = ec.excess(M.jac(t, P), d["J"], d["Jmag"])
    print("%s: K f %.3f J %.3f of K_REF %.3g" % (name, kf, kj, ec.K_REF[name]))
    assert kf <= ec.K_REF[name] and kj <= ec.K_REF[name]
    # per-problem abscissae give the same bits, and the magnitudes in the file are the helper's
    assert np.array_equal(M.f(np.tile(t, (ec.B, 1)), P), M.f(t, P))
    fmag, Jmag = ec.magnitudes(M.program, [t], P)
    assert np.array_equal(fmag.astype(np.float32), d["fmag"]) and np.array_equal(Jmag.astype(np.float32), d["Jmag"])


def test_definition_keeps_longdouble():
    M = ec.model("decay")
    P, t = ec.draw("decay")
    f = M.f(t.astype(np.longdouble), P.astype(np.longdouble))
    assert f.dtype == np.longdouble and M.jac(t, P.astype(np.longdouble)).dtype == np.longdouble
    np.testing.assert_allclose(f.astype(float), M.f(t, P), rtol=1e-14)


def test_truth_file_against_a_regeneration():
    """Where sympy and mpmath import: every fifth point of every case, generated again."""
    pytest.importorskip("sympy")
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_expr_truth", os.path.join(ROOT, "tools", "make_expr_truth.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = list(range(0, ec.POINTS, 5))
    for name in ec.CASES:
        d = ec.truth()[name]
        f, J = tool.true_values(name, d["P"], d["t"], rows)
        assert np.array_equal(f, d["f"][:, rows]) and np.array_equal(J, d["J"][:, rows]), name


# ---- fixed, tied and affine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, fixed, tied", [
    ("decay", [4], None), ("decay", None, {3: 2}), ("decay", [0], {3: (2, 4.0, 0.1)}),
    ("gauss2_line", [6], {3: (0, 0.5), 5: (2, 1.0, 0.25), 4: 1}), ("lorentz_root", [1, 3], {5: (2, -2.0)}),
    ("sum64", list(range(2, 40)), {1: 0, 63: 62}),
])
def test_bound_program_against_the_expanded_call(name, fixed, tied):
    """f bit-equal to the model at expand_x(X); jac to rounding (the order of a slot's sums differs): within
    8 eps of the magnitudes of the bound program."""
    M = ec.model(name)
    P, t = ec.draw(name)
    pm = bounded_lsq.ParamMap(M.n, fixed, tied)
    Bd = M.bind(pm)
    assert Bd.nf == pm.nf and Bd.n == M.n
    X = pm.reduce_x(P)
    full = pm.expand_x(X, P)
    assert np.array_equal(Bd.f(t, X, P), M.f(t, full))
    J, want = Bd.jac(t, X, P), pm.reduce_jac(M.jac(t, full))
    assert J.shape == want.shape == (ec.B, ec.POINTS, pm.nf)
    assert ec.excess(J, want, ec.magnitudes(Bd.program, [t], X, P)[1]) <= 8
    kinds = [(a >> 8, a & 0xff) for _, a, b in Bd.program.decode()] + [(b >> 8, b & 0xff) for _, a, b in Bd.program.decode()]
    for j in np.flatnonzero(pm.fixed):
        assert (E.PFIX, j) in kinds
    # a tie is computed once: two ops each at the most (ops that become equal under the map are merged)
    n_aff = int(np.sum((pm.ratio != 1) | (pm.offset != 0)))
    assert Bd.program.nops <= M.program.nops + 2 * n_aff
    assert M.bind(None).program is M.program and M.bind(bounded_lsq.ParamMap(M.n)).program.ops.tolist() == M.program.ops.tolist()
    with pytest.raises(ValueError, match="`param_map` is for"):
        M.bind(bounded_lsq.ParamMap(M.n + 1))


# ---- refusals before any GPU is touched ----------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from bounded_lsq import _curve_fit

    def boom(*a, **k):
        raise AssertionError("a context or the batch solver was reached")
    monkeypatch.setattr(_abi.Context, "__init__", boom)
    monkeypatch.setattr(_curve_fit, "least_squares_batch", boom)


@pytest.mark.parametrize("driver", ["host", "device"])
def test_binned_and_global_are_refused(no_device, driver):
    M = models.expression(DECAY, DECAY_PARAMS)
    t, Y, P0 = np.linspace(0, 1, 9), np.ones((2, 9)), np.ones((2, 5))
    with pytest.raises(ValueError, match="`binned=True` is not supported with the expression model"):
        bounded_lsq.curve_fit_batch(M, t, Y, P0, binned=True, driver=driver)
    with pytest.raises(ValueError, match="`binned=True` is not supported with the expression model"):
        bounded_lsq.curve_fit_batch(M, np.linspace(0, 1, 10), Y, P0, binned=True, driver=driver)
    with pytest.raises(ValueError, match="not supported in a global fit"):
        bounded_lsq.curve_fit_global(M, t, Y, P0, shared=[2], driver=driver)
    with pytest.raises(ValueError, match="not supported with the expression model"):
        models.binned(M)
    with pytest.raises(ValueError, match="not supported with the expression model"):
        models.DeviceFit(M, 5, t, Y, binned=True)
    with pytest.raises(ValueError, match="not supported in a global fit"):
        models.DeviceFit(M, 5, t, Y.reshape(1, 2, 9), global_map=bounded_lsq.GlobalMap(5, 2, [2]))
    with pytest.raises(ValueError, match="does not take n = 4"):
        bounded_lsq.curve_fit_batch(M, t, Y, np.ones((2, 4)), driver=driver)
    with pytest.raises(ValueError, match="callable `jac`"):
        bounded_lsq.curve_fit_batch(M, t, Y, P0, jac=lambda x, P: None, driver=driver)
    two = models.expression("a*u+v", ("a",), coords=("u", "v"))
    with pytest.raises(ValueError, match="2 coordinates"):
        bounded_lsq.curve_fit_batch(two, np.zeros((2, 9)), Y, np.ones((2, 1)), response=[1.0], driver=driver)


# ---- what the solver is handed -------------------------------------------------------------------------------------------
def test_what_an_expression_hands_to_the_batch_solver(monkeypatch):
    from bounded_lsq import _curve_fit
    seen = {}

    class Stop(Exception):
        pass

    def fake(fun, x0, jac, **kw):
        seen.update(fun=fun, x0=x0, jac=jac, kw=kw)
        raise Stop
    monkeypatch.setattr(_curve_fit, "least_squares_batch", fake)
    M = ec.model("decay")
    P, t = ec.draw("decay")
    Y = M.f(t, P) + 0.01
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(M, t, Y, P, driver="device", fixed=[4], tied={3: (2, 4.0)})
    fit = seen["fun"]
    assert isinstance(fit, models.DeviceFit) and fit.model is M and (fit.n, fit.n_model) == (3, 5)
    assert seen["jac"] is None and seen["x0"].shape == (3, 3)
    with pytest.raises(Stop):
        bounded_lsq.curve_fit_batch(M, t, Y, P, driver="host", sigma=0.5)
    assert np.array_equal(seen["fun"](P), 2.0 * (M.f(t, P) - Y))
    assert np.array_equal(seen["jac"](P), 2.0 * M.jac(t, P))


def test_host_fit_of_the_decay_case():
    """The decay case is well posed: scipy's least_squares on the numpy definition, inside a box, from a start 10 % off,
    comes back to the truth (noise-free data) — the problem the GPU test fits end to end on both drivers."""
    from scipy.optimize import least_squares
    M = ec.model("decay")
    P, _ = ec.draw("decay")
    t = np.linspace(0.0, 6.0, 70)
    Y = M.f(t, P)
    for b in range(ec.B):
        fun = lambda v: M.f(t, v[np.newaxis])[0] - Y[b]                            # noqa: E731
        jac = lambda v: M.jac(t, v[np.newaxis])[0]                                 # noqa: E731
        res = least_squares(fun, P[b] * np.array([1.1, 0.9, 1.1, 0.9, 1.1]), jac, bounds=(0.5 * P[b], 2.0 * P[b]),
                            ftol=1e-14, xtol=1e-14, gtol=1e-14)
        assert res.success
        np.testing.assert_allclose(res.x, P[b], rtol=1e-6)
