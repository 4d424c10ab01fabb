"""BVLS / NNLS with a sum constraint without a GPU: the export, the new ABI entry as far as it can be
reached without a context, argument handling before any context exists, the entry each call reaches (with a recording
library in the place of the real one), and ``bvls_reference(..., equality=)`` (the numpy definition of the iteration
the solve kernel runs) against a brute-force search over all active sets, the constructed cases and the infeasible
boxes.  The cases are those tests/test_fcls_gpu.py runs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import bounded_lsq
from bounded_lsq import _abi, _bvls

import _bvls_cases as bc
import _fcls_cases as fc
from test_bvls_cpu import SOLVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_EQ = SOLVE + ["const double * de", "long e_stride", "const double * dd", "double * dmultiplier"]


# ---- exports and ABI ------------------------------------------------------------------------------------------------
def test_exports_and_keywords():
    assert bounded_lsq.fcls_batch is _bvls.fcls_batch and "fcls_batch" in bounded_lsq.__all__
    for name in ("bvls_batch", "bvls", "nnls_batch", "bvls_gram_batch", "bvls_reference"):
        params = list(inspect.signature(getattr(bounded_lsq, name)).parameters.values())
        assert params[-1].name == "equality" and params[-1].default is None, name    # last: positional calls keep
    assert list(inspect.signature(bounded_lsq.fcls_batch).parameters)[:3] == ["A", "b", "sigma"]
    assert -2 in _bvls.MESSAGES and "multiplier" in _bvls.BvlsResult.FIELDS
    res = _bvls.BvlsResult(x=np.zeros((1, 2)), status=np.array([-2]))
    assert res.multiplier is None and res[0].multiplier is None and "equality" in res[0].message


def test_the_entry_is_declared_bound_and_exported():
    entry = "blsq_bvls_solve_eq_dev"
    lib = _abi.load()
    text = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % entry, src).group(1)
    params = [" ".join(p.replace("*", " * ").split()) for p in proto.split(",")]
    assert params == SOLVE_EQ
    res, args = _abi.SIGNATURES[entry]
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
    assert res is ctypes.c_int
    assert args == [_abi.vp] + [_abi.vp if "*" in p else ctype[p.split()[0]] for p in params[1:]]
    assert hasattr(lib, entry) and entry not in _abi.MODEL_EVAL_ARGS
    # the older entry keeps its signature, and the new one's first 22 arguments are that signature
    assert _abi.SIGNATURES["blsq_bvls_solve_dev"][1] == args[:22]
    # the positions of the new arguments and status -2 are documented with the entry
    assert re.search(r"e = 23, e_stride = 24, d = 25, multiplier = 26", text) and re.search(r"alone -2", text)


def test_a_null_context_is_argument_one():
    lib = _abi.load()
    assert lib.blsq_bvls_solve_eq_dev(None, 1, 1, 1, None, 0, None, None, None, 1e-10, 1, None, 0, None, None, 0, None,
                                      None, None, None, None, None, None, 0, None, None) == -1


# ---- argument handling ----------------------------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_bvls, "_context", boom)
    monkeypatch.setattr(_abi, "Context", boom)


def test_value_errors_before_any_context(no_context):
    rng = np.random.default_rng(0)
    A, b = rng.standard_normal((7, 4)), rng.standard_normal((3, 7))
    G, c = A.T @ A, b @ A
    for call in (lambda eq: bounded_lsq.bvls_batch(A, b, (0.0, 1.0), equality=eq),
                 lambda eq: bounded_lsq.nnls_batch(A, b, equality=eq),
                 lambda eq: bounded_lsq.bvls_gram_batch(G, c, (0.0, 1.0), equality=eq)):
        for e in ([1.0, 0.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], 0.0):
            with pytest.raises(ValueError, match="finite and not zero"):
                call((e, 1.0))
        for e, d in ((np.ones(3), 1.0), (np.ones((2, 4)), 1.0), (np.ones((3, 5)), 1.0), (1.0, np.ones(2)),
                     (np.ones((1, 3, 4)), 1.0)):
            with pytest.raises(ValueError, match="Inconsistent shapes between `equality`"):
                call((e, d))
        for d in (np.nan, np.inf, [1.0, -np.inf, 1.0]):
            with pytest.raises(ValueError, match="`d` of `equality` must be finite"):
                call((1.0, d))
        for eq in (1.0, (1.0,), (1.0, 1.0, 1.0)):
            with pytest.raises(ValueError, match="pair"):
                call(eq)
    with pytest.raises(ValueError, match="finite and not zero"):
        bounded_lsq.bvls(A, b[0], (0.0, 1.0), equality=(np.zeros(4), 1.0))


class _Recorder:
    """In the place of a context and of its library: every entry returns 0 and is recorded with its arguments."""
    h = None

    def __init__(self):
        self.lib, self.calls = self, []

    def __getattr__(self, name):
        if not name.startswith("blsq_"):
            raise AttributeError(name)

        def entry(*a):
            if name != "blsq_memcpy_h2d":
                self.calls.append((name, a))
            return 0
        return entry

    def malloc(self, nbytes):
        return ctypes.c_void_p(1 << 20)

    def free(self, p):
        pass

    def check(self, rc, what):
        assert rc == 0, what

    def to_host(self, p, shape, dtype):
        return np.zeros(shape, dtype=dtype)


def test_the_entry_each_call_reaches():
    """Without ``equality`` (left out, or None) a call goes through blsq_bvls_solve_dev with its 22 arguments and never
    reaches the new entry; with it, through blsq_bvls_solve_eq_dev alone, e_stride 0 for a shared e and n for (B, n)."""
    rng = np.random.default_rng(1)
    A, b = rng.standard_normal((7, 4)), rng.standard_normal((3, 7))
    for kw in ({}, {"equality": None}):
        rec = _Recorder()
        res = bounded_lsq.bvls_batch(A, b, (0.0, 1.0), ctx=rec, **kw)
        bounded_lsq.nnls_batch(A, b, ctx=rec, **kw)
        bounded_lsq.bvls(A, b[0], (0.0, 1.0), ctx=rec, **kw)
        bounded_lsq.bvls_gram_batch(A.T @ A, b @ A, (0.0, 1.0), ctx=rec, **kw)
        names = [name for name, _ in rec.calls]
        assert names == ["blsq_bvls_moments_dev", "blsq_bvls_solve_dev"] * 3 + ["blsq_bvls_solve_dev"]
        assert all(len(a) == 22 for name, a in rec.calls if name == "blsq_bvls_solve_dev")
        assert res.multiplier is None
    rec = _Recorder()
    res = bounded_lsq.bvls_batch(A, b, (0.0, 1.0), ctx=rec, equality=(1.0, 1.0))
    bounded_lsq.fcls_batch(A, b, ctx=rec)
    bounded_lsq.bvls_gram_batch(A.T @ A, b @ A, (0.0, 1.0), ctx=rec, equality=(np.ones((3, 4)), np.ones(3)))
    names = [name for name, _ in rec.calls]
    assert names == ["blsq_bvls_moments_dev", "blsq_bvls_solve_eq_dev"] * 2 + ["blsq_bvls_solve_eq_dev"]
    eq_calls = [a for name, a in rec.calls if name == "blsq_bvls_solve_eq_dev"]
    assert all(len(a) == 26 and a[22] is not None and a[24] is not None and a[25] is not None for a in eq_calls)
    assert [a[23] for a in eq_calls] == [0, 0, 4]
    assert res.multiplier.shape == (3,)


# ---- the definition against a brute-force search --------------------------------------------------------------------
@pytest.mark.parametrize("kind", fc.KINDS)
def test_reference_against_all_active_sets(kind):
    """110 seeded draws of each kind, n = 1 .. 5: status 1 and the minimiser found by solving the KKT system of every
    one of the 3^n active sets in numpy.longdouble; where no active set gives a feasible point, status -2."""
    solved = infeasible = 0
    for k in range(fc.BRUTE_DRAWS):
        G, c, lb, ub, e, d = fc.brute_draw(kind, 100 * k + fc.KINDS.index(kind))
        n = len(c)
        r = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(e, d))
        best = fc.brute_force(G, c, lb, ub, e, d)
        if best is None:
            assert not fc.feasible(lb, ub, e, d) and r["status"] == -2, (kind, k)
            assert np.array_equal(r["x"], np.clip(np.zeros(n), lb, ub)) and r["nit"] == 0 and r["nfact"] == 0
            infeasible += 1
            continue
        x = best[0].astype(np.float64)
        assert r["status"] == 1 and r["nit"] <= 5 * n, (kind, k)
        assert np.max(np.abs(r["x"] - x)) <= bc.x_tolerance(n, x) / 8.0, (kind, k)
        on = r["on_bound"]
        assert np.all(r["x"][on < 0] == lb[on < 0]) and np.all(r["x"][on > 0] == ub[on > 0])
        assert abs(e @ r["x"] - d) <= fc.sum_bound(e, r["x"]), (kind, k)
        assert r["optimality"] <= fc.kkt_bound(G, c, r["x"], e, r["multiplier"]), (kind, k)
        solved += 1
    print("%s: %d solved, %d infeasible" % (kind, solved, infeasible))
    assert solved + infeasible == fc.BRUTE_DRAWS and solved >= 90
    assert infeasible == 0 if kind == "simplex" else infeasible > 0  # (the simplex always has a point of sum 1)


# ---- the definition on the constructed cases ------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.GRAM_NS)
def test_reference_reaches_the_constructed_solution(n):
    """Status 1, the constructed active set, x* within 1 / 8 of the tolerance the GPU is held to, lambda*, and the
    certificate: the sum, the bounds bit for bit, the optimality under its bound."""
    case = fc.gram_case(n)
    G, e = case["G"], case["e"]
    for p in range(case["B"]):
        c, lb, ub, d = case["c"][p], case["lb"][p], case["ub"][p], case["d"][p]
        r = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(e, d))
        assert r["status"] == 1 and np.array_equal(r["on_bound"], case["active"][p]), (n, p)
        assert r["nit"] <= 1.5 * n + 1 and r["nfact"] <= n + 1 + 2 * r["nit"]
        assert np.max(np.abs(r["x"] - case["xstar"][p])) <= bc.x_tolerance(n, case["xstar"][p]) / 8.0, (n, p)
        on = r["on_bound"]
        assert np.all(r["x"][on < 0] == lb[on < 0]) and np.all(r["x"][on > 0] == ub[on > 0])
        assert abs(e @ r["x"] - d) <= fc.sum_bound(e, r["x"]), (n, p)
        lam = float(fc.multiplier_ld(r["g"], on, e))
        assert abs(r["multiplier"] - lam) <= 1e-12 * max(1.0, abs(lam))
        assert abs(lam - case["lam"][p]) <= fc.lam_tolerance(G, n, case["xstar"][p], e) / 8.0, (n, p)
        assert fc.optimality_ld(r["g"], on, e, lam) <= fc.kkt_bound(G, c, r["x"], e, lam), (n, p)
        x, l = fc.kkt_on_active_set(G, c, lb, ub, e, d, on)
        assert np.max(np.abs(r["x"] - x.astype(np.float64))) <= bc.x_tolerance(n, case["xstar"][p]) / 8.0


@pytest.mark.parametrize("name", list(fc.WHOLE))
def test_whole_path_cases_are_constructed_solutions(name):
    case = fc.whole_case(name)
    for p in range(case["B"]):
        A = case["A"] if case["shared"] else case["A"][p]
        b = case["b"][p]
        if case["sigma"] is not None:
            A, b = A / case["sigma"][:, None], b / case["sigma"]
        r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, case["lb"][p], case["ub"][p],
                                       equality=(case["e"], case["d"][p]))
        assert r["status"] == 1 and np.array_equal(r["on_bound"], case["active"][p]), (name, p)
        assert np.max(np.abs(r["x"] - case["xstar"][p])) <= bc.x_tolerance(case["n"], case["xstar"][p]) / 8.0


def test_reference_on_the_simplex_case():
    s = fc.simplex_case()
    A, b = s["A"], s["b"]
    r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, 0.0, np.inf, equality=(1.0, 1.0))
    assert r["status"] == 1 and np.array_equal(r["on_bound"], s["active"])
    assert np.all(r["x"][3:] == 0.0) and abs(r["x"].sum() - 1.0) <= fc.sum_bound(np.ones(5), r["x"])
    assert np.max(np.abs(r["x"] - s["xstar"])) <= bc.x_tolerance(s["n"], s["xstar"], s["kappa"]) / 8.0
    assert abs(r["multiplier"] - s["lam"]) <= fc.lam_tolerance(A.T @ A, 5, s["xstar"], np.ones(5), s["kappa"]) / 8.0
    free = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, 0.0, np.inf)             # without the sum: another answer
    assert "multiplier" not in free and abs(free["x"].sum() - 1.0) > 1e-5


# ---- status -2, -1, and the structural bounds -----------------------------------------------------------------------
def test_infeasible_boxes_give_minus_two():
    case = fc.gram_case(6)
    G, c = case["G"], case["c"][0]
    for lb, ub, e, d in ((0.0, 1.0, 1.0, 6.5), (0.0, 1.0, 1.0, -0.5), (-1.0, 1.0, [1, -1, 1, -1, 1, -1], 7.0),
                         (0.0, np.inf, 1.0, -1.0), (-np.inf, 0.0, [1, 1, 1, 1, 1, 2.0], 0.5)):
        r = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(np.asarray(e, dtype=float), d))
        assert r["status"] == -2 and r["nit"] == 0 and r["nfact"] == 0, (lb, ub, d)
        assert np.array_equal(r["x"], np.clip(np.zeros(6), lb, ub))
    # on the edge of the reach the only feasible point is a vertex: every variable on a bound, status 1
    r = bounded_lsq.bvls_reference(G, c, 0.0, 1.0, equality=(1.0, 6.0))
    assert r["status"] == 1 and np.all(r["on_bound"] == 1) and np.all(r["x"] == 1.0) and r["nfact"] == 0


def test_every_variable_on_a_bound_from_the_start():
    """x = (0.5, 0.5, 0, 0, 0, 0) is where the walk ends in the box [0, 0.5]^6 with sum 1: no free variable, the
    multiplier comes from the interval, and a singleton free set (pinned by the equality) is always accepted."""
    for seed in range(20):
        G, c, _, _, _, _ = fc.brute_draw("simplex", 7000 + seed)
        n = len(c)
        if n < 3:
            continue
        r = bounded_lsq.bvls_reference(G, c, 0.0, 0.5, equality=(1.0, 1.0))
        best = fc.brute_force(G, c, np.zeros(n), np.full(n, 0.5), np.ones(n), 1.0)
        assert r["status"] == 1 and r["nit"] <= 5 * n, seed
        assert np.max(np.abs(r["x"] - best[0].astype(np.float64))) <= bc.x_tolerance(n, r["x"]) / 8.0, seed


def test_max_iter_zero_is_the_feasible_start_after_its_drop_loop():
    case = fc.gram_case(17)
    e = case["e"]
    for p in range(case["B"]):
        G, c, lb, ub, d = case["G"], case["c"][p], case["lb"][p], case["ub"][p], case["d"][p]
        r = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(e, d), max_iter=0)
        assert r["status"] in (0, 1) and r["nit"] == 0
        assert np.all((r["x"] >= lb) & (r["x"] <= ub)) and abs(e @ r["x"] - d) <= fc.sum_bound(e, r["x"])
    full = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(e, d))
    one = bounded_lsq.bvls_reference(G, c, lb, ub, equality=(e, d), max_iter=1)
    assert full["nit"] >= 2 and one["status"] == 0 and one["nit"] == 1


@pytest.mark.parametrize("n", [1, 6, 17])
def test_nan_ends_with_status_minus_one_inside_the_bounds(n):
    case = fc.gram_case(n)
    G, c, lb, ub, e, d = case["G"], case["c"][0], case["lb"][0], case["ub"][0], case["e"], case["d"][0]
    for where in ("G", "c", "e", "d"):
        Gn, cn, en, dn = G.copy(), c.copy(), e.copy(), d
        if where == "d":
            dn = np.nan
        else:
            {"G": Gn, "c": cn, "e": en}[where][..., 0] = np.nan
        r = bounded_lsq.bvls_reference(Gn, cn, lb, ub, equality=(en, dn))
        assert r["status"] == -1 and r["nit"] == 0, (n, where)
        assert r["nfact"] == 0 or where in ("G", "c"), (n, where)    # (e and d are refused before any solve)
        assert np.all((r["x"] >= lb) & (r["x"] <= ub))
    ez = e.copy()
    ez[0] = 0.0
    assert bounded_lsq.bvls_reference(G, c, lb, ub, equality=(ez, d))["status"] == -1
