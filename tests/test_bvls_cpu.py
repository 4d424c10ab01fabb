"""BVLS / NNLS without a GPU: exports, the two ABI entries as far as they can be reached without a
context, argument handling before any context exists, and ``bvls_reference`` (the numpy definition of the iteration
the solve kernel runs) against the constructed cases, scipy's BVLS and NNLS, a conditioning sweep and the structural
loop bounds.  The cases are those tests/test_bvls_gpu.py runs."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import optimize

import bounded_lsq
from bounded_lsq import _abi, _bvls, _linear

import _bvls_cases as bc
import _linear_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOMENTS = ["blsq_ctx * ctx", "int B", "int m", "int n", "const double * dA", "long A_stride", "const double * dy",
           "const double * dw", "long w_stride", "double * dG", "long G_stride", "double * dc"]
SOLVE = ["blsq_ctx * ctx", "int B", "int m", "int n", "const double * dG", "long G_stride", "const double * dc",
         "const double * dlb", "const double * dub", "double tol", "int max_pass", "const double * dA", "long A_stride",
         "const double * dy", "const double * dw", "long w_stride", "double * dx", "int32_t * don_bound", "double * dfun",
         "double * dgrad", "double * doptimality", "int32_t * dstat"]


# ---- exports and ABI ------------------------------------------------------------------------------------------------
def test_exports():
    for name in ("bvls", "bvls_batch", "nnls_batch", "bvls_gram_batch", "bvls_reference", "BvlsResult"):
        assert getattr(bounded_lsq, name) is getattr(_bvls, name) and name in bounded_lsq.__all__
    assert _linear.METHODS == ("trf", "dogbox")                          # lsq_linear_batch is as it was


@pytest.mark.parametrize("entry,want", [("blsq_bvls_moments_dev", MOMENTS), ("blsq_bvls_solve_dev", SOLVE)])
def test_entries_are_declared_bound_and_exported(entry, want):
    lib = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blsq.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % entry, src).group(1)
    params = [" ".join(p.replace("*", " * ").split()) for p in proto.split(",")]
    assert params == want
    res, args = _abi.SIGNATURES[entry]
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
    assert res is ctypes.c_int
    assert args == [_abi.vp] + [_abi.vp if "*" in p else ctype[p.split()[0]] for p in params[1:]]
    assert hasattr(lib, entry) and entry not in _abi.MODEL_EVAL_ARGS
    assert re.search(r"#define\s+BLSQ_BVLS_MAX_N\s+128\b", src) and _bvls.BVLS_MAX_N == 128


def test_a_null_context_is_argument_one():
    """Without a device there is no context; the other positions are held on the GPU
    (test_bvls_gpu.py::test_bad_arguments_return_their_position)."""
    lib = _abi.load()
    assert lib.blsq_bvls_moments_dev(None, 1, 1, 1, None, 0, None, None, 0, None, 0, None) == -1
    assert lib.blsq_bvls_solve_dev(None, 1, 1, 1, None, 0, None, None, None, 1e-10, 1, None, 0, None, None, 0, None,
                                   None, None, None, None, None) == -1


# ---- argument handling: every refusal comes before a context exists -------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_bvls, "_context", boom)
    monkeypatch.setattr(_abi, "Context", boom)


def test_value_errors_before_any_context(no_context):
    rng = np.random.default_rng(0)
    A, b = rng.standard_normal((7, 4)), rng.standard_normal((3, 7))
    with pytest.raises(ValueError, match="lsq_linear_batch"):
        bounded_lsq.bvls_batch(rng.standard_normal((200, 129)), rng.standard_normal(200))
    with pytest.raises(ValueError, match="lsq_linear_batch"):
        bounded_lsq.bvls_gram_batch(np.eye(129), np.zeros(129))
    with pytest.raises(ValueError, match="Inconsistent shapes between `A` and `b`"):
        bounded_lsq.bvls_batch(A, rng.standard_normal((3, 6)))
    with pytest.raises(ValueError, match="`A` must have shape"):
        bounded_lsq.bvls_batch(A[0], b)
    with pytest.raises(ValueError, match="same B"):
        bounded_lsq.bvls_batch(rng.standard_normal((2, 7, 4)), b)
    with pytest.raises(ValueError, match="use `bvls_batch`"):
        bounded_lsq.bvls(A, b)
    with pytest.raises(ValueError, match="strictly less"):
        bounded_lsq.bvls_batch(A, b, bounds=(0.0, 0.0))
    with pytest.raises(ValueError, match="strictly less"):
        bounded_lsq.bvls_batch(A, b, bounds=(np.zeros(4), [1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="Inconsistent shapes between bounds"):
        bounded_lsq.bvls_batch(A, b, bounds=(np.zeros(3), np.ones(3)))
    with pytest.raises(ValueError, match="2 elements"):
        bounded_lsq.bvls_batch(A, b, bounds=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="max_iter"):
        bounded_lsq.bvls_batch(A, b, max_iter=-1)
    with pytest.raises(ValueError, match="`G` must have shape"):
        bounded_lsq.bvls_gram_batch(np.eye(3), np.zeros((2, 4)))
    with pytest.raises(ValueError, match="same B"):
        bounded_lsq.bvls_gram_batch(np.tile(np.eye(4), (3, 1, 1)), np.zeros((2, 4)))
    with pytest.raises(ValueError, match="`c` must have shape"):
        bounded_lsq.bvls_gram_batch(np.eye(4), np.zeros((2, 2, 4)))
    with pytest.raises(ValueError, match="strictly less"):
        bounded_lsq.bvls_gram_batch(np.eye(4), np.zeros(4), bounds=(1.0, 0.0))


def test_lsq_linear_batch_still_refuses_bvls(no_context):
    with pytest.raises(ValueError, match="'bvls' is not built"):
        bounded_lsq.lsq_linear_batch(np.eye(3), np.ones(3), method="bvls")


def test_result_views():
    res = _bvls.BvlsResult(x=np.arange(6.0).reshape(2, 3), cost=np.array([1.0, 2.0]), fun=None,
                           optimality=np.zeros(2), active_mask=np.zeros((2, 3), dtype=np.int32), nit=np.array([0, 4]),
                           nfact=np.array([1, 7]), status=np.array([1, 0]), success=np.array([True, False]))
    assert len(res) == 2
    one = res[1]
    assert np.array_equal(one.x, [3.0, 4.0, 5.0]) and one.cost == 2.0 and one.fun is None and one.nit == 4
    assert one.status == 0 and not one.success and "passes" in one.message
    with pytest.raises(IndexError):
        res[2]


# ---- the definition on the constructed cases ------------------------------------------------------------------------
def _problems(case):
    for p in range(case["B"]):
        A = lc.problem_matrix(case, p)
        b = case["b"][p]
        if case["sigma"] is not None:
            A, b = A / case["sigma"][:, None], b / case["sigma"]
        yield p, A, b


@pytest.mark.parametrize("name", list(lc.FIT_CASES) + ["weighted"])
def test_reference_reaches_the_constructed_solution(name):
    """Status 1, the constructed active set, passes <= 1.5 n, x* within 1 / 8 of the tolerance the GPU is held to, and
    scipy's BVLS on the same terms."""
    case = bc.weighted_case() if name == "weighted" else lc.get(name)
    n = case["n"]
    for p, A, b in _problems(case):
        r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, case["lb"][p], case["ub"][p])
        tol = bc.x_tolerance(n, case["xstar"][p]) / 8.0
        assert r["status"] == 1 and np.array_equal(r["on_bound"], case["active"][p]), (name, p)
        assert r["nit"] <= 1.5 * n and r["nfact"] <= n + 1 + 2 * r["nit"]
        assert np.max(np.abs(r["x"] - case["xstar"][p])) <= tol, (name, p)
        on = r["on_bound"]
        assert np.all(r["x"][on < 0] == case["lb"][p][on < 0]) and np.all(r["x"][on > 0] == case["ub"][p][on > 0])
        s = optimize.lsq_linear(A, b, (case["lb"][p], case["ub"][p]), method="bvls", tol=1e-14)
        assert np.array_equal(s.active_mask, on), (name, p)
        assert np.max(np.abs(r["x"] - s.x)) <= tol, (name, p)


def test_reference_on_the_nnls_case():
    c = lc.nnls_case()
    A, b = c["A"], c["b"]
    r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, 0.0, np.inf)
    tol = bc.x_tolerance(c["n"], c["xstar"]) / 8.0
    assert r["status"] == 1 and np.array_equal(r["on_bound"], [0, 0, 0, -1, -1]) and r["nit"] <= 1.5 * c["n"]
    assert np.all(r["x"][3:] == 0.0) and np.max(np.abs(r["x"] - c["xstar"])) <= tol
    assert np.max(np.abs(r["x"] - optimize.nnls(A, b)[0])) <= tol
    s = optimize.lsq_linear(A, b, (0.0, np.inf), method="bvls", tol=1e-14)
    assert np.array_equal(s.active_mask, r["on_bound"]) and np.max(np.abs(r["x"] - s.x)) <= tol


@pytest.mark.parametrize("n", bc.GRAM_NS)
def test_gram_cases_are_constructed_solutions(n):
    """The cases of the Gram-only GPU test: the definition reaches their constructed active set."""
    case = bc.gram_case(n)
    for p in range(case["B"]):
        r = bounded_lsq.bvls_reference(case["G"], case["c"][p], case["lb"][p], case["ub"][p])
        assert r["status"] == 1 and np.array_equal(r["on_bound"], case["active"][p]), (n, p)
        assert np.max(np.abs(r["x"] - case["xstar"][p])) <= bc.x_tolerance(n, case["xstar"][p]) / 8.0


# ---- the sweep ------------------------------------------------------------------------------------------------------
def test_sweep_against_scipy():
    """96 seeded draws, kappa up to 1e6: status 1 and scipy's active set on every one; the pass and factorisation counts
    stay inside what the issue measured (1.5 n and 2.4 n)."""
    worst_pass = worst_fact = 0.0
    for kappa, m, n, seed in bc.sweep():
        A, b = bc.draw(m, n, kappa, seed)
        r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX)
        s = optimize.lsq_linear(A, b, (-bc.BOX, bc.BOX), method="bvls", tol=1e-14)
        assert r["status"] == 1, (kappa, m, n, seed)
        assert np.array_equal(r["on_bound"], s.active_mask), (kappa, m, n, seed)
        assert np.all(np.abs(r["x"][r["on_bound"] != 0]) == bc.BOX)
        worst_pass, worst_fact = max(worst_pass, r["nit"] / n), max(worst_fact, r["nfact"] / n)
    print("passes / n <= %.3g, factorisations / n <= %.3g" % (worst_pass, worst_fact))
    assert worst_pass <= 1.5 and worst_fact <= 2.4


@pytest.mark.parametrize("base", bc.OTHER_SWEEP_SEEDS)
def test_sweep_from_seeds_not_chosen(base):
    """The same sweep from seeds kept as they were drawn: status 1 on every draw, and scipy's mask or, where scipy
    stopped short of its final active set, a cost that is not above scipy's."""
    differ = 0
    for kappa, m, n, seed in bc.sweep(base):
        A, b = bc.draw(m, n, kappa, seed)
        r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX)
        s = optimize.lsq_linear(A, b, (-bc.BOX, bc.BOX), method="bvls", tol=1e-14)
        assert r["status"] == 1, (kappa, m, n, seed)
        assert bc.agrees_with_scipy(A, b, r["x"], r["on_bound"], s), (kappa, m, n, seed)
        differ += not np.array_equal(r["on_bound"], s.active_mask)
        assert r["nit"] <= 1.5 * n and r["nfact"] <= 2.4 * n
    assert differ <= 3


def test_narrow_boxes_status_one_means_kkt():
    """A thousand small problems in narrow boxes, every seed kept: a released variable that crosses to its opposite
    bound does not end the pass.  Status 1 on every draw, the optimality from g = G x - c under its bound, scipy's mask
    (or a cost not above scipy's where scipy did not finish)."""
    worst, differ = 0.0, 0
    for seed in bc.NARROW_SEEDS:
        A, b, box, s = bc.narrow_with_scipy(seed)
        G, c = A.T @ A, A.T @ b
        r = bounded_lsq.bvls_reference(G, c, -box, box)
        assert r["status"] == 1 and r["nit"] <= 5 * len(c), seed
        opt, bound = bc.kkt_optimality(r["g"], r["on_bound"]), bc.kkt_bound(G, c, r["x"])
        assert opt <= bound, (seed, opt, bound)
        assert bc.agrees_with_scipy(A, b, r["x"], r["on_bound"], s), seed
        worst, differ = max(worst, opt / bound), differ + (not np.array_equal(r["on_bound"], s.active_mask))
    print("narrow boxes: optimality at most %.3g of its bound, %d masks differ from scipy's" % (worst, differ))
    assert differ <= 2


def test_draws_whose_released_variable_crosses_the_box():
    """Three of the narrow draws on which a released variable lands on its opposite bound, the first dropped in its
    pass: ending the pass there returns status 1 with an optimality of 0.1, 7.6 and 60.  The drop loop goes on."""
    seen = 0
    for seed in (301, 715, 893):                                    # draws whose first pass drops its own variable
        A, b, box, s = bc.narrow_with_scipy(seed)
        G, c = A.T @ A, A.T @ b
        r = bounded_lsq.bvls_reference(G, c, -box, box)
        assert r["status"] == 1 and np.array_equal(r["on_bound"], s.active_mask), seed
        assert bc.kkt_optimality(r["g"], r["on_bound"]) <= bc.kkt_bound(G, c, r["x"]), seed
        seen += 1
    assert seen == 3


@pytest.mark.parametrize("draw", bc.CONDITIONING)
def test_the_correction_against_A_takes_back_the_conditioning(draw):
    """The ordering the GPU test asserts, in numpy: x after one CSNE step is closer to scipy's than the Gram-domain x."""
    kappa, m, n, seed = draw
    A, b = bc.draw(m, n, kappa, seed)
    r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX)
    s = optimize.lsq_linear(A, b, (-bc.BOX, bc.BOX), method="bvls", tol=1e-14)
    assert r["status"] == 1 and np.array_equal(r["on_bound"], s.active_mask)
    xf = bc.csne_finish(A, b, r["x"], r["on_bound"], -bc.BOX, bc.BOX)
    assert np.max(np.abs(xf - s.x)) < np.max(np.abs(r["x"] - s.x))


# ---- the structural bounds ------------------------------------------------------------------------------------------
def test_max_iter_and_feasibility():
    kappa, m, n, seed = 30.0, 130, 17, bc.SWEEP_SEED + 7
    A, b = bc.draw(m, n, kappa, seed)
    full = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX)
    assert full["status"] == 1 and full["nit"] >= 2                 # (so that one pass is not enough)
    r = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX, max_iter=1)
    assert r["status"] == 0 and r["nit"] == 1 and np.all(np.abs(r["x"]) <= bc.BOX)
    r0 = bounded_lsq.bvls_reference(A.T @ A, A.T @ b, -bc.BOX, bc.BOX, max_iter=0)
    assert r0["status"] == 0 and r0["nit"] == 0


@pytest.mark.parametrize("n", [1, 6, 17])
def test_nan_and_singular_end_with_status_minus_one_inside_the_bounds(n):
    case = bc.gram_case(n)
    G, c, lb, ub = case["G"], case["c"][0], case["lb"][0], case["ub"][0]
    for where in ("G", "c"):
        Gn, cn = G.copy(), c.copy()
        (Gn if where == "G" else cn)[..., 0] = np.nan
        r = bounded_lsq.bvls_reference(Gn, cn, lb, ub)
        assert r["status"] == -1 and r["nit"] == 0 and r["nfact"] == 1, (n, where)
        assert np.all((r["x"] >= lb) & (r["x"] <= ub))


def test_a_singular_gram_matrix_is_status_minus_one():
    G, c, lb, ub = bc.singular_case()
    for p in range(3):
        r = bounded_lsq.bvls_reference(G, c[p], lb, ub)
        assert r["status"] == -1 and r["nit"] == 0 and r["nfact"] == 1
        assert np.all((r["x"] >= lb) & (r["x"] <= ub))
