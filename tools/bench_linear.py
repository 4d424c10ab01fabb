"""Bounded linear least squares on the device (linear_kernels.hip): what the device route saves a batch.

B problems ``min |A x - b|^2, 0 <= x <= 1`` against ONE (m, n) matrix (``--own``: one matrix per problem), about a quarter
of the variables on a bound at the solution.  ``lsq_linear_batch(driver='device')``, where A, b and x stay on the GPU,
against the callable route a user had before it: ``numpy_callbacks`` through ``least_squares_batch(driver='device')``,
which evaluates A x - b on the host and ships the B m n doubles of the unchanging Jacobian for every accepted step.  Same
GPU, same process, alternating; whole calls are timed (host clock around a call that ends in a download), median of
`--repeat` after one warm-up each.  A further call of the device route with every slot timed gives `slots_ms`.

``--kernel`` times the launches of blsq_linear_eval_dev alone instead: `--launches` launches each of f and of J in the
'model_eval' slot, `--rounds` timed blocks (the figure is the median of the rounds' means), for a shared and for
per-problem matrices on buffers of the same shapes.

``--method bvls`` (bvls_kernels.hip) times ``bvls_batch`` on the same batch against
``lsq_linear_batch`` with 'trf' and with 'dogbox' in one process (one block of repeats per route after its warm-up),
and prints the release passes and the
factorisations per problem as max and mean; with ``--kernel`` it times the moments launch and the solve launch
separately instead (`--rounds` blocks of `--launches` launches each, the median of the blocks' means; no weights).
``--method bvls --sum-to D`` adds the equality ``sum x = D``: ``bvls_batch(..., equality=(1, D))`` is timed
against the unconstrained ``bvls_batch`` of the same data in the same run (problems per second, release passes and
factorisations of both); with ``--kernel`` the solve launch of blsq_bvls_solve_eq_dev is timed beside the one of
blsq_bvls_solve_dev, each with its factorisations and its time per factorisation.

usage: python tools/bench_linear.py [--B 4096] [--m 64] [--n 16] [--method trf] [--own] [--repeat 5]
                                    [--kernel] [--launches 200] [--rounds 5] [--sum-to D]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import (lsq_linear_batch, least_squares_batch, bvls_batch, LinearDeviceModel, _abi, _bvls,  # noqa: E402
                         _linear)

METHODS = _linear.METHODS + ('bvls',)           # of this tool: lsq_linear_batch itself does not take 'bvls'


def problems(B, m, n, own, seed=0):
    """A with singular values in [20, 600]; b = A x_true + noise with x_true drawn over [-0.25, 1.25] and the box
    [0, 1]: roughly a quarter of the variables end on a bound."""
    rng = np.random.default_rng(seed)

    def matrix():
        U, _ = np.linalg.qr(rng.standard_normal((m, n)))
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return (U * np.logspace(np.log10(600.0), np.log10(20.0), n)) @ V.T
    A = np.stack([matrix() for _ in range(B)]) if own else matrix()
    xt = rng.uniform(-0.25, 1.25, (B, n))
    b = (A @ xt[:, :, None])[..., 0] + 0.05 * rng.standard_normal((B, m))
    return A, b


def kernel_times(ctx, A, b, launches, rounds):
    out = {}
    B, m = b.shape
    n = A.shape[-1]
    for name, Am in (("shared", A if A.ndim == 2 else A[0]),
                     ("own", A if A.ndim == 3 else np.ascontiguousarray(np.broadcast_to(A, (B, m, n))))):
        dm = LinearDeviceModel(ctx, Am, b)
        d_x = ctx.to_device(np.full((B, n), 0.5))
        d_f, d_J = ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * n)
        for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
            call()
            ctx.sync()
            per_round = []
            for _ in range(rounds):
                ctx.timing(True, only="model_eval")
                ctx.timing_reset()
                for _ in range(launches):
                    call()
                ctx.sync()
                ms, cnt = ctx.timing_read()["model_eval"]
                ctx.timing(False)
                per_round.append(round(1e3 * ms / cnt, 2))
            out["%s_%s_us" % (name, what)] = round(float(np.median(per_round)), 2)
            out["%s_%s_us_all" % (name, what)] = per_round
        for p in (d_x, d_f, d_J):
            ctx.free(p)
        dm.close()
    # bytes the algorithm needs: f reads A (once if shared), x and b and writes f; J reads A and writes B copies
    out["f_bytes"] = {"shared": 8 * (m * n + B * (n + 2 * m)), "own": 8 * B * (m * n + n + 2 * m)}
    out["J_bytes"] = {"shared": 8 * (m * n + B * m * n), "own": 16 * B * m * n}
    return out


def bvls_kernel_times(ctx, A, b, lb, ub, launches, rounds, sum_to=None):
    """The moments launch and the solve launch of one ``bvls_batch`` (no weights), each alone in the 'model_eval' slot:
    `rounds` timed blocks of `launches` launches after a warm-up, the median of the blocks' means, in ms.  `sum_to`: the
    solve launch under ``sum x = sum_to`` as well (``solve_eq_*``), on the same moments."""
    B, m = b.shape
    n = A.shape[-1]
    A_stride = m * n if A.ndim == 3 else 0
    G_stride = n * n if A_stride else 0
    eq = None if sum_to is None else (np.ones(n), np.full(B, float(sum_to)))
    need = _bvls._Buffers.need(A, b, lb, ub, 8 * n * n * (B if G_stride else 1), 8 * B * n,
                               *_bvls._output_bytes(B, m, n, True), *_bvls._equality_bytes(eq, B))
    with _bvls._Buffers(ctx, need) as buf:
        d_A, d_y, d_lb, d_ub = buf.up(A), buf.up(b), buf.up(lb), buf.up(ub)
        d_G, d_c = buf.new(8 * n * n * (B if G_stride else 1)), buf.new(8 * B * n)
        d_x, d_on, d_fun, d_grad = buf.new(8 * B * n), buf.new(4 * B * n), buf.new(8 * B * m), buf.new(8 * B * n)
        d_opt, d_stat = buf.new(16 * B), buf.new(12 * B)
        calls = {"moments": lambda: ctx.check(ctx.lib.blsq_bvls_moments_dev(ctx.h, B, m, n, d_A, A_stride, d_y, None, 0,
                                                                           d_G, G_stride, d_c), "moments"),
                 "solve": lambda: ctx.check(ctx.lib.blsq_bvls_solve_dev(ctx.h, B, m, n, d_G, G_stride, d_c, d_lb, d_ub,
                                                                       1e-10, 5 * n, d_A, A_stride, d_y, None, 0, d_x,
                                                                       d_on, d_fun, d_grad, d_opt, d_stat), "solve")}
        if eq is not None:
            d_e, d_d, d_mult = buf.up(eq[0]), buf.up(eq[1]), buf.new(8 * B)
            calls["solve_eq"] = lambda: ctx.check(ctx.lib.blsq_bvls_solve_eq_dev(
                ctx.h, B, m, n, d_G, G_stride, d_c, d_lb, d_ub, 1e-10, 5 * n, d_A, A_stride, d_y, None, 0, d_x, d_on,
                d_fun, d_grad, d_opt, d_stat, d_e, 0, d_d, d_mult), "solve_eq")
        out, stats = {}, {}
        for name, call in calls.items():
            call()
            ctx.sync()
            ms_all = []
            for _ in range(rounds):
                ctx.timing(True, only="model_eval")
                ctx.timing_reset()
                for _ in range(launches):
                    call()
                ctx.sync()
                ms, cnt = ctx.timing_read()["model_eval"]
                ms_all.append(round(ms / cnt, 4))
                ctx.timing(False)
            out[name + "_ms"] = float(np.median(ms_all))
            out[name + "_ms_all"] = ms_all
            if name != "moments":
                stats[name] = ctx.to_host(d_stat, (B, 3), np.int32)
    stat = stats["solve"]
    out["factorisations"] = int(stat[:, 2].sum())
    out["factorisations_mean"] = round(float(stat[:, 2].mean()), 3)
    # the chip's throughput: the solve launch over all factorisations of the batch (gradients and ratio tests included)
    out["solve_ns_per_factorisation"] = round(1e6 * out["solve_ms"] / max(int(stat[:, 2].sum()), 1), 1)
    if eq is not None:
        stat = stats["solve_eq"]
        out.update({"sum_to": float(sum_to), "passes_mean": round(float(stats["solve"][:, 1].mean()), 3),
                    "solve_eq_status": sorted(set(int(v) for v in stat[:, 0])),
                    "solve_eq_passes_mean": round(float(stat[:, 1].mean()), 3),
                    "solve_eq_factorisations": int(stat[:, 2].sum()),
                    "solve_eq_factorisations_mean": round(float(stat[:, 2].mean()), 3),
                    "solve_eq_ns_per_factorisation": round(1e6 * out["solve_eq_ms"] / max(int(stat[:, 2].sum()), 1), 1),
                    "solve_problems_per_s": round(1e3 * B / out["solve_ms"]),
                    "solve_eq_problems_per_s": round(1e3 * B / out["solve_eq_ms"])})
        out["ns_per_factorisation_ratio"] = round(out["solve_eq_ns_per_factorisation"]
                                                  / out["solve_ns_per_factorisation"], 3)
    return out


def bvls_sum_main(a, A, b, ctx, res, lb, ub):
    """``bvls_batch`` under ``sum x = a.sum_to`` against the unconstrained ``bvls_batch`` of the same data, alternating
    blocks in one process: whole calls, the median of `--repeat` after one warm-up each."""
    routes = {"bvls": lambda: bvls_batch(A, b, (lb, ub), ctx=ctx),
              "bvls_eq": lambda: bvls_batch(A, b, (lb, ub), ctx=ctx, equality=(1.0, a.sum_to))}
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    res["sum_to"] = a.sum_to
    for k, r in out.items():
        t = float(np.median(times[k]))
        res[k] = {"s": round(t, 4), "all_s": [round(v, 4) for v in times[k]], "problems_per_s": round(a.B / t),
                  "status": {str(v): int(np.sum(r.status == v)) for v in sorted(set(int(v) for v in r.status))},
                  "passes_mean": round(float(r.nit.mean()), 3), "factorisations_mean": round(float(r.nfact.mean()), 3),
                  "active_share": round(float(np.mean(r.active_mask != 0)), 3),
                  "max_optimality": float(np.max(r.optimality[r.status == 1], initial=0.0))}
    r = out["bvls_eq"]
    ok = r.status == 1
    res["bvls_eq"]["max_sum_error"] = float(np.max(np.abs(r.x[ok].sum(axis=1) - a.sum_to), initial=0.0))


def bvls_main(a, A, b, ctx, res):
    lb, ub = np.zeros((a.B, a.n)), np.ones((a.B, a.n))
    if a.kernel:
        res.update(launches=a.launches, rounds=a.rounds)
        res.update(bvls_kernel_times(ctx, A, b, lb, ub, a.launches, a.rounds, a.sum_to))
        return
    if a.sum_to is not None:
        bvls_sum_main(a, A, b, ctx, res, lb, ub)
        return
    tol = 1e-10
    x0 = np.full((a.B, a.n), 0.5)
    routes = {"bvls": lambda: bvls_batch(A, b, (lb, ub), tol=tol, ctx=ctx),
              "trf": lambda: lsq_linear_batch(A, b, bounds=(lb, ub), method="trf", tol=tol, x0=x0, ctx=ctx),
              "dogbox": lambda: lsq_linear_batch(A, b, bounds=(lb, ub), method="dogbox", tol=tol, x0=x0, ctx=ctx)}
    times = {k: [] for k in routes}
    out = {}
    for k, run in routes.items():                                         # one block per route: a route's big device
        out[k] = run()                                                    # buffers, released, slow the next allocations
        for _ in range(a.repeat):                                         # of any route
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    r = out["bvls"]
    for k in routes:
        res[k + "_s"] = round(float(np.median(times[k])), 4)
        res[k + "_all_s"] = [round(t, 4) for t in times[k]]
    X = {k: np.stack([q.x for q in out[k]]) for k in ("trf", "dogbox")}
    res.update({"speedup_over_trf": round(res["trf_s"] / res["bvls_s"], 2),
                "speedup_over_dogbox": round(res["dogbox_s"] / res["bvls_s"], 2),
                "status": sorted(set(int(v) for v in r.status)),
                "passes": {"max": int(r.nit.max()), "mean": round(float(r.nit.mean()), 3)},
                "factorisations": {"max": int(r.nfact.max()), "mean": round(float(r.nfact.mean()), 3)},
                "active_share": round(float(np.mean(r.active_mask != 0)), 3),
                "max_optimality": float(r.optimality.max()),
                "x_max_abs_diff": {k: float(np.max(np.abs(r.x - X[k]))) for k in X},
                # cost of the other route less the cost here, over the problems: [min, max] (an exact minimiser: >= 0)
                "cost_excess": {k: [float(f(np.array([q.cost for q in out[k]]) - r.cost)) for f in (np.min, np.max)]
                                for k in X}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--method", default="trf", choices=METHODS)
    ap.add_argument("--own", action="store_true", help="one matrix per problem instead of one for all")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--kernel", action="store_true", help="time the kernel's launches alone")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5, help="with --kernel: timed blocks of --launches launches each")
    ap.add_argument("--sum-to", type=float, default=None, dest="sum_to",
                    help="with --method bvls: the equality sum x = SUM_TO as well")
    a = ap.parse_args()
    if a.sum_to is not None and a.method != "bvls":
        ap.error("--sum-to goes with --method bvls")
    A, b = problems(a.B, a.m, a.n, a.own)
    ctx = _abi.Context(0)
    res = {"B": a.B, "m": a.m, "n": a.n, "shared": not a.own, "method": a.method}
    if a.method == "bvls":
        bvls_main(a, A, b, ctx, res)
        ctx.close()
        print(json.dumps(res))
        return
    if a.kernel:
        res.update(launches=a.launches, rounds=a.rounds)
        res.update(kernel_times(ctx, A, b, a.launches, a.rounds))
        ctx.close()
        print(json.dumps(res))
        return
    tol = 1e-10
    lb, ub = np.zeros((a.B, a.n)), np.ones((a.B, a.n))
    x0 = np.full((a.B, a.n), 0.5)
    fun, jac = _linear.numpy_callbacks(A, b)
    routes = {"device": lambda: lsq_linear_batch(A, b, bounds=(lb, ub), method=a.method, tol=tol, x0=x0, ctx=ctx),
              "callable": lambda: least_squares_batch(fun, x0, jac, bounds=(lb, ub), method=a.method, ftol=tol,
                                                      xtol=np.finfo(float).eps, gtol=tol, driver="device", ctx=ctx)}
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}                         # warm-up: code objects, plans
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    ctx.timing(True)
    ctx.timing_reset()
    routes["device"]()
    ctx.sync()
    slots = {k: (round(ms, 3), int(cnt)) for k, (ms, cnt) in ctx.timing_read().items() if cnt}
    ctx.timing(False)
    Xd, Xc = (np.stack([r.x for r in out[k]]) for k in ("device", "callable"))
    res.update({"device_s": round(float(np.median(times["device"])), 4),
                "callable_s": round(float(np.median(times["callable"])), 4),
                "device_all_s": [round(t, 4) for t in times["device"]],
                "callable_all_s": [round(t, 4) for t in times["callable"]],
                "speedup": round(float(np.median(times["callable"]) / np.median(times["device"])), 2),
                "slots_ms": {k: v[0] for k, v in slots.items()}, "model_eval_launches": slots.get("model_eval", (0, 0))[1],
                "kernels_ms": round(sum(v[0] for v in slots.values()), 3),
                "status": {k: sorted(set(int(r.status) for r in out[k])) for k in routes},
                "max_nfev": int(max(r.nfev for r in out["device"])),
                "active_share": round(float(np.mean([np.mean(r.active_mask != 0) for r in out["device"]])), 3),
                "x_max_abs_diff": float(np.max(np.abs(Xd - Xc)))})
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
