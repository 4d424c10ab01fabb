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

usage: python tools/bench_linear.py [--B 4096] [--m 64] [--n 16] [--method trf] [--own] [--repeat 5]
                                    [--kernel] [--launches 200] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import lsq_linear_batch, least_squares_batch, LinearDeviceModel, _abi, _linear      # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--method", default="trf", choices=_linear.METHODS)
    ap.add_argument("--own", action="store_true", help="one matrix per problem instead of one for all")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--kernel", action="store_true", help="time the kernel's launches alone")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5, help="with --kernel: timed blocks of --launches launches each")
    a = ap.parse_args()
    A, b = problems(a.B, a.m, a.n, a.own)
    ctx = _abi.Context(0)
    res = {"B": a.B, "m": a.m, "n": a.n, "shared": not a.own, "method": a.method}
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
