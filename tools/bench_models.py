"""Built-in fit models on the device (model_kernels.hip): what a named model saves a batch fit.

``curve_fit_batch`` on B one-peak problems ('gauss_sum', K = 1, n = 4), driver='device', the named model against the
same numpy model functions passed as callables, on the same GPU in the same process, alternating.  Whole calls are
timed (host clock around a call that ends in a download: upload, solve, covariance, results), median of `--repeat`
after one warm-up each.  The kernel's own time per call comes from the library's event timing (slot 'model_eval') in a
further call of the named route, so that the events do not sit inside the timed calls.

usage: python tools/bench_models.py [--B 4096] [--m 64] [--repeat 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import curve_fit_batch, models, _abi                    # noqa: E402


def problems(B, m, seed=0):
    rng = np.random.default_rng(seed)
    truth = np.array([1.5, 0.2, 0.6, 0.3]) * (1 + 0.05 * rng.uniform(-1, 1, (B, 4)))
    x = np.linspace(-2.0, 2.0, m)
    Y = models.get("gauss_sum").f(x, truth) + 0.01 * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    return x, Y, P0, (truth - half, truth + half)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    x, Y, P0, bounds = problems(a.B, a.m)
    M = models.get("gauss_sum")
    ctx = _abi.Context(0)
    kw = dict(sigma=0.01, bounds=bounds, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    routes = {"named": lambda: curve_fit_batch("gauss_sum", x, Y, P0, **kw),
              "callable": lambda: curve_fit_batch(M.f, x, Y, P0, jac=M.jac, **kw)}
    times = {k: [] for k in routes}
    out = {}
    for k, run in routes.items():                                         # warm-up: code objects, plans
        out[k] = run()
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    ctx.timing(True, only="model_eval")
    ctx.timing_reset()
    routes["named"]()
    ctx.sync()
    k_ms, k_n = ctx.timing_read()["model_eval"]
    ctx.timing(False)
    ok = {k: int(sum(r.success for r in out[k][2])) for k in routes}
    both = np.array([ra.success and rb.success for ra, rb in zip(out["named"][2], out["callable"][2])])
    res = {"model": "gauss_sum", "B": a.B, "m": a.m, "n": 4, "driver": "device",
           "named_s": round(float(np.median(times["named"])), 4),
           "callable_s": round(float(np.median(times["callable"])), 4),
           "named_all_s": [round(t, 4) for t in times["named"]],
           "callable_all_s": [round(t, 4) for t in times["callable"]],
           "speedup": round(float(np.median(times["callable"]) / np.median(times["named"])), 2),
           "kernel_ms_per_fit": round(k_ms, 3), "kernel_launches_per_fit": int(k_n),
           "kernel_us_per_launch": round(1e3 * k_ms / max(k_n, 1), 2),
           "converged": ok, "max_nfev": int(max(r.nfev for r in out["named"][2])),
           "popt_max_rel_diff": float(np.max(np.abs(out["named"][0][both] - out["callable"][0][both])
                                             / (np.abs(out["callable"][0][both]) + 1e-3)))}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
