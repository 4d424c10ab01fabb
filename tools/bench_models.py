"""Built-in fit models on the device (model_kernels.hip): what a named model saves a batch fit.

``curve_fit_batch`` on B one-peak problems ('gauss_sum', K = 1, n = 4), driver='device', the named model against the
same numpy model functions passed as callables, on the same GPU in the same process, alternating.  Whole calls are
timed (host clock around a call that ends in a download: upload, solve, covariance, results), median of `--repeat`
after one warm-up each.  The kernel's own time per call comes from the library's event timing (slot 'model_eval') in a
further call of the named route, so that the events do not sit inside the timed calls.

With ``--fixed`` / ``--tied`` the named route takes the keywords (the mapped kernel instances) and the
callable route is what a user has without them: the reduced model over the nf remaining variables as numpy callables
(the model's numpy functions behind ``ParamMap.wrap_f`` / ``wrap_jac``).  ``--kernel`` times the kernel alone instead:
`--launches` launches each of f and of J in the 'model_eval' slot, for the unmapped entry and (with a map) the mapped one,
and next to them for the composite 'gauss*K+poly*1' (the same model through the run-time component table
of blsq_model_eval_comp_dev), at the same size and on the same buffers' shapes.  `--rounds` repeats the timed block: the
figure is the median of the rounds' means, and `*_all` lists every round.

``--tied`` also takes ``j:i:ratio[:offset]`` (p_j = ratio * p_i + offset): the named route then runs the affine
kernel instances (blsq_model_eval_tie_dev), the callable route the same ``wrap_f`` / ``wrap_jac``.  With ``--kernel`` the
affine and the plain mapped instance are timed on the same map: for plain ties the keys `affine_*` are the affine
instance with every ratio 1 and offset 0, for affine ties the keys `plain_*` are the plain instance on the map without
its ratios and offsets.

``--estimator poisson`` fits counts instead: the same lines 40 times as high (60 counts at the peak over a
background of 12), drawn from the Poisson law, sigma None; the named route runs the Poisson kernel instances, the callable
route the numpy wrappers.  Without it nothing here changes.

``--binned`` fits histograms instead: `xdata` becomes the m + 1 edges of m contiguous bins over [-2, 2], the
amplitudes and the offset are divided by the bin width so that a bin holds what a point held, and the data are the bin
integrals; the named route runs the bin-integrated kernel instances (blsq_model_eval_bin_dev), the callable route the
numpy functions of ``models.binned``.  It combines with every other switch.  Without it nothing here changes.

``--omit FRACTION`` blanks that share of `ydata` at random (NaN; a fixed seed, every problem keeps more
points than parameters) and passes ``nan_policy='omit'`` on both routes: the named route runs the omitting kernel
instances (blsq_model_eval_nan_dev), the callable route ``models.omit_residual`` / ``omit_jacobian``.  ``--omit 0``
passes the keyword with no NaN: the cost of the flag alone.  Without it nothing here changes.

``--global S --shared i,j`` fits global problems instead: the B data sets become B // S groups of S, the
parameters i, j (of 'gauss_sum': 1,2 = position and width) are one per group, and ``curve_fit_global`` runs the whole
fit on the device route (blsq_model_eval_global_dev) against the callable route (the numpy functions behind
``GlobalMap.wrap_f`` / ``wrap_jac``).  A further call of the device route with every slot timed gives `slots_ms`, the
kernel time per slot, and `gram_share`, the part of it spent in the slots whose name holds 'gram': the measured case
for or against a structured solve.  With ``--kernel``: the launches of the global entry alone, f and J.

``--response L`` fits through an instrument response: the lines are convolved with a Gaussian kernel of L
taps (sigma L / 10 channels, centred at tap L / 3, sum 1, origin 0) before the noise is added.  Three routes are timed,
alternating: `named`, the spec on the device with ``response=`` (the model kernel, then blsq_response_apply_dev);
`plain`, the same route on unconvolved data without the keyword (what the second stage adds to a fit); `callable`, the
numpy functions with ``response=`` (``models.response_residual`` / ``response_jacobian`` on the host).  With ``--kernel``:
the response entry alone on random buffers of `--B` problems, `--m` rows and `--n` columns, f and J per launch in the
'model_eval' slot, and the bytes per second of J (G read, J written: 16 B m n bytes).

``--expr TEXT --params a,b,c`` fits an expression model instead: ``models.expression(TEXT, params)`` on
`--m` points of [0, 6], the truth `--truth v1,v2,...` jittered by 5 % per problem, noise of 0.01, p0 10 % off.  Routes,
alternating: `expr`, the ExprModel on the device (blsq_expr_eval_dev); `callable`, the same formula as numpy callables
``f(x, P)`` / ``jac(x, P)`` on the device driver, the only route there was before (the Jacobian crosses to the device on
every accepted step).  Without ``--truth`` TEXT must be the default, the two-component decay
``a*(f*exp(-t/t1)+(1-f)*exp(-t/t2))+bg``: its callables are written out by hand, and a third route `composite` fits
the equivalent 'exp*2+poly*1' (a f, 1 / t1, a (1 - f), 1 / t2, bg) for orientation.  For another TEXT the callables are
the model's numpy definition.  With ``--kernel``: the launches of blsq_expr_eval_dev alone, f and J apart (and, for the
default decay, those of the composite entry at the same shape).

``--separable`` fits with the linear parameters projected out: the default problems ('gauss_sum', or
``--peaks 2``), sigma 0.01, no bounds.  Routes, alternating: `separable`, ``curve_fit_batch(separable=True)`` on the
device with NaN in the linear entries of p0 (expand, the model kernel, blsq_varpro_reduce_dev per evaluation, then c and
the covariance of the full problem); `plain`, the same fit without the keyword from the same non-linear start, its linear
entries 10 % off the truth.  Reported: the median time of a call, the mean and the largest nfev of each route, and the
problems that converged.  With ``--kernel``: the time per evaluation in the 'model_eval' slot (HIP events) of the three
launches of the separable stage against the plain model kernel, f and J apart.  With ``--global S --shared i,j`` as
well: ``curve_fit_global(separable=True)`` against the plain global fit, whole fit and `model_eval`
slot — alone where the plain route cannot take the group (nv > 256, e.g. ``--global 300``) — and, with ``--kernel``,
the launches of the separable global stage against the global entry with the bytes of J each writes.  It takes --B, --m, --peaks, --repeat,
--kernel, --launches and --rounds only.

usage: python tools/bench_models.py [--B 4096] [--m 64] [--repeat 5] [--peaks 1] [--fixed 1,4] [--tied 5:2,4:1:1:0.42] [--kernel]
                                    [--launches 50] [--rounds 1] [--estimator lse] [--binned] [--omit FRACTION]
                                    [--global S --shared 1,2] [--response L [--n 4]]
                                    [--expr TEXT --params a,b,c [--truth 3,0.4,0.5,2.5,0.2] [--kernel]]
                                    [--separable [--kernel] [--global S --shared 1,2]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import curve_fit_batch, curve_fit_global, models, _abi, ParamMap, GlobalMap          # noqa: E402


PEAKS = {1: [1.5, 0.2, 0.6, 0.3], 2: [1.5, -0.8, 0.4, 1.0, 0.7, 0.5, 0.2]}


COUNTS = 40.0                                  # --estimator poisson: amplitudes and offset in counts


def problems(B, m, seed=0, peaks=1, fixed=(), tied=None, poisson=False, binned=False, common=None):
    """The truth satisfies the ties and p0 sits at the truth in the fixed columns.  common = (S, indices): the truth of
    those parameters is one value in every run of S problems (the groups of --global)."""
    rng = np.random.default_rng(seed)
    base = np.array(PEAKS[peaks])
    if poisson:
        base[0:-1:3] *= COUNTS
        base[-1] *= COUNTS
    if binned:
        base[0:-1:3] *= m / 4.0
        base[-1] *= m / 4.0
    truth = base * (1 + 0.05 * rng.uniform(-1, 1, (B, base.size)))
    for j, v in (tied or {}).items():
        i, r, d = (tuple(v) + (1.0, 0.0)[len(v) - 1:]) if isinstance(v, tuple) else (v, 1.0, 0.0)
        truth[:, j] = r * truth[:, i] + d
    if common:
        S, idx = common
        for j in idx:
            truth[:, j] = np.repeat(truth[::S, j], S)[:B]
    x = np.linspace(-2.0, 2.0, m + 1 if binned else m)
    M = models.binned("gauss_sum") if binned else models.get("gauss_sum")
    if poisson:
        Y = rng.poisson(M.f(x, truth)).astype(float)
    else:
        Y = M.f(x, truth) + 0.01 * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    P0[:, list(fixed)] = truth[:, list(fixed)]
    half = 0.4 * np.abs(truth) + 0.2
    return x, Y, P0, (truth - half, truth + half)


def blank(Y, fraction, n, seed=1):
    """Y with `fraction` of its entries NaN, drawn with a fixed seed; no problem is left with fewer than n + 1 points."""
    rng = np.random.default_rng(seed)
    om = rng.random(Y.shape) < fraction
    short = (~om).sum(axis=1) <= n
    om[short] = False
    return np.where(om, np.nan, Y)


def kernel_times(ctx, x, Y, P0, pm, launches, rounds=1, estimator="lse", binned=False, omit=False):
    """us per launch of f and of J ('model_eval' slot, HIP events) for the unmapped entry at P0 and, with a map, the
    mapped entry at reduce_x(P0); 'composite*': the same for 'gauss*K+poly*1' through the composite entry."""
    B, m = Y.shape
    n = P0.shape[1]
    spec = "gauss*%d+poly*1" % ((n - 1) // 3)
    out = {}
    cases = [("unmapped", "gauss_sum", None), ("composite", spec, None)]
    if pm is not None:
        cases += [("mapped", "gauss_sum", pm), ("composite_mapped", spec, pm)]
        if pm.affine:                           # the plain instance on the same map, without its ratios and offsets
            other = ParamMap(pm.n, pm.fixed, pm.tied)
            cases += [("plain", "gauss_sum", other), ("composite_plain", spec, other)]
        else:                                   # the affine instance on the same map: every ratio 1, every offset 0
            other = ParamMap(pm.n, pm.fixed, pm.tied)
            other.affine = True
            cases += [("affine", "gauss_sum", other), ("composite_affine", spec, other)]
    for key, name, mp in cases:
        dm = models.DeviceModel(ctx, name, B, m, n, x, Y, 0.01 if estimator == "lse" else None, param_map=mp,
                                Pfix=None if mp is None else P0, estimator=estimator, **({"binned": True} if binned else {}),
                                **({"nan_policy": "omit"} if omit else {}))
        X = P0 if mp is None else np.ascontiguousarray(mp.reduce_x(P0))
        d_x, d_f, d_J = ctx.to_device(X), ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * dm.n)
        for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
            call()                                                        # warm-up: the code object
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
            out["%s_%s_us" % (key, what)] = round(float(np.median(per_round)), 2)
            if rounds > 1:
                out["%s_%s_us_all" % (key, what)] = per_round
        for p in (d_x, d_f, d_J):
            ctx.free(p)
        dm.close()
    return out


def global_bench(a, ctx):
    """--global: G = B // S groups of S one-peak data sets with the parameters `a.shared` common to a group."""
    S, m = a.global_S, a.m
    G = max(1, a.B // S)
    shared = [int(v) for v in a.shared.split(",") if v]
    poisson = a.estimator == "poisson"
    x, Y, P0, (lb, ub) = problems(G * S, m, peaks=a.peaks, poisson=poisson, common=(S, shared))
    n = P0.shape[1]
    Y, P0, lb, ub = Y.reshape(G, S, m), P0.reshape(G, S, n), lb.reshape(G, S, n), ub.reshape(G, S, n)
    gm = GlobalMap(n, S, shared)
    res = {"model": "gauss_sum", "G": G, "S": S, "m": m, "n": n, "shared": shared, "M": S * m, "nv": gm.nv,
           "estimator": a.estimator}
    if a.kernel:
        dm = models.DeviceModel(ctx, "gauss_sum", G, m, n, x, Y, None if poisson else 0.01, Pfix=P0,
                                estimator=a.estimator, global_map=gm)
        d_x = ctx.to_device(np.ascontiguousarray(gm.reduce_x(P0)))
        d_f, d_J = ctx.malloc(8 * G * S * m), ctx.malloc(8 * G * S * m * gm.nv)
        for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
            call()
            ctx.sync()
            per_round = []
            for _ in range(a.rounds):
                ctx.timing(True, only="model_eval")
                ctx.timing_reset()
                for _ in range(a.launches):
                    call()
                ctx.sync()
                ms, cnt = ctx.timing_read()["model_eval"]
                ctx.timing(False)
                per_round.append(round(1e3 * ms / cnt, 2))
            res["global_%s_us" % what] = round(float(np.median(per_round)), 2)
            res["global_%s_us_all" % what] = per_round
        res["J_bytes"] = 8 * G * S * m * gm.nv
        for p in (d_x, d_f, d_J):
            ctx.free(p)
        dm.close()
        return res
    kw = dict(sigma=None if poisson else 0.01, bounds=(lb, ub), driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10,
              gtol=1e-10, estimator=a.estimator)
    M = models.get("gauss_sum")
    routes = {"named": lambda: curve_fit_global("gauss_sum", x, Y, P0, shared, **kw),
              "callable": lambda: curve_fit_global(M.f, x, Y, P0, shared, jac=M.jac, **kw)}
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
    routes["named"]()
    ctx.sync()
    slots = {k: round(ms, 3) for k, (ms, cnt) in ctx.timing_read().items() if cnt}
    ctx.timing(False)
    total = sum(slots.values())
    both = np.array([ra.success and rb.success for ra, rb in zip(out["named"][2], out["callable"][2])])
    res.update({"named_s": round(float(np.median(times["named"])), 4),
                "callable_s": round(float(np.median(times["callable"])), 4),
                "named_all_s": [round(t, 4) for t in times["named"]],
                "callable_all_s": [round(t, 4) for t in times["callable"]],
                "speedup": round(float(np.median(times["callable"]) / np.median(times["named"])), 2),
                "slots_ms": slots, "kernels_ms": round(total, 3),
                "gram_share": round(sum(v for k, v in slots.items() if "gram" in k) / total, 3) if total else None,
                "converged": {k: int(sum(r.success for r in out[k][2])) for k in routes},
                "max_nfev": int(max(r.nfev for r in out["named"][2])),
                "popt_max_rel_diff": float(np.max(np.abs(out["named"][0][both] - out["callable"][0][both])
                                                  / (np.abs(out["callable"][0][both]) + 1e-3)))})
    return res


def response_kernel(L):
    h = np.exp(-0.5 * ((np.arange(L) - L / 3.0) / max(L / 10.0, 0.5)) ** 2)
    return h / h.sum()


def response_bench(a, ctx):
    """--response L: whole fits through the response against the plain fit and the callable route; with --kernel the
    launches of blsq_response_apply_dev alone."""
    B, m, L = a.B, a.m, a.response
    h = response_kernel(L)
    res = {"B": B, "m": m, "L": L, "origin": 0}
    if a.kernel:
        nc = a.n
        rng = np.random.default_rng(0)
        d_g, d_G = ctx.to_device(rng.standard_normal((B, m))), ctx.to_device(rng.standard_normal((B, m, nc)))
        d_y, d_w, d_h = ctx.to_device(rng.standard_normal((B, m))), ctx.to_device(rng.uniform(0.5, 2, m)), ctx.to_device(h)
        d_f, d_J = ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * nc)

        def call(f, J):
            ctx.check(ctx.lib.blsq_response_apply_dev(ctx.h, 0, 0, B, 1, m, nc, L, 0, d_h, 0, d_g, d_G, d_y, d_w, 0, f, J,
                                                      None), "blsq_response_apply_dev")
        res.update({"n": nc, "launches": a.launches, "rounds": a.rounds, "J_bytes": 16 * B * m * nc})
        for what, run in (("f", lambda: call(d_f, None)), ("J", lambda: call(None, d_J))):
            run()
            ctx.sync()
            per_round = []
            for _ in range(a.rounds):
                ctx.timing(True, only="model_eval")
                ctx.timing_reset()
                for _ in range(a.launches):
                    run()
                ctx.sync()
                ms, cnt = ctx.timing_read()["model_eval"]
                ctx.timing(False)
                per_round.append(round(1e3 * ms / cnt, 2))
            res["response_%s_us" % what] = round(float(np.median(per_round)), 2)
            res["response_%s_us_all" % what] = per_round
        res["J_TB_per_s"] = round(res["J_bytes"] / (res["response_J_us"] * 1e-6) / 1e12, 3)
        res["J_gflops"] = round(2.0 * B * m * nc * L / (res["response_J_us"] * 1e-6) / 1e9, 1)
        for p in (d_g, d_G, d_y, d_w, d_h, d_f, d_J):
            ctx.free(p)
        return res
    x, Y_plain, P0, bounds = problems(B, m, peaks=a.peaks)
    rng = np.random.default_rng(1)
    M = models.get("gauss_sum")
    truth = (bounds[0] + bounds[1]) / 2                                    # (the box of `problems` is centred on it)
    Y = models.apply_response(M.f(x, truth), h, 0) + 0.01 * rng.standard_normal((B, m))
    kw = dict(sigma=0.01, bounds=bounds, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    routes = {"named": lambda: curve_fit_batch("gauss_sum", x, Y, P0, response=h, **kw),
              "plain": lambda: curve_fit_batch("gauss_sum", x, Y_plain, P0, **kw),
              "callable": lambda: curve_fit_batch(M.f, x, Y, P0, jac=M.jac, response=h, **kw)}
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}                         # warm-up: code objects, plans
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
    both = np.array([ra.success and rb.success for ra, rb in zip(out["named"][2], out["callable"][2])])
    med = {k: float(np.median(v)) for k, v in times.items()}
    res.update({"model": "gauss_sum", "n": P0.shape[1],
                **{k + "_s": round(v, 4) for k, v in med.items()},
                **{k + "_all_s": [round(t, 4) for t in v] for k, v in times.items()},
                "named_over_plain": round(med["named"] / med["plain"], 3),
                "speedup_over_callable": round(med["callable"] / med["named"], 2),
                "model_eval_ms_per_fit": round(k_ms, 3), "model_eval_units_per_fit": int(k_n),
                "converged": {k: int(sum(r.success for r in out[k][2])) for k in routes},
                "nfev": {k: int(max(r.nfev for r in out[k][2])) for k in routes},
                "popt_max_rel_diff": float(np.max(np.abs(out["named"][0][both] - out["callable"][0][both])
                                                  / (np.abs(out["callable"][0][both]) + 1e-3)))})
    return res


DECAY_TEXT = "a*(f*exp(-t/t1)+(1-f)*exp(-t/t2))+bg"
DECAY_PARAMS = "a,f,t1,t2,bg"
DECAY_TRUTH = [3.0, 0.4, 0.5, 2.5, 0.2]


def decay_f(x, P):
    a, f, t1, t2, bg = (P[:, k, np.newaxis] for k in range(5))
    return a * (f * np.exp(-x / t1) + (1 - f) * np.exp(-x / t2)) + bg


def decay_jac(x, P):
    a, f, t1, t2, bg = (P[:, k, np.newaxis] for k in range(5))
    e1, e2 = np.exp(-x / t1), np.exp(-x / t2)
    J = np.empty((P.shape[0], x.shape[-1], 5))
    J[:, :, 0] = f * e1 + (1 - f) * e2
    J[:, :, 1] = a * (e1 - e2)
    J[:, :, 2] = a * f * e1 * x / (t1 * t1)
    J[:, :, 3] = a * (1 - f) * e2 * x / (t2 * t2)
    J[:, :, 4] = 1.0
    return J


def expr_bench(a, ctx):
    """--expr: whole fits of the ExprModel on the device against the formula as numpy callables (and, for the default
    decay, against the equivalent composite)."""
    text = a.expr.replace(" ", "")
    decay = text == DECAY_TEXT and a.params == DECAY_PARAMS and not a.truth
    if not a.truth and not decay:
        raise SystemExit("--expr with a formula of your own needs --truth v1,v2,...")
    M = models.expression(a.expr, tuple(a.params.split(",")))
    base = np.array(DECAY_TRUTH if decay else [float(v) for v in a.truth.split(",")])
    if base.size != M.n:
        raise SystemExit("--truth has %d values, the model %d parameters" % (base.size, M.n))
    B, m = a.B, a.m
    rng = np.random.default_rng(0)
    truth = base * (1 + 0.05 * rng.uniform(-1, 1, (B, base.size)))
    x = np.linspace(0.0, 6.0, m)
    Y = M.f(x, truth) + 0.01 * rng.standard_normal((B, m))
    P0 = truth * (1 + 0.1 * rng.choice([-1.0, 1.0], truth.shape))
    half = 0.4 * np.abs(truth) + 0.2
    if decay:
        def comp(P):
            return np.column_stack([P[:, 0] * P[:, 1], 1 / P[:, 2], P[:, 0] * (1 - P[:, 1]), 1 / P[:, 3], P[:, 4]])
    p = M.program
    head = {"expr": M.name, "nops": p.nops, "nconst": len(p.consts), "nact": int(p.active().sum()), "B": B, "m": m,
            "n": M.n}
    if a.kernel:                                   # the launches alone, f and J apart, in the 'model_eval' slot
        head.update({"launches": a.launches, "rounds": a.rounds, "J_bytes": 8 * B * m * M.n})
        for key, name, X in [("expr", M, P0)] + ([("composite", "exp*2+poly*1", comp(P0))] if decay else []):
            dm = models.DeviceModel(ctx, name, B, m, M.n, x, Y, 0.01)
            d_x, d_f, d_J = ctx.to_device(np.ascontiguousarray(X)), ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * M.n)
            for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
                call()                                                    # warm-up: the code object
                ctx.sync()
                per_round = []
                for _ in range(a.rounds):
                    ctx.timing(True, only="model_eval")
                    ctx.timing_reset()
                    for _ in range(a.launches):
                        call()
                    ctx.sync()
                    ms, cnt = ctx.timing_read()["model_eval"]
                    ctx.timing(False)
                    per_round.append(round(1e3 * ms / cnt, 2))
                head["%s_%s_us" % (key, what)] = round(float(np.median(per_round)), 2)
                head["%s_%s_us_all" % (key, what)] = per_round
            for q in (d_x, d_f, d_J):
                ctx.free(q)
            dm.close()
        return head
    kw = dict(sigma=0.01, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    f, jac = (decay_f, decay_jac) if decay else (M.f, M.jac)
    routes = {"expr": lambda: curve_fit_batch(M, x, Y, P0, bounds=(truth - half, truth + half), **kw),
              "callable": lambda: curve_fit_batch(f, x, Y, P0, jac=jac, bounds=(truth - half, truth + half), **kw)}
    if decay:
        C, C0 = comp(truth), comp(P0)
        chalf = 0.6 * np.abs(C) + 0.2
        routes["composite"] = lambda: curve_fit_batch("exp*2+poly*1", x, Y, C0, bounds=(C - chalf, C + chalf), **kw)
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}                         # warm-up: code objects, plans
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    ctx.timing(True, only="model_eval")
    ctx.timing_reset()
    routes["expr"]()
    ctx.sync()
    k_ms, k_n = ctx.timing_read()["model_eval"]
    ctx.timing(False)
    both = np.array([ra.success and rb.success for ra, rb in zip(out["expr"][2], out["callable"][2])])
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {**head, "driver": "device",
            **{k + "_s": round(v, 4) for k, v in med.items()},
            **{k + "_all_s": [round(t, 4) for t in v] for k, v in times.items()},
            "speedup_over_callable": round(med["callable"] / med["expr"], 2),
            "kernel_ms_per_fit": round(k_ms, 3), "kernel_launches_per_fit": int(k_n),
            "kernel_us_per_launch": round(1e3 * k_ms / max(k_n, 1), 2),
            "converged": {k: int(sum(r.success for r in out[k][2])) for k in routes},
            "nfev": {k: int(max(r.nfev for r in out[k][2])) for k in routes},
            "popt_max_rel_diff": float(np.max(np.abs(out["expr"][0][both] - out["callable"][0][both])
                                              / (np.abs(out["callable"][0][both]) + 1e-3)))}


def separable_bench(a, ctx):
    """--separable: the separable fit against the plain one, or (--kernel) the three launches against the model kernel."""
    x, Y, P0, _ = problems(a.B, a.m, peaks=a.peaks)
    B, m = Y.shape
    n = P0.shape[1]
    lin, owner = models.linear_params("gauss_sum", n)
    non = np.flatnonzero(owner >= 0)
    res = {"model": "gauss_sum", "separable": True, "B": B, "m": m, "n": n, "nl": int(lin.size), "na": int(non.size)}
    if a.kernel:
        res.update(launches=a.launches, rounds=a.rounds)
        for key, sep in (("plain", False), ("separable", True)):
            dm = models.DeviceModel(ctx, "gauss_sum", B, m, n, x, Y, 0.01, **({"separable": True} if sep else {}))
            X = np.ascontiguousarray(P0[:, non]) if sep else P0
            d_x, d_f, d_J = ctx.to_device(X), ctx.malloc(8 * B * m), ctx.malloc(8 * B * m * dm.n)
            for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
                call()                                                    # warm-up: the code objects
                ctx.sync()
                per_round = []
                for _ in range(a.rounds):
                    ctx.timing(True, only="model_eval")
                    ctx.timing_reset()
                    for _ in range(a.launches):
                        call()
                    ctx.sync()
                    ms, cnt = ctx.timing_read()["model_eval"]
                    ctx.timing(False)
                    per_round.append(round(1e3 * ms / a.launches, 2))      # per evaluation: one launch, or three
                    res["%s_%s_launches_per_eval" % (key, what)] = cnt // a.launches
                res["%s_%s_us" % (key, what)] = round(float(np.median(per_round)), 2)
                if a.rounds > 1:
                    res["%s_%s_us_all" % (key, what)] = per_round
            for p in (d_x, d_f, d_J):
                ctx.free(p)
            dm.close()
        return res
    kw = dict(sigma=0.01, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    P0_sep = P0.copy()
    P0_sep[:, lin] = np.nan
    routes = {"separable": lambda: curve_fit_batch("gauss_sum", x, Y, P0_sep, separable=True, **kw),
              "plain": lambda: curve_fit_batch("gauss_sum", x, Y, P0, **kw)}
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}                         # warm-up: code objects, plans
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    both = np.array([ra.success and rb.success for ra, rb in zip(out["separable"][2], out["plain"][2])])
    for k in routes:
        nfev = np.array([r.nfev for r in out[k][2]])
        res.update({k + "_s": round(float(np.median(times[k])), 4), k + "_all_s": [round(t, 4) for t in times[k]],
                    k + "_nfev_mean": round(float(nfev.mean()), 2), k + "_nfev_max": int(nfev.max()),
                    k + "_converged": int(sum(r.success for r in out[k][2]))})
    res["speedup"] = round(res["plain_s"] / res["separable_s"], 2)
    res["popt_max_rel_diff"] = float(np.max(np.abs(out["separable"][0][both] - out["plain"][0][both])
                                            / (np.abs(out["plain"][0][both]) + 1e-3)))
    return res


def separable_global_bench(a, ctx):
    """--global S --shared i,j --separable: ``curve_fit_global(separable=True)`` against the plain global
    fit — alone where the plain route cannot take the group (nv = ns + S nl > 256) — or (--kernel) the launches of the
    separable global stage against the global entry, f and J apart, with the bytes of J each writes."""
    S, m = a.global_S, a.m
    G = max(1, a.B // S)
    shared = [int(v) for v in a.shared.split(",") if v]
    x, Y, P0, _ = problems(G * S, m, peaks=a.peaks, common=(S, shared))
    n = P0.shape[1]
    Y, P0 = Y.reshape(G, S, m), P0.reshape(G, S, n)
    gm_full = GlobalMap(n, S, shared)
    gm, lin, owner, non = models.separable_global_map("gauss_sum", n, S, shared)
    plain_fits = gm_full.nv <= 256
    res = {"model": "gauss_sum", "separable": True, "G": G, "S": S, "m": m, "n": n, "shared": shared, "M": S * m,
           "nv": gm.nv, "nv_plain": gm_full.nv, "J_bytes": 8 * G * S * m * gm.nv,
           "J_bytes_plain": 8 * G * S * m * gm_full.nv}
    if a.kernel:
        res.update(launches=a.launches, rounds=a.rounds)
        for key, sep in (("plain", False), ("separable", True)):
            if not sep and not plain_fits:
                continue
            mp = gm if sep else gm_full
            dm = models.DeviceModel(ctx, "gauss_sum", G, m, n, x, Y, 0.01, global_map=mp,
                                    **({"separable": True} if sep else {"Pfix": P0}))
            X = np.ascontiguousarray(mp.reduce_x(P0[..., non] if sep else P0))
            d_x, d_f, d_J = ctx.to_device(X), ctx.malloc(8 * G * S * m), ctx.malloc(8 * G * S * m * mp.nv)
            for what, call in (("f", lambda: dm.fun_dev(d_x, d_f, 1)), ("J", lambda: dm.jac_dev(d_x, d_J))):
                call()
                ctx.sync()
                per_round = []
                for _ in range(a.rounds):
                    ctx.timing(True, only="model_eval")
                    ctx.timing_reset()
                    for _ in range(a.launches):
                        call()
                    ctx.sync()
                    ms, cnt = ctx.timing_read()["model_eval"]
                    ctx.timing(False)
                    per_round.append(round(1e3 * ms / a.launches, 2))
                    res["%s_%s_launches_per_eval" % (key, what)] = cnt // a.launches
                res["%s_%s_us" % (key, what)] = round(float(np.median(per_round)), 2)
                if a.rounds > 1:
                    res["%s_%s_us_all" % (key, what)] = per_round
            for p in (d_x, d_f, d_J):
                ctx.free(p)
            dm.close()
        return res
    kw = dict(sigma=0.01, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    P0_sep = P0.copy()
    P0_sep[..., lin] = np.nan
    routes = {"separable": lambda: curve_fit_global("gauss_sum", x, Y, P0_sep, shared, separable=True, **kw)}
    if plain_fits:
        routes["plain"] = lambda: curve_fit_global("gauss_sum", x, Y, P0, shared, **kw)
    times = {k: [] for k in routes}
    out = {k: run() for k, run in routes.items()}                         # warm-up: code objects, plans
    for _ in range(a.repeat):
        for k, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    for k, run in routes.items():
        ctx.timing(True)
        ctx.timing_reset()
        run()
        ctx.sync()
        slots = {s: round(ms, 3) for s, (ms, cnt) in ctx.timing_read().items() if cnt}
        ctx.timing(False)
        nfev = np.array([r.nfev for r in out[k][2]])
        res.update({k + "_s": round(float(np.median(times[k])), 4), k + "_all_s": [round(t, 4) for t in times[k]],
                    k + "_nfev_mean": round(float(nfev.mean()), 2), k + "_nfev_max": int(nfev.max()),
                    k + "_converged": int(sum(r.success for r in out[k][2])), k + "_slots_ms": slots,
                    k + "_model_eval_ms": slots.get("model_eval")})
    if plain_fits:
        both = np.array([ra.success and rb.success for ra, rb in zip(out["separable"][2], out["plain"][2])])
        res["speedup"] = round(res["plain_s"] / res["separable_s"], 2)
        res["popt_max_rel_diff"] = float(np.max(np.abs(out["separable"][0][both] - out["plain"][0][both])
                                                / (np.abs(out["plain"][0][both]) + 1e-3)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--peaks", type=int, default=1, choices=sorted(PEAKS))
    ap.add_argument("--fixed", default="", help="indices held at p0, e.g. 1,4")
    ap.add_argument("--tied", default="", help="j:i pairs (p_j is p_i), e.g. 5:2, or j:i:ratio[:offset] (p_j = ratio * p_i + offset)")
    ap.add_argument("--kernel", action="store_true", help="time the kernel's launches alone")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=1, help="with --kernel: timed blocks of --launches launches each")
    ap.add_argument("--estimator", default="lse", choices=models.ESTIMATORS)
    ap.add_argument("--binned", action="store_true", help="fit bin integrals: the bin-integrated instances")
    ap.add_argument("--omit", type=float, default=None, metavar="FRACTION",
                    help="blank this share of ydata and pass nan_policy='omit' (0: the keyword with no NaN)")
    ap.add_argument("--global", dest="global_S", type=int, default=0, metavar="S",
                    help="global fits: B // S groups of S data sets (needs --shared)")
    ap.add_argument("--shared", default="", help="with --global: the parameters common to a group, e.g. 1,2")
    ap.add_argument("--response", type=int, default=0, metavar="L",
                    help="fit through an instrument response of L taps (with --kernel: the response entry alone)")
    ap.add_argument("--n", type=int, default=4, help="with --response --kernel: the columns of G and J")
    ap.add_argument("--expr", nargs="?", const=DECAY_TEXT, default=None, metavar="TEXT",
                    help="fit an expression model (default TEXT: the two-component decay)")
    ap.add_argument("--params", default=DECAY_PARAMS, help="with --expr: the parameter names, e.g. a,b,c")
    ap.add_argument("--truth", default="", help="with --expr: the parameter values the data are drawn from")
    ap.add_argument("--separable", action="store_true",
                    help="fit with the linear parameters projected out (with --kernel: the three launches per evaluation)")
    a = ap.parse_args()
    if a.separable:
        if (a.expr is not None or a.response or a.fixed or a.tied or a.binned or a.omit is not None
                or a.estimator != "lse" or (a.global_S and (a.global_S < 1 or not a.shared))):
            ap.error("--separable takes --B, --m, --peaks, --repeat, --kernel (--launches, --rounds) and "
                     "--global S --shared i,j only")
        ctx = _abi.Context(0)
        res = separable_global_bench(a, ctx) if a.global_S else separable_bench(a, ctx)
        ctx.close()
        print(json.dumps(res))
        return
    if a.expr is not None:
        if a.response or a.global_S or a.fixed or a.tied or a.binned or a.omit is not None or a.estimator != "lse":
            ap.error("--expr TEXT takes --params, --truth, --B, --m, --repeat and --kernel (--launches, --rounds) only")
        ctx = _abi.Context(0)
        res = expr_bench(a, ctx)
        ctx.close()
        print(json.dumps(res))
        return
    if a.response:
        if (not 1 <= a.response <= models.RESPONSE_MAX_L or a.global_S or a.fixed or a.tied or a.binned
                or a.omit is not None or a.estimator != "lse"):
            ap.error("--response L takes 1 <= L <= %d, without the other switches" % models.RESPONSE_MAX_L)
        ctx = _abi.Context(0)
        res = response_bench(a, ctx)
        ctx.close()
        print(json.dumps(res))
        return
    if a.global_S:
        if a.global_S < 1 or not a.shared or a.fixed or a.tied or a.binned or a.omit is not None:
            ap.error("--global S takes S >= 1 and --shared i,j, without --fixed, --tied, --binned and --omit")
        ctx = _abi.Context(0)
        res = global_bench(a, ctx)
        ctx.close()
        print(json.dumps(res))
        return
    if a.omit is not None and not 0.0 <= a.omit < 1.0:
        ap.error("--omit takes a fraction in [0, 1)")
    fixed = [int(v) for v in a.fixed.split(",") if v]
    tied = {}
    for p in a.tied.split(","):
        v = p.split(":")
        if p and not 2 <= len(v) <= 4:
            ap.error("--tied takes j:i, j:i:ratio or j:i:ratio:offset")
        if p:
            tied[int(v[0])] = int(v[1]) if len(v) == 2 else (int(v[1]),) + tuple(float(q) for q in v[2:])
    poisson = a.estimator == "poisson"
    x, Y, P0, bounds = problems(a.B, a.m, peaks=a.peaks, fixed=fixed, tied=tied, poisson=poisson, binned=a.binned)
    n = P0.shape[1]
    omit = a.omit is not None
    if omit:
        Y = blank(Y, a.omit, n)
    M = models.binned("gauss_sum") if a.binned else models.get("gauss_sum")
    pm = ParamMap(n, fixed, tied) if (fixed or tied) else None
    ctx = _abi.Context(0)
    if a.kernel:
        res = {"model": "gauss_sum", "B": a.B, "m": a.m, "n": n, "nf": n if pm is None else pm.nf, "fixed": fixed,
               "tied": a.tied, "launches": a.launches, "rounds": a.rounds, "estimator": a.estimator,
               "binned": a.binned, "omit": a.omit}
        res.update(kernel_times(ctx, x, Y, P0, pm, a.launches, a.rounds, a.estimator, a.binned, omit))
        ctx.close()
        print(json.dumps(res))
        return
    kw = dict(sigma=0.01, bounds=bounds, driver="device", ctx=ctx, ftol=1e-10, xtol=1e-10, gtol=1e-10)
    if poisson:
        kw.update(sigma=None, estimator="poisson")
    if omit:
        kw.update(nan_policy="omit")
    named_kw = dict(kw, binned=True) if a.binned else kw
    if pm is None:
        routes = {"named": lambda: curve_fit_batch("gauss_sum", x, Y, P0, **named_kw),
                  "callable": lambda: curve_fit_batch(M.f, x, Y, P0, jac=M.jac, **kw)}
    else:
        kw_red = dict(kw, bounds=pm.reduce_bounds(*bounds))
        f_red, jac_red, X0 = pm.wrap_f(M.f, P0), pm.wrap_jac(M.jac, P0), pm.reduce_x(P0)
        routes = {"named": lambda: curve_fit_batch("gauss_sum", x, Y, P0, fixed=fixed, tied=tied, **named_kw),
                  "callable": lambda: curve_fit_batch(f_red, x, Y, X0, jac=jac_red, **kw_red)}
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
    free = (lambda P: P) if pm is None else pm.reduce_x
    res = {"model": "gauss_sum", "B": a.B, "m": a.m, "n": n, "nf": n if pm is None else pm.nf, "driver": "device",
           "estimator": a.estimator, "binned": a.binned, "omit": a.omit, "named_s": round(float(np.median(times["named"])), 4),
           "callable_s": round(float(np.median(times["callable"])), 4),
           "named_all_s": [round(t, 4) for t in times["named"]],
           "callable_all_s": [round(t, 4) for t in times["callable"]],
           "speedup": round(float(np.median(times["callable"]) / np.median(times["named"])), 2),
           "kernel_ms_per_fit": round(k_ms, 3), "kernel_launches_per_fit": int(k_n),
           "kernel_us_per_launch": round(1e3 * k_ms / max(k_n, 1), 2),
           "converged": ok, "max_nfev": int(max(r.nfev for r in out["named"][2])),
           "popt_max_rel_diff": float(np.max(np.abs(free(out["named"][0])[both] - out["callable"][0][both])
                                             / (np.abs(out["callable"][0][both]) + 1e-3)))}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
