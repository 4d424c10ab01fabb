"""Parameter covariance on the device (cov_kernels.hip, blsq_cov_dev): what it costs.

For 1024 x 512 x 64, 512 x 4096 x 256 and 1 x 250000 x 128, in one run and with HIP-event timing (the per-kernel
slots of the ctx): blsq_cov_dev as a whole, its Householder tree (qr_leaf + qr_merge), its inverse + product kernels
(cov_inverse + cov_product), the gather of 'free' mode, and blsq_trf_factor_dev on the same J (the step path's
factorisation: normal-equations front end, all slots summed).  Wall times per call (stream synchronised) beside them.
The pseudo-inverse route (blsq_cov_pinv_dev) on the same J beside it: the same tree, the Jacobi SVD of
the triangle (jacobi_svd), the weights and the product kernel (cov_pinv_weights + cov_pinv_product).
The "rows" leg (blsq_cov_rows_dev): the leverages of the same J through the factor either route has left —
the `cov_rows` slot and the wall time per call for both routes, and for the pinv route the slot of the first call after
a covariance call as well (it refines the factor first) — beside the `gram` slot of blsq_trf_factor_dev on the same J:
one pass over J and about m n^2 flops, like the row forms.

usage: python tools/bench_cov.py [--out profiles/cov/bench_cov.json] [--rows-out profiles/cov/bench_rows.json]
                                 [--rows-only]      (the covariance legs run once, untimed, to leave their factors)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import TrfStepSolver, _abi                                # noqa: E402
from bounded_lsq._abi import vp                                            # noqa: E402

SHAPES = ((1024, 512, 64), (512, 4096, 256), (1, 250000, 128))


def _timed(ctx, call, reps):
    for _ in range(2):
        call()
    ctx.sync()
    ctx.timing(True)
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ctx.sync()
    wall = (time.perf_counter() - t0) / reps * 1e3
    T = {k: v[0] / reps for k, v in ctx.timing_read().items() if v[1]}
    ctx.timing(False)
    return wall, T


def bench_shape(ctx, B, m, n, reps, rows_only=False):
    rng = np.random.default_rng(0)
    blk = min(B, 16)
    Jh = np.tile(rng.standard_normal((blk, m, n)), ((B + blk - 1) // blk, 1, 1))[:B]
    d_J = ctx.to_device(Jh)
    del Jh
    mask = (rng.uniform(size=(B, n)) < 0.1).astype(np.int64)
    d_mask = ctx.to_device(mask)
    d_cov, d_rc, d_st = ctx.malloc(8 * B * n * n), ctx.malloc(8 * B), ctx.malloc(4 * B)
    d_rk, d_kr = ctx.malloc(4 * B), ctx.malloc(8 * B)
    out = {"shape": [B, m, n]}
    rows = {"shape": [B, m, n]}
    d_lev = ctx.malloc(8 * B * m)
    cov_reps = 1 if rows_only else reps

    def rows_call():
        ctx.check(ctx.lib.blsq_cov_rows_dev(h, m, d_J, None, d_lev), "cov_rows")

    h = vp()
    ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "blsq_cov_plan_create")
    try:
        for label, dm in (("all", None), ("free", d_mask)):
            wall, T = _timed(ctx, lambda: ctx.check(ctx.lib.blsq_cov_dev(h, d_J, dm, d_cov, d_rc, d_st), "cov"),
                             cov_reps)
            tree = T.get("qr_leaf", 0.0) + T.get("qr_merge", 0.0)
            tail = T.get("cov_inverse", 0.0) + T.get("cov_product", 0.0)
            out[label] = {"whole_ms": round(sum(T.values()), 4), "wall_ms": round(wall, 4), "tree_ms": round(tree, 4),
                          "inverse_ms": round(T.get("cov_inverse", 0.0), 4),
                          "product_ms": round(T.get("cov_product", 0.0), 4),
                          "inverse_plus_product_ms": round(tail, 4), "gather_ms": round(T.get("cov_gather", 0.0), 4),
                          "tail_over_tree": round(tail / tree, 3)}
            if dm is None:                           # the factor of the 'all' call is in the plan
                wall, T = _timed(ctx, rows_call, reps)
                rows["regular"] = {"cov_rows_ms": round(T.get("cov_rows", 0.0), 4), "wall_ms": round(wall, 4)}
        st = ctx.to_host(d_st, (B,), np.int32)
        out["singular"] = int(st.sum())
        for label, dm in (("pinv", None), ("free-pinv", d_mask)):
            wall, T = _timed(ctx, lambda: ctx.check(ctx.lib.blsq_cov_pinv_dev(h, d_J, dm, None, d_cov, d_rk, d_rc, d_kr,
                                                                               d_st), "cov_pinv"), cov_reps)
            tree = T.get("qr_leaf", 0.0) + T.get("qr_merge", 0.0)
            tail = T.get("cov_pinv_weights", 0.0) + T.get("cov_pinv_product", 0.0)
            out[label] = {"whole_ms": round(sum(T.values()), 4), "wall_ms": round(wall, 4), "tree_ms": round(tree, 4),
                          "jacobi_ms": round(T.get("jacobi_svd", 0.0), 4),
                          "weights_ms": round(T.get("cov_pinv_weights", 0.0), 4),
                          "product_ms": round(T.get("cov_pinv_product", 0.0), 4),
                          "weights_plus_product_ms": round(tail, 4), "gather_ms": round(T.get("cov_gather", 0.0), 4),
                          "jacobi_over_tree": round(T.get("jacobi_svd", 0.0) / tree, 3)}
            if dm is None:
                wall, T = _timed(ctx, rows_call, reps)
                rows["pinv"] = {"cov_rows_ms": round(T.get("cov_rows", 0.0), 4), "wall_ms": round(wall, 4)}

                def first_call():                    # a covariance call, then the row forms: the factor is refined
                    ctx.check(ctx.lib.blsq_cov_pinv_dev(h, d_J, None, None, d_cov, d_rk, d_rc, d_kr, d_st), "cov_pinv")
                    rows_call()
                wall, T = _timed(ctx, first_call, max(2, reps // 4))
                rows["pinv"]["cov_rows_first_call_ms"] = round(T.get("cov_rows", 0.0), 4)
        out["pinv_status_nonzero"] = int((ctx.to_host(d_st, (B,), np.int32) != 0).sum())
        out["pinv_over_inverse"] = round(out["pinv"]["whole_ms"] / out["all"]["whole_ms"], 3)
    finally:
        ctx.lib.blsq_cov_plan_destroy(h)
    # the step path's factorisation of the same J
    d_f = ctx.to_device(rng.standard_normal((B, m)))
    d_x = ctx.to_device(np.zeros((B, n)))
    d_lb = ctx.to_device(np.full((B, n), -np.inf))
    d_ub = ctx.to_device(np.full((B, n), np.inf))
    d_sc = ctx.to_device(np.ones((B, n)))
    sol = TrfStepSolver(B, m, n, ctx=ctx)
    try:
        wall, T = _timed(ctx, lambda: sol.factor_dev(d_J, d_f, d_x, d_lb, d_ub, d_sc), reps)
        out["trf_factor_dev"] = {"whole_ms": round(sum(T.values()), 4), "wall_ms": round(wall, 4),
                                 "slots_ms": {k: round(v, 4) for k, v in T.items()}}
    finally:
        sol.close()
        for p in (d_J, d_mask, d_cov, d_rc, d_st, d_rk, d_kr, d_f, d_x, d_lb, d_ub, d_sc, d_lev):
            ctx.free(p)
    out["cov_over_factor"] = round(out["all"]["whole_ms"] / out["trf_factor_dev"]["whole_ms"], 3)
    gram = out["trf_factor_dev"]["slots_ms"].get("gram", 0.0)
    rows["gram_ms"] = gram
    rows["gflop"] = round(2.0 * B * m * n * n / 2 * 1e-9, 3)      # (the triangular half of 2 m n^2)
    for route in ("regular", "pinv"):
        rows[route]["over_gram"] = round(rows[route]["cov_rows_ms"] / gram, 3) if gram > 0 else None
    return out, rows


def main():
    ctx = _abi.Context(0)
    res, res_rows = [], []
    for shp in SHAPES:
        r, rr = bench_shape(ctx, *shp, reps=5 if shp[0] * shp[1] * shp[2] > 1 << 28 else 20,
                            rows_only="--rows-only" in sys.argv)
        print(json.dumps(r), flush=True)
        print(json.dumps(rr), flush=True)
        res.append(r)
        res_rows.append(rr)
    ctx.close()
    for flag, data in (("--out", res), ("--rows-out", res_rows)):
        if flag in sys.argv:
            path = sys.argv[sys.argv.index(flag) + 1]
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as fh:
                json.dump(data, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
