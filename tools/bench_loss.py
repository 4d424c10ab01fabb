"""Robust loss functions on the device (loss_kernels.hip): what they cost.

1. The scale kernel (blsq_loss_scale_dev: J <- diag(w) J in place, f_s) on 1024 x 512 x 64 and 1 x 250000 x 128:
   bytes per second (J read + written, f read, f_s written) against the streaming copy probe (blsq_debug_probe kind 1)
   of the same size in the same run.
2. The device-resident outer driver with torch callbacks (nothing but counters leaves the GPU), soft_l1 against
   linear on the same batch: step-solves per second (trial steps of all problems / wall time), 512 x 64 and 4096 x 256.
   B problems  min sum rho(A_b tanh(x) - y_b), 10 % gross outliers, bounded.

usage: python tools/bench_loss.py [--skip-kernel] [--skip-driver]
"""
import json
import os
import sys
import time

import numpy as np
import torch                      # user-side (callbacks); imported first so ONE HIP runtime is loaded
torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import OuterDriver, _abi                                # noqa: E402
from bounded_lsq._hostmath import shift_into_interior, LOSSES           # noqa: E402


def kernel_bandwidth(ctx, B, m, n, reps=20):
    rng = np.random.default_rng(0)
    d_J = ctx.to_device(rng.standard_normal((B, m, n)))
    d_f = ctx.to_device(rng.standard_normal((B, m)) * 3.0)
    d_fs = ctx.malloc(8 * B * m)
    d_sc = ctx.to_device(np.full(B, 0.5))
    try:
        loss = LOSSES.index('soft_l1')
        for _ in range(3):                                         # warm-up (J grows by w each time: harmless)
            ctx.loss_scale_dev(B, m, n, loss, d_sc, d_f, d_J, d_fs)
        ctx.sync()
        ctx.timing(True, only="loss_scale")
        ctx.timing_reset()
        for _ in range(reps):
            ctx.loss_scale_dev(B, m, n, loss, d_sc, d_f, d_J, d_fs)
        ctx.sync()
        ms, cnt = ctx.timing_read()["loss_scale"]
        ctx.timing(False)
    finally:
        for p in (d_J, d_f, d_fs, d_sc):
            ctx.free(p)
    per = ms / cnt
    moved = 2.0 * 8 * B * m * n + 2.0 * 8 * B * m
    mib = max(1, int(8 * B * m * n / 2 ** 20))
    cp_gbs, _, _ = ctx.probe("copy", mib)
    return {"shape": [B, m, n], "ms": round(per, 4), "GBps": round(moved / per / 1e6, 1),
            "copy_probe_GBps": round(cp_gbs, 1), "fraction_of_probe": round(moved / per / 1e6 / cp_gbs, 3)}


class _Dev:                                   # raw device pointer -> torch tensor, zero copy
    def __init__(self, p, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (int(p.value), False), "version": 2}


def wrap(p, shape, typestr="<f8"):
    return torch.as_tensor(_Dev(p, shape, typestr), device="cuda")


def driver_rate(ctx, B, m, n, loss, method="trf"):
    rng = np.random.default_rng(1)
    A = rng.standard_normal((B, m, n)) / np.sqrt(n)
    xt = rng.uniform(-0.7, 0.7, (B, n))
    Y = np.einsum('bmn,bn->bm', A, np.tanh(xt)) + 1e-3 * rng.standard_normal((B, m))
    out = rng.random((B, m)) < 0.1
    Y[out] += rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(1.0, 3.0, int(out.sum()))
    X0 = np.zeros((B, n))
    lb, ub = np.full(n, -0.8), np.full(n, 0.8)
    At = torch.as_tensor(A, device="cuda")
    Yt = torch.as_tensor(Y, device="cuda")
    del A

    def fun_dev(xp, fp, reps):
        x = wrap(xp, (B, reps, n))
        f = wrap(fp, (B, reps, m))
        torch.baddbmm(-Yt.unsqueeze(1).expand(B, reps, m), torch.tanh(x), At.transpose(1, 2), out=f)

    def jac_dev(xp, Jp, mp):
        x = wrap(xp, (B, n))
        J = wrap(Jp, (B, m, n))
        Jn = At * (1.0 - torch.tanh(x) ** 2).unsqueeze(1)
        if mp is None:
            J.copy_(Jn)
        else:                                     # with a loss: the fresh Jacobians only
            sel = wrap(mp, (B,), "<i4") != 0
            J[sel] = Jn[sel]

    xs = np.stack([shift_into_interior(X0[b], lb, ub, rstep=1e-10) for b in range(B)]) if method == "trf" else X0
    with OuterDriver(method, B, m, n, ctx=ctx) as drv:
        if loss != 'linear':
            drv.set_loss(loss, 0.05)
        drv.start(X0, xs, lb, ub, np.ones(n), False, 1e-8, 1e-8, 1e-8, 50)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R = drv.run_device(fun_dev, jac_dev, sync=torch.cuda.synchronize)
        dt = time.perf_counter() - t0
    steps = int((R["nfev"] - 1).sum())
    return {"shape": [B, m, n], "method": method, "loss": loss, "s": round(dt, 4), "step_solves": steps,
            "step_solves_per_s": round(steps / dt, 1), "mean_nfev": round(float(R["nfev"].mean()), 2),
            "mean_njev": round(float(R["njev"].mean()), 2)}


def main():
    ctx = _abi.Context(0)
    res = {"kernel": [], "driver": []}
    if "--skip-kernel" not in sys.argv:
        for shp in ((1024, 512, 64), (1, 250000, 128)):
            r = kernel_bandwidth(ctx, *shp)
            print("scale kernel", json.dumps(r), flush=True)
            res["kernel"].append(r)
    if "--skip-driver" not in sys.argv:
        for shp in ((1024, 512, 64), (64, 4096, 256)):
            for method in ("trf", "dogbox"):
                base = None
                for loss in ("linear", "soft_l1"):
                    driver_rate(ctx, *shp, loss, method)             # warm-up (plans, code objects)
                    r = driver_rate(ctx, *shp, loss, method)
                    if base is None:
                        base = r
                    else:
                        r["vs_linear"] = round(r["step_solves_per_s"] / base["step_solves_per_s"], 3)
                    print("device driver", json.dumps(r), flush=True)
                    res["driver"].append(r)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
