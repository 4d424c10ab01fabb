"""Diagnostic: timeline of stage 0 of the certificate (one-pass form) for ONE problem (diagnostic build).

  BLSQ_LIB=.../libblsq_hip_diag.so python tools/cert0_stamps.py [B]

The backward solve is the shared look-ahead routine (tri_solve_upper_pf_la, tri_ops.h; stamps through the hook of
gram_cert0_kernel): per block step kb = 15 .. 1 wave 0 waits at the ONE barrier, updates the sixteen rows of block kb-1
and substitutes them, while wave 2 (one of the bulk waves) waits for its DMA pieces, passes the barrier, issues the next
panel and updates the rows above.  The three-barrier routine (blsq_debug_tri_reference) carries no stamps."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bounded-lsq_amd"))
from bounded_lsq import TrfStepSolver, _abi, _synth
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
P = _synth.trf_batch(1, B, 1024, 256)
ctx = _abi.Context(0)
sol = TrfStepSolver(B, 1024, 256, ctx=ctx)
d = {k: ctx.to_device(P[k]) for k in ("J", "f", "x", "lb", "ub", "scale")}
for _ in range(3):
    sol.factor_dev(d["J"], d["f"], d["x"], d["lb"], d["ub"], d["scale"]); ctx.sync()
st = np.zeros((4, 20, 8), dtype=np.int64)
fn = ctx.lib.blsq_debug_chol_stamps; fn.argtypes = [C.c_void_p]; fn.restype = C.c_int
assert fn(st.ctypes.data) == 0
us = lambda x: 0.01 * x
m = st[0][18]
print("B = %d: entry -> scales + share read %.2f, invdiag + init %.2f, backward solve %.2f, reductions + verdict %.2f; total %.2f us"
      % (B, us(m[1] - m[0]), us(m[2] - m[1]), us(m[3] - m[2]), us(m[4] - m[3]), us(m[4] - m[0])))
tops = [us(st[1][kb][1]) for kb in range(15, 0, -1)]
print("block steps kb = 15 .. 2, top to top of wave 0 (us):", np.round(np.diff(tops), 2))
print("barriers per block step: 1")
print("wave 0: per step — wait at the barrier, row update of block kb-1, substitution + store  | path in all")
for kb in (15, 12, 8, 4, 2):
    r = st[1][kb]
    print("  kb %2d: barrier %.2f  update %.2f  substitution %.2f  | %.2f"
          % (kb, us(r[3] - r[1]), us(r[5] - r[3]), us(r[6] - r[5]), us(r[6] - r[3])))
print("wave 2: per step — wait for its DMA pieces, barrier, issue of the next panel, bulk update  | path in all")
for kb in (15, 12, 8, 4, 2):
    r = st[2][kb]
    print("  kb %2d: vmcnt %.2f  barrier %.2f  issue %.2f  update %.2f  | %.2f"
          % (kb, us(r[2] - r[1]), us(r[3] - r[2]), us(r[4] - r[3]), us(r[6] - r[4]), us(r[6] - r[3])))
