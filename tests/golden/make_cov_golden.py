"""Capture the covariance fixture from the REFERENCE implementation (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cov_golden.py

Imports /root/reference/bounded_lsq (read-only mount), runs its MINPACK bridge
``least_squares(method='lm', scaling='jac')`` — the only path of the reference that fills ``x_covariance`` — on three
unbounded problems of tests/_suite.py and writes DATA only to tests/golden/cov_lm.json: per problem

  x             the bridge's solution
  x_covariance  its covariance (hex floats)
  d             max_ij |C_lm - inv(J^T J)_trf|_ij / sqrt(C_ii C_jj), with J the Jacobian of the reference's own
                ``method='trf'`` result for the same problem: what the reference's two solvers stopping at slightly
                different x costs by itself.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _suite import SUITE_BY_NAME  # noqa: E402
import bounded_lsq as ref  # noqa: E402  THE REFERENCE

assert ref.__file__.startswith("/root/reference"), ref.__file__

# problems with a non-zero residual at the solution: on a zero-residual problem both solvers converge quadratically
# to the same point and d measures rounding alone
NAMES = ["kowalik_osborne", "bard", "watson"]


def main():
    out = {}
    for name in NAMES:
        p = SUITE_BY_NAME[name]
        lm = ref.least_squares(p["fun"], p["x0"], p["jac"], method='lm', scaling='jac')
        tr = ref.least_squares(p["fun"], p["x0"], p["jac"], method='trf', scaling='jac')
        C = np.asarray(lm.x_covariance, dtype=float)
        J = np.asarray(tr.jac, dtype=float)
        Ct = np.linalg.inv(J.T @ J)
        s = np.sqrt(np.diag(C))
        d = float(np.max(np.abs(C - Ct) / np.outer(s, s)))
        out[name] = dict(x=[float(v).hex() for v in lm.x], x_covariance=[[float(v).hex() for v in row] for row in C],
                         d=d, lm_status=int(lm.status), trf_status=int(tr.status))
        print(name, "d =", d, "lm status", lm.status, "trf status", tr.status)
    with open(os.path.join(HERE, "cov_lm.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
