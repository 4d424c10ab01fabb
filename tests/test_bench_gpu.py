"""bench.py as the driver runs it for N > 1 — but self-sufficient: `python bench.py --gpus 2 --config c5` with no launcher
around it starts its own two ranks (torch.distributed.run as a child), the ranks bring up the library's RCCL
communicator (here the socket stand-in, two processes on the one GPU; gloo for the bench's own barrier) and rank 0's
line reports what the first real multi-GPU run needs: n_gpus, per-rank clocks, the collective library and its span
(`--full`: the communicator of the batch configs and the roofline are not part of a plain line).  And the plain line at
N = 1: exactly --steps timed steps, and --dump-outputs writes what the host API returns for the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub_ccl", "libblsq_stub_ccl.so")


def _bench(*flags, world=2):
    if not os.path.exists(STUB):
        out = subprocess.run(["make", "-C", os.path.dirname(STUB)], capture_output=True, text=True)
        assert out.returncode == 0 and os.path.exists(STUB), out.stdout[-1500:] + out.stderr[-1500:]
    env = dict(os.environ, BLSQ_RCCL_PATH=STUB, BLSQ_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "5", "--warmup", "1",
           "--min-time", "0", "--no-probe", "--no-side", "--check", "0", "--full"] + list(flags)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks_for_the_tall_problem():
    line = _bench("--config", "c5")
    assert line["n_gpus"] == 2 and line["steps"] == 5
    assert line["rccl"]["ranks"] == 2 and line["rccl"]["library"].endswith("libblsq_stub_ccl.so")
    assert len(line["per_rank"]["elapsed_s"]) == 2
    assert "250000 rows per rank" in line["config"]["sharding"]
    assert line["roofline"]["frac"] > 0 and line["value"] > 0


def test_batch_configs_at_two_ranks_report_the_communicator_too():
    line = _bench("--config", "c4")
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert line["rccl"]["ranks"] == 2
    assert len(line["per_rank"]["step_solves_per_s"]) == 2
    # (a latency-bound dominant slot claims no kernel roofline; with two ranks' launches interleaving on ONE card the
    #  slot that dominates rank 0's five steps is the Gram in some runs, the Newton rounds' Cholesky in most)
    roof = line["roofline"]
    assert roof["scope"] == ("kernel" if roof["kernel"] in ("gram", "qr_leaf") else "whole_step")
    # whole-job rate = what both ranks did over the slowest rank's clock
    assert line["value"] == pytest.approx(2 * 1024 * 5 / max(line["per_rank"]["elapsed_s"]), rel=1e-6)


def test_plain_line_times_exactly_the_steps_and_dumps_what_the_caller_gets(tmp_path):
    B, m, n = 16, 512, 64
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c4", "--batch", str(B),
           "--steps", "7", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["n_gpus"] == 1 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["unit"] == "step-solves/s" and line["value"] == pytest.approx(B * 1e3 / line["ms_per_step"], rel=1e-9)
    assert "roofline" not in line and line["parity"] is None and line["cpu_baseline"] is None

    dump = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert all(a.dtype == np.float64 and a.shape[0] == B for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) < 64e6
    # the same seeded inputs through the host API: what a caller of the timed path receives
    from bounded_lsq import TrfStepSolver, _synth
    P = _synth.trf_batch(10_000, B, m, n)
    sol = TrfStepSolver(B, m, n)
    F = sol.factor(P["J"], P["f"], P["x"], P["lb"], P["ub"], P["scale"])
    S = sol.step(np.where(np.arange(B) % 2 == 0, 10.0, 0.5), np.zeros(B))
    sol.close()
    for k in S._fields + F._fields:
        assert k in dump, k
    assert np.linalg.norm(dump["step"] - S.step) <= 1e-12 * np.linalg.norm(S.step)
    assert np.linalg.norm(dump["g"] - F.g) <= 1e-12 * np.linalg.norm(F.g)
    for k in ("hits", "active_new", "n_iter", "branch", "status"):
        assert np.array_equal(dump[k], getattr(S, k).astype(np.float64)), k
