"""The ownership rules of the host side's buffers (csrc/dev_buf.h), without a GPU: tests/dev_buf_host is a stand-alone
program that supplies hipMalloc / hipFree / hipHostMalloc / hipHostFree itself (malloc / free and a live-allocation
counter), is compiled with the address and undefined-behaviour sanitizers and run directly.  It checks moves through a
growing vector, move construction / assignment / self-move, alloc on a live buffer, alloc(0), a double release, an
alloc_all that fails half way, and that nothing is live at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dev_buf_host")


def test_dev_buf_host(tmp_path):
    exe = str(tmp_path / "dev_buf_host")
    out = subprocess.run(["make", "-C", SRC, "OUT=" + exe], capture_output=True, text=True)
    assert out.returncode == 0 and os.path.exists(exe), out.stdout[-1500:] + out.stderr[-1500:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert "dev_buf_host ok" in run.stdout and run.stderr.strip() == "", run.stdout + run.stderr
