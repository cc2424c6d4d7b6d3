"""bench.py with and without --full: a plain run prints the headline line only; --full adds the host-buffer window and
the CPU baseline, whose oracle records it checks against the GPU's.  Both in fresh child processes on one GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("host_window", "cpu_baseline", "parity_checked_reads")


def _run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "C2",
           "--reads", "5000", *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_leaves_the_extras_to_full():
    plain = _run_bench()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in plain, k
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0
    assert not any(k in plain for k in EXTRAS), sorted(plain)
    full = _run_bench("--full")
    assert all(k in full for k in EXTRAS), sorted(full)
    assert 0 < full["parity_checked_reads"] <= 5000
    assert full["host_window"]["pinned"]["ms"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["metric"] == plain["metric"] and full["config"]["status_counts"] == plain["config"]["status_counts"]
