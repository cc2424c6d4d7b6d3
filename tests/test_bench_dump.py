"""bench.py --dump-outputs: the records of the last timed step as float64 .npy files, capped at 64 MB by a fixed
sample of the reads, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from classeq2_amd import _abi
from classeq2_amd.synth import CONFIGS, SynthDb
from oracle import oracle_port as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("read",) + bench.DUMP_FIELDS


def _records(n, seed=5):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=_abi.PLACEMENT_DTYPE)
    r["status"] = rng.integers(0, 12, n)
    r["one"] = rng.integers(-5, 1 << 20, n)
    r["rest"] = rng.integers(-5, 1 << 20, n)
    r["levels"] = rng.integers(0, 900, n)
    r["clade_id"] = rng.integers(0, 1 << 40, n)
    return r


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}


def test_dump_outputs_writes_every_row_when_it_fits(tmp_path):
    recs = _records(1000)
    assert bench.dump_outputs(str(tmp_path), recs) == 1000
    got = _load(str(tmp_path))
    assert (got["read"] == np.arange(1000)).all()
    for f in bench.DUMP_FIELDS:
        assert got[f].dtype == np.float64 and (got[f] == recs[f]).all(), f


def test_dump_outputs_samples_large_outputs_within_the_cap(tmp_path):
    recs = _records(2_000_000)
    a, b = tmp_path / "a", tmp_path / "b"
    rows = bench.dump_outputs(str(a), recs)
    assert rows == bench.dump_outputs(str(b), recs) and 1_000_000 < rows < len(recs)
    assert sum(os.path.getsize(a / (k + ".npy")) for k in NAMES) <= bench.DUMP_CAP_BYTES
    ga, gb = _load(str(a)), _load(str(b))
    idx = ga["read"].astype(np.int64)
    assert len(idx) == rows and (np.diff(idx) > 0).all() and idx[-1] < len(recs)  # in stream order, no repeats
    for k in NAMES:
        assert (ga[k] == gb[k]).all(), k  # the same sample every run
    for f in bench.DUMP_FIELDS:
        assert (ga[f] == recs[f][idx]).all(), f


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """One GPU, fresh child process: --steps sets the timed steps, ms_per_step is reported, and the dumped outputs are
    the oracle's records of the same seeded reads."""
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "C2",
           "--reads", "5000", "--no-cpu-baseline", "--no-host-window", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["config"]["dumped_outputs"] == {"rows": 5000, "of": 5000}
    got = _load(str(out))
    assert (got["read"] == np.arange(5000)).all()
    cfg = CONFIGS["C2"]
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    bases, offsets, _ = s.reads(5000, cfg["read_len"], seed=3)
    want = op.OraclePort(s.flat).place_batch(bases, offsets, threads=8)
    for f in bench.DUMP_FIELDS:
        assert (got[f] == want[f]).all(), f
