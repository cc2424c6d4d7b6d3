"""Host-buffer placement on one handle vs. index groups, on the C3 shape (10 k leaves, k = 12, 1 M x 150 bp reads):
cls_place_batch, group [0], group [0, 0] and, with more than one GPU, [0 .. N-1].  Median of `--runs` timed calls after a
warm-up; prints one JSON line.  Every group's records are checked against the single handle's.
usage: group_probe.py [--reads N] [--runs R]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from classeq2_amd import engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402


def timed(fn, runs):
    fn()  # warm-up: grows the staging buffers
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=CONFIGS["C3"]["n_reads"])
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    cfg = CONFIGS["C3"]
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    bases, offsets, _ = s.reads(a.reads, cfg["read_len"], seed=3)
    res = {"config": "C3", "reads": a.reads, "runs": a.runs, "gpus": engine.device_count()}
    with engine.PlacementDb(s.flat, device=0) as db:
        sec, want = timed(lambda: db.place_batch(bases, offsets), a.runs)
        res["single_ms"] = round(sec * 1e3, 2)
    layouts = {"group_0": [0], "group_0_0": [0, 0]}
    if engine.device_count() > 1:
        layouts["group_all"] = list(range(engine.device_count()))
    for name, devs in layouts.items():
        t0 = time.perf_counter()
        with engine.PlacementDbGroup(s.flat, devs) as grp:
            res[name + "_create_s"] = round(time.perf_counter() - t0, 2)
            sec, got = timed(lambda: grp.place_batch(bases, offsets), a.runs)
        for f in ("status", "one", "rest", "levels", "clade_id"):
            assert (got[f] == want[f]).all(), (name, f)
        res[name + "_ms"] = round(sec * 1e3, 2)
    res["placements_per_s_single"] = round(a.reads / res["single_ms"] * 1e3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
