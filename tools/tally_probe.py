"""Clade tally on the C3 shape (10 k leaves, k = 12, 1 M x 150 bp reads, the bench's tree and reads).  One JSON line:
  * add_ms: device time (HIP events) of cls_tally_add_device on the 1 M device-resident records of a placement step,
    for the real records and for the worst skew (every record CLS_IDENTITY_FOUND on one leaf), each with and without
    the kernel's wave-level step (knob tally_no_wave_combine), the variants alternated run by run, median of
    `--runs`; next to it the placement step of the same run and the floor: 24 bytes a record over the HBM rate;
  * read_ms: cls_tally_read (subtree sums on the device + the copy of the counters);
  * file_s: query file -> clade report (cls_profile_sequences, one piece and the default piece size) against query
    file -> JSONL result file (cls_place_sequences_ex), FASTA and FASTQ, the routes alternated run by run, median and
    min..max of `--runs` after one warm-up of each.
Fails without a GPU: the tally has no host fallback.
usage: tally_probe.py [--reads N] [--runs R] [--hbm-tb-s X]   (GPU box)"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from classeq2_amd import _abi, engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402
from tools.fastq_probe import tree_json  # noqa: E402


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=CONFIGS["C3"]["n_reads"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hbm-tb-s", type=float, default=8.0, help="HBM rate the floor is taken from (TB/s)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tally_probe needs a GPU"
    cfg = CONFIGS["C3"]
    n, L = a.reads, cfg["read_len"]
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    bases, offsets, _ = s.reads(n, L, seed=3)
    res = {"config": "C3", "reads": n, "read_len": L, "runs": a.runs, "n_nodes": int(len(s.flat.nodes))}
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    med = statistics.median

    with engine.PlacementDb(s.flat, device=0) as db, engine.Tally(db) as tally:
        db.set_max_read_len(L + 10)
        d_b = torch.from_numpy(bases).to(dev)
        d_o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
        d_out = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        place = lambda: db.place_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr())
        place()
        torch.cuda.synchronize()
        recs = d_out.cpu().numpy().view(_abi.PLACEMENT_DTYPE)
        leaf = int(s.flat.nodes["id"][np.nonzero(s.flat.nodes["kind"] == _abi.KIND_LEAF)[0][0]])
        skew = np.zeros(n, dtype=_abi.PLACEMENT_DTYPE)
        skew["status"], skew["clade_id"], skew["one"], skew["rest"] = _abi.IDENTITY_FOUND, leaf, 40, -400
        d_skew = torch.from_numpy(skew.view(np.uint8)).to(dev)
        bufs = {"real": d_out, "one_clade": d_skew}
        times = {(k, w): [] for k in bufs for w in (0, 1)}
        place_ms = []
        for run in range(a.runs + 1):  # (run 0 warms up)
            p = event_ms(place)
            if run:
                place_ms.append(p)
            for k, buf in bufs.items():
                for w in (0, 1):
                    engine.set_tuning("tally_no_wave_combine", w)
                    ms = event_ms(lambda: tally.add_device(buf.data_ptr(), n))
                    if run:
                        times[(k, w)].append(ms)
        engine.set_tuning("tally_no_wave_combine", 0)
        floor_ms = n * 24 / (a.hbm_tb_s * 1e12) * 1e3
        res["place_step_ms"] = round(med(place_ms), 4)
        res["floor_ms"] = round(floor_ms, 5)
        res["add_ms"] = {f"{k}{'_no_wave_combine' if w else ''}": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                                                   "x_floor": round(med(v) / floor_ms, 1)} for (k, w), v in times.items()}
        res["add_over_place_step"] = round(med(times[("real", 0)]) / med(place_ms), 4)
        # the counters are what the host says (every variant added the same records the same number of times)
        tally.reset()
        tally.add_device(d_out.data_ptr(), n)
        import time
        t0 = time.perf_counter()
        got = tally.read()
        res["read_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        want = engine.tally_host(s.flat, recs)
        assert all((got[0][f] == want[0][f]).all() for f in _abi.TALLY_ROW_DTYPE.names), "device tally differs from the host's"
        res["distinct_clades"] = int((got[0]["n_direct"] > 0).sum())
        res["top_clade_share"] = round(float(got[0]["n_direct"].max()) / max(1, int(got[0]["n_direct"].sum())), 4)
        del d_b, d_o, d_out, d_skew

        rows = bases.reshape(n, L)
        rng = np.random.default_rng(1)
        quals = rng.integers(2, 41, size=(n, L), dtype=np.uint8) + 33
        tmp = tempfile.mkdtemp(prefix="cls_tally_probe_")
        try:
            tree_json(s.flat, os.path.join(tmp, "tree.json"))
            tree = engine.Tree(os.path.join(tmp, "tree.json"))
            qa, qq = os.path.join(tmp, "q.fasta"), os.path.join(tmp, "q.fq")
            open(qa, "wb").write(b"".join(b">r%d\n" % i + bytes(rows[i]) + b"\n" for i in range(n)))
            open(qq, "wb").write(b"".join(b"@r%d\n" % i + bytes(rows[i]) + b"\n+\n" + bytes(quals[i]) + b"\n" for i in range(n)))
            files = {}
            for fmt, path in (("fasta", qa), ("fastq", qq)):
                routes = {
                    "per_read_jsonl": lambda: engine.place_sequences(db, tree, path, os.path.join(tmp, "res"), overwrite=True, fmt=engine.FORMAT_JSONL,
                                                                    query_format=fmt)[1],
                    "report_one_piece": lambda: engine.profile_sequences(db, tree, path, os.path.join(tmp, "rep1.tsv"), overwrite=True, query_format=fmt,
                                                                        piece_bytes=1 << 40)[1],
                    "report_default_pieces": lambda: engine.profile_sequences(db, tree, path, os.path.join(tmp, "rep.tsv"), overwrite=True,
                                                                             query_format=fmt)[1],
                }
                secs = {k: [] for k in routes}
                for run in range(a.runs + 1):
                    for k, fn in routes.items():
                        sec = fn()
                        if run:
                            secs[k].append(sec)
                assert open(os.path.join(tmp, "rep1.tsv"), "rb").read() == open(os.path.join(tmp, "rep.tsv"), "rb").read()
                files[fmt] = {k: {"median_s": round(med(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4), "reads_per_s": round(n / med(v))}
                              for k, v in secs.items()}
                files[fmt]["report_over_per_read"] = round(med(secs["report_default_pieces"]) / med(secs["per_read_jsonl"]), 4)
            res["file_s"] = files
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
