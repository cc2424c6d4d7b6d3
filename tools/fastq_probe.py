"""FASTA vs FASTQ input on the C3 shape (10 k leaves, k = 12, 1 M x 150 bp reads, SynthDb.reads): the same reads
written once as FASTA and once as FASTQ with random qualities.  Prints one JSON line:
  * stage_ms: the device stage alone on text already in HBM (cls_fasta_scan_device, cls_fastq_scan_device with
    trimming off and with -q 20), median of `--runs`, and the input GB/s of each;
  * text_placements_per_s: cls_place_fasta_text vs cls_place_fastq_text (H2D of the text + stage + placement + D2H);
  * file_s: query file -> result file through the use-case cls-place runs (cls_place_sequences[_ex], JSONL; database
    load excluded), one warm-up then one timed run per format.
usage: fastq_probe.py [--reads N] [--runs R]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from classeq2_amd import _abi, engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402


class FastaDev(C.Structure):  # cls_fasta_dev
    _fields_ = [("n", C.c_uint32), ("truncated", C.c_uint32), ("d_headers", C.c_void_p), ("d_header_off", C.c_void_p),
                ("d_bases", C.c_void_p), ("d_base_off", C.c_void_p), ("n_header_bytes", C.c_uint64), ("n_bases", C.c_uint64)]


def median_s(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def tree_json(flat, path):
    nodes = flat.nodes
    sys.setrecursionlimit(1_000_000)
    kinds = ["ROOT", "NODE", "LEAF"]

    def clade(r):
        d = {"id": int(nodes[r]["id"]), "parent": None if int(nodes[r]["parent"]) == _abi.NO_PARENT else int(nodes[r]["parent"]),
             "kind": kinds[int(nodes[r]["kind"])]}
        if nodes[r]["kind"] == 2:
            d["name"] = f"leaf_{int(nodes[r]['id'])}"
        else:
            d["support"] = 100.0
        d["length"] = 0.01
        if nodes[r]["has_children"]:
            d["children"] = [clade(int(nodes[r]["first_child"]) + i) for i in range(int(nodes[r]["n_children"]))]
        return d

    with open(path, "w") as f:
        json.dump(clade(0), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=CONFIGS["C3"]["n_reads"])
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    cfg = CONFIGS["C3"]
    n, L = a.reads, cfg["read_len"]
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    bases, offsets, _ = s.reads(n, L, seed=3)
    rows = bases.reshape(n, L)
    rng = np.random.default_rng(1)
    quals = rng.integers(2, 41, size=(n, L), dtype=np.uint8) + 33
    fasta = b"".join(b">r%d\n" % i + bytes(rows[i]) + b"\n" for i in range(n))
    fastq = b"".join(b"@r%d\n" % i + bytes(rows[i]) + b"\n+\n" + bytes(quals[i]) + b"\n" for i in range(n))
    res = {"config": "C3", "reads": n, "read_len": L, "runs": a.runs, "fasta_bytes": len(fasta), "fastq_bytes": len(fastq)}

    lib = engine.lib()
    lib.cls_fasta_scan_device.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(FastaDev), C.c_void_p]
    lib.cls_fastq_scan_device.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_abi.FastqOpts), C.POINTER(FastaDev), C.c_void_p]
    lib.cls_fasta_dev_free.argtypes = [C.POINTER(FastaDev)]
    torch.cuda.set_device(0)
    stages = {}
    for name, text, call in (("fasta", fasta, lambda p, m, d: lib.cls_fasta_scan_device(p, m, d, None)),
                             ("fastq", fastq, lambda p, m, d: lib.cls_fastq_scan_device(p, m, C.byref(engine._fastq_opts(0, 0)), d, None)),
                             ("fastq_q20", fastq, lambda p, m, d: lib.cls_fastq_scan_device(p, m, C.byref(engine._fastq_opts(0, 20)), d, None))):
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        counts = []

        def once():
            dv = FastaDev()
            rc = call(d_text.data_ptr(), len(text), C.byref(dv))
            torch.cuda.synchronize()
            assert rc == 0, lib.cls_last_error()
            counts.append((dv.n, dv.n_bases))
            lib.cls_fasta_dev_free(C.byref(dv))

        def timed():  # (the free is outside the window)
            dv = FastaDev()
            t0 = time.perf_counter()
            rc = call(d_text.data_ptr(), len(text), C.byref(dv))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert rc == 0, lib.cls_last_error()
            lib.cls_fasta_dev_free(C.byref(dv))
            return dt

        once()
        sec = statistics.median(timed() for _ in range(a.runs))
        stages[name] = {"ms": round(sec * 1e3, 3), "GB_per_s": round(len(text) / sec / 1e9, 1), "records": counts[0][0], "bases": counts[0][1]}
        del d_text
    assert stages["fasta"]["records"] == stages["fastq"]["records"] == n and stages["fasta"]["bases"] == stages["fastq"]["bases"]
    res["stage"] = stages
    res["fastq_vs_fasta_ns_per_byte"] = round((stages["fastq"]["ms"] / len(fastq)) / (stages["fasta"]["ms"] / len(fasta)), 2)

    with engine.PlacementDb(s.flat, device=0) as db:
        ref_recs = None
        text_rate = {}
        for name, fn in (("fasta", lambda: db.place_fasta_text(fasta)), ("fastq", lambda: db.place_fastq_text(fastq)),
                         ("fastq_q20", lambda: db.place_fastq_text(fastq, trim_3p=20))):
            sec = median_s(fn, a.runs)
            text_rate[name] = {"s": round(sec, 4), "placements_per_s": round(n / sec)}
            recs = fn()[1]
            if name == "fasta":
                ref_recs = recs
            elif name == "fastq":
                assert (recs == ref_recs).all()
        res["text_placements"] = text_rate

        tmp = tempfile.mkdtemp(prefix="cls_fastq_probe_")
        try:
            tree_json(s.flat, os.path.join(tmp, "tree.json"))
            tree = engine.Tree(os.path.join(tmp, "tree.json"))
            open(os.path.join(tmp, "q.fasta"), "wb").write(fasta)
            open(os.path.join(tmp, "q.fq"), "wb").write(fastq)
            files = {}
            for name, path, kw in (("fasta", "q.fasta", {}), ("fastq", "q.fq", {"query_format": "fastq"}),
                                   ("fastq_q20", "q.fq", {"query_format": "fastq", "trim_quality": 20})):
                engine.place_sequences(db, tree, os.path.join(tmp, path), os.path.join(tmp, "warm"), overwrite=True, fmt=engine.FORMAT_JSONL, **kw)
                got, sec = engine.place_sequences(db, tree, os.path.join(tmp, path), os.path.join(tmp, "res_" + name), overwrite=True,
                                                  fmt=engine.FORMAT_JSONL, **kw)
                assert got == n
                files[name] = {"window_s": round(sec, 4), "placements_per_s": round(n / sec)}
            assert open(os.path.join(tmp, "res_fasta.jsonl"), "rb").read() == open(os.path.join(tmp, "res_fastq.jsonl"), "rb").read()
            res["file_s"] = files
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
