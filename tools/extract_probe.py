"""Read extraction on the C3 shape (10 k leaves, k = 12): 1 M reads of 150 bp as FASTQ (314 bytes a record).  One JSON
line; device times are HIP events, one warm-up, then the median (and min..max) of `--runs`.  For three selectors -- the
whole tree, one child of the root, one small deep clade -- it reports:
  * select_ms: the selection kernel (cls_select_records_device) on the records of the placement step;
  * spans_ms: the span step (cls_fastq_spans_device: the newline passes + one entry per record; it synchronises);
  * plan_ms, gather_ms: cls_extract_plan_device (lengths + exclusive sum; it synchronises) and cls_extract_gather_device;
  * bytes_out, gather_gb_s: bytes written and bytes written per second of the gather;
  * memcpy_ms: a hipMemcpyAsync device-to-device copy of the same number of bytes, in this process; gather_over_memcpy;
next to place_ms, cls_place_batch_device on the same reads, and the wall times of cls_extract_fastq_text and
cls_tally_fastq_text on the same text (H2D of the text included).  The gathered bytes are compared with cls_extract_host.
Fails without a GPU: the extraction has no host fallback.
usage: extract_probe.py [--reads N] [--runs R]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from classeq2_amd import _abi, engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def timed(fn, runs):
    v = [event_ms(fn) for _ in range(runs + 1)][1:]  # run 0: a warm-up
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def fastq_text(bases, n, L):
    """n reads of L bases -> "@r<7 digits>\\n<bases>\\n+\\n<qualities>\\n" per read, as one uint8 array."""
    rec = np.empty((n, 10 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    idx = np.arange(n)
    for d in range(7):
        rec[:, 2 + d] = ord("0") + (idx // 10 ** (6 - d)) % 10
    rec[:, 9] = 10
    rec[:, 10:10 + L] = bases.reshape(n, L)
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 13 + L:13 + 2 * L] = ord("I")
    rec[:, 13 + 2 * L] = 10
    return rec.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=CONFIGS["C3"]["n_reads"])
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "extract_probe needs a GPU"
    assert a.reads <= 10 ** 7
    cfg = CONFIGS["C3"]
    n, L = a.reads, cfg["read_len"]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    nodes = s.flat.nodes
    bases, offsets, _ = s.reads(n, L, seed=3)
    text = fastq_text(bases, n, L)
    text_bytes = text.tobytes()
    res = {"config": "C3", "reads": n, "read_len": L, "runs": a.runs, "text_bytes": len(text_bytes), "n_nodes": int(len(nodes)),
           "kernels": ["select_records_kernel", "fastq_spans_kernel", "extract_lengths_kernel", "extract_gather_kernel"]}

    depth = np.zeros(len(nodes), dtype=np.int64)
    for r in range(len(nodes)):
        fc, nc = int(nodes[r]["first_child"]), int(nodes[r]["n_children"])
        depth[fc:fc + nc] = depth[r] + 1
    inner = np.nonzero(nodes["n_children"] > 0)[0]
    deep = int(inner[np.argmax(depth[inner])])
    selectors = {"whole_tree": int(nodes["id"][0]), "root_child": int(nodes["id"][int(nodes[0]["first_child"])]), "deep_clade": int(nodes["id"][deep])}

    with engine.PlacementDb(s.flat, device=0) as db, engine.Tally(db) as tally:
        db.set_max_read_len(L + 10)
        d_b = torch.from_numpy(bases).to(dev)
        d_o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
        d_recs = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        res["place_ms"] = timed(lambda: db.place_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, d_recs.data_ptr()), a.runs)
        torch.cuda.synchronize()
        recs = d_recs.cpu().numpy().view(_abi.PLACEMENT_DTYPE).copy()
        del d_b, d_o
        d_text = torch.from_numpy(text).to(dev)
        d_sel = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_rec_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_out = torch.zeros(len(text_bytes) + 16, dtype=torch.uint8, device=dev)
        d_copy = torch.zeros(len(text_bytes) + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        res["spans_ms"] = timed(lambda: engine.fastq_spans_device(d_text.data_ptr(), len(text_bytes), n, d_rec_off.data_ptr()), a.runs)
        res["selectors"] = {}
        for name, clade in selectors.items():
            out = {"clade_id": clade}
            with engine.Selector(db, [clade]) as sel:
                out["select_ms"] = timed(lambda: sel.select_device(d_recs.data_ptr(), n, d_sel.data_ptr()), a.runs)
                tot = {}
                plan = lambda: tot.update(t=engine.extract_plan_device(d_text.data_ptr(), d_rec_off.data_ptr(), 1, n, d_sel.data_ptr(), d_out_off.data_ptr()))
                out["plan_ms"] = timed(plan, a.runs)
                nbytes = int(tot["t"]["bytes_out"])
                out["n_selected"], out["bytes_out"] = int(tot["t"]["n_selected"]), nbytes
                gather = lambda: engine.extract_gather_device(d_text.data_ptr(), d_rec_off.data_ptr(), 1, n, d_sel.data_ptr(), d_out_off.data_ptr(),
                                                              d_out.data_ptr())
                out["gather_ms"] = timed(gather, a.runs)
                out["memcpy_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy.data_ptr(), d_text.data_ptr(), max(nbytes, 1), 3, None), a.runs)
                out["gather_gb_s"] = round(nbytes / out["gather_ms"]["median"] / 1e6, 1)
                out["memcpy_gb_s"] = round(nbytes / out["memcpy_ms"]["median"] / 1e6, 1)
                out["gather_over_memcpy"] = round(out["gather_ms"]["median"] / out["memcpy_ms"]["median"], 2)
                extract_ms = out["select_ms"]["median"] + res["spans_ms"]["median"] + out["plan_ms"]["median"] + out["gather_ms"]["median"]
                out["extract_over_place"] = round(extract_ms / res["place_ms"]["median"], 4)
                torch.cuda.synchronize()
                pick = engine.select_host(s.flat, recs, [clade])
                assert np.array_equal(d_sel.cpu().numpy(), pick), "device selection differs from the host's"
                want, _ = engine.extract_host(text_bytes, pick)
                assert d_out[:nbytes].cpu().numpy().tobytes() == want, "gathered bytes differ from the host's"
                walls = {"extract": [], "tally": []}
                for run in range(3):
                    t0 = time.perf_counter()
                    got = db.extract_fastq_text(sel, text_bytes)
                    t1 = time.perf_counter()
                    tally.reset()
                    t2 = time.perf_counter()
                    db.tally_fastq_text(tally, text_bytes)
                    t3 = time.perf_counter()
                    if run:
                        walls["extract"].append(t1 - t0), walls["tally"].append(t3 - t2)
                assert got[0] == want
                out["extract_fastq_text_s"] = round(min(walls["extract"]), 4)
                out["tally_fastq_text_s"] = round(min(walls["tally"]), 4)
            res["selectors"][name] = out
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
