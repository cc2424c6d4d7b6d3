"""Index-build probe: the device builder (cls_kmers_build) on synthetic references of the benchmark's sizes, and the
host builder (cls_tree_build_kmers_map) where it finishes in reasonable time.  One JSON line per config:

  windows, distinct k-mers, output postings, device build ms per phase (hash, sort, group, D2H) and in all (wall clock
  of the call, host-side leaf -> path expansion included), peak device bytes, host builder seconds (C3, G35).

The synthetic leaf sequences are fed as records, one per leaf.  For the configs with a host number the same records go
through both builders as a Newick + MSA pair and the two maps are compared array for array.

  python tools/build_probe.py [--configs C3,G35,C5] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classeq2_amd import engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402

THREADS = 16  # host threads of the generator (a GPU machine's share)
PROBES = {
    "C3": dict(cfg="C3", leaves_only=False, host=True),
    "C3L": dict(cfg="C3", leaves_only=True, host=False),
    "G35": dict(cfg="G35", leaves_only=False, host=True),
    "C5": dict(cfg="C5", leaves_only=True, host=False),
}


def records(s):
    seqs = b"".join(s.leaf_seq(i).encode() for i in range(s.n_leaves))
    offsets = np.arange(s.n_leaves + 1, dtype=np.uint64) * np.uint64(s.ref_len)
    leaf_ids = np.array([s.leaf_id(i) for i in range(s.n_leaves)], dtype=np.uint64)
    return np.frombuffer(seqs, dtype=np.uint8), offsets, leaf_ids


def newick_and_msa(s):
    """The generator's tree as Newick (leaf names L<id>) and its leaf sequences as the MSA."""
    nodes = s.flat.nodes
    out = []
    stack = [(0, 0)]
    while stack:  # iterative post-order text
        r, state = stack.pop()
        nc, fc = int(nodes["n_children"][r]), int(nodes["first_child"][r])
        if nc == 0:
            out.append(f"L{int(nodes['id'][r])}")
            continue
        if state < nc:
            out.append("(" if state == 0 else ",")
            stack.append((r, state + 1))
            stack.append((fc + state, 0))
        else:
            out.append(")")
    msa = "".join(f">L{s.leaf_id(i)}\n{s.leaf_seq(i)}\n" for i in range(s.n_leaves))
    return "".join(out) + ";", msa.encode()


def probe(label, spec, repeat, device):
    cfg = dict(CONFIGS[spec["cfg"]])
    k, m = cfg["k_size"], cfg["m_size"]
    t0 = time.perf_counter()
    s = SynthDb(**{**cfg, "threads": THREADS, "tips_only": spec["leaves_only"] or cfg.get("tips_only", False)})
    gen_s = time.perf_counter() - t0
    bases, offsets, leaf_ids = records(s)
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        flat, info = engine.build_kmers(s.flat.nodes, bases, offsets, leaf_ids, k, m, leaves_only=spec["leaves_only"], device=device,
                                         return_info=True)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or wall < best[0]:
            best = (wall, info)
        del flat
    wall, info = best
    rec = dict(config=spec["cfg"], label=label, n_leaves=s.n_leaves, ref_len=s.ref_len, k=k, m=m,
               form="leaves" if spec["leaves_only"] else "explicit", windows=info["n_windows"], distinct_kmers=info["n_kmers"],
               leaf_postings=info["n_leaf_postings"], output_postings=info["n_node_ids"], buckets=info["n_buckets"],
               device_ms=dict(hash=round(info["ms_hash"], 3), sort=round(info["ms_sort"], 3), group=round(info["ms_group"], 3),
                              d2h=round(info["ms_d2h"], 3)),
               device_phases_ms=round(info["ms_hash"] + info["ms_sort"] + info["ms_group"] + info["ms_d2h"], 3),
               host_expand_ms=round(info["ms_expand"], 3), call_ms=round(wall, 3), sort_passes=info["sort_passes"],
               full_key=info["full_key"], peak_device_bytes=info["peak_device_bytes"], generator_s=round(gen_s, 2), repeat=repeat)
    if spec["host"]:
        nw, msa = newick_and_msa(s)
        t = engine.Tree.from_newick(nw, "synth.nwk", 0.0)
        t0 = time.perf_counter()
        t.build_kmers_map(msa, k, m, reference_header_shift=False)
        rec["host_builder_s"] = round(time.perf_counter() - t0, 3)
        d = engine.Tree.from_newick(nw, "synth.nwk", 0.0)
        t0 = time.perf_counter()
        d.build_kmers_map_device(msa, k, m, reference_header_shift=False, device=device)  # MSA text -> map, FASTA stage included
        rec["device_use_case_s"] = round(time.perf_counter() - t0, 3)
        a, b = t.flat(), d.flat()
        rec["host_equal"] = all(np.array_equal(getattr(a, f), getattr(b, f))
                                for f in ("bucket_key", "bucket_kmer_off", "kmer_hash", "kmer_node_off", "node_ids"))
    s.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,G35,C3L")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    assert engine.device_count() > 0, "build_probe needs a GPU"
    # code objects and allocator warm before the first timed build
    w = SynthDb(50, 200, 12, 4, threads=THREADS)
    engine.build_kmers(w.flat.nodes, *records(w), 12, 4, device=a.device)
    for label in a.configs.split(","):
        print(json.dumps(probe(label, PROBES[label], a.repeat if label != "C5" else 1, a.device)), flush=True)


if __name__ == "__main__":
    main()
