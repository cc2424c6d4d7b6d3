"""Paired-read reconciliation on the C3 shape (10 k leaves, k = 12), 1 M pairs of 150 bp.  One JSON line; device times
are HIP events, one warm-up, then the median (and min..max) of `--runs`:
  * place_2n_ms: cls_place_batch_device on the 2 M reads of the pairs (R1's reads, then R2's), the step the pairing
    kernel follows;
  * pair_ms: pair_records_kernel (cls_pair_records_device) on the records of that step, stride 1 (R1 | R2) and stride 2
    (the same records interleaved), next to the floor: 73 bytes a pair over the HBM rate;
  * names_ms: pair_names_kernel (cls_pair_names_device) on 1 M header pairs "r<i>/1 <comment>" / "r<i>/2";
  * deep: a deep tree (the generator's `deep` option), every pair discordant between the deepest tips of two root
    subtrees -- the worst case of the LCA climb -- next to the placement of 2 M reads of that tree.
Half of the mate 2s are the reverse complement of their mate 1, half an independent read; `classes` gives the mix.
Fails without a GPU: the pairing has no host fallback.
usage: pair_probe.py [--pairs N] [--runs R] [--hbm-tb-s X] [--deep-leaves N] [--deep-depth D]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from classeq2_amd import _abi, engine  # noqa: E402
from classeq2_amd.synth import CONFIGS, SynthDb  # noqa: E402

COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def timed(fns, runs):
    """{name: fn} -> {name: [ms] * runs}, the variants alternated run by run, run 0 a warm-up."""
    out = {k: [] for k in fns}
    for run in range(runs + 1):
        for k, fn in fns.items():
            ms = event_ms(fn)
            if run:
                out[k].append(ms)
    return out


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=CONFIGS["C3"]["n_reads"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hbm-tb-s", type=float, default=8.0, help="HBM rate the floor is taken from (TB/s)")
    ap.add_argument("--deep-leaves", type=int, default=30000)
    ap.add_argument("--deep-depth", type=int, default=900)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pair_probe needs a GPU"
    cfg = CONFIGS["C3"]
    n, L = a.pairs, cfg["read_len"]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    res = {"config": "C3", "pairs": n, "read_len": L, "runs": a.runs,
           "kernels": ["pair_records_kernel<1>", "pair_records_kernel<2>", "pair_names_kernel"]}
    floor_ms = n * 73 / (a.hbm_tb_s * 1e12) * 1e3  # 48 bytes in, 24 + 1 out
    res["floor_ms"] = round(floor_ms, 5)

    def place_times(s, bases, offsets, key):
        """Times the placement of the 2 n reads -> its records."""
        with engine.PlacementDb(s.flat, device=0) as db:
            db.set_max_read_len(L + 10)
            d_b = torch.from_numpy(bases).to(dev)
            d_o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
            d_recs = torch.zeros(2 * n * 24, dtype=torch.uint8, device=dev)
            place = lambda: db.place_batch_device(d_b.data_ptr(), d_o.data_ptr(), 2 * n, d_recs.data_ptr())
            res[key + "place_2n_ms"] = stats(timed({"place": place}, a.runs)["place"])
            torch.cuda.synchronize()
            return d_recs.cpu().numpy().view(_abi.PLACEMENT_DTYPE).copy()

    def pair_times(s, recs, key):
        with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as pairer:
            d_recs = torch.from_numpy(recs.view(np.uint8)).to(dev)
            inter = np.empty(2 * n, dtype=_abi.PLACEMENT_DTYPE)
            inter[0::2], inter[1::2] = recs[:n], recs[n:]
            d_inter = torch.from_numpy(inter.view(np.uint8)).to(dev)
            d_P = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
            d_how = torch.zeros(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            fns = {
                "stride1": lambda: pairer.pair_device(d_recs.data_ptr(), d_recs.data_ptr() + 24 * n, 1, n, d_P.data_ptr(), d_how.data_ptr()),
                "stride2": lambda: pairer.pair_device(d_inter.data_ptr(), d_inter.data_ptr() + 24, 2, n, d_P.data_ptr(), d_how.data_ptr()),
            }
            t = timed(fns, a.runs)
            res[key + "pair_ms"] = {k: dict(stats(v), x_floor=round(statistics.median(v) / floor_ms, 1)) for k, v in t.items()}
            torch.cuda.synchronize()
            P = d_P.cpu().numpy().view(_abi.PLACEMENT_DTYPE)
            how = d_how.cpu().numpy()
            want = engine.pair_host(s.flat, recs[:n], recs[n:])
            assert (how == want[1]).all() and P.tobytes() == want[0].tobytes(), "device pairs differ from the host's"
            tot = pairer.totals()
            assert int(tot["n_pairs"]) == 2 * n * (a.runs + 1)
            res[key + "classes"] = dict(zip(_abi.PAIR_CLASS_NAMES, (int(x) for x in want[2]["how_count"])))

    # ---- C3: placement of the 2 M reads, the pairing kernel, the name kernel ---------------------------------------------
    s = SynthDb(cfg["n_leaves"], cfg["ref_len"], cfg["k_size"], cfg["m_size"])
    res["n_nodes"] = int(len(s.flat.nodes))
    b1, off1, _ = s.reads(n, L, seed=3)
    b2, _, _ = s.reads(n, L, seed=4)
    rows1, rows2 = b1.reshape(n, L), b2.reshape(n, L).copy()
    rows2[0::2] = COMP[rows1[0::2, ::-1]]  # every second mate 2: the reverse complement of its mate 1
    bases = np.concatenate([b1, rows2.reshape(-1)])
    offsets = (np.arange(2 * n + 1, dtype=np.uint64) * np.uint64(L))
    recs = place_times(s, bases, offsets, "")
    pair_times(s, recs, "")
    res["pair_over_place"] = round(res["pair_ms"]["stride1"]["median"] / res["place_2n_ms"]["median"], 5)

    h1 = [b"r%d/1 1:N:0:ACGT" % i for i in range(n)]
    h2 = [b"r%d/2" % i for i in range(n)]
    bufs = []
    for hs in (h1, h2):
        off = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
        bufs.append((torch.from_numpy(np.frombuffer(b"".join(hs), dtype=np.uint8).copy()).to(dev), torch.from_numpy(off).to(dev)))
    res["header_bytes"] = int(bufs[0][0].numel() + bufs[1][0].numel())
    torch.cuda.synchronize()
    n_bad, first = C.c_uint64(0), C.c_uint64(0)

    def names():
        rc = engine.lib().cls_pair_names_device(bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), 1, n,
                                                C.byref(n_bad), C.byref(first), None)
        assert rc == 0 and n_bad.value == 0

    res["names_ms"] = stats(timed({"names": names}, a.runs)["names"])  # (includes the call's own small copies and its wait)
    del bufs
    s.close()

    # ---- a deep tree: every pair discordant between the deepest tips of two root subtrees -------------------------------
    sd = SynthDb(a.deep_leaves, 300, cfg["k_size"], cfg["m_size"], deep=1, max_depth=a.deep_depth, tips_only=True)
    nodes = sd.flat.nodes
    depth = np.zeros(len(nodes), dtype=np.int64)
    top = np.zeros(len(nodes), dtype=np.int64)
    for r in range(len(nodes)):
        fc, nc = int(nodes[r]["first_child"]), int(nodes[r]["n_children"])
        depth[fc:fc + nc] = depth[r] + 1
        top[fc:fc + nc] = np.arange(fc, fc + nc) if r == 0 else top[r]
    tips = sorted((int(np.nonzero(top == t)[0][np.argmax(depth[top == t])]) for t in np.unique(top[1:])), key=lambda r: -depth[r])[:2]
    res["deep"] = {"n_nodes": int(len(nodes)), "max_depth": int(depth.max()), "tip_depths": [int(depth[t]) for t in tips]}
    bd, offd, _ = sd.reads(2 * n, L, seed=5)
    key = "deep_"
    place_times(sd, bd, offd, key)
    worst = np.zeros(2 * n, dtype=_abi.PLACEMENT_DTYPE)
    worst["status"] = _abi.IDENTITY_FOUND
    worst["clade_id"][:n], worst["clade_id"][n:] = nodes["id"][tips[0]], nodes["id"][tips[1]]
    pair_times(sd, worst, key)
    for k in ("place_2n_ms", "pair_ms", "classes"):
        res["deep"][k] = res.pop(key + k)
    res["deep"]["pair_over_place"] = round(res["deep"]["pair_ms"]["stride1"]["median"] / res["deep"]["place_2n_ms"]["median"], 5)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
