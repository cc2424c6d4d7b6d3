"""Paired reads on the device: pair_records_kernel / pair_names_kernel through the C-ABI against cls_pair_host and
tests/pair_ref.py on crafted pairs (every size around the staging, both strides, records that start mid-slot), on a deep
tree and skewed batches; totals over calls and streams; the file-level entries, their refusals, and the cls-place pair
options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from tests import pair_ref as pr
from tests import tally_ref as tr
from tests.test_cli_e2e import CLI, write_db_json
from tests.test_pair_host import ALL_FLAGS, TREES, crafted_pairs, interleave, simulated_pairs
from tests.test_tally_gpu import upload
from tests.test_tally_host import craft

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 511, 513)


def device_pair(pairer, a, b=None, flags=0, shift_a=0, shift_b=0, shift_out=0, with_how=True, stream=0):
    """cls_pair_records_device on torch-owned buffers -> (P, how or None).  `b` None: `a` is interleaved (stride 2).
    `shift_*` = 1: that buffer's records start 8 bytes into a 16-byte slot.  The outputs are pre-filled with 0xFF and
    checked to be written over exactly n records / n bytes."""
    import torch

    stride = 2 if b is None else 1
    n = len(a) // 2 if b is None else len(a)
    ta, pa = upload(a, shift=shift_a)
    if b is None:
        tb, pb = ta, pa + 24
    else:
        tb, pb = upload(b, shift=shift_b)
    d_out = torch.full((n * 24 + 48,), 0xFF, dtype=torch.uint8, device="cuda:0")
    d_how = torch.full((n + 32,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    po = d_out.data_ptr() + 16 + 8 * shift_out
    assert d_out.data_ptr() % 16 == 0
    pairer.pair_device(pa, pb, stride, n, po, d_how.data_ptr() + 16 if with_how else 0, flags, stream)
    torch.cuda.synchronize()
    raw, hraw = d_out.cpu().numpy(), d_how.cpu().numpy()
    lo = 16 + 8 * shift_out
    assert (raw[:lo] == 0xFF).all() and (raw[lo + 24 * n:] == 0xFF).all(), "bytes outside the n records were written"
    if with_how:
        assert (hraw[:16] == 0xFF).all() and (hraw[16 + n:] == 0xFF).all(), "bytes outside how[0, n) were written"
    else:
        assert (hraw == 0xFF).all()
    del ta, tb
    return raw[lo:lo + 24 * n].copy().view(_abi.PLACEMENT_DTYPE), (hraw[16:16 + n].copy() if with_how else None)


@pytest.mark.parametrize("tree", ["k12", "k9_ids"])
def test_device_equals_host_on_crafted_pairs(tree):
    s = TREES[tree]()
    a, b = crafted_pairs(s.flat.nodes)
    both = interleave(a, b)
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p:
        for flags in ALL_FLAGS:
            want = engine.pair_host(s.flat, a, b, flags)
            pr.assert_pairs_equal(device_pair(p, a, b, flags), want, f"whole set, stride 1, flags {flags}")
            pr.assert_pairs_equal(device_pair(p, both, None, flags), want, f"whole set, stride 2, flags {flags}")
        for i, n in enumerate(SIZES):
            for shift in (0, 1):
                flags = ALL_FLAGS[(i + shift) % 4]
                want = engine.pair_host(s.flat, a[:n], b[:n], flags)
                for shift_b in (0, 1):
                    got = device_pair(p, a[:n], b[:n], flags, shift, shift_b, 1 - shift)
                    pr.assert_pairs_equal(got, want, f"n = {n}, stride 1, shifts {shift} {shift_b}, flags {flags}")
                for shift_out in (0, 1):
                    got = device_pair(p, both[:2 * n], None, flags, shift, 0, shift_out)
                    pr.assert_pairs_equal(got, want, f"n = {n}, stride 2, shifts {shift} {shift_out}, flags {flags}")
        # d_how = NULL
        want = engine.pair_host(s.flat, a[:513], b[:513])
        P, how = device_pair(p, a[:513], b[:513], with_how=False)
        pr.assert_pairs_equal((P, None), want, "d_how = NULL")
        # host records through the same kernel
        pr.assert_pairs_equal(p.pair(a, b, 3), engine.pair_host(s.flat, a, b, 3), "cls_pair_records, stride 1")
        pr.assert_pairs_equal(p.pair(both, None, 1), engine.pair_host(s.flat, a, b, 1), "cls_pair_records, stride 2")
        # refused: an unknown flag bit, a stride that is neither 1 nor 2, stride 2 with b elsewhere, d_out over an input
        before = p.totals()
        ta, pa = upload(a[:64])
        tb, pb = upload(b[:64])
        import torch

        out = torch.zeros(64 * 24, dtype=torch.uint8, device="cuda:0")
        for args in ((pa, pb, 1, 64, out.data_ptr(), 0, 4), (pa, pb, 3, 64, out.data_ptr(), 0, 0), (pa, pb, 2, 32, out.data_ptr(), 0, 0),
                     (pa, pb, 1, 64, pa + 24, 0, 0), (pa, pb, 1, 64, pb, 0, 0), (pa + 4, pb, 1, 8, out.data_ptr(), 0, 0)):
            with pytest.raises(engine.ClsError) as e:
                p.pair_device(*args)
            assert e.value.code == -1, args
        pr.assert_totals_equal(p.totals(), before, "a refused call counts nothing")


def test_deep_tree_and_skew():
    s = TREES["deep"]()
    nodes = s.flat.nodes
    t = pr.TreeIndex(nodes)
    assert max(t.depth) >= 300
    rng = np.random.default_rng(9)
    N = 1 << 18
    fc, nc = int(nodes[0]["first_child"]), int(nodes[0]["n_children"])
    top_of = {}
    for r in range(1, len(nodes)):
        top_of[r] = r if t.parent[r] == 0 else top_of[t.parent[r]]
    deepest = {}  # root child -> its deepest tip
    for r in range(1, len(nodes)):
        if nodes[r]["n_children"] == 0 and (top_of[r] not in deepest or t.depth[r] > t.depth[deepest[top_of[r]]]):
            deepest[top_of[r]] = r
    tips = sorted(deepest.values(), key=lambda r: -t.depth[r])[:2]
    assert nc >= 2 and len(tips) == 2 and t.depth[tips[0]] >= 300
    one, rest = rng.integers(-100, 100, (2, N)), rng.integers(-3000, 10, (2, N))
    leaf = int(nodes["id"][tips[0]])
    rid = lambda: nodes["id"][rng.integers(0, len(nodes), N)]
    cases = {
        "discordant between the deepest tips": (craft(np.full(N, 4, np.uint8), leaf, one[0], rest[0], 7, pad=0xFF),
                                                craft(np.full(N, 5, np.uint8), int(nodes["id"][tips[1]]), one[1], rest[1], 9, pad=0xFF)),
        "same, one leaf": (craft(rng.integers(4, 6, N).astype(np.uint8), leaf, rng.integers(-2, 2, N), rng.integers(-2, 2, N), 1, pad=0xFF),
                           craft(rng.integers(4, 6, N).astype(np.uint8), leaf, rng.integers(-2, 2, N), rng.integers(-2, 2, N), 2, pad=0xFF)),
        "uniform": (craft(rng.integers(0, 13, N).astype(np.uint8), rid(), one[0], rest[0], 3, pad=0xFF),
                    craft(rng.integers(0, 13, N).astype(np.uint8), rid(), one[1], rest[1], 4, pad=0xFF)),
        "uniform, clade-bearing": (craft(rng.integers(4, 7, N).astype(np.uint8), rid(), one[0], rest[0], 3, pad=0xFF),
                                   craft(rng.integers(4, 7, N).astype(np.uint8), rid(), one[1], rest[1], 4, pad=0xFF)),
    }
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p:
        for i, (what, (a, b)) in enumerate(cases.items()):
            flags = ALL_FLAGS[i % 4]
            want = engine.pair_host(s.flat, a, b, flags)
            p.totals(reset=True)
            if i % 2:
                got = device_pair(p, interleave(a, b), None, flags, 1, 0, 1)
            else:
                got = device_pair(p, a, b, flags, 0, 1, 0)
            pr.assert_pairs_equal(got, want, what)
            pr.assert_totals_equal(p.totals(), want[2], what)
            sub = slice(0, 3000)  # (the Python statement is slow: a part of each case)
            pr.assert_pairs_equal((got[0][sub], got[1][sub]), pr.pair_ref(nodes, a[sub], b[sub], flags, t)[:2], what + " (pair_ref)")
        a, b = cases["discordant between the deepest tips"]
        P, how, tot = engine.pair_host(s.flat, a[:10], b[:10])
        assert (how == _abi.PAIR_DISCORDANT).all() and (P["clade_id"] == nodes["id"][0]).all() and (P["levels"] == 0).all()


def test_totals_streams_reset_and_the_tally():
    import torch

    s = TREES["k12"]()
    a, b = crafted_pairs(s.flat.nodes, seed=4)
    n = len(a)
    want = engine.pair_host(s.flat, a, b)
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p, engine.Pairer(db) as other, engine.Tally(db) as tally:
        ta, pa = upload(a)
        tb, pb = upload(b)
        out = torch.full((n * 24,), 0xFF, dtype=torch.uint8, device="cuda:0")
        how = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()

        def run(lo, hi, stream):
            p.pair_device(pa + 24 * lo, pb + 24 * lo, 1, hi - lo, out.data_ptr() + 24 * lo, how.data_ptr() + lo, 0, stream)

        for stream in (0, side.cuda_stream):
            for parts in (1, 2, 7):
                assert int(p.totals(reset=True)["n_pairs"]) in (0, n)
                cuts = [n * i // parts for i in range(parts + 1)]
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    run(lo, hi, stream)  # (odd cuts: records that start mid-slot)
                pr.assert_totals_equal(p.totals(), want[2], f"{parts} calls on stream {stream}")
                torch.cuda.synchronize()
                pr.assert_pairs_equal((out.cpu().numpy().view(_abi.PLACEMENT_DTYPE), how.cpu().numpy()), want, f"{parts} calls on stream {stream}")
        # two streams at once
        p.totals(reset=True)
        half = n // 2
        run(0, half, 0)
        run(half, n, side.cuda_stream)
        pr.assert_totals_equal(p.totals(), want[2], "two streams")
        assert int(other.totals()["n_pairs"]) == 0 and not other.totals()["how_count"].any()  # the second pairer saw none of it
        run(0, n, 0)  # accumulates on top
        t2 = p.totals(reset=True)
        assert int(t2["n_pairs"]) == 2 * n and (t2["how_count"] == 2 * want[2]["how_count"]).all()
        assert int(p.totals()["n_pairs"]) == 0  # reset
        run(0, 100, 0)
        pr.assert_totals_equal(p.totals(), engine.pair_host(s.flat, a[:100], b[:100])[2], "after reset")
        # the tally on the same handle is what it was: P goes into it like any records
        torch.cuda.synchronize()
        run(0, n, 0)
        tally.add_device(out.data_ptr(), n)
        tr.assert_tally_equal(tally.read(), engine.tally_host(s.flat, want[0]), "tally of P")
        tr.assert_tally_equal(tally.read(), tr.tally_ref(s.flat.nodes, want[0]), "tally of P (numpy)")
        del ta, tb


# ---- the file-level entries ---------------------------------------------------------------------------------------------

def fastq_texts(r1, r2, seed=2):
    """-> (R1 text, R2 text, interleaved text); names "p<i>/1 <comment>" and "p<i>/2"."""
    rng = np.random.default_rng(seed)
    t1, t2 = [], []
    for i, (x, y) in enumerate(zip(r1, r2)):
        q1 = bytes((rng.integers(2, 41, len(x)) + 33).astype(np.uint8))
        q2 = bytes((rng.integers(2, 41, len(y)) + 33).astype(np.uint8))
        t1.append(b"@p%d/1 first mate\n%s\n+\n%s\n" % (i, x, q1))
        t2.append(b"@p%d/2\n%s\n+\n%s\n" % (i, y, q2))
    return b"".join(t1), b"".join(t2), b"".join(x + y for x, y in zip(t1, t2)), t1, t2


@pytest.fixture(scope="module")
def pair_texts():
    s = SynthDb(64, 3000, 12, 4)  # the tree of shape("k12")
    r1, r2 = simulated_pairs(s, 600, seed=21)
    return (s, *fastq_texts(r1, r2))


@pytest.mark.parametrize("trim", [(0, 0), (15, 25)])
def test_file_level_entries(pair_texts, trim):
    s, t1, t2, both, _, _ = pair_texts
    c5, c3 = trim
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p, engine.Tally(db) as tally:
        h1, a, tr1 = db.place_fastq_text(t1, None, c5, c3)
        h2, b, tr2 = db.place_fastq_text(t2, None, c5, c3)
        assert not tr1 and not tr2 and len(a) == len(b) == 600
        for flags in (0, 3):
            want = engine.pair_host(s.flat, a, b, flags)
            p.totals(reset=True)
            two = db.place_fastq_pairs_text(p, t1, t2, None, c5, c3, flags)
            one = db.place_fastq_pairs_text(p, both, None, None, c5, c3, flags)
            for what, (hdr, P, how, trunc) in (("two texts", two), ("interleaved", one)):
                assert hdr == h1 and not trunc, what
                pr.assert_pairs_equal((P, how), want, f"{what}, trim {trim}, flags {flags}")
            tot = p.totals(reset=True)
            assert int(tot["n_pairs"]) == 1200 and (tot["how_count"] == 2 * want[2]["how_count"]).all()
            for text2 in (t2, None):
                tally.reset()
                assert db.tally_fastq_pairs_text(p, tally, t1 if text2 else both, text2, None, c5, c3, flags) == (600, False)
                tr.assert_tally_equal(tally.read(), engine.tally_host(s.flat, want[0]), f"tally of the pairs, trim {trim}, flags {flags}")
            pr.assert_totals_equal(p.totals(), tot, "the tally entries count the classes too")
        if trim == (0, 0):
            how = engine.pair_host(s.flat, a, b)[1]
            assert len(set(int(x) for x in how)) >= 4  # the reads are worth pairing
            # no pairs at all
            hdr, P, how, trunc = db.place_fastq_pairs_text(p, b"", b"")
            assert hdr == [] and len(P) == 0 and len(how) == 0 and not trunc
            assert db.place_fastq_pairs_text(p, b"")[0] == []
            with engine.PlacementDb(s.flat, device=0) as db2, engine.Pairer(db2) as p2:  # a pairer of another handle
                with pytest.raises(engine.ClsError) as e:
                    db.place_fastq_pairs_text(p2, t1, t2)
                assert e.value.code == -1


def test_refusals(pair_texts):
    s, t1, t2, both, recs1, recs2 = pair_texts
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p:
        swapped = list(recs2)
        swapped[137], swapped[138] = swapped[138], swapped[137]
        inter_swapped = b"".join(x + y for x, y in zip(recs1, swapped))
        cases = {
            "two records of R2 swapped": (t1, b"".join(swapped)),
            "the same, interleaved": (inter_swapped, None),
            "R2 one record short": (t1, b"".join(recs2[:-1])),
            "an odd interleaved text": (both + recs1[0], None),
        }
        for what, (x, y) in cases.items():
            with pytest.raises(engine.ClsError) as e:
                db.place_fastq_pairs_text(p, x, y)
            assert e.value.code == _abi.E_BAD_PAIRS, (what, e.value)
            if "swapped" in what or "interleaved" in what and "odd" not in what:
                assert "pair 137" in e.value.msg and '"p137"' in e.value.msg and '"p138"' in e.value.msg, e.value.msg
        with pytest.raises(engine.ClsError) as e:
            db.place_fastq_pairs_text(p, t1, t2, flags=4)
        assert e.value.code == -1
        assert int(p.totals()["n_pairs"]) == 0
        # the handle still places a good pair set
        hdr, P, how, _ = db.place_fastq_pairs_text(p, t1, t2)
        _, a, _ = db.place_fastq_text(t1)
        _, b, _ = db.place_fastq_text(t2)
        pr.assert_pairs_equal((P, how), engine.pair_host(s.flat, a, b), "after the refusals")


def test_names_device():
    import torch

    n = 5000
    h1 = [b"read%d/1 c" % i for i in range(n)]
    h2 = [b"read%d/2" % i for i in range(n)]
    for bad in ((), (4999,), (70, 64, 3000), (0,)):
        g2 = list(h2)
        for j in bad:
            g2[j] = b"x" + g2[j]
        want = pr.pair_names_ref(h1, g2)
        assert engine.pair_names_host(h1, g2) == want
        for lists, stride in (((h1, g2), 1), (([h for pair in zip(h1, g2) for h in pair],) * 2, 2)):
            bufs = []
            for hs in lists:
                off = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
                bufs.append((torch.from_numpy(np.frombuffer(b"".join(hs), dtype=np.uint8).copy()).to("cuda:0"), torch.from_numpy(off).to("cuda:0")))
            torch.cuda.synchronize()
            n_bad, first = C.c_uint64(0), C.c_uint64(0)
            rc = engine.lib().cls_pair_names_device(bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), bufs[1][0].data_ptr(),
                                                    bufs[1][1].data_ptr() + (8 if stride == 2 else 0), stride, n, C.byref(n_bad), C.byref(first), None)
            assert rc == 0
            assert (n_bad.value, first.value if n_bad.value else None) == want, (bad, stride)


# ---- cls-place ----------------------------------------------------------------------------------------------------------

def test_cli_pair_options(pair_texts, tmp_path):
    s, t1, t2, both, _, _ = pair_texts
    db_json = str(tmp_path / "db.json")
    write_db_json(s.flat, db_json)
    tree = engine.Tree(db_json)
    flat = tree.flat()
    q1, q2, qi = str(tmp_path / "R1.fastq"), str(tmp_path / "R2.fastq"), str(tmp_path / "inter.fastq")
    for path, text in ((q1, t1), (q2, t2), (qi, both)):
        open(path, "wb").write(text)

    def run(*args, code=0):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == code, (args, r.stderr)
        return r

    with engine.PlacementDb(flat, device=0) as db:
        h1, a, _ = db.place_fastq_text(t1, None, 0, 20)
        _, b, _ = db.place_fastq_text(t2, None, 0, 20)
    base = ["-d", db_json, "--query-format", "fastq", "-q", "20"]
    for mode, flags in (([], 0), (["--pair-mode", "conservative", "--pair-require-both"], 3), (["--pair-mode", "deepest"], 0)):
        P, how, tot = engine.pair_host(flat, a, b, flags)
        want_yaml, want_err = tree.serialize(h1, P)
        want_report = tree.report(*engine.tally_host(flat, P))
        want_summary = "".join(f"{k}\t{v}\n" for k, v in [("n_pairs", int(tot["n_pairs"]))] + list(zip(_abi.PAIR_CLASS_NAMES, (int(x) for x in tot["how_count"]))))
        d = tmp_path / f"flags{flags}_{len(mode)}"
        d.mkdir()
        run(q1, "-2", q2, *base, "-o", str(d / "two.out"), "--report", str(d / "two.tsv"), "--pair-summary", str(d / "two.sum"), *mode)
        run(qi, "--interleaved", *base, "-o", str(d / "int.out"), "--report", str(d / "int.tsv"), "--pair-summary", str(d / "int.sum"), *mode)
        run(q1, "--mate-file", q2, *base, "--report-only", str(d / "only.tsv"), "--pair-summary", str(d / "only.sum"), *mode)
        for stem in ("two", "int"):
            assert open(d / f"{stem}.yaml", "rb").read() == want_yaml, stem
            assert open(d / f"{stem}.error", "rb").read() == want_err, stem
        for stem in ("two", "int", "only"):
            assert open(d / f"{stem}.tsv", "rb").read() == want_report, stem
            assert open(d / f"{stem}.sum").read() == want_summary, stem
        assert not os.path.exists(d / "only.yaml")
    # bad combinations exit 2
    out = str(tmp_path / "x.out")
    for args in ((q1, "-2", q2, "-d", db_json, "-o", out), (qi, "--interleaved", "-d", db_json, "-o", out),
                 (q1, "-2", q2, *base, "-o", out, "--device", "0,0"), (q1, "-2", q2, "--interleaved", *base, "-o", out),
                 (q1, *base, "-o", out, "--pair-summary", out), (q1, "-2", q2, *base, "-o", out, "--pair-mode", "shallow")):
        assert run(*args, code=2).stderr
    # mates that do not line up: exit 1 with the message
    open(q2, "wb").write(t2[:t2.rindex(b"@")])
    r = run(q1, "-2", q2, *base, "-o", out, "-f", code=1)
    assert "different numbers of records" in r.stderr
    # a run without pair options is the single-end run it always was
    run(q1, *base, "-o", str(tmp_path / "single.out"))
    assert open(tmp_path / "single.yaml", "rb").read() == tree.serialize(h1, a)[0]
    assert open(tmp_path / "single.error", "rb").read() == tree.serialize(h1, a)[1]
