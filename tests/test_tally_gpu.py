"""Clade tally on the device: cls_tally_add_device / cls_tally_read against cls_tally_host (and tests/tally_ref.py) on
placement records and on crafted, skewed batches; accumulation over calls and streams; the file-level entries, the
piece-wise profile use-case and the cls-place report options."""
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from tests import tally_ref as tr
from tests.helpers import PARAM_SETS, device_place
from tests.test_cli_e2e import CLI, write_db_json, write_fasta
from tests.test_tally_host import craft, crafted_records, shape

pytestmark = pytest.mark.gpu


def upload(recs, fill=0xFF, shift=0):
    """Records -> a torch byte buffer on cuda:0 pre-filled with `fill`; `shift` = 1: the records start 8 bytes into a
    16-byte slot.  -> (tensor kept alive, device pointer)."""
    import torch

    raw = np.full(len(recs) * 24 + 16, fill, dtype=np.uint8)
    raw[8 * shift:8 * shift + len(recs) * 24] = np.frombuffer(recs.tobytes(), dtype=np.uint8)
    t = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + 8 * shift


def device_tally(db, recs, **kw):
    with engine.Tally(db) as t:
        buf, ptr = upload(recs, **kw)
        t.add_device(ptr, len(recs))
        out = t.read()
        del buf
    return out


@pytest.mark.parametrize("name", ["k12", "k16_poly", "k12_long"])
def test_device_equals_host_on_placement_records(name):
    import torch

    s, bases, offsets = shape(name)
    n = len(offsets) - 1
    dev = torch.device("cuda:0")
    with engine.PlacementDb(s.flat, device=0) as db, engine.Tally(db) as t:
        if name == "k12_long":
            db.set_max_read_len(6000)
        d_b = torch.from_numpy(bases).to(dev)
        d_o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
        for kw in PARAM_SETS:
            d_out = torch.full((n * 24,), 0xFF, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            db.place_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), engine.make_params(**kw))
            t.reset()
            t.add_device(d_out.data_ptr(), n)  # (default stream: behind the placement)
            got = t.read()
            recs = d_out.cpu().numpy().view(_abi.PLACEMENT_DTYPE)
            assert (recs["status"] < 12).all()
            tr.assert_tally_equal(got, engine.tally_host(s.flat, recs), f"{name} {kw}")
            tr.assert_tally_equal(got, tr.tally_ref(s.flat.nodes, recs), f"{name} {kw} (numpy)")
            tr.check_invariants(s.flat.nodes, recs, *got)


def test_accumulation_streams_reset_and_two_tallies():
    import torch

    s, bases, offsets = shape("k12")
    with engine.PlacementDb(s.flat, device=0) as db:
        recs, _ = device_place(db, bases, offsets, want_stats=False)
        recs = np.concatenate([recs, crafted_records(s.flat.nodes)])
        n = len(recs)
        want = engine.tally_host(s.flat, recs)
        buf, ptr = upload(recs)
        side = torch.cuda.Stream()
        with engine.Tally(db) as t, engine.Tally(db) as other:
            for stream in (0, side.cuda_stream):
                for parts in (1, 2, 7):
                    t.reset()
                    cuts = [n * i // parts for i in range(parts + 1)]
                    for a, b in zip(cuts[:-1], cuts[1:]):
                        t.add_device(ptr + 24 * a, b - a, stream)  # (odd cuts: records that start mid-slot)
                    tr.assert_tally_equal(t.read(), want, f"{parts} adds on stream {stream}")
            # two streams at once into one tally
            t.reset()
            half = n // 2
            t.add_device(ptr, half, 0)
            t.add_device(ptr + 24 * half, n - half, side.cuda_stream)
            tr.assert_tally_equal(t.read(), want, "two streams")
            rows0, tot0 = other.read()
            assert int(tot0["n_reads"]) == 0 and not rows0["n_clade"].any()  # the second tally saw none of it
            t.add_device(ptr, n)  # accumulates on top
            rows2, tot2 = t.read()
            assert int(tot2["n_reads"]) == 2 * n and (rows2["n_clade"] == 2 * want[0]["n_clade"]).all()
            t.reset()
            t.add_device(ptr, 100)
            tr.assert_tally_equal(t.read(), engine.tally_host(s.flat, recs[:100]), "after reset")
            # host records through the same kernel
            other.add(recs)
            tr.assert_tally_equal(other.read(), want, "add (host records)")
            other.add(recs[:0])
            tr.assert_tally_equal(other.read(), want, "add of nothing")
        del buf


def test_skew_and_size():
    from classeq2_amd.synth import SynthDb

    flat = SynthDb(64, 3000, 16, 4, collapse_prob=0.4).flat
    nodes = flat.nodes
    rng = np.random.default_rng(5)
    N = 1 << 20
    leaf = int(nodes["id"][np.nonzero(nodes["kind"] == _abi.KIND_LEAF)[0][3]])
    one, rest = rng.integers(-100, 100, N), rng.integers(-3000, 10, N)
    ids = set(int(x) for x in nodes["id"])
    unknown = np.array([x for x in rng.integers(1, 1 << 62, 64, dtype=np.int64) if int(x) not in ids], dtype=np.uint64)
    cases = {
        "one leaf": craft(np.full(N, 4, np.uint8), leaf, one, rest, pad=0xFF),
        "the root": craft(np.full(N, 5, np.uint8), int(nodes["id"][0]), one, rest, pad=0xFF),
        "uniform": craft(rng.integers(0, 12, N).astype(np.uint8), nodes["id"][rng.integers(0, len(nodes), N)], one, rest, pad=0xFF),
    }
    st = rng.integers(4, 7, N).astype(np.uint8)
    cid = nodes["id"][rng.integers(0, len(nodes), N)].copy()
    bad = rng.random(N) < 0.01
    unk = rng.random(N) < 0.01
    st[bad] = rng.integers(12, 256, int(bad.sum())).astype(np.uint8)
    cid[unk] = unknown[rng.integers(0, len(unknown), int(unk.sum()))]
    cases["1 % unknown, 1 % bad"] = craft(st, cid, one, rest, pad=0xFF)
    with engine.PlacementDb(flat, device=0) as db:
        for what, recs in cases.items():
            got = device_tally(db, recs)
            tr.assert_tally_equal(got, engine.tally_host(flat, recs), what)
            tr.assert_tally_equal(got, tr.tally_ref(nodes, recs), what + " (numpy)")
            tr.check_invariants(nodes, recs, *got)
        small = cases["uniform"]
        for n in (0, 1, 63, 64, 65, 127, 128, 129, 511, 513):
            for shift in (0, 1):
                tr.assert_tally_equal(device_tally(db, small[:n], shift=shift), engine.tally_host(flat, small[:n]), f"n = {n}, shift {shift}")
        # the knob that takes the wave-level step out changes no result
        engine.set_tuning("tally_no_wave_combine", 1)
        try:
            tr.assert_tally_equal(device_tally(db, cases["one leaf"]), engine.tally_host(flat, cases["one leaf"]), "no wave combine")
        finally:
            engine.set_tuning("tally_no_wave_combine", 0)


def _texts(s, bases, offsets, n=600):
    raw = bytes(bases)
    rng = np.random.default_rng(2)
    fa, fq = [], []
    for i in range(n):
        seq = raw[int(offsets[i]):int(offsets[i + 1])]
        fa.append(b">r%d\n%s\n" % (i, seq))
        qual = bytes((rng.integers(2, 41, len(seq)) + 33).astype(np.uint8))
        fq.append(b"@r%d\n%s\n+\n%s\n" % (i, seq, qual))
    return b"".join(fa), b"".join(fq)


def test_file_level_entries():
    s, bases, offsets = shape("k12")
    fa, fq = _texts(s, bases, offsets)
    with engine.PlacementDb(s.flat, device=0) as db, engine.Tally(db) as t:
        for kw in (dict(), dict(min_match_coverage=0.0)):
            prm = engine.make_params(**kw)
            _, recs, trunc = db.place_fasta_text(fa, prm)
            t.reset()
            assert db.tally_fasta_text(t, fa, prm) == (len(recs), trunc) and not trunc
            tr.assert_tally_equal(t.read(), engine.tally_host(s.flat, recs), f"fasta {kw}")
            for c5, c3 in ((0, 0), (0, 20), (15, 25)):
                _, recs, trunc = db.place_fastq_text(fq, prm, c5, c3)
                t.reset()
                assert db.tally_fastq_text(t, fq, prm, c5, c3) == (len(recs), trunc)
                tr.assert_tally_equal(t.read(), engine.tally_host(s.flat, recs), f"fastq {c5},{c3} {kw}")
        # texts that stop early
        at = fa.index(b"\n>", 3000) + 1
        cut_fa = fa[:at] + b">\nACGT\n" + fa[at:]  # a record without a header text in the middle
        cut_fq = fq[:len(fq) // 2].rsplit(b"\n@", 1)[0] + b"\n@broken\nACGT\n+\nII\n" + fq[len(fq) // 2:]
        for text, fastq in ((cut_fa, False), (cut_fq, True)):
            _, recs, trunc = db.place_fastq_text(text) if fastq else db.place_fasta_text(text)
            t.reset()
            got = db.tally_fastq_text(t, text) if fastq else db.tally_fasta_text(t, text)
            assert got == (len(recs), trunc)
            if fastq:
                assert trunc and 0 < len(recs) < 600
            tr.assert_tally_equal(t.read(), engine.tally_host(s.flat, recs), "early stop")
        # a tally of another handle is refused
        with engine.PlacementDb(s.flat, device=0) as db2, engine.Tally(db2) as t2:
            with pytest.raises(engine.ClsError):
                db.tally_fasta_text(t2, fa)


def test_profile_sequences_pieces_and_group(tmp_path):
    s, bases, offsets = shape("k12")
    fa, fq = _texts(s, bases, offsets)
    db_json = str(tmp_path / "db.json")
    write_db_json(s.flat, db_json)
    tree = engine.Tree(db_json)
    flat = tree.flat()
    qa, qq = str(tmp_path / "q.fasta"), str(tmp_path / "q.fastq")
    open(qa, "wb").write(fa)
    open(qq, "wb").write(fq)
    broken = fq[:len(fq) // 2].rsplit(b"\n@", 1)[0] + b"\n@broken\nACGT\n+\nII\n" + fq[len(fq) // 2:]
    qb = str(tmp_path / "broken.fastq")
    open(qb, "wb").write(broken)
    with engine.PlacementDb(flat, device=0) as db, engine.PlacementDbGroup(flat, [0, 0, 0]) as grp:
        for path, text, fmt, trim in ((qa, fa, "fasta", None), (qq, fq, "fastq", 20), (qb, broken, "fastq", None)):
            piece = len(text) // 12  # (the text that stops early has no safe cut in its second half)
            split = engine.fastq_split if fmt == "fastq" else engine.fasta_split
            assert len(split(text, (len(text) + piece - 1) // piece)) - 1 >= 5
            if fmt == "fasta":
                _, recs, _ = db.place_fasta_text(text)
            else:
                _, recs, _ = db.place_fastq_text(text, None, 0, trim or 0)
            want = tree.report(*engine.tally_host(flat, recs))
            outs = {}
            for what, handle, pb in (("one piece", db, 1 << 40), ("pieces", db, piece), ("default", db, 0), ("group pieces", grp, piece),
                                     ("group one piece", grp, 1 << 40)):
                out = str(tmp_path / f"{os.path.basename(path)}.{what.replace(' ', '_')}.tsv")
                n, _ = engine.profile_sequences(handle, tree, path, out, query_format=fmt, trim_quality=trim, piece_bytes=pb)
                assert n == len(recs), (what, n, len(recs))
                outs[what] = open(out, "rb").read()
                assert outs[what] == want, (path, what)
            with pytest.raises(engine.ClsError):  # exists, no overwrite
                engine.profile_sequences(db, tree, path, out, query_format=fmt, trim_quality=trim)
            engine.profile_sequences(db, tree, path, out, query_format=fmt, trim_quality=trim, overwrite=True, all_rows=True)
            assert open(out, "rb").read() == tree.report(*engine.tally_host(flat, recs), all_rows=True)


def test_cli_report_options(tmp_path):
    s, bases, offsets = shape("k12")
    fa, fq = _texts(s, bases, offsets)
    db_json = str(tmp_path / "db.json")
    write_db_json(s.flat, db_json)
    tree = engine.Tree(db_json)
    flat = tree.flat()
    qa, qq = str(tmp_path / "q.fasta"), str(tmp_path / "q.fastq")
    open(qa, "wb").write(fa)
    open(qq, "wb").write(fq)

    def run(*args):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r

    with engine.PlacementDb(flat, device=0) as db:
        _, recs_a, _ = db.place_fasta_text(fa)
        _, recs_q, _ = db.place_fastq_text(fq, None, 0, 20)
    cases = (("fasta", [qa], recs_a, []), ("fastq", [qq, "--query-format", "fastq", "-q", "20"], recs_q, []),
             ("group", [qa], recs_a, ["--device", "0,0"]), ("all", [qa], recs_a, ["--report-all-clades"]))
    for what, q, recs, extra in cases:
        d = tmp_path / what
        d.mkdir()
        want = tree.report(*engine.tally_host(flat, recs), all_rows="--report-all-clades" in extra)
        run(*q, "-d", db_json, "-o", str(d / "res.out"), "--report", str(d / "with.tsv"), *extra)
        assert os.path.exists(d / "res.yaml") and os.path.exists(d / "res.error")
        before = sorted(os.listdir(d))
        run(*q, "-d", db_json, "--report-only", str(d / "only.tsv"), *extra)
        assert sorted(os.listdir(d)) == sorted(before + ["only.tsv"])  # no result, no .error file
        assert open(d / "with.tsv", "rb").read() == open(d / "only.tsv", "rb").read() == want, what
        # the per-read output is what a run without the report writes
        run(*q, "-d", db_json, "-o", str(d / "plain.out"), *extra)
        assert open(d / "plain.yaml", "rb").read() == open(d / "res.yaml", "rb").read()
    r = subprocess.run([CLI, qa, "-d", db_json, "--report", "a", "--report-only", "b", "-o", "c"], capture_output=True, text=True)
    assert r.returncode == 2
