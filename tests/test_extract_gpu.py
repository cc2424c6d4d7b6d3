"""Read extraction on the device: the selection kernel, the span step, plan + gather and the file-level entries through
the C-ABI against cls_select_host / cls_extract_host and tests/extract_ref.py; the cls-place extract options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from tests import extract_ref as er
from tests import tally_ref as tr
from tests.test_cli_e2e import CLI, write_db_json
from tests.test_extract_host import TREE_NAMES, complement, crafted_records, selections, selectors, texts
from tests.test_pair_gpu import fastq_texts
from tests.test_pair_host import TREES, simulated_pairs
from tests.test_tally_gpu import upload

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 511, 513)


def device_select(selector, recs, shift=0, stream=0):
    """cls_select_records_device on torch-owned buffers -> sel.  `shift` = 1: the records start 8 bytes into a 16-byte slot.
    d_sel is pre-filled with 0xFF and checked to be written for exactly n bytes."""
    import torch

    n = len(recs)
    t, p = upload(recs, shift=shift)
    d_sel = torch.full((n + 48,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    selector.select_device(p, n, d_sel.data_ptr() + 16, stream)
    torch.cuda.synchronize()
    raw = d_sel.cpu().numpy()
    assert (raw[:16] == 0xFF).all() and (raw[16 + n:] == 0xFF).all(), "bytes outside sel[0, n) were written"
    del t
    return raw[16:16 + n].copy()


@pytest.mark.parametrize("tree", TREE_NAMES)
def test_selection_kernel_equals_host(tree):
    import torch

    s = TREES[tree]()
    nodes = s.flat.nodes
    recs = crafted_records(nodes)
    with engine.PlacementDb(s.flat, device=0) as db:
        sels = selectors(nodes)
        made = {}
        for what, (inc, exc, flags) in sels.items():  # all of them alive at once on one handle
            made[what] = engine.Selector(db, inc, exc, flags=flags)
        try:
            for i, (what, (inc, exc, flags)) in enumerate(sels.items()):
                want = engine.select_host(s.flat, recs, inc, exc, flags=flags)
                assert np.array_equal(device_select(made[what], recs, shift=i % 2), want), f"{tree}, {what}"
                assert np.array_equal(made[what].select(recs), want), f"{tree}, {what}: cls_select_records"
                cinc, cexc, cflags = complement(nodes, inc, exc, flags)
                with engine.Selector(db, cinc, cexc, flags=cflags) as other:
                    assert np.array_equal(device_select(other, recs) + want, np.ones(len(recs), np.uint8)), f"{tree}, {what}: complement"
            sel = made["X, not Y, but Z"]
            inc, exc, flags = sels["X, not Y, but Z"]
            assert np.array_equal(device_select(sel, recs[:3000]), er.select_ref(nodes, recs[:3000], inc, exc, flags)), "against the Python statement"
            for n in SIZES:
                for shift in (0, 1):
                    want = engine.select_host(s.flat, recs[:n], inc, exc, flags=flags)
                    assert np.array_equal(device_select(sel, recs[:n], shift), want), f"n = {n}, shift {shift}"
            assert len(sel.select(recs[:0])) == 0
            # refusals: null arguments, a misaligned record pointer
            t, p = upload(recs[:64])
            out = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
            for args in ((0, 64, out.data_ptr()), (p, 64, 0), (p + 4, 8, out.data_ptr())):
                with pytest.raises(engine.ClsError) as e:
                    sel.select_device(*args)
                assert e.value.code == -1, args
            assert engine.lib().cls_select_records_device(None, p, 64, out.data_ptr(), None) == -1
            del t
        finally:
            for x in made.values():
                x.close()
        # selector validation on the device path
        root = int(nodes["id"][0])
        ids = set(int(x) for x in nodes["id"])
        unknown = max(ids) + 1
        for inc, exc, flags in (([root, root], [], 0), ([root], [root], 0), ([unknown], [], 0), ([root], [], 2)):
            with pytest.raises(engine.ClsError) as e:
                engine.Selector(db, inc, exc, flags=flags)
            assert e.value.code == -1


def to_device(arr):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy() if len(arr) else np.zeros(0, np.uint8)).to("cuda:0")
    if t.numel() == 0:
        t = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    return t


def test_spans_equal_reference():
    import torch

    for name, text in texts().items():
        n = len(engine.fastq_parse(text)[0])
        d_text = to_device(np.frombuffer(text, np.uint8))
        for shift in (0, 3):  # the text at a 16-byte aligned address and at an odd one
            if shift:
                buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda:0")
                buf[shift:shift + len(text)] = d_text[:len(text)]
                ptr = buf.data_ptr() + shift
            else:
                ptr = d_text.data_ptr()
            d_off = torch.full((8 * (n + 1) + 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            engine.fastq_spans_device(ptr, len(text), n, d_off.data_ptr())
            torch.cuda.synchronize()
            raw = d_off.cpu().numpy()
            assert (raw[8 * (n + 1):] == 0xFF).all()
            assert np.array_equal(raw[:8 * (n + 1)].view(np.uint64), er.spans_ref(text, n)), f"{name}, shift {shift}"


# ---- plan + gather on synthetic spans -------------------------------------------------------------------------------

LENGTHS = (0, 1, 7, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)


def synthetic(final_newline, seed=5):
    """-> (text, rec_off): every length of LENGTHS starting on every residue mod 16 (a filler item in front of each sets
    the residue; 4097 on four residues), one item of 70 001 bytes, random bytes, half of the items end in a newline."""
    rng = np.random.default_rng(seed)
    lens = []
    pos = 0
    for L in LENGTHS + (70001,):
        for r in range(16):
            if (L == 4097 and r % 4) or (L == 70001 and r != 5):
                continue
            fill = (r - pos) % 16
            lens += [fill, L]
            pos += fill + L
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    text = rng.integers(32, 127, int(off[-1])).astype(np.uint8)
    for i in range(len(lens)):
        if lens[i] and rng.random() < 0.5:
            text[int(off[i + 1]) - 1] = 10
    if len(lens) % 2:
        raise AssertionError("an even number of records is needed for stride 2")
    text[-1] = 10 if final_newline else ord("x")
    starts = off[:-1][np.array(lens) > 0]
    assert set(int(x) % 16 for x in starts) == set(range(16))
    return text.tobytes(), off


def gather_ref(text, off, sel, stride):
    parts, out_off = [], [0]
    for i in range(len(sel)):
        piece = text[int(off[i * stride]):int(off[(i + 1) * stride])] if sel[i] else b""
        if piece and not piece.endswith(b"\n"):
            piece += b"\n"
        parts.append(piece)
        out_off.append(out_off[-1] + len(piece))
    return b"".join(parts), np.array(out_off, dtype=np.uint64)


@pytest.mark.parametrize("final_newline", [True, False])
def test_plan_and_gather_on_synthetic_spans(final_newline):
    import torch

    text, off = synthetic(final_newline)
    n_rec = len(off) - 1
    d_text = to_device(np.frombuffer(text, np.uint8))
    d_off = to_device(off)
    guard = 64
    for stride in (1, 2):
        n_items = n_rec // stride
        for what, sel in selections(n_items, seed=stride).items():
            want, want_off = gather_ref(text, off, sel, stride)
            d_sel = to_device(sel)
            d_out_off = torch.full((8 * (n_items + 1) + 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            tot = engine.extract_plan_device(d_text.data_ptr(), d_off.data_ptr(), stride, n_items, d_sel.data_ptr(), d_out_off.data_ptr())
            torch.cuda.synchronize()
            raw = d_out_off.cpu().numpy()
            assert (raw[8 * (n_items + 1):] == 0xFF).all()
            assert np.array_equal(raw[:8 * (n_items + 1)].view(np.uint64), want_off), f"stride {stride}, {what}: d_out_off"
            er.assert_totals(tot, {"n_records": n_items, "n_selected": int(sel.sum()), "n_selected_unplaced": 0, "bytes_out": len(want)},
                             f"stride {stride}, {what}")
            for shift in (0, 1):  # the output at a 16-byte aligned address and at an odd one
                d_out = torch.full((len(want) + 2 * guard + 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
                assert d_out.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                engine.extract_gather_device(d_text.data_ptr(), d_off.data_ptr(), stride, n_items, d_sel.data_ptr(), d_out_off.data_ptr(),
                                             d_out.data_ptr() + guard + shift)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                lo = guard + shift
                assert (got[:lo] == 0xFF).all() and (got[lo + len(want):] == 0xFF).all(), f"stride {stride}, {what}, shift {shift}: guard bytes"
                assert got[lo:lo + len(want)].tobytes() == want, f"stride {stride}, {what}, shift {shift}"
    # refusals
    tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
    L = engine.lib()
    assert L.cls_extract_plan_device(d_text.data_ptr(), d_off.data_ptr(), 3, 4, d_text.data_ptr(), d_off.data_ptr(), tot.ctypes.data, None) == -1
    assert L.cls_extract_plan_device(d_text.data_ptr(), d_off.data_ptr(), 1, 4, d_text.data_ptr(), None, tot.ctypes.data, None) == -1
    assert L.cls_extract_gather_device(d_text.data_ptr(), d_off.data_ptr(), 1, 4, d_text.data_ptr(), d_off.data_ptr(), None, None) == -1


# ---- the file-level entries ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reads():
    s = SynthDb(64, 3000, 12, 4)
    r1, r2 = simulated_pairs(s, 600, seed=21)
    t1, t2, both, recs1, recs2 = fastq_texts(r1, r2)
    return s, t1, t2, both, recs1, recs2


def file_selectors(nodes):
    sels = selectors(nodes)
    x, y = sels["X, not Y, but Z"], sels["exclude only"]
    return {"a root child": (y[1], [], 0), "X, not Y, but Z, and the unplaced": (x[0], x[1], 1), "outside a root child": sels["outside a root child"]}


@pytest.mark.parametrize("trim", [(0, 0), (15, 25)])
def test_extract_fastq_text(reads, trim):
    s, t1, t2, both, recs1, _ = reads
    c5, c3 = trim
    nodes = s.flat.nodes
    crlf = t1[:30000].replace(b"\n", b"\r\n")
    crlf = crlf[:crlf.rindex(b"@p")]
    truncated = b"".join(recs1[:40]) + b"@broken\nACGT\n-\nIIII\n" + b"".join(recs1[40:60])
    cases = {"the reads": (t1, 600, False), "CRLF": (crlf, None, False), "truncated": (truncated, 40, True), "empty": (b"", 0, False),
             "no final newline": (t1[:-1], 600, False)}
    with engine.PlacementDb(s.flat, device=0) as db, engine.Tally(db) as tally:
        for what, (inc, exc, flags) in file_selectors(nodes).items():
            with engine.Selector(db, inc, exc, flags=flags) as sel:
                for name, (text, n_want, trunc_want) in cases.items():
                    _, recs, trunc = db.place_fastq_text(text, None, c5, c3)
                    pick = engine.select_host(s.flat, recs, inc, exc, flags=flags)
                    want, wtot = engine.extract_host(text, pick)
                    tally.reset()
                    out, tot, n, tr_ = db.extract_fastq_text(sel, text, tally if name != "CRLF" else None, None, c5, c3)
                    assert (n, tr_) == (len(recs), trunc) and trunc == trunc_want and (n_want is None or n == n_want), (what, name)
                    assert out == want, f"{what}, {name}, trim {trim}"
                    assert out == er.extract_ref(text, er.select_ref(nodes, recs, inc, exc, flags))[0], f"{what}, {name}: the Python statement"
                    n_unpl = int((pick.astype(bool) & ~er.placed_ref(nodes, recs)).sum())
                    er.assert_totals(tot, {"n_records": n, "n_selected": int(pick.sum()), "n_selected_unplaced": n_unpl, "bytes_out": len(want)},
                                     f"{what}, {name}")
                    if name != "CRLF":
                        tr.assert_tally_equal(tally.read(), engine.tally_host(s.flat, recs), f"{what}, {name}: the tally of the same pass")
                    if name == "the reads" and what == "a root child" and trim == (0, 0):
                        assert 0.05 * n < pick.sum() < 0.95 * n, "the root-child selector picks a trivial share"
                        tally.reset()
                        assert db.tally_fastq_text(tally, text, None, c5, c3) == (600, False)
                        tr.assert_tally_equal(tally.read(), engine.tally_host(s.flat, recs), "cls_tally_fastq_text")
        if trim == (0, 0):
            inc, exc, flags = file_selectors(nodes)["a root child"]
            with engine.PlacementDb(s.flat, device=0) as db2, engine.Selector(db2, inc, exc) as sel2:  # a selector of another handle
                with pytest.raises(engine.ClsError) as e:
                    db.extract_fastq_text(sel2, t1)
                assert e.value.code == -1


@pytest.mark.parametrize("trim", [(0, 0), (15, 25)])
def test_extract_fastq_pairs_text(reads, trim):
    s, t1, t2, both, recs1, recs2 = reads
    c5, c3 = trim
    nodes = s.flat.nodes
    with engine.PlacementDb(s.flat, device=0) as db, engine.Pairer(db) as p, engine.Tally(db) as tally:
        _, a, _ = db.place_fastq_text(t1, None, c5, c3)
        _, b, _ = db.place_fastq_text(t2, None, c5, c3)
        for pflags in (0, 3):
            P = engine.pair_host(s.flat, a, b, pflags)[0]
            for what, (inc, exc, flags) in file_selectors(nodes).items():
                pick = engine.select_host(s.flat, P, inc, exc, flags=flags)
                if what == "a root child" and trim == (0, 0) and pflags == 0:
                    assert 0.05 * 600 < pick.sum() < 0.95 * 600, "the root-child selector picks a trivial share"
                w1, w2, wi = engine.extract_host(t1, pick)[0], engine.extract_host(t2, pick)[0], engine.extract_host(both, pick, 2)[0]
                assert w1 == b"".join(recs1[i] for i in np.nonzero(pick)[0]) and w2 == b"".join(recs2[i] for i in np.nonzero(pick)[0])
                n_unpl = int((pick.astype(bool) & ~er.placed_ref(nodes, P)).sum())
                with engine.Selector(db, inc, exc, flags=flags) as sel:
                    tally.reset()
                    o1, o2, tot, n, trunc = db.extract_fastq_pairs_text(p, sel, t1, t2, tally, None, c5, c3, pflags)
                    assert (o1, o2, n, trunc) == (w1, w2, 600, False), f"two texts, {what}, trim {trim}, flags {pflags}"
                    er.assert_totals(tot, {"n_records": 600, "n_selected": int(pick.sum()), "n_selected_unplaced": n_unpl,
                                           "bytes_out": len(w1) + len(w2)}, f"two texts, {what}")
                    tr.assert_tally_equal(tally.read(), engine.tally_host(s.flat, P), f"tally of the pairs, {what}, flags {pflags}")
                    o1, o2, tot, n, trunc = db.extract_fastq_pairs_text(p, sel, both, None, None, None, c5, c3, pflags)
                    assert (o1, o2, n, trunc) == (wi, None, 600, False), f"interleaved, {what}, trim {trim}, flags {pflags}"
                    er.assert_totals(tot, {"n_records": 600, "n_selected": int(pick.sum()), "n_selected_unplaced": n_unpl, "bytes_out": len(wi)},
                                     f"interleaved, {what}")
        if trim == (0, 0):
            inc, exc, flags = file_selectors(nodes)["a root child"]
            with engine.Selector(db, inc, exc) as sel:
                assert db.extract_fastq_pairs_text(p, sel, b"", b"")[:2] == (b"", b"")
                assert db.extract_fastq_pairs_text(p, sel, b"")[:2] == (b"", None)
                # refusals leave no output
                swapped = list(recs2)
                swapped[137], swapped[138] = swapped[138], swapped[137]
                for x, y in ((t1, b"".join(swapped)), (t1, b"".join(recs2[:-1])), (both + recs1[0], None)):
                    o1, l1, o2, l2 = C.c_void_p(), C.c_size_t(7), C.c_void_p(), C.c_size_t(7)
                    tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
                    rc = engine.lib().cls_extract_fastq_pairs_text(db._h, p._h, sel._h, None, x, len(x), y, len(y) if y is not None else 0, None, None, 0,
                                                                   C.byref(o1), C.byref(l1), C.byref(o2), C.byref(l2), tot.ctypes.data, None, None)
                    assert rc == _abi.E_BAD_PAIRS and not o1.value and not o2.value and l1.value == 0 and l2.value == 0
                with pytest.raises(engine.ClsError) as e:
                    db.extract_fastq_pairs_text(p, sel, t1, t2, flags=4)
                assert e.value.code == -1
                with engine.PlacementDb(s.flat, device=0) as db2, engine.Pairer(db2) as p2, engine.Selector(db2, inc, exc) as sel2:
                    for pp, ss in ((p2, sel), (p, sel2)):  # a pairer / a selector of another handle
                        with pytest.raises(engine.ClsError) as e:
                            db.extract_fastq_pairs_text(pp, ss, t1, t2)
                        assert e.value.code == -1


# ---- cls-place ----------------------------------------------------------------------------------------------------------

def test_cli_extract_options(reads, tmp_path):
    s, t1, t2, both, _, _ = reads
    db_json = str(tmp_path / "db.json")
    write_db_json(s.flat, db_json)
    tree = engine.Tree(db_json)
    flat = tree.flat()
    nodes = flat.nodes
    q1, q2, qi = str(tmp_path / "R1.fastq"), str(tmp_path / "R2.fastq"), str(tmp_path / "inter.fastq")
    for path, text in ((q1, t1), (q2, t2), (qi, both)):
        open(path, "wb").write(text)

    def run(*args, code=0):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == code, (args, r.stderr)
        return r

    inc, exc, flags = file_selectors(nodes)["X, not Y, but Z, and the unplaced"]
    ids = lambda v: ",".join(str(x) for x in v)
    sel_args = ["--extract-clade", ids(inc), "--extract-exclude", ids(exc), "--extract-unplaced"]
    base = ["-d", db_json, "--query-format", "fastq", "-q", "20"]
    d = tmp_path
    with engine.PlacementDb(flat, device=0) as db, engine.Pairer(db) as p, engine.Selector(db, inc, exc, flags=flags) as sel:
        want1 = db.extract_fastq_text(sel, t1, None, None, 0, 20)[0]
        wp1, wp2 = db.extract_fastq_pairs_text(p, sel, t1, t2, None, None, 0, 20, 3)[:2]
        wi = db.extract_fastq_pairs_text(p, sel, both, None, None, None, 0, 20, 3)[0]
        _, a, _ = db.place_fastq_text(t1, None, 0, 20)
        assert 0 < len(want1) < len(t1) and 0 < len(wp1) < len(t1)
        # several pieces through the use-case's parameter: byte-equal to the one-piece run
        for piece_bytes, stem in ((0, "whole.fq"), (20000, "pieces.fq")):
            tot, n, _ = engine.extract_reads(db, tree, q1, str(d / stem), include=inc, exclude=exc, unplaced=bool(flags), trim_quality=20,
                                             piece_bytes=piece_bytes)
            assert n == 600 and open(d / stem, "rb").read() == want1 and int(tot["bytes_out"]) == len(want1), stem
        assert len(engine.fastq_split(t1, (len(t1) + 19999) // 20000)) > 3
    run(q1, *base, "--extract-out", str(d / "alone.fq"), *sel_args)
    run(q1, *base, "--extract-out", str(d / "rep.fq"), "--report-only", str(d / "rep.tsv"), *sel_args)
    run(q1, *base, "--report-only", str(d / "plain.tsv"))
    pair = ["--pair-mode", "conservative", "--pair-require-both"]
    run(q1, "-2", q2, *base, "--extract-out", str(d / "p1.fq"), "--extract-out2", str(d / "p2.fq"), "--pair-summary", str(d / "p.sum"), *pair, *sel_args)
    run(qi, "--interleaved", *base, "--extract-out", str(d / "pi.fq"), "--report", str(d / "pi.tsv"), *pair, *sel_args)
    run(qi, "--interleaved", *base, "--report-only", str(d / "pi_plain.tsv"), *pair)
    assert open(d / "alone.fq", "rb").read() == want1 and open(d / "rep.fq", "rb").read() == want1
    assert open(d / "rep.tsv", "rb").read() == open(d / "plain.tsv", "rb").read() == tree.report(*engine.tally_host(flat, a))
    assert open(d / "p1.fq", "rb").read() == wp1 and open(d / "p2.fq", "rb").read() == wp2 and open(d / "pi.fq", "rb").read() == wi
    assert open(d / "pi.tsv", "rb").read() == open(d / "pi_plain.tsv", "rb").read()
    assert open(d / "p.sum").read().startswith("n_pairs\t600\n")
    # an existing file needs -f
    assert run(q1, *base, "--extract-out", str(d / "alone.fq"), *sel_args, code=1).stderr
    run(q1, *base, "--extract-out", str(d / "alone.fq"), *sel_args, "-f")
    # refused combinations exit 2
    out = str(d / "x.fq")
    fa = str(d / "q.fasta")
    open(fa, "wb").write(b">a\nACGTACGTACGTACGT\n")
    for args in ((fa, "-d", db_json, "--extract-out", out, *sel_args),
                 (q1, *base, "--extract-out", out, "--device", "0,0", *sel_args),
                 (q1, *base, "--extract-out", out, "-o", str(d / "y.out"), *sel_args),
                 (q1, *base, "--extract-out", out, "--extract-out2", str(d / "x2.fq"), *sel_args),
                 (q1, "-2", q2, *base, "--extract-out", out, *sel_args),
                 (q1, *base, "-o", str(d / "y.out"), "--extract-clade", ids(inc)),
                 (q1, *base, "-o", str(d / "y.out"), "--extract-unplaced"),
                 (q1, *base, "--report-only", str(d / "y.tsv"), "--extract-exclude", ids(exc)),
                 (q1, *base, "--extract-out", out, "--extract-clade", "12x"),
                 (q1, *base, "--extract-out", out, "--extract-clade", "1,,2"),
                 (q1, *base, "--extract-out", out, "--extract-exclude", "-3")):
        assert run(*args, code=2).stderr, args
    assert not os.path.exists(out)
    # an id that is no clade of the tree: exit 1 with the library's message
    unknown = max(int(x) for x in nodes["id"]) + 1
    r = run(q1, *base, "--extract-out", out, "--extract-clade", str(unknown), code=1)
    assert "is no clade id of the tree" in r.stderr
    # a run without extract options writes what it wrote before
    h1 = [x[1:x.index(b"\n")] for x in reads[4]]
    run(q1, *base, "-o", str(d / "single.out"))
    assert open(d / "single.yaml", "rb").read() == tree.serialize(h1, a)[0]
    assert open(d / "single.error", "rb").read() == tree.serialize(h1, a)[1]
