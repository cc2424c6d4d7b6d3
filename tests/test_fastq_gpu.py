"""FASTQ stage on the device (cls_fastq_scan_device and what is built on it): byte for byte the host parse
(cls_fastq_parse, itself checked against the rules in tests/test_fastq_host.py) on the fixed and random cases, on a
text of many chunks and on 10 kb reads; placement of the trimmed reads equal to the oracle's; and `cls-place
--query-format fastq -q` equal to `cls-place` on the FASTA of the host-trimmed reads."""
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests.helpers import records_equal
from tests.test_cli_e2e import CLI, write_db_json, write_fasta
from tests.test_fastq_host import FASTQ_CASES, OPTS, random_fastq
from tests.test_golden import _load

pytestmark = pytest.mark.gpu


def _same(txt: bytes, c5=0, c3=0):
    want = engine.fastq_parse(txt, trim_5p=c5, trim_3p=c3)
    got = engine.fastq_parse(txt, device=0, trim_5p=c5, trim_3p=c3)
    assert got[0] == want[0], (txt[:80], c5, c3)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), (txt[:80], c5, c3)
    assert got[3] == want[3], (txt[:80], c5, c3)
    return want


@pytest.mark.parametrize("txt", FASTQ_CASES)
def test_fixed_cases(txt):
    for c5, c3 in OPTS:
        _same(txt, c5, c3)


def test_random_texts():
    rng = np.random.default_rng(21)
    n_trunc = 0
    for trial in range(300):
        txt = random_fastq(rng, bad=0.05 if trial % 2 else 0.003)
        n_trunc += _same(txt, *OPTS[trial % len(OPTS)])[3]
    assert n_trunc > 50


def _quals(rng, n, L, tail=True):
    """Phred+33 qualities: mostly high, with low-quality 5' / 3' stretches of random length on some reads."""
    q = rng.integers(25, 41, size=(n, L), dtype=np.uint8)
    if tail:
        for i in range(n):
            if rng.random() < 0.5:
                q[i, L - int(rng.integers(1, L // 2)):] = rng.integers(2, 15, dtype=np.uint8)
            if rng.random() < 0.3:
                q[i, : int(rng.integers(1, L // 4))] = rng.integers(2, 12, dtype=np.uint8)
    return q + 33


def _fastq(headers, reads, quals, crlf_every=0):
    out = []
    for i, (h, s, q) in enumerate(zip(headers, reads, quals)):
        eol = b"\r\n" if crlf_every and i % crlf_every == 0 else b"\n"
        out.append(b"@" + h + eol + s + eol + b"+" + eol + q + eol)
    return b"".join(out)


def test_many_chunks():
    """200 k reads of 150 bp (tens of MB, thousands of 4 KB chunks): CRLF records, quality lines that start with '@'
    or '+', then a malformed record near the end and what follows it."""
    rng = np.random.default_rng(8)
    n, L = 200_000, 150
    seqs = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=(n, L))
    quals = _quals(rng, n, L)
    quals[::97, 0] = ord("@")
    quals[::89, 0] = ord("+")
    text = _fastq([b"read_%d" % i for i in range(n)], [bytes(r) for r in seqs], [bytes(q) for q in quals], crlf_every=7)
    for c5, c3 in ((0, 0), (15, 20)):
        want = _same(text, c5, c3)
        assert len(want[0]) == n and not want[3]
    bad = text + b"@x\nACGT\n+\nIII\n" + text[:10000]
    want = _same(bad, 0, 20)
    assert len(want[0]) == n and want[3]


def test_long_reads():
    """10 kb and longer reads: the trimming sums run over many 64-byte pieces from either end."""
    rng = np.random.default_rng(9)
    reads, quals = [], []
    for i in range(40):
        L = int(rng.integers(10_000, 14_000))
        reads.append(bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=L)))
        q = rng.integers(25, 41, size=L, dtype=np.uint8)
        if i % 2:  # a long low-quality 3' tail (crosses many pieces) with a few good bases inside it
            t = int(rng.integers(500, 5000))
            q[L - t:] = rng.integers(2, 12, size=t, dtype=np.uint8)
            q[L - t // 2] = 40
        if i % 3 == 0:
            h = int(rng.integers(100, 3000))
            q[:h] = rng.integers(2, 12, size=h, dtype=np.uint8)
        if i % 5 == 0:
            q[:] = 5  # the whole read goes
        quals.append(bytes(q + 33))
    text = _fastq([b"long_%d" % i for i in range(40)], reads, quals, crlf_every=3)
    for c5, c3 in ((0, 0), (15, 20), (0, 20), (20, 0), (94, 0), (0, 1000)):
        want = _same(text, c5, c3)
        assert len(want[0]) == 40 and not want[3]
    trimmed = np.diff(engine.fastq_parse(text, trim_5p=15, trim_3p=20)[2])
    assert (trimmed == 0).sum() >= 8 and trimmed.max() > 9000


@pytest.mark.parametrize("trim", [(0, 0), (15, 20)])
def test_place_fastq_text_matches_the_oracle(trim):
    s = SynthDb(200, 600, 11, 4)
    n, L = 20_000, 150
    bases, offsets, _ = s.reads(n, L, err=0.02, frac_random=0.03)
    rng = np.random.default_rng(10)
    b = bases.reshape(-1, L)
    text = _fastq([b"read %d" % i for i in range(n)], [bytes(r) for r in b], [bytes(q) for q in _quals(rng, n, L)], crlf_every=5)
    hh, hb, hoff, htr = engine.fastq_parse(text, trim_5p=trim[0], trim_3p=trim[1])
    assert len(hh) == n and not htr
    assert trim == (0, 0) or int(hoff[-1]) < n * L * 0.9
    with engine.PlacementDb(s.flat, device=0) as db:
        headers, got, truncated = db.place_fastq_text(text, trim_5p=trim[0], trim_3p=trim[1])
    assert not truncated and headers == hh
    want = op.OraclePort(s.flat).place_batch(hb, hoff, threads=8)
    assert len(records_equal(got, want)) == 0


def test_cli_fastq_matches_fasta_of_the_trimmed_reads(tmp_path):
    flat, bases, offsets, params, expected = _load()
    names = [str(h).encode() for h in np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colletotrichum_k12.npz"))["headers"]]
    n = len(offsets) - 1
    raw = bytes(bases)
    rng = np.random.default_rng(11)
    seqs = [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
    quals = [bytes(_quals(rng, 1, len(s))[0]) for s in seqs]
    quals[-1] = b"I" * len(seqs[-1])  # (the last read keeps its bases: FASTA drops an empty last record)
    quals[3] = b"#" * len(seqs[3])    # one read trimmed to empty
    db = str(tmp_path / "db.json")
    write_db_json(flat, db)
    fq = str(tmp_path / "q.fq")
    open(fq, "wb").write(_fastq(names, seqs, quals, crlf_every=4))
    hh, hb, hoff, htr = engine.fastq_parse(open(fq, "rb").read(), trim_3p=20)
    assert len(hh) == n and not htr and hoff[4] == hoff[3]
    fa = str(tmp_path / "trimmed.fasta")
    write_fasta(fa, [h.decode() for h in hh], hb, hoff)
    for fmt in ("yaml", "jsonl"):
        def run(name, args, stdin=None):
            out = str(tmp_path / name / "r.out")
            r = subprocess.run([CLI, *args, "-d", db, "-o", out, "--out-format", fmt], capture_output=True, timeout=300,
                               stdin=open(stdin, "rb") if stdin else None)
            assert r.returncode == 0, r.stderr
            return open(str(tmp_path / name / f"r.{fmt}"), "rb").read(), open(str(tmp_path / name / "r.error"), "rb").read()
        want = run(f"fa_{fmt}", [fa])
        assert len(want[0]) > 0
        assert run(f"fq_{fmt}", [fq, "--query-format", "fastq", "-q", "20"]) == want
        assert run(f"fq2_{fmt}", [fq, "--query-format", "fastq", "--trim-quality", "0,20", "--device", "0,0"]) == want
        assert run(f"fqin_{fmt}", ["-", "--query-format", "fastq", "-q", "20"], stdin=fq) == want
    # the Python use-case, on one handle and on a group
    tree = engine.Tree(db)
    with engine.PlacementDb(tree.flat(), device=0) as one:
        n1, _ = engine.place_sequences(one, tree, fq, str(tmp_path / "py1" / "r.out"), query_format="fastq", trim_quality=20)
    with engine.PlacementDbGroup(tree.flat(), [0, 0, 0]) as grp:
        n3, _ = engine.place_sequences(grp, tree, fq, str(tmp_path / "py3" / "r.out"), query_format="fastq", trim_quality=(0, 20))
    assert n1 == n3 == n
    assert open(tmp_path / "py1" / "r.yaml", "rb").read() == open(tmp_path / "py3" / "r.yaml", "rb").read() == \
        open(tmp_path / "fa_yaml" / "r.yaml", "rb").read()
