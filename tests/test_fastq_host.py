"""FASTQ stage on the host (cls_fastq_parse, cls_fastq_split, cls-place's FASTQ flags): the C parser against the
Python restatement of the rules in include/cls_place.h, the trimming-off equivalence with the FASTA stage, and the
split contract.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import engine
from tests import fastq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "classeq2_amd", "csrc", "cls-place")

FASTQ_CASES = [
    b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+r2\r\nII\r\n",          # CRLF
    b"@r1 some text\nACGTacgtNN\n+r1 some text\nIIII##IIII\n",           # '+header' repeat
    b"@e\n\n+\n\n@f\nAC\n+\nII\n",                                       # an empty sequence
    b"@f\nAC\n+\nII\n@e\n\n+\n\n",                                       # ... as the last record
    b"@r\nACGT\n+\nIIII",                                                # no final newline
    b"@r\nACGT\n+\nIIII\n\n\n\r\n\n",                                    # trailing blank lines
    b"@r\nACGT\n+\nIIII\n\n@s\nAC\n+\nII\n",                             # a blank line mid-file
    b"@r\nACGT\n+\nIIII\n\n\n\n\n@s\nAC\n+\nII\n",                       # four of them
    b"@r\nACGT\n+\n@III\n@s\nAC\n+\n+I\n@t\nGG\n+\n@+\n",                # quality lines that start with '@' / '+'
    b"@r\nACGT\n+\nIII\n@s\nAC\n+\nII\n",                                # length mismatch
    b"@r\nAC\n+\nII\n@s\nAC\n+\nI \n",                                   # quality byte below '!'
    b"@r\nAC\n+\nII\n@s\nAC\n+\nI\x7f\n",                                # ... above '~'
    b"r\nAC\n+\nII\n",                                                   # missing '@'
    b"@r\nAC\nII\n+\n",                                                  # missing '+'
    b"@r\nAC\n+\nII\n@s\nAC\n",                                          # incomplete last record
    b"@r\nAC\n+\nII\n@s\nAC\n+",                                         # ... missing only its quality line
    b"@r\n\n+\n",                                                        # empty read whose quality line does not exist
    b"@r\xff\nAC\n+\nII\n",                                              # non-UTF-8 header
    b"@ok\nAC\n+\nII\n@r\xc3\nAC\n+\nII\n",                              # truncated UTF-8 sequence in a header
    b"@\nAC\n+\nII\n",                                                   # empty header
    b"@\r\nAC\r\n+\r\nII\r\n",                                           # ... once '\r' is stripped
    b"@r>x \xc3\xa9\xe2\x82\xac\nAC\n+\nII\n",                           # '>' and UTF-8 in a header are kept
    b"@r\nAC\xc3\xa9\n+\nIIII\n",                                        # non-ASCII sequence byte
    b"@r\nAC\n+\nII\r",                                                  # a '\r' that ends the text is kept
    b"@r\nAC\n\nII\n",                                                   # line 3 empty
    b"@r\nACGTACGT\n+\n!!!!!!!!\n@s\nACGTACGT\n+\nIIII!!!!\n@t\nAC\n+\n##\n",  # trimmed to empty / half
    b"@r\nACG\n+\n+?+\n@s\nACGTA\n+\n+?+?+\n",                           # ties in the running maximum
    b"@r\nNNACGTNN\n+\n5+?+5+?+\n",
    b"", b"\n", b"\n\n\r\n", b"\n@r\nAC\n+\nII\n", b"@", b"@r", b"@r\n", b"+\n",
]
OPTS = [(0, 0), (0, 20), (15, 20), (30, 0), (10, 10), (200, 200)]


def _host(txt, c5=0, c3=0):
    headers, bases, off, truncated = engine.fastq_parse(txt, trim_5p=c5, trim_3p=c3)
    recs = [(headers[i], bytes(bases[int(off[i]):int(off[i + 1])])) for i in range(len(headers))]
    return recs, truncated


@pytest.mark.parametrize("txt", FASTQ_CASES)
def test_fixed_cases_match_the_rules(txt):
    for c5, c3 in OPTS:
        assert _host(txt, c5, c3) == ref.parse(txt, c5, c3), (txt, c5, c3)


def test_fixed_cases_cover_what_they_claim():
    assert ref.parse(FASTQ_CASES[6])[1] and ref.parse(FASTQ_CASES[9])[1] and not ref.parse(FASTQ_CASES[5])[1]
    recs, _ = ref.parse(FASTQ_CASES[25], 0, 20)
    assert recs[0][1] == b"" and recs[1][1] == b"ACGT" and recs[2][1] == b""
    assert ref.trim(b"+?+", 0, 20) == (0, 2) and ref.trim(b"+?+?+", 0, 20) == (0, 4)  # the first maximum counts
    assert ref.trim(b"+?+", 20, 0) == (1, 3)
    assert ref.parse(FASTQ_CASES[8])[0][0] == (b"r", b"ACGT") and len(ref.parse(FASTQ_CASES[8])[0]) == 3


def random_fastq(rng, n_rec=None, bad=0.05, marks=True):
    """Line-structured FASTQ: mostly well-formed records, with the odd defect of every kind."""
    n_rec = int(rng.integers(0, 30)) if n_rec is None else n_rec
    out = []
    for i in range(n_rec):
        L = int(rng.integers(0, 60))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTacgtNn-", dtype=np.uint8), size=L))
        qual = bytes(rng.integers(33, 127, size=L, dtype=np.uint8)) if rng.random() < 0.5 else \
            bytes(rng.choice(np.frombuffer(b"!#+5?I@+", dtype=np.uint8), size=L))
        head = b"@r%d" % i + (b" x>y" if marks and rng.random() < 0.2 else b"")
        plus = b"+" + (head[1:] if rng.random() < 0.3 else b"")
        u = rng.random()
        if u < bad:
            head = rng.choice([b"r", b"@", b"@\xff", b"", b">r"])
        elif u < 2 * bad:
            plus = rng.choice([b"-", b"", b"@"])
        elif u < 3 * bad:
            qual = qual[:-1] if qual else b"I"
        elif u < 4 * bad and L:
            qual = qual[:-1] + bytes([int(rng.choice([32, 127, 200]))])
        elif u < 5 * bad:
            seq = seq + b"\xc3\xa9"
            qual = qual + b"II"
        lines = [head, seq, plus, qual]
        if rng.random() < bad:
            lines = lines[: int(rng.integers(1, 4))]
        if rng.random() < bad:
            lines.insert(int(rng.integers(0, len(lines) + 1)), b"")
        eol = b"\r\n" if rng.random() < 0.2 else b"\n"
        out.append(b"".join(x + eol for x in lines))
    txt = b"".join(out)
    u = rng.random()
    if u < 0.2:
        txt = txt.rstrip(b"\r\n")
    elif u < 0.4:
        txt += b"\n" * int(rng.integers(1, 4))
    return txt


def test_random_texts_match_the_rules():
    rng = np.random.default_rng(5)
    n_trunc = n_rec = 0
    for trial in range(400):
        txt = random_fastq(rng, bad=0.05 if trial % 2 else 0.003)
        c5, c3 = OPTS[trial % len(OPTS)]
        want = ref.parse(txt, c5, c3)
        assert _host(txt, c5, c3) == want, (trial, txt[:200])
        n_trunc += want[1]
        n_rec += len(want[0])
    assert n_trunc > 100 and n_rec > 2000


def test_trimming_off_equals_the_fasta_stage():
    rng = np.random.default_rng(6)
    n_cmp = 0
    for trial in range(200):
        txt = random_fastq(rng, bad=0.0, marks=False)
        for c5, c3 in ((0, 0), (15, 20)):
            recs, truncated = ref.parse(txt, c5, c3)
            lines = [c for c, _ in ref._lines(txt)]  # the FASTA of the (trimmed) sequence lines
            fasta = b"".join(b">" + lines[4 * i][1:] + b"\n" + lines[4 * i + 1][slice(*ref.trim(lines[4 * i + 3], c5, c3))] + b"\n"
                             for i in range(len(recs)))
            if truncated or not recs or not recs[-1][1]:
                continue  # (an empty last read loses its lines to rstrip; FASTA drops an empty last record)
            fq = engine.fastq_parse(txt, trim_5p=c5, trim_3p=c3)
            fa = engine.fasta_parse(fasta)
            assert fq[0] == fa[0] and np.array_equal(fq[1], fa[1]) and np.array_equal(fq[2], fa[2])
            assert fq[3] is False and fa[3] is False
            n_cmp += 1
    assert n_cmp > 200


def _check_split(txt, max_pieces):
    cuts = engine.fastq_split(txt, max_pieces)
    assert cuts[0] == 0 and cuts[-1] == len(txt) and len(cuts) <= max_pieces + 1
    assert all(a < b for a, b in zip(cuts, cuts[1:])) or cuts == [0, 0]
    ends = set(ref.well_formed_record_ends(txt))
    assert all(c in ends for c in cuts[1:-1])
    whole = engine.fastq_parse(txt, trim_3p=20)
    hs, bs, trunc = [], [], False
    for a, b in zip(cuts, cuts[1:]):
        h, bases, off, trunc = engine.fastq_parse(txt[a:b], trim_3p=20)
        hs += h
        bs += [bytes(bases[int(off[i]):int(off[i + 1])]) for i in range(len(h))]
        if trunc:
            break
    assert hs == whole[0] and trunc == whole[3]
    assert bs == [bytes(whole[1][int(whole[2][i]):int(whole[2][i + 1])]) for i in range(len(whole[0]))]
    return len(cuts) - 1


@pytest.mark.parametrize("max_pieces", range(1, 9))
def test_split_pieces_rejoin_to_the_whole_parse(max_pieces):
    rng = np.random.default_rng(100 + max_pieces)
    n_multi = 0
    for _ in range(60):
        n_multi += _check_split(random_fastq(rng, n_rec=int(rng.integers(0, 40))), max_pieces) > 1
    for txt in FASTQ_CASES:
        _check_split(txt, max_pieces)
    big = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, b"ACGT" * 30, b"I" * 120) for i in range(500))
    assert _check_split(big, max_pieces) == max_pieces
    assert max_pieces == 1 or n_multi > 20


def test_split_and_parse_reject_bad_arguments():
    with pytest.raises(engine.ClsError):
        engine.fastq_split(b"@r\nA\n+\nI\n", 0)
    o = engine._fastq_opts(0, 0)
    o.reserved[2] = 1
    f = engine._abi.Fasta()
    assert engine.lib().cls_fastq_parse(b"@r\nA\n+\nI\n", 10, engine.C.byref(o), engine.C.byref(f)) == -1


def test_cli_rejects_trimming_without_fastq(tmp_path):
    """Argument errors exit 2 before anything is loaded (the database path does not even exist)."""
    db, out = str(tmp_path / "missing.cls"), str(tmp_path / "o" / "r.out")
    for extra in (["-q", "20"], ["--trim-quality", "15,20", "--query-format", "fasta"], ["--query-format", "fastx"],
                  ["--query-format", "fastq", "-q", "x"], ["--query-format", "fastq", "-q", "1,2,3"], ["--query-format", "fastq", "-q", "-5"]):
        r = subprocess.run([CLI, "q.fq", "-d", db, "-o", out, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.stderr)
        assert "Error loading database" not in r.stderr
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--query-format" in r.stderr and "--trim-quality" in r.stderr
