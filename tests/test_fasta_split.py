"""cls_fasta_split (no GPU): the pieces it cuts parse, one by one and joined up to the first piece that stops early, to
exactly the records of the whole text, on the parser's own corner cases and on generated adversarial texts."""
import random

import pytest

from classeq2_amd import engine
from oracle import oracle_literal as lit
from tests.test_host_cpu import FASTA_CASES


def _adversarial(seed: int) -> bytes:
    """A FASTA-like text with every line shape that carries parser state across lines."""
    rng = random.Random(seed)
    headers = [b">", b">>", b">>>", b"> ", b">\r", b">h", b">a b>c", b">>x>y", b">sample_%d" % rng.randrange(1000)]
    seqs = [b"ACGT", b"acgtacgtnn", b"NNNN", b"nnnn", b"", b"A-C G.T*", b"ryk", b"GGGGCCCC" * 3, b"t"]
    eol = b"\r\n" if rng.random() < 0.3 else b"\n"
    lines = []
    if rng.random() < 0.2:  # headerless start
        lines.append(rng.choice(seqs))
    for _ in range(rng.randrange(1, 25)):
        lines.append(rng.choice(headers))
        for _ in range(rng.choice([0, 0, 1, 1, 2, 3])):
            lines.append(rng.choice(seqs))
        if rng.random() < 0.2:
            lines.append(b"")  # blank line
    if rng.random() < 0.15:  # invalid UTF-8 in a header or a sequence line
        i = rng.randrange(len(lines))
        lines[i] = lines[i] + rng.choice([b"\xff", b"\xc3", b"\xed\xa0\x80"])
    text = b""
    for i, ln in enumerate(lines):
        text += ln + (eol if rng.random() < 0.9 else b"\n")
    if rng.random() < 0.3:  # no trailing newline
        text = text.rstrip(b"\n")
    return text


TEXTS = list(FASTA_CASES) + [_adversarial(s) for s in range(300)]


def _records(text: bytes):
    headers, bases, off, truncated = engine.fasta_parse(text)
    return [(headers[i], bytes(bases[int(off[i]):int(off[i + 1])])) for i in range(len(headers))], truncated


def _safe_cuts(text: bytes):
    """Every safe cut by the header's definition, from a line-by-line walk of its own."""
    safe, header_ok, seq_ok, pos = [], False, False, 0
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            try:
                line.decode("utf-8")
                valid = True
            except UnicodeDecodeError:  # the parse stops at this line, before it emits the record
                valid = False
            if header_ok and seq_ok and valid:
                safe.append(pos)
            header_ok = line.replace(b">", b"").replace(b"\r", b"") != b""
            seq_ok = False
        else:
            seq_ok = seq_ok or any(c in b"ACGTacgt" for c in line)
        pos += len(line) + 1
    return safe


@pytest.mark.parametrize("max_pieces", range(1, 9))
def test_split_cuts_follow_the_contract(max_pieces):
    for text in TEXTS:
        cuts = engine.fasta_split(text, max_pieces)
        safe = _safe_cuts(text)
        want = [0]
        for i in range(1, max_pieces):
            t = i * len(text) // max_pieces
            nxt = [p for p in safe if p >= t]
            if nxt and nxt[0] != want[-1]:
                want.append(nxt[0])
        want.append(len(text))
        assert cuts == want, (text, max_pieces)
        assert all(a < b for a, b in zip(cuts[1:-1], cuts[2:-1])) and len(cuts) - 1 <= max_pieces
        for c in cuts[1:-1]:
            assert text[c:c + 1] == b">" and text[c - 1:c] == b"\n", (text, c)


@pytest.mark.parametrize("max_pieces", range(1, 9))
def test_pieces_parse_to_the_whole_text(max_pieces):
    n_multi = 0
    for text in TEXTS:
        cuts = engine.fasta_split(text, max_pieces)
        n_multi += len(cuts) > 2
        got, got_trunc = [], False
        for a, b in zip(cuts, cuts[1:]):
            recs, trunc = _records(text[a:b])
            got += recs
            if trunc:  # the whole parse stops here: the pieces after it are dropped
                got_trunc = True
                break
        want, want_trunc = _records(text)
        assert got == want and got_trunc == want_trunc, (text, cuts)
        # and the reference's own reader, compared as test_fasta_parse_matches_literal does
        strs = [(h.decode("utf-8"), s.decode()) for h, s in got]
        try:
            lit_want = lit.sequence_content_by_channel(text.decode("utf-8"))
            assert strs == lit_want, (text, cuts)
        except UnicodeDecodeError as e:
            cut = text.rfind(b"\n", 0, e.start) + 1
            lit_want = lit.sequence_content_by_channel(text[:cut].decode("utf-8"))
            assert strs == lit_want[: len(strs)] and got_trunc, (text, cuts)
    if max_pieces > 1:
        assert n_multi > 50  # the generated texts do get cut


def test_split_edges():
    assert engine.fasta_split(b"", 4) == [0, 0]
    assert engine.fasta_split(b">a\nAC\n", 1) == [0, 6]
    # every record boundary is safe: 8 pieces of one record each
    text = b"".join(b">r%d\nACGT\n" % i for i in range(8))
    assert engine.fasta_split(text, 8) == [0] + [i * 9 for i in range(1, 8)] + [len(text)]
    # an empty header, an N-only sequence, a '>'-only header, or a '>' line that is not valid UTF-8 (the whole parse
    # stops there without emitting the record) is no cut
    for t in (b">\nAC\n>b\nAC\n", b">a\nNN\n>b\nAC\n", b">>\r\nAC\r\n>b\nAC\n", b">a\nAC\n>b\xff\nAC\n"):
        assert engine.fasta_split(t, 2) == [0, len(t)], t
    assert engine.fasta_split(b">a\nAC\n>b\nAC\n", 2) == [0, 6, 12]
    with pytest.raises(engine.ClsError):
        engine.fasta_split(b">a\nAC\n", 0)
