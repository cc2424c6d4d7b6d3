"""The FASTQ stage's rules (include/cls_place.h) restated in plain Python: the yardstick of the C parser, which is in
turn the yardstick of the device stage.  Test infrastructure only."""


def _lines(text: bytes):
    """-> list of (content, start) per existing line: "\\n" or "\\r\\n" stripped; a line exists iff it starts before the
    end of the text."""
    out, pos = [], 0
    while pos < len(text):
        nl = text.find(b"\n", pos)
        if nl < 0:
            out.append((text[pos:], pos))
            break
        c = text[pos:nl]
        if c.endswith(b"\r"):
            c = c[:-1]
        out.append((c, pos))
        pos = nl + 1
    return out


def _utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def well_formed(lines) -> bool:
    if len(lines) < 4:
        return False
    h, s, p, q = lines
    return (h[:1] == b"@" and len(h) >= 2 and _utf8(h[1:]) and p[:1] == b"+" and all(c < 0x80 for c in s)
            and len(q) == len(s) and all(33 <= c <= 126 for c in q))


def trim(qual: bytes, c5: int, c3: int):
    """BWA / cutadapt -q: the kept window [start, stop) (start == stop: trimmed to empty)."""
    q = [c - 33 for c in qual]
    L = len(q)
    start, s, best = 0, 0, 0
    for i in range(L):
        s += c5 - q[i]
        if s < 0:
            break
        if s > best:
            best, start = s, i + 1
    stop, s, best = L, 0, 0
    for i in range(L - 1, -1, -1):
        s += c3 - q[i]
        if s < 0:
            break
        if s > best:
            best, stop = s, i
    return (start, stop) if start < stop else (0, 0)


def keep_bases(seq: bytes) -> bytes:
    return bytes(c for c in seq.upper() if c in b"ACGT")


def parse(text: bytes, c5: int = 0, c3: int = 0):
    """-> (records [(header, bases)], truncated)."""
    lines = [c for c, _ in _lines(text)]
    recs = []
    for r in range(0, len(lines), 4):
        group = lines[r:r + 4]
        if group[0] == b"":
            return recs, any(x != b"" for x in lines[r:])
        if not well_formed(group):
            return recs, True
        h, s, _, q = group
        a, b = trim(q, c5, c3)
        recs.append((h[1:], keep_bases(s[a:b])))
    return recs, False


def well_formed_record_ends(text: bytes):
    """Byte positions where a record that is well-formed ends (the starts of line 4r + 4), in order."""
    ls = _lines(text)
    lines = [c for c, _ in ls]
    out = []
    for r in range(0, len(lines), 4):
        if lines[r] != b"" and well_formed(lines[r:r + 4]):
            out.append(ls[r + 4][1] if r + 4 < len(ls) else len(text))
    return out


def to_fasta(recs) -> bytes:
    """The FASTA whose parse gives `recs` (headers without '>')."""
    return b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
