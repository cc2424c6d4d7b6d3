"""Python statement of the read-extraction rules of include/cls_place.h ("read extraction"): selection by walking parents,
record spans by splitting the text at '\\n', output by joining.  Shares no code with the C++ host statements."""
import numpy as np

from classeq2_amd import _abi

PLACED_STATUSES = (_abi.IDENTITY_FOUND, _abi.MAX_RESOLUTION, _abi.INCONCLUSIVE)


def parents(nodes):
    """-> parent row of every row (None for the root), from the child ranges."""
    par = [None] * len(nodes)
    for r in range(len(nodes)):
        fc, nc = int(nodes[r]["first_child"]), int(nodes[r]["n_children"])
        for c in range(fc, fc + nc):
            par[c] = r
    return par


def selector_ok(nodes, include, exclude, flags):
    ids = set(int(x) for x in nodes["id"])
    listed = [int(x) for x in include] + [int(x) for x in exclude]
    return flags & ~1 == 0 and len(set(listed)) == len(listed) and all(x in ids for x in listed)


def select_ref(nodes, records, include=(), exclude=(), flags=0):
    """-> u8[n]: 1 selected, 0 not."""
    assert selector_ok(nodes, include, exclude, flags)
    par = parents(nodes)
    row_of = {int(x): r for r, x in enumerate(nodes["id"])}
    mark = {row_of[int(x)]: True for x in include}
    mark.update({row_of[int(x)]: False for x in exclude})
    out = np.zeros(len(records), dtype=np.uint8)
    for i, rec in enumerate(records):
        row = row_of.get(int(rec["clade_id"])) if int(rec["status"]) in PLACED_STATUSES else None
        if row is None:
            out[i] = 1 if flags & 1 else 0
            continue
        while row is not None and row not in mark:
            row = par[row]
        out[i] = 1 if row is not None and mark[row] else 0
    return out


def placed_ref(nodes, records):
    ids = set(int(x) for x in nodes["id"])
    return np.array([int(r["status"]) in PLACED_STATUSES and int(r["clade_id"]) in ids for r in records], dtype=bool)


def spans_ref(text: bytes, n: int):
    """-> rec_off[n + 1]: the start of line 4 r, len(text) when the text ends before it."""
    lines = text.split(b"\n")  # line k starts at the sum of the lengths (+ 1 each) of the lines before it
    starts, pos = [], 0
    for ln in lines:
        starts.append(pos)
        pos += len(ln) + 1
    if text.endswith(b"\n") or not text:
        starts.pop()  # (the empty piece behind a final newline is no line)
    return np.array([starts[4 * r] if 4 * r < len(starts) else len(text) for r in range(n + 1)], dtype=np.uint64)


def extract_ref(text: bytes, sel, stride=1):
    """-> (output bytes, out_off[n_items + 1], totals dict) for one selection byte per item."""
    n_items = len(sel)
    off = [int(x) for x in spans_ref(text, n_items * stride)]
    parts, out_off = [], [0]
    for i in range(n_items):
        piece = b""
        if sel[i]:
            piece = text[off[i * stride]:off[(i + 1) * stride]]
            if piece and not piece.endswith(b"\n"):
                piece += b"\n"
        parts.append(piece)
        out_off.append(out_off[-1] + len(piece))
    out = b"".join(parts)
    totals = {"n_records": n_items, "n_selected": int(np.count_nonzero(sel)), "bytes_out": len(out)}
    return out, np.array(out_off, dtype=np.uint64), totals


def assert_totals(got, want, what=""):
    for k, v in want.items():
        assert int(got[k]) == v, f"{what}: totals.{k} = {int(got[k])}, want {v}"
