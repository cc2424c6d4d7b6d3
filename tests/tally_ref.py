"""numpy restatement of the clade tally's counting rules (include/cls_place.h) and a parser of the clade report
(include/cls_host.h).  Deliberately another algorithm than the library's two: rows are found by a sorted-id search,
counted with np.bincount, and the subtree sums are one bottom-up pass over the rows."""
import numpy as np

from classeq2_amd import _abi

BEARING = (_abi.IDENTITY_FOUND, _abi.MAX_RESOLUTION, _abi.INCONCLUSIVE)
COLUMNS = ["clade_id", "parent_id", "kind", "depth", "name", "n_clade", "n_direct", "n_identity", "n_max_resolution", "n_inconclusive",
           "mean_one", "mean_rest"]


def tally_ref(nodes: np.ndarray, records: np.ndarray):
    """-> (rows TALLY_ROW_DTYPE[n_nodes], totals TALLY_TOTALS_DTYPE scalar) of `records` over the tree `nodes`
    (children rows are larger than their parent's, as FlatDb and cls_tree lay them out)."""
    n = len(nodes)
    rows = np.zeros(n, dtype=_abi.TALLY_ROW_DTYPE)
    totals = np.zeros(1, dtype=_abi.TALLY_TOTALS_DTYPE)[0]
    rows["id"] = nodes["id"]
    st = records["status"].astype(np.int64)
    totals["n_reads"] = len(records)
    totals["n_bad_status"] = int((st >= 12).sum())
    totals["status_count"] = np.bincount(st[st < 12], minlength=12)
    bearing = np.isin(st, BEARING)
    order = np.argsort(nodes["id"], kind="stable")
    sorted_ids = nodes["id"][order]
    ids = records["clade_id"][bearing]
    pos = np.searchsorted(sorted_ids, ids)
    pos_c = np.minimum(pos, n - 1)
    known = (pos < n) & (sorted_ids[pos_c] == ids)
    totals["n_unknown_clade"] = int((~known).sum())
    row = order[pos_c[known]]
    bst = st[bearing][known]
    for status, name in zip(BEARING, ("n_identity", "n_max_resolution", "n_inconclusive")):
        rows[name] = np.bincount(row[bst == status], minlength=n)
    rows["n_direct"] = rows["n_identity"] + rows["n_max_resolution"] + rows["n_inconclusive"]
    ident = bst == _abi.IDENTITY_FOUND
    for src, dst in (("one", "sum_one"), ("rest", "sum_rest")):
        v = records[src][bearing][known][ident].astype(np.int64)
        s = np.zeros(n, dtype=np.int64)
        np.add.at(s, row[ident], v)
        rows[dst] = s
    clade = rows["n_direct"].copy()
    for r in range(n - 1, -1, -1):
        nc = int(nodes[r]["n_children"])
        if nc:
            fc = int(nodes[r]["first_child"])
            assert fc > r, "children rows must follow their parent's"
            clade[r] += clade[fc:fc + nc].sum()
    rows["n_clade"] = clade
    return rows, totals


def rows_equal(a, b):
    return all((a[f] == b[f]).all() for f in _abi.TALLY_ROW_DTYPE.names)


def totals_equal(a, b):
    a, b = np.atleast_1d(a)[0], np.atleast_1d(b)[0]
    return all(np.array_equal(a[f], b[f]) for f in _abi.TALLY_TOTALS_DTYPE.names)


def assert_tally_equal(got, want, what=""):
    (gr, gt), (wr, wt) = got, want
    for f in _abi.TALLY_ROW_DTYPE.names:
        bad = np.nonzero(gr[f] != wr[f])[0]
        assert len(bad) == 0, f"{what}: rows[{f}] differs at {len(bad)} rows; first row {bad[0]}: got {gr[f][bad[0]]}, want {wr[f][bad[0]]}"
    gt, wt = np.atleast_1d(gt)[0], np.atleast_1d(wt)[0]
    for f in _abi.TALLY_TOTALS_DTYPE.names:
        assert np.array_equal(gt[f], wt[f]), f"{what}: totals[{f}]: got {gt[f]}, want {wt[f]}"


def check_invariants(nodes, records, rows, totals):
    totals = np.atleast_1d(totals)[0]
    st = records["status"]
    assert int(totals["status_count"].sum()) + int(totals["n_bad_status"]) == int(totals["n_reads"]) == len(records)
    n_bearing = int(np.isin(st, BEARING).sum())
    assert int(rows["n_clade"][0]) + int(totals["n_unknown_clade"]) == n_bearing
    for r in range(len(nodes)):
        nc, fc = int(nodes[r]["n_children"]), int(nodes[r]["first_child"])
        below = int(rows["n_clade"][fc:fc + nc].sum()) if nc else 0
        assert int(rows["n_clade"][r]) == int(rows["n_direct"][r]) + below, r
        if nc == 0:
            assert rows["n_clade"][r] == rows["n_direct"][r]


def parse_report(text: bytes):
    """-> (header dict: reads, status {name: count}, unknown_clade, bad_status; list of line dicts keyed by COLUMNS)."""
    assert text.endswith(b"\n") and b"\r" not in text
    lines = text.decode().split("\n")[:-1]
    assert lines[0] == "# classeq2_amd clade report v1"
    head = {"status": {}}
    i = 1
    while lines[i].startswith("# "):
        f = lines[i][2:].split("\t")
        if f[0] == "status":
            assert len(f) == 3
            head["status"][f[1]] = int(f[2])
        else:
            assert len(f) == 2
            head[f[0]] = int(f[1])
        i += 1
    assert list(head["status"]) == _abi.STATUS_NAMES and i == 16
    assert lines[i].split("\t") == COLUMNS
    out = []
    for ln in lines[i + 1:]:
        f = ln.split("\t")
        assert len(f) == len(COLUMNS), ln
        out.append(dict(zip(COLUMNS, f)))
    return head, out


def fmt_mean(s, n):
    return "-" if n == 0 else "%.3f" % (float(s) / float(n))
