"""Clade tally on the host (no GPU): cls_tally_host -- the statement of the counting rules in include/cls_place.h --
against the numpy restatement in tests/tally_ref.py, on oracle records and on crafted ones; merging; the clade report."""
import json
import os

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests import tally_ref as tr
from tests.helpers import PARAM_SETS, ragged_reads

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {0: "ROOT", 1: "NODE", 2: "LEAF"}
U64_MAX = (1 << 64) - 1


def shape(name):
    """-> (SynthDb, bases, offsets): the ragged batches of tests/test_gpu_group.py (2500 reads and a tail of long ones)."""
    rng = np.random.default_rng(7)
    if name == "k12":
        s = SynthDb(64, 3000, 12, 4)
        a = ragged_reads(rng, s, 2500, 0, 200)
        b = ragged_reads(rng, s, 40, 300, 2000)
        return s, np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1][1:] + a[1][-1]]).astype(np.uint64)
    if name == "k16_poly":
        s = SynthDb(64, 3000, 16, 4, collapse_prob=0.4)
        return s, *ragged_reads(rng, s, 2500, 0, 400)
    if name == "k12_long":
        s = SynthDb(32, 6000, 12, 4)
        a = ragged_reads(rng, s, 6, 4200, 5800, lower_frac=0.0)
        b = ragged_reads(rng, s, 2000, 100, 160)
        return s, np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1][1:] + a[1][-1]]).astype(np.uint64)
    raise AssertionError(name)


def depths(nodes):
    d = np.zeros(len(nodes), dtype=np.int64)
    for r in range(len(nodes)):
        fc, nc = int(nodes[r]["first_child"]), int(nodes[r]["n_children"])
        d[fc:fc + nc] = d[r] + 1
    return d


def craft(status, clade_id, one=0, rest=0, levels=0, pad=0):
    n = len(status)
    r = np.zeros(n, dtype=_abi.PLACEMENT_DTYPE)
    r["status"], r["clade_id"], r["one"], r["rest"], r["levels"] = status, clade_id, one, rest, levels
    r["pad_"] = pad
    return r


def crafted_records(nodes, seed=0):
    """What placement cannot produce: every status on a leaf, an inner clade and the root; CLS_INCONCLUSIVE; unknown
    ids; status 12 and 255; negative one / rest; garbage in the padding bytes."""
    rng = np.random.default_rng(seed)
    leaf = int(np.nonzero(nodes["kind"] == _abi.KIND_LEAF)[0][-1])
    inner = int(np.nonzero((nodes["kind"] == _abi.KIND_NODE) & (nodes["n_children"] > 0))[0][0])
    ids = set(int(x) for x in nodes["id"])
    near = next(int(i) + d for i in nodes["id"] for d in (1, -1) if 0 < int(i) + d < U64_MAX and int(i) + d not in ids)
    parts = []
    for row in (leaf, inner, 0):
        st = np.arange(12, dtype=np.uint8)
        parts.append(craft(st, int(nodes[row]["id"]), one=rng.integers(-50, 50, 12), rest=rng.integers(-2000, 5, 12), levels=3, pad=0xFF))
    for bad_id in (0, U64_MAX, near):
        if bad_id in ids:  # (id 0 is often the root's)
            continue
        parts.append(craft(np.array([4, 5, 6, 0, 9], dtype=np.uint8), bad_id, one=7, rest=-7))
    parts.append(craft(np.array([12, 255, 12, 200], dtype=np.uint8), int(nodes[leaf]["id"]), one=5, rest=5, pad=0xAB))
    parts.append(craft(np.full(9, 6, dtype=np.uint8), int(nodes[inner]["id"]), one=3))
    parts.append(craft(np.full(5, 4, dtype=np.uint8), int(nodes[leaf]["id"]), one=-(2 ** 31), rest=2 ** 31 - 1, pad=0x5A))
    recs = np.concatenate(parts)
    return recs[rng.permutation(len(recs))]


@pytest.fixture(scope="module", params=["k12", "k16_poly"])
def oracle_case(request):
    s, bases, offsets = shape(request.param)
    oracle = op.OraclePort(s.flat)
    recs = [oracle.place_batch(bases, offsets, op.make_params(**kw), threads=8) for kw in PARAM_SETS]
    return request.param, s, recs


def test_oracle_records_cover_the_condition(oracle_case):
    """The inputs are worth counting: both placed outcomes, at least four further statuses, at least 20 clades at
    at least 3 depths receive clade-bearing records (over the batches of one shape)."""
    name, s, recs = oracle_case
    allr = np.concatenate(recs)
    seen = set(int(x) for x in np.unique(allr["status"]))
    assert _abi.IDENTITY_FOUND in seen and _abi.MAX_RESOLUTION in seen, seen
    assert len(seen - {_abi.IDENTITY_FOUND, _abi.MAX_RESOLUTION}) >= 4, seen
    bearing = allr[np.isin(allr["status"], tr.BEARING)]
    nodes = s.flat.nodes
    row_of = {int(i): r for r, i in enumerate(nodes["id"])}
    rows = sorted({row_of[int(c)] for c in np.unique(bearing["clade_id"])})
    assert len(rows) >= 20, len(rows)
    assert len(set(int(x) for x in depths(nodes)[rows])) >= 3


def test_host_equals_reference_on_oracle_records(oracle_case):
    name, s, recs = oracle_case
    for kw, r in zip(PARAM_SETS, recs):
        got = engine.tally_host(s.flat, r)
        tr.assert_tally_equal(got, tr.tally_ref(s.flat.nodes, r), f"{name} {kw}")
        tr.check_invariants(s.flat.nodes, r, *got)


@pytest.mark.parametrize("synth", [lambda: SynthDb(64, 3000, 12, 4), lambda: SynthDb(64, 3000, 16, 4, collapse_prob=0.4),
                                   lambda: SynthDb(80, 300, 9, 4, collapse_prob=0.4, id_stride=7, id_offset=3)])
def test_host_equals_reference_on_crafted_records(synth):
    flat = synth().flat
    recs = crafted_records(flat.nodes)
    assert set(range(12)) <= set(int(x) for x in recs["status"]) and (recs["status"] >= 12).any()
    got = engine.tally_host(flat, recs)
    want = tr.tally_ref(flat.nodes, recs)
    tr.assert_tally_equal(got, want, "crafted")
    tr.check_invariants(flat.nodes, recs, *got)
    rows, totals = got
    assert int(totals[0]["n_unknown_clade"]) >= 3 and int(totals[0]["n_bad_status"]) == 4
    assert int(rows["n_inconclusive"].sum()) >= 9 + 3
    leaf = int(np.nonzero(flat.nodes["kind"] == _abi.KIND_LEAF)[0][-1])
    assert int(rows["sum_one"][leaf]) <= 5 * -(2 ** 31) + 50 and int(rows["sum_rest"][leaf]) >= 5 * (2 ** 31 - 1) - 2000  # 64-bit sums
    # n = 0
    r0, t0 = engine.tally_host(flat, recs[:0])
    assert int(t0[0]["n_reads"]) == 0 and not r0["n_clade"].any() and (r0["id"] == flat.nodes["id"]).all()
    # padding bytes are not looked at
    clean = recs.copy()
    clean["pad_"] = 0
    tr.assert_tally_equal(engine.tally_host(flat, clean), got, "padding")


def test_merging_thirds(oracle_case):
    name, s, recs = oracle_case
    r = np.concatenate([recs[0], crafted_records(s.flat.nodes, seed=3)])
    whole = engine.tally_host(s.flat, r)
    k = len(r) // 3
    rows, totals = None, None
    for part in (r[2 * k:], r[:k], r[k:2 * k]):
        rows, totals = engine.tally_host(s.flat, part, rows, totals)
    tr.assert_tally_equal((rows, totals), whole, "host merge of thirds")
    # the same through cls_tally_merge, as the tallies of replicas are summed
    rows2 = np.zeros(len(s.flat.nodes), dtype=_abi.TALLY_ROW_DTYPE)
    tot2 = np.zeros(1, dtype=_abi.TALLY_TOTALS_DTYPE)
    for part in (r[:k], r[k:2 * k], r[2 * k:]):
        pr, pt = engine.tally_host(s.flat, part)
        engine.tally_merge(rows2, tot2, pr, pt)
    tr.assert_tally_equal((rows2, tot2), whole, "cls_tally_merge of thirds")
    with pytest.raises(engine.ClsError):
        other = rows2.copy()
        other["id"][1] += 1
        engine.tally_merge(rows2, tot2, other, tot2.copy())


def write_tree_json(nodes, path, names=True):
    """The node table as a tree-only JSON export (the root clade alone)."""
    def clade(r):
        d = {"id": int(nodes[r]["id"]), "parent": None if int(nodes[r]["parent"]) == _abi.NO_PARENT else int(nodes[r]["parent"]),
             "kind": KINDS[int(nodes[r]["kind"])]}
        if names and nodes[r]["kind"] == 2:
            d["name"] = f"leaf_{int(nodes[r]['id'])}"
        if nodes[r]["has_children"]:
            d["children"] = [clade(int(nodes[r]["first_child"]) + i) for i in range(int(nodes[r]["n_children"]))]
        return d

    json.dump(clade(0), open(path, "w"))


def dfs_rows(nodes):
    out, st = [], [(0, None, 0)]
    while st:
        r, parent, depth = st.pop()
        out.append((r, parent, depth))
        fc, nc = int(nodes[r]["first_child"]), int(nodes[r]["n_children"])
        for c in range(fc + nc - 1, fc - 1, -1):
            st.append((c, r, depth + 1))
    return out


def check_report(text, nodes, rows, totals, all_rows, name_of):
    totals = np.atleast_1d(totals)[0]
    head, lines = tr.parse_report(text)
    assert head["reads"] == int(totals["n_reads"]) and head["unknown_clade"] == int(totals["n_unknown_clade"])
    assert head["bad_status"] == int(totals["n_bad_status"])
    assert [head["status"][n] for n in _abi.STATUS_NAMES] == [int(x) for x in totals["status_count"]]
    want = [(r, p, d) for r, p, d in dfs_rows(nodes) if all_rows or rows["n_clade"][r] > 0]
    assert len(lines) == len(want)
    for ln, (r, p, d) in zip(lines, want):
        assert ln["clade_id"] == str(int(nodes[r]["id"]))
        assert ln["parent_id"] == ("-" if p is None else str(int(nodes[p]["id"])))
        assert ln["kind"] == KINDS[int(nodes[r]["kind"])] and ln["depth"] == str(d) and ln["name"] == name_of(r)
        for f in ("n_clade", "n_direct", "n_identity", "n_max_resolution", "n_inconclusive"):
            assert ln[f] == str(int(rows[f][r])), (f, r)
        assert ln["mean_one"] == tr.fmt_mean(rows["sum_one"][r], rows["n_identity"][r])
        assert ln["mean_rest"] == tr.fmt_mean(rows["sum_rest"][r], rows["n_identity"][r])
    return lines


def test_report_round_trip(oracle_case, tmp_path):
    name, s, recs = oracle_case
    nodes = s.flat.nodes
    path = str(tmp_path / "tree.json")
    write_tree_json(nodes, path)
    tree = engine.Tree(path)
    tn = tree.nodes()
    for f in ("id", "first_child", "n_children", "kind"):
        assert (tn[f] == nodes[f]).all()
    r = np.concatenate([recs[0], crafted_records(nodes, seed=5)])
    rows, totals = engine.tally_host(s.flat, r)
    name_of = lambda row: f"leaf_{int(nodes[row]['id'])}" if nodes[row]["kind"] == 2 else ""
    every = check_report(tree.report(rows, totals, all_rows=True), nodes, rows, totals, True, name_of)
    assert len(every) == len(nodes) and len({ln["clade_id"] for ln in every}) == len(nodes)
    some = check_report(tree.report(rows, totals), nodes, rows, totals, False, name_of)
    assert 0 < len(some) < len(nodes) and all(int(ln["n_clade"]) > 0 for ln in some)
    assert some[0]["parent_id"] == "-" and some[0]["kind"] == "ROOT" and some[0]["depth"] == "0"
    # rows of another tree are refused
    wrong = rows.copy()
    wrong["id"][3] += 1
    with pytest.raises(engine.ClsError):
        tree.report(wrong, totals)
    with pytest.raises(ValueError):
        tree.report(rows[:-1], totals)


def test_report_shows_clade_names_of_a_real_tree():
    tree = engine.Tree(os.path.join(HERE, "golden", "bsub_gyrb_tree.cls.json"))
    nodes = tree.nodes()
    doc = json.load(open(os.path.join(HERE, "golden", "bsub_gyrb_tree.cls.json")))
    root = doc.get("root", doc)
    names = {}

    def walk(c):
        names[int(c["id"])] = c.get("name") or ""
        for ch in c.get("children") or []:
            walk(ch)

    walk(root)
    assert len(names) == len(nodes) and any(names.values())
    rng = np.random.default_rng(1)
    recs = craft(rng.integers(0, 12, 4000).astype(np.uint8), nodes["id"][rng.integers(0, len(nodes), 4000)], one=rng.integers(0, 90, 4000),
                 rest=rng.integers(-900, 0, 4000))

    class F:  # (tally_host only looks at the node table)
        pass

    f = F()
    f.nodes = nodes
    rows, totals = engine.tally_host(f, recs)
    tr.assert_tally_equal((rows, totals), tr.tally_ref(nodes, recs), "bsub tree")
    lines = check_report(tree.report(rows, totals, all_rows=True), nodes, rows, totals, True, lambda r: names[int(nodes[r]["id"])])
    assert sum(1 for ln in lines if ln["name"]) == sum(1 for v in names.values() if v)
