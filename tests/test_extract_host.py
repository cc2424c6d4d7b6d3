"""Read extraction on the host (no GPU): cls_select_host and cls_extract_host -- the statements of the selection rule and
of record text / output in include/cls_place.h -- against the Python restatement in tests/extract_ref.py."""
import numpy as np
import pytest

from classeq2_amd import _abi, engine
from tests import extract_ref as er
from tests.test_pair_host import TREES
from tests.test_tally_host import craft

U64_MAX = (1 << 64) - 1
TREE_NAMES = ("k12", "k9_ids", "deep")


def crafted_records(nodes, seed=0, per_status=150):
    """Every status 0..13 and 255 on `per_status` random clades (the root and a leaf among them) and on ids that are no
    clade of the tree; garbage pad bytes."""
    rng = np.random.default_rng(seed)
    ids = set(int(x) for x in nodes["id"])
    unknown = [x for x in (U64_MAX, 0, max(ids) + 1, min(ids) + 1) if x not in ids]
    leaf = int(np.nonzero(nodes["n_children"] == 0)[0][-1])
    st, cid = [], []
    for s in list(range(14)) + [255]:
        rows = [0, leaf] + [int(x) for x in rng.integers(0, len(nodes), per_status)]
        for r in rows:
            st.append(s), cid.append(int(nodes["id"][r]))
        for u in unknown:
            st.append(s), cid.append(u)
    m = len(st)
    recs = craft(np.array(st, np.uint8), np.array(cid, np.uint64), rng.integers(-9, 9, m), rng.integers(-9, 9, m), 3)
    recs["pad_"] = rng.integers(0, 256, (m, 3))
    return recs[rng.permutation(m)]


def selectors(nodes):
    """name -> (include, exclude, flags) on the tree `nodes`."""
    par = er.parents(nodes)
    depth, todo = [0] * len(nodes), [0]
    for r in todo:
        for c in range(int(nodes[r]["first_child"]), int(nodes[r]["first_child"]) + int(nodes[r]["n_children"])):
            depth[c] = depth[r] + 1
            todo.append(c)
    z = max(range(len(nodes)), key=lambda r: depth[r])
    assert depth[z] >= 3
    y, x = par[z], par[par[z]]
    ident = lambda r: int(nodes["id"][r])
    leaf = int(np.nonzero(nodes["n_children"] == 0)[0][0])
    top = int(nodes[0]["first_child"])
    return {
        "root": ([ident(0)], [], 0),
        "one leaf": ([ident(leaf)], [], 0),
        "X, not Y, but Z": ([ident(x), ident(z)], [ident(y)], 0),
        "exclude only": ([], [ident(top)], 0),
        "the unplaced only": ([], [], 1),
        "everything": ([ident(0)], [], 1),
        "outside a root child": ([ident(0)], [ident(top)], 0),
    }


def complement(nodes, inc, exc, flags):
    """The selector that picks exactly what (inc, exc, flags) does not: the root joins the excludes if it is not listed
    (which changes nothing), the lists change places, UNPLACED flips."""
    root = int(nodes["id"][0])
    if root not in inc and root not in exc:
        exc = list(exc) + [root]
    return list(exc), list(inc), flags ^ 1


@pytest.fixture(scope="module", params=TREE_NAMES)
def case(request):
    s = TREES[request.param]()
    return request.param, s, crafted_records(s.flat.nodes)


def test_select_host_equals_reference(case):
    name, s, recs = case
    nodes = s.flat.nodes
    placed = er.placed_ref(nodes, recs)
    assert placed.any() and (~placed).any() and set(range(14)) <= set(int(x) for x in recs["status"])
    for what, (inc, exc, flags) in selectors(nodes).items():
        want = er.select_ref(nodes, recs, inc, exc, flags)
        got = engine.select_host(s.flat, recs, inc, exc, flags=flags)
        assert np.array_equal(got, want), f"{name}, {what}"
        assert set(np.unique(got)) <= {0, 1}
        cinc, cexc, cflags = complement(nodes, inc, exc, flags)
        other = engine.select_host(s.flat, recs, cinc, cexc, flags=cflags)
        assert np.array_equal(got + other, np.ones(len(recs), np.uint8)), f"{name}, {what}: a selector and its complement partition the records"
    sel = selectors(nodes)
    assert np.array_equal(engine.select_host(s.flat, recs, *sel["root"][:2]) == 1, placed)
    assert np.array_equal(engine.select_host(s.flat, recs, unplaced=True) == 1, ~placed)
    assert engine.select_host(s.flat, recs, *sel["everything"][:2], unplaced=True).all()
    xyz = engine.select_host(s.flat, recs, *sel["X, not Y, but Z"][:2])
    assert 0 < xyz.sum() < placed.sum()
    pad0 = recs.copy()
    pad0["pad_"] = 0
    assert np.array_equal(engine.select_host(s.flat, pad0, *sel["one leaf"][:2]), engine.select_host(s.flat, recs, *sel["one leaf"][:2]))
    assert len(engine.select_host(s.flat, recs[:0], *sel["root"][:2])) == 0


def test_selector_validation(case):
    name, s, recs = case
    nodes = s.flat.nodes
    root, kid = int(nodes["id"][0]), int(nodes["id"][1])
    ids = set(int(x) for x in nodes["id"])
    unknown = next(x for x in (U64_MAX, max(ids) + 1) if x not in ids)
    for inc, exc, flags in (([root, root], [], 0), ([], [kid, kid], 0), ([root], [root], 0), ([unknown], [], 0), ([root], [unknown], 0),
                            ([root], [], 2), ([root], [], 1 << 31)):
        assert not er.selector_ok(nodes, inc, exc, flags)
        with pytest.raises(engine.ClsError) as e:
            engine.select_host(s.flat, recs[:5], inc, exc, flags=flags)
        assert e.value.code == -1, (inc, exc, flags)


# ---- record text and output --------------------------------------------------------------------------------------------

def fastq_records(n, seed=0, eol=b"\n"):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 40)) if i % 5 else int(rng.integers(150, 400))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), L))
        qual = bytes((rng.integers(0, 41, L) + 33).astype(np.uint8))
        recs.append(b"@r%d some comment" % i + eol + seq + eol + b"+" + (b"r%d" % i if i % 3 == 0 else b"") + eol + qual + eol)
    return recs


def texts():
    """name -> FASTQ text (the cases of the issue)."""
    lf, crlf = fastq_records(23, 1), fastq_records(23, 2, b"\r\n")
    bad = list(lf)
    bad[11] = b"@broken\nACGT\n-\nIIII\n"
    return {
        "LF": b"".join(lf),
        "CRLF": b"".join(crlf),
        "no final newline": b"".join(lf)[:-1],
        "CRLF, no final newline": b"".join(crlf)[:-2],
        "trailing blank lines": b"".join(lf) + b"\n\n\n",
        "malformed record in the middle": b"".join(bad),
        "one record": lf[0],
        "empty": b"",
    }


def selections(n_items, seed=0):
    rng = np.random.default_rng(seed)
    pats = {"none": np.zeros(n_items, np.uint8), "all": np.ones(n_items, np.uint8), "alternating": (np.arange(n_items) % 2).astype(np.uint8),
            "random": rng.integers(0, 2, n_items).astype(np.uint8)}
    first, last = np.zeros(n_items, np.uint8), np.zeros(n_items, np.uint8)
    if n_items:
        first[0], last[-1] = 1, 1
    pats["only the first"], pats["only the last"] = first, last
    return pats


@pytest.mark.parametrize("name", list(texts()))
def test_extract_host_equals_reference(name):
    text = texts()[name]
    headers, bases, boff, truncated = engine.fastq_parse(text)
    n = len(headers)
    assert truncated == (name == "malformed record in the middle")
    assert n == {"malformed record in the middle": 11, "one record": 1, "empty": 0}.get(name, 23)
    for stride in (1, 2):
        n_items = n // stride
        for what, sel in selections(n_items).items():
            want, _, totals = er.extract_ref(text, sel, stride)
            got, tot = engine.extract_host(text, sel, stride)
            assert got == want, f"{name}, stride {stride}, {what}"
            er.assert_totals(tot, totals, f"{name}, stride {stride}, {what}")
            assert int(tot["n_selected_unplaced"]) == 0
            # the output parses to exactly the selected records
            h2, b2, o2, tr2 = engine.fastq_parse(got)
            keep = [i * stride + j for i in range(n_items) if sel[i] for j in range(stride)]
            assert not tr2 and h2 == [headers[i] for i in keep], f"{name}, stride {stride}, {what}"
            assert [bytes(b2[int(o2[k]):int(o2[k + 1])]) for k in range(len(keep))] == [bytes(bases[int(boff[i]):int(boff[i + 1])]) for i in keep]
        # everything selected: the emitted records' text itself, plus the one newline where due
        got, tot = engine.extract_host(text, np.ones(n_items, np.uint8), stride)
        end = int(er.spans_ref(text, n_items * stride)[-1])
        assert got == text[:end] + (b"\n" if end and not text[:end].endswith(b"\n") else b"")
        assert int(tot["bytes_out"]) == len(got)


def test_extract_host_refusals():
    text = texts()["LF"]
    for stride in (0, 3):
        with pytest.raises(engine.ClsError) as e:
            engine.extract_host(text, np.ones(2, np.uint8), stride)
        assert e.value.code == -1
    # items beyond the text's lines are empty: nothing is read past the end
    got, tot = engine.extract_host(b"@a\nAC\n+\nII\n", np.ones(5, np.uint8))
    assert got == b"@a\nAC\n+\nII\n" and int(tot["n_selected"]) == 5
