"""Paired reads on the host (no GPU): cls_pair_host and cls_pair_names_host -- the statements of the pairing rule and of
the mate-name rule in include/cls_place.h -- against the Python restatement in tests/pair_ref.py, on crafted records and
on records the oracle port places for simulated read pairs."""
import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests import pair_ref as pr
from tests.test_tally_host import craft

U64_MAX = (1 << 64) - 1
STATUSES = list(range(12)) + [12, 255]
RELATIONS = ("same", "parent", "grandparent", "descendant", "sibling", "cousin", "root", "unknown")
ALL_FLAGS = (0, _abi.PAIR_CONSERVATIVE, _abi.PAIR_REQUIRE_BOTH, _abi.PAIR_CONSERVATIVE | _abi.PAIR_REQUIRE_BOTH)
TREES = {
    "k12": lambda: SynthDb(64, 3000, 12, 4),
    "k16_poly": lambda: SynthDb(64, 3000, 16, 4, collapse_prob=0.4),
    "k9_ids": lambda: SynthDb(80, 300, 9, 4, collapse_prob=0.4, id_stride=7, id_offset=3),
    "deep": lambda: SynthDb(700, 120, 9, 4, deep=2),  # a ladder: more than 300 levels
}


def crafted_pairs(nodes, seed=0, per_relation=64):
    """-> (a, b): mate records no placement run yields together.  Every status 0..11, 12 and 255 on both mates for every
    clade relation (same, parent, grandparent, descendant, sibling, cousin under the root, the root itself, unknown id);
    a block of clade-bearing pairs per relation with small, often equal, partly negative one / rest (the tie-break);
    the extremes of one / rest; garbage pad bytes; then all of it again with the mates swapped."""
    rng = np.random.default_rng(seed)
    t = pr.TreeIndex(nodes)
    n = len(nodes)
    kids = lambda r: list(range(int(nodes[r]["first_child"]), int(nodes[r]["first_child"]) + int(nodes[r]["n_children"])))
    deep_rows = [r for r in range(n) if t.depth[r] >= 2]
    with_sibling = [r for r in range(1, n) if len(kids(t.parent[r])) >= 2]
    tops = kids(0)
    assert len(tops) >= 2 and deep_rows and with_sibling
    top_of = {}
    for r in range(1, n):
        top_of[r] = r if t.parent[r] == 0 else top_of[t.parent[r]]
    ids = set(t.ids)
    unknown = [x for x in (U64_MAX, 0, max(ids) + 1, min(ids) + 1) if x not in ids]

    def rows_for(rel):
        if rel == "same":
            x = int(rng.integers(0, n))
            return x, x
        if rel == "parent":
            x = int(rng.integers(1, n))
            return x, t.parent[x]
        if rel == "grandparent":
            x = deep_rows[int(rng.integers(0, len(deep_rows)))]
            return x, t.parent[t.parent[x]]
        if rel == "descendant":
            y = deep_rows[int(rng.integers(0, len(deep_rows)))]
            x = y
            for _ in range(int(rng.integers(1, t.depth[y] + 1))):
                x = t.parent[x]
            return x, y
        if rel == "sibling":
            x = with_sibling[int(rng.integers(0, len(with_sibling)))]
            sib = [c for c in kids(t.parent[x]) if c != x]
            return x, sib[int(rng.integers(0, len(sib)))]
        if rel == "cousin":
            while True:
                x, y = int(rng.integers(1, n)), int(rng.integers(1, n))
                if top_of[x] != top_of[y]:
                    return x, y
        if rel == "root":
            return int(rng.integers(0, n)), 0
        return int(rng.integers(0, n)), None  # unknown id on mate 2

    ra, rb, sa, sb, one, rest = [], [], [], [], [], []
    for rel in RELATIONS:
        for s1 in STATUSES:
            for s2 in STATUSES:
                x, y = rows_for(rel)
                ra.append(x), rb.append(y), sa.append(s1), sb.append(s2)
                one.append(rng.integers(-2 ** 31, 2 ** 31, 2)), rest.append(rng.integers(-2 ** 31, 2 ** 31, 2))
        for _ in range(per_relation):
            x, y = rows_for(rel)
            ra.append(x), rb.append(y), sa.append(int(rng.integers(4, 6))), sb.append(int(rng.integers(4, 6)))
            one.append(rng.integers(-1, 2, 2)), rest.append(rng.integers(-1, 2, 2))
    m = len(ra)
    one, rest = np.array(one), np.array(rest)
    ida = np.array([t.ids[x] for x in ra], dtype=np.uint64)
    idb = np.array([t.ids[y] if y is not None else unknown[i % len(unknown)] for i, y in enumerate(rb)], dtype=np.uint64)
    a = craft(np.array(sa, np.uint8), ida, one[:, 0], rest[:, 0], rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32))
    b = craft(np.array(sb, np.uint8), idb, one[:, 1], rest[:, 1], rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32))
    a["pad_"] = rng.integers(0, 256, (m, 3))
    b["pad_"] = rng.integers(0, 256, (m, 3))
    perm = rng.permutation(2 * m)
    return np.concatenate([a, b])[perm], np.concatenate([b, a])[perm]


def interleave(a, b):
    out = np.empty(2 * len(a), dtype=_abi.PLACEMENT_DTYPE)
    out[0::2], out[1::2] = a, b
    return out


@pytest.fixture(scope="module", params=list(TREES))
def case(request):
    """One tree, its crafted pairs and the reference answer per flag combination (computed once, shared, left unchanged)."""
    s = TREES[request.param]()
    nodes = s.flat.nodes
    a, b = crafted_pairs(nodes)
    tree = pr.TreeIndex(nodes)
    ref = {f: pr.pair_ref(nodes, a, b, f, tree) for f in ALL_FLAGS}
    return request.param, s, a, b, ref, tree


def test_crafted_pairs_cover_the_condition(case):
    """Asserted from pair_ref: every class at least 50 times; discordant LCAs at three or more depths, the root included;
    on the deep tree the tree has at least 300 levels."""
    name, s, a, b, ref, tree = case
    P, how, totals = ref[0]
    assert set(STATUSES) <= set(int(x) for x in a["status"]) and set(STATUSES) <= set(int(x) for x in b["status"])
    counts = np.bincount(how, minlength=8)
    assert (counts[:7] >= 50).all() and counts[7] == 0, counts
    lca_depths = set(int(x) for x in P["levels"][how == _abi.PAIR_DISCORDANT])
    assert 0 in lca_depths and len(lca_depths) >= 3, lca_depths
    assert (a["pad_"] != 0).any() and (a["one"] < 0).any() and (b["rest"] < 0).any()
    same = how == _abi.PAIR_SAME
    tied = same & (a["status"] == b["status"])
    assert (tied & (a["one"] != b["one"])).sum() >= 5 and (tied & (a["one"] == b["one"]) & (a["rest"] != b["rest"])).sum() >= 3
    assert (tied & (a["one"] == b["one"]) & (a["rest"] == b["rest"])).sum() >= 1
    if name == "deep":
        assert max(tree.depth) >= 300


def test_host_equals_reference_on_crafted_pairs(case):
    name, s, a, b, ref, _ = case
    both = interleave(a, b)
    for flags in ALL_FLAGS:
        got = engine.pair_host(s.flat, a, b, flags)
        pr.assert_pairs_equal(got, ref[flags], f"{name} flags {flags} stride 1")
        pr.assert_pairs_equal(engine.pair_host(s.flat, both, None, flags), ref[flags], f"{name} flags {flags} stride 2")
    # n = 0; pad bytes are not looked at
    P0, how0, tot0 = engine.pair_host(s.flat, a[:0], b[:0])
    assert len(P0) == 0 and len(how0) == 0 and int(tot0["n_pairs"]) == 0
    ca, cb = a.copy(), b.copy()
    ca["pad_"], cb["pad_"] = 0, 0
    pr.assert_pairs_equal(engine.pair_host(s.flat, ca, cb), ref[0], "padding")
    for bad in (4, 8, 1 << 31):
        with pytest.raises(engine.ClsError) as e:
            engine.pair_host(s.flat, a, b, bad)
        assert e.value.code == -1


def test_invariants(case):
    name, s, a, b, ref, tree = case
    P0, how0, tot0 = engine.pair_host(s.flat, a, b, 0)
    for flags in ALL_FLAGS:
        P, how, tot = engine.pair_host(s.flat, a, b, flags)
        assert (how == how0).all(), "how depends on the flags"
        assert int(tot["how_count"].sum()) == int(tot["n_pairs"]) == len(a) and int(tot["how_count"][7]) == 0
        assert not P["pad_"].any()
    Pc, _, _ = engine.pair_host(s.flat, a, b, _abi.PAIR_CONSERVATIVE)
    for i in np.nonzero(how0 >= _abi.PAIR_SAME)[0]:  # both mates usable: P names a clade in both modes
        x, y = tree.row_of[int(Pc["clade_id"][i])], tree.row_of[int(P0["clade_id"][i])]
        assert tree.holds(x, y), f"pair {i}: the default clade is not at or below the conservative one"
    others = how0 < _abi.PAIR_SAME
    assert (P0["clade_id"][others] == Pc["clade_id"][others]).all()
    # REQUIRE_BOTH leaves the ONLY classes unplaced
    Pr, _, _ = engine.pair_host(s.flat, a, b, _abi.PAIR_REQUIRE_BOTH)
    only = (how0 == _abi.PAIR_ONLY_1) | (how0 == _abi.PAIR_ONLY_2)
    placed = np.isin(Pr["status"], pr.USABLE) & np.isin(Pr["clade_id"], s.flat.nodes["id"])
    assert not placed[only].any() and placed[how0 >= _abi.PAIR_SAME].all()
    # totals are associative over batches: cls_pair_host adds to the totals it is given
    nodes = np.ascontiguousarray(s.flat.nodes, dtype=_abi.NODE_DTYPE)
    acc = np.zeros(1, dtype=_abi.PAIR_TOTALS_DTYPE)
    cuts = [0, len(a) // 3, len(a) // 3 + 1, len(a)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        pa, pb = np.ascontiguousarray(a[lo:hi]), np.ascontiguousarray(b[lo:hi])
        out = np.zeros(hi - lo, dtype=_abi.PLACEMENT_DTYPE)
        rc = engine.lib().cls_pair_host(nodes.ctypes.data, len(nodes), pa.ctypes.data, pb.ctypes.data, 1, hi - lo, 0, out.ctypes.data, None,
                                        acc.ctypes.data)
        assert rc == 0
        pr.assert_pairs_equal((out, None), (P0[lo:hi], None), "part")
    pr.assert_totals_equal(acc, tot0, "sum of the parts' totals")


# ---- records of simulated read pairs, placed by the oracle port --------------------------------------------------------

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def simulated_pairs(s, n, seed, short2=0.15, short1=0.10, other_leaf=0.15, sub_rate=0.03, read_len=150):
    """-> (reads1, reads2): mate 1 is a window of a leaf sequence; mate 2 the reverse complement of a later window of the
    same leaf.  A share `short2` of the mate 2s and `short1` of the mate 1s is cut below k (the two overlap by chance);
    a share `other_leaf` of the mate 2s is drawn from a different leaf; bases are substituted at `sub_rate`; mate 2s of
    every length from k up occur, so the two mates need not resolve to the same depth."""
    rng = np.random.default_rng(seed)
    k = int(s.flat.k_size)
    seqs = [s.leaf_seq(i).encode() for i in range(s.n_leaves)]
    r1, r2 = [], []
    for _ in range(n):
        leaf = int(rng.integers(0, s.n_leaves))
        ref = seqs[leaf]
        p1 = int(rng.integers(0, len(ref) - 3 * read_len))
        p2 = p1 + int(rng.integers(read_len // 2, 2 * read_len))
        src2 = seqs[int(rng.integers(0, s.n_leaves))] if rng.random() < other_leaf else ref
        len2 = int(rng.integers(k, read_len + 1))
        m1 = bytearray(ref[p1:p1 + read_len])
        m2 = bytearray(src2[p2:p2 + len2])
        for m in (m1, m2):
            for j in np.nonzero(rng.random(len(m)) < sub_rate)[0]:
                m[j] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < short1:
            m1 = m1[:int(rng.integers(0, k))]
        if rng.random() < short2:
            m2 = m2[:int(rng.integers(0, k))]
        r1.append(bytes(m1))
        r2.append(bytes(m2).translate(COMP)[::-1])
    return r1, r2


def pack_reads(reads):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8), off


@pytest.fixture(scope="module")
def oracle_pairs():
    s = SynthDb(64, 3000, 12, 4)
    r1, r2 = simulated_pairs(s, 1500, seed=11)
    oracle = op.OraclePort(s.flat)
    a = oracle.place_batch(*pack_reads(r1), op.make_params(), threads=8)
    b = oracle.place_batch(*pack_reads(r2), op.make_params(), threads=8)
    return s, a, b


def test_oracle_pairs_cover_the_classes(oracle_pairs):
    """The shares of simulated_pairs are chosen so that the reference alone yields SAME, a NESTED class, both ONLY classes
    and NEITHER (asserted from pair_ref)."""
    s, a, b = oracle_pairs
    _, how, _ = pr.pair_ref(s.flat.nodes, a, b)
    counts = np.bincount(how, minlength=8)
    assert counts[_abi.PAIR_SAME] > 0 and counts[_abi.PAIR_ONLY_1] > 0 and counts[_abi.PAIR_ONLY_2] > 0 and counts[_abi.PAIR_NEITHER] > 0, counts
    assert counts[_abi.PAIR_NESTED_1] + counts[_abi.PAIR_NESTED_2] > 0, counts


def test_host_equals_reference_on_oracle_pairs(oracle_pairs):
    s, a, b = oracle_pairs
    tree = pr.TreeIndex(s.flat.nodes)
    for flags in ALL_FLAGS:
        want = pr.pair_ref(s.flat.nodes, a, b, flags, tree)
        pr.assert_pairs_equal(engine.pair_host(s.flat, a, b, flags), want, f"oracle pairs, flags {flags}")
        pr.assert_pairs_equal(engine.pair_host(s.flat, interleave(a, b), None, flags), want, f"oracle pairs interleaved, flags {flags}")


# ---- the mate-name rule ------------------------------------------------------------------------------------------------

NAME_CASES = [
    (b"read1/1", b"read1/2", True),
    (b"read1/2", b"read1/1", True),            # the suffixes are not checked against the mate's position
    (b"read1/1", b"read1/1", True),
    (b"read1", b"read1/2", True),
    (b"read1 1:N:0:ACGT", b"read1 2:N:0:ACGT", True),
    (b"read1\tcomment one", b"read1 other", True),
    (b"read1/1 comment", b"read1/2\tcomment", True),
    (b"/1", b"/2", True),                      # a name that is only the suffix: empty names, equal
    (b"/1", b"", True),
    (b"/1", b"x/1", False),
    (b"read1", b"read10", False),              # differing lengths
    (b"read10/1", b"read1/1", False),
    (b"read1/3", b"read1", False),             # only /1 and /2 are dropped
    (b"read1/1/1", b"read1/1", False),         # dropped once
    (b"read1/", b"read1", False),
    (b">read1/1", b">read1/2", True),          # a '>' is a byte like any other
    (b">read1", b"read1", False),
    (b"re>ad 1", b"re>ad 2", True),
    (b"read1 /1", b"read1", True),
    (b" read1", b" other", True),              # the name ends at the first space: empty
    (b"Read1", b"read1", False),
]


def test_name_rule():
    for h1, h2, agree in NAME_CASES:
        assert (pr.name_of(h1) == pr.name_of(h2)) == agree, (h1, h2)
        assert engine.pair_names_host([h1], [h2]) == ((0, None) if agree else (1, 0)), (h1, h2)
        assert engine.pair_names_host([h1, h2]) == ((0, None) if agree else (1, 0)), (h1, h2)
    h1 = [c[0] for c in NAME_CASES]
    h2 = [c[1] for c in NAME_CASES]
    want = pr.pair_names_ref(h1, h2)
    assert want == (sum(1 for c in NAME_CASES if not c[2]), next(i for i, c in enumerate(NAME_CASES) if not c[2]))
    assert engine.pair_names_host(h1, h2) == want
    inter = [h for pair in zip(h1, h2) for h in pair]
    assert engine.pair_names_host(inter) == want
    # the first disagreeing index is reported, wherever it is
    rng = np.random.default_rng(3)
    good = [(b"r%d/1 x" % i, b"r%d/2" % i) for i in range(300)]
    for at in (0, 1, 137, 299):
        g1, g2 = [x for x, _ in good], [y for _, y in good]
        g2[at] = b"other/2"
        if at < 200:
            g2[250] = b"late/2"
        assert engine.pair_names_host(g1, g2) == pr.pair_names_ref(g1, g2) == (2 if at < 200 else 1, at)
    assert engine.pair_names_host([], []) == (0, None)
    swapped = [y for _, y in good]
    j = int(rng.integers(0, 299))
    swapped[j], swapped[j + 1] = swapped[j + 1], swapped[j]
    assert engine.pair_names_host([x for x, _ in good], swapped) == (2, j)
