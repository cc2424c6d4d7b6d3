"""CPU: pin the oracle (murmur KATs from the reference docs), and check the C
port against the literal restatement record for record."""
import numpy as np
import pytest

from classeq2_amd.synth import SynthDb
from oracle import oracle_literal as lit
from oracle import oracle_port as op
from tests.helpers import ODD_PARAM_SETS, PARAM_SETS, drop_random_nodes, ragged_reads, records_equal

# Known answers printed in the reference's own docs (docs/book/02-build-db.md:181-196):
# minimizer keys + k-mer hashes of the bsub-gyrB model (k=35, m=4); the two
# 35-mers occur in tests/data/public/.../input/*.fasta of the reference.
KATS = [
    (b"CCAA", 10631256518523097406),
    (b"ATAC", 10517626403121597142),
    (b"CCAAAGCCAGGCTTGCAGCGTTATAAAGGTCTTGG", 15277858258350234285),
    (b"ATACAATGACAAGGAGCTTGAAGAACTGTTAAAAA", 13045666331085307167),
    (b"", 0),                          # MinimizerKey(0) for mSize == 0, kmers_map.rs:131-134
    (b"hello", 0xCBD8A7B341BD9B02),    # public MurmurHash3_x64_128 vector
]


@pytest.mark.parametrize("data,want", KATS)
def test_murmur_kat(data, want):
    assert lit.murmurhash3_x64_128(data, 0)[0] == want
    assert op.lib().cls_oracle_murmur3_h1(data, len(data)) == want


def test_murmur_c_vs_literal_all_lengths():
    rng = np.random.default_rng(0)
    for n in range(0, 70):
        data = bytes(rng.integers(65, 91, size=n, dtype=np.uint8))
        assert op.lib().cls_oracle_murmur3_h1(data, n) == lit.murmurhash3_x64_128(data, 0)[0]


def test_rust_round_and_debug():
    assert lit.rust_round(0.5) == 1.0 and lit.rust_round(1.5) == 2.0 and lit.rust_round(2.4999) == 2.0
    assert lit.rust_round(0.49999999999999994) == 0.0
    assert lit.rust_debug_header('a"b\\c\n') == 'SequenceHeader("a\\"b\\\\c\\n")'


CASES = [
    (40, 200, 6, 3, 0.0, 1, 0, 60),
    (60, 300, 8, 4, 0.3, 3, 7, 80),
    (100, 300, 10, 4, 0.5, 1, 0, 100),
    (30, 120, 5, 0, 0.5, 5, 100, 40),
    (50, 200, 7, 9, 0.0, 1, 0, 20),
]


@pytest.mark.parametrize("case", CASES)
def test_port_matches_literal(case):
    nl, rl, k, m, cp, stride, off, rdlen = case
    s = SynthDb(nl, rl, k, m, collapse_prob=cp, id_stride=stride, id_offset=off)
    tree = op.flat_to_literal(s.flat)
    port = op.OraclePort(s.flat)
    bases, offsets, _ = s.reads(150, rdlen, frac_random=0.05, err=0.02)
    for kw in PARAM_SETS + (ODD_PARAM_SETS if nl == 60 else []):
        want = op.literal_place_batch(tree, bases, offsets, **kw)
        got = port.place_batch(bases, offsets, op.make_params(**kw), threads=2)
        assert len(records_equal(got, want)) == 0, kw


def test_port_matches_literal_sets_with_nothing_below_the_root():
    """Node sets {root} and {}: counted in |M| (and |M_root|), never a vote."""
    from tests.helpers import truncate_random_sets

    s = SynthDb(60, 300, 9, 4)
    flat = truncate_random_sets(s.flat, 0.15, seed=4)
    tree = op.flat_to_literal(flat)
    port = op.OraclePort(flat)
    bases, offsets, _ = s.reads(150, 110, frac_random=0.05, err=0.02)
    for kw in (dict(), dict(min_match_coverage=1.0)):
        want = op.literal_place_batch(tree, bases, offsets, **kw)
        got, st = port.place_batch(bases, offsets, op.make_params(**kw), threads=2, want_stats=True)
        assert len(records_equal(got, want)) == 0, kw
    assert (st["n_matched"] > st["n_with_root"]).any()


def test_port_matches_literal_non_closed_and_ragged():
    s = SynthDb(60, 300, 8, 4, collapse_prob=0.3)
    flat = drop_random_nodes(s.flat, 0.2, seed=3)
    tree = op.flat_to_literal(flat)
    port = op.OraclePort(flat)
    bases, offsets = ragged_reads(np.random.default_rng(1), s, 150, 0, 120)
    bases = bases.copy()
    bases[int(offsets[5]) + 3] = ord("N")
    want = op.literal_place_batch(tree, bases, offsets)
    got = port.place_batch(bases, offsets)
    assert len(records_equal(got, want)) == 0
    # trace counters of the literal oracle vs the port's stats
    got, st = port.place_batch(bases, offsets, want_stats=True)
    raw = bytes(bases)
    for i in range(0, 150, 7):
        tr = lit.Trace()
        try:
            lit.place_sequence(f"r{i}", raw[int(offsets[i]):int(offsets[i + 1])].decode(), tree, trace=tr)
        except (lit.PlaceError, ValueError):
            continue
        assert (tr.n_query_kmers, tr.query_kmers_len) == (st[i]["n_query_kmers"], st[i]["n_matched"])


def test_duplicate_hash_across_buckets_semantics():
    """A hash present under two buckets: |M| counts both entries, K_c counts the
    hash once (kmers_map.rs:189-203 flattens into one HashSet)."""
    root = dict(id=0, parent=None, kind="ROOT", children=[
        dict(id=1, parent=0, kind="NODE", children=[dict(id=3, parent=1, kind="LEAF"), dict(id=4, parent=1, kind="NODE", children=[dict(id=6, parent=4, kind="LEAF")])]),
        dict(id=2, parent=0, kind="NODE", children=[dict(id=5, parent=2, kind="LEAF")]),
    ])
    from classeq2_amd.flatdb import FlatDb
    seq = "ACGTTGCA"
    k, m = 4, 2
    km = lit.KmersMap(k, m)
    for kmer, h in km.build_kmer_from_string(seq):
        km.insert_or_append_kmer_hash(kmer, h, {0, 1, 4})
    # plant the hash of "ACGT" under the bucket of "TG" as well, with another node set
    h_acgt = lit.hash_kmer("ACGT")
    km.map.setdefault(lit.hash_kmer("TG"), {})[h_acgt] = {0, 2}
    flat = FlatDb.from_nested(root, k, m, km.map)
    tree = op.flat_to_literal(flat)
    bases = np.frombuffer(seq.encode(), dtype=np.uint8)
    offsets = np.array([0, len(seq)], dtype=np.uint64)
    want = op.literal_place_batch(tree, bases, offsets)
    got, st = op.OraclePort(flat).place_batch(bases, offsets, want_stats=True)
    assert len(records_equal(got, want)) == 0
    tr = lit.Trace()
    lit.place_sequence("q", seq, tree, trace=tr)
    assert st[0]["n_matched"] == tr.query_kmers_len


def test_fasta_literal_semantics():
    txt = ">a b>c\nACGTnnacgt\r\n\n>second\n\n>third\nNNNN\n>z\nGG"
    recs = lit.sequence_content_by_channel(txt)
    assert recs == [("a bc", "ACGTACGT"), ("second", ""), ("third", ""), ("z", "GG")]
    assert lit.sequence_content_by_channel("ACGT\n>h\nAC\n") == []  # sequence before any header -> error, nothing sent


@pytest.mark.parametrize("case", [(60, 300, 8, 4, 0.0, 0), (80, 300, 10, 4, 0.4, 0), (120, 400, 12, 4, 0.0, 1), (50, 200, 17, 4, 0.3, 1)])
def test_leaves_only_oracle_equals_explicit_oracle(case):
    """CLS_SETS_LEAVES input (include/cls_place.h): the C oracle keeps such node sets lazily (a clade is a member iff
    a listed leaf lies below it).  Held to the explicit-set oracle -- the restatement of the reference -- on the same
    indexes: generated both ways, and derived from the explicit one by filtering on kind; records and counters."""
    nl, rl, k, m, cp, deep = case
    s = SynthDb(nl, rl, k, m, collapse_prob=cp, deep=deep)
    t = SynthDb(nl, rl, k, m, collapse_prob=cp, deep=deep, tips_only=True)
    assert t.flat.leaves_only and not s.flat.leaves_only
    derived = s.flat.to_leaves_only()
    assert np.array_equal(t.flat.kmer_hash, s.flat.kmer_hash) and np.array_equal(t.flat.kmer_node_off, derived.kmer_node_off)
    for j in range(0, s.flat.n_kmers, 97):  # same leaves per k-mer (any order)
        a, b = int(derived.kmer_node_off[j]), int(derived.kmer_node_off[j + 1])
        assert sorted(t.flat.node_ids[a:b]) == sorted(derived.node_ids[a:b])
    back = t.flat.to_explicit()
    for j in range(0, s.flat.n_kmers, 211):
        a, b = int(s.flat.kmer_node_off[j]), int(s.flat.kmer_node_off[j + 1])
        c, d = int(back.kmer_node_off[j]), int(back.kmer_node_off[j + 1])
        assert sorted(s.flat.node_ids[a:b]) == sorted(back.node_ids[c:d])
    bases, offsets, _ = s.reads(400, min(rl, 150), frac_random=0.05, err=0.02)
    for kw in (dict(), dict(remove_intersection=True), dict(min_match_coverage=1.0), dict(max_iterations=3)):
        want, wst = op.OraclePort(s.flat).place_batch(bases, offsets, op.make_params(**kw), threads=4, want_stats=True)
        for flat in (t.flat, derived):
            got, gst = op.OraclePort(flat).place_batch(bases, offsets, op.make_params(**kw), threads=4, want_stats=True)
            for f in ("status", "one", "rest", "levels", "clade_id"):
                assert (got[f] == want[f]).all(), (f, kw)
            for f in ("n_query_kmers", "n_matched", "n_with_root", "leaf_postings"):
                assert (gst[f] == wst[f]).all(), (f, kw)


# ---- foreign buckets: entries filed under a bucket that is not their own prefix's --------------------------------------
# kmers_map.rs:279-297 keeps a hit if its bucket's key is the minimizer of SOME query k-mer (either strand, k-mer start
# positions only), not necessarily the hit's own.  The GPU tests (tests/test_gpu_foreign_buckets.py) hold the kernels to
# the C port on such indexes; these pin the C port to the literal restatement there.

def _node_sets_by_hash(flat):
    off = flat.kmer_node_off.astype(np.int64)
    return {int(h): sorted(flat.node_ids[off[j]:off[j + 1]].tolist()) for j, h in enumerate(flat.kmer_hash)}


def test_refile_helpers_keep_every_entry():
    from tests.helpers import drop_kmers, foreign_refile, kmer_bucket_index, kmers_inside_clade, clade_with_leaves, split_buckets

    s = SynthDb(30, 300, 12, 7)
    flat = s.flat
    move = kmers_inside_clade(flat, clade_with_leaves(flat, 5, 10)) & (np.random.default_rng(1).random(flat.n_kmers) < 0.3)
    g, moved = foreign_refile(flat, move, seed=2)
    assert moved.sum() > 100 and not (moved & ~move).any()
    assert _node_sets_by_hash(g) == _node_sets_by_hash(flat) and len(np.unique(g.kmer_hash)) == g.n_kmers
    key_of = dict(zip(g.kmer_hash.tolist(), g.bucket_key[kmer_bucket_index(g)].tolist()))
    own = flat.bucket_key[kmer_bucket_index(flat)]
    assert all(key_of[int(h)] != int(k) for h, k in zip(flat.kmer_hash[moved], own[moved]))
    assert all(key_of[int(h)] == int(k) for h, k in zip(flat.kmer_hash[~moved], own[~moved]))
    assert len(np.unique(g.bucket_key)) == len(g.bucket_key)
    d = drop_kmers(flat, moved)
    assert d.n_kmers == flat.n_kmers - moved.sum() and not np.isin(d.kmer_hash, flat.kmer_hash[moved]).any()
    sp = split_buckets(flat, 20, seed=3)
    assert len(sp.bucket_key) == len(flat.bucket_key) + 20 and _node_sets_by_hash(sp) == _node_sets_by_hash(flat)
    lo = foreign_refile(flat.to_leaves_only(), move, seed=2)[0]
    assert lo.leaves_only and _node_sets_by_hash(lo.to_explicit()) == _node_sets_by_hash(g)


def _foreign_index(k, m, variant, n_leaves=30, ref_len=300, seed=2):
    """A small SynthDb index with ~30 % of the k-mers of one clade refiled under foreign keys."""
    from tests.helpers import clade_with_leaves, foreign_refile, kmers_inside_clade, split_buckets

    s = SynthDb(n_leaves, ref_len, k, m)
    flat = split_buckets(s.flat, 40, seed=seed) if variant == "dup" else s.flat
    move = kmers_inside_clade(flat, clade_with_leaves(flat, n_leaves // 6, n_leaves // 2)) & (np.random.default_rng(seed).random(flat.n_kmers) < 0.3)
    refiled, moved = foreign_refile(flat, move, seed=seed, unhashed_frac=1.0 if variant == "unhashed" else 0.3)
    if variant == "leaves":
        refiled = foreign_refile(flat.to_leaves_only(), move, seed=seed, unhashed_frac=0.3)[0]
    return s, flat, refiled, moved


@pytest.mark.parametrize("k,m,variant", [(10, 0, "mixed"), (12, 4, "mixed"), (12, 7, "mixed"), (12, 8, "dup"), (12, 10, "mixed"),
                                         (10, 11, "mixed"), (12, 7, "unhashed"), (17, 10, "dup"), (12, 7, "leaves")])
def test_port_matches_literal_on_foreign_buckets(k, m, variant):
    """m = 0 (one key, 0: a foreign key is never any query's minimizer), m <= 8 and 9..k (the two regimes of the kernels'
    bucket table), m > k (the minimizer is the whole k-mer's hash: a foreign key is another k-mer's), keys no m-string
    hashes to, duplicate bucket keys, a leaves-only input.  Records, and |M| against the literal trace."""
    s, flat, refiled, moved = _foreign_index(k, m, variant)
    explicit = refiled.to_explicit() if refiled.leaves_only else refiled
    tree = op.flat_to_literal(explicit)
    port = op.OraclePort(refiled)
    bases, offsets, _ = s.reads(300, 150, frac_random=0.05, err=0.02)
    for kw in (dict(), dict(remove_intersection=True), dict(min_match_coverage=1.0)):
        want = op.literal_place_batch(tree, bases, offsets, **kw)
        got, st = port.place_batch(bases, offsets, op.make_params(**kw), threads=2, want_stats=True)
        assert len(records_equal(got, want)) == 0, kw
    raw = bytes(bases)
    for i in range(0, 300, 5):
        tr = lit.Trace()
        try:
            lit.place_sequence(f"r{i}", raw[int(offsets[i]):int(offsets[i + 1])].decode(), tree, trace=tr)
        except (lit.PlaceError, ValueError):
            continue
        assert (tr.n_query_kmers, tr.query_kmers_len) == (st[i]["n_query_kmers"], st[i]["n_matched"])
    # the input is discriminating: the refiled entries change |M| against leaving them in their own bucket
    own = op.OraclePort(flat).place_batch(bases, offsets, threads=2, want_stats=True)[1]
    assert (own["n_matched"] != st["n_matched"]).mean() > 0.05


def _revcomp(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _starts(seq: str, k: int, m: int) -> set:
    """The m-prefixes of the k-mers of both strands: the query's minimizers, as strings."""
    rc = _revcomp(seq)
    return {x[i:i + m] for x in (seq, rc) for i in range(len(seq) - k + 1)}


@pytest.mark.parametrize("layout,accepted", [("rc_strand", True), ("last_k_minus_1", False), ("at_L_minus_k", True)])
def test_foreign_key_found_among_the_query_minimizers(layout, accepted):
    """Crafted reads for ONE refiled k-mer X, filed under the key of an m-string P that is not X's prefix: P is the prefix
    of a k-mer of the reverse-complement strand only (accepted); P lies inside the last k-1 bases, where no k-mer starts
    (rejected); P starts at L-k (accepted).  The read's property is checked by string search; |M| must be the own-bucket
    index's (accepted) or one less (rejected)."""
    from tests.helpers import refile_kmers

    k, m = 10, 5
    s = SynthDb(30, 300, k, m)
    flat = s.flat
    leaf = s.leaf_seq(3)
    X = leaf[100:100 + k]
    hx = lit.hash_kmer(X)
    j = int(np.nonzero(flat.kmer_hash == np.uint64(hx))[0][0])
    rng = np.random.default_rng(7)
    P = "".join("ACGT"[c] for c in rng.integers(0, 4, m))
    while P == X[:m] or P in leaf or _revcomp(P) in leaf:
        P = "".join("ACGT"[c] for c in rng.integers(0, 4, m))
    move = np.zeros(flat.n_kmers, dtype=bool)
    move[j] = True
    target = np.zeros(flat.n_kmers, dtype=np.uint64)
    target[j] = lit.hash_kmer(P)
    refiled = refile_kmers(flat, move, target)
    for attempt in range(200):
        r = np.random.default_rng(100 + attempt)
        fill = "".join("ACGT"[c] for c in r.integers(0, 4, 30))
        if layout == "rc_strand":
            read = X + fill + _revcomp(P)  # P starts the reverse complement's first k-mer
        elif layout == "last_k_minus_1":
            read = X + fill + P + fill[:k - 1 - m]  # P ends the read, inside the last k-1 bases
        else:
            read = X + fill + P + fill[:k - m]  # P starts the last forward k-mer
        L = len(read)
        fwd = {read[i:i + m] for i in range(L - k + 1)}
        rcs = {_revcomp(read)[i:i + m] for i in range(L - k + 1)}
        if read.count(X) != 1 or X in _revcomp(read):
            continue
        if layout == "rc_strand" and P in rcs and P not in fwd:
            break
        if layout == "last_k_minus_1" and P not in fwd | rcs and P in read[L - k + 1:]:
            break
        if layout == "at_L_minus_k" and [i for i in range(L - k + 1) if read[i:i + m] == P] == [L - k] and P not in rcs:
            break
    else:
        raise AssertionError("no read with the intended property")
    assert (P in _starts(read, k, m)) == accepted
    bases = np.frombuffer(read.encode(), dtype=np.uint8)
    offsets = np.array([0, L], dtype=np.uint64)
    n = {}
    for tag, f in (("refiled", refiled), ("own", flat)):
        tr = lit.Trace()
        lit.place_sequence("q", read, op.flat_to_literal(f), trace=tr)
        got, st = op.OraclePort(f).place_batch(bases, offsets, want_stats=True)
        assert len(records_equal(got, op.literal_place_batch(op.flat_to_literal(f), bases, offsets))) == 0
        assert st[0]["n_matched"] == tr.query_kmers_len
        n[tag] = tr.query_kmers_len
    assert n["refiled"] == (n["own"] if accepted else n["own"] - 1)
