"""GPU parity on indexes with entries filed under a bucket that is not their own prefix's ("foreign" buckets).

The reference keeps a hit if its bucket's key is the minimizer of SOME query k-mer -- either strand, k-mer start
positions only (kmers_map.rs:279-297).  `cls build-db` files every k-mer under its own prefix's key, but the C-ABI takes
any DB file, and every kernel family has its own code for the other case: the generic front's wave-wide search, the
hashed wave-per-read front (with and without the bucket table), the LDS-tiled kernel's spill to the workspace kernel,
and the encoder, which drops the direct table when any entry is foreign.  Each case asserts the path it reaches, and that
its input is discriminating: the oracle on the refiled index differs from the oracle on the index with the entries left
in their own bucket (a kernel that skips the filter) and with the entries deleted (a kernel that never accepts a
foreign entry).
"""
import numpy as np
import pytest

from classeq2_amd import engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests.helpers import (clade_with_leaves, describe, device_place, drop_kmers, drop_random_nodes, foreign_refile, kmers_inside_clade,
                           ragged_reads, records_equal, split_buckets, stats_equal)

pytestmark = pytest.mark.gpu

KWS = (dict(), dict(remove_intersection=True), dict(min_match_coverage=1.0))
_COMP = np.arange(256, dtype=np.uint8)
for a, b in (b"AT", b"TA", b"CG", b"GC", b"at", b"ta", b"cg", b"gc"):
    _COMP[a] = b


def _check(flat, bases, offsets, kw, threads=16, device=False, want=None):
    """Records and the four counters against the oracle (or `want`: its records and counters, computed before), stats and
    non-stats kernels (and the device-buffer entry)."""
    with engine.PlacementDb(flat, device=0) as db:
        got, gst = db.place_batch(bases, offsets, engine.make_params(**kw), want_stats=True)
        got2 = db.place_batch(bases, offsets, engine.make_params(**kw))
        if device:
            db.set_max_read_len(int(np.diff(offsets.astype(np.int64)).max()))
            dev, dst = device_place(db, bases, offsets, engine.make_params(**kw))
    want, wst = want or op.OraclePort(flat).place_batch(bases, offsets, op.make_params(**kw), threads=threads, want_stats=True)
    bad = records_equal(got, want)
    assert len(bad) == 0, f"{len(bad)} records differ, first {bad[0]}: got {describe(got[bad[0]])} want {describe(want[bad[0]])}"
    assert len(records_equal(got, got2)) == 0, "stats and non-stats kernels disagree"
    sb = stats_equal(gst, wst)
    assert len(sb) == 0, f"{len(sb)} stats differ, first {sb[0]}: got {gst[sb[0]]} want {wst[sb[0]]}"
    if device:
        assert len(records_equal(dev, want)) == 0 and len(stats_equal(dst, wst)) == 0, "device-buffer entry"
    return got, gst


def _check_all(flat, bases, offsets, threads=16, device=False):
    return {tuple(kw): _check(flat, bases, offsets, kw, threads, device and not kw) for kw in KWS}


def _sensitive(flat, refiled, moved, bases, offsets, reject_only=False, threads=16):
    """The oracle on the refiled index against (a) the entries left in their own bucket and (b) the entries deleted:
    each differs in |M| on >= 5 % of the reads and in some records.  Entries that can only be rejected (m = 0, keys no
    m-string hashes to) equal (b) by construction."""
    want, wst = op.OraclePort(refiled).place_batch(bases, offsets, threads=threads, want_stats=True)
    n_matched = []
    for tag, base in (("own bucket", flat), ("deleted", drop_kmers(flat, moved))):
        rec, st = op.OraclePort(base).place_batch(bases, offsets, threads=threads, want_stats=True)
        n_matched.append(st["n_matched"])
        frac, n_rec = float((st["n_matched"] != wst["n_matched"]).mean()), len(records_equal(rec, want))
        if reject_only and tag == "deleted":
            assert frac == 0.0 and n_rec == 0, "entries under a key no query minimizer can match were accepted"
        else:
            assert frac >= 0.05 and n_rec > 0, f"not discriminating against the index with the entries {tag}: |M| on {frac:.1%}, {n_rec} records"
    return n_matched


def _refiled(s, frac, seed, leaves=(0.15, 0.4), unhashed_frac=0.3, base=None):
    """`frac` of the k-mers of one clade (leaves[0]..leaves[1] of the tree's leaves) refiled under foreign keys."""
    flat = s.flat if base is None else base
    n = int(s.n_leaves)
    move = kmers_inside_clade(flat, clade_with_leaves(flat, int(leaves[0] * n), int(leaves[1] * n)))
    move &= np.random.default_rng(seed).random(flat.n_kmers) < frac
    refiled, moved = foreign_refile(flat, move, seed=seed, unhashed_frac=unhashed_frac)
    return flat, refiled, moved


def _revcomp_batch(bases, offsets):
    """Every read reverse-complemented; read i of the result is read n-1-i's reverse complement."""
    o = offsets.astype(np.int64)
    return _COMP[bases[o[0]:o[-1]][::-1]], (o[-1] - o[::-1]).astype(np.uint64)


def _strand_symmetric(flat, bases, offsets, want):
    """The reference's k-mer set (and its minimizers) is the same for a read and its reverse complement."""
    rb, ro = _revcomp_batch(bases, offsets)
    with engine.PlacementDb(flat, device=0) as db:
        got, st = db.place_batch(rb, ro, want_stats=True)
    assert len(records_equal(got[::-1].copy(), want)) == 0, "a read and its reverse complement are placed differently"


def _info(flat):
    with engine.PlacementDb(flat, device=0) as db:
        return db.info, db.kernel_name()


def _own_direct_table(flat):
    """The index with every entry in its own bucket has a direct table: the refiled entries are what turn it off."""
    info, _ = _info(flat)
    assert info.direct_table != 0


@pytest.mark.parametrize("k,m", [(12, 7), (21, 6)])
def test_hashed_fast_front_with_bucket_table(k, m):
    """Wave-per-read kernel, MurmurHash3 front with the bucket table (m_eff <= 8, distinct keys), binary tree; both strands
    of every read, the device-buffer entry."""
    s = SynthDb(150, 600, k, m)
    flat, refiled, moved = _refiled(s, 0.3, seed=k)
    if k <= 15:
        _own_direct_table(flat)
    info, name = _info(refiled)
    assert (info.format, info.binary_tree, info.direct_table) == (1, 1, 0)
    assert len(np.unique(refiled.bucket_key)) == len(refiled.bucket_key) and min(m, k) <= 8  # (the bucket table's conditions)
    assert name.startswith("place_fast_kernel<") and name.endswith(", 2, false>"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    got = _check_all(refiled, bases, offsets, device=True)
    _strand_symmetric(refiled, bases, offsets, got[()][0])


@pytest.mark.parametrize("k,m,dup", [(17, 10, False), (12, 7, True)])
def test_hashed_fast_front_without_bucket_table(k, m, dup):
    """The same kernel comparing bucket keys: m_eff > 8, or two buckets with the same key."""
    s = SynthDb(150, 600, k, m)
    base = split_buckets(s.flat, 200, seed=3) if dup else None
    flat, refiled, moved = _refiled(s, 0.3, seed=k, base=base)
    info, name = _info(refiled)
    assert (info.format, info.binary_tree, info.direct_table) == (1, 1, 0)
    assert min(m, k) > 8 or len(np.unique(refiled.bucket_key)) < len(refiled.bucket_key)
    assert name.startswith("place_fast_kernel<") and name.endswith(", 2, false>"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    got = _check_all(refiled, bases, offsets)
    _strand_symmetric(refiled, bases, offsets, got[()][0])


def test_polytomy_fast_kernel():
    s = SynthDb(150, 600, 12, 7, collapse_prob=0.4)
    flat, refiled, moved = _refiled(s, 0.3, seed=5)
    _own_direct_table(flat)
    info, name = _info(refiled)
    assert (info.format, info.binary_tree, info.direct_table) == (1, 0, 0)
    assert name.startswith("place_fast_kernel<") and name.endswith(", 2, true>"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    _check_all(refiled, bases, offsets)


@pytest.mark.parametrize("collapse", [0.0, 0.4])
def test_generic_split_kernel(collapse):
    """Knob `no_fast`: the generic wave-per-read kernel on split records (its wave-wide search for the foreign key)."""
    s = SynthDb(150, 600, 12, 7, collapse_prob=collapse)
    flat, refiled, moved = _refiled(s, 0.3, seed=6)
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    engine.set_tuning("no_fast", 1)
    try:
        info, name = _info(refiled)
        assert info.format == 1 and info.direct_table == 0 and name.startswith("place_split_kernel<"), name
        _check_all(refiled, bases, offsets)
    finally:
        engine.set_tuning("no_fast", 0)


def test_generic_list_kernel():
    """Node sets not closed under `parent` (sorted lists, FMT_LIST) composed with refiling: place_wave_kernel."""
    s = SynthDb(150, 600, 12, 7, collapse_prob=0.3)
    flat, refiled, moved = _refiled(s, 0.3, seed=7, base=drop_random_nodes(s.flat, 0.1, seed=7))
    info, name = _info(refiled)
    assert info.format == 0 and name.startswith("place_wave_kernel<"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    _check_all(refiled, bases, offsets)


@pytest.mark.parametrize("k,collapse", [(12, 0.0), (21, 0.4)])
def test_gene_length_reads(k, collapse):
    """Reads of 600..3500 bp: the LDS-tiled kernel's hashed front (a foreign hit spills the read to the workspace kernel),
    and with knob `no_tile` the workgroup-per-read kernel; same records."""
    s = SynthDb(120, 4000, k, 7, collapse_prob=collapse)
    flat, refiled, moved = _refiled(s, 0.03, seed=8)
    rng = np.random.default_rng(21)
    bases, offsets = ragged_reads(rng, s, 100, 600, 3500, lower_frac=0.05)
    _sensitive(flat, refiled, moved, bases, offsets)
    engine.set_tuning("time_class", 2)  # (cls_db_kernel_name then names the kernel of the reads of 513..4096 + k - 1 bases)
    try:
        with engine.PlacementDb(refiled, device=0) as db:
            assert db.info.format == 1 and db.info.direct_table == 0
            db.set_max_read_len(3500)
            assert db.kernel_name().startswith("place_tile_kernel<") and ", 2, " in db.kernel_name(), db.kernel_name()
            engine.set_tuning("no_tile", 1)
            assert db.kernel_name().startswith("place_block_kernel<"), db.kernel_name()
    finally:
        engine.set_tuning("time_class", 0)
        engine.set_tuning("no_tile", 0)
    got = _check_all(refiled, bases, offsets)
    engine.set_tuning("no_tile", 1)
    try:
        for kw in KWS:
            _check(refiled, bases, offsets, kw, want=got[tuple(kw)])
    finally:
        engine.set_tuning("no_tile", 0)


@pytest.mark.parametrize("k,m", [(15, 7), (21, 10)])
def test_long_reads_tile_kernel_spills_to_the_workspace_kernel(k, m):
    """Reads of 4..10 kb, a few % of one clade's k-mers refiled: the reads that meet one spill from the LDS-tiled kernel
    to the workspace kernel (its serial search over all k-mers), the others stay.  Same records with the tiled kernel
    off, with one pass into a small set and with passes over hash partitions; both strands of every read."""
    s = SynthDb(150, 11000, k, m, deep=1)
    flat, refiled, moved = _refiled(s, 0.02, seed=k, leaves=(0.2, 0.45))
    if k <= 15:
        _own_direct_table(flat)
    rng = np.random.default_rng(46 + k)
    bases, offsets = ragged_reads(rng, s, 40, 4200, 10000, lower_frac=0.05)
    own, deleted = _sensitive(flat, refiled, moved, bases, offsets)
    meets = own != deleted
    assert 0.1 < meets.mean() < 0.9, "the batch must mix reads that meet refiled entries with reads that do not"
    with engine.PlacementDb(refiled, device=0) as db:
        assert (db.info.format, db.info.binary_tree, db.info.direct_table) == (1, 1, 0)
        db.set_max_read_len(10000)
        assert db.kernel_name().startswith("place_tile_kernel<") and ", 2, " in db.kernel_name(), db.kernel_name()
    got = _check_all(refiled, bases, offsets)
    _strand_symmetric(refiled, bases, offsets, got[()][0])
    engine.set_tuning("no_tile", 1)
    try:
        _check(refiled, bases, offsets, {}, want=got[()])
    finally:
        engine.set_tuning("no_tile", 0)
    for pass_codes, set_words in ((1 << 30, 4096), (1024, 4096)):
        engine.set_tuning("tile_pass_codes", pass_codes)
        engine.set_tuning("tile_set_words", set_words)
        try:
            _check(refiled, bases, offsets, {}, want=got[()])
        finally:
            engine.set_tuning("tile_pass_codes", 0)
            engine.set_tuning("tile_set_words", 0)


def test_locality_ordered_batch():
    """>= 4096 reads: the key kernels and the ordered walk on the hashed front; same records with knob `no_order`."""
    s = SynthDb(300, 900, 12, 7)
    flat, refiled, moved = _refiled(s, 0.3, seed=9)
    _own_direct_table(flat)
    info, name = _info(refiled)
    assert info.direct_table == 0 and name.startswith("place_fast_kernel<") and ", 2, " in name, name
    rng = np.random.default_rng(17)
    bases, offsets = ragged_reads(rng, s, 5000, 60, 480, lower_frac=0.02)
    assert len(offsets) - 1 >= 4096
    _sensitive(flat, refiled, moved, bases, offsets)
    got = {tuple(kw): _check(refiled, bases, offsets, kw) for kw in KWS[:2]}
    engine.set_tuning("no_order", 1)
    try:
        _check(refiled, bases, offsets, {}, want=got[()])
    finally:
        engine.set_tuning("no_order", 0)


@pytest.mark.parametrize("k,m", [(10, 0), (10, 11)])
def test_minimizer_length_extremes(k, m):
    """m = 0: every minimizer is key 0, so an entry under any other key is always rejected.  m > k: the minimizer is the
    whole k-mer's hash, so a foreign key is another k-mer's hash (accepted when that k-mer is in the read)."""
    s = SynthDb(150, 600, k, m)
    flat, refiled, moved = _refiled(s, 0.3, seed=10, unhashed_frac=0.1)
    _own_direct_table(flat)
    info, name = _info(refiled)
    assert (info.format, info.binary_tree, info.direct_table) == (1, 1, 0)
    assert name.startswith("place_fast_kernel<") and name.endswith(", 2, false>"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets, reject_only=m == 0)
    got = _check_all(refiled, bases, offsets)
    _strand_symmetric(refiled, bases, offsets, got[()][0])


def test_keys_no_m_string_hashes_to():
    """Every refiled entry under a key that is no bucket's and no m-string's hash (key 0 among them): always rejected."""
    s = SynthDb(150, 600, 12, 7)
    flat, refiled, moved = _refiled(s, 0.3, seed=11, unhashed_frac=1.0)
    info, name = _info(refiled)
    assert info.direct_table == 0 and name.startswith("place_fast_kernel<"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets, reject_only=True)
    _check_all(refiled, bases, offsets)


def test_leaves_only_input():
    """CLS_SETS_LEAVES input, refiled."""
    s = SynthDb(150, 600, 12, 7)
    flat, refiled, moved = _refiled(s, 0.3, seed=12, base=s.flat.to_leaves_only())
    assert refiled.leaves_only
    info, name = _info(refiled)
    assert (info.format, info.direct_table) == (1, 0) and name.startswith("place_fast_kernel<"), name
    bases, offsets, _ = s.reads(1500, 150, frac_random=0.05, err=0.02)
    _sensitive(flat, refiled, moved, bases, offsets)
    _check_all(refiled, bases, offsets)
