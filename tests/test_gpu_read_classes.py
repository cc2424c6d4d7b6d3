"""Reads at every read-length class boundary, on every index shape, against the oracle.

A batch is binned by k-mer count (nk = 2(L - k + 1)) into up to eight read-length classes (classify_kernel), each with a
kernel and LDS / workspace sized for the longest read it may get.  A read of exactly `cap` k-mers is the largest one a
class's buffers must hold, `cap + 2` the smallest one the next class gets.  The limits come from
PlacePlan::class_caps through PlacementDb.read_classes(); the hard-coded ones below keep that introspection honest.
"""
import contextlib

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests.helpers import describe, device_place, drop_random_nodes, records_equal, stats_equal, truncate_random_sets

pytestmark = pytest.mark.gpu

# Every host batch holds one read of N_MAX bases: the host entry plans each chunk from its longest read, and the LDS-tiled
# kernel's limits depend on that plan.  16 000 bases are beyond the whole-CU LDS on every shape (the workspace kernel is
# in the plan too), so the host entry's limits are read_classes(N_MAX).
N_MAX = 16000
REF_LEN = N_MAX + 100
N_LEAVES = 64
# device entry: cls_db_set_max_read_len(n) with 2n at c - 2, c and c + 2 around 320, 1024 and 8192 k-mers
DEVICE_N = (0, 159, 160, 161, 511, 512, 513, 4095, 4096, 4097)
KNOBS = ((), (("no_tile", 1),), (("tile_one_per_cu", 1),), (("tile_min_kmers", 2000),), (("no_fast", 1),))
PLACED = (_abi.IDENTITY_FOUND, _abi.MAX_RESOLUTION)


def _shape(name):
    """-> (FlatDb, SynthDb it was made from, (format, binary_tree, direct_table, fat_direct_table), class-0 kernel)"""
    fast = "place_fast_kernel<5, 9, false, true, {}, {}>"
    if name == "k12":  # closed sets, binary: fat canonical table (the C3 shape)
        s = SynthDb(N_LEAVES, REF_LEN, 12, 4)
        return s.flat, s, (1, 1, 2, 1), fast.format(4, "false")
    if name == "k15_deep":  # canonical direct table, not fat (4^15 entries: 64-bit offsets)
        s = SynthDb(N_LEAVES, REF_LEN, 15, 4, deep=1)
        return s.flat, s, (1, 1, 2, 0), "place_fast_kernel<5, 9, false, false, 1, false>"
    if name == "k13_trunc":  # not strand-symmetric: one tile lookup per k-mer
        s = SynthDb(N_LEAVES, REF_LEN, 13, 4)
        return truncate_random_sets(s.flat, 0.02, seed=3), s, (1, 1, 1, 0), fast.format(0, "false")
    if name in ("k21", "k35"):  # hashed front
        s = SynthDb(N_LEAVES, REF_LEN, int(name[1:]), 4)
        return s.flat, s, (1, 1, 0, 0), fast.format(2, "false")
    if name == "k11_poly":  # polytomies: fast path with child walk, tile child counters
        s = SynthDb(N_LEAVES, REF_LEN, 11, 4, collapse_prob=0.4)
        return s.flat, s, (1, 0, 2, 1), fast.format(4, "true")
    if name == "k16_poly":
        s = SynthDb(N_LEAVES, REF_LEN, 16, 4, collapse_prob=0.4)
        return s.flat, s, (1, 0, 0, 0), fast.format(2, "true")
    if name == "k14_list":  # node sets not closed: sorted lists (wave, block and workspace kernels only)
        s = SynthDb(N_LEAVES, REF_LEN, 14, 4)
        return drop_random_nodes(s.flat, 0.1, seed=5), s, (0, 1, 0, 0), "place_wave_kernel<5, 9, false, true>"
    raise AssertionError(name)


@contextlib.contextmanager
def _knobs(settings):
    try:
        for name, value in settings:
            engine.set_tuning(name, value)
        yield
    finally:
        for name, _ in settings:
            engine.set_tuning(name, 0)


def _boundary_batch(s, k, caps, seed):
    """Reads of c - 2, c and c + 2 k-mers for every cap c (64 per length at caps <= 1024, else 16), at each cap one read with
    N as its last base, one with N as its first, one in lower case; reads of 0, k - 1 and k bases; one of N_MAX bases.
    Shuffled.  -> (bases, offsets, {cap: indices of its plain reads})"""
    rng = np.random.default_rng(seed)
    reads, at_cap = [], {}

    def add(L, n, err=0.01):
        b, _, _ = s.reads(n, L, seed=int(rng.integers(1 << 30)), err=err, frac_random=0.02)
        first = len(reads)
        reads.extend(b.reshape(n, L))
        return list(range(first, first + n))

    for c in sorted(caps):
        L_cap = c // 2 + k - 1  # nk = c, or c - 1 for an odd cap (nk is always even)
        n = 64 if c <= 1024 else 16
        at_cap[c] = [i for d in (-1, 0, 1) for i in add(L_cap + d, n)]
        tail, head, low = (reads[i].copy() for i in add(L_cap, 3))
        tail[-1] = ord("N")
        head[0] = ord("N")
        reads.extend([tail, head, low | 0x20])
    reads.extend(np.zeros(0, np.uint8) for _ in range(4))
    for L in (k - 1, k):
        add(L, 8)
    add(N_MAX, 1)
    perm = rng.permutation(len(reads))
    where = np.empty_like(perm)
    where[perm] = np.arange(len(perm))
    lens = np.array([len(reads[i]) for i in perm], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bases = np.concatenate([reads[i] for i in perm]).astype(np.uint8)
    return bases, offsets, {c: where[idx] for c, idx in at_cap.items()}


def _caps(classes):
    return [c for _, c, _ in classes]


def _assert_equal(got, want, what, gst=None, wst=None, idx=None):
    bad = records_equal(got, want)
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} records differ, first {i if idx is None else idx[i]}: got {describe(got[i])} want {describe(want[i])}")
    if gst is not None:
        sb = stats_equal(gst, wst)
        assert len(sb) == 0, f"{what}: {len(sb)} stats differ, first {sb[0]}: got {gst[sb[0]]} want {wst[sb[0]]}"


SHAPES = ["k12", "k15_deep", "k13_trunc", "k21", "k35", "k11_poly", "k16_poly", "k14_list"]
# remove_intersection on one canonical and one hashed shape
PARAMS = {name: [dict()] + ([dict(remove_intersection=True)] if name in ("k12", "k21") else []) for name in SHAPES}


@pytest.mark.parametrize("name", SHAPES)
def test_reads_at_every_class_limit(name):
    flat, s, shape, class0 = _shape(name)
    k = int(flat.k_size)
    with engine.PlacementDb(flat, device=0) as db:
        info = db.info
        assert (info.format, info.binary_tree, info.direct_table, info.fat_direct_table) == shape
        tiled = info.format == 1
        # ---- the limits, and what every knob configuration does to them
        default = db.read_classes()
        assert default[0][0] == 0 and default[0][1] == 320 and default[0][2] == class0, default
        assert default[1][:2] == (1, 1024), default
        assert max(_caps(default)) == 8192 == info.max_read_kmers, default
        host = {}  # knobs -> classes of a host batch (longest read N_MAX)
        for knobs in KNOBS:
            with _knobs(knobs):
                cl = db.read_classes(N_MAX)
                assert _caps(db.read_classes(N_MAX, stats=True)) == _caps(cl)
                assert _caps(cl)[:2] == [320, 1024] and cl[-1][0] == 7, cl
                assert all(a < b for a, b in zip(_caps(cl), _caps(cl)[1:])), cl
                host[knobs] = cl
        lists = {kn: [c[0] for c in cl] for kn, cl in host.items()}
        if tiled:
            # (the whole-CU launch takes what the shared ones cannot hold; on a direct table the 512-thread one reaches its limit)
            assert set(lists[()]) & {3, 4, 5, 6} and 2 not in lists[()], host[()]
            assert not set(lists[(("no_tile", 1),)]) & {3, 4, 5, 6}, host
            assert not set(lists[(("tile_one_per_cu", 1),)]) & {3, 4, 5} and 6 in lists[(("tile_one_per_cu", 1),)], host
            assert host[(("tile_min_kmers", 2000),)][2][:2] == (2, 2000), host
            assert host[(("tile_min_kmers", 2000),)][2][2].startswith("place_block_kernel<"), host
            assert host[(("no_fast", 1),)][0][2].startswith("place_split_kernel<"), host
        else:
            assert all(lists[kn] == [0, 1, 2, 7] for kn in lists), host
            assert host[()][2][1] == 8192 and host[()][2][2].startswith("place_block_kernel<"), host
        device = {}
        for n in DEVICE_N:
            cl = db.read_classes(n)
            device[n] = cl
            expect = 320 if 0 < n <= 160 else 1024 if 0 < n <= 512 else None
            if expect is not None:
                assert max(_caps(cl)) == expect, (n, cl)
        caps = {c for cl in list(host.values()) + list(device.values()) for c in _caps(cl) if c // 2 + k <= N_MAX}
        bases, offsets, at_cap = _boundary_batch(s, k, caps, seed=len(name))
        lens = np.diff(offsets.astype(np.int64))
        nk = np.where(lens < k, 0, 2 * (lens - k + 1))
        oracle = op.OraclePort(flat)
        for kw in PARAMS[name]:
            want, wst = oracle.place_batch(bases, offsets, op.make_params(**kw), threads=16, want_stats=True)
            prm = engine.make_params(**kw)
            if not kw:
                for c, idx in at_cap.items():
                    placed = np.isin(want["status"][idx], PLACED).mean()
                    assert placed >= 0.5, f"cap {c}: only {placed:.2f} of the reads at it are placed"
            # ---- host entry, every knob configuration, with and without counters
            for knobs in KNOBS:
                with _knobs(knobs):
                    assert _caps(db.read_classes(N_MAX)) == _caps(host[knobs])
                    got, gst = db.place_batch(bases, offsets, prm, want_stats=True)
                    _assert_equal(got, want, f"host entry {knobs} {kw}", gst, wst)
                    _assert_equal(db.place_batch(bases, offsets, prm), want, f"host entry without counters {knobs} {kw}")
                    # the device entry at its default under the same knobs
                    refresh = db.refresh_info().max_read_kmers
                    assert refresh == max(_caps(db.read_classes())) == 8192
                    got, gst = device_place(db, bases, offsets, prm, fill=0xFF)
                    within = nk <= refresh
                    _assert_equal(got[within], want[within], f"device entry {knobs} {kw}", gst[within], wst[within])
            # ---- device entry at every declared read length around the limits
            for n in DEVICE_N:
                db.set_max_read_len(n)
                cap = db.info.max_read_kmers
                assert cap == max(_caps(device[n])) == max(_caps(db.read_classes(n))), (n, cap, device[n])
                got, gst = device_place(db, bases, offsets, prm, fill=0xFF)
                within = nk <= cap
                _assert_equal(got[within], want[within], f"device entry n={n} {kw}", gst[within], wst[within], np.nonzero(within)[0])
                assert (got["status"][~within] == _abi.ERR_READ_TOO_LONG).all(), (n, got["status"][~within])
                assert (gst["n_query_kmers"][~within] == nk[~within]).all(), n
            db.set_max_read_len(0)
            # ---- locality-ordered batch: class-0 and class-1 reads at 320 / 1024 interleaved in one shared list
            short = np.nonzero(nk <= 1026)[0]
            idx = np.random.default_rng(7).permutation(np.resize(short, max(4096, len(short))))
            ob = np.concatenate([bases[int(offsets[i]):int(offsets[i + 1])] for i in idx])
            oo = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.uint64)
            for knobs in ((), (("no_order", 1),)):
                with _knobs(knobs):
                    got, gst = device_place(db, ob, oo, prm, fill=0xFF)
                    _assert_equal(got, want[idx], f"ordered batch, device entry {knobs} {kw}", gst, wst[idx], idx)
                    got, gst = db.place_batch(ob, oo, prm, want_stats=True)
                    _assert_equal(got, want[idx], f"ordered batch, host entry {knobs} {kw}", gst, wst[idx], idx)
