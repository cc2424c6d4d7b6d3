"""Index groups (cls_db_group_*, cls_place_batch_group, cls_place_sequences_group, cls-place --device a,b,..): one index
encoded once and uploaded to several replicas; a batch is cut across them.  On a one-GPU machine the replicas share
device 0 ({0, 0, ...}), which exercises everything but the second device."""
import os
import subprocess
import threading

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb
from oracle import oracle_port as op
from tests.helpers import PARAM_SETS, describe, ragged_reads, records_equal, stats_equal
from tests.test_cli_e2e import CLI, write_db_json, write_fasta
from tests.test_golden import _load

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 3, 5)


def _shape(name):
    """-> (SynthDb, bases, offsets) of a ragged batch with skewed lengths."""
    rng = np.random.default_rng(7)
    if name == "k12":  # closed sets, binary: fat canonical direct table
        s = SynthDb(64, 3000, 12, 4)
        short = ragged_reads(rng, s, 2500, 0, 200)
        longr = ragged_reads(rng, s, 40, 300, 2000)  # a tail of longer reads: the last shard gets few, long reads
        return s, *_concat(short, longr)
    if name == "k16_poly":  # hashed front, polytomies
        s = SynthDb(64, 3000, 16, 4, collapse_prob=0.4)
        return s, *ragged_reads(rng, s, 2500, 0, 400)
    if name == "k12_long":  # reads beyond 8192 k-mers, all at the front: the tile / workspace kernels run in replica 0
        s = SynthDb(32, 6000, 12, 4)
        longr = ragged_reads(rng, s, 6, 4200, 5800, lower_frac=0.0)
        short = ragged_reads(rng, s, 2000, 100, 160)
        return s, *_concat(longr, short)
    raise AssertionError(name)


def _concat(a, b):
    bases = np.concatenate([a[0], b[0]])
    offsets = np.concatenate([a[1], b[1][1:] + a[1][-1]]).astype(np.uint64)
    return bases, offsets


def _assert_equal(got, want, what):
    bad = records_equal(got, want)
    assert len(bad) == 0, f"{what}: {len(bad)} records differ; first #{bad[0]}: got {describe(got[bad[0]])}, want {describe(want[bad[0]])}"


@pytest.mark.parametrize("shape", ["k12", "k16_poly", "k12_long"])
def test_group_parity(shape):
    s, bases, offsets = _shape(shape)
    n_all = len(offsets) - 1
    oracle = op.OraclePort(s.flat)
    groups = {g: engine.PlacementDbGroup(s.flat, [0] * g) for g in GROUPS}
    with engine.PlacementDb(s.flat, device=0) as single:
        for kw in PARAM_SETS:
            prm = engine.make_params(**kw)
            want, wst = oracle.place_batch(bases, offsets, op.make_params(**kw), threads=16, want_stats=True)
            one, ost = single.place_batch(bases, offsets, prm, want_stats=True)
            _assert_equal(one, want, f"{shape} single handle {kw}")
            for g, grp in groups.items():
                assert grp.size == g
                for n in sorted({0, 1, max(g - 1, 0), g, n_all}):
                    off = offsets[: n + 1]
                    got, gst = grp.place_batch(bases, off, prm, want_stats=True)
                    _assert_equal(got, want[:n], f"{shape} group {g} n={n} {kw}")
                    _assert_equal(got, one[:n], f"{shape} group {g} n={n} {kw} vs single")
                    assert len(stats_equal(gst, wst[:n])) == 0, f"{shape} group {g} n={n} {kw}: counters"
                    assert len(stats_equal(gst, ost[:n])) == 0
                _assert_equal(grp.place_batch(bases, offsets, prm), want, f"{shape} group {g} without counters {kw}")
    for grp in groups.values():
        grp.close()


def test_every_replica_places_a_shard():
    s = SynthDb(64, 3000, 12, 4)
    bases, offsets, _ = s.reads(3000, 150)
    with engine.PlacementDbGroup(s.flat, [0, 0, 0]) as grp:
        reps = [grp.replica(i) for i in range(grp.size)]
        for r in reps:
            r.kernel_time(reset=True)
        got = grp.place_batch(bases, offsets)
        launches = [r.kernel_time()[1] for r in reps]
        assert all(x > 0 for x in launches), launches
        _assert_equal(got, op.OraclePort(s.flat).place_batch(bases, offsets, threads=16), "3 replicas")
        del reps


def test_replica_info_matches_a_separate_handle():
    s = SynthDb(64, 3000, 16, 4, collapse_prob=0.4)
    with engine.PlacementDbGroup(s.flat, [0, 0]) as grp, engine.PlacementDb(s.flat, device=0) as db:
        want = {f: getattr(db.info, f) for f, _ in _abi.DbInfo._fields_ if f != "scratch_slots"}
        for i in range(grp.size):
            r = grp.replica(i)
            assert {f: getattr(r.info, f) for f in want} == want
            r.close()  # a view: the replica stays with the group
            del r
        # the replicas still place after their views are gone
        bases, offsets, _ = s.reads(100, 150)
        _assert_equal(grp.place_batch(bases, offsets), db.place_batch(bases, offsets), "after views closed")


def test_group_errors():
    s = SynthDb(64, 3000, 12, 4)
    n_dev = engine.device_count()
    with pytest.raises(engine.ClsError) as e:
        engine.PlacementDbGroup(s.flat, [0, n_dev])
    assert e.value.code == -1 and "out of range" in e.value.msg
    with pytest.raises(engine.ClsError) as e:
        engine.PlacementDbGroup(s.flat, [-1])
    assert e.value.code == -1
    with engine.PlacementDbGroup(s.flat, [0, 0]) as grp:
        bases, offsets, _ = s.reads(500, 150)
        wrong = offsets.copy()
        wrong[300] = wrong[301] + 1  # not monotone
        with pytest.raises(engine.ClsError) as e:
            grp.place_batch(bases, wrong)
        assert e.value.code == -1 and "offsets not monotone" in e.value.msg  # (read on the calling thread)
        _assert_equal(grp.place_batch(bases, offsets), op.OraclePort(s.flat).place_batch(bases, offsets, threads=16), "after error")


def test_bad_descriptor_is_bad_db():
    """A descriptor the encoder refuses: CLS_E_BAD_DB, as cls_db_create returns for it."""
    s = SynthDb(64, 3000, 12, 4)
    from classeq2_amd.flatdb import FlatDb
    f = FlatDb.from_desc(s.flat.desc(), copy=True)
    f.bucket_kmer_off[-1] += 1  # the buckets no longer span the k-mers
    with pytest.raises(engine.ClsError) as e1:
        engine.PlacementDb(f, device=0)
    with pytest.raises(engine.ClsError) as e2:
        engine.PlacementDbGroup(f, [0, 0])
    assert e2.value.code == e1.value.code == -3, (e1.value, e2.value)


def test_two_threads_share_a_group():
    s = SynthDb(64, 3000, 12, 4)
    rng = np.random.default_rng(11)
    batches = [ragged_reads(rng, s, 3000, 0, 300) for _ in range(2)]
    oracle = op.OraclePort(s.flat)
    want = [oracle.place_batch(b, o, threads=8) for b, o in batches]
    got = [None, None]
    with engine.PlacementDbGroup(s.flat, [0, 0, 0]) as grp:
        def run(i):
            for _ in range(3):
                got[i] = grp.place_batch(*batches[i])
                _assert_equal(got[i], want[i], f"thread {i}")

        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    for i in range(2):
        assert got[i] is not None
        _assert_equal(got[i], want[i], f"thread {i}")


def test_place_sequences_group_matches_single(tmp_path):
    """engine.place_sequences on a group writes what it writes on one handle."""
    flat, bases, offsets, params, expected = _load()
    db_json = str(tmp_path / "db.json")
    write_db_json(flat, db_json)
    tree = engine.Tree(db_json)
    fa = str(tmp_path / "q.fasta")
    write_fasta(fa, [f"q{i}" for i in range(len(offsets) - 1)], bases, offsets)
    with engine.PlacementDb(tree.flat(), device=0) as db:
        n1, _ = engine.place_sequences(db, tree, fa, str(tmp_path / "one" / "r.out"))
    with engine.PlacementDbGroup(tree.flat(), [0, 0, 0]) as grp:
        n3, _ = engine.place_sequences(grp, tree, fa, str(tmp_path / "three" / "r.out"))
    assert n1 == n3 == len(offsets) - 1
    for ext in ("yaml", "error"):
        assert open(tmp_path / "one" / f"r.{ext}", "rb").read() == open(tmp_path / "three" / f"r.{ext}", "rb").read()


def _adversarial_fasta(bases, offsets, n_pieces):
    """A multi-record FASTA whose lines at the split targets are '>' lines that are no safe cut: an empty header,
    '>'-only and N-only records, blank lines and CRLF around real reads."""
    raw = bytes(bases)
    recs = [b">r%d\n%s\n" % (i, raw[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)]
    traps = [b">>\r\nNNNN\r\n", b">r_empty\n\n", b">nn\nnnnn\n", b">\n"]
    text = b"".join(recs)
    # put a trap at every split target of the final text (the targets move little as traps are added)
    for _ in range(3):
        out, last = b"", 0
        targets = [i * len(text) // n_pieces for i in range(1, n_pieces)]
        for t in targets:
            p = text.find(b"\n>", t)
            if p < 0:
                break
            out += text[last:p + 1] + traps[len(out) % len(traps)]
            last = p + 1
        text = out + text[last:]
    return text


@pytest.mark.parametrize("fmt", ["yaml", "jsonl"])
def test_cli_device_list_matches_single_device(tmp_path, fmt):
    flat, bases, offsets, params, expected = _load()
    headers = [str(h) for h in np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colletotrichum_k12.npz"))["headers"]]
    db = str(tmp_path / "db.json")
    write_db_json(flat, db)
    fa = str(tmp_path / "q.fasta")
    write_fasta(fa, headers, bases, offsets)
    adv = str(tmp_path / "adv.fasta")
    text = _adversarial_fasta(bases, offsets, 3)
    open(adv, "wb").write(text)
    cuts = engine.fasta_split(text, 3)
    assert len(cuts) == 4, cuts  # three pieces
    for q in (fa, adv):
        outs = {}
        for dev in ("0", "0,0,0"):
            out = str(tmp_path / f"res_{dev.replace(',', '_')}_{os.path.basename(q)}" / "result.out")
            r = subprocess.run([CLI, q, "-d", db, "-o", out, "--out-format", fmt, "--device", dev], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            base = out[: -len(".out")]
            outs[dev] = (open(f"{base}.{fmt}", "rb").read(), open(f"{base}.error", "rb").read())
        assert outs["0"] == outs["0,0,0"], q
        assert len(outs["0"][0]) > 0
    r = subprocess.run([CLI, fa, "-d", db, "-o", str(tmp_path / "x" / "r.out"), "--device", "0,x"], capture_output=True, text=True)
    assert r.returncode == 2 and "--device" in r.stderr


def test_two_distinct_devices():
    if engine.device_count() < 2:
        pytest.skip("needs two GPUs")
    s = SynthDb(64, 3000, 12, 4)
    bases, offsets, _ = s.reads(4000, 150)
    with engine.PlacementDbGroup(s.flat, [0, 1]) as grp:
        assert [grp.replica(i).info.device for i in range(2)] == [0, 1]
        _assert_equal(grp.place_batch(bases, offsets), op.OraclePort(s.flat).place_batch(bases, offsets, threads=16), "[0, 1]")
