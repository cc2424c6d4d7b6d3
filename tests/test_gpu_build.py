"""The device index builder (cls_kmers_build, cls_tree_build_kmers_map_device) against the host builder, which gives the
same bytes in the same canonical order, against the synthetic generator and against a database the reference built."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.flatdb import FlatDb

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID_ARG, E_BAD_DB = -1, -3
ARRAYS = ("bucket_key", "bucket_kmer_off", "kmer_hash", "kmer_node_off", "node_ids")


def assert_same(got: FlatDb, want: FlatDb, what=""):
    for f in ARRAYS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)
    assert (got.k_size, got.m_size, got.leaves_only) == (want.k_size, want.m_size, want.leaves_only), what


def copy_flat(t: engine.Tree) -> FlatDb:
    d = _abi.DbDesc()
    engine._check_host(engine.lib().cls_tree_desc(t._h, C.byref(d)))
    return FlatDb.from_desc(d, copy=True)


def host_build(tree_fn, msa: bytes, k, m, shift, fwd) -> FlatDb:
    t = tree_fn()
    t.build_kmers_map(msa, k, m, reference_header_shift=shift, forward_only=fwd)
    return copy_flat(t)


def device_build(tree_fn, msa: bytes, k, m, shift, fwd, leaves_only=False) -> FlatDb:
    t = tree_fn()
    t.build_kmers_map_device(msa, k, m, reference_header_shift=shift, forward_only=fwd, device=0, leaves_only=leaves_only)
    return copy_flat(t)


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    g = json.load(open(os.path.join(GOLD, "builder_colletotrichum.json")))
    p = tmp_path_factory.mktemp("b") / "tree.json"
    p.write_text(g["tree_json"])
    g["tree_fn"] = lambda: engine.Tree(str(p))
    g["msa"] = g["msa_fasta"].encode()
    return g


# ---- 1. the Colletotrichum fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("fwd", [True, False])
def test_colletotrichum_device_equals_host(gold, shift, fwd):
    k, m = gold["k_size"], gold["m_size"]
    want = host_build(gold["tree_fn"], gold["msa"], k, m, shift, fwd)
    got = device_build(gold["tree_fn"], gold["msa"], k, m, shift, fwd)
    assert_same(got, want, (shift, fwd))
    assert len(got.kmer_hash) > 1000
    if shift and fwd:  # what the reference's own build wrote
        d = {}
        for b in range(len(got.bucket_key)):
            for j in range(int(got.bucket_kmer_off[b]), int(got.bucket_kmer_off[b + 1])):
                d[int(got.kmer_hash[j])] = (int(got.bucket_key[b]), [int(x) for x in got.node_ids[got.kmer_node_off[j]:got.kmer_node_off[j + 1]]])
        expected = {int(h): (int(v["bucket"]), sorted(v["nodes"])) for h, v in gold["expected"].items()}
        assert d == expected


# ---- 2. every k class, every m class, odd records ------------------------------------------------------------------
def _random_newick(rng, n_leaves):
    nodes = [f"L{i}" for i in range(n_leaves)]
    while len(nodes) > 1:
        i = rng.randrange(len(nodes) - 1)
        nodes[i:i + 2] = [f"({nodes[i]},{nodes[i + 1]})99"]
    return nodes[0] + ";"


def _random_msa(rng, names, lengths):
    out = []
    for name, L in zip(names, lengths):
        seq = "".join(rng.choice("ACGT") for _ in range(L))
        out.append(f">{name}\n{seq}\n")
    return out


@pytest.fixture(scope="module")
def small():
    rng = random.Random(7)
    n = 14
    nw = _random_newick(rng, n)
    names = [f"L{i}" for i in range(n)] + ["L3", "L5", "L0", "L9"]  # records filed under a leaf twice
    lengths = [rng.randrange(20, 400) for _ in range(n)] + [rng.randrange(60, 200), 5, 150, 30]
    recs = _random_msa(rng, names, lengths)
    recs.insert(4, ">L11\n\n")            # an empty record
    recs.insert(9, ">L12\nNNNN-xx--\n")   # no ACGT: empty once filtered
    recs.insert(2, ">L13\nacgtACGTnnACG\n")  # lower case is filtered out (sequence.rs:47-56)
    return dict(tree_fn=lambda: engine.Tree.from_newick(nw, "small.nwk", 0.0), msa="".join(recs).encode())


@pytest.mark.parametrize("k", [1, 8, 12, 15, 16, 17, 31, 32, 33, 35, 64])
def test_k_m_sweep_equals_host(small, k):
    for m in (0, 4, k, k + 3):
        for shift, fwd in ((False, False), (True, True)):
            want = host_build(small["tree_fn"], small["msa"], k, m, shift, fwd)
            got = device_build(small["tree_fn"], small["msa"], k, m, shift, fwd)
            assert_same(got, want, (k, m, shift, fwd))


@pytest.mark.parametrize("k", [1, 12, 35])
def test_full_key_sort_path_equals_host(small, k):
    """The (bucket key, hash) sort a 64-bit hash collision takes gives the same map."""
    engine.set_tuning("build_full_key", 1)
    try:
        for m in (0, 4):
            want = host_build(small["tree_fn"], small["msa"], k, m, False, False)
            got = device_build(small["tree_fn"], small["msa"], k, m, False, False)
            assert_same(got, want, (k, m))
    finally:
        engine.set_tuning("build_full_key", 0)


# ---- 3. leaves-only -------------------------------------------------------------------------------------------------
def test_leaves_only_equals_reduced_explicit(gold, small):
    for src, k, m in ((gold, gold["k_size"], gold["m_size"]), (small, 17, 4)):
        explicit = device_build(src["tree_fn"], src["msa"], k, m, False, False)
        leaves = device_build(src["tree_fn"], src["msa"], k, m, False, False, leaves_only=True)
        assert leaves.leaves_only
        assert_same(leaves, explicit.to_leaves_only())


def test_deep_caterpillar():
    rng = random.Random(11)
    n = 330
    nw = f"L{n - 1}"
    for i in range(n - 2, -1, -1):
        nw = f"(L{i},{nw})90"
    nw += ";"
    msa = "".join(_random_msa(rng, [f"L{i}" for i in range(n)], [rng.randrange(40, 120) for _ in range(n)])).encode()
    tree_fn = lambda: engine.Tree.from_newick(nw, "deep.nwk", 0.0)  # noqa: E731
    host = host_build(tree_fn, msa, 9, 3, False, False)
    depth = int(np.diff(host.kmer_node_off).max())
    assert depth >= 300  # some k-mer's node set holds a root path of the full depth
    leaves = device_build(tree_fn, msa, 9, 3, False, False, leaves_only=True)
    assert_same(leaves, host.to_leaves_only())
    assert_same(device_build(tree_fn, msa, 9, 3, False, False), host)


# ---- 4. the synthetic generator -------------------------------------------------------------------------------------
def canonical(f: FlatDb):
    """(bucket key, hash) ascending, ids ascending inside a k-mer: the generator scrambles its order."""
    kb = np.repeat(f.bucket_key, np.diff(f.bucket_kmer_off).astype(np.int64))
    order = np.lexsort((f.kmer_hash, kb))
    cnt = np.diff(f.kmer_node_off).astype(np.int64)
    seg = np.repeat(np.arange(len(cnt)), cnt)
    ids = f.node_ids[np.lexsort((f.node_ids, seg))]  # ids sorted inside every k-mer, k-mers in place
    starts = f.kmer_node_off[:-1].astype(np.int64)
    cnt_o = cnt[order]
    off = np.concatenate([[0], np.cumsum(cnt_o)]).astype(np.int64)
    src = np.repeat(starts[order] - off[:-1], cnt_o) + np.arange(off[-1])
    return kb[order], f.kmer_hash[order], off.astype(np.uint64), ids[src]


def _synth_records(s):
    seqs = b"".join(s.leaf_seq(i).encode() for i in range(s.n_leaves))
    bases = np.frombuffer(seqs, dtype=np.uint8)
    offsets = np.arange(s.n_leaves + 1, dtype=np.uint64) * np.uint64(s.ref_len)
    leaf_ids = np.array([s.leaf_id(i) for i in range(s.n_leaves)], dtype=np.uint64)
    return bases, offsets, leaf_ids


def _assert_canonical_equal(got, want):
    a, b = canonical(got), canonical(want)
    for x, y, name in zip(a, b, ("bucket", "hash", "offsets", "ids")):
        assert np.array_equal(x, y), name
    # and the device result is canonical already
    for x, y in zip(a, (np.repeat(got.bucket_key, np.diff(got.bucket_kmer_off).astype(np.int64)), got.kmer_hash, got.kmer_node_off, got.node_ids)):
        assert np.array_equal(x, y)


def test_synth_2k_leaves_explicit():
    from classeq2_amd.synth import SynthDb
    s = SynthDb(2000, 800, 10, 4, threads=16)
    bases, offsets, leaf_ids = _synth_records(s)
    got = engine.build_kmers(s.flat.nodes, bases, offsets, leaf_ids, 10, 4)
    _assert_canonical_equal(got, s.flat)


def test_synth_c3_size_leaves_only():
    """10 k leaves x 1.5 kb, k = 12: 29.8 M windows, a sort of more than 2^24 records in several workgroup-tiled passes."""
    from classeq2_amd.synth import SynthDb
    s = SynthDb(10_000, 1500, 12, 4, threads=16, tips_only=True)
    assert s.flat.leaves_only
    bases, offsets, leaf_ids = _synth_records(s)
    got, info = engine.build_kmers(s.flat.nodes, bases, offsets, leaf_ids, 12, 4, leaves_only=True, return_info=True)
    assert info["n_windows"] == 10_000 * (1500 - 12 + 1) * 2 > 1 << 24
    assert info["n_kmers"] == len(got.kmer_hash) and info["n_leaf_postings"] == len(got.node_ids)
    _assert_canonical_equal(got, s.flat)


# ---- 5. build on the device, place ------------------------------------------------------------------------------------
def test_device_built_index_places_like_host_built(gold):
    from oracle import oracle_port as op
    from tests.helpers import records_equal
    k, m = gold["k_size"], gold["m_size"]
    host = host_build(gold["tree_fn"], gold["msa"], k, m, False, False)
    _, bases, off, _ = engine.fasta_parse(gold["msa"])
    want = op.OraclePort(host).place_batch(bases, off, threads=8)
    with engine.PlacementDb(host, device=0) as db:
        via_host = db.place_batch(bases, off)
    assert len(records_equal(via_host, want)) == 0
    for leaves_only in (False, True):
        flat = device_build(gold["tree_fn"], gold["msa"], k, m, False, False, leaves_only=leaves_only)
        with engine.PlacementDb(flat, device=0) as db:
            got = db.place_batch(bases, off)
        assert len(records_equal(got, want)) == 0, leaves_only


# ---- 6. errors -------------------------------------------------------------------------------------------------------
def test_errors_leave_the_device_usable(gold, small):
    bad_msa = b">nobody\nACGTACGTACGTACGT\n>nobody2\nACGTACGTACGTAAAA\n"
    t = gold["tree_fn"]()
    with pytest.raises(engine.ClsError) as host_err:
        t.build_kmers_map(bad_msa, 12, 4)
    with pytest.raises(engine.ClsError) as dev_err:
        gold["tree_fn"]().build_kmers_map_device(bad_msa, 12, 4)
    assert dev_err.value.msg == host_err.value.msg and dev_err.value.code == E_BAD_DB
    with pytest.raises(engine.ClsError) as e:
        gold["tree_fn"]().build_kmers_map_device(gold["msa"], 0, 4)
    assert e.value.code == E_INVALID_ARG
    with pytest.raises(engine.ClsError) as e:
        gold["tree_fn"]().build_kmers_map_device(gold["msa"], 12, 4, device=engine.device_count() + 3)
    assert e.value.code == E_INVALID_ARG

    flat = host_build(gold["tree_fn"], gold["msa"], 12, 4, False, False)
    nodes = flat.nodes
    leaf = nodes["id"][nodes["kind"] == _abi.KIND_LEAF][:2]
    bases = np.frombuffer(b"ACGTACGTACGTACGTAAAACCCC", dtype=np.uint8)
    offsets = np.array([0, 12, 24], dtype=np.uint64)
    for kwargs, code in ((dict(k=0), E_INVALID_ARG), (dict(device=engine.device_count()), E_INVALID_ARG), (dict(device=-7), E_INVALID_ARG)):
        args = dict(k=5, m=2, device=0)
        args.update(kwargs)
        with pytest.raises(engine.ClsError) as e:
            engine.build_kmers(nodes, bases, offsets, leaf, args["k"], args["m"], device=args["device"])
        assert e.value.code == code, kwargs
    with pytest.raises(engine.ClsError) as e:  # the root is not a LEAF
        engine.build_kmers(nodes, bases, offsets, np.array([leaf[0], nodes["id"][0]], dtype=np.uint64), 5, 2)
    assert e.value.code == E_BAD_DB
    with pytest.raises(engine.ClsError) as e:  # an id the tree does not hold
        engine.build_kmers(nodes, bases, offsets, np.array([leaf[0], 10**15], dtype=np.uint64), 5, 2)
    assert e.value.code == E_BAD_DB
    # after every failure: builds in the same process still succeed and agree with the host
    got = engine.build_kmers(nodes, bases, offsets, leaf, 5, 2)
    assert len(got.kmer_hash) > 0
    assert_same(device_build(gold["tree_fn"], gold["msa"], 12, 4, False, False), flat)
