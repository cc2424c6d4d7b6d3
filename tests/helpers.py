"""Shared test helpers (test infrastructure; may use oracle/)."""
import numpy as np

from classeq2_amd import _abi
from classeq2_amd.flatdb import FlatDb

PARAM_SETS = [
    dict(),
    dict(remove_intersection=True),
    dict(min_match_coverage=1.0),
    dict(min_match_coverage=0.0, remove_intersection=False),
    dict(max_iterations=2),
    dict(max_iterations=0),
]
# Option<> corner values: clamping (place_sequence.rs:67-75), NaN coverage (`as usize` -> 0), negative iteration caps
ODD_PARAM_SETS = [
    dict(min_match_coverage=7.5),
    dict(min_match_coverage=-3.0),
    dict(min_match_coverage=float("nan")),
    dict(min_match_coverage=0.5, remove_intersection=True, max_iterations=1000000),
    dict(max_iterations=-4),
    dict(max_iterations=1),
]


def records_equal(a: np.ndarray, b: np.ndarray):
    """Field-wise comparison of cls_placement arrays (padding ignored)."""
    bad = np.zeros(len(a), dtype=bool)
    for f in ("status", "one", "rest", "levels", "clade_id"):
        bad |= a[f] != b[f]
    return np.nonzero(bad)[0]


def stats_equal(a: np.ndarray, b: np.ndarray):
    bad = np.zeros(len(a), dtype=bool)
    for f in ("n_query_kmers", "n_matched", "n_with_root", "leaf_postings"):
        bad |= a[f] != b[f]
    return np.nonzero(bad)[0]


def device_place(db, bases, offsets, params=None, want_stats=True, fill=0):
    """cls_place_batch_device on torch-owned HBM buffers (cuda:0) -> (records, stats).  `fill`: the byte the output
    buffers hold before the launch (0xFF: a record no kernel writes cannot pass for a real one)."""
    import torch

    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    d_b = torch.from_numpy(bases if len(bases) else np.zeros(1, np.uint8)).to(dev)
    d_o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_out = torch.full((n * 24,), fill, dtype=torch.uint8, device=dev)
    d_st = torch.full((n * 24,), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    db.place_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), params, d_st.data_ptr() if want_stats else 0, 0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(_abi.PLACEMENT_DTYPE), d_st.cpu().numpy().view(_abi.STATS_DTYPE)


def describe(rec) -> str:
    st = int(rec["status"])
    name = _abi.STATUS_NAMES[st] if st < len(_abi.STATUS_NAMES) else f"status {st} (never written)"
    return f"{name} one={rec['one']} rest={rec['rest']} levels={rec['levels']} clade={rec['clade_id']}"


def drop_random_nodes(flat: FlatDb, frac: float, seed: int, keep_root_frac: float = 0.9) -> FlatDb:
    """Make node sets that are NOT closed under `parent` (arbitrary DB files are
    allowed at the boundary): delete a random fraction of the ids of every set."""
    rng = np.random.default_rng(seed)
    root_id = int(flat.nodes[0]["id"])
    keep = rng.random(len(flat.node_ids)) >= frac
    is_root = flat.node_ids == root_id
    keep[is_root] = rng.random(int(is_root.sum())) < keep_root_frac
    new_ids = flat.node_ids[keep]
    csum = np.concatenate([[0], np.cumsum(keep)])
    new_off = csum[flat.kmer_node_off.astype(np.int64)].astype(np.uint64)
    return FlatDb(nodes=flat.nodes.copy(), k_size=flat.k_size, m_size=flat.m_size, bucket_key=flat.bucket_key.copy(),
                  bucket_kmer_off=flat.bucket_kmer_off.copy(), kmer_hash=flat.kmer_hash.copy(),
                  kmer_node_off=new_off, node_ids=new_ids)


def truncate_random_sets(flat: FlatDb, frac: float, seed: int) -> FlatDb:
    """Node sets that stay closed under `parent` but hold nothing below the root: a random fraction of the k-mers
    keeps only {root}, another one the empty set (an index file may say so; `cls build-db` never does)."""
    rng = np.random.default_rng(seed)
    root_id = int(flat.nodes[0]["id"])
    off = flat.kmer_node_off.astype(np.int64)
    nk = len(off) - 1
    u = rng.random(nk)
    mode = np.where(u < frac, 1, np.where(u < 2 * frac, 2, 0))  # 1: {root}, 2: {}
    owner = np.repeat(np.arange(nk), np.diff(off))
    is_root = flat.node_ids == root_id
    keep = (mode[owner] == 0) | ((mode[owner] == 1) & is_root)
    new_ids = flat.node_ids[keep]
    csum = np.concatenate([[0], np.cumsum(keep)])
    return FlatDb(nodes=flat.nodes.copy(), k_size=flat.k_size, m_size=flat.m_size, bucket_key=flat.bucket_key.copy(),
                  bucket_kmer_off=flat.bucket_kmer_off.copy(), kmer_hash=flat.kmer_hash.copy(),
                  kmer_node_off=csum[off].astype(np.uint64), node_ids=new_ids)


def ragged_reads(rng, synth, n, min_len, max_len, err=0.02, frac_random=0.05, lower_frac=0.1):
    """Reads of varying length (incl. shorter than k and empty), some lower-case."""
    lens = rng.integers(min_len, max_len + 1, size=n)
    parts, offs = [], [0]
    for i, L in enumerate(lens):
        L = int(L)
        if L == 0:
            offs.append(offs[-1])
            continue
        b, _, _ = synth.reads(1, L, seed=int(rng.integers(1 << 30)), first=i, err=err, frac_random=frac_random)
        if rng.random() < lower_frac:
            b = b | 0x20  # lower-case
        parts.append(b)
        offs.append(offs[-1] + L)
    bases = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return bases, np.array(offs, dtype=np.uint64)


def star_of_cherries(n_cherries: int, seq_len: int = 60, k: int = 7, m: int = 3, seed: int = 0):
    """A root with `n_cherries` internal children of two leaves each (a polytomy whose non-LEAF arity is
    n_cherries), indexed like `cls build-db` does.  -> (FlatDb, list of leaf sequences)"""
    from oracle import oracle_literal as lit

    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    root = dict(id=0, parent=None, kind="ROOT", children=[])
    km = lit.KmersMap(k, m)
    seqs = []
    nid = 1
    for _ in range(n_cherries):
        base = alphabet[rng.integers(0, 4, seq_len)]
        node = dict(id=nid, parent=0, kind="NODE", children=[])
        nid += 1
        for _leaf in range(2):
            sq = base.copy()
            pos = rng.integers(0, seq_len, 2)
            sq[pos] = alphabet[rng.integers(0, 4, 2)]
            seq = bytes(sq).decode()
            seqs.append(seq)
            node["children"].append(dict(id=nid, parent=node["id"], kind="LEAF"))
            for kmer, h in km.build_kmer_from_string(seq):
                km.insert_or_append_kmer_hash(kmer, h, {0, node["id"], nid})
            nid += 1
        root["children"].append(node)
    return FlatDb.from_nested(root, k, m, km.map), seqs


# ---- index surgery: entries filed under a bucket that is not their own prefix's ("foreign" buckets) ------------------
# The reference keeps a hit if its bucket's key is the minimizer of SOME query k-mer (kmers_map.rs:279-297); `cls build-db`
# and the synthetic generator file every k-mer under its own prefix's key, so these helpers make the other shapes a DB
# file may hold.

def kmer_bucket_index(flat: FlatDb) -> np.ndarray:
    """Bucket row of every k-mer (int64[n_kmers])."""
    return np.repeat(np.arange(len(flat.bucket_key)), np.diff(flat.bucket_kmer_off.astype(np.int64)))


def _regroup(flat: FlatDb, bucket_of: np.ndarray, keys: np.ndarray) -> FlatDb:
    """The index with k-mer j filed under bucket row bucket_of[j] of `keys` (< 0: dropped); node sets travel with their
    k-mers, k-mers keep their relative order within a bucket, empty buckets are left out."""
    sel = np.nonzero(bucket_of >= 0)[0]
    perm = sel[np.argsort(bucket_of[sel], kind="stable")]
    counts = np.bincount(bucket_of[sel], minlength=len(keys))
    nonempty = counts > 0
    off = flat.kmer_node_off.astype(np.int64)
    lens = np.diff(off)[perm]
    new_off = np.concatenate([[0], np.cumsum(lens)])
    gather = np.repeat(off[perm] - new_off[:-1], lens) + np.arange(new_off[-1])
    return FlatDb(nodes=flat.nodes.copy(), k_size=flat.k_size, m_size=flat.m_size, bucket_key=np.asarray(keys, dtype=np.uint64)[nonempty],
                  bucket_kmer_off=np.concatenate([[0], np.cumsum(counts[nonempty])]).astype(np.uint64), kmer_hash=flat.kmer_hash[perm],
                  kmer_node_off=new_off.astype(np.uint64), node_ids=flat.node_ids[gather], leaves_only=flat.leaves_only)


def refile_kmers(flat: FlatDb, move: np.ndarray, target_key: np.ndarray) -> FlatDb:
    """The selected k-mers moved into the bucket keyed `target_key[j]` (the first bucket with that key, or a new one).
    Every hash stays in exactly one bucket, so cls_db_create accepts the result."""
    move = np.asarray(move, dtype=bool)
    target_key = np.asarray(target_key, dtype=np.uint64)
    bucket_of = kmer_bucket_index(flat)
    keys = flat.bucket_key
    row_of_key = {}
    for b in range(len(keys) - 1, -1, -1):  # (the first row of a duplicated key)
        row_of_key[int(keys[b])] = b
    extra = []
    for j in np.nonzero(move)[0]:
        t = int(target_key[j])
        if t not in row_of_key:
            row_of_key[t] = len(keys) + len(extra)
            extra.append(t)
        bucket_of[j] = row_of_key[t]
    return _regroup(flat, bucket_of, np.concatenate([keys, np.array(extra, dtype=np.uint64)]))


def drop_kmers(flat: FlatDb, mask: np.ndarray) -> FlatDb:
    """The same index without the selected k-mers."""
    bucket_of = kmer_bucket_index(flat)
    bucket_of[np.asarray(mask, dtype=bool)] = -1
    return _regroup(flat, bucket_of, flat.bucket_key)


def split_buckets(flat: FlatDb, n: int, seed: int) -> FlatDb:
    """Duplicate bucket keys: `n` random buckets of two or more k-mers each give their second half to a new bucket with
    the SAME key (a HashMap cannot hold that; a DB file can)."""
    rng = np.random.default_rng(seed)
    sizes = np.diff(flat.bucket_kmer_off.astype(np.int64))
    pick = rng.choice(np.nonzero(sizes >= 2)[0], n, replace=False)
    bucket_of = kmer_bucket_index(flat)
    keys = list(flat.bucket_key)
    for b in pick:
        lo, hi = int(flat.bucket_kmer_off[b]), int(flat.bucket_kmer_off[b + 1])
        bucket_of[(lo + hi) // 2:hi] = len(keys)
        keys.append(flat.bucket_key[b])
    out = _regroup(flat, bucket_of, np.array(keys, dtype=np.uint64))
    assert len(np.unique(out.bucket_key)) < len(out.bucket_key)
    return out


def kmers_inside_clade(flat: FlatDb, row: int) -> np.ndarray:
    """bool[n_kmers]: the node set names a clade at or below node row `row` and nothing outside it but its ancestors --
    reads from that clade meet these k-mers, reads from elsewhere mostly do not."""
    nodes = flat.nodes
    inside = np.zeros(len(nodes), dtype=bool)
    stack = [row]
    while stack:
        r = stack.pop()
        inside[r] = True
        if nodes[r]["has_children"]:
            fc = int(nodes[r]["first_child"])
            stack.extend(range(fc, fc + int(nodes[r]["n_children"])))
    above = np.zeros(len(nodes), dtype=bool)
    row_of_id = {int(i): r for r, i in enumerate(nodes["id"])}
    p = int(nodes[row]["parent"])
    while p != _abi.NO_PARENT:
        r = row_of_id[p]
        above[r] = True
        p = int(nodes[r]["parent"])
    order = np.argsort(nodes["id"])
    rows = order[np.searchsorted(nodes["id"][order], flat.node_ids)]
    off = flat.kmer_node_off.astype(np.int64)
    owner = np.repeat(np.arange(flat.n_kmers), np.diff(off))
    n_in = np.bincount(owner, weights=inside[rows], minlength=flat.n_kmers)
    n_out = np.bincount(owner, weights=~(inside[rows] | above[rows]), minlength=flat.n_kmers)
    return (n_in > 0) & (n_out == 0)


def clade_with_leaves(flat: FlatDb, lo: int, hi: int) -> int:
    """Row of the first internal clade (breadth-first) with lo..hi leaves below it."""
    nodes = flat.nodes
    n_leaves = (nodes["kind"] == _abi.KIND_LEAF).astype(np.int64)
    for r in range(len(nodes) - 1, -1, -1):  # (children rows are larger than their parent's)
        if nodes[r]["has_children"]:
            fc = int(nodes[r]["first_child"])
            n_leaves[r] = n_leaves[fc:fc + int(nodes[r]["n_children"])].sum()
    for r in range(1, len(nodes)):
        if nodes[r]["kind"] != _abi.KIND_LEAF and lo <= n_leaves[r] <= hi:
            return r
    raise AssertionError(f"no clade with {lo}..{hi} leaves")


def foreign_refile(flat: FlatDb, move: np.ndarray, seed: int, unhashed_frac: float = 0.5):
    """Refile the `move` k-mers under foreign keys: the key of another bucket of the index (accepted when a query k-mer
    of either strand starts with that bucket's prefix), or, for a fraction `unhashed_frac`, a key no m-string hashes to
    (never accepted).  -> (refiled FlatDb, target keys u64[n_kmers])"""
    rng = np.random.default_rng(seed)
    move = np.asarray(move, dtype=bool)
    own = flat.bucket_key[kmer_bucket_index(flat)]
    target = own.copy()
    idx = np.nonzero(move)[0]
    others = flat.bucket_key[rng.integers(0, len(flat.bucket_key), len(idx))]
    for _ in range(8):  # redraw the picks that landed on their own bucket
        same = others == own[idx]
        if not same.any():
            break
        others[same] = flat.bucket_key[rng.integers(0, len(flat.bucket_key), int(same.sum()))]
    unhashed = rng.random(len(idx)) < unhashed_frac
    target[idx] = np.where(unhashed, unhashed_keys(flat, len(idx), rng), others)
    keep = target[idx] != own[idx]  # (a single-bucket index has no other bucket: those stay put)
    move = move.copy()
    move[idx[~keep]] = False
    assert (target[move] != own[move]).all() and move.any()
    return refile_kmers(flat, move, target), move


def unhashed_keys(flat: FlatDb, n: int, rng) -> np.ndarray:
    """`n` random 64-bit keys that are no bucket's key and (checked by enumeration for m <= 8; a 2^-40 chance beyond)
    not the hash of any ACGT m-string; key 0 -- the minimizer of m = 0 -- among them when m > 0."""
    from oracle import oracle_port as op

    m = min(flat.m_size, flat.k_size)
    keys = rng.integers(1, np.iinfo(np.int64).max, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    if m > 0 and n:
        keys[0] = 0
    if 0 < m <= 8:
        lib = op.lib()
        codes = np.arange(4 ** m)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[(codes[:, None] >> (2 * np.arange(m))) & 3]
        hashed = {lib.cls_oracle_murmur3_h1(bytes(s), m) for s in letters}
        assert not hashed.intersection(int(x) for x in keys)
    assert not np.isin(keys, flat.bucket_key).any()
    return keys
