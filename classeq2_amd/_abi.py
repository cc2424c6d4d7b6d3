"""ctypes mirror of include/cls_place.h and csrc/cls_synth.h (struct layouts only)."""

import ctypes as C

ABI_VERSION = 2
SETS_EXPLICIT, SETS_LEAVES = 0, 1

KIND_ROOT, KIND_NODE, KIND_LEAF = 0, 1, 2
NO_PARENT = (1 << 64) - 1

HAS_MAX_ITERATIONS = 1
HAS_MIN_MATCH_COVERAGE = 2
HAS_REMOVE_INTERSECTION = 4

(
    UNCLASSIFIABLE_NO_MATCH,
    UNCLASSIFIABLE_NO_ROOT,
    UNCLASSIFIABLE_COVERAGE,
    UNCLASSIFIABLE_LEVEL1,
    IDENTITY_FOUND,
    MAX_RESOLUTION,
    INCONCLUSIVE,
    ERR_TOO_FEW_KMERS,
    ERR_MAX_ITER,
    ERR_ROOT_NO_CHILDREN,
    ERR_INVALID_BASE,
    ERR_READ_TOO_LONG,
) = range(12)

STATUS_NAMES = [
    "UNCLASSIFIABLE_NO_MATCH",
    "UNCLASSIFIABLE_NO_ROOT",
    "UNCLASSIFIABLE_COVERAGE",
    "UNCLASSIFIABLE_LEVEL1",
    "IDENTITY_FOUND",
    "MAX_RESOLUTION",
    "INCONCLUSIVE",
    "ERR_TOO_FEW_KMERS",
    "ERR_MAX_ITER",
    "ERR_ROOT_NO_CHILDREN",
    "ERR_INVALID_BASE",
    "ERR_READ_TOO_LONG",
]


class Node(C.Structure):
    _fields_ = [
        ("id", C.c_uint64),
        ("parent", C.c_uint64),
        ("first_child", C.c_uint32),
        ("n_children", C.c_uint32),
        ("kind", C.c_uint8),
        ("has_children", C.c_uint8),
        ("pad_", C.c_uint8 * 6),
    ]


class DbDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_nodes", C.c_uint32),
        ("nodes", C.POINTER(Node)),
        ("k_size", C.c_uint64),
        ("m_size", C.c_uint64),
        ("n_buckets", C.c_uint64),
        ("bucket_key", C.POINTER(C.c_uint64)),
        ("bucket_kmer_off", C.POINTER(C.c_uint64)),
        ("n_kmers", C.c_uint64),
        ("kmer_hash", C.POINTER(C.c_uint64)),
        ("kmer_node_off", C.POINTER(C.c_uint64)),
        ("node_ids", C.POINTER(C.c_uint64)),
        ("node_set_kind", C.c_uint32),
        ("pad_", C.c_uint32),
    ]


BUILD_REFERENCE_HEADER_SHIFT, BUILD_FORWARD_ONLY, BUILD_LEAVES_ONLY = 1, 2, 4


class BuildDesc(C.Structure):
    """cls_build_desc (cls_kmers_build)."""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_nodes", C.c_uint32),
        ("nodes", C.POINTER(Node)),
        ("k_size", C.c_uint64),
        ("m_size", C.c_uint64),
        ("n_records", C.c_uint32),
        ("flags", C.c_uint32),
        ("bases", C.c_void_p),
        ("offsets", C.POINTER(C.c_uint64)),
        ("leaf_id", C.POINTER(C.c_uint64)),
    ]


class KmersInfo(C.Structure):
    """cls_kmers_info."""
    _fields_ = [
        ("n_windows", C.c_uint64),
        ("n_kmers", C.c_uint64),
        ("n_leaf_postings", C.c_uint64),
        ("n_node_ids", C.c_uint64),
        ("n_buckets", C.c_uint64),
        ("peak_device_bytes", C.c_uint64),
        ("ms_hash", C.c_double),
        ("ms_sort", C.c_double),
        ("ms_group", C.c_double),
        ("ms_d2h", C.c_double),
        ("ms_expand", C.c_double),
        ("sort_passes", C.c_uint32),
        ("full_key", C.c_uint32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("flags", C.c_uint32),
        ("max_iterations", C.c_int32),
        ("min_match_coverage", C.c_double),
        ("remove_intersection", C.c_uint8),
        ("pad_", C.c_uint8 * 7),
    ]


class Placement(C.Structure):
    _fields_ = [
        ("status", C.c_uint8),
        ("pad_", C.c_uint8 * 3),
        ("one", C.c_int32),
        ("rest", C.c_int32),
        ("levels", C.c_uint32),
        ("clade_id", C.c_uint64),
    ]


class QueryStats(C.Structure):
    _fields_ = [
        ("n_query_kmers", C.c_uint32),
        ("n_matched", C.c_uint32),
        ("n_with_root", C.c_uint32),
        ("index_bytes", C.c_uint32),
        ("leaf_postings", C.c_uint64),
    ]


class DbInfo(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("max_nonleaf_arity", C.c_uint32),
        ("k_size", C.c_uint32),
        ("m_size", C.c_uint32),
        ("n_buckets", C.c_uint32),
        ("n_kmers", C.c_uint64),
        ("n_closed_kmers", C.c_uint64),
        ("table_slots", C.c_uint64),
        ("postings_words", C.c_uint64),
        ("hbm_bytes", C.c_uint64),
        ("max_read_kmers", C.c_uint32),
        ("device", C.c_int32),
        ("format", C.c_uint32),
        ("binary_tree", C.c_uint32),
        ("direct_table", C.c_uint32),
        ("n_tip_sets", C.c_uint32),
        ("scratch_slots", C.c_uint32),
        ("fat_direct_table", C.c_uint32),
    ]


class ReadClass(C.Structure):
    """cls_read_class (cls_db_read_classes)."""
    _fields_ = [
        ("list", C.c_uint32),
        ("max_kmers", C.c_uint32),
        ("kernel", C.c_char * 112),
    ]


class Fasta(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("truncated", C.c_uint32),
        ("headers", C.POINTER(C.c_char)),
        ("header_off", C.POINTER(C.c_uint64)),
        ("bases", C.POINTER(C.c_char)),
        ("base_off", C.POINTER(C.c_uint64)),
    ]



class FastqOpts(C.Structure):
    """cls_fastq_opts: quality cutoffs of the FASTQ stage (0: that end is not trimmed)."""
    _fields_ = [
        ("trim_5p", C.c_uint32),
        ("trim_3p", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


QUERY_FASTA, QUERY_FASTQ = 0, 1  # cls_place_sequences_ex (include/cls_host.h)

class ServiceStats(C.Structure):
    _fields_ = [
        ("jobs_submitted", C.c_uint64),
        ("jobs_done", C.c_uint64),
        ("reads_placed", C.c_uint64),
        ("device_batches", C.c_uint64),
        ("max_jobs_in_batch", C.c_uint64),
        ("models", C.c_uint64),
    ]


class SynthCfg(C.Structure):
    _fields_ = [
        ("n_leaves", C.c_uint32),
        ("ref_len", C.c_uint32),
        ("k_size", C.c_uint32),
        ("m_size", C.c_uint32),
        ("seed_tree", C.c_uint64),
        ("seed_refseq", C.c_uint64),
        ("edge_sub_rate", C.c_double),
        ("deep", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("collapse_prob", C.c_double),
        ("id_stride", C.c_uint64),
        ("id_offset", C.c_uint64),
        ("threads", C.c_uint32),
        ("tips_only", C.c_uint32),
    ]


assert C.sizeof(Node) == 32
assert C.sizeof(Placement) == 24
assert C.sizeof(QueryStats) == 24
assert C.sizeof(Params) == 24
assert C.sizeof(BuildDesc) == 64 and C.sizeof(KmersInfo) == 96

import numpy as np  # noqa: E402

NODE_DTYPE = np.dtype(
    [
        ("id", "<u8"),
        ("parent", "<u8"),
        ("first_child", "<u4"),
        ("n_children", "<u4"),
        ("kind", "u1"),
        ("has_children", "u1"),
        ("pad_", "u1", (6,)),
    ]
)
PLACEMENT_DTYPE = np.dtype(
    [("status", "u1"), ("pad_", "u1", (3,)), ("one", "<i4"), ("rest", "<i4"), ("levels", "<u4"), ("clade_id", "<u8")]
)
STATS_DTYPE = np.dtype(
    [("n_query_kmers", "<u4"), ("n_matched", "<u4"), ("n_with_root", "<u4"), ("index_bytes", "<u4"), ("leaf_postings", "<u8")]
)
# clade tally (cls_tally_row, cls_tally_totals)
TALLY_ROW_DTYPE = np.dtype(
    [("id", "<u8"), ("n_clade", "<u8"), ("n_direct", "<u8"), ("n_identity", "<u8"), ("n_max_resolution", "<u8"), ("n_inconclusive", "<u8"),
     ("sum_one", "<i8"), ("sum_rest", "<i8")]
)
TALLY_TOTALS_DTYPE = np.dtype([("n_reads", "<u8"), ("status_count", "<u8", (12,)), ("n_unknown_clade", "<u8"), ("n_bad_status", "<u8")])
# paired reads (cls_pair_totals, CLS_PAIR_*)
(PAIR_NEITHER, PAIR_ONLY_1, PAIR_ONLY_2, PAIR_SAME, PAIR_NESTED_1, PAIR_NESTED_2, PAIR_DISCORDANT) = range(7)
PAIR_CLASS_NAMES = ["NEITHER", "ONLY_1", "ONLY_2", "SAME", "NESTED_1", "NESTED_2", "DISCORDANT"]
PAIR_CONSERVATIVE, PAIR_REQUIRE_BOTH = 1, 2
E_BAD_PAIRS = -8
PAIR_TOTALS_DTYPE = np.dtype([("n_pairs", "<u8"), ("how_count", "<u8", (8,))])
assert PAIR_TOTALS_DTYPE.itemsize == 72
# read extraction (cls_extract_totals, CLS_SELECT_*)
SELECT_UNPLACED = 1
EXTRACT_TOTALS_DTYPE = np.dtype([("n_records", "<u8"), ("n_selected", "<u8"), ("n_selected_unplaced", "<u8"), ("bytes_out", "<u8")])
assert EXTRACT_TOTALS_DTYPE.itemsize == 32
assert NODE_DTYPE.itemsize == 32 and PLACEMENT_DTYPE.itemsize == 24 and STATS_DTYPE.itemsize == 24
assert TALLY_ROW_DTYPE.itemsize == 64 and TALLY_TOTALS_DTYPE.itemsize == 120
