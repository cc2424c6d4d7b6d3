"""ctypes binding of libclsplace.so -- the C-ABI of include/cls_place.h.

Host-side plumbing only: every placement runs in the HIP kernels behind
`cls_place_batch*`; there is no CPU fallback, and a missing or unloadable
extension raises instead of degrading.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _abi
from .flatdb import FlatDb

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CLS_PLACE_LIB: an experiment build of the same library, tools/build_variant.sh)
LIB_PATH = os.environ.get("CLS_PLACE_LIB") or os.path.join(_HERE, "csrc", "libclsplace.so")
_LIB = None

EXPORTS = [
    "cls_device_count", "cls_db_create", "cls_db_validate", "cls_db_destroy", "cls_db_info_get", "cls_db_info_get2", "cls_db_kernel_time", "cls_db_kernel_name",
    "cls_db_read_classes", "cls_db_set_max_read_len", "cls_place_batch",
    "cls_db_group_create", "cls_db_group_destroy", "cls_db_group_size", "cls_db_group_replica", "cls_place_batch_group", "cls_fasta_split",
    "cls_place_batch_device", "cls_place_batch_stats", "cls_fasta_parse", "cls_fasta_free", "cls_fasta_scan_device", "cls_fasta_dev_free",
    "cls_fasta_parse_gpu", "cls_place_fasta_text", "cls_fastq_parse", "cls_fastq_split", "cls_fastq_scan_device", "cls_fastq_parse_gpu",
    "cls_place_fastq_text", "cls_last_error",
    "cls_tally_create", "cls_tally_destroy", "cls_tally_reset", "cls_tally_add_device", "cls_tally_add", "cls_tally_read", "cls_tally_host",
    "cls_tally_merge", "cls_tally_fasta_text", "cls_tally_fastq_text",
    "cls_pairer_create", "cls_pairer_destroy", "cls_pairer_totals", "cls_pair_records_device", "cls_pair_records", "cls_pair_host",
    "cls_pair_names_host", "cls_pair_names_device", "cls_place_fastq_pairs_text", "cls_tally_fastq_pairs_text",
    "cls_selector_create", "cls_selector_destroy", "cls_select_records_device", "cls_select_records", "cls_select_host",
    "cls_fastq_spans_device", "cls_extract_plan_device", "cls_extract_gather_device", "cls_extract_host", "cls_extract_fastq_text",
    "cls_extract_fastq_pairs_text",
    "cls_version", "cls_set_tuning", "cls_tuning_from_env", "cls_kmers_build", "cls_kmers_desc", "cls_kmers_info_get", "cls_kmers_free",
]
HOST_EXPORTS = [
    "cls_tree_load_json", "cls_tree_load", "cls_tree_init_from_file", "cls_tree_from_newick", "cls_tree_serialize", "cls_tree_save", "cls_tree_free", "cls_tree_set_annotations_yaml", "cls_tree_build_kmers_map", "cls_tree_build_kmers_map_device", "cls_tree_desc", "cls_serialize_results",
    "cls_host_free", "cls_place_sequences", "cls_place_sequences_group", "cls_place_sequences_ex", "cls_place_sequences_group_ex",
    "cls_host_last_error", "cls_tally_report", "cls_profile_sequences", "cls_profile_sequences_group", "cls_place_sequences_report", "cls_tree_nodes",
    "cls_place_pairs", "cls_extract_reads",
]
SERVICE_EXPORTS = [
    "cls_service_create", "cls_service_destroy", "cls_service_add_model", "cls_service_submit", "cls_service_wait", "cls_service_pause",
    "cls_service_stats_get",
]
FORMAT_YAML, FORMAT_JSONL = 0, 1
DB_FORMAT_ZSTD, DB_FORMAT_YAML, DB_FORMAT_JSON = 0, 1, 2


class ClsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.msg = msg


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the placement path has no CPU fallback)"
            )
        L = C.CDLL(LIB_PATH)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        L.cls_device_count.restype = i32
        L.cls_db_create.argtypes = [C.POINTER(_abi.DbDesc), i32, C.POINTER(vp)]
        L.cls_db_create.restype = i32
        L.cls_db_validate.argtypes = [C.POINTER(_abi.DbDesc)]
        L.cls_db_validate.restype = i32
        L.cls_db_destroy.argtypes = [vp]
        L.cls_db_destroy.restype = None
        L.cls_db_info_get.argtypes = [vp, C.POINTER(_abi.DbInfo)]
        L.cls_db_info_get.restype = i32
        L.cls_db_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), i32]
        L.cls_db_kernel_time.restype = i32
        L.cls_db_kernel_name.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.cls_db_kernel_name.restype = i32
        L.cls_db_read_classes.argtypes = [vp, C.c_uint64, i32, C.POINTER(_abi.ReadClass), i32, C.POINTER(i32)]
        L.cls_db_read_classes.restype = i32
        L.cls_db_set_max_read_len.argtypes = [vp, C.c_uint64]
        L.cls_db_set_max_read_len.restype = i32
        L.cls_place_batch.argtypes = [vp, vp, vp, u32, C.POINTER(_abi.Params), vp]
        L.cls_place_batch.restype = i32
        L.cls_place_batch_stats.argtypes = [vp, vp, vp, u32, C.POINTER(_abi.Params), vp, vp]
        L.cls_place_batch_stats.restype = i32
        L.cls_place_batch_device.argtypes = [vp, vp, vp, u32, C.POINTER(_abi.Params), vp, vp, vp]
        L.cls_place_batch_device.restype = i32
        L.cls_db_group_create.argtypes = [C.POINTER(_abi.DbDesc), C.POINTER(i32), u32, C.POINTER(vp)]
        L.cls_db_group_create.restype = i32
        L.cls_db_group_destroy.argtypes = [vp]
        L.cls_db_group_destroy.restype = None
        L.cls_db_group_size.argtypes = [vp, C.POINTER(u32)]
        L.cls_db_group_size.restype = i32
        L.cls_db_group_replica.argtypes = [vp, u32, C.POINTER(vp)]
        L.cls_db_group_replica.restype = i32
        L.cls_place_batch_group.argtypes = [vp, vp, vp, u32, C.POINTER(_abi.Params), vp, vp]
        L.cls_place_batch_group.restype = i32
        L.cls_fasta_split.argtypes = [C.c_char_p, C.c_size_t, u32, C.POINTER(C.c_uint64), C.POINTER(u32)]
        L.cls_fasta_split.restype = i32
        L.cls_fasta_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_abi.Fasta)]
        L.cls_fasta_parse.restype = i32
        L.cls_fasta_parse_gpu.argtypes = [C.c_char_p, C.c_size_t, i32, C.POINTER(_abi.Fasta)]
        L.cls_fasta_parse_gpu.restype = i32
        L.cls_place_fasta_text.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(_abi.Fasta), C.POINTER(vp)]
        L.cls_place_fasta_text.restype = i32
        L.cls_fastq_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_abi.FastqOpts), C.POINTER(_abi.Fasta)]
        L.cls_fastq_parse.restype = i32
        L.cls_fastq_parse_gpu.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_abi.FastqOpts), i32, C.POINTER(_abi.Fasta)]
        L.cls_fastq_parse_gpu.restype = i32
        L.cls_fastq_split.argtypes = [C.c_char_p, C.c_size_t, u32, C.POINTER(C.c_uint64), C.POINTER(u32)]
        L.cls_fastq_split.restype = i32
        L.cls_place_fastq_text.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(_abi.FastqOpts), C.POINTER(_abi.Fasta),
                                           C.POINTER(vp)]
        L.cls_place_fastq_text.restype = i32
        L.cls_tally_create.argtypes = [vp, C.POINTER(vp)]
        L.cls_tally_create.restype = i32
        L.cls_tally_destroy.argtypes = [vp]
        L.cls_tally_destroy.restype = None
        L.cls_tally_reset.argtypes = [vp]
        L.cls_tally_reset.restype = i32
        L.cls_tally_add_device.argtypes = [vp, vp, u32, vp]
        L.cls_tally_add_device.restype = i32
        L.cls_tally_add.argtypes = [vp, vp, u32]
        L.cls_tally_add.restype = i32
        L.cls_tally_read.argtypes = [vp, vp, u32, vp]
        L.cls_tally_read.restype = i32
        L.cls_tally_host.argtypes = [vp, u32, vp, C.c_uint64, vp, vp]
        L.cls_tally_host.restype = i32
        L.cls_tally_merge.argtypes = [vp, vp, vp, vp, u32]
        L.cls_tally_merge.restype = i32
        L.cls_tally_fasta_text.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(u32), C.POINTER(u32)]
        L.cls_tally_fasta_text.restype = i32
        L.cls_tally_fastq_text.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(_abi.FastqOpts), C.POINTER(u32),
                                           C.POINTER(u32)]
        L.cls_tally_fastq_text.restype = i32
        u64 = C.c_uint64
        L.cls_pairer_create.argtypes = [vp, C.POINTER(vp)]
        L.cls_pairer_create.restype = i32
        L.cls_pairer_destroy.argtypes = [vp]
        L.cls_pairer_destroy.restype = None
        L.cls_pairer_totals.argtypes = [vp, vp, i32]
        L.cls_pairer_totals.restype = i32
        L.cls_pair_records_device.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp]
        L.cls_pair_records_device.restype = i32
        L.cls_pair_records.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
        L.cls_pair_records.restype = i32
        L.cls_pair_host.argtypes = [vp, u32, vp, vp, u32, u64, u32, vp, vp, vp]
        L.cls_pair_host.restype = i32
        L.cls_pair_names_host.argtypes = [vp, vp, vp, vp, u32, u64, C.POINTER(u64), C.POINTER(u64)]
        L.cls_pair_names_host.restype = i32
        L.cls_pair_names_device.argtypes = [vp, vp, vp, vp, u32, u32, C.POINTER(u64), C.POINTER(u64), vp]
        L.cls_pair_names_device.restype = i32
        L.cls_place_fastq_pairs_text.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params),
                                                 C.POINTER(_abi.FastqOpts), u32, C.POINTER(_abi.Fasta), C.POINTER(vp), C.POINTER(vp)]
        L.cls_place_fastq_pairs_text.restype = i32
        L.cls_tally_fastq_pairs_text.argtypes = [vp, vp, vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params),
                                                 C.POINTER(_abi.FastqOpts), u32, C.POINTER(u32), C.POINTER(u32)]
        L.cls_tally_fastq_pairs_text.restype = i32
        L.cls_selector_create.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(vp)]
        L.cls_selector_create.restype = i32
        L.cls_selector_destroy.argtypes = [vp]
        L.cls_selector_destroy.restype = None
        L.cls_select_records_device.argtypes = [vp, vp, u32, vp, vp]
        L.cls_select_records_device.restype = i32
        L.cls_select_records.argtypes = [vp, vp, u32, vp]
        L.cls_select_records.restype = i32
        L.cls_select_host.argtypes = [vp, u32, vp, u32, vp, u32, u32, vp, u64, vp]
        L.cls_select_host.restype = i32
        L.cls_fastq_spans_device.argtypes = [vp, u64, u32, vp, vp]
        L.cls_fastq_spans_device.restype = i32
        L.cls_extract_plan_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
        L.cls_extract_plan_device.restype = i32
        L.cls_extract_gather_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
        L.cls_extract_gather_device.restype = i32
        L.cls_extract_host.argtypes = [C.c_char_p, C.c_size_t, u32, vp, u64, C.POINTER(vp), C.POINTER(C.c_size_t), vp]
        L.cls_extract_host.restype = i32
        L.cls_extract_fastq_text.argtypes = [vp, vp, vp, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(_abi.FastqOpts), C.POINTER(vp),
                                             C.POINTER(C.c_size_t), vp, C.POINTER(u32), C.POINTER(u32)]
        L.cls_extract_fastq_text.restype = i32
        L.cls_extract_fastq_pairs_text.argtypes = [vp, vp, vp, vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params),
                                                   C.POINTER(_abi.FastqOpts), u32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                                   C.POINTER(C.c_size_t), vp, C.POINTER(u32), C.POINTER(u32)]
        L.cls_extract_fastq_pairs_text.restype = i32
        L.cls_fasta_free.argtypes = [C.POINTER(_abi.Fasta)]
        L.cls_fasta_free.restype = None
        L.cls_last_error.restype = C.c_char_p
        L.cls_version.restype = C.c_char_p
        L.cls_set_tuning.argtypes = [C.c_char_p, i32]
        L.cls_set_tuning.restype = i32
        L.cls_tuning_from_env.argtypes = []
        L.cls_tuning_from_env.restype = None
        L.cls_kmers_build.argtypes = [C.POINTER(_abi.BuildDesc), i32, C.POINTER(vp)]
        L.cls_kmers_build.restype = i32
        L.cls_kmers_desc.argtypes = [vp, C.POINTER(_abi.BuildDesc), C.POINTER(_abi.DbDesc)]
        L.cls_kmers_desc.restype = i32
        L.cls_kmers_info_get.argtypes = [vp, C.POINTER(_abi.KmersInfo)]
        L.cls_kmers_info_get.restype = i32
        L.cls_kmers_free.argtypes = [vp]
        L.cls_kmers_free.restype = None
        # host-side mirror (include/cls_host.h)
        L.cls_tree_load_json.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.cls_tree_load_json.restype = i32
        L.cls_tree_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.cls_tree_load.restype = i32
        L.cls_tree_init_from_file.argtypes = [C.c_char_p, C.c_double, C.POINTER(vp)]
        L.cls_tree_init_from_file.restype = i32
        L.cls_tree_from_newick.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.POINTER(vp)]
        L.cls_tree_from_newick.restype = i32
        L.cls_tree_serialize.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.cls_tree_serialize.restype = i32
        L.cls_tree_save.argtypes = [vp, C.c_char_p, i32, i32]
        L.cls_tree_save.restype = i32
        L.cls_tree_free.argtypes = [vp]
        L.cls_tree_free.restype = None
        L.cls_tree_set_annotations_yaml.argtypes = [vp, C.c_char_p]
        L.cls_tree_set_annotations_yaml.restype = i32
        L.cls_tree_build_kmers_map.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, u32]
        L.cls_tree_build_kmers_map.restype = i32
        L.cls_tree_build_kmers_map_device.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, u32, i32]
        L.cls_tree_build_kmers_map_device.restype = i32
        L.cls_tree_desc.argtypes = [vp, C.POINTER(_abi.DbDesc)]
        L.cls_tree_desc.restype = i32
        L.cls_serialize_results.argtypes = [vp, C.c_char_p, vp, u32, vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t),
                                            C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.cls_serialize_results.restype = i32
        L.cls_host_free.argtypes = [vp]
        L.cls_host_free.restype = None
        L.cls_place_sequences.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params), i32, i32,
                                          C.POINTER(u32), C.POINTER(C.c_double)]
        L.cls_place_sequences.restype = i32
        L.cls_place_sequences_group.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params), i32, i32,
                                                C.POINTER(u32), C.POINTER(C.c_double)]
        L.cls_place_sequences_group.restype = i32
        for name in ("cls_place_sequences_ex", "cls_place_sequences_group_ex"):
            getattr(L, name).argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params), i32, i32, i32, C.POINTER(_abi.FastqOpts),
                                         C.POINTER(u32), C.POINTER(C.c_double)]
            getattr(L, name).restype = i32
        L.cls_host_last_error.restype = C.c_char_p
        L.cls_tree_nodes.argtypes = [vp, C.POINTER(C.POINTER(_abi.Node)), C.POINTER(u32)]
        L.cls_tree_nodes.restype = i32
        L.cls_tally_report.argtypes = [vp, vp, vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.cls_tally_report.restype = i32
        for name in ("cls_profile_sequences", "cls_profile_sequences_group"):
            getattr(L, name).argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params), i32, i32, C.POINTER(_abi.FastqOpts), C.c_uint64, i32,
                                         C.POINTER(u32), C.POINTER(C.c_double)]
            getattr(L, name).restype = i32
        L.cls_place_sequences_report.argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params), i32, i32, i32, C.POINTER(_abi.FastqOpts),
                                                 C.c_char_p, i32, C.POINTER(u32), C.POINTER(C.c_double)]
        L.cls_place_sequences_report.restype = i32
        L.cls_place_pairs.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(_abi.Params),
                                      C.POINTER(_abi.FastqOpts), u32, i32, i32, i32, C.POINTER(u32), C.POINTER(C.c_double)]
        L.cls_place_pairs.restype = i32
        L.cls_extract_reads.argtypes = [vp, vp, C.c_char_p, C.c_char_p, i32, vp, u32, vp, u32, u32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                        C.POINTER(_abi.Params), C.POINTER(_abi.FastqOpts), u32, i32, i32, C.c_uint64, vp, C.POINTER(u32),
                                        C.POINTER(C.c_double)]
        L.cls_extract_reads.restype = i32
        # resident batching service (include/cls_service.h)
        L.cls_service_create.argtypes = [C.POINTER(vp)]
        L.cls_service_create.restype = i32
        L.cls_service_destroy.argtypes = [vp]
        L.cls_service_destroy.restype = None
        L.cls_service_add_model.argtypes = [vp, C.c_char_p, vp]
        L.cls_service_add_model.restype = i32
        L.cls_service_submit.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(_abi.Params), C.POINTER(C.c_uint64)]
        L.cls_service_submit.restype = i32
        L.cls_service_wait.argtypes = [vp, C.c_uint64, C.POINTER(_abi.Fasta), C.POINTER(vp)]
        L.cls_service_wait.restype = i32
        L.cls_service_pause.argtypes = [vp, i32]
        L.cls_service_pause.restype = i32
        L.cls_service_stats_get.argtypes = [vp, C.POINTER(_abi.ServiceStats)]
        L.cls_service_stats_get.restype = i32
        _LIB = L
    return _LIB


def _check(rc: int):
    if rc != 0:
        raise ClsError(rc, lib().cls_last_error().decode(errors="replace"))


def make_params(max_iterations: Optional[int] = None, min_match_coverage: Optional[float] = None,
                remove_intersection: Optional[bool] = None) -> _abi.Params:
    """The three Option<> arguments of place_sequence (place_sequence.rs:46-48)."""
    p = _abi.Params()
    if max_iterations is not None:
        p.flags |= _abi.HAS_MAX_ITERATIONS
        p.max_iterations = max_iterations
    if min_match_coverage is not None:
        p.flags |= _abi.HAS_MIN_MATCH_COVERAGE
        p.min_match_coverage = min_match_coverage
    if remove_intersection is not None:
        p.flags |= _abi.HAS_REMOVE_INTERSECTION
        p.remove_intersection = 1 if remove_intersection else 0
    return p


def set_tuning(name: str, value: int) -> None:
    """An experiment knob of the library (csrc/cls_tuning.h); none changes a result."""
    _check(lib().cls_set_tuning(name.encode(), int(value)))


def tuning_from_env() -> None:
    """Take every knob from its CLS_* environment variable (tools/ and A/B runs; the library never does on its own)."""
    lib().cls_tuning_from_env()


def device_count() -> int:
    return lib().cls_device_count()


def validate(flat: FlatDb) -> None:
    d = flat.desc()
    _check(lib().cls_db_validate(C.byref(d)))


def fasta_parse(text: bytes, device: Optional[int] = None):
    """-> (headers: list[bytes], bases u8[], offsets u64[n+1], truncated: bool); a1 semantics.
    `device`: run the stage's data-parallel passes on that GPU (cls_fasta_parse_gpu) instead of the host parser."""
    f = _abi.Fasta()
    if device is None:
        _check(lib().cls_fasta_parse(text, len(text), C.byref(f)))
    else:
        _check(lib().cls_fasta_parse_gpu(text, len(text), device, C.byref(f)))
    try:
        n = f.n
        hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
        boff = np.ctypeslib.as_array(f.base_off, shape=(n + 1,)).copy()
        hraw = C.string_at(f.headers, int(hoff[-1]))
        bases = np.frombuffer(C.string_at(f.bases, int(boff[-1])), dtype=np.uint8).copy()
        headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
        return headers, bases, boff, bool(f.truncated)
    finally:
        lib().cls_fasta_free(C.byref(f))


def _fastq_opts(trim_5p: int = 0, trim_3p: int = 0) -> _abi.FastqOpts:
    o = _abi.FastqOpts()
    o.trim_5p, o.trim_3p = int(trim_5p), int(trim_3p)
    return o


def fastq_parse(text: bytes, device: Optional[int] = None, trim_5p: int = 0, trim_3p: int = 0):
    """Strict four-line FASTQ, quality-trimmed (include/cls_place.h) -> the tuple of fasta_parse.
    `device`: run the stage's data-parallel passes on that GPU (cls_fastq_parse_gpu) instead of the host parser."""
    f = _abi.Fasta()
    o = _fastq_opts(trim_5p, trim_3p)
    if device is None:
        _check(lib().cls_fastq_parse(text, len(text), C.byref(o), C.byref(f)))
    else:
        _check(lib().cls_fastq_parse_gpu(text, len(text), C.byref(o), device, C.byref(f)))
    try:
        n = f.n
        hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
        boff = np.ctypeslib.as_array(f.base_off, shape=(n + 1,)).copy()
        hraw = C.string_at(f.headers, int(hoff[-1]))
        bases = np.frombuffer(C.string_at(f.bases, int(boff[-1])), dtype=np.uint8).copy()
        headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
        return headers, bases, boff, bool(f.truncated)
    finally:
        lib().cls_fasta_free(C.byref(f))


def fastq_split(text: bytes, max_pieces: int) -> list:
    """Cut points for parsing FASTQ `text` in up to `max_pieces` pieces (cls_fastq_split): [0, ..., len(text)]."""
    cuts = (C.c_uint64 * (max_pieces + 1))()
    n = C.c_uint32(0)
    _check(lib().cls_fastq_split(text, len(text), max_pieces, cuts, C.byref(n)))
    return [int(c) for c in cuts[: n.value + 1]]


def build_kmers(nodes: np.ndarray, bases: np.ndarray, offsets: np.ndarray, leaf_ids: np.ndarray, k: int, m: int, *,
                leaves_only: bool = False, forward_only: bool = False, device: int = 0, return_info: bool = False):
    """The k-mer index of `nodes` (NODE_DTYPE rows) built on the GPU from records `bases[offsets[i]:offsets[i+1]]`
    (filtered upper-case ACGT), record i filed under the LEAF clade `leaf_ids[i]` (cls_kmers_build) -> FlatDb in
    canonical order; with `return_info`, (FlatDb, dict of cls_kmers_info)."""
    nodes = np.ascontiguousarray(nodes, dtype=_abi.NODE_DTYPE)
    bases = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    leaf_ids = np.ascontiguousarray(leaf_ids, dtype=np.uint64)
    if len(offsets) != len(leaf_ids) + 1:
        raise ValueError("offsets must hold one entry more than leaf_ids")
    b = _abi.BuildDesc()
    b.abi_version = _abi.ABI_VERSION
    b.n_nodes = len(nodes)
    b.nodes = nodes.ctypes.data_as(C.POINTER(_abi.Node))
    b.k_size, b.m_size = k, m
    b.n_records = len(leaf_ids)
    b.flags = (_abi.BUILD_LEAVES_ONLY if leaves_only else 0) | (_abi.BUILD_FORWARD_ONLY if forward_only else 0)
    b.bases = bases.ctypes.data
    b.offsets = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    b.leaf_id = leaf_ids.ctypes.data_as(C.POINTER(C.c_uint64))
    km = C.c_void_p()
    _check(lib().cls_kmers_build(C.byref(b), device, C.byref(km)))
    try:
        d = _abi.DbDesc()
        _check(lib().cls_kmers_desc(km, C.byref(b), C.byref(d)))
        flat = FlatDb.from_desc(d, copy=True)
        inf = _abi.KmersInfo()
        _check(lib().cls_kmers_info_get(km, C.byref(inf)))
    finally:
        lib().cls_kmers_free(km)
    if return_info:
        return flat, {name: getattr(inf, name) for name, _ in _abi.KmersInfo._fields_}
    return flat


def fasta_split(text: bytes, max_pieces: int) -> list:
    """Cut points for parsing `text` in up to `max_pieces` pieces (cls_fasta_split): [0, ..., len(text)]."""
    cuts = (C.c_uint64 * (max_pieces + 1))()
    n = C.c_uint32(0)
    _check(lib().cls_fasta_split(text, len(text), max_pieces, cuts, C.byref(n)))
    return [int(c) for c in cuts[: n.value + 1]]


class PlacementDb:
    """Owned handle on a device-resident index (cls_db)."""

    def __init__(self, flat: FlatDb, device: int = -1):
        self._h = C.c_void_p()
        d = flat.desc()
        _check(lib().cls_db_create(C.byref(d), device, C.byref(self._h)))
        info = _abi.DbInfo()
        _check(lib().cls_db_info_get(self._h, C.byref(info)))
        self.info = info

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def refresh_info(self):
        """Re-read cls_db_info (scratch_slots and max_read_kmers change over a handle's life)."""
        _check(lib().cls_db_info_get(self._h, C.byref(self.info)))
        return self.info

    def kernel_name(self) -> str:
        """Template instance of the dominant placement kernel this handle launches (cls_db_kernel_name)."""
        buf = C.create_string_buffer(256)
        _check(lib().cls_db_kernel_name(self._h, buf, len(buf)))
        return buf.value.decode()

    def read_classes(self, n_bases: int = 0, stats: bool = False):
        """Test and measurement aid (cls_db_read_classes): the read-length classes of a device-buffer launch provisioned
        for reads of up to `n_bases` bases (0: the default), in binning order -> [(list, max_kmers, kernel instance)].
        Follows the tuning knobs at the time of the call."""
        buf = (_abi.ReadClass * 8)()
        n = C.c_int(0)
        _check(lib().cls_db_read_classes(self._h, n_bases, 1 if stats else 0, buf, len(buf), C.byref(n)))
        assert n.value <= len(buf)
        return [(int(c.list), int(c.max_kmers), c.kernel.decode()) for c in buf[:n.value]]

    def place_batch(self, bases: np.ndarray, offsets: np.ndarray, params: Optional[_abi.Params] = None,
                    want_stats: bool = False, out: Optional[np.ndarray] = None):
        """Host buffers in, host records out (cls_place_batch / cls_place_batch_stats).  `out`: caller-owned record
        array (e.g. in pinned memory) to fill instead of a fresh one."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if out is None:
            out = np.zeros(n, dtype=_abi.PLACEMENT_DTYPE)
        assert out.dtype == _abi.PLACEMENT_DTYPE and len(out) >= n and out.flags.c_contiguous
        pp = C.byref(params) if params is not None else None
        if want_stats:
            stats = np.zeros(n, dtype=_abi.STATS_DTYPE)
            _check(lib().cls_place_batch_stats(self._h, bases.ctypes.data, offsets.ctypes.data, n, pp,
                                               out.ctypes.data, stats.ctypes.data))
            return out, stats
        _check(lib().cls_place_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, pp, out.ctypes.data))
        return out

    def kernel_time(self, reset: bool = False):
        """(sum of ms, launches) of the dominant placement kernel since the last reset (cls_db_kernel_time)."""
        ms, cnt = C.c_double(0), C.c_uint64(0)
        _check(lib().cls_db_kernel_time(self._h, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value

    def place_fasta_text(self, text: bytes, params: Optional[_abi.Params] = None):
        """FASTA text -> (headers, records, truncated) with the FASTA stage and the placement on the device
        (cls_place_fasta_text): the reads never return to the host."""
        f = _abi.Fasta()
        recs = C.c_void_p()
        pp = C.byref(params) if params is not None else None
        _check(lib().cls_place_fasta_text(self._h, text, len(text), pp, C.byref(f), C.byref(recs)))
        try:
            n = f.n
            hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
            hraw = C.string_at(f.headers, int(hoff[-1]))
            headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
            out = np.frombuffer(C.string_at(recs, n * 24), dtype=_abi.PLACEMENT_DTYPE).copy() if n else np.zeros(0, _abi.PLACEMENT_DTYPE)
            return headers, out, bool(f.truncated)
        finally:
            lib().cls_fasta_free(C.byref(f))
            lib().cls_host_free(recs)

    def place_fastq_text(self, text: bytes, params: Optional[_abi.Params] = None, trim_5p: int = 0, trim_3p: int = 0):
        """FASTQ text -> (headers, records, truncated), parsed and quality-trimmed on the device and placed there
        (cls_place_fastq_text)."""
        f = _abi.Fasta()
        recs = C.c_void_p()
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_place_fastq_text(self._h, text, len(text), pp, C.byref(o), C.byref(f), C.byref(recs)))
        try:
            n = f.n
            hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
            hraw = C.string_at(f.headers, int(hoff[-1]))
            headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
            out = np.frombuffer(C.string_at(recs, n * 24), dtype=_abi.PLACEMENT_DTYPE).copy() if n else np.zeros(0, _abi.PLACEMENT_DTYPE)
            return headers, out, bool(f.truncated)
        finally:
            lib().cls_fasta_free(C.byref(f))
            lib().cls_host_free(recs)

    def tally_fasta_text(self, tally: "Tally", text: bytes, params: Optional[_abi.Params] = None):
        """FASTA text -> records added to `tally` on the device; nothing per read returns (cls_tally_fasta_text)
        -> (records placed, truncated)."""
        n, tr = C.c_uint32(0), C.c_uint32(0)
        pp = C.byref(params) if params is not None else None
        _check(lib().cls_tally_fasta_text(self._h, tally._h, text, len(text), pp, C.byref(n), C.byref(tr)))
        return n.value, bool(tr.value)

    def tally_fastq_text(self, tally: "Tally", text: bytes, params: Optional[_abi.Params] = None, trim_5p: int = 0, trim_3p: int = 0):
        """The FASTQ twin (cls_tally_fastq_text) -> (records placed, truncated)."""
        n, tr = C.c_uint32(0), C.c_uint32(0)
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_tally_fastq_text(self._h, tally._h, text, len(text), pp, C.byref(o), C.byref(n), C.byref(tr)))
        return n.value, bool(tr.value)

    def place_fastq_pairs_text(self, pairer: "Pairer", text1: bytes, text2: Optional[bytes] = None, params: Optional[_abi.Params] = None,
                               trim_5p: int = 0, trim_3p: int = 0, flags: int = 0):
        """Paired FASTQ text (`text2` None: `text1` is interleaved) -> (mate 1's headers, P, how, truncated): both mates
        placed as one batch and reconciled on the device (cls_place_fastq_pairs_text); the classes go to `pairer`."""
        f = _abi.Fasta()
        recs, how = C.c_void_p(), C.c_void_p()
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_place_fastq_pairs_text(self._h, pairer._h, text1, len(text1), text2, len(text2) if text2 is not None else 0, pp,
                                                C.byref(o), flags, C.byref(f), C.byref(recs), C.byref(how)))
        try:
            n = f.n
            hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
            hraw = C.string_at(f.headers, int(hoff[-1]))
            headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
            out = np.frombuffer(C.string_at(recs, n * 24), dtype=_abi.PLACEMENT_DTYPE).copy() if n else np.zeros(0, _abi.PLACEMENT_DTYPE)
            hw = np.frombuffer(C.string_at(how, n), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
            return headers, out, hw, bool(f.truncated)
        finally:
            lib().cls_fasta_free(C.byref(f))
            lib().cls_host_free(recs)
            lib().cls_host_free(how)

    def tally_fastq_pairs_text(self, pairer: "Pairer", tally: "Tally", text1: bytes, text2: Optional[bytes] = None,
                               params: Optional[_abi.Params] = None, trim_5p: int = 0, trim_3p: int = 0, flags: int = 0):
        """The same pipeline with P added to `tally` on the device (cls_tally_fastq_pairs_text) -> (pairs, truncated)."""
        n, tr = C.c_uint32(0), C.c_uint32(0)
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_tally_fastq_pairs_text(self._h, pairer._h, tally._h, text1, len(text1), text2, len(text2) if text2 is not None else 0,
                                                pp, C.byref(o), flags, C.byref(n), C.byref(tr)))
        return n.value, bool(tr.value)

    def extract_fastq_text(self, selector: "Selector", text: bytes, tally: Optional["Tally"] = None, params: Optional[_abi.Params] = None,
                           trim_5p: int = 0, trim_3p: int = 0):
        """FASTQ text -> (the selected records' bytes, totals: EXTRACT_TOTALS_DTYPE scalar, records placed, truncated): placed and
        selected on the device, only the selected bytes return (cls_extract_fastq_text).  `tally` also receives the records."""
        out, out_len = C.c_void_p(), C.c_size_t(0)
        tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
        n, tr = C.c_uint32(0), C.c_uint32(0)
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_extract_fastq_text(self._h, selector._h, tally._h if tally is not None else None, text, len(text), pp, C.byref(o),
                                            C.byref(out), C.byref(out_len), tot.ctypes.data, C.byref(n), C.byref(tr)))
        try:
            return C.string_at(out, out_len.value), tot[0], n.value, bool(tr.value)
        finally:
            lib().cls_host_free(out)

    def extract_fastq_pairs_text(self, pairer: "Pairer", selector: "Selector", text1: bytes, text2: Optional[bytes] = None,
                                 tally: Optional["Tally"] = None, params: Optional[_abi.Params] = None, trim_5p: int = 0, trim_3p: int = 0,
                                 flags: int = 0):
        """Paired FASTQ text (`text2` None: interleaved) -> (out1, out2 or None, totals, pairs, truncated): the pair's record
        decides for both mates (cls_extract_fastq_pairs_text)."""
        o1, l1, o2, l2 = C.c_void_p(), C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
        tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
        n, tr = C.c_uint32(0), C.c_uint32(0)
        pp = C.byref(params) if params is not None else None
        o = _fastq_opts(trim_5p, trim_3p)
        _check(lib().cls_extract_fastq_pairs_text(self._h, pairer._h, selector._h, tally._h if tally is not None else None, text1, len(text1),
                                                  text2, len(text2) if text2 is not None else 0, pp, C.byref(o), flags, C.byref(o1),
                                                  C.byref(l1), C.byref(o2), C.byref(l2), tot.ctypes.data, C.byref(n), C.byref(tr)))
        try:
            return (C.string_at(o1, l1.value), C.string_at(o2, l2.value) if text2 is not None else None, tot[0], n.value, bool(tr.value))
        finally:
            lib().cls_host_free(o1)
            lib().cls_host_free(o2)

    def set_max_read_len(self, n_bases: int) -> None:
        """Longest read place_batch_device() provisions for (cls_db_set_max_read_len)."""
        _check(lib().cls_db_set_max_read_len(self._h, n_bases))
        _check(lib().cls_db_info_get(self._h, C.byref(self.info)))

    def place_batch_device(self, d_bases: int, d_offsets: int, n: int, d_out: int, params: Optional[_abi.Params] = None,
                           d_stats: int = 0, stream: int = 0) -> None:
        """Device pointers in/out, asynchronous on `stream` (cls_place_batch_device)."""
        pp = C.byref(params) if params is not None else None
        _check(lib().cls_place_batch_device(self._h, d_bases, d_offsets, n, pp, d_out, d_stats or None, stream or None))


class Tally:
    """Device-resident per-clade accumulator bound to one PlacementDb (cls_tally): add placement records batch after
    batch, read one row per clade (in the row order of the FlatDb the handle was made from) plus totals."""

    def __init__(self, db: PlacementDb):
        self._db = db  # (the tally borrows the handle)
        self._h = C.c_void_p()
        _check(lib().cls_tally_create(db._h, C.byref(self._h)))
        self.n_nodes = int(db.info.n_nodes)

    def add(self, records: np.ndarray) -> None:
        """Host records: copied to the device and added there (cls_tally_add)."""
        recs = np.ascontiguousarray(records, dtype=_abi.PLACEMENT_DTYPE)
        _check(lib().cls_tally_add(self._h, recs.ctypes.data, len(recs)))

    def add_device(self, d_records: int, n: int, stream: int = 0) -> None:
        """`n` records in the HBM of the handle's device, asynchronous on `stream` (cls_tally_add_device)."""
        _check(lib().cls_tally_add_device(self._h, d_records or None, n, stream or None))

    def read(self):
        """-> (rows TALLY_ROW_DTYPE[n_nodes], totals: TALLY_TOTALS_DTYPE scalar); waits for the adds in flight."""
        rows = np.zeros(self.n_nodes, dtype=_abi.TALLY_ROW_DTYPE)
        totals = np.zeros(1, dtype=_abi.TALLY_TOTALS_DTYPE)
        _check(lib().cls_tally_read(self._h, rows.ctypes.data, len(rows), totals.ctypes.data))
        return rows, totals[0]

    def reset(self) -> None:
        _check(lib().cls_tally_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_tally_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def tally_host(flat: FlatDb, records: np.ndarray, rows: Optional[np.ndarray] = None, totals: Optional[np.ndarray] = None):
    """The counting rules of the clade tally on the host, no device (cls_tally_host) -> (rows, totals) in the row order
    of `flat.nodes`.  `rows` / `totals` (a 1-element TALLY_TOTALS_DTYPE array) from an earlier call are added to in place."""
    nodes = np.ascontiguousarray(flat.nodes, dtype=_abi.NODE_DTYPE)
    recs = np.ascontiguousarray(records, dtype=_abi.PLACEMENT_DTYPE)
    if rows is None:
        rows = np.zeros(len(nodes), dtype=_abi.TALLY_ROW_DTYPE)
    if totals is None:
        totals = np.zeros(1, dtype=_abi.TALLY_TOTALS_DTYPE)
    assert rows.dtype == _abi.TALLY_ROW_DTYPE and len(rows) == len(nodes) and rows.flags.c_contiguous
    assert totals.dtype == _abi.TALLY_TOTALS_DTYPE and totals.shape == (1,)
    _check(lib().cls_tally_host(nodes.ctypes.data, len(nodes), recs.ctypes.data, len(recs), rows.ctypes.data, totals.ctypes.data))
    return rows, totals


def tally_merge(rows: np.ndarray, totals: np.ndarray, add_rows: np.ndarray, add_totals) -> None:
    """rows += add_rows, totals += add_totals in place (cls_tally_merge): how the tallies of replicas or ranks are summed."""
    add_rows = np.ascontiguousarray(add_rows, dtype=_abi.TALLY_ROW_DTYPE)
    add_totals = np.ascontiguousarray(np.atleast_1d(add_totals), dtype=_abi.TALLY_TOTALS_DTYPE)
    assert rows.dtype == _abi.TALLY_ROW_DTYPE and len(rows) == len(add_rows) and rows.flags.c_contiguous
    assert totals.dtype == _abi.TALLY_TOTALS_DTYPE and totals.shape == (1,)
    _check(lib().cls_tally_merge(rows.ctypes.data, totals.ctypes.data, add_rows.ctypes.data, add_totals.ctypes.data, len(rows)))


class Pairer:
    """Device-resident reconciler of paired reads bound to one PlacementDb (cls_pairer): the two mates' placement records
    -> one record per pair plus a class byte; counts the classes over every call."""

    def __init__(self, db: PlacementDb):
        self._db = db  # (the pairer borrows the handle)
        self._h = C.c_void_p()
        _check(lib().cls_pairer_create(db._h, C.byref(self._h)))

    def pair_device(self, d_a: int, d_b: int, stride: int, n: int, d_out: int, d_how: int = 0, flags: int = 0, stream: int = 0) -> None:
        """Device pointers in / out, asynchronous on `stream` (cls_pair_records_device)."""
        _check(lib().cls_pair_records_device(self._h, d_a or None, d_b or None, stride, n, flags, d_out or None, d_how or None, stream or None))

    def pair(self, a: np.ndarray, b: Optional[np.ndarray] = None, flags: int = 0):
        """Host records through the kernel (cls_pair_records) -> (P, how).  `b` None: `a` is interleaved."""
        return _pair_call(lambda *args: lib().cls_pair_records(self._h, *args), a, b, flags, totals=False)

    def totals(self, reset: bool = False):
        """-> PAIR_TOTALS_DTYPE scalar; waits for the launches in flight (cls_pairer_totals)."""
        t = np.zeros(1, dtype=_abi.PAIR_TOTALS_DTYPE)
        _check(lib().cls_pairer_totals(self._h, t.ctypes.data, 1 if reset else 0))
        return t[0]

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_pairer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _id_list(ids):
    a = np.ascontiguousarray(np.asarray(list(ids) if ids is not None else [], dtype=np.uint64))
    return a, (a.ctypes.data if len(a) else None), len(a)


class Selector:
    """A selection rule on the device of one PlacementDb (cls_selector): include / exclude clade ids, the nearest listed
    clade on a record's path to the root decides; `unplaced` selects the records without a clade of the tree."""

    def __init__(self, db: PlacementDb, include=(), exclude=(), unplaced: bool = False, flags: Optional[int] = None):
        self._db = db  # (the selector borrows the handle)
        self._h = C.c_void_p()
        inc, pi, ni = _id_list(include)
        exc, pe, ne = _id_list(exclude)
        f = flags if flags is not None else (_abi.SELECT_UNPLACED if unplaced else 0)
        _check(lib().cls_selector_create(db._h, pi, ni, pe, ne, f, C.byref(self._h)))

    def select_device(self, d_records: int, n: int, d_sel: int, stream: int = 0) -> None:
        """Device pointers in / out, asynchronous on `stream` (cls_select_records_device)."""
        _check(lib().cls_select_records_device(self._h, d_records or None, n, d_sel or None, stream or None))

    def select(self, records: np.ndarray) -> np.ndarray:
        """Host records through the kernel (cls_select_records) -> one byte per record."""
        recs = np.ascontiguousarray(records, dtype=_abi.PLACEMENT_DTYPE)
        sel = np.full(len(recs), 0xFF, dtype=np.uint8)
        _check(lib().cls_select_records(self._h, recs.ctypes.data, len(recs), sel.ctypes.data))
        return sel

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_selector_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def select_host(flat, records: np.ndarray, include=(), exclude=(), unplaced: bool = False, flags: Optional[int] = None) -> np.ndarray:
    """The selection rule on the host, no device (cls_select_host) -> one byte per record."""
    nodes = np.ascontiguousarray(flat.nodes, dtype=_abi.NODE_DTYPE)
    recs = np.ascontiguousarray(records, dtype=_abi.PLACEMENT_DTYPE)
    inc, pi, ni = _id_list(include)
    exc, pe, ne = _id_list(exclude)
    f = flags if flags is not None else (_abi.SELECT_UNPLACED if unplaced else 0)
    sel = np.full(len(recs), 0xFF, dtype=np.uint8)
    _check(lib().cls_select_host(nodes.ctypes.data, len(nodes), pi, ni, pe, ne, f, recs.ctypes.data, len(recs), sel.ctypes.data))
    return sel


def extract_host(text: bytes, sel: np.ndarray, stride: int = 1):
    """Record text + output on the host, no device (cls_extract_host) -> (bytes, totals).  `sel`: one byte per item."""
    sel = np.ascontiguousarray(sel, dtype=np.uint8)
    out, out_len = C.c_void_p(), C.c_size_t(0)
    tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
    _check(lib().cls_extract_host(text, len(text), stride, sel.ctypes.data if len(sel) else None, len(sel), C.byref(out), C.byref(out_len),
                                  tot.ctypes.data))
    try:
        return C.string_at(out, out_len.value), tot[0]
    finally:
        lib().cls_host_free(out)


def fastq_spans_device(d_text: int, length: int, n: int, d_rec_off: int, stream: int = 0) -> None:
    """rec_off[n + 1] of a FASTQ text in HBM (cls_fastq_spans_device)."""
    _check(lib().cls_fastq_spans_device(d_text or None, length, n, d_rec_off or None, stream or None))


def extract_plan_device(d_text: int, d_rec_off: int, stride: int, n_items: int, d_sel: int, d_out_off: int, stream: int = 0):
    """The plan of the compaction on raw device pointers (cls_extract_plan_device) -> totals."""
    tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
    _check(lib().cls_extract_plan_device(d_text or None, d_rec_off or None, stride, n_items, d_sel or None, d_out_off or None, tot.ctypes.data,
                                         stream or None))
    return tot[0]


def extract_gather_device(d_text: int, d_rec_off: int, stride: int, n_items: int, d_sel: int, d_out_off: int, d_out: int,
                          stream: int = 0) -> None:
    """The gather of the compaction on raw device pointers (cls_extract_gather_device); asynchronous on `stream`."""
    _check(lib().cls_extract_gather_device(d_text or None, d_rec_off or None, stride, n_items, d_sel or None, d_out_off or None, d_out or None,
                                           stream or None))


def _pair_call(fn, a, b, flags, totals):
    """Shared argument plumbing of pair_host / Pairer.pair: `b` None means `a` holds interleaved records (stride 2)."""
    a = np.ascontiguousarray(a, dtype=_abi.PLACEMENT_DTYPE)
    if b is None:
        if len(a) % 2:
            raise ValueError("an interleaved batch holds an even number of records")
        stride, n, pb = 2, len(a) // 2, a.ctypes.data + 24
    else:
        b = np.ascontiguousarray(b, dtype=_abi.PLACEMENT_DTYPE)
        if len(a) != len(b):
            raise ValueError("the two mates' record arrays differ in length")
        stride, n, pb = 1, len(a), b.ctypes.data
    out = np.full(n, 0xFF, dtype=np.uint8).repeat(24).view(_abi.PLACEMENT_DTYPE)  # (pad bytes must come back as 0)
    how = np.full(n, 0xFF, dtype=np.uint8)
    if totals:
        tot = np.zeros(1, dtype=_abi.PAIR_TOTALS_DTYPE)
        _check(fn(a.ctypes.data, pb, stride, n, flags, out.ctypes.data, how.ctypes.data, tot.ctypes.data))
        return out, how, tot[0]
    _check(fn(a.ctypes.data, pb, stride, n, flags, out.ctypes.data, how.ctypes.data))
    return out, how


def pair_host(flat, a: np.ndarray, b: Optional[np.ndarray] = None, flags: int = 0):
    """The pairing rule on the host, no device (cls_pair_host) -> (P, how, totals).  `b` None: `a` is interleaved."""
    nodes = np.ascontiguousarray(flat.nodes, dtype=_abi.NODE_DTYPE)
    return _pair_call(lambda *args: lib().cls_pair_host(nodes.ctypes.data, len(nodes), *args), a, b, flags, totals=True)


def pair_names_host(headers1, headers2=None):
    """The mate-name rule on the host (cls_pair_names_host) -> (disagreeing pairs, lowest disagreeing index or None).
    `headers2` None: `headers1` is an interleaved list (mates alternate)."""
    def pack(hs):
        hb = [h if isinstance(h, bytes) else h.encode() for h in hs]
        return b"".join(hb), np.concatenate([[0], np.cumsum([len(h) for h in hb])]).astype(np.uint64)

    t1, o1 = pack(headers1)
    if headers2 is None:
        if len(headers1) % 2:
            raise ValueError("an interleaved list holds an even number of headers")
        t2, p2, stride, n = t1, o1.ctypes.data + 8, 2, len(headers1) // 2
    else:
        if len(headers1) != len(headers2):
            raise ValueError("the two header lists differ in length")
        t2, o2 = pack(headers2)
        p2, stride, n = o2.ctypes.data, 1, len(headers1)
    n_bad, first = C.c_uint64(0), C.c_uint64(0)
    _check(lib().cls_pair_names_host(t1, o1.ctypes.data, t2, p2, stride, n, C.byref(n_bad), C.byref(first)))
    return n_bad.value, (first.value if n_bad.value else None)


class _ReplicaView(PlacementDb):
    """Non-owning PlacementDb on one replica of a PlacementDbGroup (cls_db_group_replica); keeps the group alive."""

    def __init__(self, group: "PlacementDbGroup", handle: C.c_void_p):
        self._group = group
        self._h = handle
        self.info = _abi.DbInfo()
        _check(lib().cls_db_info_get(self._h, C.byref(self.info)))

    def close(self):
        self._h = C.c_void_p()  # (the group owns the handle)


class PlacementDbGroup:
    """Owned group of replicas of one index (cls_db_group): encoded once, one replica per entry of `devices`
    (repeats allowed; None: every visible device once).  place_batch cuts a batch across the replicas."""

    def __init__(self, flat: FlatDb, devices=None):
        self._h = C.c_void_p()
        d = flat.desc()
        devs = list(devices) if devices is not None else []
        arr = (C.c_int * len(devs))(*devs) if devs else None
        _check(lib().cls_db_group_create(C.byref(d), arr, len(devs), C.byref(self._h)))
        n = C.c_uint32(0)
        _check(lib().cls_db_group_size(self._h, C.byref(n)))
        self.size = n.value

    def replica(self, i: int) -> PlacementDb:
        """Replica i as a PlacementDb view; closing or dropping the view leaves the replica to the group."""
        h = C.c_void_p()
        _check(lib().cls_db_group_replica(self._h, i, C.byref(h)))
        return _ReplicaView(self, h)

    def place_batch(self, bases: np.ndarray, offsets: np.ndarray, params: Optional[_abi.Params] = None,
                    want_stats: bool = False):
        """Host buffers in, host records out, across the replicas (cls_place_batch_group)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(n, dtype=_abi.PLACEMENT_DTYPE)
        stats = np.zeros(n, dtype=_abi.STATS_DTYPE) if want_stats else None
        pp = C.byref(params) if params is not None else None
        _check(lib().cls_place_batch_group(self._h, bases.ctypes.data, offsets.ctypes.data, n, pp, out.ctypes.data,
                                           stats.ctypes.data if want_stats else None))
        return (out, stats) if want_stats else out

    def close(self):
        """Frees every replica: views from replica() must not be used afterwards."""
        if getattr(self, "_h", None):
            lib().cls_db_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _check_host(rc: int):
    if rc != 0:
        msg = lib().cls_host_last_error().decode(errors="replace") or lib().cls_last_error().decode(errors="replace")
        raise ClsError(rc, msg)


class Tree:
    """cls_tree: the reference's database / tree JSON export + optional annotations (include/cls_host.h)."""

    def __init__(self, path: Optional[str] = None, annotations_yaml: Optional[str] = None, *, _handle=None):
        """`path`: a database / tree file in any form load_database reads (.cls zstd YAML, YAML, JSON)."""
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        elif path.endswith(".json"):
            _check_host(lib().cls_tree_load_json(path.encode(), C.byref(self._h)))
        else:
            _check_host(lib().cls_tree_load(path.encode(), C.byref(self._h)))
        if annotations_yaml:
            _check_host(lib().cls_tree_set_annotations_yaml(self._h, annotations_yaml.encode()))

    @classmethod
    def from_newick_file(cls, tree_path: str, min_branch_support: float = 70.0) -> "Tree":
        """Tree::init_from_file: Newick -> sanitized tree (cls_tree_init_from_file)."""
        h = C.c_void_p()
        _check_host(lib().cls_tree_init_from_file(tree_path.encode(), min_branch_support, C.byref(h)))
        return cls(_handle=h)

    @classmethod
    def from_newick(cls, text: str, name: Optional[str] = None, min_branch_support: float = 70.0) -> "Tree":
        h = C.c_void_p()
        _check_host(lib().cls_tree_from_newick(text.encode(), name.encode() if name else None, min_branch_support, C.byref(h)))
        return cls(_handle=h)

    def dumps(self, fmt: int = DB_FORMAT_YAML, only_tree: bool = False) -> bytes:
        """`cls convert database` serialisation (cls_tree_serialize)."""
        buf, n = C.c_void_p(), C.c_size_t()
        _check_host(lib().cls_tree_serialize(self._h, fmt, 1 if only_tree else 0, C.byref(buf), C.byref(n)))
        try:
            return C.string_at(buf, n.value)
        finally:
            lib().cls_host_free(buf)

    def save(self, path: str, fmt: int = DB_FORMAT_ZSTD, only_tree: bool = False) -> None:
        _check_host(lib().cls_tree_save(self._h, path.encode(), fmt, 1 if only_tree else 0))

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_tree_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_kmers_map(self, msa_text: bytes, k_size: int, m_size: int = 4, reference_header_shift: bool = True,
                        forward_only: bool = False) -> None:
        """`cls build-db` (map_kmers_to_tree) on this tree; see include/cls_host.h."""
        flags = (1 if reference_header_shift else 0) | (2 if forward_only else 0)
        _check_host(lib().cls_tree_build_kmers_map(self._h, msa_text, len(msa_text), k_size, m_size, flags))

    def build_kmers_map_device(self, msa_text: bytes, k_size: int, m_size: int = 4, reference_header_shift: bool = True,
                               forward_only: bool = False, device: int = 0, leaves_only: bool = False) -> None:
        """The same map built on the GPU (cls_tree_build_kmers_map_device); `leaves_only` keeps it as CLS_SETS_LEAVES
        (then `dumps` / `save` need only_tree)."""
        flags = ((_abi.BUILD_REFERENCE_HEADER_SHIFT if reference_header_shift else 0) | (_abi.BUILD_FORWARD_ONLY if forward_only else 0)
                 | (_abi.BUILD_LEAVES_ONLY if leaves_only else 0))
        _check_host(lib().cls_tree_build_kmers_map_device(self._h, msa_text, len(msa_text), k_size, m_size, flags, device))

    def flat(self) -> FlatDb:
        d = _abi.DbDesc()
        _check_host(lib().cls_tree_desc(self._h, C.byref(d)))
        return FlatDb.from_desc(d, keepalive=self)

    def nodes(self) -> np.ndarray:
        """The tree's node table (NODE_DTYPE rows, a copy), also for a tree-only file (cls_tree_nodes)."""
        p, n = C.POINTER(_abi.Node)(), C.c_uint32(0)
        _check_host(lib().cls_tree_nodes(self._h, C.byref(p), C.byref(n)))
        return np.frombuffer(C.string_at(p, n.value * 32), dtype=_abi.NODE_DTYPE).copy()

    def report(self, rows: np.ndarray, totals, all_rows: bool = False) -> bytes:
        """The clade report (cls_tally_report, format in include/cls_host.h) of a tally over this tree: `rows` in the
        row order of flat().nodes, as Tally.read / tally_host return them."""
        rows = np.ascontiguousarray(rows, dtype=_abi.TALLY_ROW_DTYPE)
        tot = np.ascontiguousarray(np.atleast_1d(totals), dtype=_abi.TALLY_TOTALS_DTYPE)
        n_nodes = len(self.nodes())
        if len(rows) != n_nodes:
            raise ValueError(f"{len(rows)} rows for a tree of {n_nodes} clades")
        buf, n = C.c_void_p(), C.c_size_t()
        _check_host(lib().cls_tally_report(self._h, rows.ctypes.data, tot.ctypes.data, 1 if all_rows else 0, C.byref(buf), C.byref(n)))
        try:
            return C.string_at(buf, n.value)
        finally:
            lib().cls_host_free(buf)

    def serialize(self, headers, records: np.ndarray, fmt: int = FORMAT_YAML):
        """-> (result text, error text) exactly as `place_sequences` would append them to its two files."""
        hb = [h if isinstance(h, bytes) else h.encode() for h in headers]
        off = np.concatenate([[0], np.cumsum([len(h) for h in hb])]).astype(np.uint64)
        recs = np.ascontiguousarray(records, dtype=_abi.PLACEMENT_DTYPE)
        out, err = C.c_void_p(), C.c_void_p()
        ol, el = C.c_size_t(0), C.c_size_t(0)
        _check_host(lib().cls_serialize_results(self._h, b"".join(hb), off.ctypes.data, len(hb), recs.ctypes.data, fmt,
                                                C.byref(out), C.byref(ol), C.byref(err), C.byref(el)))
        try:
            return C.string_at(out, ol.value), C.string_at(err, el.value)
        finally:
            lib().cls_host_free(out)
            lib().cls_host_free(err)


def _trim_pair(trim_quality):
    if trim_quality is None:
        return 0, 0
    if isinstance(trim_quality, int):
        return 0, trim_quality
    return trim_quality


def profile_sequences(db, tree: Tree, query_path: str, report_path: str, params: Optional[_abi.Params] = None, overwrite: bool = False,
                      query_format: str = "fasta", trim_quality=None, piece_bytes: int = 0, all_rows: bool = False):
    """Query file -> clade report with the reads tallied on the device (cls_profile_sequences, or
    cls_profile_sequences_group when `db` is a PlacementDbGroup) -> (records tallied, seconds).  `piece_bytes`: the
    query is processed in pieces of about that size (0: the library's default)."""
    if query_format not in ("fasta", "fastq"):
        raise ValueError(f"query_format must be 'fasta' or 'fastq', not {query_format!r}")
    if trim_quality is not None and query_format != "fastq":
        raise ValueError("trim_quality needs query_format='fastq'")
    n, sec = C.c_uint32(0), C.c_double(0)
    o = _fastq_opts(*_trim_pair(trim_quality))
    fn = lib().cls_profile_sequences_group if isinstance(db, PlacementDbGroup) else lib().cls_profile_sequences
    _check_host(fn(db._h, tree._h, query_path.encode(), report_path.encode(), C.byref(params) if params is not None else None,
                   1 if overwrite else 0, _abi.QUERY_FASTQ if query_format == "fastq" else _abi.QUERY_FASTA, C.byref(o), piece_bytes,
                   1 if all_rows else 0, C.byref(n), C.byref(sec)))
    return n.value, sec.value


def place_sequences(db, tree: Tree, query_path: str, out_file: str, params: Optional[_abi.Params] = None,
                    overwrite: bool = False, fmt: int = FORMAT_YAML, query_format: str = "fasta", trim_quality=None):
    """The whole use-case (mod.rs:43-270) through cls_place_sequences, or cls_place_sequences_group when `db` is a
    PlacementDbGroup: -> (records read, seconds).  `query_format` "fastq": strict four-line FASTQ, quality-trimmed by
    `trim_quality` (cutadapt's -q: a 3' cutoff, or a (5', 3') pair; None: no trimming), through the _ex entries."""
    if query_format not in ("fasta", "fastq"):
        raise ValueError(f"query_format must be 'fasta' or 'fastq', not {query_format!r}")
    if trim_quality is not None and query_format != "fastq":
        raise ValueError("trim_quality needs query_format='fastq'")
    n, sec = C.c_uint32(0), C.c_double(0)
    group = isinstance(db, PlacementDbGroup)
    pp = C.byref(params) if params is not None else None
    if query_format == "fasta":
        fn = lib().cls_place_sequences_group if group else lib().cls_place_sequences
        _check_host(fn(db._h, tree._h, query_path.encode(), out_file.encode(), pp, 1 if overwrite else 0, fmt, C.byref(n), C.byref(sec)))
        return n.value, sec.value
    if trim_quality is None:
        c5, c3 = 0, 0
    elif isinstance(trim_quality, int):
        c5, c3 = 0, trim_quality
    else:
        c5, c3 = trim_quality
    o = _fastq_opts(c5, c3)
    fn = lib().cls_place_sequences_group_ex if group else lib().cls_place_sequences_ex
    _check_host(fn(db._h, tree._h, query_path.encode(), out_file.encode(), pp, 1 if overwrite else 0, fmt, _abi.QUERY_FASTQ, C.byref(o),
                   C.byref(n), C.byref(sec)))
    return n.value, sec.value


def place_pairs(db: PlacementDb, tree: Tree, query1: str, query2: Optional[str] = None, out_file: Optional[str] = None,
                report_path: Optional[str] = None, summary_path: Optional[str] = None, params: Optional[_abi.Params] = None,
                trim_quality=None, flags: int = 0, fmt: int = FORMAT_YAML, overwrite: bool = False, all_rows: bool = False):
    """The paired-end use-case (cls_place_pairs): FASTQ mate files (`query2` None: `query1` is interleaved) -> per-pair
    result / error files, the clade report and the pair summary, each optional -> (pairs, seconds)."""
    n, sec = C.c_uint32(0), C.c_double(0)
    o = _fastq_opts(*_trim_pair(trim_quality))
    enc = lambda x: x.encode() if x is not None else None
    _check_host(lib().cls_place_pairs(db._h, tree._h, query1.encode(), enc(query2), enc(out_file), enc(report_path), enc(summary_path),
                                      C.byref(params) if params is not None else None, C.byref(o), flags, fmt, 1 if overwrite else 0,
                                      1 if all_rows else 0, C.byref(n), C.byref(sec)))
    return n.value, sec.value


def extract_reads(db: PlacementDb, tree: Tree, query1: str, extract_path1: str, query2: Optional[str] = None, extract_path2: Optional[str] = None,
                  interleaved: bool = False, include=(), exclude=(), unplaced: bool = False, report_path: Optional[str] = None,
                  summary_path: Optional[str] = None, params: Optional[_abi.Params] = None, trim_quality=None, pair_flags: int = 0,
                  overwrite: bool = False, all_rows: bool = False, piece_bytes: int = 0):
    """The read-extraction use-case (cls_extract_reads): FASTQ file(s) -> the FASTQ records of the reads (or pairs) the
    selector picks, plus the optional clade report / pair summary of the same pass -> (totals, records or pairs, seconds)."""
    n, sec = C.c_uint32(0), C.c_double(0)
    o = _fastq_opts(*_trim_pair(trim_quality))
    enc = lambda x: x.encode() if x is not None else None
    inc, pi, ni = _id_list(include)
    exc, pe, ne = _id_list(exclude)
    tot = np.zeros(1, dtype=_abi.EXTRACT_TOTALS_DTYPE)
    _check_host(lib().cls_extract_reads(db._h, tree._h, query1.encode(), enc(query2), 1 if interleaved else 0, pi, ni, pe, ne,
                                        _abi.SELECT_UNPLACED if unplaced else 0, extract_path1.encode(), enc(extract_path2), enc(report_path),
                                        enc(summary_path), C.byref(params) if params is not None else None, C.byref(o), pair_flags,
                                        1 if overwrite else 0, 1 if all_rows else 0, piece_bytes, tot.ctypes.data, C.byref(n), C.byref(sec)))
    return tot[0], n.value, sec.value


class Service:
    """Resident batching service (include/cls_service.h): models stay on the device, waiting jobs share batches."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().cls_service_create(C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().cls_service_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_model(self, model_id: str, db: "PlacementDb") -> None:
        """The service takes the handle over (`db` must not be used or closed afterwards)."""
        _check(lib().cls_service_add_model(self._h, model_id.encode(), db._h))
        db._h = C.c_void_p()

    def submit(self, model_id: str, fasta_text: bytes, params: Optional[_abi.Params] = None) -> int:
        t = C.c_uint64(0)
        _check(lib().cls_service_submit(self._h, model_id.encode(), fasta_text, len(fasta_text),
                                        C.byref(params) if params is not None else None, C.byref(t)))
        return t.value

    def wait(self, ticket: int):
        """-> (headers, records, truncated) of the job."""
        f = _abi.Fasta()
        recs = C.c_void_p()
        _check(lib().cls_service_wait(self._h, ticket, C.byref(f), C.byref(recs)))
        try:
            n = f.n
            hoff = np.ctypeslib.as_array(f.header_off, shape=(n + 1,)).copy()
            hraw = C.string_at(f.headers, int(hoff[-1]))
            headers = [hraw[int(hoff[i]) : int(hoff[i + 1])] for i in range(n)]
            out = np.frombuffer(C.string_at(recs, n * 24), dtype=_abi.PLACEMENT_DTYPE).copy() if n else np.zeros(0, _abi.PLACEMENT_DTYPE)
            return headers, out, bool(f.truncated)
        finally:
            lib().cls_fasta_free(C.byref(f))
            lib().cls_host_free(recs)

    def pause(self, paused: bool = True) -> None:
        _check(lib().cls_service_pause(self._h, 1 if paused else 0))

    def stats(self) -> dict:
        st = _abi.ServiceStats()
        _check(lib().cls_service_stats_get(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _abi.ServiceStats._fields_}
