// Device side of the read extraction (csrc/cls_extract.hip): what cls_api.cpp launches.  See DESIGN.md "Read extraction".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cls_place.h"
#include "cls_tally.h"

namespace cls {

// One selector: the id table is of the tally's kind (IdSlot, tally_hash); sel_by_pre[p] = 1 iff the nearest listed clade
// on the path from the clade with pre-order index p to the root is an include.
struct SelectDev {
    const IdSlot* table;
    uint32_t table_mask;
    uint32_t n_nodes;
    const uint8_t* sel_by_pre;
    uint32_t unplaced;               // 1: CLS_SELECT_UNPLACED
};

// `d_records`: n cls_placement records, 8-byte aligned.  d_sel[i] = 1 / 0.  `d_n_unplaced` (may be NULL) += the selected
// records that are not placed.
hipError_t launch_select_records(const SelectDev& s, const void* d_records, uint32_t n, uint8_t* d_sel, unsigned long long* d_n_unplaced,
                                 hipStream_t stream);

// rec_off[r], r <= n, from the line starts of the FASTQ stage (ls[k], k <= n_nl + 1: fq_line_starts): the start of line
// 4 r, `len` when the text ends before it.  `d_ls` NULL (the empty text): every entry is `len`.
hipError_t launch_fastq_spans(const uint64_t* d_ls, uint64_t n_nl, uint64_t len, uint32_t n, uint64_t* d_rec_off, hipStream_t stream);

// The plan: d_out_off[i] = emitted length of item i (0 when it is not selected), d_out_off[n_items] = 0, *d_n_selected +=
// selected items; then the exclusive sum in place.
size_t extract_scan_tmp_bytes(uint32_t n_items);
hipError_t launch_extract_plan(const uint8_t* d_text, const uint64_t* d_rec_off, uint32_t stride, uint32_t n_items, const uint8_t* d_sel,
                               uint64_t* d_out_off, unsigned long long* d_n_selected, void* d_tmp, size_t tmp_bytes, hipStream_t stream);
// The gather: bytes [d_out_off[i], d_out_off[i + 1]) of `d_out` = item i's bytes (+ '\n' when one more byte is planned).
hipError_t launch_extract_gather(const uint8_t* d_text, const uint64_t* d_rec_off, uint32_t stride, uint32_t n_items, const uint8_t* d_sel,
                                 const uint64_t* d_out_off, uint8_t* d_out, hipStream_t stream);

// cls_fasta_gpu.hip: the line starts of a text in HBM (ls[0] = 0, ls[k + 1] = the position after newline k,
// ls[n_nl + 1] = len + 1) as a hipMalloc'ed array the caller frees; NULL for the empty text.  Synchronises `stream`.
int fastq_line_starts_device(const void* d_text, uint64_t len, uint64_t** d_ls, uint64_t* n_nl, hipStream_t stream);
// cls_fastq_scan_device that hands its line starts over instead of freeing them (same array, same ownership).
int fastq_scan_device_keep(const void* d_text, uint64_t len, const cls_fastq_opts* opts, cls_fasta_dev* out, hipStream_t stream,
                           uint64_t** d_ls, uint64_t* n_nl);

}  // namespace cls
