// Device side of the paired-read reconciliation (csrc/cls_pair.hip): what cls_api.cpp launches.  See DESIGN.md
// "Paired reads".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cls_tally.h"

namespace cls {

constexpr uint32_t PAIR_CLASSES = 8;  // how_count[8]; entry 7 is never counted

// The clade index of one pairer, by pre-order index `p` (the id table is the tally's: IdSlot, tally_hash).
struct PairDev {
    const IdSlot* table;
    uint32_t table_mask;
    uint32_t n_nodes;
    const uint32_t* size_by_pre;     // subtree size: x contains y  <=>  pre(x) <= pre(y) < pre(x) + size(x)
    const uint32_t* parent_by_pre;   // pre of the parent (the root's: itself)
    const uint32_t* depth_by_pre;    // edges below the root
    const uint64_t* id_by_pre;
    unsigned long long* totals;      // [PAIR_CLASSES] pairs per class (64-bit, device-scope atomics)
};

// `d_a` / `d_b`: mate 1 / mate 2 of pair i at record i * stride (8-byte aligned; stride 2: d_b = d_a + one record).
// `d_out`: n records; `d_how`: n bytes or NULL.
hipError_t launch_pair_records(const PairDev& p, const void* d_a, const void* d_b, uint32_t stride, uint32_t n, uint32_t flags,
                               void* d_out, void* d_how, uint32_t n_cu, hipStream_t stream);

// Mate-name check.  Header of mate m of pair i: bytes [off_m[i * stride], off_m[i * stride + 1]) of headers_m.
// d_result[0] += disagreeing pairs; d_result[1] = min(d_result[1], lowest disagreeing index).
hipError_t launch_pair_names(const char* d_headers1, const uint64_t* d_off1, const char* d_headers2, const uint64_t* d_off2,
                             uint32_t stride, uint32_t n, unsigned long long* d_result, hipStream_t stream);

// dst[new_off[i] ..) = src[off[i * stride] .. off[i * stride + 1]) for i < n: the headers of every stride-th record.
hipError_t launch_pair_gather_headers(const char* d_src, const uint64_t* d_off, uint32_t stride, uint32_t n, const uint64_t* d_new_off,
                                      char* d_dst, hipStream_t stream);

// The name of a header: its bytes up to the first space or tab, without a trailing "/1" or "/2".
__host__ __device__ inline uint64_t pair_name_len(const char* h, uint64_t len) {
    uint64_t m = 0;
    while (m < len && h[m] != ' ' && h[m] != '\t') ++m;
    if (m >= 2 && h[m - 2] == '/' && (h[m - 1] == '1' || h[m - 1] == '2')) m -= 2;
    return m;
}

}  // namespace cls
