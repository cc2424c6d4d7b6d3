// Device side of the clade tally (csrc/cls_tally.hip): what cls_api.cpp launches.  See DESIGN.md "Clade tally".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cls {

// id -> pre-order index: open addressing, linear probing, power-of-two capacity >= 2 n_nodes.  An id may be any
// 64-bit value, so the empty mark is in `pre`.
struct IdSlot {
    uint64_t id;
    uint32_t pre;   // TALLY_NO_PRE: empty
    uint32_t pad;
};
static_assert(sizeof(IdSlot) == 16, "IdSlot");
constexpr uint32_t TALLY_NO_PRE = 0xFFFFFFFFu;
constexpr uint32_t TALLY_MAX_NODES = 1u << 30;  // (pre, status) keys are pre * 4 + (status - 4) in 32 bits

__host__ __device__ inline uint64_t tally_hash(uint64_t x) {  // the 64-bit finaliser of MurmurHash3
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

// Totals, 16 counters: [0, 12) per status, then records with a status >= 12 and clade-bearing records of no clade.
constexpr uint32_t TALLY_BAD = 12, TALLY_UNKNOWN = 13, TALLY_TOTALS = 16;

// One accumulator, indexed by pre-order index `p` (64-bit counters, device-scope atomics):
//   cnt[3 p + (status - CLS_IDENTITY_FOUND)]   records placed exactly at the clade, by clade-bearing status
//   sums[2 p], sums[2 p + 1]                   sum of `one`, of `rest` over its CLS_IDENTITY_FOUND records
struct TallyDev {
    const IdSlot* table;
    uint32_t table_mask;
    uint32_t n_nodes;
    unsigned long long* cnt;
    long long* sums;
    unsigned long long* totals;
    // read-out
    const uint32_t* size_by_pre;   // subtree size of the clade with pre-order index p
    unsigned long long* prefix;    // [n_nodes + 1] n_direct by pre, then its exclusive prefix sum
    unsigned long long* clade;     // [n_nodes]     n_clade by pre
    void* scan_tmp;
    size_t scan_tmp_bytes;
};

size_t tally_scan_tmp_bytes(uint32_t n_nodes);
// `d_records`: n cls_placement records, 8-byte aligned.  `wave_combine` = 0: without the wave-level step (A/B knob).
hipError_t launch_tally_add(const TallyDev& t, const void* d_records, uint32_t n, uint32_t n_cu, int wave_combine, hipStream_t stream);
// n_direct by pre -> prefix sum -> n_clade(p) = prefix[p + size(p)] - prefix[p]
hipError_t launch_tally_finish(const TallyDev& t, hipStream_t stream);

}  // namespace cls
