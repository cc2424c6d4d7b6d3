// Index builder on the device: map_kmers_to_tree (core/src/use_cases/build_database/mod.rs:26-181) for records whose
// bases are filtered already, one LEAF clade each (cls_kmers_build, include/cls_place.h).  gfx950.
//
// The output is the k-mer map in canonical order (buckets ascending by key, k-mers by hash inside a bucket, ids
// ascending inside a k-mer), the order cls_build.cpp produces, so the host builder is a byte-for-byte oracle.
//
// Phases (one stream, HIP events between them: cls_kmers_info):
//   hash   One workgroup per 256 window positions of a record stages the record's bytes in LDS and writes, per window,
//          (k-mer hash, bucket key, leaf ordinal) for the forward k-mer and its reverse complement: SoA, 20 bytes a
//          window.  Leaf ordinal = rank of the leaf's clade id among the leaves in use, and the records are laid out in
//          ordinal order (a stable host sort of the records), so the window array starts out sorted by ordinal.
//   sort   LSD radix sort, 8-bit digits, of the windows by hash: 8 passes of histogram / exclusive scan / scatter.
//          The scatter is stable: a workgroup takes its 4096 windows in 16 rounds of 256 in index order; inside a round
//          a window's rank is the number of lower lanes of its wave with the same digit (peer mask from 8 ballots) plus
//          the counts of that digit in the lower waves; the per-workgroup offsets come from a scan of the digit-major
//          count table (digit, workgroup), i.e. in workgroup order.  Stable passes over a hash keep the ordinal order
//          inside equal hashes: the result is sorted by (hash, ordinal) with no pass over the ordinal.
//   group  Flags (new k-mer: hash or bucket key differ from the previous window; new posting: new k-mer or ordinal
//          differs), two device scans, compaction into distinct k-mers and distinct (k-mer, leaf) postings.  The
//          distinct k-mers (far fewer than the windows) are then put in bucket order by a stable radix sort on the
//          bucket key alone, which leaves them in hash order inside a bucket; the postings follow their k-mer by a
//          scan of the per-k-mer counts, and the ordinals become clade ids through a device table.
//
// The sort keys on the 64-bit hash only; the bucket is carried through it and checked.  Two different k-mers with
// equal hashes but different first m characters (a 64-bit collision: it cannot be built in a test, about n^2 / 2^65
// for n distinct k-mers) would sit interleaved in one run of equal hashes.  The group pass detects it (equal
// neighbouring hashes with different bucket keys) and then the windows are hashed again and sorted on the full key:
// 8 passes by bucket key, then 8 by hash, so the runs are (hash, bucket key) and the k-mers come out as the host
// builder keys them, (bucket, hash).  Equal hashes with equal bucket keys are one k-mer, in both builders, as in the
// reference (kmers_map.rs:125-149).  The knob build_full_key takes that path unconditionally (tests).
//
// Memory: every phase checks what it allocates against hipMemGetInfo first (CLS_E_NOMEM with a message); windows are
// indexed in 32 bits (at most 2^32 - 2^16 of them: 20 bytes a window, double-buffered, is beyond any device's HBM well
// before that).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "cls_build.h"
#include "cls_db.h"
#include "cls_devutil.h"
#include "cls_tuning.h"

extern "C" void cls_internal_set_error(const char* msg);  // cls_api.cpp: the thread-local text behind cls_last_error()

namespace cls {
namespace {

constexpr int BT = 256;                                   // threads of every builder kernel
constexpr int RADIX_BITS = 8, RADIX = 1 << RADIX_BITS;    // one bin per thread in the histogram / scatter kernels
constexpr int RADIX_ITEMS = 16, RADIX_TILE = BT * RADIX_ITEMS;
constexpr int SCAN_ITEMS = 16, SCAN_CHUNK = BT * SCAN_ITEMS;
constexpr uint32_t HASH_TILE = BT;                         // window positions a hash workgroup takes
constexpr uint32_t LDS_TEXT = HASH_TILE + (uint32_t)MAX_K + 16;  // (murmur3_h1_lds reads up to 15 bytes past a message)
constexpr uint64_t MAX_WINDOWS = 0xFFFF0000ull;
static_assert(RADIX == BT, "one radix bin per thread");

struct Slot {       // a record with at least k bases, in leaf-ordinal order
    uint64_t off;   // first base in the device copy of the bases
    uint64_t len;   // bases
    uint32_t win;   // its first window
    uint32_t ord;   // its leaf's ordinal
};

__device__ __forceinline__ uint8_t complement(uint8_t c) {  // as cls_build.cpp: every byte but A, C, G complements to 'A'
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
}

__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * BT + threadIdx.x; }

// ---- hash ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void build_hash_kernel(const char* __restrict__ bases, const Slot* __restrict__ slots,
                                                        const uint32_t* __restrict__ tile_start, uint32_t n_slots, uint32_t K,
                                                        uint32_t M, uint32_t both, uint64_t* __restrict__ hash,
                                                        uint64_t* __restrict__ bkey, uint32_t* __restrict__ ord) {
    __shared__ uint8_t text[LDS_TEXT];
    const uint32_t t = blockIdx.x;
    uint32_t lo = 0, hi = n_slots;  // the slot of tile t: the last s with tile_start[s] <= t (tile_start[0] = 0)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_start[mid] <= t) lo = mid; else hi = mid;
    }
    const Slot s = slots[lo];
    const uint64_t q0 = (uint64_t)(t - tile_start[lo]) * HASH_TILE, P = s.len - K + 1;
    const uint32_t n_text = (uint32_t)min(s.len - q0, (uint64_t)(HASH_TILE + K - 1));
    for (uint32_t i = threadIdx.x; i < n_text; i += BT) text[i] = (uint8_t)bases[s.off + q0 + i];
    __syncthreads();
    const uint64_t q = q0 + threadIdx.x;
    if (q >= P) return;
    const uint8_t* w = text + threadIdx.x;  // the forward k-mer at q; its reverse complement is the same bases backwards
    const uint32_t i = s.win + (uint32_t)q;
    hash[i] = murmur3_h1_lds(w, K);
    bkey[i] = M ? murmur3_h1_lds(w, M) : 0ull;  // MinimizerKey(0) when m = 0 (kmers_map.rs:131-134)
    ord[i] = s.ord;
    if (both) {
        auto rc = [w, K](uint32_t j) { return complement(w[K - 1 - j]); };
        const uint32_t r = i + (uint32_t)P;
        hash[r] = murmur3_h1(rc, K);
        bkey[r] = M ? murmur3_h1(rc, M) : 0ull;
        ord[r] = s.ord;
    }
}

// ---- block scan helper: inclusive scan of one value per thread; `total` = the workgroup's sum ----------------------
__device__ __forceinline__ uint32_t block_incl_scan(uint32_t v, uint32_t* wtot, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = __shfl_up(incl, o);
        if ((int)lane >= o) incl += x;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < BT / 64; ++w) {
        const uint32_t x = wtot[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();  // (wtot is reused by the next call)
    return before + incl;
}

// ---- exclusive scan of u32 in place: chunk sums, a one-workgroup scan of them, the chunks with their offsets -------
__global__ __launch_bounds__(BT) void scan_reduce_kernel(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[BT / 64];
    uint32_t s = 0;
    const size_t base = (size_t)blockIdx.x * SCAN_CHUNK;
#pragma unroll 4
    for (int r = 0; r < SCAN_ITEMS; ++r) {
        const size_t i = base + (size_t)r * BT + threadIdx.x;
        if (i < n) s += in[i];
    }
    uint32_t total;
    block_incl_scan(s, wtot, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(BT) void scan_sums_kernel(uint32_t* __restrict__ sums, uint32_t n, uint32_t* __restrict__ total_out) {
    __shared__ uint32_t wtot[BT / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += BT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n ? sums[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_incl_scan(v, wtot, total);
        if (i < n) sums[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(BT) void scan_down_kernel(uint32_t* __restrict__ data, size_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[BT / 64];
    uint32_t carry = sums[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SCAN_CHUNK;
    for (int r = 0; r < SCAN_ITEMS; ++r) {
        const size_t i = base + (size_t)r * BT + threadIdx.x;
        const uint32_t v = i < n ? data[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_incl_scan(v, wtot, total);
        if (i < n) data[i] = carry + incl - v;
        carry += total;
    }
}

// ---- radix sort pass ----------------------------------------------------------------------------------------------
// counts[digit * n_tiles + tile]: digit-major, so one exclusive scan gives every (digit, tile) its first output slot
// with the tiles of a digit in index order.
__global__ __launch_bounds__(BT) void radix_hist_kernel(const uint64_t* __restrict__ key, size_t n, int shift, uint32_t n_tiles,
                                                        uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RADIX_TILE;
#pragma unroll 4
    for (int r = 0; r < RADIX_ITEMS; ++r) {
        const size_t i = base + (size_t)r * BT + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(key[i] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

template <bool PAY64>
__global__ __launch_bounds__(BT) void radix_scatter_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ p64,
                                                           const uint32_t* __restrict__ p32, uint64_t* __restrict__ key_o,
                                                           uint64_t* __restrict__ p64_o, uint32_t* __restrict__ p32_o, size_t n,
                                                           int shift, uint32_t n_tiles, const uint32_t* __restrict__ start) {
    __shared__ uint32_t base[RADIX];
    __shared__ uint32_t wcnt[BT / 64][RADIX];  // (round + 1) << 8 | windows of the digit in the wave that round; other rounds' entries read as 0
    base[threadIdx.x] = start[(size_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < BT / 64; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lower = (1ull << lane) - 1;
    for (uint32_t r = 0; r < RADIX_ITEMS; ++r) {
        const size_t i = (size_t)blockIdx.x * RADIX_TILE + (size_t)r * BT + threadIdx.x;
        const bool valid = i < n;
        const uint64_t k = valid ? key[i] : 0ull;
        const uint32_t d = (uint32_t)(k >> shift) & (RADIX - 1);
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lower), cnt = (uint32_t)__popcll(peers);
        const bool leader = valid && rank == 0;
        if (leader) wcnt[wave][d] = ((r + 1) << 8) | cnt;
        __syncthreads();
        if (valid) {
            uint32_t at = base[d] + rank;
            for (uint32_t w = 0; w < wave; ++w) {
                const uint32_t v = wcnt[w][d];
                if ((v >> 8) == r + 1) at += v & 255u;
            }
            key_o[at] = k;
            if constexpr (PAY64) p64_o[at] = p64[i];
            p32_o[at] = p32[i];
        }
        __syncthreads();
        if (leader) atomicAdd(&base[d], cnt);
    }
}

// ---- group --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void group_flags_kernel(const uint64_t* __restrict__ H, const uint64_t* __restrict__ B,
                                                         const uint32_t* __restrict__ O, size_t n, uint32_t* __restrict__ kflag,
                                                         uint32_t* __restrict__ pflag, uint32_t* __restrict__ collide) {
    const size_t i = gid();
    if (i >= n) return;
    uint32_t head = 1, keep = 1;
    if (i > 0) {
        const bool same_h = H[i] == H[i - 1], same_b = B[i] == B[i - 1];
        head = !(same_h && same_b);
        keep = head || O[i] != O[i - 1];
        if (same_h && !same_b) *collide = 1u;
    }
    kflag[i] = head;
    pflag[i] = keep;
}

__global__ __launch_bounds__(BT) void group_compact_kernel(const uint64_t* __restrict__ H, const uint64_t* __restrict__ B,
                                                           const uint32_t* __restrict__ O, size_t n, const uint32_t* __restrict__ kscan,
                                                           const uint32_t* __restrict__ pscan, uint32_t D, uint32_t P,
                                                           uint64_t* __restrict__ kh, uint64_t* __restrict__ kb, uint32_t* __restrict__ kpost,
                                                           uint32_t* __restrict__ post_ord, uint32_t* __restrict__ post_kid) {
    const size_t i = gid();
    if (i >= n) return;
    bool head = true, keep = true;
    if (i > 0) {
        head = H[i] != H[i - 1] || B[i] != B[i - 1];
        keep = head || O[i] != O[i - 1];
    }
    const uint32_t kid = head ? kscan[i] : kscan[i] - 1;  // (exclusive scan of the heads)
    if (head) { kh[kid] = H[i]; kb[kid] = B[i]; kpost[kid] = pscan[i]; }
    if (keep) { post_ord[pscan[i]] = O[i]; post_kid[pscan[i]] = kid; }
    if (i == 0) kpost[D] = P;
}

__global__ __launch_bounds__(BT) void iota_kernel(uint32_t* __restrict__ a, size_t n) {
    const size_t i = gid();
    if (i < n) a[i] = (uint32_t)i;
}

// k-mers in bucket order: perm[j] = the hash-order index of the k-mer at canonical position j
__global__ __launch_bounds__(BT) void kmer_gather_kernel(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ kb_sorted,
                                                         uint32_t D, const uint64_t* __restrict__ kh, const uint32_t* __restrict__ kpost,
                                                         uint64_t* __restrict__ out_hash, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ inv, uint32_t* __restrict__ bflag) {
    const size_t j = gid();
    if (j >= D) return;
    const uint32_t kid = perm[j];
    out_hash[j] = kh[kid];
    cnt[j] = kpost[kid + 1] - kpost[kid];
    inv[kid] = (uint32_t)j;
    bflag[j] = j == 0 || kb_sorted[j] != kb_sorted[j - 1];
}

__global__ __launch_bounds__(BT) void kmer_out_kernel(uint32_t D, uint32_t P, uint32_t NB, const uint64_t* __restrict__ kb_sorted,
                                                      const uint32_t* __restrict__ noff, const uint32_t* __restrict__ bidx,
                                                      uint64_t* __restrict__ node_off, uint64_t* __restrict__ bucket_key,
                                                      uint64_t* __restrict__ bucket_off) {
    const size_t j = gid();
    if (j >= D) return;
    node_off[j] = noff[j];
    if (j == D - 1) { node_off[D] = P; bucket_off[NB] = D; }
    if (j == 0 || kb_sorted[j] != kb_sorted[j - 1]) { bucket_key[bidx[j]] = kb_sorted[j]; bucket_off[bidx[j]] = j; }
}

__global__ __launch_bounds__(BT) void posting_out_kernel(uint32_t P, const uint32_t* __restrict__ post_kid, const uint32_t* __restrict__ post_ord,
                                                         const uint32_t* __restrict__ kpost, const uint32_t* __restrict__ inv,
                                                         const uint32_t* __restrict__ noff, const uint64_t* __restrict__ ord_id,
                                                         uint64_t* __restrict__ node_ids) {
    const size_t p = gid();
    if (p >= P) return;
    const uint32_t kid = post_kid[p];
    node_ids[noff[inv[kid]] + ((uint32_t)p - kpost[kid])] = ord_id[post_ord[p]];
}

// ---- host side ----------------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg) {
    cls_internal_set_error(msg.c_str());
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_kmers_build: ") + what + ": " + hipGetErrorString(e));
}
#define B_HIP(expr)                                            \
    do {                                                       \
        const hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);      \
    } while (0)
#define B_LAUNCH(kernel, blocks, ...)                                                          \
    do {                                                                                       \
        if ((blocks) > 0) {                                                                    \
            hipLaunchKernelGGL(kernel, dim3((uint32_t)(blocks)), dim3(BT), 0, st, __VA_ARGS__); \
            B_HIP(hipGetLastError());                                                          \
        }                                                                                      \
    } while (0)

size_t blocks_of(size_t n, size_t per) { return (n + per - 1) / per; }

// One build: its device allocations (freed on every path, each hipFree checked), stream and events.
struct Build {
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {};
    std::vector<std::pair<void*, size_t>> live;
    size_t cur = 0, peak = 0;

    template <class T>
    int alloc(T** p, size_t count) {
        *p = nullptr;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        live.emplace_back((void*)*p, bytes);
        cur += bytes;
        peak = std::max(peak, cur);
        return CLS_OK;
    }
    int release(void* p) {
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i].first == p) {
                cur -= live[i].second;
                live.erase(live.begin() + (long)i);
                B_HIP(hipFree(p));
                return CLS_OK;
            }
        return CLS_OK;
    }
    // free space check before a phase allocates `bytes`
    int reserve(size_t bytes, const char* phase) {
        size_t fr = 0, total = 0;
        B_HIP(hipMemGetInfo(&fr, &total));
        const size_t slack = 64ull << 20;
        if (bytes + slack > fr)
            return fail(CLS_E_NOMEM, std::string("cls_kmers_build: the ") + phase + " phase needs " + std::to_string(bytes >> 20) +
                                         " MiB of device memory, " + std::to_string(fr >> 20) + " MiB are free");
        return CLS_OK;
    }
    int finish(int rc) {  // frees everything; the first error wins
        auto keep = [&](int r) { if (rc == CLS_OK) rc = r; };
        if (st) {
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) keep(hip_fail(e, "hipStreamSynchronize"));
        }
        for (auto& a : live) {
            const hipError_t e = hipFree(a.first);
            if (e != hipSuccess) keep(hip_fail(e, "hipFree"));
        }
        live.clear();
        cur = 0;
        for (hipEvent_t& e : ev)
            if (e) {
                const hipError_t x = hipEventDestroy(e);
                if (x != hipSuccess) keep(hip_fail(x, "hipEventDestroy"));
                e = nullptr;
            }
        if (st) {
            const hipError_t e = hipStreamDestroy(st);
            if (e != hipSuccess) keep(hip_fail(e, "hipStreamDestroy"));
            st = nullptr;
        }
        return rc;
    }
};

// exclusive scan of data[0 .. n) in place; the sum lands in *d_total (device)
int scan(Build& bd, uint32_t* data, size_t n, uint32_t* sums, uint32_t* d_total) {
    hipStream_t st = bd.st;
    if (n == 0) { B_HIP(hipMemsetAsync(d_total, 0, sizeof(uint32_t), st)); return CLS_OK; }
    const size_t nb = blocks_of(n, SCAN_CHUNK);
    B_LAUNCH(scan_reduce_kernel, nb, (const uint32_t*)data, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(BT), 0, st, sums, (uint32_t)nb, d_total);
    B_HIP(hipGetLastError());
    B_LAUNCH(scan_down_kernel, nb, data, n, (const uint32_t*)sums);
    return CLS_OK;
}
size_t scan_sums_len(size_t n) { return std::max<size_t>(1, blocks_of(n, SCAN_CHUNK)); }

// Stable LSD radix sort of n keys by bits [lo_bit, 64) in 8-bit digits, carrying p64 (may be null) and p32; `passes`
// digits.  Buffers ping-pong between (key, p64, p32) and the *2 ones; an even number of passes ends in the first set.
int radix_sort(Build& bd, size_t n, int passes, uint64_t* key, uint64_t* key2, uint64_t* p64, uint64_t* p64_2, uint32_t* p32,
               uint32_t* p32_2, uint32_t* counts, uint32_t* sums, uint32_t* d_total) {
    hipStream_t st = bd.st;
    const size_t tiles = blocks_of(n, RADIX_TILE);
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = pass * RADIX_BITS;
        B_LAUNCH(radix_hist_kernel, tiles, (const uint64_t*)key, n, shift, (uint32_t)tiles, counts);
        int rc = scan(bd, counts, tiles * RADIX, sums, d_total);
        if (rc != CLS_OK) return rc;
        if (p64) B_LAUNCH(radix_scatter_kernel<true>, tiles, (const uint64_t*)key, (const uint64_t*)p64, (const uint32_t*)p32, key2, p64_2, p32_2, n, shift, (uint32_t)tiles, (const uint32_t*)counts);
        else B_LAUNCH(radix_scatter_kernel<false>, tiles, (const uint64_t*)key, (const uint64_t*)nullptr, (const uint32_t*)p32, key2, (uint64_t*)nullptr, p32_2, n, shift, (uint32_t)tiles, (const uint32_t*)counts);
        std::swap(key, key2);
        std::swap(p64, p64_2);
        std::swap(p32, p32_2);
    }
    return CLS_OK;
}

int d2h_u32(Build& bd, const uint32_t* d, uint32_t* h) {
    B_HIP(hipMemcpyAsync(h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, bd.st));
    B_HIP(hipStreamSynchronize(bd.st));
    return CLS_OK;
}

struct Plan {  // what the host derives from the descriptor before any device work
    std::vector<uint32_t> parent_row;   // per row; UINT32_MAX at the root
    std::vector<uint64_t> ord_id;       // leaf ordinal -> clade id, ascending
    std::vector<uint32_t> rec_ord;      // per record
    std::vector<Slot> slots;
    std::vector<uint32_t> tile_start;   // [n_slots + 1]
    uint64_t n_windows = 0;
    uint64_t base_lo = 0, base_hi = 0;  // the byte range of `bases` the records use
};

int plan_build(const cls_build_desc* b, Plan& pl) {
    const uint32_t N = b->n_nodes;
    // the tree: rows reached from row 0 through the children ranges, each once
    pl.parent_row.assign(N, UINT32_MAX);
    std::vector<uint8_t> seen(N, 0);
    std::vector<uint32_t> q{0};
    seen[0] = 1;
    for (size_t h = 0; h < q.size(); ++h) {
        const cls_node& nd = b->nodes[q[h]];
        if (nd.n_children && ((uint64_t)nd.first_child + nd.n_children > N || nd.first_child == 0))
            return fail(CLS_E_BAD_TREE, "cls_kmers_build: children of row " + std::to_string(q[h]) + " out of range");
        for (uint32_t c = nd.first_child; c < nd.first_child + nd.n_children; ++c) {
            if (seen[c]) return fail(CLS_E_BAD_TREE, "cls_kmers_build: row " + std::to_string(c) + " has two parents");
            seen[c] = 1;
            pl.parent_row[c] = q[h];
            q.push_back(c);
        }
    }
    std::unordered_map<uint64_t, uint32_t> row_of;
    row_of.reserve(N);
    for (uint32_t r : q) row_of.emplace(b->nodes[r].id, r);  // first row in BFS order
    const uint64_t K = b->k_size;
    std::vector<uint64_t> used;
    for (uint32_t i = 0; i < b->n_records; ++i) {
        auto it = row_of.find(b->leaf_id[i]);
        if (it == row_of.end() || b->nodes[it->second].kind != CLS_KIND_LEAF || b->nodes[it->second].n_children)
            return fail(CLS_E_BAD_DB, "cls_kmers_build: leaf_id " + std::to_string(b->leaf_id[i]) + " of record " + std::to_string(i) +
                                          " is not a childless LEAF clade of the tree");
        if (b->offsets[i + 1] - b->offsets[i] >= K) used.push_back(b->leaf_id[i]);
    }
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    pl.ord_id = used;
    pl.rec_ord.assign(b->n_records, UINT32_MAX);
    std::vector<uint32_t> recs;
    for (uint32_t i = 0; i < b->n_records; ++i)
        if (b->offsets[i + 1] - b->offsets[i] >= K) {
            pl.rec_ord[i] = (uint32_t)(std::lower_bound(used.begin(), used.end(), b->leaf_id[i]) - used.begin());
            recs.push_back(i);
        }
    std::stable_sort(recs.begin(), recs.end(), [&](uint32_t x, uint32_t y) { return pl.rec_ord[x] < pl.rec_ord[y]; });
    const uint64_t strands = (b->flags & CLS_BUILD_FORWARD_ONLY) ? 1 : 2;
    pl.base_lo = b->n_records ? b->offsets[0] : 0;
    pl.base_hi = b->n_records ? b->offsets[b->n_records] : 0;
    uint64_t win = 0, tiles = 0;
    pl.tile_start.assign(1, 0);
    for (uint32_t i : recs) {
        const uint64_t L = b->offsets[i + 1] - b->offsets[i], P = L - K + 1;
        if (win + P * strands > MAX_WINDOWS)
            return fail(CLS_E_NOMEM, "cls_kmers_build: more than " + std::to_string(MAX_WINDOWS) + " windows");
        pl.slots.push_back({b->offsets[i] - pl.base_lo, L, (uint32_t)win, pl.rec_ord[i]});
        win += P * strands;
        tiles += (P + HASH_TILE - 1) / HASH_TILE;
        pl.tile_start.push_back((uint32_t)tiles);
    }
    pl.n_windows = win;
    return CLS_OK;
}

int ms_between(hipEvent_t a, hipEvent_t b, double* out) {
    float ms = 0.0f;
    B_HIP(hipEventElapsedTime(&ms, a, b));
    *out = ms;
    return CLS_OK;
}

// The device phases: km's five arrays in leaves-only form (node_ids = leaf clade ids).
int run_device(Build& bd, const cls_build_desc* b, bool bases_on_device, const Plan& pl, cls_kmers* km) {
    hipStream_t& st = bd.st;
    cls_kmers_info& info = km->info;
    const size_t NW = pl.n_windows, NS = pl.slots.size();
    const uint32_t K = (uint32_t)b->k_size, M = (uint32_t)std::min<uint64_t>(b->m_size, b->k_size);
    B_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (hipEvent_t& e : bd.ev) B_HIP(hipEventCreate(&e));
    const bool full_key_forced = tuning().build_full_key != 0;
    const size_t tiles = blocks_of(NW, RADIX_TILE), n_counts = tiles * RADIX;
    const size_t n_text = bases_on_device ? 0 : pl.base_hi - pl.base_lo;
    int rc = bd.reserve(n_text + NS * sizeof(Slot) + (NS + 1) * 4 + NW * 40 + n_counts * 4 + scan_sums_len(std::max(n_counts, NW)) * 4 + 64, "hash and sort");
    if (rc) return rc;
    char* d_text = nullptr;
    Slot* d_slots = nullptr;
    uint32_t *d_tile = nullptr, *d_counts = nullptr, *d_sums = nullptr, *d_misc = nullptr;  // misc: [0] total, [1] collision
    uint64_t *H = nullptr, *B = nullptr, *H2 = nullptr, *B2 = nullptr;
    uint32_t *O = nullptr, *O2 = nullptr;
    if ((rc = bd.alloc(&d_slots, NS)) || (rc = bd.alloc(&d_tile, NS + 1)) || (rc = bd.alloc(&H, NW)) || (rc = bd.alloc(&B, NW)) ||
        (rc = bd.alloc(&O, NW)) || (rc = bd.alloc(&H2, NW)) || (rc = bd.alloc(&B2, NW)) || (rc = bd.alloc(&O2, NW)) ||
        (rc = bd.alloc(&d_counts, n_counts)) || (rc = bd.alloc(&d_sums, scan_sums_len(std::max(n_counts, NW)))) || (rc = bd.alloc(&d_misc, 4)))
        return rc;
    B_HIP(hipEventRecord(bd.ev[0], st));
    const char* bases = b->bases;
    if (!bases_on_device) {
        if ((rc = bd.alloc(&d_text, n_text))) return rc;
        if (n_text) B_HIP(hipMemcpyAsync(d_text, b->bases + pl.base_lo, n_text, hipMemcpyHostToDevice, st));
        bases = d_text;
    } else {
        bases = b->bases + pl.base_lo;
    }
    B_HIP(hipMemcpyAsync(d_slots, pl.slots.data(), NS * sizeof(Slot), hipMemcpyHostToDevice, st));
    B_HIP(hipMemcpyAsync(d_tile, pl.tile_start.data(), (NS + 1) * 4, hipMemcpyHostToDevice, st));
    B_HIP(hipMemsetAsync(d_misc, 0, 4 * sizeof(uint32_t), st));
    const uint32_t both = (b->flags & CLS_BUILD_FORWARD_ONLY) ? 0u : 1u;
    const uint32_t n_hash_tiles = pl.tile_start.back();
    B_LAUNCH(build_hash_kernel, n_hash_tiles, bases, (const Slot*)d_slots, (const uint32_t*)d_tile, (uint32_t)NS, K, M, both, H, B, O);
    B_HIP(hipEventRecord(bd.ev[1], st));
    // sort: by hash; by (hash, bucket key) when two k-mers share a hash
    uint32_t* kflag = reinterpret_cast<uint32_t*>(H2);  // (the second buffers are free once a sort has ended in the first)
    uint32_t* pflag = kflag + NW;
    bool full = full_key_forced;
    for (int attempt = 0;; ++attempt) {
        if (attempt == 1) B_LAUNCH(build_hash_kernel, n_hash_tiles, bases, (const Slot*)d_slots, (const uint32_t*)d_tile, (uint32_t)NS, K, M, both, H, B, O);
        if (full) {
            if ((rc = radix_sort(bd, NW, 8, B, B2, H, H2, O, O2, d_counts, d_sums, d_misc))) return rc;
            info.sort_passes += 8;
        }
        if ((rc = radix_sort(bd, NW, 8, H, H2, B, B2, O, O2, d_counts, d_sums, d_misc))) return rc;
        info.sort_passes += 8;
        B_LAUNCH(group_flags_kernel, blocks_of(NW, BT), (const uint64_t*)H, (const uint64_t*)B, (const uint32_t*)O, NW, kflag, pflag, d_misc + 1);
        if (full) break;
        uint32_t collide = 0;
        if ((rc = d2h_u32(bd, d_misc + 1, &collide))) return rc;
        if (!collide) break;
        full = true;
    }
    info.full_key = full ? 1 : 0;
    B_HIP(hipEventRecord(bd.ev[2], st));
    // group: distinct k-mers and (k-mer, leaf) postings in hash order
    uint32_t D = 0, P = 0;
    if ((rc = scan(bd, kflag, NW, d_sums, d_misc)) || (rc = d2h_u32(bd, d_misc, &D))) return rc;
    if ((rc = scan(bd, pflag, NW, d_sums, d_misc)) || (rc = d2h_u32(bd, d_misc, &P))) return rc;
    const size_t n_ord = pl.ord_id.size();
    if ((rc = bd.reserve((size_t)D * 20 + 4 + (size_t)P * 8, "group"))) return rc;
    uint64_t *kh = nullptr, *kb = nullptr;
    uint32_t *kpost = nullptr, *post_ord = nullptr, *post_kid = nullptr;
    if ((rc = bd.alloc(&kh, D)) || (rc = bd.alloc(&kb, D)) || (rc = bd.alloc(&kpost, (size_t)D + 1)) || (rc = bd.alloc(&post_ord, P)) ||
        (rc = bd.alloc(&post_kid, P)))
        return rc;
    B_LAUNCH(group_compact_kernel, blocks_of(NW, BT), (const uint64_t*)H, (const uint64_t*)B, (const uint32_t*)O, NW, (const uint32_t*)kflag,
             (const uint32_t*)pflag, D, P, kh, kb, kpost, post_ord, post_kid);
    for (void* p : {(void*)H, (void*)B, (void*)O, (void*)H2, (void*)B2, (void*)O2, (void*)d_counts})
        if ((rc = bd.release(p))) return rc;
    // bucket order of the distinct k-mers: stable radix sort by bucket key (m = 0: one bucket, already in order)
    const size_t k_tiles = blocks_of(D, RADIX_TILE);
    if ((rc = bd.reserve((size_t)D * 60 + 32 + (size_t)P * 8 + n_ord * 8 + k_tiles * RADIX * 4, "bucket order"))) return rc;
    uint64_t *kb2 = nullptr, *out_hash = nullptr, *out_node_off = nullptr, *out_bkey = nullptr, *out_boff = nullptr, *out_ids = nullptr, *d_ord_id = nullptr;
    uint32_t *perm = nullptr, *perm2 = nullptr, *inv = nullptr, *cnt = nullptr, *bflag = nullptr, *k_counts = nullptr;
    if ((rc = bd.alloc(&kb2, D)) || (rc = bd.alloc(&perm, D)) || (rc = bd.alloc(&perm2, D)) || (rc = bd.alloc(&inv, D)) || (rc = bd.alloc(&cnt, D)) ||
        (rc = bd.alloc(&bflag, D)) || (rc = bd.alloc(&out_hash, D)) || (rc = bd.alloc(&out_node_off, (size_t)D + 1)) || (rc = bd.alloc(&out_bkey, D)) ||
        (rc = bd.alloc(&out_boff, (size_t)D + 1)) || (rc = bd.alloc(&out_ids, P)) || (rc = bd.alloc(&d_ord_id, n_ord)) ||
        (rc = bd.alloc(&k_counts, k_tiles * RADIX)))
        return rc;
    B_HIP(hipMemcpyAsync(d_ord_id, pl.ord_id.data(), n_ord * 8, hipMemcpyHostToDevice, st));
    B_LAUNCH(iota_kernel, blocks_of(D, BT), perm, (size_t)D);
    if (M) {
        if ((rc = radix_sort(bd, D, 8, kb, kb2, nullptr, nullptr, perm, perm2, k_counts, d_sums, d_misc))) return rc;
    }
    uint32_t NB = 0;
    B_LAUNCH(kmer_gather_kernel, blocks_of(D, BT), (const uint32_t*)perm, (const uint64_t*)kb, D, (const uint64_t*)kh, (const uint32_t*)kpost,
             out_hash, cnt, inv, bflag);
    if ((rc = scan(bd, cnt, D, d_sums, d_misc))) return rc;
    if ((rc = scan(bd, bflag, D, d_sums, d_misc + 2)) || (rc = d2h_u32(bd, d_misc + 2, &NB))) return rc;
    B_LAUNCH(kmer_out_kernel, blocks_of(D, BT), D, P, NB, (const uint64_t*)kb, (const uint32_t*)cnt, (const uint32_t*)bflag, out_node_off,
             out_bkey, out_boff);
    B_LAUNCH(posting_out_kernel, blocks_of(P, BT), P, (const uint32_t*)post_kid, (const uint32_t*)post_ord, (const uint32_t*)kpost,
             (const uint32_t*)inv, (const uint32_t*)cnt, (const uint64_t*)d_ord_id, out_ids);
    B_HIP(hipEventRecord(bd.ev[3], st));
    km->bucket_key.resize(NB);
    km->bucket_kmer_off.resize((size_t)NB + 1);
    km->kmer_hash.resize(D);
    km->kmer_node_off.resize((size_t)D + 1);
    km->node_ids.resize(P);
    B_HIP(hipMemcpyAsync(km->bucket_key.data(), out_bkey, (size_t)NB * 8, hipMemcpyDeviceToHost, st));
    B_HIP(hipMemcpyAsync(km->bucket_kmer_off.data(), out_boff, ((size_t)NB + 1) * 8, hipMemcpyDeviceToHost, st));
    B_HIP(hipMemcpyAsync(km->kmer_hash.data(), out_hash, (size_t)D * 8, hipMemcpyDeviceToHost, st));
    B_HIP(hipMemcpyAsync(km->kmer_node_off.data(), out_node_off, ((size_t)D + 1) * 8, hipMemcpyDeviceToHost, st));
    B_HIP(hipMemcpyAsync(km->node_ids.data(), out_ids, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    B_HIP(hipEventRecord(bd.ev[4], st));
    B_HIP(hipStreamSynchronize(st));
    if ((rc = ms_between(bd.ev[0], bd.ev[1], &info.ms_hash)) || (rc = ms_between(bd.ev[1], bd.ev[2], &info.ms_sort)) ||
        (rc = ms_between(bd.ev[2], bd.ev[3], &info.ms_group)) || (rc = ms_between(bd.ev[3], bd.ev[4], &info.ms_d2h)))
        return rc;
    info.n_kmers = D;
    info.n_leaf_postings = P;
    info.n_buckets = NB;
    return CLS_OK;
}

}  // namespace

int kmers_build(const cls_build_desc* b, int device, bool bases_on_device, cls_kmers** out) {
    if (!b || !out) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: null argument");
    *out = nullptr;
    if (b->abi_version != CLS_ABI_VERSION) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: abi_version must be " + std::to_string(CLS_ABI_VERSION));
    if (b->k_size == 0 || b->k_size > MAX_K) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: k_size must be in [1, " + std::to_string(MAX_K) + "]");
    if (b->flags & ~(CLS_BUILD_FORWARD_ONLY | CLS_BUILD_LEAVES_ONLY)) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: unknown flags");
    if (!b->n_nodes || !b->nodes) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: empty tree");
    if (b->n_records && (!b->offsets || !b->leaf_id)) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: null records");
    for (uint32_t i = 0; i < b->n_records; ++i)
        if (b->offsets[i + 1] < b->offsets[i]) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: offsets decrease at record " + std::to_string(i));
    if (b->n_records && b->offsets[b->n_records] > b->offsets[0] && !b->bases) return fail(CLS_E_INVALID_ARG, "cls_kmers_build: null bases");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(CLS_E_NO_DEVICE, "cls_kmers_build: no HIP device");
    if (device < -1 || device >= n_dev)
        return fail(CLS_E_INVALID_ARG, "cls_kmers_build: device " + std::to_string(device) + " out of range (" + std::to_string(n_dev) + " devices)");
    int prev = 0;
    B_HIP(hipGetDevice(&prev));
    if (device < 0) device = prev;
    try {
        Plan pl;
        int rc = plan_build(b, pl);
        if (rc != CLS_OK) return rc;
        cls_kmers* km = new cls_kmers();
        km->k_size = b->k_size;
        km->m_size = b->m_size;
        km->node_set_kind = (b->flags & CLS_BUILD_LEAVES_ONLY) ? CLS_SETS_LEAVES : CLS_SETS_EXPLICIT;
        km->info.n_windows = pl.n_windows;
        if (pl.n_windows == 0) {
            km->bucket_kmer_off.assign(1, 0);
            km->kmer_node_off.assign(1, 0);
        } else {
            if (device != prev) {
                const hipError_t e = hipSetDevice(device);
                if (e != hipSuccess) { delete km; return hip_fail(e, "hipSetDevice"); }
            }
            Build bd;
            rc = run_device(bd, b, bases_on_device, pl, km);
            rc = bd.finish(rc);
            km->info.peak_device_bytes = bd.peak;
            if (device != prev) {
                const hipError_t e = hipSetDevice(prev);
                if (e != hipSuccess && rc == CLS_OK) rc = hip_fail(e, "hipSetDevice");
            }
            if (rc != CLS_OK) { delete km; return rc; }
        }
        if (km->node_set_kind == CLS_SETS_EXPLICIT) {
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<std::vector<uint64_t>> paths(pl.ord_id.size());
            std::unordered_map<uint64_t, uint32_t> row_of;
            for (uint32_t r = b->n_nodes; r-- > 0;) row_of[b->nodes[r].id] = r;  // (the first row of an id wins, as in plan_build)
            for (size_t o = 0; o < paths.size(); ++o) {
                for (uint32_t r = row_of.at(pl.ord_id[o]); r != UINT32_MAX; r = pl.parent_row[r]) paths[o].push_back(b->nodes[r].id);
                std::reverse(paths[o].begin(), paths[o].end());
            }
            std::vector<uint32_t> ref(km->node_ids.size());
            for (size_t p = 0; p < ref.size(); ++p)
                ref[p] = (uint32_t)(std::lower_bound(pl.ord_id.begin(), pl.ord_id.end(), km->node_ids[p]) - pl.ord_id.begin());
            const std::vector<uint64_t> leaf_off = std::move(km->kmer_node_off);
            expand_leaf_paths(km->kmer_hash.size(), leaf_off.data(), ref.data(), paths, km->kmer_node_off, km->node_ids);
            km->info.ms_expand = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        km->info.n_node_ids = km->node_ids.size();
        *out = km;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_kmers_build: out of host memory");
    } catch (const std::exception& e) {
        return fail(CLS_E_INTERNAL, std::string("cls_kmers_build: ") + e.what());
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_kmers_build: unknown exception");
    }
}

}  // namespace cls

extern "C" int cls_kmers_build(const cls_build_desc* b, int device, cls_kmers** out) { return cls::kmers_build(b, device, false, out); }

extern "C" int cls_kmers_desc(const cls_kmers* km, const cls_build_desc* b, cls_db_desc* d) {
    if (!km || !b || !d) return cls::fail(CLS_E_INVALID_ARG, "cls_kmers_desc: null argument");
    memset(d, 0, sizeof *d);
    d->abi_version = CLS_ABI_VERSION;
    d->n_nodes = b->n_nodes;
    d->nodes = b->nodes;
    d->k_size = km->k_size;
    d->m_size = km->m_size;
    d->n_buckets = km->bucket_key.size();
    d->bucket_key = km->bucket_key.data();
    d->bucket_kmer_off = km->bucket_kmer_off.data();
    d->n_kmers = km->kmer_hash.size();
    d->kmer_hash = km->kmer_hash.data();
    d->kmer_node_off = km->kmer_node_off.data();
    d->node_ids = km->node_ids.data();
    d->node_set_kind = km->node_set_kind;
    return CLS_OK;
}

extern "C" int cls_kmers_info_get(const cls_kmers* km, cls_kmers_info* info) {
    if (!km || !info) return cls::fail(CLS_E_INVALID_ARG, "cls_kmers_info_get: null argument");
    *info = km->info;
    return CLS_OK;
}

extern "C" void cls_kmers_free(cls_kmers* km) { delete km; }
