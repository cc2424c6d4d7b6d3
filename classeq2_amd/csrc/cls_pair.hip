// Paired reads: the two mates' placement records -> one record per pair, on the device (include/cls_place.h "paired
// reads").
//
// pair_records_kernel moves records as whole lines, the way tally_add_kernel does: a wave takes 128 pairs at a time,
// loads their 24-byte records with 16-byte loads into an LDS stage (stride 1: 3 KiB of mate 1 and 3 KiB of mate 2;
// stride 2: 6 KiB of interleaved records, a pair is 48 contiguous bytes), every lane reconciles two pairs from the stage,
// and the 128 result records go back out through a second stage with 16-byte stores.  A buffer may start 8 bytes into a
// 16-byte slot: the words before the first and behind the last record of a span are moved one by one, never touched
// outside it.  Ids are looked up in the pairer's copy of the tally's table (IdSlot, tally_hash); ancestry is a test on
// pre-order intervals, the LCA of a discordant pair a climb over parent_by_pre bounded by the clade's depth.  The seven
// classes are counted with ballots into registers, reduced per workgroup, and leave as one device-scope 64-bit atomic
// per class and workgroup.
// pair_names_kernel compares the mates' names, one pair per lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cls_pair.h"
#include "cls_place.h"

namespace cls {
namespace {

constexpr int TB = 256;               // threads per workgroup
constexpr int WAVES = TB / 64;
constexpr int CHUNK_PAIRS = 128;      // pairs a wave stages at a time
constexpr int SEG_WORDS = 3 * CHUNK_PAIRS;   // 8-byte words of 128 records: 3 x (64 lanes x 16 bytes)
constexpr int SEG_STAGE = SEG_WORDS + 2;     // one more word when the records start in the upper half of a 16-byte slot
constexpr int IN_STAGE = 2 * SEG_STAGE;      // stride 1: mate 1's segment, then mate 2's; stride 2: 256 records in one span
static_assert((SEG_STAGE * 8) % 16 == 0, "the second segment of the stage is 16-byte aligned");

__device__ inline void global_add(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Words [a0, a0 + 128 ROUNDS] of `q` -> st[0 ..], as far as they belong to the records: word a of `q` (the 16-byte
// aligned address at or below the first record) does iff w0 <= a < end_word.  a0 is even.
template <int ROUNDS>
__device__ inline void stage_in(unsigned long long* st, const unsigned long long* __restrict__ q, uint32_t w0, uint64_t end_word, uint64_t a0,
                                int lane) {
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const int s = lane + 64 * j;
        const uint64_t lo = a0 + 2ull * (uint64_t)s;
        const bool lo_ok = lo >= w0 && lo < end_word, hi_ok = lo + 1 < end_word;
        if (lo_ok && hi_ok) {
            const uint4 v = *reinterpret_cast<const uint4*>(q + lo);
            *reinterpret_cast<uint4*>(&st[2 * s]) = v;
        } else {
            if (lo_ok) st[2 * s] = q[lo];
            if (hi_ok) st[2 * s + 1] = q[lo + 1];
        }
    }
    if (w0 && lane == 0 && a0 + 128 * ROUNDS < end_word) st[128 * ROUNDS] = q[a0 + 128 * ROUNDS];
}

struct Rec {
    uint32_t status;
    int one, rest;
    uint32_t levels;
    unsigned long long clade;
};

__device__ inline Rec unpack(const unsigned long long* w) {
    Rec r;
    const unsigned long long x0 = w[0], x1 = w[1];
    r.status = (uint32_t)(x0 & 0xFFu);
    r.one = (int)(uint32_t)(x0 >> 32);
    r.rest = (int)(uint32_t)x1;
    r.levels = (uint32_t)(x1 >> 32);
    r.clade = w[2];
    return r;
}

// pre-order index of a clade-bearing record's clade, TALLY_NO_PRE when the mate is not usable
__device__ inline uint32_t usable_pre(const PairDev& p, const Rec& r) {
    if (r.status < CLS_IDENTITY_FOUND || r.status > CLS_INCONCLUSIVE) return TALLY_NO_PRE;
    uint32_t h = (uint32_t)tally_hash(r.clade) & p.table_mask;
    for (uint32_t probe = 0; probe <= p.table_mask; ++probe) {
        const uint4 e = *reinterpret_cast<const uint4*>(&p.table[h]);
        if (e.z == TALLY_NO_PRE) break;
        if ((((unsigned long long)e.y << 32) | e.x) == r.clade) return e.z;
        h = (h + 1) & p.table_mask;
    }
    return TALLY_NO_PRE;
}

// `qa` / `qb` / `qo`: the 16-byte-aligned addresses at or below the first record of mate 1 / mate 2 / the output, as
// 8-byte words; `wa` / `wb` / `wo`: the word the first record starts at (0 or 1).  STRIDE 2: `qb` is not used, the pair
// i is records 2 i and 2 i + 1 of `qa`.
template <int STRIDE>
__global__ __launch_bounds__(TB) void pair_records_kernel(PairDev p, const unsigned long long* __restrict__ qa, uint32_t wa,
                                                          const unsigned long long* __restrict__ qb, uint32_t wb, uint32_t n, uint32_t flags,
                                                          unsigned long long* __restrict__ qo, uint32_t wo, uint8_t* __restrict__ how) {
    __shared__ __attribute__((aligned(16))) unsigned long long stage[WAVES][IN_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned long long ostage[WAVES][SEG_STAGE];
    __shared__ uint32_t s_tot[PAIR_CLASSES];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < (int)PAIR_CLASSES) s_tot[tid] = 0;
    __syncthreads();

    const uint64_t n_chunks = ((uint64_t)n + CHUNK_PAIRS - 1) / CHUNK_PAIRS;
    const uint64_t end_a = (uint64_t)wa + 3ull * STRIDE * n, end_b = (uint64_t)wb + 3ull * n;
    const bool conservative = (flags & CLS_PAIR_CONSERVATIVE) != 0, require_both = (flags & CLS_PAIR_REQUIRE_BOTH) != 0;
    uint32_t acc = 0;  // lane s < 7: pairs of class s
    unsigned long long* st_w = stage[wave];
    unsigned long long* os_w = ostage[wave];

    // every wave of the workgroup makes the same number of rounds (the barriers below)
    for (uint64_t base = (uint64_t)blockIdx.x * WAVES; base < n_chunks; base += (uint64_t)gridDim.x * WAVES) {
        const uint64_t c = base + (uint64_t)wave;
        const bool active = c < n_chunks;
        if (active) {
            if (STRIDE == 2) stage_in<6>(st_w, qa, wa, end_a, c * (2 * SEG_WORDS), lane);
            else {
                stage_in<3>(st_w, qa, wa, end_a, c * SEG_WORDS, lane);
                stage_in<3>(st_w + SEG_STAGE, qb, wb, end_b, c * SEG_WORDS, lane);
            }
        }
        __syncthreads();
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int rl = lane + 64 * h2;
            const uint64_t r = c * CHUNK_PAIRS + (uint64_t)rl;
            const bool valid = active && r < n;
            uint32_t klass = 15u;
            if (valid) {
                const Rec a = unpack(STRIDE == 2 ? &st_w[6 * rl + wa] : &st_w[3 * rl + wa]);
                const Rec b = unpack(STRIDE == 2 ? &st_w[6 * rl + 3 + wa] : &st_w[SEG_STAGE + 3 * rl + wb]);
                const uint32_t pa = usable_pre(p, a), pb = usable_pre(p, b);
                const bool ua = pa != TALLY_NO_PRE, ub = pb != TALLY_NO_PRE;
                int sel = 0;  // 0: copy mate 1; 1: copy mate 2; 2: the LCA
                uint32_t lca = 0;
                if (!ua && !ub) klass = CLS_PAIR_NEITHER;
                else if (ua && !ub) { klass = CLS_PAIR_ONLY_1; sel = require_both ? 1 : 0; }
                else if (!ua) { klass = CLS_PAIR_ONLY_2; sel = require_both ? 0 : 1; }
                else if (pa == pb) {
                    klass = CLS_PAIR_SAME;
                    sel = (b.status < a.status || (b.status == a.status && (b.one > a.one || (b.one == a.one && b.rest < a.rest)))) ? 1 : 0;
                } else if (pb <= pa && pa - pb < p.size_by_pre[pb]) { klass = CLS_PAIR_NESTED_1; sel = conservative ? 1 : 0; }
                else if (pa <= pb && pb - pa < p.size_by_pre[pa]) { klass = CLS_PAIR_NESTED_2; sel = conservative ? 0 : 1; }
                else {
                    klass = CLS_PAIR_DISCORDANT;
                    sel = 2;
                    lca = pa;
                    for (uint32_t g = p.depth_by_pre[pa]; g > 0; --g) {  // (the root holds every clade)
                        lca = p.parent_by_pre[lca];
                        if (lca <= pb && pb - lca < p.size_by_pre[lca]) break;
                    }
                }
                Rec o = sel == 1 ? b : a;
                if (sel == 2) { o.status = CLS_MAX_RESOLUTION; o.one = 0; o.rest = 0; o.levels = p.depth_by_pre[lca]; o.clade = p.id_by_pre[lca]; }
                os_w[3 * rl + wo] = (unsigned long long)(o.status & 0xFFu) | ((unsigned long long)(uint32_t)o.one << 32);  // (pad bytes: 0)
                os_w[3 * rl + wo + 1] = (unsigned long long)(uint32_t)o.rest | ((unsigned long long)o.levels << 32);
                os_w[3 * rl + wo + 2] = o.clade;
                if (how) how[r] = (uint8_t)klass;
            }
#pragma unroll
            for (uint32_t s = 0; s < 7; ++s) {
                const uint32_t k = (uint32_t)__popcll(__ballot(klass == s));
                if ((uint32_t)lane == s) acc += k;
            }
        }
        __syncthreads();
        if (active) {
            // the chunk's records are words [lo_min, hi_max) of `qo`; stage word i holds word a0 + i
            const uint64_t a0 = c * SEG_WORDS;
            const uint64_t left = (uint64_t)n - c * CHUNK_PAIRS, cnt = left < CHUNK_PAIRS ? left : CHUNK_PAIRS;
            const uint64_t lo_min = a0 + wo, hi_max = lo_min + 3 * cnt;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int s = lane + 64 * j;
                const uint64_t lo = a0 + 2ull * (uint64_t)s;
                const bool lo_ok = lo >= lo_min && lo < hi_max, hi_ok = lo + 1 >= lo_min && lo + 1 < hi_max;
                if (lo_ok && hi_ok) *reinterpret_cast<uint4*>(qo + lo) = *reinterpret_cast<const uint4*>(&os_w[2 * s]);
                else {
                    if (lo_ok) qo[lo] = os_w[2 * s];
                    if (hi_ok) qo[lo + 1] = os_w[2 * s + 1];
                }
            }
            if (wo && lane == 0 && a0 + SEG_WORDS < hi_max) qo[a0 + SEG_WORDS] = os_w[SEG_WORDS];
        }
        // (the next round's loads rewrite `stage` only; `ostage` is rewritten behind the next round's first barrier)
    }

    if (lane < 7 && acc) atomicAdd(&s_tot[lane], acc);
    __syncthreads();
    if (tid < 7 && s_tot[tid]) global_add(&p.totals[tid], s_tot[tid]);
}

__global__ __launch_bounds__(256) void pair_names_kernel(const char* __restrict__ h1, const uint64_t* __restrict__ off1, const char* __restrict__ h2,
                                                         const uint64_t* __restrict__ off2, uint32_t stride, uint32_t n,
                                                         unsigned long long* __restrict__ result) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint64_t r = i * stride;
        const uint64_t o1 = off1[r], o2 = off2[r];
        const uint64_t l1 = pair_name_len(h1 + o1, off1[r + 1] - o1), l2 = pair_name_len(h2 + o2, off2[r + 1] - o2);
        bad = l1 != l2;
        for (uint64_t k = 0; !bad && k < l1; ++k) bad = h1[o1 + k] != h2[o2 + k];
    }
    const unsigned long long mask = __ballot(bad);
    if (mask && (threadIdx.x & 63) == 0) {  // lane 0 of the wave; the wave's lowest disagreeing lane is its lowest index
        global_add(&result[0], (unsigned long long)__popcll(mask));
        (void)atomicMin(&result[1], i + (unsigned long long)(__ffsll(mask) - 1));
    }
}

__global__ __launch_bounds__(256) void pair_gather_headers_kernel(const char* __restrict__ src, const uint64_t* __restrict__ off, uint32_t stride,
                                                                  uint32_t n, const uint64_t* __restrict__ new_off, char* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i * stride], len = off[i * stride + 1] - o, d = new_off[i];
    for (uint64_t k = 0; k < len; ++k) dst[d + k] = src[o + k];
}

}  // namespace

hipError_t launch_pair_records(const PairDev& p, const void* d_a, const void* d_b, uint32_t stride, uint32_t n, uint32_t flags, void* d_out,
                               void* d_how, uint32_t n_cu, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uintptr_t a = (uintptr_t)d_a, b = (uintptr_t)d_b, o = (uintptr_t)d_out;
    const unsigned long long* qa = (const unsigned long long*)(a & ~(uintptr_t)15);
    const unsigned long long* qb = (const unsigned long long*)(b & ~(uintptr_t)15);
    unsigned long long* qo = (unsigned long long*)(o & ~(uintptr_t)15);
    const uint32_t wa = (uint32_t)((a >> 3) & 1u), wb = (uint32_t)((b >> 3) & 1u), wo = (uint32_t)((o >> 3) & 1u);
    const uint64_t n_chunks = ((uint64_t)n + CHUNK_PAIRS - 1) / CHUNK_PAIRS;
    const uint64_t want = (n_chunks + WAVES - 1) / WAVES;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(want, (uint64_t)std::max(1u, n_cu) * 4);  // (four workgroups' LDS fit a CU)
    if (stride == 2) hipLaunchKernelGGL(pair_records_kernel<2>, dim3(blocks), dim3(TB), 0, stream, p, qa, wa, qb, wb, n, flags, qo, wo, (uint8_t*)d_how);
    else hipLaunchKernelGGL(pair_records_kernel<1>, dim3(blocks), dim3(TB), 0, stream, p, qa, wa, qb, wb, n, flags, qo, wo, (uint8_t*)d_how);
    return hipGetLastError();
}

hipError_t launch_pair_names(const char* d_headers1, const uint64_t* d_off1, const char* d_headers2, const uint64_t* d_off2, uint32_t stride,
                             uint32_t n, unsigned long long* d_result, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(pair_names_kernel, dim3(blocks), dim3(256), 0, stream, d_headers1, d_off1, d_headers2, d_off2, stride, n, d_result);
    return hipGetLastError();
}

hipError_t launch_pair_gather_headers(const char* d_src, const uint64_t* d_off, uint32_t stride, uint32_t n, const uint64_t* d_new_off, char* d_dst,
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(pair_gather_headers_kernel, dim3(blocks), dim3(256), 0, stream, d_src, d_off, stride, n, d_new_off, d_dst);
    return hipGetLastError();
}

}  // namespace cls
