// Clade tally: placement records -> per-clade counters, on the device (include/cls_place.h "clade tally").
//
// tally_add_kernel reads the 24-byte records as whole lines (16-byte loads, a wave takes 128 records = 3 KiB at a time
// through an LDS stage), finds each clade-bearing record's pre-order index in the tally's id table, and combines
// equal (clade, status) keys before anything leaves the CU:
//   1. per wave: when every key of a wave step is the same one (a single-organism sample), the wave adds its count and
//      its two sums once;
//   2. per workgroup: an LDS hash table keyed by pre * 4 + (status - 4) with 32-bit counts and 64-bit sums; a key that
//      finds no slot within LT_PROBES probes goes straight to the global counters;
//   3. per launch: one global 64-bit atomic (device scope) per counter and occupied slot, when the workgroup ends.
// The twelve status totals are counted with ballots into registers and reduced per workgroup.  Nothing depends on
// `status` or `clade_id` being sane: a status >= 12 is counted as such, an id that is no clade's as unknown.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "cls_place.h"
#include "cls_tally.h"

namespace cls {
namespace {

constexpr int TB = 256;              // threads per workgroup
constexpr int WAVES = TB / 64;
constexpr int CHUNK_RECS = 128;      // records a wave stages at a time: 3 x (64 lanes x 16 bytes)
constexpr int CHUNK_WORDS = 3 * CHUNK_RECS;
constexpr int STAGE_WORDS = CHUNK_WORDS + 2;  // one more word when the records start in the upper half of a 16-byte slot
constexpr uint32_t LT_SLOTS = 1024;  // LDS table: 4 + 4 + 8 + 8 bytes a slot = 24 KiB
constexpr int LT_PROBES = 8;
constexpr uint32_t LT_EMPTY = 0xFFFFFFFFu;

__device__ inline void global_add(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// `q`: the 16-byte-aligned address at or below the first record, as 8-byte words; `w0`: the word of `q` the first
// record starts at (0 or 1).  Word a of `q` belongs to the records iff w0 <= a < w0 + 3 n.
__global__ __launch_bounds__(TB) void tally_add_kernel(TallyDev t, const unsigned long long* __restrict__ q, uint32_t w0, uint32_t n,
                                                       int wave_combine) {
    __shared__ __attribute__((aligned(16))) unsigned long long stage[WAVES][STAGE_WORDS];
    __shared__ uint32_t s_key[LT_SLOTS];
    __shared__ uint32_t s_cnt[LT_SLOTS];
    __shared__ unsigned long long s_one[LT_SLOTS];
    __shared__ unsigned long long s_rest[LT_SLOTS];
    __shared__ uint32_t s_tot[TALLY_TOTALS];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = (uint32_t)tid; i < LT_SLOTS; i += TB) { s_key[i] = LT_EMPTY; s_cnt[i] = 0; s_one[i] = 0; s_rest[i] = 0; }
    if (tid < (int)TALLY_TOTALS) s_tot[tid] = 0;
    __syncthreads();

    const uint64_t end_word = (uint64_t)w0 + 3ull * n;
    const uint64_t n_chunks = ((uint64_t)n + CHUNK_RECS - 1) / CHUNK_RECS;
    uint32_t acc = 0;  // lane s < 12: records of status s; lane 12: status >= 12; lane 13: unknown clade
    unsigned long long* st_w = stage[wave];

    // one add into the workgroup's table, or into the global counters when the key finds no slot
    auto add_key = [&](uint32_t key, uint32_t c, long long so, long long sr) {
        uint32_t h = (key * 2654435761u) >> 22;
        static_assert(LT_SLOTS == 1u << 10, "the hash keeps ten bits");
        for (int probe = 0; probe < LT_PROBES; ++probe) {
            const uint32_t old = atomicCAS(&s_key[h], LT_EMPTY, key);
            if (old == LT_EMPTY || old == key) {
                atomicAdd(&s_cnt[h], c);
                if ((key & 3u) == 0) {  // CLS_IDENTITY_FOUND: the two sums
                    atomicAdd(&s_one[h], (unsigned long long)so);
                    atomicAdd(&s_rest[h], (unsigned long long)sr);
                }
                return;
            }
            h = (h + 1) & (LT_SLOTS - 1);
        }
        const uint32_t pre = key >> 2;
        global_add(&t.cnt[3ull * pre + (key & 3u)], c);
        if ((key & 3u) == 0) {
            global_add((unsigned long long*)&t.sums[2ull * pre], (unsigned long long)so);
            global_add((unsigned long long*)&t.sums[2ull * pre + 1], (unsigned long long)sr);
        }
    };

    // every wave of the workgroup makes the same number of rounds (the barriers below)
    for (uint64_t base = (uint64_t)blockIdx.x * WAVES; base < n_chunks; base += (uint64_t)gridDim.x * WAVES) {
        const uint64_t c = base + (uint64_t)wave;
        const bool active = c < n_chunks;
        if (active) {
            const uint64_t a0 = c * CHUNK_WORDS;  // the chunk's first word of `q`; stage word i holds word a0 + i
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int s = lane + 64 * j;
                const uint64_t lo = a0 + 2ull * (uint64_t)s;
                const bool lo_ok = lo >= w0 && lo < end_word, hi_ok = lo + 1 < end_word;
                if (lo_ok && hi_ok) {
                    const uint4 v = *reinterpret_cast<const uint4*>(q + lo);
                    *reinterpret_cast<uint4*>(&st_w[2 * s]) = v;
                } else {
                    if (lo_ok) st_w[2 * s] = q[lo];
                    if (hi_ok) st_w[2 * s + 1] = q[lo + 1];
                }
            }
            if (w0 && lane == 0 && a0 + CHUNK_WORDS < end_word) st_w[CHUNK_WORDS] = q[a0 + CHUNK_WORDS];
        }
        __syncthreads();
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int rl = lane + 64 * h2;
            const uint64_t r = c * CHUNK_RECS + (uint64_t)rl;
            const bool valid = active && r < n;
            unsigned long long x0 = 0, x1 = 0, x2 = 0;
            if (valid) { x0 = st_w[3 * rl + w0]; x1 = st_w[3 * rl + w0 + 1]; x2 = st_w[3 * rl + w0 + 2]; }
            const uint32_t st = (uint32_t)(x0 & 0xFFu);
            const int one = (int)(uint32_t)(x0 >> 32), rest = (int)(uint32_t)x1;
            const uint32_t klass = valid ? (st < 12 ? st : TALLY_BAD) : 15u;
            const bool bearing = valid && st >= CLS_IDENTITY_FOUND && st <= CLS_INCONCLUSIVE;
            uint32_t pre = TALLY_NO_PRE;
            if (bearing) {
                uint32_t h = (uint32_t)tally_hash(x2) & t.table_mask;
                for (uint32_t probe = 0; probe <= t.table_mask; ++probe) {
                    const uint4 e = *reinterpret_cast<const uint4*>(&t.table[h]);
                    if (e.z == TALLY_NO_PRE) break;
                    if ((((unsigned long long)e.y << 32) | e.x) == x2) { pre = e.z; break; }
                    h = (h + 1) & t.table_mask;
                }
            }
#pragma unroll
            for (uint32_t s = 0; s <= TALLY_BAD; ++s) {
                const uint32_t k = (uint32_t)__popcll(__ballot(klass == s));
                if ((uint32_t)lane == s) acc += k;
            }
            {
                const uint32_t k = (uint32_t)__popcll(__ballot(bearing && pre == TALLY_NO_PRE));
                if ((uint32_t)lane == TALLY_UNKNOWN) acc += k;
            }
            const bool has = bearing && pre != TALLY_NO_PRE;
            const uint32_t key = has ? pre * 4u + (st - CLS_IDENTITY_FOUND) : LT_EMPTY;
            const unsigned long long mask = __ballot(has);
            if (mask == 0) continue;
            const int first = __ffsll(mask) - 1;
            const uint32_t k0 = (uint32_t)__shfl((int)key, first, 64);
            if (wave_combine && __ballot(has && key == k0) == mask) {  // (wave-uniform: ballots)
                const long long so = wave_sum(has ? (long long)one : 0), sr = wave_sum(has ? (long long)rest : 0);
                if (lane == first) add_key(k0, (uint32_t)__popcll(mask), so, sr);
            } else if (has) {
                add_key(key, 1u, (long long)one, (long long)rest);
            }
        }
        __syncthreads();  // the stage is rewritten in the next round
    }

    if (lane < (int)TALLY_TOTALS && acc) atomicAdd(&s_tot[lane], acc);
    __syncthreads();
    if (tid < (int)TALLY_TOTALS && s_tot[tid]) global_add(&t.totals[tid], s_tot[tid]);
    for (uint32_t i = (uint32_t)tid; i < LT_SLOTS; i += TB) {
        const uint32_t key = s_key[i];
        if (key == LT_EMPTY) continue;
        const uint32_t pre = key >> 2;
        global_add(&t.cnt[3ull * pre + (key & 3u)], s_cnt[i]);
        if ((key & 3u) == 0) {
            global_add((unsigned long long*)&t.sums[2ull * pre], s_one[i]);
            global_add((unsigned long long*)&t.sums[2ull * pre + 1], s_rest[i]);
        }
    }
}

__global__ __launch_bounds__(256) void tally_direct_kernel(TallyDev t) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < t.n_nodes) t.prefix[p] = t.cnt[3ull * p] + t.cnt[3ull * p + 1] + t.cnt[3ull * p + 2];
    else if (p == t.n_nodes) t.prefix[p] = 0;
}

__global__ __launch_bounds__(256) void tally_clade_kernel(TallyDev t) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= t.n_nodes) return;
    const uint64_t hi = (uint64_t)p + t.size_by_pre[p];
    t.clade[p] = t.prefix[hi < t.n_nodes ? hi : t.n_nodes] - t.prefix[p];
}

}  // namespace

size_t tally_scan_tmp_bytes(uint32_t n_nodes) {
    size_t need = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(n_nodes + 1), nullptr);
    return need ? need : 16;
}

hipError_t launch_tally_add(const TallyDev& t, const void* d_records, uint32_t n, uint32_t n_cu, int wave_combine, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uintptr_t a = (uintptr_t)d_records;
    const uint32_t w0 = (uint32_t)((a >> 3) & 1u);
    const unsigned long long* q = (const unsigned long long*)(a & ~(uintptr_t)15);
    const uint64_t n_chunks = ((uint64_t)n + CHUNK_RECS - 1) / CHUNK_RECS;
    const uint64_t want = (n_chunks + WAVES - 1) / WAVES;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(want, (uint64_t)std::max(1u, n_cu) * 4);  // (four workgroups' LDS fit a CU)
    hipLaunchKernelGGL(tally_add_kernel, dim3(blocks), dim3(TB), 0, stream, t, q, w0, n, wave_combine);
    return hipGetLastError();
}

hipError_t launch_tally_finish(const TallyDev& t, hipStream_t stream) {
    const uint32_t blocks = (t.n_nodes + 1 + 255) / 256;
    hipLaunchKernelGGL(tally_direct_kernel, dim3(blocks), dim3(256), 0, stream, t);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = t.scan_tmp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(t.scan_tmp, bytes, t.prefix, t.prefix, (int)(t.n_nodes + 1), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tally_clade_kernel, dim3(blocks), dim3(256), 0, stream, t);
    return hipGetLastError();
}

}  // namespace cls
