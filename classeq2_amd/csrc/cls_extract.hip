// Read extraction: placement records -> one selected / not byte per record, and the selected records' original FASTQ
// bytes gathered into one output text, on the device (include/cls_place.h "read extraction").
//
// select_records_kernel: one record per lane.  A record is 24 bytes at an 8-byte aligned address; the lane reads its
// first and its third 8-byte word (status, clade id), which is aligned wherever the buffer starts in a 16-byte slot.
// One probe of the id table (the tally's: IdSlot, tally_hash) and one byte of the selector's painted pre-order table.
// fastq_spans_kernel: rec_off[r] = the start of line 4 r from the FASTQ stage's line starts.
// extract_lengths_kernel + a device-wide exclusive sum: the plan (where every selected item goes).
// extract_gather_kernel, the hot path: the items that are not selected have length 0 in the plan, so the 64 items of a
// group go to ONE contiguous range of the output, and a wave copies that range, not the items: the 64 output offsets,
// source offsets and lengths of the group sit in LDS, every lane takes a 16-byte aligned piece of the output, finds
// the item it lies in with a six-step search over the group's offsets, reads the 16 source bytes from wherever they
// start (source and destination are not mutually aligned) and writes them with one aligned 16-byte store.  Every lane
// has work whatever the items' lengths are; a piece that spans two items, or the appended newline, is put together
// byte by byte in registers and still leaves as one store.  The up to 15 bytes in front of the first aligned piece and
// behind the last one are written one byte per lane.  Nothing outside [out_off[first item], out_off[last item + 1]) is
// written, nothing outside the selected items is read.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "cls_extract.h"

namespace cls {
namespace {

constexpr int TB = 256;
constexpr int WAVES = TB / 64;
constexpr int GROUP = 64;             // items of one wave's round
constexpr uint32_t MAX_BLOCKS = 2048; // grid-stride beyond (256 CUs x 8 workgroups)

__device__ inline void global_add(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TB) void select_records_kernel(SelectDev s, const unsigned long long* __restrict__ q, uint32_t n,
                                                            uint8_t* __restrict__ sel, unsigned long long* __restrict__ n_unplaced) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    bool unplaced_pick = false;
    if (i < n) {
        const uint32_t status = (uint32_t)(q[3 * i] & 0xFFu);
        uint32_t pre = TALLY_NO_PRE;
        if (status >= CLS_IDENTITY_FOUND && status <= CLS_INCONCLUSIVE) {
            const unsigned long long clade = q[3 * i + 2];
            uint32_t h = (uint32_t)tally_hash(clade) & s.table_mask;
            for (uint32_t probe = 0; probe <= s.table_mask; ++probe) {
                const uint4 e = *reinterpret_cast<const uint4*>(&s.table[h]);
                if (e.z == TALLY_NO_PRE) break;
                if ((((unsigned long long)e.y << 32) | e.x) == clade) { pre = e.z; break; }
                h = (h + 1) & s.table_mask;
            }
        }
        bool pick;
        if (pre != TALLY_NO_PRE) pick = s.sel_by_pre[pre] != 0;
        else pick = unplaced_pick = s.unplaced != 0;
        sel[i] = pick ? 1 : 0;
    }
    if (n_unplaced) {
        const unsigned long long m = __ballot(unplaced_pick);
        if (m && (threadIdx.x & 63) == 0) global_add(n_unplaced, (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(TB) void fastq_spans_kernel(const uint64_t* __restrict__ ls, uint64_t n_nl, uint64_t len, uint32_t n,
                                                         uint64_t* __restrict__ rec_off) {
    const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (r > n) return;
    uint64_t o = len;
    if (ls && 4 * r <= n_nl) o = ls[4 * r] < len ? ls[4 * r] : len;
    rec_off[r] = o;
}

__global__ __launch_bounds__(TB) void extract_lengths_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ rec_off, uint32_t stride,
                                                             uint32_t n_items, const uint8_t* __restrict__ sel, uint64_t* __restrict__ out_off,
                                                             unsigned long long* __restrict__ n_selected) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const bool picked = i < n_items && sel[i] != 0;
    uint64_t e = 0;
    if (picked) {
        const uint64_t a = rec_off[i * stride], b = rec_off[(i + 1) * stride];
        e = b - a;
        if (e && text[b - 1] != '\n') ++e;  // (the last record of a text without a final newline)
    }
    if (i <= n_items) out_off[i] = e;
    const unsigned long long m = __ballot(picked);
    if (m && (threadIdx.x & 63) == 0) global_add(n_selected, (unsigned long long)__popcll(m));
}

// the item of the group whose output range holds offset p (d[0] <= p < d[GROUP]): the last j with d[j] <= p
__device__ __forceinline__ int find_item(const uint64_t* d, uint64_t p) {
    int j = 0;
#pragma unroll
    for (int s = GROUP / 2; s > 0; s >>= 1)
        if (d[j + s] <= p) j += s;
    return j;
}

__global__ __launch_bounds__(TB) void extract_gather_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ rec_off, uint32_t stride,
                                                            uint32_t n_items, const uint8_t* __restrict__ sel, const uint64_t* __restrict__ out_off,
                                                            uint8_t* __restrict__ out) {
    __shared__ uint64_t s_d[WAVES][GROUP + 1];  // where item j of the group starts in the output
    __shared__ uint64_t s_a[WAVES][GROUP];      // where it starts in the text
    __shared__ uint64_t s_l[WAVES][GROUP];      // its bytes in the text (0: not selected); one more in the output: a '\n'
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint64_t n_groups = ((uint64_t)n_items + GROUP - 1) / GROUP;
    uint64_t* d = s_d[wave];
    uint64_t* a = s_a[wave];
    uint64_t* l = s_l[wave];
    const uintptr_t out_addr = (uintptr_t)out;

    // every wave of the workgroup makes the same number of rounds (the barriers below)
    for (uint64_t base = (uint64_t)blockIdx.x * WAVES; base < n_groups; base += (uint64_t)gridDim.x * WAVES) {
        const uint64_t g = base + (uint64_t)wave;
        const bool active = g < n_groups;
        uint64_t lo = 0, hi = 0;
        if (active) {
            const uint64_t i = g * GROUP + (uint64_t)lane;
            const bool valid = i < n_items;
            const uint64_t last = std::min<uint64_t>(g * GROUP + GROUP, n_items);
            const uint64_t dj = out_off[valid ? i : (uint64_t)n_items];
            hi = out_off[last];
            lo = __shfl(dj, 0, 64);
            uint64_t aj = 0, lj = 0;
            if (valid && hi > lo && sel[i] != 0) {
                aj = rec_off[i * stride];
                lj = rec_off[(i + 1) * stride] - aj;
            }
            d[lane] = dj;
            a[lane] = aj;
            l[lane] = lj;
            if (lane == 0) d[GROUP] = hi;
        }
        __syncthreads();
        if (active && hi > lo) {
            auto byte_at = [&](uint64_t p) -> uint8_t {
                const int j = find_item(d, p);
                const uint64_t q = p - d[j];
                return q < l[j] ? text[a[j] + q] : (uint8_t)'\n';
            };
            // [lo, head_end): up to the first 16-byte boundary of the output; [head_end, body_end): whole aligned pieces
            const uint64_t head_end = std::min<uint64_t>(hi, lo + ((16 - ((out_addr + lo) & 15)) & 15));
            const uint64_t n_pieces = (hi - head_end) >> 4;
            const uint64_t body_end = head_end + (n_pieces << 4);
            if (lo + (uint64_t)lane < head_end) out[lo + lane] = byte_at(lo + lane);
            if (body_end + (uint64_t)lane < hi) out[body_end + lane] = byte_at(body_end + lane);
            for (uint64_t c = (uint64_t)lane; c < n_pieces; c += 64) {
                const uint64_t p = head_end + (c << 4);
                int j = find_item(d, p);
                const uint64_t q = p - d[j];
                uint4 v;
                if (q + 16 <= l[j]) {
                    __builtin_memcpy(&v, text + a[j] + q, 16);  // (any alignment)
                } else {  // the piece holds the end of item j: its last bytes, an appended '\n', the next items' first bytes
                    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const uint64_t pp = p + (uint64_t)k;
                        while (d[j + 1] <= pp) ++j;  // (pp < hi = d[GROUP]: j stays below GROUP)
                        const uint64_t qq = pp - d[j];
                        const uint32_t b = qq < l[j] ? text[a[j] + qq] : (uint32_t)'\n';
                        w[k >> 2] |= b << (8 * (k & 3));
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *reinterpret_cast<uint4*>(out + p) = v;
            }
        }
        __syncthreads();  // (the next round rewrites the group's tables)
    }
}

}  // namespace

hipError_t launch_select_records(const SelectDev& s, const void* d_records, uint32_t n, uint8_t* d_sel, unsigned long long* d_n_unplaced,
                                 hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + TB - 1) / TB);
    hipLaunchKernelGGL(select_records_kernel, dim3(blocks), dim3(TB), 0, stream, s, (const unsigned long long*)d_records, n, d_sel, d_n_unplaced);
    return hipGetLastError();
}

hipError_t launch_fastq_spans(const uint64_t* d_ls, uint64_t n_nl, uint64_t len, uint32_t n, uint64_t* d_rec_off, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 1 + TB - 1) / TB);
    hipLaunchKernelGGL(fastq_spans_kernel, dim3(blocks), dim3(TB), 0, stream, d_ls, n_nl, len, n, d_rec_off);
    return hipGetLastError();
}

size_t extract_scan_tmp_bytes(uint32_t n_items) {
    size_t bytes = 0;
    uint64_t* p = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, p, p, (uint64_t)n_items + 1, nullptr);
    return bytes ? bytes : 16;
}

hipError_t launch_extract_plan(const uint8_t* d_text, const uint64_t* d_rec_off, uint32_t stride, uint32_t n_items, const uint8_t* d_sel,
                               uint64_t* d_out_off, unsigned long long* d_n_selected, void* d_tmp, size_t tmp_bytes, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)(((uint64_t)n_items + 1 + TB - 1) / TB);
    hipLaunchKernelGGL(extract_lengths_kernel, dim3(blocks), dim3(TB), 0, stream, d_text, d_rec_off, stride, n_items, d_sel, d_out_off, d_n_selected);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_out_off, d_out_off, (uint64_t)n_items + 1, stream);
}

hipError_t launch_extract_gather(const uint8_t* d_text, const uint64_t* d_rec_off, uint32_t stride, uint32_t n_items, const uint8_t* d_sel,
                                 const uint64_t* d_out_off, uint8_t* d_out, hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    const uint64_t n_groups = ((uint64_t)n_items + GROUP - 1) / GROUP;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_groups + WAVES - 1) / WAVES, MAX_BLOCKS);
    hipLaunchKernelGGL(extract_gather_kernel, dim3(blocks), dim3(TB), 0, stream, d_text, d_rec_off, stride, n_items, d_sel, d_out_off, d_out);
    return hipGetLastError();
}

}  // namespace cls
