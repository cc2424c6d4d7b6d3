// FASTA input stage on the device: the record semantics of
// FileOrStdin::sequence_content_by_channel (core/src/domain/dtos/file_or_stdin.rs:76-116) and
// SequenceBody::remove_non_iupac_from_sequence (core/src/domain/dtos/sequence.rs:47-56), as data-parallel passes
// over the file text in HBM.  The filtered bases and their offsets stay on the device, where
// cls_place_batch_device() takes them: the reads never return to the host.
//
// The reference is a line-by-line state machine {header, sequence}.  Restated per header line j (h_j = the line
// with every '>' removed, seq_j = the kept bases up to the next header line, seq_-1 = those before the first):
//   * at header line j: h_{j-1} non-empty -> emit (h_{j-1}, seq_{j-1}), even if seq is empty (:92-95);
//                       h_{j-1} empty and seq_{j-1} non-empty -> "unexpected sequence without header": stop (:96-100)
//   * at end of file: emit (h_last, seq_last) iff both are non-empty (:111-113)
//   * a line that is not valid UTF-8 stops everything when it is reached (BufRead::lines -> `line?`), the pending
//     record is lost; empty lines (after "\n" / "\r\n" stripping) are skipped, which changes nothing
// so every per-byte decision needs only the first character of the byte's own line, and the stop conditions are
// minima over header lines.  Bytes of records that are not emitted always sit at the tail of the two output
// streams, so the streams need no second compaction.
//
// Passes (CH = 4096 bytes per workgroup, 16 per thread):
//   1. last newline inside every chunk                      -> exclusive prefix maximum = newline before the chunk
//   2. count per chunk: kept bases, kept header bytes, header lines; first byte that breaks UTF-8 (atomicMin)
//   3. exclusive sums of the three counts                   (hipCUB)           [host reads the three totals]
//   4. the same classification again, scattering bases / header bytes / per-header-line offsets
//   5. per header line: stop conditions, emitted flag -> exclusive sum -> record offset tables
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <string>

#include "cls_extract.h"
#include "cls_place.h"

extern "C" void cls_internal_set_error(const char* msg);  // cls_api.cpp: the thread-local text behind cls_last_error()

namespace {

constexpr int FA_THREADS = 256, FA_PER_THREAD = 16, FA_CHUNK = FA_THREADS * FA_PER_THREAD;
constexpr unsigned long long NO_POS = ~0ull;

int fa_fail(int code, const std::string& m) { cls_internal_set_error(m.c_str()); return code; }

struct MaxOp { __host__ __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };

__device__ __forceinline__ uint8_t byte_at(const uint8_t* __restrict__ t, uint64_t len, uint64_t i) { return i < len ? t[i] : (uint8_t)'\n'; }

// pass 1: position of the last '\n' inside every chunk (-1: none)
__global__ __launch_bounds__(FA_THREADS) void fa_last_newline(const uint8_t* __restrict__ text, uint64_t len, long long* __restrict__ chunk_last_nl) {
    __shared__ long long best;
    if (threadIdx.x == 0) best = -1;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * FA_CHUNK + (uint64_t)threadIdx.x * FA_PER_THREAD;
    long long mine = -1;
    for (int k = 0; k < FA_PER_THREAD; ++k)
        if (base + k < len && text[base + k] == '\n') mine = (long long)(base + k);
    if (mine >= 0) atomicMax(&best, mine);
    __syncthreads();
    if (threadIdx.x == 0) chunk_last_nl[blockIdx.x] = best;
}

// Is byte i part of a well-formed UTF-8 sequence?  Decided from the bytes around it (a sequence is at most 4 bytes
// and cannot cross a '\n', which is no continuation byte); the end of the text truncates like a line end.
__device__ __forceinline__ bool utf8_ok_at(const uint8_t* __restrict__ t, uint64_t len, uint64_t i) {
    const uint8_t b = t[i];
    if (b < 0x80) return true;
    auto cont = [&](uint64_t j) { return j < len && (t[j] & 0xC0) == 0x80; };
    if ((b & 0xC0) == 0x80) {  // continuation byte: a lead byte within the 3 bytes before must claim it
        for (uint64_t k = 1; k <= 3 && k <= i; ++k) {
            const uint8_t p = t[i - k];
            if ((p & 0xC0) == 0x80) continue;
            const uint32_t need = p >= 0xF0 && p <= 0xF4 ? 3 : p >= 0xE0 && p <= 0xEF ? 2 : p >= 0xC2 && p <= 0xDF ? 1 : 0;
            return need >= k;
        }
        return false;
    }
    if (b >= 0xC2 && b <= 0xDF) return cont(i + 1);
    if (b >= 0xE0 && b <= 0xEF) {
        if (!cont(i + 1) || !cont(i + 2)) return false;
        const uint8_t s = t[i + 1];
        return !(b == 0xE0 && s < 0xA0) && !(b == 0xED && s > 0x9F);  // overlong / surrogates
    }
    if (b >= 0xF0 && b <= 0xF4) {
        if (!cont(i + 1) || !cont(i + 2) || !cont(i + 3)) return false;
        const uint8_t s = t[i + 1];
        return !(b == 0xF0 && s < 0x90) && !(b == 0xF4 && s > 0x8F);  // overlong / beyond U+10FFFF
    }
    return false;  // 0xC0, 0xC1, 0xF5..0xFF
}

struct FaOut {
    uint8_t* bases;
    uint8_t* headers;
    uint64_t* line_pos;       // per header line: its position in the text,
    uint64_t* line_base_off;  // kept bases before it,
    uint64_t* line_hdr_off;   // kept header bytes before it
};

// passes 2 and 4: classify every byte of the chunk; count (WRITE = false) or scatter (WRITE = true)
template <bool WRITE>
__global__ __launch_bounds__(FA_THREADS) void fa_pass(const uint8_t* __restrict__ text, uint64_t len, const long long* __restrict__ prev_nl,
                                                      uint64_t* __restrict__ cnt_bases, uint64_t* __restrict__ cnt_hdr, uint64_t* __restrict__ cnt_lines,
                                                      unsigned long long* __restrict__ first_bad, FaOut out) {
    __shared__ long long s_nl[FA_THREADS];
    __shared__ uint32_t s_cnt[3][FA_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * FA_CHUNK + (uint64_t)tid * FA_PER_THREAD;
    uint8_t b[FA_PER_THREAD + 1];
    for (int k = 0; k <= FA_PER_THREAD; ++k) b[k] = byte_at(text, len, base + k);
    // last newline at or before the end of each thread's bytes: inclusive maximum over the threads before it
    long long mine = -1;
    for (int k = 0; k < FA_PER_THREAD; ++k) if (base + k < len && b[k] == '\n') mine = (long long)(base + k);
    s_nl[tid] = mine;
    __syncthreads();
    for (int o = 1; o < FA_THREADS; o <<= 1) {
        const long long v = tid >= (uint32_t)o ? s_nl[tid - o] : -1;
        __syncthreads();
        if (v > s_nl[tid]) s_nl[tid] = v;
        __syncthreads();
    }
    long long last_nl = tid ? s_nl[tid - 1] : -1;          // last newline before this thread's first byte, inside the chunk
    if (last_nl < 0) last_nl = prev_nl[blockIdx.x];        // ... or before the chunk (-1: none at all)
    bool is_hdr = byte_at(text, len, (uint64_t)(last_nl + 1)) == '>' && (uint64_t)(last_nl + 1) < len;
    uint32_t flags_base = 0, flags_hdr = 0, flags_line = 0;
    bool bad = false;
    uint64_t bad_pos = 0;
    for (int k = 0; k < FA_PER_THREAD; ++k) {
        const uint64_t i = base + k;
        if (i >= len) break;
        const uint8_t c = b[k];
        if ((uint64_t)(last_nl + 1) == i) {  // a line starts here
            is_hdr = c == '>';
            if (is_hdr) flags_line |= 1u << k;
        }
        if (c >= 0x80 && !bad && !utf8_ok_at(text, len, i)) { bad = true; bad_pos = i; }
        if (is_hdr) {
            // the header is the line without its terminator ("\n" or "\r\n") and without any '>' (:102)
            if (c != '>' && c != '\n' && !(c == '\r' && i + 1 < len && b[k + 1] == '\n')) flags_hdr |= 1u << k;
        } else {
            const uint8_t u = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
            if (u == 'A' || u == 'C' || u == 'G' || u == 'T') flags_base |= 1u << k;
        }
        if (c == '\n') last_nl = (long long)i;
    }
    if (bad && !WRITE) atomicMin(first_bad, (unsigned long long)bad_pos);
    s_cnt[0][tid] = __popc(flags_base);
    s_cnt[1][tid] = __popc(flags_hdr);
    s_cnt[2][tid] = __popc(flags_line);
    __syncthreads();
    for (int o = 1; o < FA_THREADS; o <<= 1) {  // inclusive sums over the threads of the chunk
        uint32_t v[3];
        for (int a = 0; a < 3; ++a) v[a] = tid >= (uint32_t)o ? s_cnt[a][tid - o] : 0u;
        __syncthreads();
        for (int a = 0; a < 3; ++a) s_cnt[a][tid] += v[a];
        __syncthreads();
    }
    if (!WRITE) {
        if (tid == FA_THREADS - 1) { cnt_bases[blockIdx.x] = s_cnt[0][tid]; cnt_hdr[blockIdx.x] = s_cnt[1][tid]; cnt_lines[blockIdx.x] = s_cnt[2][tid]; }
        return;
    }
    uint64_t ob = cnt_bases[blockIdx.x] + (tid ? s_cnt[0][tid - 1] : 0u);   // (the arrays now hold the exclusive sums over chunks)
    uint64_t oh = cnt_hdr[blockIdx.x] + (tid ? s_cnt[1][tid - 1] : 0u);
    uint64_t ol = cnt_lines[blockIdx.x] + (tid ? s_cnt[2][tid - 1] : 0u);
    for (int k = 0; k < FA_PER_THREAD; ++k) {
        const uint8_t c = b[k];
        if ((flags_line >> k) & 1u) { out.line_pos[ol] = base + k; out.line_base_off[ol] = ob; out.line_hdr_off[ol] = oh; ++ol; }
        if ((flags_base >> k) & 1u) out.bases[ob++] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
        if ((flags_hdr >> k) & 1u) out.headers[oh++] = c;
    }
}

// pass 5a: where does the reference stop?  -> stop[0] = number of header lines it processes, stop[1] = truncated
__global__ void fa_stop(const uint8_t* __restrict__ text, uint64_t len, uint64_t n_lines, const uint64_t* __restrict__ line_pos,
                        const uint64_t* __restrict__ line_base_off, const uint64_t* __restrict__ line_hdr_off, uint64_t total_bases,
                        uint64_t total_hdr, unsigned long long first_bad, unsigned long long* __restrict__ stop) {
    // "unexpected sequence without header" at header line j: the header before it is empty, bases in between
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_lines) {
        const bool prev_empty = j == 0 ? true : line_hdr_off[j] == line_hdr_off[j - 1];
        const uint64_t seq = j == 0 ? line_base_off[0] : line_base_off[j] - line_base_off[j - 1];
        if (prev_empty && seq > 0) atomicMin(&stop[0], (unsigned long long)j);
    }
    if (j == 0 && first_bad != NO_POS) {
        // header lines that start before the line holding the first invalid byte
        uint64_t ls = first_bad;
        while (ls > 0 && text[ls - 1] != '\n') --ls;
        uint64_t lo = 0, hi = n_lines;  // first header line with line_pos >= ls
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (line_pos[mid] < ls) lo = mid + 1; else hi = mid; }
        atomicMin(&stop[0], (unsigned long long)lo);
        stop[1] = 1;
    }
    (void)len; (void)total_bases; (void)total_hdr;
}

// pass 5b: emitted flag per header line (record i is emitted when header line i+1 is processed, or at the end of file)
__global__ void fa_emit_flags(uint64_t n_lines, const uint64_t* __restrict__ line_base_off, const uint64_t* __restrict__ line_hdr_off,
                              uint64_t total_bases, uint64_t total_hdr, const unsigned long long* __restrict__ stop, uint64_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const uint64_t n_proc = stop[0] < n_lines ? stop[0] : n_lines;       // header lines processed
    const bool stopped = stop[0] <= n_lines && (stop[0] < n_lines || stop[1] != 0);
    const uint64_t hlen = (i + 1 < n_lines ? line_hdr_off[i + 1] : total_hdr) - line_hdr_off[i];
    bool emit = false;
    if (i + 1 < n_proc) emit = hlen > 0;                                   // emitted at header line i + 1
    else if (i + 1 == n_lines && !stopped && n_proc == n_lines) emit = hlen > 0 && total_bases - line_base_off[i] > 0;  // at end of file
    flag[i] = emit ? 1 : 0;
}

// pass 5c: offset tables of the emitted records
__global__ void fa_records(uint64_t n_lines, const uint64_t* __restrict__ flag, const uint64_t* __restrict__ rank,
                           const uint64_t* __restrict__ line_base_off, const uint64_t* __restrict__ line_hdr_off, uint64_t total_bases,
                           uint64_t total_hdr, uint64_t* __restrict__ base_off, uint64_t* __restrict__ header_off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines || !flag[i]) return;
    const uint64_t r = rank[i];
    base_off[r] = line_base_off[i];
    header_off[r] = line_hdr_off[i];
    // the end of record r = the start of the next header line (everything up to the next emitted record is empty)
    base_off[r + 1] = i + 1 < n_lines ? line_base_off[i + 1] : total_bases;
    header_off[r + 1] = i + 1 < n_lines ? line_hdr_off[i + 1] : total_hdr;
}

#define FA_HIP(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) { cleanup(); return fa_fail(e_ == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
    } while (0)

}  // namespace

extern "C" void cls_fasta_dev_free(cls_fasta_dev* f) {
    if (!f) return;
    if (f->d_headers) (void)hipFree(f->d_headers);
    if (f->d_header_off) (void)hipFree(f->d_header_off);
    if (f->d_bases) (void)hipFree(f->d_bases);
    if (f->d_base_off) (void)hipFree(f->d_base_off);
    memset(f, 0, sizeof *f);
}

extern "C" int cls_fasta_scan_device(const void* d_text, uint64_t len, cls_fasta_dev* out, void* hip_stream) {
    if (!out || (!d_text && len)) return fa_fail(CLS_E_INVALID_ARG, "cls_fasta_scan_device: null argument");
    memset(out, 0, sizeof *out);
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint8_t* text = (const uint8_t*)d_text;
    const uint64_t n_chunks = (len + FA_CHUNK - 1) / FA_CHUNK;
    long long *d_last = nullptr, *d_prev = nullptr;
    uint64_t *d_cnt = nullptr, *d_line = nullptr, *d_flag = nullptr, *d_rank = nullptr;
    unsigned long long* d_misc = nullptr;  // [0] first invalid byte, [1..2] stop
    void* d_tmp = nullptr;
    bool ok = false;
    auto cleanup = [&]() {
        for (void* p : {(void*)d_last, (void*)d_prev, (void*)d_cnt, (void*)d_line, (void*)d_flag, (void*)d_rank, (void*)d_misc, d_tmp}) if (p) (void)hipFree(p);
        d_last = d_prev = nullptr; d_cnt = d_line = d_flag = d_rank = nullptr; d_misc = nullptr; d_tmp = nullptr;
        if (!ok) cls_fasta_dev_free(out);
    };
    auto fail_out = [&](int rc) { return rc; };
    try {
        FA_HIP(hipMalloc((void**)&d_misc, 4 * sizeof(unsigned long long)));
        const unsigned long long init[4] = {NO_POS, NO_POS, 0, 0};
        FA_HIP(hipMemcpyAsync(d_misc, init, sizeof init, hipMemcpyHostToDevice, stream));
        uint64_t totals[3] = {0, 0, 0};  // bases, header bytes, header lines
        unsigned long long first_bad = NO_POS;
        if (n_chunks) {
            FA_HIP(hipMalloc((void**)&d_last, n_chunks * 8));
            FA_HIP(hipMalloc((void**)&d_prev, n_chunks * 8));
            FA_HIP(hipMalloc((void**)&d_cnt, 3 * (n_chunks + 1) * 8));
            uint64_t* cnt[3] = {d_cnt, d_cnt + (n_chunks + 1), d_cnt + 2 * (n_chunks + 1)};
            hipLaunchKernelGGL(fa_last_newline, dim3((unsigned)n_chunks), dim3(FA_THREADS), 0, stream, text, len, d_last);
            size_t tmp_bytes = 0, need = 0;
            (void)hipcub::DeviceScan::ExclusiveScan(nullptr, need, d_last, d_prev, MaxOp(), (long long)-1, (int)n_chunks, stream);
            tmp_bytes = need;
            (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need, cnt[0], cnt[0], (int)(n_chunks + 1), stream);
            tmp_bytes = std::max(tmp_bytes, need);
            FA_HIP(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
            FA_HIP(hipcub::DeviceScan::ExclusiveScan(d_tmp, tmp_bytes, d_last, d_prev, MaxOp(), (long long)-1, (int)n_chunks, stream));
            FA_HIP(hipMemsetAsync(d_cnt, 0, 3 * (n_chunks + 1) * 8, stream));
            hipLaunchKernelGGL((fa_pass<false>), dim3((unsigned)n_chunks), dim3(FA_THREADS), 0, stream, text, len, d_prev, cnt[0], cnt[1], cnt[2],
                               d_misc, FaOut{});
            for (int a = 0; a < 3; ++a) FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, cnt[a], cnt[a], (int)(n_chunks + 1), stream));
            for (int a = 0; a < 3; ++a) FA_HIP(hipMemcpyAsync(&totals[a], cnt[a] + n_chunks, 8, hipMemcpyDeviceToHost, stream));
            FA_HIP(hipMemcpyAsync(&first_bad, d_misc, 8, hipMemcpyDeviceToHost, stream));
            FA_HIP(hipStreamSynchronize(stream));
            // outputs (sized exactly) + the per-header-line tables
            const uint64_t nb = totals[0], nh = totals[1], nl = totals[2];
            FA_HIP(hipMalloc(&out->d_bases, nb ? nb : 16));
            FA_HIP(hipMalloc(&out->d_headers, nh ? nh : 16));
            FA_HIP(hipMalloc((void**)&d_line, 3 * (nl + 1) * 8));
            FaOut fo{(uint8_t*)out->d_bases, (uint8_t*)out->d_headers, d_line, d_line + (nl + 1), d_line + 2 * (nl + 1)};
            hipLaunchKernelGGL((fa_pass<true>), dim3((unsigned)n_chunks), dim3(FA_THREADS), 0, stream, text, len, d_prev, cnt[0], cnt[1], cnt[2],
                               d_misc, fo);
            uint64_t n_rec = 0;
            unsigned long long stop_h[2] = {NO_POS, 0};
            FA_HIP(hipMalloc((void**)&out->d_base_off, (nl + 2) * 8));
            FA_HIP(hipMalloc((void**)&out->d_header_off, (nl + 2) * 8));
            FA_HIP(hipMemsetAsync(out->d_base_off, 0, 8, stream));
            FA_HIP(hipMemsetAsync(out->d_header_off, 0, 8, stream));
            if (nl) {
                const unsigned blocks = (unsigned)((nl + 255) / 256);
                hipLaunchKernelGGL(fa_stop, dim3(blocks), dim3(256), 0, stream, text, len, nl, fo.line_pos, fo.line_base_off, fo.line_hdr_off, nb, nh,
                                   first_bad, d_misc + 1);
                FA_HIP(hipMalloc((void**)&d_flag, (nl + 1) * 8));
                FA_HIP(hipMalloc((void**)&d_rank, (nl + 1) * 8));
                FA_HIP(hipMemsetAsync(d_flag, 0, (nl + 1) * 8, stream));
                hipLaunchKernelGGL(fa_emit_flags, dim3(blocks), dim3(256), 0, stream, nl, fo.line_base_off, fo.line_hdr_off, nb, nh, d_misc + 1, d_flag);
                size_t need2 = 0;
                (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need2, d_flag, d_rank, (int)(nl + 1), stream);
                if (need2 > tmp_bytes) { (void)hipFree(d_tmp); d_tmp = nullptr; FA_HIP(hipMalloc(&d_tmp, need2)); tmp_bytes = need2; }
                FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_flag, d_rank, (int)(nl + 1), stream));
                hipLaunchKernelGGL(fa_records, dim3(blocks), dim3(256), 0, stream, nl, d_flag, d_rank, fo.line_base_off, fo.line_hdr_off, nb, nh,
                                   (uint64_t*)out->d_base_off, (uint64_t*)out->d_header_off);
                FA_HIP(hipMemcpyAsync(&n_rec, d_rank + nl, 8, hipMemcpyDeviceToHost, stream));
                FA_HIP(hipMemcpyAsync(stop_h, d_misc + 1, 16, hipMemcpyDeviceToHost, stream));
                FA_HIP(hipStreamSynchronize(stream));
            } else if (first_bad != NO_POS) {
                stop_h[1] = 1;
            } else if (nb > 0) {
                stop_h[0] = 0;  // bases but no header line at all: nothing is emitted, no error either (the end-of-file test needs a header)
            }
            if (n_rec > 0xFFFFFFFFull) { cleanup(); return fail_out(fa_fail(CLS_E_INVALID_ARG, "cls_fasta_scan_device: more than 2^32 records")); }
            out->n = (uint32_t)n_rec;
            out->truncated = (stop_h[1] != 0 || (nl && stop_h[0] < nl)) ? 1u : 0u;
            if (hipGetLastError() != hipSuccess) { cleanup(); return fail_out(fa_fail(CLS_E_HIP, "cls_fasta_scan_device: kernel launch failed")); }
            // the record tables say how much of the two streams belongs to emitted records
            uint64_t ends[2] = {0, 0};
            FA_HIP(hipMemcpyAsync(&ends[0], (uint64_t*)out->d_base_off + n_rec, 8, hipMemcpyDeviceToHost, stream));
            FA_HIP(hipMemcpyAsync(&ends[1], (uint64_t*)out->d_header_off + n_rec, 8, hipMemcpyDeviceToHost, stream));
            FA_HIP(hipStreamSynchronize(stream));
            out->n_bases = ends[0];
            out->n_header_bytes = ends[1];
        } else {
            FA_HIP(hipMalloc(&out->d_bases, 16));
            FA_HIP(hipMalloc(&out->d_headers, 16));
            FA_HIP(hipMalloc((void**)&out->d_base_off, 16));
            FA_HIP(hipMalloc((void**)&out->d_header_off, 16));
            FA_HIP(hipMemsetAsync(out->d_base_off, 0, 16, stream));
            FA_HIP(hipMemsetAsync(out->d_header_off, 0, 16, stream));
            FA_HIP(hipStreamSynchronize(stream));
        }
        ok = true;
        cleanup();
        return CLS_OK;
    } catch (...) {
        cleanup();
        return fail_out(fa_fail(CLS_E_INTERNAL, "cls_fasta_scan_device: unknown exception"));
    }
}

// Host text in, host records out, through the device passes (what the tests compare with cls_fasta_parse).
extern "C" int cls_fasta_parse_gpu(const char* text, size_t len, int device, cls_fasta* out) {
    if (!out || (!text && len)) return fa_fail(CLS_E_INVALID_ARG, "cls_fasta_parse_gpu: null argument");
    memset(out, 0, sizeof *out);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fa_fail(CLS_E_NO_DEVICE, "cls_fasta_parse_gpu: no HIP device is visible");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return fa_fail(CLS_E_INVALID_ARG, "cls_fasta_parse_gpu: bad device ordinal");
    void* d_text = nullptr;
    cls_fasta_dev dv;
    memset(&dv, 0, sizeof dv);
    auto cleanup = [&]() { if (d_text) (void)hipFree(d_text); cls_fasta_dev_free(&dv); };
    FA_HIP(hipMalloc(&d_text, len ? len : 16));
    if (len) FA_HIP(hipMemcpy(d_text, text, len, hipMemcpyHostToDevice));
    int rc = cls_fasta_scan_device(d_text, len, &dv, nullptr);
    if (rc != CLS_OK) { cleanup(); return rc; }
    out->n = dv.n;
    out->truncated = dv.truncated;
    out->headers = (char*)malloc(dv.n_header_bytes + 1);
    out->bases = (char*)malloc(dv.n_bases + 1);
    out->header_off = (uint64_t*)malloc(((size_t)dv.n + 1) * 8);
    out->base_off = (uint64_t*)malloc(((size_t)dv.n + 1) * 8);
    if (!out->headers || !out->bases || !out->header_off || !out->base_off) { cleanup(); cls_fasta_free(out); return fa_fail(CLS_E_NOMEM, "cls_fasta_parse_gpu: out of host memory"); }
    if (dv.n_header_bytes) FA_HIP(hipMemcpy(out->headers, dv.d_headers, dv.n_header_bytes, hipMemcpyDeviceToHost));
    if (dv.n_bases) FA_HIP(hipMemcpy(out->bases, dv.d_bases, dv.n_bases, hipMemcpyDeviceToHost));
    FA_HIP(hipMemcpy(out->header_off, dv.d_header_off, ((size_t)dv.n + 1) * 8, hipMemcpyDeviceToHost));
    FA_HIP(hipMemcpy(out->base_off, dv.d_base_off, ((size_t)dv.n + 1) * 8, hipMemcpyDeviceToHost));
    cleanup();
    return CLS_OK;
}

// ---- FASTQ stage on the device (include/cls_place.h states the rules) -----------------------------------------
// Record r is lines 4r .. 4r+3 by line index, so the structure needs only the line starts, never the lines' content
// (a quality line starting with '@' or '+' is no trap).  Passes:
//   1. per 4096-byte chunk: newlines, last byte that is not part of a line terminator
//   2. exclusive sum of the newline counts                          [host reads the line count: sync 1]
//   3. line-start offsets (64-bit) from the newlines' in-chunk ranks
//   4. one wave per record: validate the four lines, trim (wave64 prefix sums over 64-byte pieces of the quality
//      line, from the front for the 5' end, from the back for the 3' end, stopping at the first negative running sum),
//      count the kept bases; the first record that is not well-formed (atomicMin) ends the parse
//   5. exclusive sums of kept bases and header bytes = the record offset tables
//   6. where the parse ends, and whether that is a clean end (blank lines only from there on)  [sync 2: sizes]
//   7. one wave per emitted record: scatter its header bytes and its kept bases (in-wave compaction by ballot)
namespace {

constexpr int FQ_THREADS = 256, FQ_WAVES = FQ_THREADS / 64;
enum : uint8_t { FQ_OK = 0, FQ_BAD = 1, FQ_BLANK = 2 };  // record kinds (FQ_BLANK: line 1 is empty)

// the chunk's bytes of thread `tid` (+ one look-ahead byte; '\n' beyond the text)
__device__ __forceinline__ void fq_load16(const uint8_t* __restrict__ t, uint64_t len, uint64_t base, bool aligned, uint8_t b[FA_PER_THREAD + 1]) {
    if (aligned && base + FA_PER_THREAD <= len) {
        const uint4 v = *reinterpret_cast<const uint4*>(t + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < FA_PER_THREAD; ++k) b[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    } else {
        for (int k = 0; k < FA_PER_THREAD; ++k) b[k] = byte_at(t, len, base + k);
    }
    b[FA_PER_THREAD] = byte_at(t, len, base + FA_PER_THREAD);
}

// pass 1: newlines per chunk, and the last byte of the chunk that is not '\n' nor a '\r' before a '\n' (-1: none)
__global__ __launch_bounds__(FQ_THREADS) void fq_count_lines(const uint8_t* __restrict__ text, uint64_t len, bool aligned,
                                                             uint64_t* __restrict__ cnt_nl, long long* __restrict__ last_text) {
    typedef hipcub::BlockReduce<uint32_t, FQ_THREADS> SumR;
    typedef hipcub::BlockReduce<long long, FQ_THREADS> MaxR;
    __shared__ union { typename SumR::TempStorage s; typename MaxR::TempStorage m; } tmp;
    const uint64_t base = (uint64_t)blockIdx.x * FA_CHUNK + (uint64_t)threadIdx.x * FA_PER_THREAD;
    uint8_t b[FA_PER_THREAD + 1];
    fq_load16(text, len, base, aligned, b);
    uint32_t n = 0;
    long long lt = -1;
    for (int k = 0; k < FA_PER_THREAD; ++k) {
        const uint64_t i = base + k;
        if (i >= len) break;
        if (b[k] == '\n') ++n;
        else if (!(b[k] == '\r' && i + 1 < len && b[k + 1] == '\n')) lt = (long long)i;
    }
    const uint32_t tot = SumR(tmp.s).Sum(n);
    __syncthreads();
    const long long mx = MaxR(tmp.m).Reduce(lt, MaxOp());
    if (threadIdx.x == 0) { cnt_nl[blockIdx.x] = tot; last_text[blockIdx.x] = mx; }
}

// pass 3: ls[k + 1] = the position after newline k; ls[0] = 0, ls[n_nl + 1] = len + 1 (the end of a last line
// without a newline, one past the text like a newline's position + 1)
__global__ __launch_bounds__(FQ_THREADS) void fq_line_starts(const uint8_t* __restrict__ text, uint64_t len, bool aligned,
                                                             const uint64_t* __restrict__ nl_before, uint64_t n_nl, uint64_t* __restrict__ ls) {
    typedef hipcub::BlockScan<uint32_t, FQ_THREADS> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const uint64_t base = (uint64_t)blockIdx.x * FA_CHUNK + (uint64_t)threadIdx.x * FA_PER_THREAD;
    uint8_t b[FA_PER_THREAD + 1];
    fq_load16(text, len, base, aligned, b);
    uint32_t n = 0;
    for (int k = 0; k < FA_PER_THREAD; ++k) n += base + k < len && b[k] == '\n';
    uint32_t rank = 0;
    Scan(tmp).ExclusiveSum(n, rank);
    uint64_t o = nl_before[blockIdx.x] + rank;
    for (int k = 0; k < FA_PER_THREAD; ++k)
        if (base + k < len && b[k] == '\n' && o < n_nl) ls[++o] = base + k + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ls[0] = 0; ls[n_nl + 1] = len + 1; }
}

// content [s, e) of line k (k < the line count): "\n" or "\r\n" stripped
__device__ __forceinline__ void fq_bounds(const uint8_t* __restrict__ t, uint64_t len, const uint64_t* __restrict__ ls, uint64_t k, uint64_t& s, uint64_t& e) {
    s = ls[k];
    const uint64_t nx = ls[k + 1];
    e = nx - 1;
    if (nx - 1 < len && e > s && t[e - 1] == '\r') --e;
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(v, o, 64);
        if (lane >= o) v += x;
    }
    return v;
}

__device__ __forceinline__ int wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ bool is_acgt(uint8_t c) {
    const uint8_t u = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// One end of the trimming rule on the quality bytes q[0, L), by the whole wave: the running sum s of c - q[i] over
// pieces of 64 positions (from the front, or from the back when `from_end`), lanes in visiting order, stops at the
// first negative s; the result is the position after (front) / at (back) the first visit that reached the maximum
// s > 0, else `dflt`.
__device__ uint64_t wave_trim(const uint8_t* __restrict__ q, uint64_t L, int c, bool from_end, int lane, uint64_t dflt) {
    long long carry = 0, best = 0;
    uint64_t res = dflt;
    for (uint64_t base = 0; base < L; base += 64) {
        const uint64_t j = base + (uint64_t)lane;
        const bool valid = j < L;
        const int d = valid ? c - ((int)q[from_end ? L - 1 - j : j] - 33) : 0;
        const int p = wave_incl_sum(d, lane);
        const unsigned long long neg = __ballot(valid && carry + p < 0);
        const int lim = neg ? __ffsll((unsigned long long)neg) - 1 : 64;
        const bool cand = valid && lane < lim;
        const int pm = wave_max(cand ? p : INT_MIN);
        if (pm != INT_MIN && carry + pm > best) {
            best = carry + pm;
            const uint64_t jf = base + (uint64_t)(__ffsll((unsigned long long)__ballot(cand && p == pm)) - 1);
            res = from_end ? L - 1 - jf : jf + 1;
        }
        if (neg) break;
        carry += __shfl(p, 63, 64);
    }
    return res;
}

// pass 4: one wave per record candidate r < n_cand (line 4r exists)
__global__ __launch_bounds__(FQ_THREADS) void fq_records(const uint8_t* __restrict__ text, uint64_t len, const uint64_t* __restrict__ ls,
                                                         uint64_t n_lines, uint64_t n_cand, int c5, int c3, uint64_t* __restrict__ nb,
                                                         uint64_t* __restrict__ nh, uint64_t* __restrict__ win, uint8_t* __restrict__ kind,
                                                         unsigned long long* __restrict__ first_stop) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6);
    if (r >= n_cand) return;
    uint64_t s[4], e[4];
    fq_bounds(text, len, ls, 4 * r, s[0], e[0]);
    uint8_t k = FQ_OK;
    if (s[0] == e[0]) k = FQ_BLANK;
    else if (4 * r + 3 >= n_lines) k = FQ_BAD;  // incomplete
    uint64_t L = 0, lo = 0, hi = 0, cnt = 0;
    if (k == FQ_OK) {
        for (int x = 1; x < 4; ++x) fq_bounds(text, len, ls, 4 * r + x, s[x], e[x]);
        L = e[1] - s[1];
        bool ok = text[s[0]] == '@' && e[0] - s[0] >= 2 && text[s[2]] == '+' && e[3] - s[3] == L;
        bool bad = false;
        if (ok)
            for (uint64_t i = s[0] + 1 + lane; i < e[0]; i += 64) bad |= text[i] >= 0x80 && !utf8_ok_at(text, len, i);
        if (ok)
            for (uint64_t j = lane; j < L; j += 64) {
                const uint8_t c = text[s[1] + j], q = text[s[3] + j];
                bad |= c >= 0x80 || q < '!' || q > '~';
            }
        ok = ok && !__any(bad);
        if (!ok) k = FQ_BAD;
    }
    if (k == FQ_OK) {
        const uint8_t* q = text + s[3];
        const uint64_t a = c5 ? wave_trim(q, L, c5, false, lane, 0) : 0;
        const uint64_t b = c3 ? wave_trim(q, L, c3, true, lane, L) : L;
        if (a < b) { lo = s[1] + a; hi = s[1] + b; }
        for (uint64_t p = lo; p < hi; p += 64) {
            const uint64_t i = p + (uint64_t)lane;
            cnt += __popcll(__ballot(i < hi && is_acgt(text[i])));
        }
    }
    if (lane == 0) {
        kind[r] = k;
        nb[r] = cnt;
        nh[r] = k == FQ_OK ? e[0] - s[0] - 1 : 0;
        win[2 * r] = lo;
        win[2 * r + 1] = hi;
        if (k != FQ_OK) atomicMin(first_stop, (unsigned long long)r);
    }
}

// pass 6: res = {records emitted, truncated, kept bases, header bytes}
__global__ __launch_bounds__(FQ_THREADS) void fq_finish(const uint64_t* __restrict__ ls, uint64_t n_cand, const uint8_t* __restrict__ kind,
                                                        const long long* __restrict__ last_text, uint64_t n_chunks,
                                                        const uint64_t* __restrict__ base_off, const uint64_t* __restrict__ hdr_off,
                                                        const unsigned long long* __restrict__ first_stop, unsigned long long* __restrict__ res) {
    const uint64_t rs = *first_stop;
    const uint64_t n = rs < n_cand ? rs : n_cand;
    bool trunc = false;
    if (rs < n_cand) {
        if (kind[rs] == FQ_BAD) trunc = true;
        else {  // an empty line where record rs starts: a clean end iff no line after it holds anything
            const uint64_t P = ls[4 * rs];
            for (uint64_t c0 = P / FA_CHUNK; c0 < n_chunks; c0 += FQ_THREADS) {
                const uint64_t c = c0 + threadIdx.x;
                if (__syncthreads_or(c < n_chunks && last_text[c] >= (long long)P))  { trunc = true; break; }
            }
        }
    }
    if (threadIdx.x == 0) { res[0] = n; res[1] = trunc ? 1 : 0; res[2] = base_off[n]; res[3] = hdr_off[n]; }
}

// pass 7: one wave per emitted record
__global__ __launch_bounds__(FQ_THREADS) void fq_scatter(const uint8_t* __restrict__ text, const uint64_t* __restrict__ ls, uint64_t n,
                                                         const uint64_t* __restrict__ win, const uint64_t* __restrict__ base_off,
                                                         const uint64_t* __restrict__ hdr_off, uint8_t* __restrict__ bases,
                                                         uint8_t* __restrict__ headers) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint64_t hs = ls[4 * r] + 1, ho = hdr_off[r], hn = hdr_off[r + 1] - ho;
    for (uint64_t j = lane; j < hn; j += 64) headers[ho + j] = text[hs + j];
    const uint64_t lo = win[2 * r], hi = win[2 * r + 1], end = base_off[r + 1];
    uint64_t o = base_off[r];
    const unsigned long long below = (1ull << lane) - 1;
    for (uint64_t p = lo; p < hi; p += 64) {
        const uint64_t i = p + (uint64_t)lane;
        const uint8_t c = i < hi ? text[i] : (uint8_t)0;
        const bool keep = i < hi && is_acgt(c);
        const unsigned long long m = __ballot(keep);
        const uint64_t dst = o + (uint64_t)__popcll(m & below);
        if (keep && dst < end) bases[dst] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
        o += (uint64_t)__popcll(m);
    }
}

}  // namespace

// `keep_ls` != NULL: the line starts (ls[0 .. n_nl + 1]; NULL for the empty text) are handed to the caller, who frees them.
static int fastq_scan_impl(const void* d_text, uint64_t len, const cls_fastq_opts* opts, cls_fasta_dev* out, void* hip_stream,
                           uint64_t** keep_ls, uint64_t* keep_n_nl) {
    if (!out || (!d_text && len)) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_scan_device: null argument");
    memset(out, 0, sizeof *out);
    if (keep_ls) { *keep_ls = nullptr; *keep_n_nl = 0; }
    cls_fastq_opts o{};
    if (opts) {
        o = *opts;
        for (uint32_t x : o.reserved) if (x) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_scan_device: reserved options must be 0");
    }
    const int c5 = (int)std::min<uint32_t>(o.trim_5p, 94), c3 = (int)std::min<uint32_t>(o.trim_3p, 94);  // (exact, cls_place.h)
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint8_t* text = (const uint8_t*)d_text;
    const bool aligned = ((uintptr_t)d_text & 15) == 0;
    const uint64_t n_chunks = (len + FA_CHUNK - 1) / FA_CHUNK;
    uint64_t *d_cnt = nullptr, *d_ls = nullptr, *d_win = nullptr;
    long long* d_lt = nullptr;
    uint8_t* d_kind = nullptr;
    unsigned long long* d_misc = nullptr;  // [0] first record that is not well-formed, [1..4] fq_finish's result
    void* d_tmp = nullptr;
    bool ok = false;
    auto cleanup = [&]() {
        for (void* p : {(void*)d_cnt, (void*)d_ls, (void*)d_win, (void*)d_lt, (void*)d_kind, (void*)d_misc, d_tmp}) if (p) (void)hipFree(p);
        d_cnt = d_ls = d_win = nullptr; d_lt = nullptr; d_kind = nullptr; d_misc = nullptr; d_tmp = nullptr;
        if (!ok) cls_fasta_dev_free(out);
    };
    try {
        if (n_chunks == 0) {
            FA_HIP(hipMalloc(&out->d_bases, 16));
            FA_HIP(hipMalloc(&out->d_headers, 16));
            FA_HIP(hipMalloc((void**)&out->d_base_off, 16));
            FA_HIP(hipMalloc((void**)&out->d_header_off, 16));
            FA_HIP(hipMemsetAsync(out->d_base_off, 0, 16, stream));
            FA_HIP(hipMemsetAsync(out->d_header_off, 0, 16, stream));
            FA_HIP(hipStreamSynchronize(stream));
            ok = true;
            cleanup();
            return CLS_OK;
        }
        FA_HIP(hipMalloc((void**)&d_misc, 8 * sizeof(unsigned long long)));
        FA_HIP(hipMemsetAsync(d_misc, 0xFF, 8, stream));
        FA_HIP(hipMalloc((void**)&d_cnt, (n_chunks + 1) * 8));
        FA_HIP(hipMalloc((void**)&d_lt, n_chunks * 8));
        FA_HIP(hipMemsetAsync(d_cnt + n_chunks, 0, 8, stream));
        hipLaunchKernelGGL(fq_count_lines, dim3((unsigned)n_chunks), dim3(FQ_THREADS), 0, stream, text, len, aligned, d_cnt, d_lt);
        size_t tmp_bytes = 0;
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt, d_cnt, (int)(n_chunks + 1), stream));
        FA_HIP(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, d_cnt, (int)(n_chunks + 1), stream));
        uint64_t n_nl = 0;
        uint8_t last = 0;
        FA_HIP(hipMemcpyAsync(&n_nl, d_cnt + n_chunks, 8, hipMemcpyDeviceToHost, stream));
        FA_HIP(hipMemcpyAsync(&last, text + len - 1, 1, hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));  // sync 1: the line count
        const uint64_t n_lines = n_nl + (last != '\n' ? 1 : 0), n_cand = (n_lines + 3) / 4;
        FA_HIP(hipMalloc((void**)&d_ls, (n_nl + 2) * 8));
        hipLaunchKernelGGL(fq_line_starts, dim3((unsigned)n_chunks), dim3(FQ_THREADS), 0, stream, text, len, aligned, d_cnt, n_nl, d_ls);
        FA_HIP(hipMalloc((void**)&out->d_base_off, (n_cand + 1) * 8));
        FA_HIP(hipMalloc((void**)&out->d_header_off, (n_cand + 1) * 8));
        FA_HIP(hipMalloc((void**)&d_win, 2 * n_cand * 8));
        FA_HIP(hipMalloc((void**)&d_kind, n_cand));
        uint64_t* nb = (uint64_t*)out->d_base_off;
        uint64_t* nh = (uint64_t*)out->d_header_off;
        FA_HIP(hipMemsetAsync(nb + n_cand, 0, 8, stream));
        FA_HIP(hipMemsetAsync(nh + n_cand, 0, 8, stream));
        hipLaunchKernelGGL(fq_records, dim3((unsigned)((n_cand + FQ_WAVES - 1) / FQ_WAVES)), dim3(FQ_THREADS), 0, stream, text, len, d_ls, n_lines,
                           n_cand, c5, c3, nb, nh, d_win, d_kind, d_misc);
        size_t need = 0;
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, nb, nb, (int)(n_cand + 1), stream));
        if (need > tmp_bytes) { (void)hipFree(d_tmp); d_tmp = nullptr; FA_HIP(hipMalloc(&d_tmp, need)); tmp_bytes = need; }
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, nb, nb, (int)(n_cand + 1), stream));
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, nh, nh, (int)(n_cand + 1), stream));
        hipLaunchKernelGGL(fq_finish, dim3(1), dim3(FQ_THREADS), 0, stream, d_ls, n_cand, d_kind, d_lt, n_chunks, nb, nh, d_misc, d_misc + 1);
        unsigned long long res[4] = {0, 0, 0, 0};
        FA_HIP(hipMemcpyAsync(res, d_misc + 1, sizeof res, hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));  // sync 2: the output sizes
        if (hipGetLastError() != hipSuccess) { cleanup(); return fa_fail(CLS_E_HIP, "cls_fastq_scan_device: kernel launch failed"); }
        if (res[0] > 0xFFFFFFFFull) { cleanup(); return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_scan_device: more than 2^32 records"); }
        out->n = (uint32_t)res[0];
        out->truncated = (uint32_t)res[1];
        out->n_bases = res[2];
        out->n_header_bytes = res[3];
        FA_HIP(hipMalloc(&out->d_bases, res[2] ? res[2] : 16));
        FA_HIP(hipMalloc(&out->d_headers, res[3] ? res[3] : 16));
        if (res[0])
            hipLaunchKernelGGL(fq_scatter, dim3((unsigned)((res[0] + FQ_WAVES - 1) / FQ_WAVES)), dim3(FQ_THREADS), 0, stream, text, d_ls, res[0], d_win,
                               nb, nh, (uint8_t*)out->d_bases, (uint8_t*)out->d_headers);
        if (hipGetLastError() != hipSuccess) { cleanup(); return fa_fail(CLS_E_HIP, "cls_fastq_scan_device: kernel launch failed"); }
        // (the temporaries are freed below; hipFree waits for the work that still reads them)
        if (keep_ls) { *keep_ls = d_ls; *keep_n_nl = n_nl; d_ls = nullptr; }
        ok = true;
        cleanup();
        return CLS_OK;
    } catch (...) {
        cleanup();
        return fa_fail(CLS_E_INTERNAL, "cls_fastq_scan_device: unknown exception");
    }
}

extern "C" int cls_fastq_scan_device(const void* d_text, uint64_t len, const cls_fastq_opts* opts, cls_fasta_dev* out, void* hip_stream) {
    return fastq_scan_impl(d_text, len, opts, out, hip_stream, nullptr, nullptr);
}

namespace cls {

int fastq_scan_device_keep(const void* d_text, uint64_t len, const cls_fastq_opts* opts, cls_fasta_dev* out, hipStream_t stream, uint64_t** d_ls,
                           uint64_t* n_nl) {
    if (!d_ls || !n_nl) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_scan_device: null argument");
    return fastq_scan_impl(d_text, len, opts, out, (void*)stream, d_ls, n_nl);
}

// Passes 1 to 3 of the FASTQ stage on their own (the stand-alone cls_fastq_spans_device).
int fastq_line_starts_device(const void* d_text, uint64_t len, uint64_t** d_ls_out, uint64_t* n_nl_out, hipStream_t stream) {
    if (!d_ls_out || !n_nl_out || (!d_text && len)) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_spans_device: null argument");
    *d_ls_out = nullptr;
    *n_nl_out = 0;
    const uint64_t n_chunks = (len + FA_CHUNK - 1) / FA_CHUNK;
    if (n_chunks == 0) return CLS_OK;
    const uint8_t* text = (const uint8_t*)d_text;
    const bool aligned = ((uintptr_t)d_text & 15) == 0;
    uint64_t *d_cnt = nullptr, *d_ls = nullptr;
    long long* d_lt = nullptr;
    void* d_tmp = nullptr;
    auto cleanup = [&]() {
        for (void* p : {(void*)d_cnt, (void*)d_ls, (void*)d_lt, d_tmp}) if (p) (void)hipFree(p);
        d_cnt = d_ls = nullptr; d_lt = nullptr; d_tmp = nullptr;
    };
    try {
        FA_HIP(hipMalloc((void**)&d_cnt, (n_chunks + 1) * 8));
        FA_HIP(hipMalloc((void**)&d_lt, n_chunks * 8));
        FA_HIP(hipMemsetAsync(d_cnt + n_chunks, 0, 8, stream));
        hipLaunchKernelGGL(fq_count_lines, dim3((unsigned)n_chunks), dim3(FQ_THREADS), 0, stream, text, len, aligned, d_cnt, d_lt);
        size_t tmp_bytes = 0;
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt, d_cnt, (int)(n_chunks + 1), stream));
        FA_HIP(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
        FA_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, d_cnt, (int)(n_chunks + 1), stream));
        uint64_t n_nl = 0;
        FA_HIP(hipMemcpyAsync(&n_nl, d_cnt + n_chunks, 8, hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        FA_HIP(hipMalloc((void**)&d_ls, (n_nl + 2) * 8));
        hipLaunchKernelGGL(fq_line_starts, dim3((unsigned)n_chunks), dim3(FQ_THREADS), 0, stream, text, len, aligned, d_cnt, n_nl, d_ls);
        FA_HIP(hipStreamSynchronize(stream));
        if (hipGetLastError() != hipSuccess) { cleanup(); return fa_fail(CLS_E_HIP, "cls_fastq_spans_device: kernel launch failed"); }
        *d_ls_out = d_ls;
        *n_nl_out = n_nl;
        d_ls = nullptr;
        cleanup();
        return CLS_OK;
    } catch (...) {
        cleanup();
        return fa_fail(CLS_E_INTERNAL, "cls_fastq_spans_device: unknown exception");
    }
}

}  // namespace cls

// Host text in, host records out, through the device passes (what the tests compare with cls_fastq_parse).
extern "C" int cls_fastq_parse_gpu(const char* text, size_t len, const cls_fastq_opts* opts, int device, cls_fasta* out) {
    if (!out || (!text && len)) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_parse_gpu: null argument");
    memset(out, 0, sizeof *out);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fa_fail(CLS_E_NO_DEVICE, "cls_fastq_parse_gpu: no HIP device is visible");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return fa_fail(CLS_E_INVALID_ARG, "cls_fastq_parse_gpu: bad device ordinal");
    void* d_text = nullptr;
    cls_fasta_dev dv;
    memset(&dv, 0, sizeof dv);
    auto cleanup = [&]() { if (d_text) (void)hipFree(d_text); cls_fasta_dev_free(&dv); };
    FA_HIP(hipMalloc(&d_text, len ? len : 16));
    if (len) FA_HIP(hipMemcpy(d_text, text, len, hipMemcpyHostToDevice));
    int rc = cls_fastq_scan_device(d_text, len, opts, &dv, nullptr);
    if (rc != CLS_OK) { cleanup(); return rc; }
    out->n = dv.n;
    out->truncated = dv.truncated;
    out->headers = (char*)malloc(dv.n_header_bytes + 1);
    out->bases = (char*)malloc(dv.n_bases + 1);
    out->header_off = (uint64_t*)malloc(((size_t)dv.n + 1) * 8);
    out->base_off = (uint64_t*)malloc(((size_t)dv.n + 1) * 8);
    if (!out->headers || !out->bases || !out->header_off || !out->base_off) { cleanup(); cls_fasta_free(out); return fa_fail(CLS_E_NOMEM, "cls_fastq_parse_gpu: out of host memory"); }
    if (dv.n_header_bytes) FA_HIP(hipMemcpy(out->headers, dv.d_headers, dv.n_header_bytes, hipMemcpyDeviceToHost));
    if (dv.n_bases) FA_HIP(hipMemcpy(out->bases, dv.d_bases, dv.n_bases, hipMemcpyDeviceToHost));
    FA_HIP(hipMemcpy(out->header_off, dv.d_header_off, ((size_t)dv.n + 1) * 8, hipMemcpyDeviceToHost));
    FA_HIP(hipMemcpy(out->base_off, dv.d_base_off, ((size_t)dv.n + 1) * 8, hipMemcpyDeviceToHost));
    cleanup();
    return CLS_OK;
}
