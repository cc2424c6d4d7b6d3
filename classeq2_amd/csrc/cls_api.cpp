// C-ABI of libclsplace.so (include/cls_place.h): handle management, upload,
// the host-buffer and device-buffer batch entry points.  Nothing unwinds across
// the boundary; every failure leaves a thread-local message for cls_last_error().
#include <hip/hip_runtime.h>
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cls_db.h"
#include "cls_device.h"
#include "cls_extract.h"
#include "cls_kernels.h"
#include "cls_pair.h"
#include "cls_place.h"
#include "cls_tally.h"
#include "cls_tuning.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define CLS_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(CLS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Workspace {
    uint32_t* ptr = nullptr;
    uint64_t words = 0;
    hipEvent_t done = nullptr;
    hipStream_t stream = nullptr;           // stream of the slot's last user: the next launch on the SAME stream is ordered
                                            // behind it and may take the slot at once
    uint64_t seq = 0;                       // acquisition counter (the oldest busy slot is the one to wait for)
    int launching = 0;                      // callers between acquire and their `done` record
    bool busy = false;
    bool recorded = false;                  // `done` has been recorded for the current user (until then the event still
                                            // shows the PREVIOUS launch as complete: the slot must not be reclaimed)
};
// HIP events around the dominant kernel of one launch (cls_db_kernel_time); pooled, independent of the scratch slots
struct TimedPair {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool pending = false;                   // recorded, not yet folded into the handle's accumulators
    bool in_use = false;                    // handed to a launch that has not recorded it yet (set and cleared under ws_mu)
};
constexpr size_t MAX_WS_SLOTS = 8;          // scratch slots per handle; beyond it a caller waits for the oldest launch
constexpr size_t MAX_TIMED_PAIRS = 256;     // launches in flight whose kernel time is still to be harvested

// Stream + device staging buffers of one host-buffer call, recycled across calls (a hipMalloc / hipFree / stream
// create per call cost milliseconds -- and hipFree synchronises the device, stalling every other caller).
struct CallSlot {
    hipStream_t stream = nullptr;
    void *d_bases = nullptr, *d_off = nullptr, *d_out = nullptr, *d_stats = nullptr;
    uint64_t cap_bytes = 0;
    uint32_t cap_reads = 0, cap_stats = 0;
    bool busy = false;
};

cls::PlaceParams resolve(const cls_params* p) {
    // place_sequence.rs:64-75
    cls::PlaceParams r;
    r.max_iterations = (p && (p->flags & CLS_HAS_MAX_ITERATIONS)) ? p->max_iterations : 1000;
    r.remove_intersection = (p && (p->flags & CLS_HAS_REMOVE_INTERSECTION)) ? (p->remove_intersection != 0) : 0;
    double c = 0.7;
    if (p && (p->flags & CLS_HAS_MIN_MATCH_COVERAGE)) {
        c = p->min_match_coverage;
        if (c > 1.0) c = 1.0; else if (c < 0.0) c = 0.0;
    }
    r.min_match_coverage = c;
    return r;
}

}  // namespace

struct cls_db {
    int device = 0;
    int n_cu = 0;
    cls::DbDev dev{};
    cls_db_info info{};
    void* d_nodes = nullptr;
    void* d_kids = nullptr;
    void* d_table = nullptr;
    void* d_postings = nullptr;
    void* d_postings2 = nullptr;
    void* d_bucket_key = nullptr;
    void* d_mz_bucket = nullptr;
    void* d_direct = nullptr;
    void* d_direct16 = nullptr;
    void* d_sets = nullptr;
    void* d_sets2 = nullptr;
    std::mutex ws_mu;
    uint64_t max_read_len = 0;  // what the device-buffer entry provisions its long-read slices for (0: none, reads of up to
                                // MAX_READ_KMERS k-mers only; cls_db_set_max_read_len opts in)
                                // (info.max_read_kmers is not kept: cls_db_info_get takes it from the plan, device_plan)
    double kernel_ms_sum = 0.0;
    uint64_t kernel_launches = 0;
    std::vector<Workspace> ws;  // per-call scratch (class lists, child counters), recycled once their launch has finished
    std::vector<TimedPair> timed;
    uint64_t ws_seq = 0;
    std::vector<CallSlot> calls;  // host-buffer calls: stream + staging buffers (ws_mu)
    struct TreeRow { uint64_t id; uint32_t pre, size; };
    std::vector<TreeRow> tree_rows;  // per row of the descriptor's node table (the clade tally reports in that order)
};

// ---- experiment knobs (csrc/cls_tuning.h) ------------------------------------------------------------------
namespace cls {
Tuning& tuning() {
    static Tuning t;
    return t;
}
}  // namespace cls
namespace {
struct Knob { const char* name; int cls::Tuning::*field; };
const Knob KNOBS[] = {
    {"no_fast", &cls::Tuning::no_fast}, {"no_order", &cls::Tuning::no_order}, {"force_list", &cls::Tuning::force_list},
    {"no_mask_halves", &cls::Tuning::no_mask_halves}, {"no_fat_direct", &cls::Tuning::no_fat_direct}, {"no_tile", &cls::Tuning::no_tile}, {"tile_pass_codes", &cls::Tuning::tile_pass_codes}, {"tile_set_words", &cls::Tuning::tile_set_words}, {"time_class", &cls::Tuning::time_class}, {"tile_one_per_cu", &cls::Tuning::tile_one_per_cu}, {"tile_min_kmers", &cls::Tuning::tile_min_kmers}, {"no_tile_order", &cls::Tuning::no_tile_order}, {"tile_deal", &cls::Tuning::tile_deal}, {"blocks_per_cu", &cls::Tuning::blocks_per_cu}, {"key_blocks_per_cu", &cls::Tuning::key_blocks_per_cu},
    {"long_blocks_per_cu", &cls::Tuning::long_blocks_per_cu}, {"order_mode", &cls::Tuning::order_mode},
    {"order_windows", &cls::Tuning::order_windows}, {"order_both_strands", &cls::Tuning::order_both_strands},
    {"order_block_shift", &cls::Tuning::order_block_shift}, {"order_sample_shift", &cls::Tuning::order_sample_shift},
    {"profile_stop", &cls::Tuning::profile_stop}, {"timing", &cls::Tuning::timing},
    {"build_full_key", &cls::Tuning::build_full_key}, {"tally_no_wave_combine", &cls::Tuning::tally_no_wave_combine},
};
}  // namespace

extern "C" int cls_set_tuning(const char* name, int value) {
    if (!name) return fail(CLS_E_INVALID_ARG, "cls_set_tuning: null name");
    for (const Knob& k : KNOBS)
        if (strcmp(k.name, name) == 0) { cls::tuning().*(k.field) = value; return CLS_OK; }
    return fail(CLS_E_INVALID_ARG, std::string("cls_set_tuning: unknown knob ") + name);
}

extern "C" void cls_tuning_from_env(void) {
    for (const Knob& k : KNOBS) {
        std::string var = "CLS_";
        for (const char* c = k.name; *c; ++c) var += (char)toupper((unsigned char)*c);
        if (const char* v = getenv(var.c_str())) cls::tuning().*(k.field) = *v ? atoi(v) : 1;  // (an empty value means "on")
    }
}

extern "C" const char* cls_last_error(void) { return g_err.c_str(); }
extern "C" void cls_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }  // for the library's other translation units

extern "C" const char* cls_version(void) { return "classeq2_amd 0.1.0 gfx950 abi1"; }

extern "C" int cls_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void cls_db_destroy(cls_db* db) {
    if (!db) return;
    int prev = 0;
    bool have_prev = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(db->device);
    for (auto& w : db->ws) {
        if (w.done) { if (w.recorded) (void)hipEventSynchronize(w.done); (void)hipEventDestroy(w.done); }
        if (w.ptr) (void)hipFree(w.ptr);
    }
    for (auto& t : db->timed) {
        if (t.t0) (void)hipEventDestroy(t.t0);
        if (t.t1) (void)hipEventDestroy(t.t1);
    }
    for (auto& c : db->calls) {
        if (c.stream) { (void)hipStreamSynchronize(c.stream); (void)hipStreamDestroy(c.stream); }
        for (void* p : {c.d_bases, c.d_off, c.d_out, c.d_stats}) if (p) (void)hipFree(p);
    }
    if (db->d_nodes) (void)hipFree(db->d_nodes);
    if (db->d_kids) (void)hipFree(db->d_kids);
    if (db->d_table) (void)hipFree(db->d_table);
    if (db->d_postings) (void)hipFree(db->d_postings);
    if (db->d_postings2) (void)hipFree(db->d_postings2);
    if (db->d_bucket_key) (void)hipFree(db->d_bucket_key);
    if (db->d_mz_bucket) (void)hipFree(db->d_mz_bucket);
    if (db->d_direct) (void)hipFree(db->d_direct);
    if (db->d_direct16) (void)hipFree(db->d_direct16);
    if (db->d_sets) (void)hipFree(db->d_sets);
    if (db->d_sets2) (void)hipFree(db->d_sets2);
    if (have_prev) (void)hipSetDevice(prev);
    delete db;
}

// Validation + re-encoding of a descriptor, for cls_db_create and cls_db_group_create (`who`: the entry's name).
static int encode(const cls_db_desc* d, cls::EncodedDb& E, const char* who) {
    std::string err;
    int rc = cls::encode_db(d, E, err);
    if (rc != CLS_OK) return fail(rc, std::string(who) + ": " + err);
    if (E.format == cls::FMT_LIST && E.postings.size() >= (1ULL << 32)) return fail(CLS_E_BAD_DB, std::string(who) + ": sorted-list postings exceed 2^32 words");
    return CLS_OK;
}

// The device half of cls_db_create: an encoded index -> a handle on `device` (-1: the current device).  `n_buckets`:
// the descriptor's, for cls_db_info.  Leaves `device` current on the calling thread.  May throw std::bad_alloc.
static int upload(const cls::EncodedDb& E, uint32_t n_buckets, int device, cls_db** out) {
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return fail(CLS_E_NO_DEVICE, "cls_db_create: no HIP device is visible (the placement path has no CPU fallback)");
    if (device < 0) CLS_HIP(hipGetDevice(&device));
    if (device >= n_dev) return fail(CLS_E_INVALID_ARG, "cls_db_create: device ordinal out of range");
    CLS_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    CLS_HIP(hipGetDeviceProperties(&prop, device));
    std::vector<cls_db::TreeRow> tree_rows(E.nodes.size());
    for (size_t r = 0; r < E.nodes.size(); ++r) tree_rows[E.desc_row[r]] = {E.nodes[r].id, E.nodes[r].pre, E.nodes[r].size};
    cls_db* db = new cls_db();
    db->device = device;
    db->n_cu = prop.multiProcessorCount;
    db->tree_rows = std::move(tree_rows);
    auto up = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, bytes + 64);  // (tail pad: the kernels read node records in pairs and 16-byte entries speculatively)
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e;
    if ((e = up(&db->d_nodes, E.nodes.data(), E.nodes.size() * sizeof(cls::DNode))) != hipSuccess ||
        (e = up(&db->d_kids, E.kids.data(), E.kids.size() * 4)) != hipSuccess ||
        (e = up(&db->d_table, E.table.data(), E.table.size() * sizeof(cls::Slot))) != hipSuccess ||
        (e = up(&db->d_postings, E.postings.data(), E.postings.size() * 4)) != hipSuccess ||
        (!E.postings2.empty() && (e = up(&db->d_postings2, E.postings2.data(), E.postings2.size() * 4)) != hipSuccess) ||
        (e = up(&db->d_bucket_key, E.bucket_key.data(), E.bucket_key.size() * 8)) != hipSuccess ||
        (!E.mz_bucket.empty() && (e = up(&db->d_mz_bucket, E.mz_bucket.data(), E.mz_bucket.size() * 4)) != hipSuccess) ||
        (!E.direct.empty() && (e = up(&db->d_direct, E.direct.data(), E.direct.size() * 4)) != hipSuccess) ||
        (!E.direct16.empty() && (e = up(&db->d_direct16, E.direct16.data(), E.direct16.size() * 4)) != hipSuccess) ||
        (!E.sets.empty() && (e = up(&db->d_sets, E.sets.data(), E.sets.size() * sizeof(cls::SetRec))) != hipSuccess) ||
        (!E.sets2.empty() && (e = up(&db->d_sets2, E.sets2.data(), E.sets2.size() * sizeof(cls::SetRec))) != hipSuccess)) {
        cls_db_destroy(db);
        return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_db_create: upload failed: ") + hipGetErrorString(e));
    }
    cls::DbDev& v = db->dev;
    v.nodes = (const cls::DNode*)db->d_nodes;
    v.kids = (const uint32_t*)db->d_kids;
    v.table = (const cls::Slot*)db->d_table;
    v.postings = (const uint32_t*)db->d_postings;
    v.postings2 = (const uint32_t*)db->d_postings2;
    v.bucket_key = (const uint64_t*)db->d_bucket_key;
    v.mz_bucket = (const uint32_t*)db->d_mz_bucket;
    v.direct = (const uint32_t*)db->d_direct;
    v.direct16 = (const uint32_t*)db->d_direct16;
    v.sets = (const cls::SetRec*)db->d_sets;
    v.sets2 = (const cls::SetRec*)db->d_sets2;
    v.table_mask = E.table.size() - 1;
    v.n_nodes = (uint32_t)E.nodes.size();
    v.n_buckets = (uint32_t)E.bucket_key.size();
    v.k = E.k;
    v.m_eff = E.m_eff;
    v.max_nonleaf_arity = E.max_nonleaf_arity;
    v.format = E.format;
    v.binary_tree = E.strictly_binary ? 1u : 0u;
    v.canonical = E.canonical ? 1u : 0u;
    v.n_sets = (uint32_t)E.sets.size();
    v.set_bits = 1;
    while (v.set_bits < 32 && (1ull << v.set_bits) < (uint64_t)E.sets.size()) ++v.set_bits;
    v.addr32 = (E.postings.size() * 4 < (1ull << 32) && E.direct.size() * 4 < (1ull << 32) && E.sets.size() * sizeof(cls::SetRec) < (1ull << 32)) ? 1u : 0u;
    cls_db_info& i = db->info;
    i.n_nodes = v.n_nodes;
    i.max_depth = E.max_depth;
    i.max_nonleaf_arity = E.max_nonleaf_arity;
    i.k_size = E.k;
    i.m_size = E.m;
    i.n_buckets = n_buckets;
    i.n_kmers = E.n_kmers;
    i.n_closed_kmers = E.n_closed;
    i.table_slots = E.table.size();
    i.postings_words = E.postings.size();
    i.hbm_bytes = E.nodes.size() * sizeof(cls::DNode) + E.table.size() * sizeof(cls::Slot) + (E.postings.size() + E.postings2.size()) * 4 + E.bucket_key.size() * 8 + E.mz_bucket.size() * 4 + E.direct.size() * 4 + E.direct16.size() * 4 + (E.sets.size() + E.sets2.size()) * sizeof(cls::SetRec);
    i.device = device;
    i.format = E.format;
    i.binary_tree = E.strictly_binary ? 1u : 0u;
    i.direct_table = E.direct.empty() ? 0u : (E.canonical ? 2u : 1u);
    i.n_tip_sets = (uint32_t)E.n_sets;
    i.fat_direct_table = E.direct16.empty() ? 0u : 1u;
    *out = db;
    return CLS_OK;
}

extern "C" int cls_db_create(const cls_db_desc* d, int device, cls_db** out) {
    if (!out) return fail(CLS_E_INVALID_ARG, "cls_db_create: out is null");
    *out = nullptr;
    try {
        cls::EncodedDb E;
        int rc = encode(d, E, "cls_db_create");
        if (rc != CLS_OK) return rc;
        return upload(E, (uint32_t)d->n_buckets, device, out);
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_db_create: out of host memory");
    } catch (const std::exception& ex) {
        return fail(CLS_E_INTERNAL, std::string("cls_db_create: ") + ex.what());
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_db_create: unknown exception");
    }
}

extern "C" int cls_db_validate(const cls_db_desc* d) {
    try {
        cls::EncodedDb E;
        std::string err;
        int rc = cls::encode_db(d, E, err);
        if (rc != CLS_OK) return fail(rc, "cls_db_validate: " + err);
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_db_validate: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_db_validate: unknown exception");
    }
}

// The plan cls_place_batch_device() makes for reads of up to n_bases bases (0: its default, reads of up to MAX_READ_KMERS
// k-mers); the host-buffer entries plan each chunk the same way from its longest read.  The class limits and the kernel
// instances do not depend on the batch size.
static cls::PlacePlan device_plan(const cls_db* db, uint64_t n_bases, bool stats) {
    return cls::plan_place(db->dev, 4096, (uint32_t)db->n_cu, stats, (uint32_t)(2 * n_bases), n_bases ? 4096 : 0);
}

static uint64_t declared_read_len(const cls_db* db) {
    std::lock_guard<std::mutex> g(const_cast<cls_db*>(db)->ws_mu);
    return db->max_read_len;
}

extern "C" int cls_db_info_get(const cls_db* db, cls_db_info* info) {
    if (!db || !info) return fail(CLS_E_INVALID_ARG, "cls_db_info_get: null argument");
    try {
        // the largest read the device-buffer entry's plan places, as it would launch now (declared read length, knobs)
        uint32_t cap[cls::N_LISTS];
        device_plan(db, declared_read_len(db), false).class_caps(cap);
        cls_db* mdb = const_cast<cls_db*>(db);
        std::lock_guard<std::mutex> g(mdb->ws_mu);
        *info = db->info;
        info->scratch_slots = (uint32_t)db->ws.size();
        info->max_read_kmers = *std::max_element(cap, cap + cls::N_LISTS);
        return CLS_OK;
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_db_info_get: unknown exception");
    }
}

extern "C" int cls_db_info_get2(const cls_db* db, void* info, size_t info_size) {
    if (!db || !info) return fail(CLS_E_INVALID_ARG, "cls_db_info_get2: null argument");
    cls_db_info full;
    const int rc = cls_db_info_get(db, &full);
    if (rc != CLS_OK) return rc;
    memcpy(info, &full, info_size < sizeof(full) ? info_size : sizeof(full));
    return CLS_OK;
}

// fold finished kernel timings into the handle's accumulators (ws_mu held); `wait`: also those still running
static void harvest(cls_db* db, bool wait) {
    for (auto& t : db->timed) {
        if (!t.pending) continue;
        if (wait ? hipEventSynchronize(t.t1) != hipSuccess : hipEventQuery(t.t1) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.t0, t.t1) == hipSuccess) { db->kernel_ms_sum += ms; db->kernel_launches++; }
        t.pending = false;
    }
}

// An event pair for one launch's dominant kernel (ws_mu held); SIZE_MAX: none free, the launch goes untimed.
static size_t acquire_timed(cls_db* db) {
    harvest(db, false);
    for (size_t i = 0; i < db->timed.size(); ++i)
        if (!db->timed[i].pending && !db->timed[i].in_use && db->timed[i].t0) { db->timed[i].in_use = true; return i; }
    if (db->timed.size() >= MAX_TIMED_PAIRS) return SIZE_MAX;
    TimedPair t;
    if (hipEventCreate(&t.t0) != hipSuccess) return SIZE_MAX;
    if (hipEventCreate(&t.t1) != hipSuccess) { (void)hipEventDestroy(t.t0); return SIZE_MAX; }
    t.in_use = true;
    db->timed.push_back(t);
    return db->timed.size() - 1;
}

// Take a scratch workspace for a launch on `stream`:
//  * a slot whose last user ran on the SAME stream is taken at once (stream order makes the reuse safe), so a caller
//    that pipelines many batches on one stream keeps ONE slot however far ahead of the device it runs;
//  * else a slot whose launch has finished;
//  * else a new one, up to MAX_WS_SLOTS; beyond that the caller waits for the oldest launch in flight.
// Idle slots that are too small are freed before a larger one is allocated.
// `*use` = a copy of the slot taken under the lock: the vector may grow (and move) while the caller launches.
static int acquire_ws(cls_db* db, uint64_t words, hipStream_t stream, size_t* slot, Workspace* use) {
    std::unique_lock<std::mutex> g(db->ws_mu);
    for (;;) {
        size_t oldest = SIZE_MAX;
        for (size_t i = 0; i < db->ws.size(); ++i) {
            Workspace& w = db->ws[i];
            if (w.busy && w.recorded && w.launching == 0 && hipEventQuery(w.done) == hipSuccess) w.busy = false;
            // (hipStreamPerThread is ONE handle value that names a different stream in every host thread: never a "same stream")
            const bool same_stream = w.busy && w.recorded && w.launching == 0 && w.stream == stream && stream != hipStreamPerThread;
            if ((!w.busy || same_stream) && w.words >= words) {
                w.busy = true; w.recorded = false; w.launching = 1; w.stream = stream; w.seq = ++db->ws_seq;
                *slot = i; *use = w;
                return CLS_OK;
            }
            if (w.busy && w.recorded && w.launching == 0 && (oldest == SIZE_MAX || w.seq < db->ws[oldest].seq)) oldest = i;
        }
        // nothing fits: drop idle slots (they are too small), then grow or wait
        for (size_t i = 0; i < db->ws.size();) {
            Workspace& w = db->ws[i];
            if (!w.busy) {
                (void)hipEventDestroy(w.done);
                (void)hipFree(w.ptr);
                db->ws.erase(db->ws.begin() + (ptrdiff_t)i);
                oldest = SIZE_MAX;  // (indices moved: recomputed on the next round if needed)
            } else ++i;
        }
        if (db->ws.size() < MAX_WS_SLOTS) break;
        if (oldest == SIZE_MAX) {
            for (size_t i = 0; i < db->ws.size(); ++i)
                if (db->ws[i].busy && db->ws[i].recorded && db->ws[i].launching == 0 && (oldest == SIZE_MAX || db->ws[i].seq < db->ws[oldest].seq)) oldest = i;
        }
        if (oldest == SIZE_MAX) {  // every slot is between acquire and record on another thread: let them get on
            g.unlock();
            std::this_thread::yield();
            g.lock();
            continue;
        }
        hipEvent_t ev = db->ws[oldest].done;
        g.unlock();
        if (hipEventSynchronize(ev) != hipSuccess) return fail(CLS_E_HIP, "hipEventSynchronize failed while waiting for a scratch slot");
        g.lock();
    }
    Workspace w;
    if (hipMalloc((void**)&w.ptr, words * 4) != hipSuccess) return fail(CLS_E_NOMEM, "scratch workspace allocation failed");
    if (hipEventCreateWithFlags(&w.done, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(w.ptr);
        return fail(CLS_E_HIP, "hipEventCreate failed");
    }
    w.words = words;
    w.busy = true;
    w.recorded = false;
    w.launching = 1;
    w.stream = stream;
    w.seq = ++db->ws_seq;
    db->ws.push_back(w);
    *slot = db->ws.size() - 1;
    *use = w;
    return CLS_OK;
}

// Longest read (bases) any kernel is provisioned for: 2^25 bases = 2^26 k-mers per read.
static constexpr uint64_t HARD_MAX_READ_LEN = 1ull << 25;

extern "C" int cls_db_set_max_read_len(cls_db* db, uint64_t n_bases) {
    if (!db) return fail(CLS_E_INVALID_ARG, "cls_db_set_max_read_len: null handle");
    if (n_bases > HARD_MAX_READ_LEN) return fail(CLS_E_INVALID_ARG, "cls_db_set_max_read_len: at most 2^25 bases per read");
    std::lock_guard<std::mutex> g(db->ws_mu);
    db->max_read_len = n_bases;
    return CLS_OK;
}

// `long_cap` = k-mers per read to provision beyond the register-resident kernels (0: none), `n_long` = how many
// such reads the batch can hold at most.
static int place_device(cls_db* db, const void* d_bases, const void* d_offsets, uint32_t n, const cls_params* params,
                        void* d_out, void* d_stats, hipStream_t stream, uint32_t long_cap, uint32_t n_long) {
    const cls::PlaceParams prm = resolve(params);
    const cls::PlacePlan plan = cls::plan_place(db->dev, n, (uint32_t)db->n_cu, d_stats != nullptr, long_cap, n_long);
    size_t slot = 0;
    Workspace use;
    int rc = acquire_ws(db, (plan.ws_bytes + 3) / 4, stream, &slot, &use);
    if (rc != CLS_OK) return rc;
    size_t tp = SIZE_MAX;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    {
        std::lock_guard<std::mutex> g(db->ws_mu);
        tp = acquire_timed(db);
        if (tp != SIZE_MAX) { t0 = db->timed[tp].t0; t1 = db->timed[tp].t1; }
    }
    hipError_t e = cls::launch_place(db->dev, prm, plan, (const uint8_t*)d_bases, (const uint64_t*)d_offsets, n,
                                     (cls_placement*)d_out, (cls_query_stats*)d_stats, use.ptr, stream, t0, t1);
    bool record_failed = false;
    {
        std::lock_guard<std::mutex> g(db->ws_mu);
        if (tp != SIZE_MAX) { db->timed[tp].pending = (e == hipSuccess); db->timed[tp].in_use = false; }
        // (another thread may have grown the vector meanwhile; slots are only erased while idle, never this one)
        for (size_t i = 0; i < db->ws.size(); ++i)
            if (db->ws[i].ptr == use.ptr) { slot = i; break; }
        record_failed = hipEventRecord(db->ws[slot].done, stream) != hipSuccess;
    }
    if (record_failed) (void)hipStreamSynchronize(stream);  // the kernels may still be running: drain before the slot is handed on
    {
        std::lock_guard<std::mutex> g(db->ws_mu);
        for (size_t i = 0; i < db->ws.size(); ++i)
            if (db->ws[i].ptr == use.ptr) { slot = i; break; }
        db->ws[slot].launching = 0;
        db->ws[slot].recorded = !record_failed;
        if (record_failed) db->ws[slot].busy = false;
    }
    if (e != hipSuccess) return fail(CLS_E_HIP, std::string("kernel launch failed: ") + hipGetErrorString(e));
    return CLS_OK;
}

extern "C" int cls_place_batch_device(cls_db* db, const void* d_bases, const void* d_offsets, uint32_t n,
                                      const cls_params* params, void* d_out, void* d_stats, void* hip_stream) {
    if (!db) return fail(CLS_E_INVALID_ARG, "cls_place_batch_device: null handle");
    if (n == 0) return CLS_OK;
    if (!d_offsets || !d_out) return fail(CLS_E_INVALID_ARG, "cls_place_batch_device: null buffer");
    // the handle's device must be current for the scratch allocation, the events and the launches
    int prev = 0;
    CLS_HIP(hipGetDevice(&prev));
    if (prev != db->device) CLS_HIP(hipSetDevice(db->device));
    int rc;
    try {
        uint64_t max_len;
        { std::lock_guard<std::mutex> g(db->ws_mu); max_len = db->max_read_len; }
        // the read lengths are only known on the device: provision for the handle's limit (0: the register-resident
        // kernels only -- the long-read slices are provisioned when the caller opts in, cls_db_set_max_read_len)
        rc = place_device(db, d_bases, d_offsets, n, params, d_out, d_stats, (hipStream_t)hip_stream, (uint32_t)(2 * max_len), max_len ? n : 0);
    } catch (...) {
        rc = fail(CLS_E_INTERNAL, "cls_place_batch_device: unknown exception");
    }
    if (prev != db->device) (void)hipSetDevice(prev);
    return rc;
}

extern "C" int cls_db_kernel_name(const cls_db* db, char* buf, size_t len) {
    if (!db || !buf || !len) return fail(CLS_E_INVALID_ARG, "cls_db_kernel_name: null argument");
    try {
        snprintf(buf, len, "%s", device_plan(db, declared_read_len(db), false).timed_name.c_str());
        return CLS_OK;
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_db_kernel_name: unknown exception");
    }
}

extern "C" int cls_db_read_classes(const cls_db* db, uint64_t n_bases, int stats, cls_read_class* out, int max, int* n_out) {
    if (!db || !n_out || max < 0 || (max > 0 && !out)) return fail(CLS_E_INVALID_ARG, "cls_db_read_classes: null argument");
    if (n_bases > HARD_MAX_READ_LEN) return fail(CLS_E_INVALID_ARG, "cls_db_read_classes: at most 2^25 bases per read");
    try {
        const cls::PlacePlan plan = device_plan(db, n_bases, stats != 0);
        uint32_t cap[cls::N_LISTS];
        plan.class_caps(cap);
        // a list takes the reads above every earlier list's limit and up to its own (classify_kernel): those with none are left out
        int n = 0;
        uint32_t below = 0;
        for (int c = 0; c < cls::N_LISTS; ++c) {
            if (c > 0 && cap[c] <= below) continue;
            below = cap[c];
            if (n < max) {
                out[n].list = (uint32_t)c;
                out[n].max_kmers = cap[c];
                snprintf(out[n].kernel, sizeof out[n].kernel, "%s", plan.class_kernel_name(db->dev, c, stats != 0).c_str());
            }
            ++n;
        }
        *n_out = n;
        return CLS_OK;
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_db_read_classes: unknown exception");
    }
}

extern "C" int cls_db_kernel_time(cls_db* db, double* sum_ms, uint64_t* launches, int reset) {
    if (!db) return fail(CLS_E_INVALID_ARG, "cls_db_kernel_time: null handle");
    std::lock_guard<std::mutex> g(db->ws_mu);
    harvest(db, true);
    if (sum_ms) *sum_ms = db->kernel_ms_sum;
    if (launches) *launches = db->kernel_launches;
    if (reset) { db->kernel_ms_sum = 0.0; db->kernel_launches = 0; }
    return CLS_OK;
}

// The buffer checks of the host-buffer entries (n > 0).
static int check_host_args(const char* bases, const uint64_t* offsets, uint32_t n, const cls_placement* out) {
    if (!offsets || !out || (!bases && offsets[n] != offsets[0])) return fail(CLS_E_INVALID_ARG, "cls_place_batch: null buffer");
    for (uint32_t i = 0; i < n; ++i)
        if (offsets[i] > offsets[i + 1]) return fail(CLS_E_INVALID_ARG, "cls_place_batch: offsets not monotone");
    return CLS_OK;
}

static int place_host_checked(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n, const cls_params* params,
                              cls_placement* out, cls_query_stats* stats);

static int place_host(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n, const cls_params* params,
                      cls_placement* out, cls_query_stats* stats) {
    if (!db) return fail(CLS_E_INVALID_ARG, "cls_place_batch: null handle");
    if (n == 0) return CLS_OK;
    const int rc = check_host_args(bases, offsets, n, out);
    if (rc != CLS_OK) return rc;
    return place_host_checked(db, bases, offsets, n, params, out, stats);
}

// place_host once its arguments are checked (n > 0); saves and restores the calling thread's current device.
static int place_host_checked(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n, const cls_params* params,
                              cls_placement* out, cls_query_stats* stats) {
    int prev = 0;
    CLS_HIP(hipGetDevice(&prev));
    CLS_HIP(hipSetDevice(db->device));
    // Large batches go through in chunks on TWO call slots (stream + grow-only staging buffers from the handle's pool):
    // the copy-in of chunk i+1 and the copy-out of chunk i-1 overlap the kernels of chunk i.
    const uint32_t chunk_reads = 256u << 10;       // reads per chunk (each chunk is still ordered as a whole: >= 4096 reads)
    const uint64_t chunk_bytes = 256ull << 20;     // bases per chunk
    const bool two = n > chunk_reads || offsets[n] - offsets[0] > chunk_bytes;
    size_t ci[2] = {0, 0};
    CallSlot cs[2];
    const int n_slots = two ? 2 : 1;
    {
        std::lock_guard<std::mutex> g(db->ws_mu);
        for (int k = 0; k < n_slots; ++k) {
            size_t i = 0;
            while (i < db->calls.size() && db->calls[i].busy) ++i;
            if (i == db->calls.size()) db->calls.emplace_back();
            db->calls[i].busy = true;
            ci[k] = i;
            cs[k] = db->calls[i];
        }
    }
    auto cleanup = [&]() {  // drain, then hand the slots (with whatever they have grown to) back
        for (int k = 0; k < n_slots; ++k) if (cs[k].stream) (void)hipStreamSynchronize(cs[k].stream);
        std::lock_guard<std::mutex> g(db->ws_mu);
        for (int k = 0; k < n_slots; ++k) { cs[k].busy = false; db->calls[ci[k]] = cs[k]; }
        (void)hipSetDevice(prev);
    };
#define CLS_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
    } while (0)
    try {
        std::vector<uint64_t> rel[2];
        struct Pending { bool on = false; uint32_t first = 0, cnt = 0; } pend[2];
        auto copy_out = [&](int k) -> hipError_t {  // records (and counters) of the chunk slot k last ran
            if (!pend[k].on) return hipSuccess;
            pend[k].on = false;
            hipError_t e = hipMemcpyAsync(out + pend[k].first, cs[k].d_out, (size_t)pend[k].cnt * sizeof(cls_placement), hipMemcpyDeviceToHost, cs[k].stream);
            if (e == hipSuccess && stats)
                e = hipMemcpyAsync(stats + pend[k].first, cs[k].d_stats, (size_t)pend[k].cnt * sizeof(cls_query_stats), hipMemcpyDeviceToHost, cs[k].stream);
            return e;
        };
        int turn = 0;
        for (uint32_t first = 0; first < n; turn ^= (n_slots - 1)) {
            CallSlot& c = cs[turn];
            uint32_t cnt = 0;
            while (first + cnt < n && cnt < chunk_reads && (cnt == 0 || offsets[first + cnt + 1] - offsets[first] <= chunk_bytes)) ++cnt;
            const uint64_t nbytes = offsets[first + cnt] - offsets[first];
            CLS_TRY(copy_out(turn));  // the slot's previous chunk leaves before its buffers are reused (stream order)
            if (!c.stream) CLS_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
            if (nbytes > c.cap_bytes || !c.d_bases) {
                CLS_TRY(hipStreamSynchronize(c.stream));
                if (c.d_bases) { (void)hipFree(c.d_bases); c.d_bases = nullptr; c.cap_bytes = 0; }
                const uint64_t want = std::max<uint64_t>(nbytes + nbytes / 4, 1 << 16);  // (some slack: jobs of similar size reuse it)
                CLS_TRY(hipMalloc(&c.d_bases, want));
                c.cap_bytes = want;
            }
            if (cnt > c.cap_reads) {
                CLS_TRY(hipStreamSynchronize(c.stream));
                for (void** pp : {&c.d_off, &c.d_out, &c.d_stats}) if (*pp) { (void)hipFree(*pp); *pp = nullptr; }
                c.cap_reads = c.cap_stats = 0;
                const uint32_t want = (uint32_t)std::max<uint64_t>((uint64_t)cnt + cnt / 4, 1024);
                CLS_TRY(hipMalloc(&c.d_off, ((size_t)want + 1) * 8));
                CLS_TRY(hipMalloc(&c.d_out, (size_t)want * sizeof(cls_placement)));
                c.cap_reads = want;
            }
            if (stats && c.cap_stats < c.cap_reads) {
                CLS_TRY(hipStreamSynchronize(c.stream));
                if (c.d_stats) { (void)hipFree(c.d_stats); c.d_stats = nullptr; }
                CLS_TRY(hipMalloc(&c.d_stats, (size_t)c.cap_reads * sizeof(cls_query_stats)));
                c.cap_stats = c.cap_reads;
            }
            std::vector<uint64_t>& ro = rel[turn];
            ro.resize((size_t)cnt + 1);
            for (uint32_t i = 0; i <= cnt; ++i) ro[i] = offsets[first + i] - offsets[first];
            // provision exactly what this chunk needs: the classes beyond its longest read are not launched
            uint64_t longest = 1;
            uint32_t n_long = 1;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint64_t len = ro[i + 1] - ro[i];
                const uint64_t nk = len < db->dev.k ? 0 : 2 * (len - db->dev.k + 1);
                longest = std::max(longest, std::min(len, HARD_MAX_READ_LEN));
                if (nk > cls::MAX_READ_KMERS) ++n_long;
            }
            if (nbytes) CLS_TRY(hipMemcpyAsync(c.d_bases, bases + offsets[first], nbytes, hipMemcpyHostToDevice, c.stream));
            CLS_TRY(hipMemcpyAsync(c.d_off, ro.data(), ((size_t)cnt + 1) * 8, hipMemcpyHostToDevice, c.stream));
            const int rc = place_device(db, c.d_bases, c.d_off, cnt, params, c.d_out, stats ? c.d_stats : nullptr, c.stream, (uint32_t)(2 * longest), n_long);
            if (rc != CLS_OK) { cleanup(); return rc; }
            pend[turn].on = true;
            pend[turn].first = first;
            pend[turn].cnt = cnt;
            first += cnt;
            // while this chunk computes, bring the other slot's finished records home
            if (n_slots == 2) CLS_TRY(copy_out(turn ^ 1));
        }
        for (int k = 0; k < n_slots; ++k) CLS_TRY(copy_out(k));
        for (int k = 0; k < n_slots; ++k) CLS_TRY(hipStreamSynchronize(cs[k].stream));
    } catch (const std::bad_alloc&) {
        cleanup();
        return fail(CLS_E_NOMEM, "cls_place_batch: out of host memory");
    } catch (...) {
        cleanup();
        return fail(CLS_E_INTERNAL, "cls_place_batch: unknown exception");
    }
    cleanup();
    return CLS_OK;
#undef CLS_TRY
}

extern "C" int cls_place_batch(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n,
                               const cls_params* params, cls_placement* out) {
    return place_host(db, bases, offsets, n, params, out, nullptr);
}

extern "C" int cls_place_batch_stats(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n,
                                     const cls_params* params, cls_placement* out, cls_query_stats* stats) {
    if (!stats) return fail(CLS_E_INVALID_ARG, "cls_place_batch_stats: stats is null");
    return place_host(db, bases, offsets, n, params, out, stats);
}

// ---- index groups: one index encoded once, uploaded to several devices --------------------------------------------

struct cls_db_group {
    std::vector<cls_db*> replicas;  // replica i lives on devices[i]
    std::vector<int> devices;
};

extern "C" void cls_db_group_destroy(cls_db_group* g) {
    if (!g) return;
    for (cls_db* db : g->replicas) cls_db_destroy(db);
    delete g;
}

extern "C" int cls_db_group_create(const cls_db_desc* d, const int* devices, uint32_t n_devices, cls_db_group** out) {
    if (!out) return fail(CLS_E_INVALID_ARG, "cls_db_group_create: out is null");
    *out = nullptr;
    cls_db_group* g = nullptr;
    try {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
            return fail(CLS_E_NO_DEVICE, "cls_db_group_create: no HIP device is visible (the placement path has no CPU fallback)");
        std::vector<int> devs;
        if (!devices || n_devices == 0) {
            for (int i = 0; i < n_dev; ++i) devs.push_back(i);
        } else {
            for (uint32_t i = 0; i < n_devices; ++i) {
                if (devices[i] < 0 || devices[i] >= n_dev)
                    return fail(CLS_E_INVALID_ARG, "cls_db_group_create: device ordinal " + std::to_string(devices[i]) + " out of range (" +
                                                       std::to_string(n_dev) + " visible)");
                devs.push_back(devices[i]);
            }
        }
        cls::EncodedDb E;
        int rc = encode(d, E, "cls_db_group_create");
        if (rc != CLS_OK) return rc;
        const size_t n = devs.size();
        g = new cls_db_group();
        g->devices = devs;
        g->replicas.assign(n, nullptr);
        // one host thread per replica: the copies to the devices overlap, and the caller's current device is untouched
        std::vector<int> rcs(n, CLS_E_INTERNAL);
        std::vector<std::string> msgs(n, "upload thread not started");
        auto work = [&](size_t i) {
            try {
                rcs[i] = upload(E, (uint32_t)d->n_buckets, devs[i], &g->replicas[i]);
                if (rcs[i] != CLS_OK) msgs[i] = g_err;
            } catch (const std::bad_alloc&) {
                rcs[i] = CLS_E_NOMEM;
                msgs[i] = "out of host memory";
            } catch (...) {
                rcs[i] = CLS_E_INTERNAL;
                msgs[i] = "unknown exception";
            }
        };
        std::vector<std::thread> th;
        try {
            for (size_t i = 0; i < n; ++i) th.emplace_back(work, i);
        } catch (...) {  // (a thread that could not be started leaves its replica's error in place)
        }
        for (auto& t : th) t.join();
        for (size_t i = 0; i < n; ++i) {
            if (rcs[i] == CLS_OK) continue;
            const std::string m = "cls_db_group_create: replica " + std::to_string(i) + " (device " + std::to_string(devs[i]) + "): " + msgs[i];
            rc = rcs[i];
            cls_db_group_destroy(g);
            return fail(rc, m);
        }
        *out = g;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_db_group_destroy(g);
        return fail(CLS_E_NOMEM, "cls_db_group_create: out of host memory");
    } catch (const std::exception& ex) {
        cls_db_group_destroy(g);
        return fail(CLS_E_INTERNAL, std::string("cls_db_group_create: ") + ex.what());
    } catch (...) {
        cls_db_group_destroy(g);
        return fail(CLS_E_INTERNAL, "cls_db_group_create: unknown exception");
    }
}

extern "C" int cls_db_group_size(const cls_db_group* g, uint32_t* n) {
    if (!g || !n) return fail(CLS_E_INVALID_ARG, "cls_db_group_size: null argument");
    *n = (uint32_t)g->replicas.size();
    return CLS_OK;
}

extern "C" int cls_db_group_replica(cls_db_group* g, uint32_t i, cls_db** db) {
    if (!g || !db) return fail(CLS_E_INVALID_ARG, "cls_db_group_replica: null argument");
    if (i >= g->replicas.size()) return fail(CLS_E_INVALID_ARG, "cls_db_group_replica: replica index out of range");
    *db = g->replicas[i];
    return CLS_OK;
}

extern "C" int cls_place_batch_group(cls_db_group* g, const char* bases, const uint64_t* offsets, uint32_t n,
                                     const cls_params* params, cls_placement* out, cls_query_stats* stats) {
    if (!g) return fail(CLS_E_INVALID_ARG, "cls_place_batch_group: null handle");
    if (n == 0) return CLS_OK;
    int rc = check_host_args(bases, offsets, n, out);
    if (rc != CLS_OK) return rc;
    try {
        // min(G, n) contiguous shards of about equal weight (bases + 1 per read: empty reads count too)
        const uint32_t n_shards = (uint32_t)std::min<size_t>(g->replicas.size(), n);
        const unsigned __int128 total = (unsigned __int128)(offsets[n] - offsets[0]) + n;
        std::vector<uint32_t> cut(n_shards + 1, 0);
        cut[n_shards] = n;
        for (uint32_t j = 1; j < n_shards; ++j) {
            // first read i whose prefix weight (offsets[i] - offsets[0] + i) reaches j / n_shards of the total
            uint32_t lo = cut[j - 1], hi = n;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                const unsigned __int128 w = (unsigned __int128)(offsets[mid] - offsets[0]) + mid;
                if (w * n_shards >= total * j) hi = mid; else lo = mid + 1;
            }
            cut[j] = lo;
        }
        auto shard = [&](uint32_t j) {
            const uint32_t lo = cut[j];
            return place_host_checked(g->replicas[j], bases, offsets + lo, cut[j + 1] - lo, params, out + lo, stats ? stats + lo : nullptr);
        };
        std::vector<int> rcs(n_shards, CLS_OK);
        std::vector<std::string> msgs(n_shards);
        std::vector<std::thread> th;
        if (n_shards == 1) {  // (one shard: the calling thread places it)
            rcs[0] = shard(0);
            if (rcs[0] != CLS_OK) msgs[0] = g_err;
        } else {
            try {
                for (uint32_t j = 0; j < n_shards; ++j) {
                    if (cut[j] == cut[j + 1]) continue;
                    th.emplace_back([&, j]() {
                        try {
                            rcs[j] = shard(j);
                            if (rcs[j] != CLS_OK) msgs[j] = g_err;  // (g_err is the worker's own: hand the message back)
                        } catch (...) {
                            rcs[j] = CLS_E_INTERNAL;
                            msgs[j] = "unknown exception";
                        }
                    });
                }
            } catch (...) {
                for (auto& t : th) t.join();
                return fail(CLS_E_INTERNAL, "cls_place_batch_group: could not start a worker thread");
            }
        }
        for (auto& t : th) t.join();
        for (uint32_t j = 0; j < n_shards; ++j)
            if (rcs[j] != CLS_OK)
                return fail(rcs[j], "replica " + std::to_string(j) + " (device " + std::to_string(g->devices[j]) + "): " + msgs[j]);
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_place_batch_group: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_place_batch_group: unknown exception");
    }
}

// ---- clade tally (include/cls_place.h; kernels in cls_tally.hip) ----------------------------------------------------

// id -> pre-order index of the handle's clades as the kernels probe it (IdSlot, tally_hash): the tally, the pairer and
// the selector each upload a copy.
static std::vector<cls::IdSlot> id_table(const cls_db* db) {
    const uint32_t n = (uint32_t)db->tree_rows.size();
    uint32_t cap = 16;
    while (cap < 2 * n) cap *= 2;
    std::vector<cls::IdSlot> table(cap, cls::IdSlot{0, cls::TALLY_NO_PRE, 0});
    for (const auto& r : db->tree_rows) {
        uint32_t h = (uint32_t)cls::tally_hash(r.id) & (cap - 1);
        while (table[h].pre != cls::TALLY_NO_PRE) h = (h + 1) & (cap - 1);
        table[h].id = r.id;
        table[h].pre = r.pre;
    }
    return table;
}

struct cls_tally {
    cls_db* db = nullptr;
    cls::TallyDev dev{};
    void* d_table = nullptr;
    void* d_acc = nullptr;        // cnt[3 n] | sums[2 n] | totals[16], 8 bytes each: one memset zeroes the tally
    void* d_work = nullptr;       // prefix[n + 1] | clade[n]
    void* d_size = nullptr;
    void* d_tmp = nullptr;
    size_t acc_bytes = 0;
    hipStream_t stream = nullptr; // read-out, reset and the host-record adds
    std::mutex mu;
    struct Mark { hipStream_t stream; hipEvent_t ev; };
    std::vector<Mark> marks;      // per caller stream: an event behind its last add (cls_tally_read waits for them)
};
constexpr size_t MAX_TALLY_MARKS = 64;

namespace {
// RAII: the handle's device current for the scope
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int device) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev != device) { e = hipSetDevice(device); switched = e == hipSuccess; }
        return e;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

// every add launched so far has finished (t->mu held)
int tally_drain(cls_tally* t) {
    for (auto& m : t->marks) CLS_HIP(hipEventSynchronize(m.ev));
    return CLS_OK;
}

}  // namespace

extern "C" void cls_tally_destroy(cls_tally* t) {
    if (!t) return;
    DeviceScope ds;
    (void)ds.enter(t->db->device);
    for (auto& m : t->marks) { (void)hipEventSynchronize(m.ev); (void)hipEventDestroy(m.ev); }
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    for (void* p : {t->d_table, t->d_acc, t->d_work, t->d_size, t->d_tmp}) if (p) (void)hipFree(p);
    delete t;
}

extern "C" int cls_tally_create(cls_db* db, cls_tally** out) {
    if (!db || !out) return fail(CLS_E_INVALID_ARG, "cls_tally_create: null argument");
    *out = nullptr;
    cls_tally* t = nullptr;
    try {
        const uint32_t n = (uint32_t)db->tree_rows.size();
        if (n == 0 || n >= cls::TALLY_MAX_NODES) return fail(CLS_E_INVALID_ARG, "cls_tally_create: the tree has too many clades for a tally");
        const std::vector<cls::IdSlot> table = id_table(db);
        const uint32_t cap = (uint32_t)table.size();
        std::vector<uint32_t> size_by_pre(n);
        for (const auto& r : db->tree_rows) size_by_pre[r.pre] = r.size;
        DeviceScope ds;
        CLS_HIP(ds.enter(db->device));
        t = new cls_tally();
        t->db = db;
        t->acc_bytes = (5 * (size_t)n + cls::TALLY_TOTALS) * 8;
        const size_t tmp_bytes = cls::tally_scan_tmp_bytes(n);
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipMalloc(&t->d_table, (size_t)cap * sizeof(cls::IdSlot))) != hipSuccess ||
            (e = hipMalloc(&t->d_acc, t->acc_bytes)) != hipSuccess ||
            (e = hipMalloc(&t->d_work, (2 * (size_t)n + 1) * 8)) != hipSuccess ||
            (e = hipMalloc(&t->d_size, (size_t)n * 4)) != hipSuccess ||
            (e = hipMalloc(&t->d_tmp, tmp_bytes)) != hipSuccess ||
            (e = hipMemcpyAsync(t->d_table, table.data(), (size_t)cap * sizeof(cls::IdSlot), hipMemcpyHostToDevice, t->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(t->d_size, size_by_pre.data(), (size_t)n * 4, hipMemcpyHostToDevice, t->stream)) != hipSuccess ||
            (e = hipMemsetAsync(t->d_acc, 0, t->acc_bytes, t->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(t->stream)) != hipSuccess) {
            cls_tally_destroy(t);
            return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_tally_create: ") + hipGetErrorString(e));
        }
        cls::TallyDev& d = t->dev;
        d.table = (const cls::IdSlot*)t->d_table;
        d.table_mask = cap - 1;
        d.n_nodes = n;
        d.cnt = (unsigned long long*)t->d_acc;
        d.sums = (long long*)t->d_acc + 3 * (size_t)n;
        d.totals = (unsigned long long*)t->d_acc + 5 * (size_t)n;
        d.size_by_pre = (const uint32_t*)t->d_size;
        d.prefix = (unsigned long long*)t->d_work;
        d.clade = (unsigned long long*)t->d_work + (size_t)n + 1;
        d.scan_tmp = t->d_tmp;
        d.scan_tmp_bytes = tmp_bytes;
        *out = t;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_tally_destroy(t);
        return fail(CLS_E_NOMEM, "cls_tally_create: out of host memory");
    } catch (...) {
        cls_tally_destroy(t);
        return fail(CLS_E_INTERNAL, "cls_tally_create: unknown exception");
    }
}

extern "C" int cls_tally_reset(cls_tally* t) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_reset: null handle");
    DeviceScope ds;
    CLS_HIP(ds.enter(t->db->device));
    std::lock_guard<std::mutex> g(t->mu);
    if (int rc = tally_drain(t)) return rc;
    CLS_HIP(hipMemsetAsync(t->d_acc, 0, t->acc_bytes, t->stream));
    CLS_HIP(hipStreamSynchronize(t->stream));
    return CLS_OK;
}

// The add on `stream` (the handle's device is current), and the mark cls_tally_read waits for.
// `mark` = false: the caller synchronises `stream` itself before it returns.
static int tally_add_on(cls_tally* t, const void* d_records, uint32_t n, hipStream_t stream, bool mark = true) {
    if (((uintptr_t)d_records & 7) != 0) return fail(CLS_E_INVALID_ARG, "cls_tally_add_device: records must be 8-byte aligned");
    std::lock_guard<std::mutex> g(t->mu);
    CLS_HIP(cls::launch_tally_add(t->dev, d_records, n, (uint32_t)t->db->n_cu, cls::tuning().tally_no_wave_combine ? 0 : 1, stream));
    if (!mark) return CLS_OK;
    // (hipStreamPerThread is one handle value that names a different stream in every host thread: never cached)
    if (stream != hipStreamPerThread) {
        for (auto& m : t->marks)
            if (m.stream == stream) { CLS_HIP(hipEventRecord(m.ev, stream)); return CLS_OK; }
        if (t->marks.size() < MAX_TALLY_MARKS) {
            hipEvent_t ev = nullptr;
            CLS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            if (hipEventRecord(ev, stream) != hipSuccess) { (void)hipEventDestroy(ev); return fail(CLS_E_HIP, "cls_tally_add_device: hipEventRecord failed"); }
            t->marks.push_back({stream, ev});
            return CLS_OK;
        }
    }
    CLS_HIP(hipStreamSynchronize(stream));  // no mark to leave: the add is waited for here
    return CLS_OK;
}

extern "C" int cls_tally_add_device(cls_tally* t, const void* d_records, uint32_t n, void* hip_stream) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_add_device: null handle");
    if (n == 0) return CLS_OK;
    if (!d_records) return fail(CLS_E_INVALID_ARG, "cls_tally_add_device: null buffer");
    DeviceScope ds;
    CLS_HIP(ds.enter(t->db->device));
    try {
        return tally_add_on(t, d_records, n, (hipStream_t)hip_stream);
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_tally_add_device: unknown exception");
    }
}

extern "C" int cls_tally_add(cls_tally* t, const cls_placement* records, uint32_t n) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_add: null handle");
    if (n == 0) return CLS_OK;
    if (!records) return fail(CLS_E_INVALID_ARG, "cls_tally_add: null buffer");
    DeviceScope ds;
    CLS_HIP(ds.enter(t->db->device));
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, (size_t)n * sizeof(cls_placement));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_tally_add: ") + hipGetErrorString(e));
    int rc = CLS_OK;
    try {
        if ((e = hipMemcpyAsync(d, records, (size_t)n * sizeof(cls_placement), hipMemcpyHostToDevice, t->stream)) != hipSuccess)
            rc = fail(CLS_E_HIP, std::string("cls_tally_add: ") + hipGetErrorString(e));
        else rc = tally_add_on(t, d, n, t->stream);
    } catch (...) {
        rc = fail(CLS_E_INTERNAL, "cls_tally_add: unknown exception");
    }
    (void)hipStreamSynchronize(t->stream);  // synchronous; the staging copy is freed behind the kernel
    (void)hipFree(d);
    return rc;
}

extern "C" int cls_tally_read(cls_tally* t, cls_tally_row* rows, uint32_t n_rows, cls_tally_totals* totals) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_read: null handle");
    const uint32_t n = t->dev.n_nodes;
    if (rows && n_rows != n) return fail(CLS_E_INVALID_ARG, "cls_tally_read: n_rows must be the tree's n_nodes (" + std::to_string(n) + ")");
    DeviceScope ds;
    CLS_HIP(ds.enter(t->db->device));
    try {
        std::vector<unsigned long long> acc(5 * (size_t)n + cls::TALLY_TOTALS), clade(n);
        {
            std::lock_guard<std::mutex> g(t->mu);
            if (int rc = tally_drain(t)) return rc;
            if (rows) {
                CLS_HIP(cls::launch_tally_finish(t->dev, t->stream));
                CLS_HIP(hipMemcpyAsync(clade.data(), t->dev.clade, (size_t)n * 8, hipMemcpyDeviceToHost, t->stream));
            }
            CLS_HIP(hipMemcpyAsync(acc.data(), t->d_acc, t->acc_bytes, hipMemcpyDeviceToHost, t->stream));
            CLS_HIP(hipStreamSynchronize(t->stream));
        }
        if (rows) {
            const unsigned long long* cnt = acc.data();
            const long long* sums = (const long long*)acc.data() + 3 * (size_t)n;
            for (uint32_t i = 0; i < n; ++i) {
                const auto& tr = t->db->tree_rows[i];
                cls_tally_row& r = rows[i];
                r.id = tr.id;
                r.n_clade = clade[tr.pre];
                r.n_identity = cnt[3 * (size_t)tr.pre];
                r.n_max_resolution = cnt[3 * (size_t)tr.pre + 1];
                r.n_inconclusive = cnt[3 * (size_t)tr.pre + 2];
                r.n_direct = r.n_identity + r.n_max_resolution + r.n_inconclusive;
                r.sum_one = sums[2 * (size_t)tr.pre];
                r.sum_rest = sums[2 * (size_t)tr.pre + 1];
            }
        }
        if (totals) {
            const unsigned long long* tot = acc.data() + 5 * (size_t)n;
            memset(totals, 0, sizeof *totals);
            for (int s = 0; s < 12; ++s) { totals->status_count[s] = tot[s]; totals->n_reads += tot[s]; }
            totals->n_bad_status = tot[cls::TALLY_BAD];
            totals->n_unknown_clade = tot[cls::TALLY_UNKNOWN];
            totals->n_reads += totals->n_bad_status;
        }
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_tally_read: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_tally_read: unknown exception");
    }
}

extern "C" int cls_tally_merge(cls_tally_row* rows, cls_tally_totals* totals, const cls_tally_row* add_rows,
                               const cls_tally_totals* add_totals, uint32_t n_rows) {
    if ((n_rows && (!rows || !add_rows)) || (!totals != !add_totals)) return fail(CLS_E_INVALID_ARG, "cls_tally_merge: null argument");
    for (uint32_t i = 0; i < n_rows; ++i) {
        const bool fresh = rows[i].id == 0 && rows[i].n_clade == 0 && rows[i].n_direct == 0;
        if (!fresh && rows[i].id != add_rows[i].id) return fail(CLS_E_INVALID_ARG, "cls_tally_merge: row " + std::to_string(i) + " names different clades");
    }
    for (uint32_t i = 0; i < n_rows; ++i) {
        cls_tally_row& r = rows[i];
        const cls_tally_row& a = add_rows[i];
        r.id = a.id;
        r.n_clade += a.n_clade; r.n_direct += a.n_direct; r.n_identity += a.n_identity;
        r.n_max_resolution += a.n_max_resolution; r.n_inconclusive += a.n_inconclusive;
        r.sum_one += a.sum_one; r.sum_rest += a.sum_rest;
    }
    if (totals) {
        totals->n_reads += add_totals->n_reads;
        for (int s = 0; s < 12; ++s) totals->status_count[s] += add_totals->status_count[s];
        totals->n_unknown_clade += add_totals->n_unknown_clade;
        totals->n_bad_status += add_totals->n_bad_status;
    }
    return CLS_OK;
}

// The counting rules as they are written in cls_place.h, one record after the other: a sorted id -> row list, the
// direct counters per row, then the call's n_direct summed bottom-up over the rows in reverse breadth-first order.
extern "C" int cls_tally_host(const cls_node* nodes, uint32_t n_nodes, const cls_placement* records, uint64_t n,
                              cls_tally_row* rows, cls_tally_totals* totals) {
    if (!nodes || n_nodes == 0 || !rows || !totals || (!records && n)) return fail(CLS_E_INVALID_ARG, "cls_tally_host: null argument");
    try {
        // parent row of every row, from the child ranges (`parent` ids are informational); row 0 is the root
        std::vector<uint32_t> parent_row(n_nodes, UINT32_MAX);
        std::vector<std::pair<uint64_t, uint32_t>> by_id(n_nodes);
        for (uint32_t r = 0; r < n_nodes; ++r) {
            by_id[r] = {nodes[r].id, r};
            if (nodes[r].n_children == 0) continue;
            if ((uint64_t)nodes[r].first_child + nodes[r].n_children > n_nodes || nodes[r].first_child == 0)
                return fail(CLS_E_BAD_TREE, "cls_tally_host: child rows out of range");
            for (uint32_t c = nodes[r].first_child; c < nodes[r].first_child + nodes[r].n_children; ++c) {
                if (parent_row[c] != UINT32_MAX) return fail(CLS_E_BAD_TREE, "cls_tally_host: row is the child of two parents (not a tree)");
                parent_row[c] = r;
            }
        }
        if (parent_row[0] != UINT32_MAX) return fail(CLS_E_BAD_TREE, "cls_tally_host: the root has a parent");
        for (uint32_t r = 1; r < n_nodes; ++r)
            if (parent_row[r] == UINT32_MAX) return fail(CLS_E_BAD_TREE, "cls_tally_host: rows unreachable from the root");
        std::vector<uint32_t> bfs;  // parents before their children
        bfs.reserve(n_nodes);
        bfs.push_back(0);
        for (size_t i = 0; i < bfs.size(); ++i)
            for (uint32_t c = 0; c < nodes[bfs[i]].n_children; ++c) bfs.push_back(nodes[bfs[i]].first_child + c);
        if (bfs.size() != n_nodes) return fail(CLS_E_BAD_TREE, "cls_tally_host: rows unreachable from the root");
        std::vector<uint64_t> below(n_nodes, 0);  // this call's n_direct, then its subtree sums
        std::sort(by_id.begin(), by_id.end());
        for (uint32_t r = 1; r < n_nodes; ++r)
            if (by_id[r].first == by_id[r - 1].first) return fail(CLS_E_BAD_TREE, "cls_tally_host: duplicate clade id " + std::to_string(by_id[r].first));
        for (uint32_t r = 0; r < n_nodes; ++r) {
            if (rows[r].id != nodes[r].id && (rows[r].id != 0 || rows[r].n_clade != 0))
                return fail(CLS_E_INVALID_ARG, "cls_tally_host: rows[" + std::to_string(r) + "] was filled for another tree");
            rows[r].id = nodes[r].id;
        }
        for (uint64_t i = 0; i < n; ++i) {
            const cls_placement& p = records[i];
            totals->n_reads++;
            if (p.status >= 12) { totals->n_bad_status++; continue; }
            totals->status_count[p.status]++;
            if (p.status != CLS_IDENTITY_FOUND && p.status != CLS_MAX_RESOLUTION && p.status != CLS_INCONCLUSIVE) continue;
            auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair((uint64_t)p.clade_id, (uint32_t)0));
            if (it == by_id.end() || it->first != p.clade_id) { totals->n_unknown_clade++; continue; }
            cls_tally_row& r = rows[it->second];
            r.n_direct++;
            below[it->second]++;
            if (p.status == CLS_IDENTITY_FOUND) { r.n_identity++; r.sum_one += p.one; r.sum_rest += p.rest; }
            else if (p.status == CLS_MAX_RESOLUTION) r.n_max_resolution++;
            else r.n_inconclusive++;
        }
        for (size_t i = n_nodes; i-- > 1;) below[parent_row[bfs[i]]] += below[bfs[i]];
        for (uint32_t r = 0; r < n_nodes; ++r) rows[r].n_clade += below[r];
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_tally_host: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_tally_host: unknown exception");
    }
}

// ---- read extraction (include/cls_place.h; kernels in cls_extract.hip) ------------------------------------------------

struct cls_selector {
    cls_db* db = nullptr;
    cls::SelectDev dev{};
    void* d_table = nullptr;      // a copy of the id table (id_table)
    void* d_sel = nullptr;        // sel_by_pre[n]
    hipStream_t stream = nullptr; // upload and the host-record calls
    std::mutex mu;                // (one host-record call at a time on `stream`)
};

// The two lists as (id, 1: include / 2: exclude), ascending by id; refuses what cls_place.h refuses.
static int selector_lists(const char* who, const uint64_t* include, uint32_t n_include, const uint64_t* exclude, uint32_t n_exclude, uint32_t flags,
                          std::vector<std::pair<uint64_t, uint8_t>>& listed) {
    if ((n_include && !include) || (n_exclude && !exclude)) return fail(CLS_E_INVALID_ARG, std::string(who) + ": null list");
    if (flags & ~CLS_SELECT_UNPLACED) return fail(CLS_E_INVALID_ARG, std::string(who) + ": unknown flag bit");
    listed.clear();
    listed.reserve((size_t)n_include + n_exclude);
    for (uint32_t i = 0; i < n_include; ++i) listed.push_back({include[i], (uint8_t)1});
    for (uint32_t i = 0; i < n_exclude; ++i) listed.push_back({exclude[i], (uint8_t)2});
    std::sort(listed.begin(), listed.end());
    for (size_t i = 1; i < listed.size(); ++i)
        if (listed[i].first == listed[i - 1].first)
            return fail(CLS_E_INVALID_ARG, std::string(who) + ": clade id " + std::to_string(listed[i].first) +
                                               (listed[i].second == listed[i - 1].second ? " is listed twice" : " is listed as include and as exclude"));
    return CLS_OK;
}

extern "C" void cls_selector_destroy(cls_selector* s) {
    if (!s) return;
    DeviceScope ds;
    (void)ds.enter(s->db->device);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    for (void* x : {s->d_table, s->d_sel}) if (x) (void)hipFree(x);
    delete s;
}

extern "C" int cls_selector_create(cls_db* db, const uint64_t* include, uint32_t n_include, const uint64_t* exclude, uint32_t n_exclude,
                                   uint32_t flags, cls_selector** out) {
    if (!db || !out) return fail(CLS_E_INVALID_ARG, "cls_selector_create: null argument");
    *out = nullptr;
    cls_selector* s = nullptr;
    try {
        const uint32_t n = (uint32_t)db->tree_rows.size();
        if (n == 0 || n >= cls::TALLY_MAX_NODES) return fail(CLS_E_INVALID_ARG, "cls_selector_create: the tree has too many clades for a selector");
        std::vector<std::pair<uint64_t, uint8_t>> listed;
        if (int rc = selector_lists("cls_selector_create", include, n_include, exclude, n_exclude, flags, listed)) return rc;
        // the listed clades' pre-order intervals, painted ancestors first: the innermost listed clade decides
        std::vector<std::pair<uint64_t, uint32_t>> by_id(n);
        for (uint32_t r = 0; r < n; ++r) by_id[r] = {db->tree_rows[r].id, r};
        std::sort(by_id.begin(), by_id.end());
        struct Span { uint32_t pre, size; uint8_t kind; };
        std::vector<Span> spans;
        spans.reserve(listed.size());
        for (const auto& x : listed) {
            auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(x.first, (uint32_t)0));
            if (it == by_id.end() || it->first != x.first)
                return fail(CLS_E_INVALID_ARG, "cls_selector_create: " + std::to_string(x.first) + " is no clade id of the tree");
            const auto& tr = db->tree_rows[it->second];
            spans.push_back({tr.pre, tr.size, x.second});
        }
        std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.pre < b.pre; });
        std::vector<uint8_t> sel_by_pre(n, 0);
        for (const Span& x : spans) std::fill(sel_by_pre.begin() + x.pre, sel_by_pre.begin() + x.pre + x.size, (uint8_t)(x.kind == 1 ? 1 : 0));
        const std::vector<cls::IdSlot> table = id_table(db);
        DeviceScope ds;
        CLS_HIP(ds.enter(db->device));
        s = new cls_selector();
        s->db = db;
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipMalloc(&s->d_table, table.size() * sizeof(cls::IdSlot))) != hipSuccess ||
            (e = hipMalloc(&s->d_sel, n)) != hipSuccess ||
            (e = hipMemcpyAsync(s->d_table, table.data(), table.size() * sizeof(cls::IdSlot), hipMemcpyHostToDevice, s->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(s->d_sel, sel_by_pre.data(), n, hipMemcpyHostToDevice, s->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(s->stream)) != hipSuccess) {
            cls_selector_destroy(s);
            return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_selector_create: ") + hipGetErrorString(e));
        }
        s->dev.table = (const cls::IdSlot*)s->d_table;
        s->dev.table_mask = (uint32_t)table.size() - 1;
        s->dev.n_nodes = n;
        s->dev.sel_by_pre = (const uint8_t*)s->d_sel;
        s->dev.unplaced = (flags & CLS_SELECT_UNPLACED) ? 1u : 0u;
        *out = s;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_selector_destroy(s);
        return fail(CLS_E_NOMEM, "cls_selector_create: out of host memory");
    } catch (...) {
        cls_selector_destroy(s);
        return fail(CLS_E_INTERNAL, "cls_selector_create: unknown exception");
    }
}

// The launch on `stream` (the handle's device is current).  `d_n_unplaced`: see launch_select_records.
static int select_on(cls_selector* s, const void* d_records, uint32_t n, void* d_sel, unsigned long long* d_n_unplaced, hipStream_t stream) {
    if (((uintptr_t)d_records & 7) != 0) return fail(CLS_E_INVALID_ARG, "cls_select_records_device: records must be 8-byte aligned");
    CLS_HIP(cls::launch_select_records(s->dev, d_records, n, (uint8_t*)d_sel, d_n_unplaced, stream));
    return CLS_OK;
}

extern "C" int cls_select_records_device(cls_selector* s, const void* d_records, uint32_t n, void* d_sel, void* hip_stream) {
    if (!s) return fail(CLS_E_INVALID_ARG, "cls_select_records_device: null handle");
    if (n == 0) return CLS_OK;
    if (!d_records || !d_sel) return fail(CLS_E_INVALID_ARG, "cls_select_records_device: null buffer");
    DeviceScope ds;
    CLS_HIP(ds.enter(s->db->device));
    return select_on(s, d_records, n, d_sel, nullptr, (hipStream_t)hip_stream);
}

extern "C" int cls_select_records(cls_selector* s, const cls_placement* records, uint32_t n, uint8_t* sel) {
    if (!s) return fail(CLS_E_INVALID_ARG, "cls_select_records: null handle");
    if (n == 0) return CLS_OK;
    if (!records || !sel) return fail(CLS_E_INVALID_ARG, "cls_select_records: null buffer");
    DeviceScope ds;
    CLS_HIP(ds.enter(s->db->device));
    const size_t rec_bytes = (size_t)n * sizeof(cls_placement);
    char* d = nullptr;  // records | sel
    hipError_t e = hipMalloc((void**)&d, rec_bytes + n);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_select_records: ") + hipGetErrorString(e));
    int rc = CLS_OK;
    {
        std::lock_guard<std::mutex> g(s->mu);
        if ((e = hipMemcpyAsync(d, records, rec_bytes, hipMemcpyHostToDevice, s->stream)) != hipSuccess)
            rc = fail(CLS_E_HIP, std::string("cls_select_records: ") + hipGetErrorString(e));
        else rc = select_on(s, d, n, d + rec_bytes, nullptr, s->stream);
        if (rc == CLS_OK && (e = hipMemcpyAsync(sel, d + rec_bytes, n, hipMemcpyDeviceToHost, s->stream)) != hipSuccess)
            rc = fail(CLS_E_HIP, std::string("cls_select_records: ") + hipGetErrorString(e));
        e = hipStreamSynchronize(s->stream);  // synchronous; the staging copy is freed behind the kernel
        if (rc == CLS_OK && e != hipSuccess) rc = fail(CLS_E_HIP, std::string("cls_select_records: ") + hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

// The selection rule as it is written in cls_place.h, one record after the other: a sorted id -> row list, parent rows
// from the child ranges, and a walk from the record's clade towards the root until a listed clade is met.
extern "C" int cls_select_host(const cls_node* nodes, uint32_t n_nodes, const uint64_t* include, uint32_t n_include, const uint64_t* exclude,
                               uint32_t n_exclude, uint32_t flags, const cls_placement* records, uint64_t n, uint8_t* sel) {
    if (!nodes || n_nodes == 0 || (n && (!records || !sel))) return fail(CLS_E_INVALID_ARG, "cls_select_host: null argument");
    try {
        std::vector<std::pair<uint64_t, uint8_t>> listed;
        if (int rc = selector_lists("cls_select_host", include, n_include, exclude, n_exclude, flags, listed)) return rc;
        constexpr uint32_t NONE = UINT32_MAX;
        std::vector<uint32_t> parent_row(n_nodes, NONE);
        std::vector<std::pair<uint64_t, uint32_t>> by_id(n_nodes);
        for (uint32_t r = 0; r < n_nodes; ++r) {
            by_id[r] = {nodes[r].id, r};
            if (nodes[r].n_children == 0) continue;
            if ((uint64_t)nodes[r].first_child + nodes[r].n_children > n_nodes || nodes[r].first_child == 0)
                return fail(CLS_E_BAD_TREE, "cls_select_host: child rows out of range");
            for (uint32_t c = nodes[r].first_child; c < nodes[r].first_child + nodes[r].n_children; ++c) {
                if (parent_row[c] != NONE) return fail(CLS_E_BAD_TREE, "cls_select_host: row is the child of two parents (not a tree)");
                parent_row[c] = r;
            }
        }
        if (parent_row[0] != NONE) return fail(CLS_E_BAD_TREE, "cls_select_host: the root has a parent");
        for (uint32_t r = 1; r < n_nodes; ++r)
            if (parent_row[r] == NONE) return fail(CLS_E_BAD_TREE, "cls_select_host: rows unreachable from the root");
        std::sort(by_id.begin(), by_id.end());
        for (uint32_t r = 1; r < n_nodes; ++r)
            if (by_id[r].first == by_id[r - 1].first) return fail(CLS_E_BAD_TREE, "cls_select_host: duplicate clade id " + std::to_string(by_id[r].first));
        auto row_of = [&](uint64_t id) -> uint32_t {
            auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, (uint32_t)0));
            return (it == by_id.end() || it->first != id) ? NONE : it->second;
        };
        std::vector<uint8_t> mark(n_nodes, 0);  // 1: include, 2: exclude
        for (const auto& x : listed) {
            const uint32_t r = row_of(x.first);
            if (r == NONE) return fail(CLS_E_INVALID_ARG, "cls_select_host: " + std::to_string(x.first) + " is no clade id of the tree");
            mark[r] = x.second;
        }
        const bool unplaced = (flags & CLS_SELECT_UNPLACED) != 0;
        for (uint64_t i = 0; i < n; ++i) {
            const cls_placement& p = records[i];
            uint32_t r = NONE;
            if (p.status == CLS_IDENTITY_FOUND || p.status == CLS_MAX_RESOLUTION || p.status == CLS_INCONCLUSIVE) r = row_of(p.clade_id);
            if (r == NONE) { sel[i] = unplaced ? 1 : 0; continue; }
            while (mark[r] == 0 && parent_row[r] != NONE) r = parent_row[r];
            sel[i] = mark[r] == 1 ? 1 : 0;
        }
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_select_host: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_select_host: unknown exception");
    }
}

extern "C" int cls_fastq_spans_device(const void* d_text, uint64_t len, uint32_t n, void* d_rec_off, void* hip_stream) {
    if (!d_rec_off || (!d_text && len)) return fail(CLS_E_INVALID_ARG, "cls_fastq_spans_device: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    uint64_t* d_ls = nullptr;
    uint64_t n_nl = 0;
    if (int rc = cls::fastq_line_starts_device(d_text, len, &d_ls, &n_nl, stream)) return rc;
    hipError_t e = cls::launch_fastq_spans(d_ls, n_nl, len, n, (uint64_t*)d_rec_off, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // (the line starts are freed behind the kernel)
    if (d_ls) (void)hipFree(d_ls);
    if (e != hipSuccess) return fail(CLS_E_HIP, std::string("cls_fastq_spans_device: ") + hipGetErrorString(e));
    return CLS_OK;
}

static int check_extract_args(const char* who, uint32_t stride, uint64_t n_items) {
    if (stride != 1 && stride != 2) return fail(CLS_E_INVALID_ARG, std::string(who) + ": stride must be 1 or 2");
    if (n_items * stride > 0xFFFFFFFFull) return fail(CLS_E_INVALID_ARG, std::string(who) + ": more than 2^32 - 1 records");
    return CLS_OK;
}

// The plan on `stream` with scratch of its own; synchronises `stream` to hand the sizes back.
static int extract_plan_on(const char* who, const void* d_text, const void* d_rec_off, uint32_t stride, uint32_t n_items, const void* d_sel,
                           void* d_out_off, cls_extract_totals* totals, hipStream_t stream) {
    memset(totals, 0, sizeof *totals);
    totals->n_records = n_items;
    void* d_tmp = nullptr;
    unsigned long long* d_cnt = nullptr;
    const size_t tmp_bytes = cls::extract_scan_tmp_bytes(n_items);
    unsigned long long cnt = 0;
    uint64_t bytes = 0;
    hipError_t e;
    if ((e = hipMalloc(&d_tmp, tmp_bytes)) == hipSuccess && (e = hipMalloc((void**)&d_cnt, 8)) == hipSuccess &&
        (e = hipMemsetAsync(d_cnt, 0, 8, stream)) == hipSuccess &&
        (e = cls::launch_extract_plan((const uint8_t*)d_text, (const uint64_t*)d_rec_off, stride, n_items, (const uint8_t*)d_sel, (uint64_t*)d_out_off,
                                      d_cnt, d_tmp, tmp_bytes, stream)) == hipSuccess &&
        (e = hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, stream)) == hipSuccess &&
        (e = hipMemcpyAsync(&bytes, (const uint64_t*)d_out_off + n_items, 8, hipMemcpyDeviceToHost, stream)) == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (d_tmp) (void)hipFree(d_tmp);
    if (d_cnt) (void)hipFree(d_cnt);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    totals->n_selected = cnt;
    totals->bytes_out = bytes;
    return CLS_OK;
}

extern "C" int cls_extract_plan_device(const void* d_text, const void* d_rec_off, uint32_t stride, uint32_t n_items, const void* d_sel,
                                       void* d_out_off, cls_extract_totals* totals, void* hip_stream) {
    if (!d_out_off || !totals || (n_items && (!d_rec_off || !d_sel))) return fail(CLS_E_INVALID_ARG, "cls_extract_plan_device: null argument");
    if (int rc = check_extract_args("cls_extract_plan_device", stride, n_items)) return rc;
    if ((uintptr_t)d_out_off & 7 || (uintptr_t)d_rec_off & 7) return fail(CLS_E_INVALID_ARG, "cls_extract_plan_device: offsets must be 8-byte aligned");
    return extract_plan_on("cls_extract_plan_device", d_text, d_rec_off, stride, n_items, d_sel, d_out_off, totals, (hipStream_t)hip_stream);
}

extern "C" int cls_extract_gather_device(const void* d_text, const void* d_rec_off, uint32_t stride, uint32_t n_items, const void* d_sel,
                                         const void* d_out_off, void* d_out, void* hip_stream) {
    if (int rc = check_extract_args("cls_extract_gather_device", stride, n_items)) return rc;
    if (n_items == 0) return CLS_OK;
    if (!d_rec_off || !d_sel || !d_out_off || !d_out) return fail(CLS_E_INVALID_ARG, "cls_extract_gather_device: null argument");
    if ((uintptr_t)d_out_off & 7 || (uintptr_t)d_rec_off & 7) return fail(CLS_E_INVALID_ARG, "cls_extract_gather_device: offsets must be 8-byte aligned");
    CLS_HIP(cls::launch_extract_gather((const uint8_t*)d_text, (const uint64_t*)d_rec_off, stride, n_items, (const uint8_t*)d_sel,
                                       (const uint64_t*)d_out_off, (uint8_t*)d_out, (hipStream_t)hip_stream));
    return CLS_OK;
}

// Record text and output as they are written in cls_place.h, one line and one item after the other.
extern "C" int cls_extract_host(const char* text, size_t len, uint32_t stride, const uint8_t* sel, uint64_t n_items, char** out, size_t* out_len,
                                cls_extract_totals* totals) {
    if (!out || !out_len || !totals || (!text && len) || (n_items && !sel)) return fail(CLS_E_INVALID_ARG, "cls_extract_host: null argument");
    *out = nullptr;
    *out_len = 0;
    if (int rc = check_extract_args("cls_extract_host", stride, n_items)) return rc;
    try {
        const uint64_t n = n_items * stride;
        std::vector<uint64_t> rec_off(n + 1, (uint64_t)len);  // (a line that does not start inside the text: `len`)
        uint64_t pos = 0;                                      // the start of line `line`
        for (uint64_t line = 0; line <= 4 * n && pos < len; ++line) {
            if (line % 4 == 0) rec_off[line / 4] = pos;
            const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
            pos = nl ? (uint64_t)(nl - text) + 1 : (uint64_t)len;
        }
        memset(totals, 0, sizeof *totals);
        totals->n_records = n_items;
        uint64_t bytes = 0;
        for (uint64_t i = 0; i < n_items; ++i) {
            if (!sel[i]) continue;
            totals->n_selected++;
            const uint64_t a = rec_off[i * stride], b = rec_off[(i + 1) * stride];
            if (b > a) bytes += (b - a) + (text[b - 1] != '\n' ? 1 : 0);
        }
        char* o = (char*)malloc(bytes + 1);
        if (!o) return fail(CLS_E_NOMEM, "cls_extract_host: out of host memory");
        uint64_t w = 0;
        for (uint64_t i = 0; i < n_items; ++i) {
            if (!sel[i]) continue;
            const uint64_t a = rec_off[i * stride], b = rec_off[(i + 1) * stride];
            if (b <= a) continue;
            memcpy(o + w, text + a, b - a);
            w += b - a;
            if (text[b - 1] != '\n') o[w++] = '\n';
        }
        o[w] = 0;
        totals->bytes_out = bytes;
        *out = o;
        *out_len = (size_t)bytes;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_extract_host: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_extract_host: unknown exception");
    }
}

// What the extract entries hang on place_text / pairs_text: the text stays on the device until the gather.
struct ExtractHook {
    cls_selector* s;
    char** out1;
    size_t* out1_len;
    char** out2;                 // pairs with two texts: R2's records
    size_t* out2_len;
    cls_extract_totals* totals;
};

// Spans from the FASTQ stage's line starts, plan, gather, D2H of the selected bytes: one text of a fused entry.
// *out is malloc'ed on success only.  totals: n_selected is set, bytes_out is ADDED to.
static int extract_stage(const char* who, const void* d_text, uint64_t len, const uint64_t* d_ls, uint64_t n_nl, uint32_t n_records,
                         uint32_t stride, uint32_t n_items, const void* d_sel, hipStream_t stream, char** out, size_t* out_len,
                         cls_extract_totals* totals) {
    void *d_rec_off = nullptr, *d_out_off = nullptr, *d_bytes = nullptr;
    char* h = nullptr;
    auto done = [&](int rc) {
        for (void* x : {d_rec_off, d_out_off, d_bytes}) if (x) (void)hipFree(x);
        if (rc != CLS_OK) free(h);
        return rc;
    };
    auto hip_fail = [&](hipError_t e) { return done(fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(who) + ": " + hipGetErrorString(e))); };
    hipError_t e;
    if ((e = hipMalloc(&d_rec_off, ((size_t)n_records + 1) * 8)) != hipSuccess || (e = hipMalloc(&d_out_off, ((size_t)n_items + 1) * 8)) != hipSuccess ||
        (e = cls::launch_fastq_spans(d_ls, n_nl, len, n_records, (uint64_t*)d_rec_off, stream)) != hipSuccess)
        return hip_fail(e);
    cls_extract_totals t;
    if (int rc = extract_plan_on(who, d_text, d_rec_off, stride, n_items, d_sel, d_out_off, &t, stream)) return done(rc);
    h = (char*)malloc(t.bytes_out + 1);
    if (!h) return done(fail(CLS_E_NOMEM, std::string(who) + ": out of host memory"));
    if ((e = hipMalloc(&d_bytes, t.bytes_out + 16)) != hipSuccess ||
        (e = cls::launch_extract_gather((const uint8_t*)d_text, (const uint64_t*)d_rec_off, stride, n_items, (const uint8_t*)d_sel,
                                        (const uint64_t*)d_out_off, (uint8_t*)d_bytes, stream)) != hipSuccess ||
        (t.bytes_out && (e = hipMemcpyAsync(h, d_bytes, t.bytes_out, hipMemcpyDeviceToHost, stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return hip_fail(e);
    h[t.bytes_out] = 0;
    totals->n_selected = t.n_selected;
    totals->bytes_out += t.bytes_out;
    *out = h;
    *out_len = (size_t)t.bytes_out;
    return done(CLS_OK);
}

// Query text -> records, all on the device: H2D of the file bytes, `scan` (the device FASTA or FASTQ stage),
// placement straight from the scanned bases, D2H of the 24-byte records and of the headers (the output stage needs
// those on the host).  `fa->bases` / `fa->base_off` come back NULL: the bases never leave the device.  `who` names the
// entry in messages.
using ScanText = int (*)(const void* d_text, uint64_t len, const void* opts, cls_fasta_dev* out, hipStream_t stream);
// With `tally` (the cls_tally_*_text entries) the records are added to it on the device instead: `fa` only carries n and
// truncated, `records` is NULL, and neither the headers, their offsets nor the records are copied back.
// With `ex` (cls_extract_fastq_text; FASTQ only, `scan` is not used) nothing per read is copied back either: the text
// stays on the device behind the scan, every chunk's records go through the selector, and the selected records' bytes
// are gathered from the text and returned.
static int place_text(const char* who, cls_db* db, const char* text, size_t len, const cls_params* params, ScanText scan,
                      const void* scan_opts, cls_fasta* fa, cls_placement** records, cls_tally* tally = nullptr, const ExtractHook* ex = nullptr) {
    if (!db || !fa || (!records && !tally && !ex) || (!text && len)) return fail(CLS_E_INVALID_ARG, std::string(who) + ": null argument");
    if (tally && tally->db != db) return fail(CLS_E_INVALID_ARG, std::string(who) + ": the tally belongs to another handle");
    if (ex && ex->s->db != db) return fail(CLS_E_INVALID_ARG, std::string(who) + ": the selector belongs to another handle");
    memset(fa, 0, sizeof *fa);
    if (records) *records = nullptr;
    int prev = 0;
    CLS_HIP(hipGetDevice(&prev));
    CLS_HIP(hipSetDevice(db->device));
    hipStream_t stream = nullptr;
    void *d_text = nullptr, *d_out = nullptr;
    uint64_t* d_ls = nullptr;      // `ex`: the scan's line starts
    uint64_t n_nl = 0;
    char* d_selbuf = nullptr;      // `ex`: the selected-unplaced counter (8 bytes) | one byte per record
    cls_fasta_dev dv;
    memset(&dv, 0, sizeof dv);
    cls_placement* recs = nullptr;
    bool ok = false;
    auto cleanup = [&]() {
        if (d_text) (void)hipFree(d_text);
        if (d_out) (void)hipFree(d_out);
        if (d_ls) (void)hipFree(d_ls);
        if (d_selbuf) (void)hipFree(d_selbuf);
        cls_fasta_dev_free(&dv);
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipSetDevice(prev);
        if (!ok) { free(recs); cls_fasta_free(fa); }
    };
#define CLS_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
    } while (0)
    try {
        CLS_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        CLS_TRY(hipMalloc(&d_text, len ? len : 16));
        if (len) CLS_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, stream));
        int rc = ex ? cls::fastq_scan_device_keep(d_text, len, (const cls_fastq_opts*)scan_opts, &dv, stream, &d_ls, &n_nl)
                    : scan(d_text, len, scan_opts, &dv, stream);
        if (rc != CLS_OK) { cleanup(); return rc; }
        if (!ex) {  // (an extraction gathers from the text at the end)
            (void)hipFree(d_text);
            d_text = nullptr;
        }
        const uint32_t n = dv.n;
        fa->n = n;
        fa->truncated = dv.truncated;
        std::vector<uint64_t> boff((size_t)n + 1);
        if (ex) {
            CLS_TRY(hipMalloc((void**)&d_selbuf, 8 + (size_t)n + 8));
            CLS_TRY(hipMemsetAsync(d_selbuf, 0, 8, stream));
        }
        if (!tally && !ex) {
            fa->headers = (char*)malloc(dv.n_header_bytes + 1);
            fa->header_off = (uint64_t*)malloc(((size_t)n + 1) * 8);
            recs = (cls_placement*)malloc(((size_t)n + 1) * sizeof(cls_placement));
            if (!fa->headers || !fa->header_off || !recs) { cleanup(); return fail(CLS_E_NOMEM, std::string(who) + ": out of host memory"); }
            if (dv.n_header_bytes) CLS_TRY(hipMemcpyAsync(fa->headers, dv.d_headers, dv.n_header_bytes, hipMemcpyDeviceToHost, stream));
            CLS_TRY(hipMemcpyAsync(fa->header_off, dv.d_header_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
        }
        CLS_TRY(hipMemcpyAsync(boff.data(), dv.d_base_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
        CLS_TRY(hipStreamSynchronize(stream));
        const uint32_t max_reads = 16u << 20;  // bounds the per-call scratch (class lists, sort keys)
        if (n) CLS_TRY(hipMalloc(&d_out, (size_t)std::min(n, max_reads) * sizeof(cls_placement)));
        for (uint32_t first = 0; first < n; first += max_reads) {
            const uint32_t cnt = std::min(max_reads, n - first);
            uint64_t longest = 1;  // (the classes beyond the chunk's longest read are not launched)
            uint32_t n_long = 1;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint64_t l = boff[first + i + 1] - boff[first + i];
                const uint64_t nk = l < db->dev.k ? 0 : 2 * (l - db->dev.k + 1);
                longest = std::max(longest, std::min(l, HARD_MAX_READ_LEN));
                if (nk > cls::MAX_READ_KMERS) ++n_long;
            }
            rc = place_device(db, dv.d_bases, (const uint64_t*)dv.d_base_off + first, cnt, params, d_out, nullptr, stream, (uint32_t)(2 * longest), n_long);
            if (rc != CLS_OK) { cleanup(); return rc; }
            if (tally) {
                rc = tally_add_on(tally, d_out, cnt, stream, false);  // (in stream order behind the placement; waited for below)
                if (rc != CLS_OK) { cleanup(); return rc; }
            } else if (!ex) CLS_TRY(hipMemcpyAsync(recs + first, d_out, (size_t)cnt * sizeof(cls_placement), hipMemcpyDeviceToHost, stream));
            if (ex) {
                rc = select_on(ex->s, d_out, cnt, d_selbuf + 8 + first, (unsigned long long*)d_selbuf, stream);
                if (rc != CLS_OK) { cleanup(); return rc; }
            }
            CLS_TRY(hipStreamSynchronize(stream));
        }
        if (ex) {
            unsigned long long n_unplaced = 0;
            CLS_TRY(hipMemcpyAsync(&n_unplaced, d_selbuf, 8, hipMemcpyDeviceToHost, stream));
            CLS_TRY(hipStreamSynchronize(stream));
            memset(ex->totals, 0, sizeof *ex->totals);
            ex->totals->n_records = n;
            ex->totals->n_selected_unplaced = n_unplaced;
            rc = extract_stage(who, d_text, len, d_ls, n_nl, n, 1, n, d_selbuf + 8, stream, ex->out1, ex->out1_len, ex->totals);
            if (rc != CLS_OK) { cleanup(); return rc; }
        }
        if (records) *records = recs;
        ok = true;
        cleanup();
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cleanup();
        return fail(CLS_E_NOMEM, std::string(who) + ": out of host memory");
    } catch (...) {
        cleanup();
        return fail(CLS_E_INTERNAL, std::string(who) + ": unknown exception");
    }
#undef CLS_TRY
}

extern "C" int cls_place_fasta_text(cls_db* db, const char* text, size_t len, const cls_params* params, cls_fasta* fa,
                                    cls_placement** records) {
    return place_text("cls_place_fasta_text", db, text, len, params,
                      [](const void* d, uint64_t n, const void*, cls_fasta_dev* out, hipStream_t st) { return cls_fasta_scan_device(d, n, out, st); },
                      nullptr, fa, records);
}

// The FASTQ twin: the device FASTQ stage (parse + quality trimming) in front of the same placement.
extern "C" int cls_place_fastq_text(cls_db* db, const char* text, size_t len, const cls_params* params, const cls_fastq_opts* opts,
                                    cls_fasta* fa, cls_placement** records) {
    return place_text("cls_place_fastq_text", db, text, len, params,
                      [](const void* d, uint64_t n, const void* o, cls_fasta_dev* out, hipStream_t st) {
                          return cls_fastq_scan_device(d, n, (const cls_fastq_opts*)o, out, st);
                      },
                      opts, fa, records);
}

// The same two routes into a tally: nothing per read returns to the host.
extern "C" int cls_tally_fasta_text(cls_db* db, cls_tally* t, const char* text, size_t len, const cls_params* params,
                                    uint32_t* n, uint32_t* truncated) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_fasta_text: null tally");
    cls_fasta fa;
    const int rc = place_text("cls_tally_fasta_text", db, text, len, params,
                              [](const void* d, uint64_t m, const void*, cls_fasta_dev* out, hipStream_t st) { return cls_fasta_scan_device(d, m, out, st); },
                              nullptr, &fa, nullptr, t);
    if (rc != CLS_OK) return rc;
    if (n) *n = fa.n;
    if (truncated) *truncated = fa.truncated;
    return CLS_OK;
}

extern "C" int cls_tally_fastq_text(cls_db* db, cls_tally* t, const char* text, size_t len, const cls_params* params,
                                    const cls_fastq_opts* opts, uint32_t* n, uint32_t* truncated) {
    if (!t) return fail(CLS_E_INVALID_ARG, "cls_tally_fastq_text: null tally");
    cls_fasta fa;
    const int rc = place_text("cls_tally_fastq_text", db, text, len, params,
                              [](const void* d, uint64_t m, const void* o, cls_fasta_dev* out, hipStream_t st) {
                                  return cls_fastq_scan_device(d, m, (const cls_fastq_opts*)o, out, st);
                              },
                              opts, &fa, nullptr, t);
    if (rc != CLS_OK) return rc;
    if (n) *n = fa.n;
    if (truncated) *truncated = fa.truncated;
    return CLS_OK;
}

// ---- paired reads (include/cls_place.h; kernels in cls_pair.hip) ----------------------------------------------------

struct cls_pairer {
    cls_db* db = nullptr;
    cls::PairDev dev{};
    void* d_table = nullptr;      // a copy of the tally's id table: the tally's own objects stay as they are
    void* d_tree = nullptr;       // size_by_pre[n] | parent_by_pre[n] | depth_by_pre[n]
    void* d_id = nullptr;         // id_by_pre[n]
    void* d_totals = nullptr;     // PAIR_CLASSES counters
    hipStream_t stream = nullptr; // read-out, reset and the host-record calls
    std::mutex mu;
    struct Mark { hipStream_t stream; hipEvent_t ev; };
    std::vector<Mark> marks;      // per caller stream: an event behind its last launch (cls_pairer_totals waits for them)
};
constexpr size_t MAX_PAIR_MARKS = 64;

extern "C" void cls_pairer_destroy(cls_pairer* p) {
    if (!p) return;
    DeviceScope ds;
    (void)ds.enter(p->db->device);
    for (auto& m : p->marks) { (void)hipEventSynchronize(m.ev); (void)hipEventDestroy(m.ev); }
    if (p->stream) { (void)hipStreamSynchronize(p->stream); (void)hipStreamDestroy(p->stream); }
    for (void* x : {p->d_table, p->d_tree, p->d_id, p->d_totals}) if (x) (void)hipFree(x);
    delete p;
}

extern "C" int cls_pairer_create(cls_db* db, cls_pairer** out) {
    if (!db || !out) return fail(CLS_E_INVALID_ARG, "cls_pairer_create: null argument");
    *out = nullptr;
    cls_pairer* p = nullptr;
    try {
        const uint32_t n = (uint32_t)db->tree_rows.size();
        if (n == 0 || n >= cls::TALLY_MAX_NODES) return fail(CLS_E_INVALID_ARG, "cls_pairer_create: the tree has too many clades for a pairer");
        const std::vector<cls::IdSlot> table = id_table(db);
        const uint32_t cap = (uint32_t)table.size();
        std::vector<uint32_t> tree(3 * (size_t)n);  // size | parent | depth, by pre
        std::vector<uint64_t> id_by_pre(n);
        uint32_t* size_by_pre = tree.data();
        uint32_t* parent_by_pre = tree.data() + n;
        uint32_t* depth_by_pre = tree.data() + 2 * (size_t)n;
        for (const auto& r : db->tree_rows) {
            size_by_pre[r.pre] = r.size;
            id_by_pre[r.pre] = r.id;
        }
        // parents and depths from the intervals: the clades open at pre-order index q are the ancestors of q
        std::vector<uint32_t> open;
        for (uint32_t q = 0; q < n; ++q) {
            while (!open.empty() && (uint64_t)open.back() + size_by_pre[open.back()] <= q) open.pop_back();
            parent_by_pre[q] = open.empty() ? q : open.back();
            depth_by_pre[q] = (uint32_t)open.size();
            open.push_back(q);
        }
        DeviceScope ds;
        CLS_HIP(ds.enter(db->device));
        p = new cls_pairer();
        p->db = db;
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipMalloc(&p->d_table, (size_t)cap * sizeof(cls::IdSlot))) != hipSuccess ||
            (e = hipMalloc(&p->d_tree, tree.size() * 4)) != hipSuccess ||
            (e = hipMalloc(&p->d_id, (size_t)n * 8)) != hipSuccess ||
            (e = hipMalloc(&p->d_totals, cls::PAIR_CLASSES * 8)) != hipSuccess ||
            (e = hipMemcpyAsync(p->d_table, table.data(), (size_t)cap * sizeof(cls::IdSlot), hipMemcpyHostToDevice, p->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(p->d_tree, tree.data(), tree.size() * 4, hipMemcpyHostToDevice, p->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(p->d_id, id_by_pre.data(), (size_t)n * 8, hipMemcpyHostToDevice, p->stream)) != hipSuccess ||
            (e = hipMemsetAsync(p->d_totals, 0, cls::PAIR_CLASSES * 8, p->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(p->stream)) != hipSuccess) {
            cls_pairer_destroy(p);
            return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_pairer_create: ") + hipGetErrorString(e));
        }
        cls::PairDev& d = p->dev;
        d.table = (const cls::IdSlot*)p->d_table;
        d.table_mask = cap - 1;
        d.n_nodes = n;
        d.size_by_pre = (const uint32_t*)p->d_tree;
        d.parent_by_pre = (const uint32_t*)p->d_tree + n;
        d.depth_by_pre = (const uint32_t*)p->d_tree + 2 * (size_t)n;
        d.id_by_pre = (const uint64_t*)p->d_id;
        d.totals = (unsigned long long*)p->d_totals;
        *out = p;
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_pairer_destroy(p);
        return fail(CLS_E_NOMEM, "cls_pairer_create: out of host memory");
    } catch (...) {
        cls_pairer_destroy(p);
        return fail(CLS_E_INTERNAL, "cls_pairer_create: unknown exception");
    }
}

extern "C" int cls_pairer_totals(cls_pairer* p, cls_pair_totals* totals, int reset) {
    if (!p || !totals) return fail(CLS_E_INVALID_ARG, "cls_pairer_totals: null argument");
    DeviceScope ds;
    CLS_HIP(ds.enter(p->db->device));
    std::lock_guard<std::mutex> g(p->mu);
    for (auto& m : p->marks) CLS_HIP(hipEventSynchronize(m.ev));
    unsigned long long tot[cls::PAIR_CLASSES];
    CLS_HIP(hipMemcpyAsync(tot, p->d_totals, sizeof tot, hipMemcpyDeviceToHost, p->stream));
    if (reset) CLS_HIP(hipMemsetAsync(p->d_totals, 0, sizeof tot, p->stream));
    CLS_HIP(hipStreamSynchronize(p->stream));
    memset(totals, 0, sizeof *totals);
    for (int s = 0; s < 7; ++s) { totals->how_count[s] = tot[s]; totals->n_pairs += tot[s]; }
    return CLS_OK;
}

static int check_pair_flags(const char* who, uint32_t stride, uint32_t flags) {
    if (stride != 1 && stride != 2) return fail(CLS_E_INVALID_ARG, std::string(who) + ": stride must be 1 or 2");
    if (flags & ~(CLS_PAIR_CONSERVATIVE | CLS_PAIR_REQUIRE_BOTH)) return fail(CLS_E_INVALID_ARG, std::string(who) + ": unknown flag bit");
    return CLS_OK;
}

// The launch on `stream` (the handle's device is current), and the mark cls_pairer_totals waits for.
// `mark` = false: the caller synchronises `stream` itself before it returns.
static int pair_on(cls_pairer* p, const void* d_a, const void* d_b, uint32_t stride, uint32_t n, uint32_t flags, void* d_out, void* d_how,
                   hipStream_t stream, bool mark = true) {
    const uintptr_t a = (uintptr_t)d_a, b = (uintptr_t)d_b, o = (uintptr_t)d_out;
    const size_t rec = sizeof(cls_placement);
    if ((a | b | o) & 7) return fail(CLS_E_INVALID_ARG, "cls_pair_records_device: records must be 8-byte aligned");
    if (stride == 2 && b != a + rec) return fail(CLS_E_INVALID_ARG, "cls_pair_records_device: stride 2 takes d_b = d_a + one record");
    auto overlaps = [&](uintptr_t x, uint64_t n_recs) { return o < x + n_recs * rec && x < o + (uint64_t)n * rec; };
    if (overlaps(a, stride == 2 ? 2ull * n : n) || (stride == 1 && overlaps(b, n)))
        return fail(CLS_E_INVALID_ARG, "cls_pair_records_device: d_out must not alias the inputs");
    std::lock_guard<std::mutex> g(p->mu);
    CLS_HIP(cls::launch_pair_records(p->dev, d_a, d_b, stride, n, flags, d_out, d_how, (uint32_t)p->db->n_cu, stream));
    if (!mark) return CLS_OK;
    // (hipStreamPerThread is one handle value that names a different stream in every host thread: never cached)
    if (stream != hipStreamPerThread) {
        for (auto& m : p->marks)
            if (m.stream == stream) { CLS_HIP(hipEventRecord(m.ev, stream)); return CLS_OK; }
        if (p->marks.size() < MAX_PAIR_MARKS) {
            hipEvent_t ev = nullptr;
            CLS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            if (hipEventRecord(ev, stream) != hipSuccess) { (void)hipEventDestroy(ev); return fail(CLS_E_HIP, "cls_pair_records_device: hipEventRecord failed"); }
            p->marks.push_back({stream, ev});
            return CLS_OK;
        }
    }
    CLS_HIP(hipStreamSynchronize(stream));  // no mark to leave: the launch is waited for here
    return CLS_OK;
}

extern "C" int cls_pair_records_device(cls_pairer* p, const void* d_a, const void* d_b, uint32_t stride, uint32_t n, uint32_t flags,
                                       void* d_out, void* d_how, void* hip_stream) {
    if (!p) return fail(CLS_E_INVALID_ARG, "cls_pair_records_device: null handle");
    if (int rc = check_pair_flags("cls_pair_records_device", stride, flags)) return rc;
    if (n == 0) return CLS_OK;
    if (!d_a || !d_b || !d_out) return fail(CLS_E_INVALID_ARG, "cls_pair_records_device: null buffer");
    DeviceScope ds;
    CLS_HIP(ds.enter(p->db->device));
    try {
        return pair_on(p, d_a, d_b, stride, n, flags, d_out, d_how, (hipStream_t)hip_stream);
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_pair_records_device: unknown exception");
    }
}

extern "C" int cls_pair_records(cls_pairer* p, const cls_placement* a, const cls_placement* b, uint32_t stride, uint32_t n, uint32_t flags,
                                cls_placement* out, uint8_t* how) {
    if (!p) return fail(CLS_E_INVALID_ARG, "cls_pair_records: null handle");
    if (int rc = check_pair_flags("cls_pair_records", stride, flags)) return rc;
    if (n == 0) return CLS_OK;
    if (!a || !b || !out) return fail(CLS_E_INVALID_ARG, "cls_pair_records: null buffer");
    if (stride == 2 && b != a + 1) return fail(CLS_E_INVALID_ARG, "cls_pair_records: stride 2 takes b = a + 1");
    DeviceScope ds;
    CLS_HIP(ds.enter(p->db->device));
    const size_t rec = sizeof(cls_placement), in_recs = 2 * (size_t)n;
    char* d = nullptr;  // mate 1 | mate 2 (or the interleaved records) | P | how
    hipError_t e = hipMalloc((void**)&d, (in_recs + n) * rec + n);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_pair_records: ") + hipGetErrorString(e));
    char *d_a = d, *d_b = stride == 2 ? d + rec : d + (size_t)n * rec, *d_out = d + in_recs * rec, *d_how = d_out + (size_t)n * rec;
    int rc = CLS_OK;
    try {
        if (stride == 2) e = hipMemcpyAsync(d_a, a, in_recs * rec, hipMemcpyHostToDevice, p->stream);
        else if ((e = hipMemcpyAsync(d_a, a, (size_t)n * rec, hipMemcpyHostToDevice, p->stream)) == hipSuccess)
            e = hipMemcpyAsync(d_b, b, (size_t)n * rec, hipMemcpyHostToDevice, p->stream);
        if (e != hipSuccess) rc = fail(CLS_E_HIP, std::string("cls_pair_records: ") + hipGetErrorString(e));
        else rc = pair_on(p, d_a, d_b, stride, n, flags, d_out, d_how, p->stream, false);
        if (rc == CLS_OK && ((e = hipMemcpyAsync(out, d_out, (size_t)n * rec, hipMemcpyDeviceToHost, p->stream)) != hipSuccess ||
                             (how && (e = hipMemcpyAsync(how, d_how, n, hipMemcpyDeviceToHost, p->stream)) != hipSuccess)))
            rc = fail(CLS_E_HIP, std::string("cls_pair_records: ") + hipGetErrorString(e));
    } catch (...) {
        rc = fail(CLS_E_INTERNAL, "cls_pair_records: unknown exception");
    }
    e = hipStreamSynchronize(p->stream);  // synchronous; the staging copy is freed behind the kernel
    if (rc == CLS_OK && e != hipSuccess) rc = fail(CLS_E_HIP, std::string("cls_pair_records: ") + hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}

// The pairing rule as it is written in cls_place.h, one pair after the other: a sorted id -> row list, parent rows and
// depths from the child ranges, the LCA by climbing from the deeper clade.
extern "C" int cls_pair_host(const cls_node* nodes, uint32_t n_nodes, const cls_placement* a, const cls_placement* b, uint32_t stride,
                             uint64_t n, uint32_t flags, cls_placement* out, uint8_t* how, cls_pair_totals* totals) {
    if (!nodes || n_nodes == 0 || (n && (!a || !b || !out))) return fail(CLS_E_INVALID_ARG, "cls_pair_host: null argument");
    if (int rc = check_pair_flags("cls_pair_host", stride, flags)) return rc;
    try {
        constexpr uint32_t NONE = UINT32_MAX;
        std::vector<uint32_t> parent_row(n_nodes, NONE), depth(n_nodes, 0);
        std::vector<std::pair<uint64_t, uint32_t>> by_id(n_nodes);
        for (uint32_t r = 0; r < n_nodes; ++r) {
            by_id[r] = {nodes[r].id, r};
            if (nodes[r].n_children == 0) continue;
            if ((uint64_t)nodes[r].first_child + nodes[r].n_children > n_nodes || nodes[r].first_child == 0)
                return fail(CLS_E_BAD_TREE, "cls_pair_host: child rows out of range");
            for (uint32_t c = nodes[r].first_child; c < nodes[r].first_child + nodes[r].n_children; ++c) {
                if (parent_row[c] != NONE) return fail(CLS_E_BAD_TREE, "cls_pair_host: row is the child of two parents (not a tree)");
                parent_row[c] = r;
            }
        }
        if (parent_row[0] != NONE) return fail(CLS_E_BAD_TREE, "cls_pair_host: the root has a parent");
        std::vector<uint32_t> bfs;  // parents before their children
        bfs.reserve(n_nodes);
        bfs.push_back(0);
        for (size_t i = 0; i < bfs.size(); ++i)
            for (uint32_t c = 0; c < nodes[bfs[i]].n_children; ++c) {
                const uint32_t row = nodes[bfs[i]].first_child + c;
                depth[row] = depth[bfs[i]] + 1;
                bfs.push_back(row);
            }
        if (bfs.size() != n_nodes) return fail(CLS_E_BAD_TREE, "cls_pair_host: rows unreachable from the root");
        std::sort(by_id.begin(), by_id.end());
        for (uint32_t r = 1; r < n_nodes; ++r)
            if (by_id[r].first == by_id[r - 1].first) return fail(CLS_E_BAD_TREE, "cls_pair_host: duplicate clade id " + std::to_string(by_id[r].first));
        auto usable_row = [&](const cls_placement& m) -> uint32_t {
            if (m.status != CLS_IDENTITY_FOUND && m.status != CLS_MAX_RESOLUTION && m.status != CLS_INCONCLUSIVE) return NONE;
            auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair((uint64_t)m.clade_id, (uint32_t)0));
            return (it == by_id.end() || it->first != m.clade_id) ? NONE : it->second;
        };
        auto copy = [](cls_placement& dst, const cls_placement& src) {
            memset(&dst, 0, sizeof dst);
            dst.status = src.status; dst.one = src.one; dst.rest = src.rest; dst.levels = src.levels; dst.clade_id = src.clade_id;
        };
        const bool conservative = flags & CLS_PAIR_CONSERVATIVE, require_both = flags & CLS_PAIR_REQUIRE_BOTH;
        for (uint64_t i = 0; i < n; ++i) {
            const cls_placement &m1 = a[i * stride], &m2 = b[i * stride];
            const uint32_t r1 = usable_row(m1), r2 = usable_row(m2);
            uint8_t klass;
            cls_placement& P = out[i];
            if (r1 == NONE && r2 == NONE) { klass = CLS_PAIR_NEITHER; copy(P, m1); }
            else if (r2 == NONE) { klass = CLS_PAIR_ONLY_1; copy(P, require_both ? m2 : m1); }
            else if (r1 == NONE) { klass = CLS_PAIR_ONLY_2; copy(P, require_both ? m1 : m2); }
            else if (r1 == r2) {
                klass = CLS_PAIR_SAME;
                bool second = false;
                if (m2.status != m1.status) second = m2.status < m1.status;
                else if (m2.one != m1.one) second = m2.one > m1.one;
                else if (m2.rest != m1.rest) second = m2.rest < m1.rest;
                copy(P, second ? m2 : m1);
            } else {
                uint32_t x = r1, y = r2;
                while (depth[x] > depth[y]) x = parent_row[x];
                while (depth[y] > depth[x]) y = parent_row[y];
                while (x != y) { x = parent_row[x]; y = parent_row[y]; }
                if (x == r2) { klass = CLS_PAIR_NESTED_1; copy(P, conservative ? m2 : m1); }       // mate 1 lies below mate 2
                else if (x == r1) { klass = CLS_PAIR_NESTED_2; copy(P, conservative ? m1 : m2); }
                else {
                    klass = CLS_PAIR_DISCORDANT;
                    memset(&P, 0, sizeof P);
                    P.status = CLS_MAX_RESOLUTION;
                    P.levels = depth[x];
                    P.clade_id = nodes[x].id;
                }
            }
            if (how) how[i] = klass;
            if (totals) { totals->n_pairs++; totals->how_count[klass]++; }
        }
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return fail(CLS_E_NOMEM, "cls_pair_host: out of host memory");
    } catch (...) {
        return fail(CLS_E_INTERNAL, "cls_pair_host: unknown exception");
    }
}

extern "C" int cls_pair_names_host(const char* headers1, const uint64_t* off1, const char* headers2, const uint64_t* off2, uint32_t stride,
                                   uint64_t n, uint64_t* n_bad, uint64_t* first_bad) {
    if (!n_bad || !first_bad || (n && (!headers1 || !off1 || !headers2 || !off2))) return fail(CLS_E_INVALID_ARG, "cls_pair_names_host: null argument");
    if (stride != 1 && stride != 2) return fail(CLS_E_INVALID_ARG, "cls_pair_names_host: stride must be 1 or 2");
    *n_bad = 0;
    *first_bad = UINT64_MAX;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t r = i * stride;
        const char *h1 = headers1 + off1[r], *h2 = headers2 + off2[r];
        const uint64_t l1 = cls::pair_name_len(h1, off1[r + 1] - off1[r]), l2 = cls::pair_name_len(h2, off2[r + 1] - off2[r]);
        if (l1 == l2 && memcmp(h1, h2, l1) == 0) continue;
        if (*n_bad == 0) *first_bad = i;
        ++*n_bad;
    }
    return CLS_OK;
}

// The name kernel on `stream` with a result buffer of its own; synchronises `stream`.
static int pair_names_on(const void* d_headers1, const void* d_off1, const void* d_headers2, const void* d_off2, uint32_t stride, uint32_t n,
                         uint64_t* n_bad, uint64_t* first_bad, hipStream_t stream) {
    *n_bad = 0;
    *first_bad = UINT64_MAX;
    if (n == 0) return CLS_OK;
    unsigned long long* d_res = nullptr;
    unsigned long long res[2] = {0, ~0ull};
    hipError_t e = hipMalloc((void**)&d_res, sizeof res);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string("cls_pair_names_device: ") + hipGetErrorString(e));
    if ((e = hipMemcpyAsync(d_res, res, sizeof res, hipMemcpyHostToDevice, stream)) == hipSuccess &&
        (e = hipStreamSynchronize(stream)) == hipSuccess &&  // (`res` is reused for the way back)
        (e = cls::launch_pair_names((const char*)d_headers1, (const uint64_t*)d_off1, (const char*)d_headers2, (const uint64_t*)d_off2, stride, n,
                                    d_res, stream)) == hipSuccess &&
        (e = hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, stream)) == hipSuccess)
        e = hipStreamSynchronize(stream);
    (void)hipFree(d_res);
    if (e != hipSuccess) return fail(CLS_E_HIP, std::string("cls_pair_names_device: ") + hipGetErrorString(e));
    *n_bad = res[0];
    *first_bad = res[1];
    return CLS_OK;
}

extern "C" int cls_pair_names_device(const void* d_headers1, const void* d_off1, const void* d_headers2, const void* d_off2, uint32_t stride,
                                     uint32_t n, uint64_t* n_bad, uint64_t* first_bad, void* hip_stream) {
    if (!n_bad || !first_bad || (n && (!d_off1 || !d_off2))) return fail(CLS_E_INVALID_ARG, "cls_pair_names_device: null argument");
    if (stride != 1 && stride != 2) return fail(CLS_E_INVALID_ARG, "cls_pair_names_device: stride must be 1 or 2");
    return pair_names_on(d_headers1, d_off1, d_headers2, d_off2, stride, n, n_bad, first_bad, (hipStream_t)hip_stream);
}

// Paired FASTQ text -> P (and `how`), all on the device; see cls_place_fastq_pairs_text in cls_place.h.  With `tally`
// P is added to it on the device instead and nothing per read is copied back (`fa` carries n and truncated only).
// With `ex` (cls_extract_fastq_pairs_text) nothing per pair is copied back: both texts stay on the device behind their
// scans, P goes through the selector, and the selected pairs' bytes are gathered from each text.
static int pairs_text(const char* who, cls_db* db, cls_pairer* p, cls_tally* tally, const char* text1, size_t len1, const char* text2,
                      size_t len2, const cls_params* params, const cls_fastq_opts* opts, uint32_t flags, cls_fasta* fa,
                      cls_placement** records, uint8_t** how, const ExtractHook* ex = nullptr) {
    if (!db || !p || !fa || (!records && !tally && !ex) || (!text1 && len1) || (!text2 && len2)) return fail(CLS_E_INVALID_ARG, std::string(who) + ": null argument");
    if (p->db != db) return fail(CLS_E_INVALID_ARG, std::string(who) + ": the pairer belongs to another handle");
    if (ex && ex->s->db != db) return fail(CLS_E_INVALID_ARG, std::string(who) + ": the selector belongs to another handle");
    if (tally && tally->db != db) return fail(CLS_E_INVALID_ARG, std::string(who) + ": the tally belongs to another handle");
    const uint32_t stride = text2 ? 1u : 2u;
    if (int rc = check_pair_flags(who, stride, flags)) return rc;
    memset(fa, 0, sizeof *fa);
    if (records) *records = nullptr;
    if (how) *how = nullptr;
    int prev = 0;
    CLS_HIP(hipGetDevice(&prev));
    CLS_HIP(hipSetDevice(db->device));
    hipStream_t stream = nullptr;
    void *d_text = nullptr, *d_bases = nullptr, *d_off = nullptr, *d_recs = nullptr, *d_P = nullptr, *d_how = nullptr, *d_hdr = nullptr, *d_new_off = nullptr;
    void* d_kept[2] = {nullptr, nullptr};   // `ex`: the texts, kept for the gather
    uint64_t* d_ls[2] = {nullptr, nullptr}; // `ex`: their line starts
    uint64_t n_nl[2] = {0, 0};
    char* d_selbuf = nullptr;               // `ex`: the selected-unplaced counter (8 bytes) | one byte per pair
    cls_fasta_dev dv1, dv2;
    memset(&dv1, 0, sizeof dv1);
    memset(&dv2, 0, sizeof dv2);
    cls_placement* recs = nullptr;
    uint8_t* h_how = nullptr;
    bool ok = false;
    auto cleanup = [&]() {
        for (void* x : {d_text, d_bases, d_off, d_recs, d_P, d_how, d_hdr, d_new_off, d_kept[0], d_kept[1], (void*)d_ls[0], (void*)d_ls[1], (void*)d_selbuf})
            if (x) (void)hipFree(x);
        cls_fasta_dev_free(&dv1);
        cls_fasta_dev_free(&dv2);
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipSetDevice(prev);
        if (!ok) { free(recs); free(h_how); cls_fasta_free(fa); }
    };
#define CLS_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
    } while (0)
    try {
        CLS_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        // ---- both texts to the device once, the FASTQ stage on each ------------------------------------------------
        const char* texts[2] = {text1, text2};
        const size_t lens[2] = {len1, len2};
        cls_fasta_dev* dvs[2] = {&dv1, &dv2};
        for (int m = 0; m < (text2 ? 2 : 1); ++m) {
            CLS_TRY(hipMalloc(&d_text, lens[m] ? lens[m] : 16));
            if (lens[m]) CLS_TRY(hipMemcpyAsync(d_text, texts[m], lens[m], hipMemcpyHostToDevice, stream));
            const int rc = ex ? cls::fastq_scan_device_keep(d_text, lens[m], opts, dvs[m], stream, &d_ls[m], &n_nl[m])
                              : cls_fastq_scan_device(d_text, lens[m], opts, dvs[m], stream);
            if (rc != CLS_OK) { cleanup(); return rc; }
            if (ex) d_kept[m] = d_text;  // (an extraction gathers from the text at the end)
            else (void)hipFree(d_text);
            d_text = nullptr;
        }
        if (text2 && dv1.n != dv2.n) {
            const std::string msg = std::string(who) + ": the mate files hold different numbers of records (" + std::to_string(dv1.n) + " and " +
                                    std::to_string(dv2.n) + ")";
            cleanup();
            return fail(CLS_E_BAD_PAIRS, msg);
        }
        if (!text2 && (dv1.n & 1u)) {
            const std::string msg = std::string(who) + ": the interleaved text holds an odd number of records (" + std::to_string(dv1.n) + ")";
            cleanup();
            return fail(CLS_E_BAD_PAIRS, msg);
        }
        const uint64_t n64 = text2 ? dv1.n : dv1.n / 2;
        if (n64 > 0x7FFFFFFFull) { cleanup(); return fail(CLS_E_BAD_PAIRS, std::string(who) + ": more than 2^31 - 1 pairs"); }
        const uint32_t n = (uint32_t)n64;
        const uint64_t n_reads = 2 * n64;
        fa->n = n;
        fa->truncated = dv1.truncated | dv2.truncated;
        // ---- the name check ------------------------------------------------------------------------------------------
        const char* d_h2 = (const char*)(text2 ? dv2.d_headers : dv1.d_headers);
        const uint64_t* d_o1 = (const uint64_t*)dv1.d_header_off;
        const uint64_t* d_o2 = text2 ? (const uint64_t*)dv2.d_header_off : d_o1 + 1;
        uint64_t n_bad = 0, first_bad = 0;
        int rc = pair_names_on(dv1.d_headers, d_o1, d_h2, d_o2, stride, n, &n_bad, &first_bad, stream);
        if (rc != CLS_OK) { cleanup(); return rc; }
        if (n_bad) {
            std::string names[2];
            const char* hs[2] = {(const char*)dv1.d_headers, d_h2};
            const uint64_t* os[2] = {d_o1, d_o2};
            for (int m = 0; m < 2; ++m) {
                uint64_t o[2];
                CLS_TRY(hipMemcpy(o, os[m] + first_bad * stride, sizeof o, hipMemcpyDeviceToHost));
                std::string h(o[1] - o[0], '\0');
                if (!h.empty()) CLS_TRY(hipMemcpy(&h[0], hs[m] + o[0], h.size(), hipMemcpyDeviceToHost));
                names[m] = h.substr(0, cls::pair_name_len(h.data(), h.size()));
            }
            const std::string msg = std::string(who) + ": the mates' names disagree in " + std::to_string(n_bad) + " pair(s), first at pair " +
                                    std::to_string(first_bad) + ": \"" + names[0] + "\" and \"" + names[1] + "\"";
            cleanup();
            return fail(CLS_E_BAD_PAIRS, msg);
        }
        // ---- one batch of 2 n reads: R1's bases then R2's, or the interleaved batch as it is ----------------------------
        std::vector<uint64_t> boff(n_reads + 1);
        CLS_TRY(hipMemcpyAsync(boff.data(), dv1.d_base_off, ((size_t)dv1.n + 1) * 8, hipMemcpyDeviceToHost, stream));
        const void* d_all_bases = dv1.d_bases;
        const uint64_t* d_all_off = (const uint64_t*)dv1.d_base_off;
        if (text2) {
            CLS_TRY(hipMemcpyAsync(boff.data() + n, dv2.d_base_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
            CLS_TRY(hipStreamSynchronize(stream));
            for (uint64_t i = n; i <= n_reads; ++i) boff[i] += dv1.n_bases;  // (boff[n] was R1's end, is R2's first offset + that)
            CLS_TRY(hipMalloc(&d_bases, dv1.n_bases + dv2.n_bases + 16));
            CLS_TRY(hipMalloc(&d_off, (n_reads + 1) * 8));
            if (dv1.n_bases) CLS_TRY(hipMemcpyAsync(d_bases, dv1.d_bases, dv1.n_bases, hipMemcpyDeviceToDevice, stream));
            if (dv2.n_bases) CLS_TRY(hipMemcpyAsync((char*)d_bases + dv1.n_bases, dv2.d_bases, dv2.n_bases, hipMemcpyDeviceToDevice, stream));
            CLS_TRY(hipMemcpyAsync(d_off, boff.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice, stream));
            d_all_bases = d_bases;
            d_all_off = (const uint64_t*)d_off;
        }
        CLS_TRY(hipStreamSynchronize(stream));
        if (n) {
            CLS_TRY(hipMalloc(&d_recs, n_reads * sizeof(cls_placement)));
            CLS_TRY(hipMalloc(&d_P, (size_t)n * sizeof(cls_placement)));
            CLS_TRY(hipMalloc(&d_how, n));
        }
        const uint64_t max_reads = 16u << 20;  // bounds the per-call scratch (class lists, sort keys): one call up to 8 M pairs
        for (uint64_t first = 0; first < n_reads; first += max_reads) {
            const uint32_t cnt = (uint32_t)std::min(max_reads, n_reads - first);
            uint64_t longest = 1;  // (the classes beyond the chunk's longest read are not launched)
            uint32_t n_long = 1;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint64_t l = boff[first + i + 1] - boff[first + i];
                const uint64_t nk = l < db->dev.k ? 0 : 2 * (l - db->dev.k + 1);
                longest = std::max(longest, std::min(l, HARD_MAX_READ_LEN));
                if (nk > cls::MAX_READ_KMERS) ++n_long;
            }
            rc = place_device(db, d_all_bases, d_all_off + first, cnt, params, (cls_placement*)d_recs + first, nullptr, stream, (uint32_t)(2 * longest), n_long);
            if (rc != CLS_OK) { cleanup(); return rc; }
            CLS_TRY(hipStreamSynchronize(stream));
        }
        // ---- the pairing kernel, then what returns --------------------------------------------------------------------
        if (n) {
            const cls_placement* d_a = (const cls_placement*)d_recs;
            rc = pair_on(p, d_a, stride == 2 ? d_a + 1 : d_a + n, stride, n, flags, d_P, d_how, stream, false);
            if (rc != CLS_OK) { cleanup(); return rc; }
        }
        if (ex) {
            CLS_TRY(hipMalloc((void**)&d_selbuf, 8 + (size_t)n + 8));
            CLS_TRY(hipMemsetAsync(d_selbuf, 0, 8, stream));
            if (n) {
                rc = select_on(ex->s, d_P, n, d_selbuf + 8, (unsigned long long*)d_selbuf, stream);
                if (rc != CLS_OK) { cleanup(); return rc; }
            }
        }
        if (tally) {
            if (n) {
                rc = tally_add_on(tally, d_P, n, stream, false);
                if (rc != CLS_OK) { cleanup(); return rc; }
            }
        } else if (!ex) {
            fa->header_off = (uint64_t*)malloc(((size_t)n + 1) * 8);
            recs = (cls_placement*)malloc(((size_t)n + 1) * sizeof(cls_placement));
            h_how = (uint8_t*)malloc((size_t)n + 1);
            if (!fa->header_off || !recs || !h_how) { cleanup(); return fail(CLS_E_NOMEM, std::string(who) + ": out of host memory"); }
            uint64_t n_hdr = dv1.n_header_bytes;
            const void* d_hdr_src = dv1.d_headers;
            if (text2) CLS_TRY(hipMemcpyAsync(fa->header_off, dv1.d_header_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
            else {
                // mate 1's headers of an interleaved set: every second one, gathered on the device
                std::vector<uint64_t> hoff(n_reads + 1);
                CLS_TRY(hipMemcpyAsync(hoff.data(), dv1.d_header_off, (n_reads + 1) * 8, hipMemcpyDeviceToHost, stream));
                CLS_TRY(hipStreamSynchronize(stream));
                fa->header_off[0] = 0;
                for (uint32_t i = 0; i < n; ++i) fa->header_off[i + 1] = fa->header_off[i] + (hoff[2 * (size_t)i + 1] - hoff[2 * (size_t)i]);
                n_hdr = fa->header_off[n];
                CLS_TRY(hipMalloc(&d_new_off, ((size_t)n + 1) * 8));
                CLS_TRY(hipMalloc(&d_hdr, n_hdr + 16));
                CLS_TRY(hipMemcpyAsync(d_new_off, fa->header_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
                CLS_TRY(cls::launch_pair_gather_headers((const char*)dv1.d_headers, d_o1, 2, n, (const uint64_t*)d_new_off, (char*)d_hdr, stream));
                d_hdr_src = d_hdr;
            }
            fa->headers = (char*)malloc(n_hdr + 1);
            if (!fa->headers) { cleanup(); return fail(CLS_E_NOMEM, std::string(who) + ": out of host memory"); }
            if (n_hdr) CLS_TRY(hipMemcpyAsync(fa->headers, d_hdr_src, n_hdr, hipMemcpyDeviceToHost, stream));
            if (n) {
                CLS_TRY(hipMemcpyAsync(recs, d_P, (size_t)n * sizeof(cls_placement), hipMemcpyDeviceToHost, stream));
                CLS_TRY(hipMemcpyAsync(h_how, d_how, n, hipMemcpyDeviceToHost, stream));
            }
        }
        CLS_TRY(hipStreamSynchronize(stream));
        if (ex) {
            unsigned long long n_unplaced = 0;
            CLS_TRY(hipMemcpyAsync(&n_unplaced, d_selbuf, 8, hipMemcpyDeviceToHost, stream));
            CLS_TRY(hipStreamSynchronize(stream));
            memset(ex->totals, 0, sizeof *ex->totals);
            ex->totals->n_records = n;
            ex->totals->n_selected_unplaced = n_unplaced;
            rc = extract_stage(who, d_kept[0], len1, d_ls[0], n_nl[0], dv1.n, stride, n, d_selbuf + 8, stream, ex->out1, ex->out1_len, ex->totals);
            if (rc == CLS_OK && text2) {
                rc = extract_stage(who, d_kept[1], len2, d_ls[1], n_nl[1], dv2.n, 1, n, d_selbuf + 8, stream, ex->out2, ex->out2_len, ex->totals);
                if (rc != CLS_OK) { free(*ex->out1); *ex->out1 = nullptr; *ex->out1_len = 0; }
            }
            if (rc != CLS_OK) { cleanup(); return rc; }
        }
        if (records) *records = recs; else free(recs);
        if (how) *how = h_how; else free(h_how);
        ok = true;
        cleanup();
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cleanup();
        return fail(CLS_E_NOMEM, std::string(who) + ": out of host memory");
    } catch (...) {
        cleanup();
        return fail(CLS_E_INTERNAL, std::string(who) + ": unknown exception");
    }
#undef CLS_TRY
}

extern "C" int cls_place_fastq_pairs_text(cls_db* db, cls_pairer* p, const char* text1, size_t len1, const char* text2, size_t len2,
                                          const cls_params* params, const cls_fastq_opts* opts, uint32_t flags, cls_fasta* fa,
                                          cls_placement** records, uint8_t** how) {
    if (!records) return fail(CLS_E_INVALID_ARG, "cls_place_fastq_pairs_text: null argument");
    return pairs_text("cls_place_fastq_pairs_text", db, p, nullptr, text1, len1, text2, len2, params, opts, flags, fa, records, how);
}

extern "C" int cls_tally_fastq_pairs_text(cls_db* db, cls_pairer* p, cls_tally* tally, const char* text1, size_t len1, const char* text2,
                                          size_t len2, const cls_params* params, const cls_fastq_opts* opts, uint32_t flags,
                                          uint32_t* n_pairs, uint32_t* truncated) {
    if (!tally) return fail(CLS_E_INVALID_ARG, "cls_tally_fastq_pairs_text: null tally");
    cls_fasta fa;
    const int rc = pairs_text("cls_tally_fastq_pairs_text", db, p, tally, text1, len1, text2, len2, params, opts, flags, &fa, nullptr, nullptr);
    if (rc != CLS_OK) return rc;
    if (n_pairs) *n_pairs = fa.n;
    if (truncated) *truncated = fa.truncated;
    return CLS_OK;
}

// ---- query text -> the selected records' text ----------------------------------------------------------------------------

extern "C" int cls_extract_fastq_text(cls_db* db, cls_selector* s, cls_tally* tally, const char* text, size_t len, const cls_params* params,
                                      const cls_fastq_opts* opts, char** out, size_t* out_len, cls_extract_totals* totals, uint32_t* n,
                                      uint32_t* truncated) {
    if (!s || !out || !out_len || !totals) return fail(CLS_E_INVALID_ARG, "cls_extract_fastq_text: null argument");
    *out = nullptr;
    *out_len = 0;
    memset(totals, 0, sizeof *totals);
    const ExtractHook ex{s, out, out_len, nullptr, nullptr, totals};
    cls_fasta fa;
    const int rc = place_text("cls_extract_fastq_text", db, text, len, params, nullptr, opts, &fa, nullptr, tally, &ex);
    if (rc != CLS_OK) return rc;
    if (n) *n = fa.n;
    if (truncated) *truncated = fa.truncated;
    return CLS_OK;
}

extern "C" int cls_extract_fastq_pairs_text(cls_db* db, cls_pairer* p, cls_selector* s, cls_tally* tally, const char* text1, size_t len1,
                                            const char* text2, size_t len2, const cls_params* params, const cls_fastq_opts* opts, uint32_t flags,
                                            char** out1, size_t* out1_len, char** out2, size_t* out2_len, cls_extract_totals* totals,
                                            uint32_t* n_pairs, uint32_t* truncated) {
    if (!s || !out1 || !out1_len || !totals || (text2 && (!out2 || !out2_len))) return fail(CLS_E_INVALID_ARG, "cls_extract_fastq_pairs_text: null argument");
    *out1 = nullptr;
    *out1_len = 0;
    if (out2) *out2 = nullptr;
    if (out2_len) *out2_len = 0;
    memset(totals, 0, sizeof *totals);
    const ExtractHook ex{s, out1, out1_len, out2, out2_len, totals};
    cls_fasta fa;
    const int rc = pairs_text("cls_extract_fastq_pairs_text", db, p, tally, text1, len1, text2, len2, params, opts, flags, &fa, nullptr, nullptr, &ex);
    if (rc != CLS_OK) return rc;
    if (n_pairs) *n_pairs = fa.n;
    if (truncated) *truncated = fa.truncated;
    return CLS_OK;
}
