// Host-side index builder: the reference's `map_kmers_to_tree`
// (core/src/use_cases/build_database/mod.rs:26-181) on an already parsed tree.
//   every MSA record -> forward + reverse-complement k-mers (kmers_map.rs:375-398)
//   -> (minimizer bucket = murmur3 of the first m chars, k-mer hash) -> union of the root->leaf id paths
//      of the leaves it is filed under (clade.rs:127-156, kmers_map.rs:125-149).
// CLS_BUILD_REFERENCE_HEADER_SHIFT reproduces the reference's record/header skew
// (build_database/mod.rs:93-116: a record's k-mers are sent with the NEXT record's header, the first
// header receives none, the last record is never indexed) -- what every database written by the
// reference actually contains, and what the golden fixture pins (tests/test_builder.py).
// cls_tree_build_kmers_map_device feeds the same records to the device builder (cls_build.hip); both expand leaves
// into node sets through cls::expand_leaf_paths, so they give the same bytes.
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "cls_build.h"
#include "cls_host.h"
#include "cls_host_internal.h"
#include "cls_murmur.h"

namespace {
struct Rec {
    uint64_t bkey, hash;
    uint32_t leaf;  // index into the leaf table
};
struct Leaf { std::string name; std::vector<uint64_t> path; };

// leaves in get_leaves_with_paths order (DFS), with their root->leaf id paths; first match by name wins, like
// `tree_leaves.iter().find(..)` (mod.rs:139-141)
void leaf_table(const cls_tree* t, std::vector<Leaf>& leaves, std::map<std::string, uint32_t>& by_name) {
    cls_tree_visit_leaves(t, [&](const char* name, const std::vector<uint64_t>& path) {
        by_name.emplace(name ? name : "", (uint32_t)leaves.size());
        leaves.push_back({name ? name : "", path});
    });
}

// Which leaf each record's k-mers are filed under (rec_leaf[i]; UINT32_MAX: record i is not indexed), or the
// reference's error for the first header that names no leaf.
std::string file_records(const cls_fasta& fa, const std::map<std::string, uint32_t>& by_name, bool shift, std::vector<uint32_t>& rec_leaf) {
    rec_leaf.assign(fa.n, UINT32_MAX);
    for (uint32_t i = 0; i < fa.n; ++i) {
        uint32_t hi = i;
        if (shift) { if (i + 1 >= fa.n) break; hi = i + 1; }  // the last record is never indexed
        const std::string header(fa.headers + fa.header_off[hi], fa.headers + fa.header_off[hi + 1]);
        auto it = by_name.find(header);
        if (it == by_name.end()) return "The sequence header does not match any tree leaf: " + header;
        rec_leaf[i] = it->second;
    }
    if (shift && fa.n) {  // the first header still has to name a leaf (it receives an empty k-mer list)
        const std::string h0(fa.headers + fa.header_off[0], fa.headers + fa.header_off[1]);
        if (!by_name.count(h0)) return "The sequence header does not match any tree leaf: " + h0;
    }
    return "";
}
}  // namespace

namespace cls {
void expand_leaf_paths(size_t n_kmers, const uint64_t* leaf_off, const uint32_t* leaf_ref,
                       const std::vector<std::vector<uint64_t>>& paths, std::vector<uint64_t>& node_off,
                       std::vector<uint64_t>& node_ids) {
    // contiguous k-mer ranges on up to 16 host threads, each into its own buffer; the pieces are joined in order
    const size_t nt = n_kmers < 4096 ? 1 : std::max<size_t>(1, std::min<size_t>(16, std::thread::hardware_concurrency()));
    std::vector<std::vector<uint64_t>> ids(nt), sizes(nt);
    auto work = [&](size_t t) {
        const size_t lo = n_kmers * t / nt, hi = n_kmers * (t + 1) / nt;
        std::vector<uint64_t> set;
        sizes[t].reserve(hi - lo);
        for (size_t j = lo; j < hi; ++j) {
            set.clear();
            for (uint64_t p = leaf_off[j]; p < leaf_off[j + 1]; ++p) set.insert(set.end(), paths[leaf_ref[p]].begin(), paths[leaf_ref[p]].end());
            std::sort(set.begin(), set.end());
            set.erase(std::unique(set.begin(), set.end()), set.end());
            ids[t].insert(ids[t].end(), set.begin(), set.end());
            sizes[t].push_back(set.size());
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    size_t total = 0;
    for (auto& v : ids) total += v.size();
    node_off.assign(1, 0);
    node_off.reserve(n_kmers + 1);
    node_ids.clear();
    node_ids.reserve(total);
    for (size_t t = 0; t < nt; ++t) {
        for (uint64_t n : sizes[t]) node_off.push_back(node_off.back() + n);
        node_ids.insert(node_ids.end(), ids[t].begin(), ids[t].end());
        std::vector<uint64_t>().swap(ids[t]);
    }
}
}  // namespace cls

extern "C" int cls_tree_build_kmers_map(cls_tree* t, const char* msa_text, size_t msa_len, uint64_t k_size, uint64_t m_size,
                                        uint32_t flags) {
    if (!t || (!msa_text && msa_len) || k_size == 0) return cls_host_fail(CLS_E_INVALID_ARG, "cls_tree_build_kmers_map: invalid argument");
    try {
        std::vector<Leaf> leaves;
        std::map<std::string, uint32_t> by_name;
        leaf_table(t, leaves, by_name);
        cls_fasta fa;
        int rc = cls_fasta_parse(msa_text, msa_len, &fa);
        if (rc != CLS_OK) return cls_host_fail(rc, "cls_tree_build_kmers_map: cannot parse the MSA");
        const bool fwd_only = flags & CLS_BUILD_FORWARD_ONLY;
        const uint32_t K = (uint32_t)k_size, M = (uint32_t)std::min<uint64_t>(m_size, k_size);
        std::vector<uint32_t> rec_leaf;
        const std::string err = file_records(fa, by_name, flags & CLS_BUILD_REFERENCE_HEADER_SHIFT, rec_leaf);
        std::vector<Rec> recs;
        for (uint32_t i = 0; i < fa.n && err.empty(); ++i) {
            if (rec_leaf[i] == UINT32_MAX) continue;
            const char* s = fa.bases + fa.base_off[i];
            const uint64_t L = fa.base_off[i + 1] - fa.base_off[i];
            if (L < K) continue;  // build_kmer_from_string: shorter than k -> []
            for (int strand = 0; strand < (fwd_only ? 1 : 2); ++strand) {
                for (uint64_t p = 0; p + K <= L; ++p) {
                    auto get = [&](uint32_t j) -> uint8_t {
                        if (!strand) return (uint8_t)s[p + j];
                        const char c = s[L - 1 - p - j];
                        return (uint8_t)(c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A');
                    };
                    recs.push_back({m_size == 0 ? 0ull : cls::murmur3_h1(get, M), cls::murmur3_h1(get, K), rec_leaf[i]});
                }
            }
        }
        cls_fasta_free(&fa);
        if (!err.empty()) return cls_host_fail(CLS_E_BAD_DB, err);
        std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
            if (a.bkey != b.bkey) return a.bkey < b.bkey;
            if (a.hash != b.hash) return a.hash < b.hash;
            return a.leaf < b.leaf;
        });
        // k-mers in (bucket, hash) order with their distinct leaves, then the node sets
        std::vector<uint64_t> bucket_key, bucket_kmer_off{0}, kmer_hash, leaf_off{0};
        std::vector<uint32_t> leaf_ref;
        for (size_t i = 0; i < recs.size();) {
            size_t j = i;
            uint32_t prev = UINT32_MAX;
            for (; j < recs.size() && recs[j].bkey == recs[i].bkey && recs[j].hash == recs[i].hash; ++j) {
                if (recs[j].leaf == prev) continue;
                prev = recs[j].leaf;
                leaf_ref.push_back(prev);
            }
            if (bucket_key.empty() || bucket_key.back() != recs[i].bkey) {
                if (!bucket_key.empty()) bucket_kmer_off.push_back(kmer_hash.size());
                bucket_key.push_back(recs[i].bkey);
            }
            kmer_hash.push_back(recs[i].hash);
            leaf_off.push_back(leaf_ref.size());
            i = j;
        }
        if (!bucket_key.empty()) bucket_kmer_off.push_back(kmer_hash.size());
        std::vector<uint64_t> kmer_node_off, node_ids;
        if (flags & CLS_BUILD_LEAVES_ONLY) {  // the distinct leaves' clade ids, ascending
            node_ids.resize(leaf_ref.size());
            for (size_t p = 0; p < leaf_ref.size(); ++p) node_ids[p] = leaves[leaf_ref[p]].path.back();
            for (size_t j = 0; j + 1 < leaf_off.size(); ++j) std::sort(node_ids.begin() + (long)leaf_off[j], node_ids.begin() + (long)leaf_off[j + 1]);
            kmer_node_off = std::move(leaf_off);
        } else {
            std::vector<std::vector<uint64_t>> paths(leaves.size());
            for (size_t l = 0; l < leaves.size(); ++l) paths[l] = std::move(leaves[l].path);
            cls::expand_leaf_paths(kmer_hash.size(), leaf_off.data(), leaf_ref.data(), paths, kmer_node_off, node_ids);
        }
        cls_tree_set_kmers_map(t, k_size, m_size, std::move(bucket_key), std::move(bucket_kmer_off), std::move(kmer_hash),
                               std::move(kmer_node_off), std::move(node_ids),
                               (flags & CLS_BUILD_LEAVES_ONLY) ? CLS_SETS_LEAVES : CLS_SETS_EXPLICIT);
        return CLS_OK;
    } catch (const std::exception& e) {
        return cls_host_fail(CLS_E_INTERNAL, std::string("cls_tree_build_kmers_map: ") + e.what());
    } catch (...) {
        return cls_host_fail(CLS_E_INTERNAL, "cls_tree_build_kmers_map: unknown exception");
    }
}

// The device builder on the same tree and MSA: the text goes through the device FASTA stage; only the headers and the
// record offsets come back, the bases stay in device memory for cls::kmers_build.
extern "C" int cls_tree_build_kmers_map_device(cls_tree* t, const char* msa_text, size_t msa_len, uint64_t k_size, uint64_t m_size,
                                               uint32_t flags, int device) {
    static const char* WHO = "cls_tree_build_kmers_map_device: ";
    if (!t || (!msa_text && msa_len) || k_size == 0 ||
        (flags & ~(CLS_BUILD_REFERENCE_HEADER_SHIFT | CLS_BUILD_FORWARD_ONLY | CLS_BUILD_LEAVES_ONLY)))
        return cls_host_fail(CLS_E_INVALID_ARG, std::string(WHO) + "invalid argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return cls_host_fail(CLS_E_NO_DEVICE, std::string(WHO) + "no HIP device");
    if (device < -1 || device >= n_dev) return cls_host_fail(CLS_E_INVALID_ARG, std::string(WHO) + "device " + std::to_string(device) + " out of range");
    int prev = 0;
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return cls_host_fail(CLS_E_HIP, std::string(WHO) + "hipGetDevice: " + hipGetErrorString(e));
    if (device < 0) device = prev;
    void* d_text = nullptr;
    cls_fasta_dev fd;
    memset(&fd, 0, sizeof fd);
    int rc = CLS_OK;
    std::string msg;
    auto hip_err = [&](hipError_t x, const char* what) {
        rc = x == hipErrorOutOfMemory ? CLS_E_NOMEM : CLS_E_HIP;
        msg = std::string(WHO) + what + ": " + hipGetErrorString(x);
    };
    try {
        std::vector<Leaf> leaves;
        std::map<std::string, uint32_t> by_name;
        leaf_table(t, leaves, by_name);
        if (device != prev && (e = hipSetDevice(device)) != hipSuccess) return cls_host_fail(CLS_E_HIP, std::string(WHO) + "hipSetDevice: " + hipGetErrorString(e));
        do {
            if ((e = hipMalloc(&d_text, std::max<size_t>(msa_len, 1))) != hipSuccess) { hip_err(e, "hipMalloc"); break; }
            if (msa_len && (e = hipMemcpy(d_text, msa_text, msa_len, hipMemcpyHostToDevice)) != hipSuccess) { hip_err(e, "hipMemcpy"); break; }
            if ((rc = cls_fasta_scan_device(d_text, msa_len, &fd, nullptr)) != CLS_OK) { msg = std::string(WHO) + "cannot parse the MSA: " + cls_last_error(); break; }
            if ((e = hipFree(d_text)) != hipSuccess) { d_text = nullptr; hip_err(e, "hipFree"); break; }
            d_text = nullptr;
            // headers and offsets to the host (the FASTA stage synchronised its stream)
            cls_fasta fa;
            memset(&fa, 0, sizeof fa);
            std::vector<char> headers(fd.n_header_bytes);
            std::vector<uint64_t> header_off((size_t)fd.n + 1), base_off((size_t)fd.n + 1);
            if (fd.n_header_bytes && (e = hipMemcpy(headers.data(), fd.d_headers, fd.n_header_bytes, hipMemcpyDeviceToHost)) != hipSuccess) { hip_err(e, "hipMemcpy"); break; }
            if ((e = hipMemcpy(header_off.data(), fd.d_header_off, header_off.size() * 8, hipMemcpyDeviceToHost)) != hipSuccess) { hip_err(e, "hipMemcpy"); break; }
            if ((e = hipMemcpy(base_off.data(), fd.d_base_off, base_off.size() * 8, hipMemcpyDeviceToHost)) != hipSuccess) { hip_err(e, "hipMemcpy"); break; }
            fa.n = fd.n;
            fa.headers = headers.data();
            fa.header_off = header_off.data();
            std::vector<uint32_t> rec_leaf;
            const std::string err = file_records(fa, by_name, flags & CLS_BUILD_REFERENCE_HEADER_SHIFT, rec_leaf);
            if (!err.empty()) { rc = CLS_E_BAD_DB; msg = err; break; }
            // the indexed records, in input order, as the flat entry takes them
            std::vector<uint64_t> offs{0}, leaf_id;
            uint32_t n_rec = 0;
            for (uint32_t i = 0; i < fa.n; ++i)
                if (rec_leaf[i] != UINT32_MAX) { n_rec = i + 1; leaf_id.push_back(leaves[rec_leaf[i]].path.back()); }
            offs.assign(base_off.begin(), base_off.begin() + n_rec + 1);
            cls_build_desc b;
            memset(&b, 0, sizeof b);
            b.abi_version = CLS_ABI_VERSION;
            b.n_nodes = (uint32_t)t->rows.size();
            b.nodes = t->rows.data();
            b.k_size = k_size;
            b.m_size = m_size;
            b.n_records = n_rec;
            b.flags = flags & (CLS_BUILD_FORWARD_ONLY | CLS_BUILD_LEAVES_ONLY);
            b.bases = (const char*)fd.d_bases;
            b.offsets = offs.data();
            b.leaf_id = leaf_id.data();
            cls_kmers* km = nullptr;
            if ((rc = cls::kmers_build(&b, device, true, &km)) != CLS_OK) { msg = std::string(WHO) + cls_last_error(); break; }
            cls_tree_set_kmers_map(t, k_size, m_size, std::move(km->bucket_key), std::move(km->bucket_kmer_off), std::move(km->kmer_hash),
                                   std::move(km->kmer_node_off), std::move(km->node_ids), km->node_set_kind);
            cls_kmers_free(km);
        } while (false);
    } catch (const std::bad_alloc&) {
        rc = CLS_E_NOMEM;
        msg = std::string(WHO) + "out of host memory";
    } catch (const std::exception& x) {
        rc = CLS_E_INTERNAL;
        msg = std::string(WHO) + x.what();
    }
    if (d_text && (e = hipFree(d_text)) != hipSuccess && rc == CLS_OK) hip_err(e, "hipFree");
    cls_fasta_dev_free(&fd);
    if (device != prev && (e = hipSetDevice(prev)) != hipSuccess && rc == CLS_OK) hip_err(e, "hipSetDevice");
    return rc == CLS_OK ? CLS_OK : cls_host_fail(rc, msg);
}
