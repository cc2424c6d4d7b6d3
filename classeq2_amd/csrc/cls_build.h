// Internal glue of the two index builders (cls_build.cpp on the host, cls_build.hip on the device); not part of the
// C-ABI.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "cls_place.h"

struct cls_kmers {
    uint64_t k_size = 0, m_size = 0;
    uint32_t node_set_kind = CLS_SETS_EXPLICIT;
    std::vector<uint64_t> bucket_key, bucket_kmer_off, kmer_hash, kmer_node_off, node_ids;
    cls_kmers_info info{};
};

namespace cls {

// Node set of each k-mer := sorted union of the root->leaf paths of its leaves (build_database/mod.rs:160-169).
// k-mer j lists leaf_ref[leaf_off[j] .. leaf_off[j + 1]) (indices into `paths`); node_off / node_ids are replaced.
// Both builders expand through it, so their explicit maps are the same bytes.
void expand_leaf_paths(size_t n_kmers, const uint64_t* leaf_off, const uint32_t* leaf_ref,
                       const std::vector<std::vector<uint64_t>>& paths, std::vector<uint64_t>& node_off,
                       std::vector<uint64_t>& node_ids);

// cls_kmers_build with the records' bases already in the memory of `device` (`bases_on_device`: b->bases is a device
// pointer; its offsets and leaf ids stay host arrays).  The error text is left for cls_last_error().
int kmers_build(const cls_build_desc* b, int device, bool bases_on_device, cls_kmers** out);

}  // namespace cls
