/*
 * cls_place.h -- C-ABI of the MI355X placement engine (libclsplace.so).
 *
 * Drop-in boundary for ONE path of LepistaBioinformatics/classeq2: the
 * `core::use_cases::place_sequences` use-case.  The reference has no FFI of
 * its own; the seam a maintainer binds is the pure function
 *
 *     place_sequence(header, sequence, &Tree, Option<i32>, Option<f64>,
 *                    Option<bool>) -> Result<PlacementStatus, MappedErrors>
 *     (core/src/use_cases/place_sequences/place_sequence.rs:42-50)
 *
 * called once per query by the batch driver
 * (core/src/use_cases/place_sequences/mod.rs:123-159).  The entry points
 * below replace that call for a whole batch; everything around it (FASTA
 * reader, annotations, YAML/JSONL writer) can stay in the Rust caller, see
 * INTEGRATION.md for the Rust `extern "C"` shim.
 *
 * Plain pointers and sizes only; no C++ or torch types; nothing unwinds
 * across this boundary.  All functions return 0 on success, a negative
 * CLS_E_* code otherwise; cls_last_error() gives the thread-local message.
 */
#ifndef CLS_PLACE_H
#define CLS_PLACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLS_ABI_VERSION 2u  /* 1 is still accepted: cls_db_desc without the trailing node_set_kind */

/* ---- error codes ------------------------------------------------------- */
#define CLS_OK 0
#define CLS_E_INVALID_ARG (-1)   /* null pointer, bad sizes, bad abi_version     */
#define CLS_E_BAD_TREE (-2)      /* node table is not a tree rooted at row 0     */
#define CLS_E_BAD_DB (-3)        /* k-mer map inconsistent / unsupported shape   */
#define CLS_E_NO_DEVICE (-4)     /* no HIP device / HIP extension unusable       */
#define CLS_E_HIP (-5)           /* a HIP runtime call failed                    */
#define CLS_E_NOMEM (-6)
#define CLS_E_INTERNAL (-7)
#define CLS_E_BAD_PAIRS (-8)     /* paired input whose mates do not line up      */

/* ---- tree: Clade (core/src/domain/dtos/clade.rs:18-38) ------------------ */
/* NodeType, clade.rs:5-16.  LEAF-ness is decided by `kind` only
 * (clade.rs:166-172), never by the absence of children. */
enum { CLS_KIND_ROOT = 0, CLS_KIND_NODE = 1, CLS_KIND_LEAF = 2 };

#define CLS_NO_PARENT UINT64_MAX

/* One row per clade.  Row 0 is `tree.root`; the children of a row occupy
 * `n_children` consecutive rows starting at `first_child`, in the order of
 * `Clade.children`.  `id` is the clade's (arbitrary, non-dense) u64 id. */
typedef struct cls_node {
    uint64_t id;
    uint64_t parent;       /* Clade.parent or CLS_NO_PARENT (informational)      */
    uint32_t first_child;  /* row of the first child (ignored if n_children==0)  */
    uint32_t n_children;
    uint8_t kind;          /* CLS_KIND_*                                         */
    uint8_t has_children;  /* 0: `children: None`; 1: `Some(vec)` (maybe empty)  */
    uint8_t pad_[6];
} cls_node;                /* 32 bytes */

/* ---- k-mer index: KmersMap (core/src/domain/dtos/kmers_map.rs:77-87) ---- */
/* Borrowed flat view of
 *   KmersMap{ k_size, m_size, map: HashMap<MinimizerKey, MinimizerValue> }
 *   MinimizerValue(HashMap<u64 /+kmer hash+/, HashSet<u64 /+node ids+/>>)
 * as two nested CSR levels.  Bucket b holds k-mers
 * [bucket_kmer_off[b], bucket_kmer_off[b+1]); k-mer j holds node ids
 * node_ids[kmer_node_off[j] .. kmer_node_off[j+1]) in any order. */
typedef struct cls_db_desc {
    uint32_t abi_version;  /* CLS_ABI_VERSION */
    uint32_t n_nodes;
    const cls_node* nodes;
    uint64_t k_size;       /* kSize */
    uint64_t m_size;       /* mSize */
    uint64_t n_buckets;
    const uint64_t* bucket_key;       /* [n_buckets]   MinimizerKey.0            */
    const uint64_t* bucket_kmer_off;  /* [n_buckets+1]                           */
    uint64_t n_kmers;
    const uint64_t* kmer_hash;        /* [n_kmers]     murmur3_x64_128(kmer,0).0 */
    const uint64_t* kmer_node_off;    /* [n_kmers+1]                             */
    const uint64_t* node_ids;         /* [kmer_node_off[n_kmers]] clade ids      */
    /* abi_version >= 2 */
    uint32_t node_set_kind;           /* CLS_SETS_*                              */
    uint32_t pad_;
} cls_db_desc;

/* What `node_ids` lists per k-mer:
 * CLS_SETS_EXPLICIT  every member of the node set, as the reference's index file holds it
 *                    (MinimizerValue: HashSet<u64> of clade ids, kmers_map.rs:16-17);
 * CLS_SETS_LEAVES    only the LEAF-kind members.  `map_kmers_to_tree` builds every node set as a union of
 *                    root->leaf paths (build_database/mod.rs:160-169; `get_path_to_root`, clade.rs:127-156), so the
 *                    leaves determine it: node set := union over the listed leaves of {leaf, its ancestors, root}.
 *                    The explicit sets of a deep tree are depth times larger (50 k leaves at depth 900: terabytes);
 *                    this form is what a caller derives from them (filter by kind) or builds directly.  Every id
 *                    must be a childless LEAF-kind clade of the tree (else CLS_E_BAD_DB). */
#define CLS_SETS_EXPLICIT 0u
#define CLS_SETS_LEAVES 1u

/* ---- per-call parameters: the three Option<> arguments ------------------ */
#define CLS_HAS_MAX_ITERATIONS 1u      /* Some(max_iterations); else 1000        */
#define CLS_HAS_MIN_MATCH_COVERAGE 2u  /* Some(min_match_coverage); else 0.7     */
#define CLS_HAS_REMOVE_INTERSECTION 4u /* Some(remove_intersection); else false  */

typedef struct cls_params {
    uint32_t flags;             /* CLS_HAS_* bits                                */
    int32_t max_iterations;     /* place_sequence.rs:65                          */
    double min_match_coverage;  /* clamped to [0,1], place_sequence.rs:67-75     */
    uint8_t remove_intersection;/* place_sequence.rs:64                          */
    uint8_t pad_[7];
} cls_params;                   /* NULL == all None */

/* ---- result: PlacementStatus / MappedErrors as a fixed record ----------- */
/* One per query, in input order.  The caller rebuilds
 * Result<PlacementStatus, MappedErrors> from it:
 *
 * status                         reference outcome (place_sequence.rs)
 * CLS_UNCLASSIFIABLE_NO_MATCH    Ok(Unclassifiable("Query sequence {header:?} may not be related to the phylogeny")) :130-139
 * CLS_UNCLASSIFIABLE_NO_ROOT     Ok(Unclassifiable("Query sequence has no overlapping kmers with the reference tree")) :156-164
 * CLS_UNCLASSIFIABLE_COVERAGE    Ok(Unclassifiable("Insufficient kmers coverage: {one}")) :247-254   (one = coverage)
 * CLS_UNCLASSIFIABLE_LEVEL1      Ok(Unclassifiable("Tree introspection not possible. ...")) :446-453
 * CLS_IDENTITY_FOUND             Ok(IdentityFound(AdherenceTest{clade=clade_id, one, rest})) update_introspection_node.rs:45-85
 * CLS_MAX_RESOLUTION             Ok(MaxResolutionReached(clade_id, "LCA Accepted")) :461-464
 * CLS_INCONCLUSIVE               Ok(Inconclusive(.., "Multiple proposals")) :584-598 (set-theoretically
 *                                unreachable; one = number of tied proposals, clade_id = parent)
 * CLS_ERR_TOO_FEW_KMERS          Err("The sequence does not contain enough kmers.", UCPLACE0005) :98-102
 * CLS_ERR_MAX_ITER               Err("The maximum number of iterations has been reached.", UCPLACE0010) :295-301
 * CLS_ERR_ROOT_NO_CHILDREN       Err("The root node does not have children. This is unexpected.") :199-206
 * CLS_ERR_INVALID_BASE           the reference panics (kmers_map.rs:440); reported per read instead
 * CLS_ERR_READ_TOO_LONG          device-buffer entry only: the read is longer than the handle provisions for
 *                                (cls_db_set_max_read_len; cls_db_info.max_read_kmers); the host-buffer entries size
 *                                themselves by the batch and place reads of up to 2^25 bases
 */
enum {
    CLS_UNCLASSIFIABLE_NO_MATCH = 0,
    CLS_UNCLASSIFIABLE_NO_ROOT = 1,
    CLS_UNCLASSIFIABLE_COVERAGE = 2,
    CLS_UNCLASSIFIABLE_LEVEL1 = 3,
    CLS_IDENTITY_FOUND = 4,
    CLS_MAX_RESOLUTION = 5,
    CLS_INCONCLUSIVE = 6,
    CLS_ERR_TOO_FEW_KMERS = 7,
    CLS_ERR_MAX_ITER = 8,
    CLS_ERR_ROOT_NO_CHILDREN = 9,
    CLS_ERR_INVALID_BASE = 10,
    CLS_ERR_READ_TOO_LONG = 11
};

typedef struct cls_placement {
    uint8_t status;     /* CLS_* above                                           */
    uint8_t pad_[3];
    int32_t one;        /* AdherenceTest.one  (adherence_test.rs:12)             */
    int32_t rest;       /* AdherenceTest.rest (adherence_test.rs:15)             */
    uint32_t levels;    /* introspection levels entered (`iteration`, :280)      */
    uint64_t clade_id;  /* Clade.id of the placement                             */
} cls_placement;        /* 24 bytes */

/* Optional per-query counters (the tracing span fields
 * place_sequence.rs:30-41); used by parity tests and by the roofline
 * accounting of bench.py. */
typedef struct cls_query_stats {
    uint32_t n_query_kmers;    /* query.kmers.count       = 2(L-k+1)             */
    uint32_t n_matched;        /* query.kmers.treeMatches = |M|                  */
    uint32_t n_with_root;      /* subject.kmers.queryMatches = |M_root|          */
    uint32_t index_bytes;      /* engine-side accounting, not a reference quantity: bytes of index data (table
                                * entries, node records, split records) the kernels asked for to place this read;
                                * bench.py's roofline numerator; 0 where a kernel does not count it */
    uint64_t leaf_postings;    /* sum over M of |{LEAF-kind ids in nodes(h)}|    */
} cls_query_stats;             /* 24 bytes */

typedef struct cls_db cls_db;  /* opaque, immutable after create (Send + Sync)   */

typedef struct cls_db_info {
    uint32_t n_nodes;
    uint32_t max_depth;        /* levels below the root                          */
    uint32_t max_nonleaf_arity;
    uint32_t k_size;
    uint32_t m_size;
    uint32_t n_buckets;
    uint64_t n_kmers;
    uint64_t n_closed_kmers;   /* node-set closed under `parent` (tip-compressed)*/
    uint64_t table_slots;
    uint64_t postings_words;
    uint64_t hbm_bytes;        /* device bytes held by the handle                */
    uint32_t max_read_kmers;   /* per-read k-mer capacity of the device-buffer entry as it would launch now (declared
                                * read length, tuning knobs): the largest read it places; longer ones are CLS_ERR_READ_TOO_LONG */
    int32_t device;
    uint32_t format;           /* 0: sorted lists (some node set is not closed under `parent`); 1: split-tree records */
    uint32_t binary_tree;      /* 1: every clade has zero or two children        */
    uint32_t direct_table;     /* 1: 2-bit-code direct table in use (k <= 15); 2: and the index is strand-symmetric
                                * (every k-mer shares its node set with its reverse complement: one lookup per window) */
    uint32_t n_tip_sets;       /* format 1: distinct tip lists (k-mers with the same one share a split tree) */
    uint32_t scratch_slots;    /* per-call scratch workspaces the handle holds right now (a caller that pipelines
                                * batches on ONE stream keeps one; at most 8) */
    uint32_t fat_direct_table; /* 1: k <= 12, the direct table is also kept with the set record inside its 16-byte entries */
} cls_db_info;

/* Number of usable HIP devices (0 if none). */
int cls_device_count(void);

/* Validate + re-encode + upload the index to `device` (-1: current device).
 * The views in `d` are only borrowed for the duration of the call.
 * Replaces nothing in the reference (it keeps the Tree in host hash maps,
 * ports/lib/src/functions/load_database.rs:9-53); called once after it. */
int cls_db_create(const cls_db_desc* d, int device, cls_db** out);
/* Host-only: run the validation + re-encoding of cls_db_create without
 * touching a device (CLS_OK, or the code cls_db_create would return). */
int cls_db_validate(const cls_db_desc* d);
void cls_db_destroy(cls_db* db);
int cls_db_info_get(const cls_db* db, cls_db_info* info);
/* The same for a caller compiled against an OLDER header: copies the first min(info_size, sizeof(cls_db_info))
 * bytes.  The struct only ever grows at its end (88 bytes in round 1, 96 since `fat_direct_table`): a binding that
 * may meet a newer library passes its own sizeof and never has bytes written past its struct. */
int cls_db_info_get2(const cls_db* db, void* info, size_t info_size);

/* Place `n` queries.  `bases` holds the concatenated sequences exactly as
 * `SequenceBody` holds them when place_sequence receives them (after the
 * FASTA stage, sequence.rs:47-56), `offsets[n+1]` their byte ranges.
 * Host pointers; synchronous; `out[n]` caller-allocated, input order.
 * Re-entrant: each call uses its own HIP stream.
 * Replaces: the per-query place_sequence() call, mod.rs:151-159. */
int cls_place_batch(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n,
                    const cls_params* params, cls_placement* out);

/* Same, with every buffer already resident in the HBM of the handle's
 * device; asynchronous on `hip_stream` (a hipStream_t, NULL = default
 * stream).  `d_stats` may be NULL.  This is the entry bench.py times. */
int cls_place_batch_device(cls_db* db, const void* d_bases, const void* d_offsets, uint32_t n,
                           const cls_params* params, void* d_out, void* d_stats, void* hip_stream);

/* Longest read (bases) cls_place_batch_device() provisions for (the lengths of a device-resident batch are not
 * known to the host).  Default 0: reads of up to 8192 k-mers (4096 + k - 1 bases), every read-length class launched;
 * longer reads are reported CLS_ERR_READ_TOO_LONG.  With n_bases set, the launch follows it: the read-length classes
 * beyond n_bases are not launched (a batch of 150 bp reads then costs one placement kernel, not one per class) and a
 * read longer than n_bases may be reported CLS_ERR_READ_TOO_LONG; a caller with reads beyond 8192 k-mers opts in
 * here.  cls_db_info.max_read_kmers reports the capacity that results (n_bases = 160: 320 k-mers).  Reads the
 * LDS-tiled kernel cannot hold keep their per-k-mer state in the workspace: 80 bytes per base and resident workgroup.
 * At most 2^25. */
int cls_db_set_max_read_len(cls_db* db, uint64_t n_bases);

/* Device time of the DOMINANT placement kernel (the wave-per-read kernel of the
 * 320-k-mer class; for a handle provisioned for long reads, cls_db_set_max_read_len,
 * the LDS-tiled kernel -- all of its launches together; the tuning knob time_class = 2 selects it for gene-length
 * reads too), accumulated over every cls_place_batch_device() launch on this
 * handle since the last reset: HIP events recorded around that kernel on the
 * caller's stream.  Waits for the launches still in flight.  Measurement aid for
 * bench.py's roofline figure; `reset` != 0 clears the accumulators afterwards. */
int cls_db_kernel_time(cls_db* db, double* sum_ms, uint64_t* launches, int reset);
/* Name (template instance, as rocprofv3 prints it without the argument list) of that dominant kernel for this
 * handle, without statistics: lets bench.py tie a committed profile to the kernel it really launches. */
int cls_db_kernel_name(const cls_db* db, char* buf, size_t len);

/* Test and measurement aid, not part of the Rust shim's surface: the read-length classes of a cls_place_batch_device()
 * launch provisioned for reads of up to n_bases bases (as after cls_db_set_max_read_len(db, n_bases); 0: its default) --
 * a host-buffer call plans each chunk the same way from its longest read -- in the order the reads are binned: class `list`
 * takes the reads of up to `max_kmers` k-mers (2(L - k + 1)) that no class before it takes, placed by the kernel instance
 * `kernel` (as cls_db_kernel_name names it).  `stats` != 0: the instances of a launch with per-query counters.  Follows
 * the tuning knobs at the time of the call.  Writes at most `max` entries; *n_out = how many classes there are. */
typedef struct cls_read_class {
    uint32_t list;         /* class list, 0 .. 7                                  */
    uint32_t max_kmers;    /* the longest read (k-mers) the class takes           */
    char kernel[112];
} cls_read_class;          /* 120 bytes */
int cls_db_read_classes(const cls_db* db, uint64_t n_bases, int stats, cls_read_class* out, int max, int* n_out);

/* Host-buffer variant that also returns the per-query counters. */
int cls_place_batch_stats(cls_db* db, const char* bases, const uint64_t* offsets, uint32_t n,
                          const cls_params* params, cls_placement* out, cls_query_stats* stats);

/* ---- index groups: one index on several devices, one process --------------
 * N replicas of one index, each a cls_db of its own.  The descriptor is validated and re-encoded once on the
 * host (the costly half of cls_db_create) and uploaded to every replica in parallel, one host thread each.
 * `devices` lists one ordinal per replica; repeats are allowed ({0, 0}: two replicas on device 0).  NULL or
 * n_devices == 0: every visible device, once each.  Every ordinal is checked before the encoding: out of range is
 * CLS_E_INVALID_ARG; no device at all is CLS_E_NO_DEVICE.  When an upload fails every replica is freed and the error
 * names the replica and its device. */
typedef struct cls_db_group cls_db_group;   /* opaque; N replicas of one index */
int cls_db_group_create(const cls_db_desc* d, const int* devices, uint32_t n_devices, cls_db_group** out);
void cls_db_group_destroy(cls_db_group* g);
int cls_db_group_size(const cls_db_group* g, uint32_t* n);
/* Replica i as a cls_db for every per-handle entry (info, kernel time, device-buffer batches).  Borrowed: it lives
 * as long as the group; never cls_db_destroy it. */
int cls_db_group_replica(cls_db_group* g, uint32_t i, cls_db** db);
/* cls_place_batch / cls_place_batch_stats across the group: host buffers, synchronous, `out[n]` (and `stats[n]`,
 * may be NULL) in input order, re-entrant.  The batch is cut into min(N, n) contiguous shards of about equal weight
 * (bases + 1 per read); replica i places shard i on a host thread of its own (one shard: on the calling thread),
 * straight into the caller's buffers.  Waits for every shard; the error of the lowest failing shard is returned,
 * its message prefixed "replica i (device d): ".  Records and counters equal those of cls_place_batch on one handle. */
int cls_place_batch_group(cls_db_group* g, const char* bases, const uint64_t* offsets, uint32_t n,
                          const cls_params* params, cls_placement* out, cls_query_stats* stats);

/* ---- index builder: map_kmers_to_tree (core/src/use_cases/build_database/mod.rs:26-181) on the device ----------
 * Records (filtered bases, one LEAF clade each) -> the k-mer map of cls_db_desc, without a cls_tree (cls_host.h has the
 * Newick + MSA use-case above it).  Every window of k bases of a record gives its forward k-mer and its reverse
 * complement (kmers_map.rs:375-398); a record shorter than k gives none.  k-mer hash = murmur3_x64_128(k-mer, 0).0,
 * bucket key = the same of its first min(m, k) characters, 0 when m = 0 (kmers_map.rs:125-149).  The result is in
 * canonical order: buckets ascending by key, k-mers ascending by hash inside a bucket, ids ascending inside a k-mer --
 * byte for byte what the host builder (cls_tree_build_kmers_map) makes of the same records. */
#define CLS_BUILD_FORWARD_ONLY 2u /* forward k-mers only (builds older than the reverse-complement change)           */
#define CLS_BUILD_LEAVES_ONLY 4u  /* node sets as CLS_SETS_LEAVES (the distinct leaves of each k-mer), not explicit  */

typedef struct cls_build_desc {
    uint32_t abi_version;       /* CLS_ABI_VERSION                                                              */
    uint32_t n_nodes;
    const cls_node* nodes;      /* the tree exactly as cls_db_create takes it                                   */
    uint64_t k_size;            /* [1, 1024]                                                                    */
    uint64_t m_size;
    uint32_t n_records;
    uint32_t flags;             /* CLS_BUILD_FORWARD_ONLY | CLS_BUILD_LEAVES_ONLY                               */
    const char* bases;          /* host memory: concatenated records (filtered upper-case ACGT)                 */
    const uint64_t* offsets;    /* [n_records + 1] non-decreasing byte offsets into `bases`                     */
    const uint64_t* leaf_id;    /* [n_records] id of the childless LEAF-kind clade each record is filed under   */
} cls_build_desc;

typedef struct cls_kmers cls_kmers; /* owned result of a build */

/* Measurement aid: sizes and device times (HIP events) of one build. */
typedef struct cls_kmers_info {
    uint64_t n_windows;         /* k-mer occurrences hashed (both strands)                                      */
    uint64_t n_kmers;           /* distinct (bucket, hash)                                                      */
    uint64_t n_leaf_postings;   /* distinct (k-mer, leaf) pairs                                                 */
    uint64_t n_node_ids;        /* ids of the result (= n_leaf_postings for CLS_BUILD_LEAVES_ONLY)             */
    uint64_t n_buckets;
    uint64_t peak_device_bytes; /* device memory the build held at its peak (input bases included)             */
    double ms_hash;             /* H2D of the records' tables + window hashing                                  */
    double ms_sort;             /* the window sort                                                              */
    double ms_group;            /* unique (k-mer, leaf), CSR offsets, bucket order                              */
    double ms_d2h;              /* copies of the result to the host                                             */
    double ms_expand;           /* host: leaves -> explicit node sets (0 with CLS_BUILD_LEAVES_ONLY)            */
    uint32_t sort_passes;       /* radix passes over the windows                                                */
    uint32_t full_key;          /* 1: the sort also keyed on the bucket (two k-mers shared a 64-bit hash)      */
} cls_kmers_info;

/* Build on `device` (-1: the current one).  Bad sizes, flags or a device out of range: CLS_E_INVALID_ARG; a leaf_id
 * that is not a childless LEAF of the tree: CLS_E_BAD_DB; a build whose device memory exceeds what hipMemGetInfo
 * reports free: CLS_E_NOMEM.  The views of `b` are borrowed for the call only.  Frees every device allocation it
 * made, whatever the outcome. */
int cls_kmers_build(const cls_build_desc* b, int device, cls_kmers** out);
/* Borrowed view for cls_db_create(): the arrays of `km`, the tree of `b`; node_set_kind follows CLS_BUILD_LEAVES_ONLY
 * of the build.  Valid while both live. */
int cls_kmers_desc(const cls_kmers* km, const cls_build_desc* b, cls_db_desc* d);
int cls_kmers_info_get(const cls_kmers* km, cls_kmers_info* info);
void cls_kmers_free(cls_kmers* km);

/* ---- FASTA input stage (file_or_stdin.rs:76-116, sequence.rs:47-56) ------ */
typedef struct cls_fasta {
    uint32_t n;               /* records                                        */
    uint32_t truncated;       /* 1: stopped at "unexpected sequence without header" (error ignored by the caller, mod.rs:119) */
    char* headers;            /* concatenated header bytes                      */
    uint64_t* header_off;     /* [n+1]                                          */
    char* bases;              /* concatenated filtered (upper-case ACGT) bases  */
    uint64_t* base_off;       /* [n+1]                                          */
} cls_fasta;

int cls_fasta_parse(const char* text, size_t len, cls_fasta* out);
void cls_fasta_free(cls_fasta* f);
/* Host only: cut points for parsing `text` in up to `max_pieces` pieces, one cls_fasta_parse (or device FASTA stage)
 * each.  cuts[0] = 0 <= cuts[1] < ... < cuts[*n_pieces] = len (`cuts` holds max_pieces + 1 entries).  Interior cut i is
 * the first safe cut at or after i * len / max_pieces (duplicates dropped).  A safe cut starts a '>' line that is
 * valid UTF-8 and ends a record whose header line is not empty once '\r' and every '>' are removed and whose sequence
 * lines hold one of ACGTacgt: the parse of the whole text emits that record there, the parse of the piece emits it at
 * its end, and the next piece starts in the parser's initial state.  Concatenating the pieces' records, up to and including the first
 * piece that reports `truncated` (the pieces after it are dropped), gives the records of the whole text. */
int cls_fasta_split(const char* text, size_t len, uint32_t max_pieces, uint64_t* cuts, uint32_t* n_pieces);

/* The same stage as data-parallel passes on the device: `d_text` = the file's bytes in HBM; the filtered bases
 * and their offsets stay in HBM, ready for cls_place_batch_device() (the reads never return to the host); the
 * headers are only needed by the output stage.  Synchronises `hip_stream` (the sizes of the outputs depend on
 * the text).  Buffers hold at least n_bases / n_header_bytes bytes and n + 1 offsets. */
typedef struct cls_fasta_dev {
    uint32_t n;
    uint32_t truncated;
    void* d_headers;          /* concatenated header bytes                      */
    void* d_header_off;       /* uint64 [n+1]                                   */
    void* d_bases;            /* concatenated filtered (upper-case ACGT) bases  */
    void* d_base_off;         /* uint64 [n+1]                                   */
    uint64_t n_header_bytes;
    uint64_t n_bases;
} cls_fasta_dev;
int cls_fasta_scan_device(const void* d_text, uint64_t len, cls_fasta_dev* out, void* hip_stream);
void cls_fasta_dev_free(cls_fasta_dev* f);
/* Host text in, host records out, through the device passes on `device` (-1: current). */
int cls_fasta_parse_gpu(const char* text, size_t len, int device, cls_fasta* out);
/* FASTA text -> placement records without the reads ever returning to the host: H2D of the file, the device
 * FASTA stage, cls_place_batch_device() on its output, D2H of the records (`*records`, free() it) and of the
 * headers (`fa`: n, truncated, headers, header_off; its bases / base_off stay NULL; cls_fasta_free() it).
 * Replaces mod.rs:108-159 (reader thread + channel + per-query place_sequence). */
int cls_place_fasta_text(cls_db* db, const char* text, size_t len, const cls_params* params, cls_fasta* fa,
                         cls_placement** records);

/* ---- FASTQ input stage, with quality trimming ------------------------------
 * Input: strict four-line FASTQ.  Lines end in "\n" or "\r\n" (the '\r' is stripped, as in the FASTA stage; a '\r'
 * that ends the text without a '\n' is kept); the last line may lack its newline.  A line exists iff it starts
 * before the end of the text.  Record r is lines 4r .. 4r+3, by line index alone, whatever the lines hold (a quality
 * line that starts with '@' or '+' is a quality line):
 *   1. "@header"   2. the sequence line   3. "+" and anything after it   4. the quality line
 * Record r is well-formed iff all four lines exist, line 1 starts with '@', the header (line 1 without its '@') is
 * non-empty and valid UTF-8, line 3 starts with '+', the sequence line is ASCII, and the quality line has as many
 * bytes as the sequence line, each in '!'..'~' (Phred+33).  Multi-line FASTQ shows up as a malformed record.
 * The parse emits records 0, 1, .. and stops at the first record that is not well-formed:
 *   - its line 1 is empty and every line from there on is empty: the text ends there cleanly (trailing blank lines);
 *   - otherwise (malformed, incomplete, or an empty line followed by a non-empty one): that record and everything
 *     after it are dropped and `truncated` = 1 (callers ignore it, like the FASTA stage's stop, mod.rs:119).
 * Quality trimming (the BWA / cutadapt `-q` rule), with q[i] = qual[i] - 33, L = the read length, and the cutoffs
 * c5 = trim_5p, c3 = trim_3p (0: that end is not trimmed; a cutoff above 93 acts like 94: every base goes):
 *   start: s = 0, best = 0, start = 0; for i = 0 .. L-1:   s += c5 - q[i]; if s < 0 stop; if s > best: best = s, start = i + 1
 *   stop:  s = 0, best = 0, stop = L;  for i = L-1 .. 0:   s += c3 - q[i]; if s < 0 stop; if s > best: best = s, stop = i
 *   start >= stop: the read is trimmed to empty; it is still emitted (and placed like an empty FASTA record).
 * Bases: the kept window [start, stop) of the sequence line, upper-cased, ACGT only (the FASTA filter,
 * sequence.rs:47-56).  Header bytes are kept as they are (a '>' included).
 * With both cutoffs 0, a well-formed text parses to the records of the FASTA stage on ">" header "\n" sequence "\n"
 * per record (headers without '>'), except that FASTA drops an empty last record (file_or_stdin.rs:111-113). */
typedef struct cls_fastq_opts {
    uint32_t trim_5p;         /* c5: 5' quality cutoff (0: off)                 */
    uint32_t trim_3p;         /* c3: 3' quality cutoff (0: off)                 */
    uint32_t reserved[6];     /* must be 0 (room for later options, 0 = off)    */
} cls_fastq_opts;             /* NULL wherever a `const cls_fastq_opts*` is taken: no trimming */

/* Host, sequential: the statement of the rules above.  Output as cls_fasta_parse (release with cls_fasta_free). */
int cls_fastq_parse(const char* text, size_t len, const cls_fastq_opts* opts, cls_fasta* out);
/* Host only: cut points as cls_fasta_split (same array contract).  A safe cut is the start of a record (a line
 * index that is a multiple of 4) whose preceding record is well-formed.  Concatenating the pieces' records, up to
 * and including the first piece that reports `truncated`, gives the records of the whole text. */
int cls_fastq_split(const char* text, size_t len, uint32_t max_pieces, uint64_t* cuts, uint32_t* n_pieces);
/* The same stage as data-parallel passes on the device, output as cls_fasta_scan_device (release with
 * cls_fasta_dev_free).  Synchronises `hip_stream` to learn the line count and the output sizes; the outputs are
 * complete in stream order on `hip_stream`. */
int cls_fastq_scan_device(const void* d_text, uint64_t len, const cls_fastq_opts* opts, cls_fasta_dev* out, void* hip_stream);
/* Host text in, host records out, through the device passes on `device` (-1: current). */
int cls_fastq_parse_gpu(const char* text, size_t len, const cls_fastq_opts* opts, int device, cls_fasta* out);
/* The FASTQ twin of cls_place_fasta_text: H2D of the file, the device FASTQ stage, placement on its output, D2H of
 * the records and headers (same outputs, same ownership). */
int cls_place_fastq_text(cls_db* db, const char* text, size_t len, const cls_params* params, const cls_fastq_opts* opts,
                         cls_fasta* fa, cls_placement** records);

/* ---- clade tally: placement records -> a per-clade abundance profile -------------
 * A tally is a small accumulator in the HBM of one handle's device.  Records are added to it batch after batch;
 * reading it gives one row per clade plus totals.  The counting rules, for a set of records and the tree of a handle:
 *   - status_count[s], s = 0 .. 11: records with that status.  n_reads: all records added.
 *   - a record is CLADE-BEARING iff its status is CLS_IDENTITY_FOUND, CLS_MAX_RESOLUTION or CLS_INCONCLUSIVE (the
 *     outcomes for which `clade_id` is set); for every other status `clade_id` is not looked at.
 *   - per clade v: n_identity, n_max_resolution, n_inconclusive = clade-bearing records with clade_id == id(v), by
 *     status; n_direct = their sum; n_clade = the sum of n_direct over v and every descendant of v; sum_one, sum_rest
 *     = the sums of `one` and `rest` over the CLS_IDENTITY_FOUND records of v only, as signed 64-bit sums.
 *   - a clade-bearing record whose clade_id is no clade of the tree counts in n_unknown_clade and in its
 *     status_count, in no row.  A record with status >= 12 counts in n_bad_status and in n_reads, nowhere else.
 *     Neither is an error: the entries take whatever bytes the caller's buffer holds (padding bytes are ignored).
 *   - every counter is 64 bits wide and everything is integer: adding is associative and commutative, the tally after
 *     adding batches A then B is the tally of their concatenation, in any order and any split, exactly.
 *   - rows come back in the row order of the cls_db_desc.nodes the handle was created from: row i describes nodes[i]
 *     and carries its id. */
typedef struct cls_tally cls_tally;   /* opaque; bound to one cls_db, lives on its device */
typedef struct cls_tally_row {
    uint64_t id;
    uint64_t n_clade;
    uint64_t n_direct;
    uint64_t n_identity;
    uint64_t n_max_resolution;
    uint64_t n_inconclusive;
    int64_t sum_one;
    int64_t sum_rest;
} cls_tally_row;                      /* 64 bytes */
typedef struct cls_tally_totals {
    uint64_t n_reads;
    uint64_t status_count[12];
    uint64_t n_unknown_clade;
    uint64_t n_bad_status;
} cls_tally_totals;                   /* 120 bytes */

/* A zeroed tally on the device of `db`.  It borrows the handle (a replica of a group included): destroy it first. */
int cls_tally_create(cls_db* db, cls_tally** out);
void cls_tally_destroy(cls_tally* t);
/* Waits for the adds in flight, then zeroes every counter. */
int cls_tally_reset(cls_tally* t);
/* `n` records already in the HBM of the handle's device (the d_out of cls_place_batch_device), 8-byte aligned;
 * asynchronous on `hip_stream`, in stream order behind whatever wrote them.  Adds on different streams may overlap. */
int cls_tally_add_device(cls_tally* t, const void* d_records, uint32_t n, void* hip_stream);
/* Host records: copied to the device and added by the same kernel; synchronous. */
int cls_tally_add(cls_tally* t, const cls_placement* records, uint32_t n);
/* Waits for the adds in flight; the subtree sums are made on the device.  `rows` holds n_rows = the tree's n_nodes
 * entries; `rows` (with n_rows = 0) or `totals` may be NULL. */
int cls_tally_read(cls_tally* t, cls_tally_row* rows, uint32_t n_rows, cls_tally_totals* totals);
/* Host only, sequential, no device: the statement of the rules above and the yardstick of the kernel.  Takes the tree
 * as cls_db_create takes it.  rows[n_nodes] and `totals` are ADDED to (the caller zeroes them before the first call;
 * row ids are set), so the call also merges: the tallies of the replicas of an index group are summed by adding
 * each one's rows and totals (see cls_tally_merge). */
int cls_tally_host(const cls_node* nodes, uint32_t n_nodes, const cls_placement* records, uint64_t n,
                   cls_tally_row* rows, cls_tally_totals* totals);
/* rows[i] += add_rows[i] for n_rows rows (ids must agree, or the target's are 0 and are set), totals += add_totals. */
int cls_tally_merge(cls_tally_row* rows, cls_tally_totals* totals, const cls_tally_row* add_rows,
                    const cls_tally_totals* add_totals, uint32_t n_rows);
/* Query text -> tally; nothing per read returns to the host: H2D of the text, the device FASTA / FASTQ stage,
 * placement, cls_tally_add_device on its output.  *n = records placed, *truncated as cls_fasta.truncated (either
 * may be NULL).  Synchronous. */
int cls_tally_fasta_text(cls_db* db, cls_tally* t, const char* text, size_t len, const cls_params* params,
                         uint32_t* n, uint32_t* truncated);
int cls_tally_fastq_text(cls_db* db, cls_tally* t, const char* text, size_t len, const cls_params* params,
                         const cls_fastq_opts* opts, uint32_t* n, uint32_t* truncated);

/* ---- paired reads: the two mates' placements -> one record per pair ------------------------
 * Inputs: two record sequences, mate 1 = a[i * stride], mate 2 = b[i * stride] for i < n, stride 1 or 2.  Stride 2 with
 * b = a + 1 is an interleaved batch; stride 1 with b = a + n is "all of R1, then all of R2".  Outputs: one cls_placement
 * P[i] per pair (same layout: the tally, cls_serialize_results and the clade report work on P unchanged) and one class
 * byte how[i].  Integer-only and exact:
 *   - a mate is USABLE iff its status is CLS_IDENTITY_FOUND, CLS_MAX_RESOLUTION or CLS_INCONCLUSIVE and its clade_id is
 *     a clade of the tree.  A status >= 12, another status or an unknown id makes it not usable; none is an error.
 *   - "copy" = the fields status, one, rest, levels, clade_id; the pad bytes of P are always written as 0.
 *   how                                   condition                                   P
 *   CLS_PAIR_NEITHER                      neither mate usable                         copy of mate 1
 *   CLS_PAIR_ONLY_1 / CLS_PAIR_ONLY_2     exactly that mate usable                    copy of the usable mate
 *   CLS_PAIR_SAME                         both usable, same clade                     copy of the mate with the lower status
 *                                                                                     value, then the larger `one`, then the
 *                                                                                     smaller `rest`, then mate 1
 *   CLS_PAIR_NESTED_1 / CLS_PAIR_NESTED_2 both usable, that mate's clade is a proper  copy of the descendant mate
 *                                         descendant of the other's
 *   CLS_PAIR_DISCORDANT                   both usable, neither clade holds the other  status = CLS_MAX_RESOLUTION, clade_id =
 *                                                                                     id(LCA), one = rest = 0, levels = depth
 *                                                                                     of the LCA in edges below the root
 * Flags change P only, never `how`.  CLS_PAIR_CONSERVATIVE: in the NESTED classes copy the ancestor mate instead.
 * CLS_PAIR_REQUIRE_BOTH: in the ONLY classes copy the mate that is NOT usable (the pair stays unplaced).  Any other
 * flag bit is CLS_E_INVALID_ARG.
 * Totals: 64-bit counters, associative over batches like the tally's. */
enum {
    CLS_PAIR_NEITHER = 0,
    CLS_PAIR_ONLY_1 = 1,
    CLS_PAIR_ONLY_2 = 2,
    CLS_PAIR_SAME = 3,
    CLS_PAIR_NESTED_1 = 4,
    CLS_PAIR_NESTED_2 = 5,
    CLS_PAIR_DISCORDANT = 6
};
#define CLS_PAIR_CONSERVATIVE 1u
#define CLS_PAIR_REQUIRE_BOTH 2u

typedef struct cls_pair_totals {
    uint64_t n_pairs;
    uint64_t how_count[8];            /* per CLS_PAIR_* class; entry 7 is unused, always 0 */
} cls_pair_totals;                    /* 72 bytes */

typedef struct cls_pairer cls_pairer; /* opaque; bound to one cls_db (a replica of a group included), lives on its device */

/* A pairer with zeroed totals on the device of `db`.  It borrows the handle, like cls_tally: destroy it first. */
int cls_pairer_create(cls_db* db, cls_pairer** out);
void cls_pairer_destroy(cls_pairer* p);
/* Waits for the launches in flight; `reset` != 0 zeroes the totals afterwards. */
int cls_pairer_totals(cls_pairer* p, cls_pair_totals* totals, int reset);
/* Records in the HBM of the handle's device, 8-byte aligned; stride 2 needs d_b = d_a + one record.  Asynchronous on
 * `hip_stream`, in stream order; calls on different streams may overlap.  `d_out` (n records) must not alias the
 * inputs; `d_how` (n bytes) may be NULL.  The classes are added to the pairer's totals. */
int cls_pair_records_device(cls_pairer* p, const void* d_a, const void* d_b, uint32_t stride, uint32_t n, uint32_t flags,
                            void* d_out, void* d_how, void* hip_stream);
/* Host buffers through the same kernel; synchronous.  `how` may be NULL. */
int cls_pair_records(cls_pairer* p, const cls_placement* a, const cls_placement* b, uint32_t stride, uint32_t n, uint32_t flags,
                     cls_placement* out, uint8_t* how);
/* Host only, sequential, no device: the statement of the rules above and the yardstick of the kernel.  The tree as
 * cls_tally_host takes it.  `how` may be NULL; `totals` (may be NULL) is ADDED to. */
int cls_pair_host(const cls_node* nodes, uint32_t n_nodes, const cls_placement* a, const cls_placement* b, uint32_t stride,
                  uint64_t n, uint32_t flags, cls_placement* out, uint8_t* how, cls_pair_totals* totals);

/* Mate names.  The name of a header is its bytes up to the first space or tab; if that ends in "/1" or "/2", those two
 * bytes are dropped.  A pair agrees iff the two names are byte-equal (the suffixes are not checked against the mate's
 * position).  Header of mate m of pair i: bytes [off_m[i * stride], off_m[i * stride + 1]) of headers_m -- two header
 * sets with stride 1, or one interleaved set with stride 2 and off2 = off1 + 1.  *n_bad = disagreeing pairs,
 * *first_bad = the lowest disagreeing index (UINT64_MAX if none). */
int cls_pair_names_host(const char* headers1, const uint64_t* off1, const char* headers2, const uint64_t* off2, uint32_t stride,
                        uint64_t n, uint64_t* n_bad, uint64_t* first_bad);
/* Its device twin: the arrays are in the HBM of the current device (cls_fasta_dev of the FASTQ stage); synchronises
 * `hip_stream` to hand the two results back. */
int cls_pair_names_device(const void* d_headers1, const void* d_off1, const void* d_headers2, const void* d_off2, uint32_t stride,
                          uint32_t n, uint64_t* n_bad, uint64_t* first_bad, void* hip_stream);

/* Paired FASTQ text -> one record per pair.  `text2` == NULL: `text1` is interleaved (records 2 i and 2 i + 1 are the
 * mates of pair i).  Both texts go to the device once; the FASTQ stage runs on each (one scan for interleaved input);
 * all 2 n reads are placed as ONE cls_place_batch_device batch (R1's bases then R2's, or the interleaved batch as it
 * is); then the name check and the pairing kernel.  Only mate 1's headers (`fa`: n = pairs, truncated, headers,
 * header_off; cls_fasta_free() it), P (`*records`) and `*how` (may be NULL; free() both) return to the host.  The
 * classes are added to the totals of `p`.  CLS_E_BAD_PAIRS: the two texts hold different numbers of records, an odd
 * interleaved count, more than 2^31 - 1 pairs, or a pair whose names disagree (the message carries the lowest such pair
 * index and both names). */
int cls_place_fastq_pairs_text(cls_db* db, cls_pairer* p, const char* text1, size_t len1, const char* text2, size_t len2,
                               const cls_params* params, const cls_fastq_opts* opts, uint32_t flags, cls_fasta* fa,
                               cls_placement** records, uint8_t** how);
/* The same pipeline into a tally: P is added to `tally` on the device, nothing per read returns.  *n_pairs,
 * *truncated may be NULL. */
int cls_tally_fastq_pairs_text(cls_db* db, cls_pairer* p, cls_tally* tally, const char* text1, size_t len1, const char* text2,
                               size_t len2, const cls_params* params, const cls_fastq_opts* opts, uint32_t flags,
                               uint32_t* n_pairs, uint32_t* truncated);

/* ---- read extraction: placement records -> the selected reads' original FASTQ text ------------------------------
 * Selection.  A selector is a list of INCLUDE clade ids, a list of EXCLUDE clade ids and flags, against the tree of a
 * handle.  A record is PLACED iff its status is CLS_IDENTITY_FOUND, CLS_MAX_RESOLUTION or CLS_INCONCLUSIVE and its
 * clade_id is a clade of the tree (the pairing rule's "usable"); every other record is UNPLACED -- a status >= 12 and
 * an unknown id included; none is an error.
 *   - a placed record at clade v is selected iff the NEAREST listed clade on the path v -> root, v included, is an
 *     include; with no listed clade on the path it is not selected.  So "include X, exclude Y below X, include Z below
 *     Y" means what it reads.
 *   - an unplaced record is selected iff CLS_SELECT_UNPLACED is set.
 *   - CLS_E_INVALID_ARG: an id listed twice or in both lists, an id that is no clade of the tree, an unknown flag bit.
 *     Empty lists are fine: no include + CLS_SELECT_UNPLACED is "the unplaced reads only"; include root + exclude X
 *     is "everything placed outside X".
 * Record text.  For the n records the FASTQ stage emits, record r is the bytes of lines 4r .. 4r+3 of the text as they
 * are: '@', '+', the quality line and any '\r' stay, nothing is trimmed or filtered (quality trimming decides the
 * placement, not the bytes written).  The spans are contiguous: record r = [rec_off[r], rec_off[r+1]), rec_off[r] = the
 * start of line 4r, rec_off[n] = the start of line 4n, or `len` if the text ends inside line 4n-1.
 * Items.  With `stride` s (1 or 2), item i covers [rec_off[i s], rec_off[(i+1) s]); s = 2 is an interleaved pair, both
 * mates as they stand in the file.
 * Output.  The bytes of the selected items in input order, concatenated; an item whose last byte is not '\n' gets one
 * '\n' appended (only the last record of a text without a final newline); a zero-length item emits nothing.
 * Totals per call, all 64-bit: n_records (items looked at), n_selected, n_selected_unplaced (the selected items whose
 * record is unplaced; the plan and cls_extract_host see selection bytes, not records, and report 0), bytes_out. */
typedef struct cls_selector cls_selector;      /* opaque; bound to one cls_db (a replica of a group included), lives on its device */
#define CLS_SELECT_UNPLACED 1u
typedef struct cls_extract_totals {
    uint64_t n_records;
    uint64_t n_selected;
    uint64_t n_selected_unplaced;
    uint64_t bytes_out;
} cls_extract_totals;                          /* 32 bytes */

/* A selector on the device of `db`.  It borrows the handle, like cls_tally: destroy it first.  Immutable: any number of
 * launches may use it at once. */
int cls_selector_create(cls_db* db, const uint64_t* include, uint32_t n_include, const uint64_t* exclude, uint32_t n_exclude,
                        uint32_t flags, cls_selector** out);
void cls_selector_destroy(cls_selector* s);
/* `n` records in the HBM of the handle's device (8-byte aligned, as the tally takes them) -> one byte per record in
 * `d_sel`: 1 selected, 0 not.  Asynchronous on `hip_stream`. */
int cls_select_records_device(cls_selector* s, const void* d_records, uint32_t n, void* d_sel, void* hip_stream);
/* Host buffers through the same kernel; synchronous. */
int cls_select_records(cls_selector* s, const cls_placement* records, uint32_t n, uint8_t* sel);
/* Host only, sequential, no device: the statement of the selection rule and the yardstick of the kernel.  The tree as
 * cls_tally_host takes it. */
int cls_select_host(const cls_node* nodes, uint32_t n_nodes, const uint64_t* include, uint32_t n_include,
                    const uint64_t* exclude, uint32_t n_exclude, uint32_t flags,
                    const cls_placement* records, uint64_t n, uint8_t* sel);

/* rec_off[n + 1] (uint64) of the first n records of a FASTQ text in HBM (n = what cls_fastq_scan_device reported for
 * it); the line structure alone decides, whatever the lines hold.  Synchronises `hip_stream`. */
int cls_fastq_spans_device(const void* d_text, uint64_t len, uint32_t n, void* d_rec_off, void* hip_stream);

/* The compaction in two steps, every buffer in the HBM of the current device, `d_sel` one byte per ITEM.
 * plan: d_out_off[n_items + 1] (uint64) = the exclusive sum of the emitted lengths (0 for items that are not selected);
 * synchronises `hip_stream` to return the sizes.  gather: copies; asynchronous; `d_out` holds totals->bytes_out bytes
 * (any alignment) and must not alias the text; it writes those bytes and nothing else. */
int cls_extract_plan_device(const void* d_text, const void* d_rec_off, uint32_t stride, uint32_t n_items, const void* d_sel,
                            void* d_out_off, cls_extract_totals* totals, void* hip_stream);
int cls_extract_gather_device(const void* d_text, const void* d_rec_off, uint32_t stride, uint32_t n_items, const void* d_sel,
                              const void* d_out_off, void* d_out, void* hip_stream);
/* Host only, sequential, no device: record text + items + output as stated above, from host text and one selection byte
 * per item (it finds the lines itself; `n_items` = the emitted records / stride).  *out: malloc'ed, free() it. */
int cls_extract_host(const char* text, size_t len, uint32_t stride, const uint8_t* sel, uint64_t n_items, char** out, size_t* out_len,
                     cls_extract_totals* totals);

/* Query text -> extracted text: the text goes to the device once (and stays there until the gather), the FASTQ stage,
 * placement, the selection kernel on the records, plan + gather; only the selected bytes come back.  `tally` (may be
 * NULL) receives the records on the device as in cls_tally_fastq_text.  *out: malloc'ed, free() it.  *n, *truncated as
 * there (either may be NULL).  Synchronous. */
int cls_extract_fastq_text(cls_db* db, cls_selector* s, cls_tally* tally, const char* text, size_t len, const cls_params* params,
                           const cls_fastq_opts* opts, char** out, size_t* out_len, cls_extract_totals* totals,
                           uint32_t* n, uint32_t* truncated);
/* Pairs: the pair's record P (the pairing rule above with `flags`) decides for BOTH mates.  `text2` != NULL: *out1 /
 * *out2 get R1's / R2's records of the selected pairs, in step.  `text2` == NULL (interleaved): *out1 gets both mates of
 * each selected pair, *out2 stays NULL (`out2`, `out2_len` may be NULL).  The totals count pairs; bytes_out is the sum
 * over both outputs.  `tally` (may be NULL) receives P.  Refusals as cls_place_fastq_pairs_text (CLS_E_BAD_PAIRS). */
int cls_extract_fastq_pairs_text(cls_db* db, cls_pairer* p, cls_selector* s, cls_tally* tally, const char* text1, size_t len1,
                                 const char* text2, size_t len2, const cls_params* params, const cls_fastq_opts* opts, uint32_t flags,
                                 char** out1, size_t* out1_len, char** out2, size_t* out2_len, cls_extract_totals* totals,
                                 uint32_t* n_pairs, uint32_t* truncated);

/* Experiment knobs (grid sizes, locality-key definition, kernel family; none changes a result; names in
 * csrc/cls_tuning.h are the CLS_* variables in lower case without the prefix, e.g. "no_order").  Process-global,
 * meant for A/B runs: the library itself never reads the environment.  cls_tuning_from_env() takes every knob
 * from its CLS_* variable, once, when a tool asks for it.  Set knobs before creating handles. */
int cls_set_tuning(const char* name, int value);
void cls_tuning_from_env(void);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* cls_last_error(void);

/* "classeq2_amd <version> gfx950 abi<N>" */
const char* cls_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CLS_PLACE_H */
