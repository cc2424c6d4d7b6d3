/*
 * cls_host.h -- host-side mirror of the reference's batch driver (part of libclsplace.so).
 *
 * The reference's `place_sequences` (core/src/use_cases/place_sequences/mod.rs:43-270) reads a
 * multi-FASTA, places every record and appends one YAML document or JSON line per record to
 * `<out>.yaml|.jsonl`, per-query errors to `<out>.error`.  These entry points do the same above the
 * GPU path, for callers that do not keep the Rust front-end (the C++ `cls-place` tool in csrc/ is one).
 * Tree / index / annotations come from the reference's own file formats:
 *   - database: the JSON export of `cls convert database -f json` (ports/cli/src/cmds/convert.rs:161-205);
 *   - annotations: the YAML list of `Annotation` (core/src/domain/dtos/annotation.rs:25-34).
 */
#ifndef CLS_HOST_H
#define CLS_HOST_H

#include "cls_place.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cls_tree cls_tree; /* Tree: root clade (+ names, supports, lengths), annotations, k-mer map */

enum { CLS_FORMAT_YAML = 0, CLS_FORMAT_JSONL = 1 }; /* OutputFormat, core/src/domain/dtos/output_format.rs:3-11 */

/* Parse a database (or `--only-tree`) JSON export.  Replaces load_database
 * (ports/lib/src/functions/load_database.rs:9-53) for the JSON form. */
int cls_tree_load_json(const char* path, cls_tree** out);
void cls_tree_free(cls_tree* t);
/* Tree::init_from_file (core/src/domain/dtos/tree.rs:164-230): parse a rooted Newick tree (.nwk/.newick/.tree),
 * node ids = pre-order of the text (what the phylotree arena yields), internal labels = support values, then
 * sanitize (tree.rs:252-291: a clade whose support is below `min_branch_support` hands its children to its
 * parent) and fix_parent_ids.  Tree.name = the file name, Tree.id = UUID v3 (DNS namespace) of it. */
int cls_tree_init_from_file(const char* tree_path, double min_branch_support, cls_tree** out);
/* The same from text already in memory (`tree_name` NULL: "UnnamedTree"). */
int cls_tree_from_newick(const char* newick_text, const char* tree_name, double min_branch_support, cls_tree** out);
/* load_database (ports/lib/src/functions/load_database.rs:9-53): a `.cls` file (zstd-compressed YAML, needs the
 * system's libzstd.so.1 at run time), plain YAML, or the JSON export; a whole database or an `--only-tree` file;
 * also the k-mer-keyed map of databases written before the minimizer buckets existed. */
int cls_tree_load(const char* path, cls_tree** out);
/* `cls convert database -f {zstd|yaml|json} [--only-tree]` (ports/cli/src/cmds/convert.rs:161-205) and the file
 * `cls build-db` writes (ports/cli/src/cmds/build_db.rs:70-76): serde_yaml / serde_json::to_writer_pretty of the
 * Tree (or of its root clade).  cls_tree_save forces the reference's extensions (.cls / .cls.yaml / .cls.json). */
#define CLS_DB_FORMAT_ZSTD 0
#define CLS_DB_FORMAT_YAML 1
#define CLS_DB_FORMAT_JSON 2
int cls_tree_serialize(const cls_tree* t, int format, int only_tree, char** out, size_t* out_len); /* cls_host_free(*out) */
int cls_tree_save(const cls_tree* t, const char* path, int format, int only_tree);
/* `-a/--annotations-file-path` of `cls place` (ports/cli/src/cmds/place_sequences.rs:137-144). */
int cls_tree_set_annotations_yaml(cls_tree* t, const char* path);
/* `cls build-db` on an already parsed tree: map_kmers_to_tree (core/src/use_cases/build_database/mod.rs:26-181).
 * `msa_text` is the multi-FASTA whose headers name the tree's leaves.  Replaces the tree's k-mer map. */
#define CLS_BUILD_REFERENCE_HEADER_SHIFT 1u /* file record i's k-mers under header i+1, never index the last record
                                             * (what the reference does, build_database/mod.rs:93-116) */
/* CLS_BUILD_FORWARD_ONLY, CLS_BUILD_LEAVES_ONLY: cls_place.h.  With CLS_BUILD_LEAVES_ONLY the tree keeps the map as
 * CLS_SETS_LEAVES (cls_tree_desc reports it); the reference's file format holds explicit sets, so cls_tree_serialize
 * and cls_tree_save then refuse unless `only_tree`. */
int cls_tree_build_kmers_map(cls_tree* t, const char* msa_text, size_t msa_len, uint64_t k_size, uint64_t m_size,
                             uint32_t flags);
/* The same on the GPU `device` (-1: the current one): the MSA text goes through the device FASTA stage, only its
 * headers come back to be matched to leaves (as above, same errors), and cls_kmers_build makes the map.  The map is
 * byte for byte the one cls_tree_build_kmers_map makes.  k_size at most 1024. */
int cls_tree_build_kmers_map_device(cls_tree* t, const char* msa_text, size_t msa_len, uint64_t k_size, uint64_t m_size,
                                    uint32_t flags, int device);
/* Borrowed flat view for cls_db_create(); valid while `t` lives. */
int cls_tree_desc(const cls_tree* t, cls_db_desc* d);

/* PlacementResponse serialisation (mod.rs:170-248, placement_response.rs:30-94): one YAML document
 * ("---\n" + mapping) or one JSON line per non-error record, in input order; the messages of error
 * records concatenated as the reference appends them to `<out>.error`.  Buffers are malloc'ed; release
 * them with cls_host_free().  `err_text` may be NULL. */
int cls_serialize_results(const cls_tree* t, const char* headers, const uint64_t* header_off, uint32_t n,
                          const cls_placement* recs, int format, char** out_text, size_t* out_len,
                          char** err_text, size_t* err_len);
void cls_host_free(void* p);

/* The whole use-case: FASTA (`query_path`, "-" = stdin) -> placements on the GPU -> result + error files.
 * `out_file` gets its extension replaced like PathBuf::set_extension (mod.rs:76-81); `overwrite` is
 * `--force-overwrite`.  Returns the number of records read and the UCPLACE0001->0002 wall time. */
int cls_place_sequences(cls_db* db, const cls_tree* t, const char* query_path, const char* out_file,
                        const cls_params* params, int overwrite, int format, uint32_t* n_placed, double* seconds);
/* The same use-case on an index group: the text is cut with cls_fasta_split into one piece per replica, each
 * replica runs cls_place_fasta_text on its piece on a host thread of its own, and the pieces' headers and records are
 * joined in input order (up to the first piece that stops early) before the output stage.  The files are
 * byte-identical to those of cls_place_sequences on one handle. */
int cls_place_sequences_group(cls_db_group* g, const cls_tree* t, const char* query_path, const char* out_file,
                              const cls_params* params, int overwrite, int format, uint32_t* n_placed, double* seconds);

/* The same two use-cases for either query format.  CLS_QUERY_FASTA: exactly cls_place_sequences[_group] (`fastq`
 * must then be NULL or all zero).  CLS_QUERY_FASTQ: the query is strict four-line FASTQ (cls_place.h), parsed and
 * quality-trimmed by `fastq` (NULL: no trimming) on the device with cls_place_fastq_text; the group form cuts the
 * text with cls_fastq_split.  The output stage is the same for both formats. */
enum { CLS_QUERY_FASTA = 0, CLS_QUERY_FASTQ = 1 };
int cls_place_sequences_ex(cls_db* db, const cls_tree* t, const char* query_path, const char* out_file, const cls_params* params,
                           int overwrite, int format, int query_format, const cls_fastq_opts* fastq, uint32_t* n_placed,
                           double* seconds);
int cls_place_sequences_group_ex(cls_db_group* g, const cls_tree* t, const char* query_path, const char* out_file,
                                 const cls_params* params, int overwrite, int format, int query_format,
                                 const cls_fastq_opts* fastq, uint32_t* n_placed, double* seconds);

/* Borrowed node table of the tree (the `nodes` of cls_tree_desc), also for a tree-only file; valid while `t` lives. */
int cls_tree_nodes(const cls_tree* t, const cls_node** nodes, uint32_t* n_nodes);

/* ---- clade report: the per-clade abundance profile of a run (the clade tally of cls_place.h as a text file) ------
 * `rows` = one cls_tally_row per row of the tree's node table (cls_tree_desc order: what cls_tally_read and
 * cls_tally_host give for it), `totals` with them.  Tab-separated text, "\n" line ends (release with cls_host_free):
 *   # classeq2_amd clade report v1
 *   # reads\t<n_reads>
 *   # status\t<NAME>\t<count>            twelve lines, in enum order (UNCLASSIFIABLE_NO_MATCH .. ERR_READ_TOO_LONG)
 *   # unknown_clade\t<n>
 *   # bad_status\t<n>
 *   clade_id\tparent_id\tkind\tdepth\tname\tn_clade\tn_direct\tn_identity\tn_max_resolution\tn_inconclusive\tmean_one\tmean_rest
 *   one line per clade in DFS pre-order (children in Clade.children order); without `all_rows` only the clades with
 *   n_clade > 0.  parent_id: "-" for the root; kind: ROOT / NODE / LEAF; depth: levels below the root; name: the
 *   clade's name or empty; mean_one / mean_rest: sum / n_identity with "%.3f", or "-" when n_identity is 0. */
int cls_tally_report(const cls_tree* t, const cls_tally_row* rows, const cls_tally_totals* totals, int all_rows,
                     char** out_text, size_t* out_len);
/* Query file -> clade report, nothing per read leaves the device: the query (`query_path`, "-" = stdin) is cut with
 * cls_fasta_split / cls_fastq_split into pieces of about `piece_bytes` (0: 64 MiB), each piece goes through
 * cls_tally_fasta_text / cls_tally_fastq_text into ONE tally (device memory is bounded by the piece, not by the file),
 * the pieces after the first one that stops early (`truncated`) are dropped as cls_place_sequences_group drops them,
 * and the report is written to `report_path` (no extension is forced; an existing file needs `overwrite`).
 * `n_placed`: records tallied.  `seconds`: read + place + write.  query_format / fastq as cls_place_sequences_ex. */
int cls_profile_sequences(cls_db* db, const cls_tree* t, const char* query_path, const char* report_path,
                          const cls_params* params, int overwrite, int query_format, const cls_fastq_opts* fastq,
                          uint64_t piece_bytes, int all_rows, uint32_t* n_placed, double* seconds);
/* The same on an index group: piece i goes to replica i mod N, every replica on a host thread of its own with a tally
 * of its own; the replicas' rows and totals are summed with cls_tally_merge.  The report is byte-identical to the
 * one of cls_profile_sequences. */
int cls_profile_sequences_group(cls_db_group* g, const cls_tree* t, const char* query_path, const char* report_path,
                                const cls_params* params, int overwrite, int query_format, const cls_fastq_opts* fastq,
                                uint64_t piece_bytes, int all_rows, uint32_t* n_placed, double* seconds);
/* cls_place_sequences_ex / cls_place_sequences_group_ex (exactly one of `db`, `g` is non-NULL) that also write the
 * clade report of the run to `report_path`, counted on the host (cls_tally_host) from the records the run has anyway:
 * no second placement.  The report is byte-identical to the one cls_profile_sequences writes for the same input. */
int cls_place_sequences_report(cls_db* db, cls_db_group* g, const cls_tree* t, const char* query_path, const char* out_file,
                               const cls_params* params, int overwrite, int format, int query_format,
                               const cls_fastq_opts* fastq, const char* report_path, int all_rows, uint32_t* n_placed,
                               double* seconds);

/* ---- paired-end use-case: FASTQ mate files -> one placement per pair ----------------------------------------------
 * `query1` / `query2`: the R1 / R2 files; `query2` == NULL: `query1` is interleaved.  The reads go through
 * cls_place_fastq_pairs_text (cls_place.h "paired reads": one placement batch, the mate-name check, the pairing rule
 * with `flags`) on one handle.  Every output is optional (at least one is needed):
 *   out_file      per-pair result + error files through the existing serialiser, under mate 1's headers as they are
 *                 (extension and overwrite policy as cls_place_sequences);
 *   report_path   the clade report (cls_tally_report) over the tally of the pairs' records -- a fragment counts once;
 *   summary_path  tab-separated "name\tcount" lines: n_pairs, then NEITHER, ONLY_1, ONLY_2, SAME, NESTED_1, NESTED_2,
 *                 DISCORDANT.
 * Without `out_file` nothing per pair leaves the device (cls_tally_fastq_pairs_text).  Mates that do not line up:
 * CLS_E_BAD_PAIRS.  `n_pairs`, `seconds` may be NULL. */
int cls_place_pairs(cls_db* db, const cls_tree* t, const char* query1, const char* query2, const char* out_file,
                    const char* report_path, const char* summary_path, const cls_params* params, const cls_fastq_opts* opts,
                    uint32_t flags, int format, int overwrite, int all_rows, uint32_t* n_pairs, double* seconds);

/* ---- read extraction use-case: FASTQ file(s) -> the FASTQ records of the reads placed where the selector says -------
 * The selector (cls_place.h "read extraction") is `include` / `exclude` / `select_flags`.
 * Single-end (`query2` NULL, `interleaved` 0; `query1` "-" = stdin): the query is cut with cls_fastq_split into pieces of
 * about `piece_bytes` (0: 64 MiB) as cls_profile_sequences does, each piece goes through cls_extract_fastq_text with ONE
 * selector (and one tally when `report_path` is given), each piece's output is appended to `extract_path1`, the pieces
 * after the first truncated one are dropped: device and host memory are bounded by the piece.
 * Paired (`query2` = the R2 file, or `interleaved`): whole files through cls_extract_fastq_pairs_text with `pair_flags`,
 * as cls_place_pairs; with `query2`, `extract_path2` gets R2's records (both or neither); `summary_path` as there.
 * `report_path` (may be NULL): the clade report of the same pass (of the pairs' records for paired input).  An existing
 * file needs `overwrite`.  One JSON line of totals goes to stderr.  `totals`, `n_placed` (records, or pairs), `seconds`
 * may be NULL. */
int cls_extract_reads(cls_db* db, const cls_tree* t, const char* query1, const char* query2, int interleaved,
                      const uint64_t* include, uint32_t n_include, const uint64_t* exclude, uint32_t n_exclude, uint32_t select_flags,
                      const char* extract_path1, const char* extract_path2, const char* report_path, const char* summary_path,
                      const cls_params* params, const cls_fastq_opts* opts, uint32_t pair_flags, int overwrite, int all_rows,
                      uint64_t piece_bytes, cls_extract_totals* totals, uint32_t* n_placed, double* seconds);

const char* cls_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
