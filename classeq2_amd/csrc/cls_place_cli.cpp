// cls-place: C++ look-alike of the reference's `cls place` sub-command
// (ports/cli/src/cmds/place_sequences.rs:18-82 flag surface, :84-223 behaviour) on the GPU path.
//   cls-place [QUERY|-] -d DB -o OUT [-a ANNOTATIONS.yaml] [--out-format yaml|jsonl]
//             [-i N] [-m COV] [-r] [-f] [--device N[,N...]] [--query-format fasta|fastq] [-q [5P,]3P]
//             [--report PATH | --report-only PATH] [--report-all-clades]
//             [-2 MATES | --interleaved] [--pair-mode deepest|conservative] [--pair-require-both] [--pair-summary PATH]
//             [--extract-out FILE [--extract-out2 FILE] [--extract-clade ID[,ID...]] [--extract-exclude ID[,ID...]] [--extract-unplaced]]
// --extract-out writes the FASTQ records of the reads (or pairs) placed where the --extract-... options say, instead of
// per-read results (include/cls_host.h "read extraction").
// -2 / --interleaved place paired-end FASTQ: one result per pair, under mate 1's header (include/cls_host.h).
// --report also writes the per-clade abundance profile of the run (include/cls_host.h "clade report"); --report-only
// writes nothing else: the reads are tallied on the device and no per-read output exists (-o is then not needed).
// The database is read like load_database does (ports/lib/src/functions/load_database.rs:9-53): the `.cls`
// file of `cls build-db` (zstd-compressed YAML), plain YAML, or the JSON export.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cls_host.h"

static void usage() {
    fprintf(stderr,
            "Usage: cls-place [QUERY] --database-file-path <DB> --output-file-path <OUT> [OPTIONS]\n\n"
            "Arguments:\n  [QUERY]  multi-FASTA (or, with --query-format fastq, FASTQ) file, or \"-\" for STDIN [default: -]\n\n"
            "Options:\n"
            "  -d, --database-file-path <PATH>     classeq database (.cls, .cls.yaml or .cls.json)\n"
            "  -o, --output-file-path <PATH>       output file (extension replaced by .yaml / .jsonl; errors go to .error)\n"
            "  -a, --annotations-file-path <PATH>  annotations in YAML format\n"
            "      --out-format <yaml|jsonl>       [default: yaml]\n"
            "  -i, --iterations <N>                maximum number of tree levels [default: 1000]\n"
            "  -m, --match-coverage <F>            minimum match coverage [default: 0.7]\n"
            "  -r, --remove-intersection           one-vs-rest without the shared k-mers\n"
            "  -f, --force-overwrite               overwrite an existing output file\n"
            "      --device <N[,N...]>             GPU ordinal [default: 0]; a comma list places on one replica of the\n"
            "                                      index per entry (repeats allowed)\n"
            "      --query-format <fasta|fastq>    format of QUERY [default: fasta]; fastq = strict four-line FASTQ, Phred+33\n"
            "  -q, --trim-quality <[5P,]3P>        fastq only: trim low-quality ends (BWA / cutadapt -q rule); one value\n"
            "                                      trims the 3' end, two values the 5' and the 3' end [default: 0,0 = off]\n"
            "      --report <PATH>                 also write the clade report: reads per clade (exactly at it / at or below\n"
            "                                      it), per status, unplaced reads by reason (tab-separated text)\n"
            "      --report-only <PATH>            write only the clade report: the reads are counted on the GPU, no per-read\n"
            "                                      result or .error file is written and -o is not required\n"
            "      --report-all-clades             list every clade in the report, not only those with reads\n"
            "  -2, --mate-file <PATH>              fastq only: QUERY holds the first mates, PATH the second; one result per pair\n"
            "      --interleaved                   fastq only: QUERY holds the pairs' mates in turn\n"
            "      --pair-mode <deepest|conservative>  mates placed at a clade and at its ancestor: keep the deeper one, or\n"
            "                                      the ancestor [default: deepest]\n"
            "      --pair-require-both             leave a pair unplaced unless both mates are placed\n"
            "      --pair-summary <PATH>           write the pair classes (tab-separated name, count)\n"
            "      --extract-out <FILE>            fastq only: write the reads selected below, as they stand in QUERY, instead of\n"
            "                                      per-read results (no -o); --report / --report-only still write the report\n"
            "      --extract-out2 <FILE>           with -2: the second mates of the selected pairs\n"
            "      --extract-clade <ID[,ID...]>    select the reads placed at or below these clades (Clade.id, decimal)\n"
            "      --extract-exclude <ID[,ID...]>  but not those at or below these; the nearest listed clade above a read decides\n"
            "      --extract-unplaced              select the reads that were not placed\n");
}

// cutadapt's -q: "3P" or "5P,3P", each a cutoff in 0 .. 2^31 - 1
static bool parse_cutoffs(const std::string& v, uint32_t* c5, uint32_t* c3) {
    const size_t comma = v.find(',');
    auto one = [](const std::string& x, uint32_t* c) {
        if (x.empty() || x.size() > 10 || x.find_first_not_of("0123456789") != std::string::npos) return false;
        const unsigned long long n = strtoull(x.c_str(), nullptr, 10);
        if (n > 0x7FFFFFFFull) return false;
        *c = (uint32_t)n;
        return true;
    };
    if (comma == std::string::npos) { *c5 = 0; return one(v, c3); }
    return one(v.substr(0, comma), c5) && one(v.substr(comma + 1), c3);
}

// "ID[,ID...]": decimal Clade.id values
static bool parse_ids(const std::string& v, std::vector<uint64_t>* ids) {
    for (size_t p0 = 0; p0 <= v.size();) {
        size_t p1 = v.find(',', p0);
        if (p1 == std::string::npos) p1 = v.size();
        const std::string x = v.substr(p0, p1 - p0);
        if (x.empty() || x.size() > 20 || x.find_first_not_of("0123456789") != std::string::npos) return false;
        if (x.size() == 20 && x > "18446744073709551615") return false;
        ids->push_back(strtoull(x.c_str(), nullptr, 10));
        p0 = p1 + 1;
    }
    return true;
}

int main(int argc, char** argv) {
    std::string query = "-", db_path, out_path, ann_path, fmt = "yaml";
    cls_params p;
    memset(&p, 0, sizeof p);
    int overwrite = 0, device = 0;
    std::vector<int> devices;  // --device with a comma: an index group, one replica per entry
    std::string qfmt = "fasta", trim, report, report_only;
    int all_rows = 0;
    std::string mate_file, pair_mode, pair_summary;
    bool interleaved = false, pair_require_both = false;
    std::string extract_out, extract_out2;
    std::vector<std::string> extract_clade, extract_exclude;
    bool extract_unplaced = false;
    cls_fastq_opts fq;
    memset(&fq, 0, sizeof fq);
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "-d" || a == "--database-file-path") db_path = need("--database-file-path");
        else if (a == "-o" || a == "--output-file-path") out_path = need("--output-file-path");
        else if (a == "-a" || a == "--annotations-file-path") ann_path = need("--annotations-file-path");
        else if (a == "--out-format") fmt = need("--out-format");
        else if (a == "-i" || a == "--iterations") { p.flags |= CLS_HAS_MAX_ITERATIONS; p.max_iterations = atoi(need("--iterations")); }
        else if (a == "-m" || a == "--match-coverage") { p.flags |= CLS_HAS_MIN_MATCH_COVERAGE; p.min_match_coverage = atof(need("--match-coverage")); }
        else if (a == "-r" || a == "--remove-intersection") { p.flags |= CLS_HAS_REMOVE_INTERSECTION; p.remove_intersection = 1; }
        else if (a == "-f" || a == "--force-overwrite") overwrite = 1;
        else if (a == "--device") {
            const std::string v = need("--device");
            if (v.find(',') == std::string::npos) device = atoi(v.c_str());
            else {
                for (size_t p0 = 0; p0 <= v.size();) {
                    size_t p1 = v.find(',', p0);
                    if (p1 == std::string::npos) p1 = v.size();
                    const std::string item = v.substr(p0, p1 - p0);
                    char* end = nullptr;
                    const long d = strtol(item.c_str(), &end, 10);
                    if (item.empty() || *end || d < 0 || d > 1 << 20) { fprintf(stderr, "error: invalid value '%s' for '--device'\n", v.c_str()); return 2; }
                    devices.push_back((int)d);
                    p0 = p1 + 1;
                }
            }
        }
        else if (a == "--query-format") qfmt = need("--query-format");
        else if (a == "-q" || a == "--trim-quality") trim = need("--trim-quality");
        else if (a == "--report") report = need("--report");
        else if (a == "--report-only") report_only = need("--report-only");
        else if (a == "--report-all-clades") all_rows = 1;
        else if (a == "-2" || a == "--mate-file") mate_file = need("--mate-file");
        else if (a == "--interleaved") interleaved = true;
        else if (a == "--pair-mode") pair_mode = need("--pair-mode");
        else if (a == "--pair-require-both") pair_require_both = true;
        else if (a == "--pair-summary") pair_summary = need("--pair-summary");
        else if (a == "--extract-out") extract_out = need("--extract-out");
        else if (a == "--extract-out2") extract_out2 = need("--extract-out2");
        else if (a == "--extract-clade") extract_clade.push_back(need("--extract-clade"));
        else if (a == "--extract-exclude") extract_exclude.push_back(need("--extract-exclude"));
        else if (a == "--extract-unplaced") extract_unplaced = true;
        else if (!a.empty() && a[0] == '-' && a != "-") { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); usage(); return 2; }
        else query = a;
    }
    const bool extract = !extract_out.empty();
    if (!extract && (!extract_out2.empty() || !extract_clade.empty() || !extract_exclude.empty() || extract_unplaced)) {
        fprintf(stderr, "error: the '--extract-...' options need '--extract-out'\n");
        return 2;
    }
    std::vector<uint64_t> include_ids, exclude_ids;
    if (extract) {
        if (!out_path.empty()) { fprintf(stderr, "error: '--extract-out' cannot be used with '--output-file-path'\n"); return 2; }
        if (qfmt != "fastq") { fprintf(stderr, "error: '--extract-out' needs '--query-format fastq'\n"); return 2; }
        if (!devices.empty()) { fprintf(stderr, "error: reads are extracted on one device: '--device' takes one ordinal\n"); return 2; }
        if (!extract_out2.empty() && mate_file.empty()) { fprintf(stderr, "error: '--extract-out2' needs '--mate-file'\n"); return 2; }
        if (extract_out2.empty() && !mate_file.empty()) { fprintf(stderr, "error: '--mate-file' with '--extract-out' needs '--extract-out2'\n"); return 2; }
        for (const auto& v : extract_clade)
            if (!parse_ids(v, &include_ids)) { fprintf(stderr, "error: invalid value '%s' for '--extract-clade'\n", v.c_str()); return 2; }
        for (const auto& v : extract_exclude)
            if (!parse_ids(v, &exclude_ids)) { fprintf(stderr, "error: invalid value '%s' for '--extract-exclude'\n", v.c_str()); return 2; }
    }
    if (db_path.empty() || (out_path.empty() && report_only.empty() && !extract)) { usage(); return 2; }
    if (!report.empty() && !report_only.empty()) { fprintf(stderr, "error: '--report' cannot be used with '--report-only'\n"); return 2; }
    if (fmt != "yaml" && fmt != "jsonl") { fprintf(stderr, "error: invalid value '%s' for '--out-format'\n", fmt.c_str()); return 2; }
    if (qfmt != "fasta" && qfmt != "fastq") { fprintf(stderr, "error: invalid value '%s' for '--query-format'\n", qfmt.c_str()); return 2; }
    if (!trim.empty()) {
        if (qfmt != "fastq") { fprintf(stderr, "error: '--trim-quality' needs '--query-format fastq'\n"); return 2; }
        if (!parse_cutoffs(trim, &fq.trim_5p, &fq.trim_3p)) { fprintf(stderr, "error: invalid value '%s' for '--trim-quality'\n", trim.c_str()); return 2; }
    }
    const int query_format = qfmt == "fastq" ? CLS_QUERY_FASTQ : CLS_QUERY_FASTA;
    const bool pairs = !mate_file.empty() || interleaved;
    if (!pairs && (!pair_mode.empty() || pair_require_both || !pair_summary.empty())) {
        fprintf(stderr, "error: the '--pair-...' options need '--mate-file' or '--interleaved'\n");
        return 2;
    }
    uint32_t pair_flags = 0;
    if (pairs) {
        if (qfmt != "fastq") { fprintf(stderr, "error: paired reads need '--query-format fastq'\n"); return 2; }
        if (!mate_file.empty() && interleaved) { fprintf(stderr, "error: '--mate-file' cannot be used with '--interleaved'\n"); return 2; }
        if (!devices.empty()) { fprintf(stderr, "error: paired reads are placed on one device: '--device' takes one ordinal\n"); return 2; }
        if (!pair_mode.empty() && pair_mode != "deepest" && pair_mode != "conservative") {
            fprintf(stderr, "error: invalid value '%s' for '--pair-mode'\n", pair_mode.c_str());
            return 2;
        }
        if (query == "-") { fprintf(stderr, "error: paired reads are read from files\n"); return 2; }
        if (pair_mode == "conservative") pair_flags |= CLS_PAIR_CONSERVATIVE;
        if (pair_require_both) pair_flags |= CLS_PAIR_REQUIRE_BOTH;
    }

    cls_tree* tree = nullptr;
    if (cls_tree_load(db_path.c_str(), &tree) != CLS_OK) { fprintf(stderr, "Error loading database: %s\n", cls_host_last_error()); return 1; }
    if (!ann_path.empty() && cls_tree_set_annotations_yaml(tree, ann_path.c_str()) != CLS_OK) {
        fprintf(stderr, "Error loading annotations: %s\n", cls_host_last_error());
        return 1;
    }
    cls_db_desc desc;
    cls_db* db = nullptr;
    cls_db_group* group = nullptr;
    if (cls_tree_desc(tree, &desc) != CLS_OK) { fprintf(stderr, "%s\n", cls_host_last_error()); return 1; }
    if (devices.empty()) {
        if (cls_db_create(&desc, device, &db) != CLS_OK) { fprintf(stderr, "%s\n", cls_last_error()); return 1; }
    } else if (cls_db_group_create(&desc, devices.data(), (uint32_t)devices.size(), &group) != CLS_OK) {
        fprintf(stderr, "%s\n", cls_last_error());
        return 1;
    }
    uint32_t n = 0;
    double seconds = 0;
    const int format = fmt == "yaml" ? CLS_FORMAT_YAML : CLS_FORMAT_JSONL;
    int rc;
    if (extract) {
        const std::string& rep = report_only.empty() ? report : report_only;
        rc = cls_extract_reads(db, tree, query.c_str(), mate_file.empty() ? nullptr : mate_file.c_str(), interleaved ? 1 : 0, include_ids.data(),
                               (uint32_t)include_ids.size(), exclude_ids.data(), (uint32_t)exclude_ids.size(), extract_unplaced ? CLS_SELECT_UNPLACED : 0u,
                               extract_out.c_str(), extract_out2.empty() ? nullptr : extract_out2.c_str(), rep.empty() ? nullptr : rep.c_str(),
                               pair_summary.empty() ? nullptr : pair_summary.c_str(), &p, &fq, pair_flags, overwrite, all_rows, 0, nullptr, &n, &seconds);
    } else if (pairs) {
        const std::string& rep = report_only.empty() ? report : report_only;
        rc = cls_place_pairs(db, tree, query.c_str(), mate_file.empty() ? nullptr : mate_file.c_str(), report_only.empty() ? out_path.c_str() : nullptr,
                             rep.empty() ? nullptr : rep.c_str(), pair_summary.empty() ? nullptr : pair_summary.c_str(), &p, &fq, pair_flags, format,
                             overwrite, all_rows, &n, &seconds);
    } else if (!report_only.empty())
        rc = db ? cls_profile_sequences(db, tree, query.c_str(), report_only.c_str(), &p, overwrite, query_format, &fq, 0, all_rows, &n, &seconds)
                : cls_profile_sequences_group(group, tree, query.c_str(), report_only.c_str(), &p, overwrite, query_format, &fq, 0, all_rows, &n,
                                              &seconds);
    else if (!report.empty())
        rc = cls_place_sequences_report(db, group, tree, query.c_str(), out_path.c_str(), &p, overwrite, format, query_format, &fq, report.c_str(),
                                        all_rows, &n, &seconds);
    else
        rc = db ? cls_place_sequences_ex(db, tree, query.c_str(), out_path.c_str(), &p, overwrite, format, query_format, &fq, &n, &seconds)
                : cls_place_sequences_group_ex(group, tree, query.c_str(), out_path.c_str(), &p, overwrite, format, query_format, &fq, &n,
                                               &seconds);
    if (rc != CLS_OK) fprintf(stderr, "%s\n", cls_host_last_error());
    else fprintf(stderr, "{\"code\":\"CLIPLACE0002\",\"sequences\":%u,\"totalSeconds\":%.6f,\"averageSeconds\":%.9f}\n", n, seconds, n ? seconds / n : 0.0);
    cls_db_destroy(db);
    cls_db_group_destroy(group);
    cls_tree_free(tree);
    return rc == CLS_OK ? 0 : 1;
}
