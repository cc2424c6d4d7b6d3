// cls-build-db: C++ look-alike of the reference's `cls build-db` sub-command
// (ports/cli/src/cmds/build_db.rs:6-42 flag surface, :44-79 behaviour): Newick tree + MSA -> the `.cls` database
// (zstd-compressed YAML) that `cls-place -d` reads.
//   cls-build-db TREE MSA [-k N] [-m N] [-s F] [-o OUT] [-t N] [--device N] [--host] [--no-header-shift]
// The k-mer map is built on the GPU (cls_tree_build_kmers_map_device); --host builds it on the host instead.  Errors
// print one line and exit 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "cls_host.h"

static void usage() {
    fprintf(stdout,
            "Usage: cls-build-db [OPTIONS] <TREE> <MSA>\n\n"
            "Arguments:\n"
            "  <TREE>  rooted phylogenetic tree in Newick format\n"
            "  <MSA>   multi-FASTA whose headers name the tree's leaves\n\n"
            "Options:\n"
            "  -k, --k-size <N>                  k-mer size [default: 35]\n"
            "  -m, --m-size <N>                  minimizer (bucket prefix) size [default: 4]\n"
            "  -s, --min-branch-support <F>      branches below this support are collapsed [default: 70]\n"
            "  -o, --output-file-path <PATH>     database file, extension forced to .cls [default: classeq-database.cls]\n"
            "  -t, --threads <N>                 accepted for compatibility, ignored\n"
            "      --device <N>                  GPU ordinal [default: 0]\n"
            "      --host                        build the k-mer map on the host (no GPU needed)\n"
            "      --no-header-shift             file each record's k-mers under its own header; the reference files them\n"
            "                                    under the next record's header and never indexes the last record\n"
            "  -h, --help                        print this help\n");
}

static int die(std::string msg) {
    for (char& c : msg) if (c == '\n' || c == '\r') c = ' ';
    fprintf(stderr, "error: %s\n", msg.c_str());
    return 1;
}

static bool parse_u64(const char* s, unsigned long long* v) {
    if (!s || !*s || *s == '-') return false;
    char* end = nullptr;
    *v = strtoull(s, &end, 10);
    return *end == '\0';
}

static bool parse_f64(const char* s, double* v) {
    if (!s || !*s) return false;
    char* end = nullptr;
    *v = strtod(s, &end);
    return *end == '\0';
}

int main(int argc, char** argv) {
    std::string tree_path, msa_path, out_path = "classeq-database.cls";
    unsigned long long k = 35, m = 4, ull = 0;
    double support = 70;
    int device = 0;
    bool host = false, shift = true;
    int n_pos = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const char* val = nullptr;
        auto need = [&]() -> bool {
            if (i + 1 >= argc) return false;
            val = argv[++i];
            return true;
        };
        if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "-k" || a == "--k-size") {
            if (!need() || !parse_u64(val, &k) || k == 0) return die("invalid value for '--k-size': a positive integer is required");
        } else if (a == "-m" || a == "--m-size") {
            if (!need() || !parse_u64(val, &m)) return die("invalid value for '--m-size': a non-negative integer is required");
        } else if (a == "-s" || a == "--min-branch-support") {
            if (!need() || !parse_f64(val, &support)) return die("invalid value for '--min-branch-support': a number is required");
        } else if (a == "-o" || a == "--output-file-path") {
            if (!need() || !*val) return die("a value is required for '--output-file-path'");
            out_path = val;
        } else if (a == "-t" || a == "--threads") {
            if (!need() || !parse_u64(val, &ull)) return die("invalid value for '--threads': a non-negative integer is required");
        } else if (a == "--device") {
            if (!need() || !parse_u64(val, &ull) || ull > (1u << 20)) return die("invalid value for '--device': a GPU ordinal is required");
            device = (int)ull;
        } else if (a == "--host") host = true;
        else if (a == "--no-header-shift") shift = false;
        else if (a.size() > 1 && a[0] == '-') return die("unexpected argument '" + a + "' (see --help)");
        else if (n_pos == 0) { tree_path = a; ++n_pos; }
        else if (n_pos == 1) { msa_path = a; ++n_pos; }
        else return die("unexpected argument '" + a + "' (see --help)");
    }
    if (n_pos < 2) return die("the arguments <TREE> and <MSA> are required (see --help)");

    FILE* f = fopen(msa_path.c_str(), "rb");
    if (!f) return die("cannot open the MSA file " + msa_path);
    std::string msa;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) msa.append(buf, got);
    const bool read_ok = !ferror(f);
    fclose(f);
    if (!read_ok) return die("cannot read the MSA file " + msa_path);

    cls_tree* tree = nullptr;
    if (cls_tree_init_from_file(tree_path.c_str(), support, &tree) != CLS_OK) return die(cls_host_last_error());
    const uint32_t flags = shift ? CLS_BUILD_REFERENCE_HEADER_SHIFT : 0u;
    int rc = host ? cls_tree_build_kmers_map(tree, msa.data(), msa.size(), k, m, flags)
                  : cls_tree_build_kmers_map_device(tree, msa.data(), msa.size(), k, m, flags, device);
    if (rc == CLS_OK) rc = cls_tree_save(tree, out_path.c_str(), CLS_DB_FORMAT_ZSTD, 0);
    const std::string err = rc == CLS_OK ? "" : cls_host_last_error();
    cls_tree_free(tree);
    if (rc != CLS_OK) return die(err);
    return 0;
}
