// FASTA input stage of the placement path, with the reference's exact record
// semantics: FileOrStdin::sequence_content_by_channel
// (core/src/domain/dtos/file_or_stdin.rs:76-116) and
// SequenceBody::remove_non_iupac_from_sequence (core/src/domain/dtos/sequence.rs:47-56).
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "cls_place.h"

namespace {

// std::io::BufRead::lines() yields Err on a line that is not valid UTF-8; the
// reference propagates it (`line?`) and the caller drops it (mod.rs:119).
bool valid_utf8(const unsigned char* s, size_t n) {
    size_t i = 0;
    while (i < n) {
        unsigned char c = s[i];
        if (c < 0x80) { ++i; continue; }
        size_t need;
        uint32_t cp;
        if ((c & 0xE0) == 0xC0) { need = 1; cp = c & 0x1F; if (cp < 2) return false; }
        else if ((c & 0xF0) == 0xE0) { need = 2; cp = c & 0x0F; }
        else if ((c & 0xF8) == 0xF0) { need = 3; cp = c & 0x07; if (cp > 4) return false; }
        else return false;
        if (i + need >= n) return false;  // truncated multi-byte sequence
        for (size_t k = 1; k <= need; ++k) {
            unsigned char d = s[i + k];
            if ((d & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (d & 0x3F);
        }
        if (need == 2 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) return false;
        if (need == 3 && (cp < 0x10000 || cp > 0x10FFFF)) return false;
        i += need + 1;
    }
    return true;
}

}  // namespace

extern "C" void cls_fasta_free(cls_fasta* f) {
    if (!f) return;
    free(f->headers); free(f->header_off); free(f->bases); free(f->base_off);
    memset(f, 0, sizeof *f);
}

extern "C" int cls_fasta_parse(const char* text, size_t len, cls_fasta* out) {
    if (!out || (!text && len)) return CLS_E_INVALID_ARG;
    memset(out, 0, sizeof *out);
    try {
        std::string headers, bases, header, sequence;
        std::vector<uint64_t> hoff{0}, boff{0};
        bool truncated = false;
        auto emit = [&]() {
            headers += header; hoff.push_back(headers.size());
            bases += sequence; boff.push_back(bases.size());
        };
        size_t pos = 0;
        while (pos < len) {
            const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
            size_t end = nl ? (size_t)(nl - text) : len;
            size_t lend = end;
            if (nl && lend > pos && text[lend - 1] == '\r') --lend;  // lines() strips "\n" or "\r\n"
            const char* line = text + pos;
            size_t ll = lend - pos;
            pos = nl ? end + 1 : len;
            if (!valid_utf8((const unsigned char*)line, ll)) { truncated = true; break; }
            if (ll == 0) continue;                                    // :87-89
            if (line[0] == '>') {
                if (!header.empty()) {                                // :92-95 (emitted even if the sequence is empty)
                    emit();
                    sequence.clear();
                } else if (!sequence.empty()) {                       // :96-100
                    truncated = true;
                    break;
                }
                header.clear();
                for (size_t i = 0; i < ll; ++i) if (line[i] != '>') header.push_back(line[i]);  // replace(">", "") :102
            } else {
                for (size_t i = 0; i < ll; ++i) {                     // sequence.rs:47-56
                    char c = line[i];
                    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
                    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') sequence.push_back(c);
                }
            }
        }
        if (!truncated && !header.empty() && !sequence.empty()) emit();  // :111-113
        out->n = (uint32_t)(hoff.size() - 1);
        out->truncated = truncated ? 1 : 0;
        out->headers = (char*)malloc(headers.size() + 1);
        out->bases = (char*)malloc(bases.size() + 1);
        out->header_off = (uint64_t*)malloc(hoff.size() * 8);
        out->base_off = (uint64_t*)malloc(boff.size() * 8);
        if (!out->headers || !out->bases || !out->header_off || !out->base_off) { cls_fasta_free(out); return CLS_E_NOMEM; }
        memcpy(out->headers, headers.data(), headers.size());
        memcpy(out->bases, bases.data(), bases.size());
        memcpy(out->header_off, hoff.data(), hoff.size() * 8);
        memcpy(out->base_off, boff.data(), boff.size() * 8);
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_fasta_free(out);
        return CLS_E_NOMEM;
    } catch (...) {
        cls_fasta_free(out);
        return CLS_E_INTERNAL;
    }
}

// One pass over the lines, tracking whether the record open at the current line would be emitted by a '>' line here
// AND by the end of a piece ending here (the conditions of a safe cut, include/cls_place.h).
extern "C" int cls_fasta_split(const char* text, size_t len, uint32_t max_pieces, uint64_t* cuts, uint32_t* n_pieces) {
    if (!cuts || !n_pieces || max_pieces == 0 || (!text && len)) return CLS_E_INVALID_ARG;
    uint32_t np = 0;
    cuts[0] = 0;
    uint32_t next = 1;  // the next interior target: next * len / max_pieces
    auto target = [&](uint32_t i) { return (uint64_t)((unsigned __int128)i * len / max_pieces); };
    bool header_ok = false, seq_ok = false;  // of the record the current line belongs to
    size_t pos = 0;
    while (pos < len && next < max_pieces) {
        const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
        const size_t end = nl ? (size_t)(nl - text) : len;
        if (text[pos] == '>') {
            // (an invalid UTF-8 line stops the parse before the record is emitted: no cut at it)
            if (header_ok && seq_ok && pos >= target(next) && valid_utf8((const unsigned char*)text + pos, end - pos)) {
                cuts[++np] = pos;
                while (next < max_pieces && target(next) <= pos) ++next;
            }
            header_ok = false;
            for (size_t i = pos; i < end && !header_ok; ++i) header_ok = text[i] != '>' && text[i] != '\r';
            seq_ok = false;
        } else {
            for (size_t i = pos; i < end && !seq_ok; ++i) {
                const char c = (char)(text[i] & ~0x20);  // (upper case)
                seq_ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
            }
        }
        pos = nl ? end + 1 : len;
    }
    cuts[++np] = len;
    *n_pieces = np;
    return CLS_OK;
}

// ---- FASTQ stage (include/cls_place.h states the rules) -------------------------------------------------------
namespace {

struct FqLine {
    size_t s, e;      // content [s, e): the terminator, and a '\r' before a '\n', stripped
    size_t next;      // start of the next line
};

// the line starting at `pos` (< len)
FqLine fq_line(const char* text, size_t len, size_t pos) {
    const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
    FqLine l{pos, nl ? (size_t)(nl - text) : len, nl ? (size_t)(nl - text) + 1 : len};
    if (nl && l.e > l.s && text[l.e - 1] == '\r') --l.e;
    return l;
}

enum FqStatus { FQ_OK, FQ_END, FQ_BAD };

// The record whose line 1 starts at `pos`: FQ_OK (lines in `l`, `*next` = the start of the next record), FQ_END
// (nothing but empty lines from `pos` on), FQ_BAD (malformed or incomplete).
FqStatus fq_record(const char* text, size_t len, size_t pos, FqLine l[4], size_t* next) {
    if (pos >= len) return FQ_END;
    l[0] = fq_line(text, len, pos);
    if (l[0].s == l[0].e) {  // an empty line where a record starts: the end, if nothing but empty lines follow
        for (size_t p = l[0].next; p < len;) {
            const FqLine x = fq_line(text, len, p);
            if (x.s != x.e) return FQ_BAD;
            p = x.next;
        }
        return FQ_END;
    }
    for (int k = 1; k < 4; ++k) {
        if (l[k - 1].next >= len) return FQ_BAD;  // incomplete
        l[k] = fq_line(text, len, l[k - 1].next);
    }
    *next = l[3].next;
    const size_t L = l[1].e - l[1].s;
    if (text[l[0].s] != '@' || l[0].e - l[0].s < 2 || text[l[2].s] != '+' || l[3].e - l[3].s != L) return FQ_BAD;
    if (!valid_utf8((const unsigned char*)text + l[0].s + 1, l[0].e - l[0].s - 1)) return FQ_BAD;
    for (size_t i = 0; i < L; ++i) {
        const unsigned char c = (unsigned char)text[l[1].s + i], q = (unsigned char)text[l[3].s + i];
        if (c >= 0x80 || q < '!' || q > '~') return FQ_BAD;
    }
    return FQ_OK;
}

// the kept window [*start, *stop) of a read of quality `q` (Phred+33 bytes), length L
void fq_trim(const unsigned char* q, size_t L, uint32_t c5, uint32_t c3, size_t* start, size_t* stop) {
    const int64_t a = c5 > 94 ? 94 : c5, b = c3 > 94 ? 94 : c3;  // (exact: from 94 on, every step raises the sum)
    size_t st = 0, sp = L;
    if (a) {
        int64_t s = 0, best = 0;
        for (size_t i = 0; i < L; ++i) {
            s += a - (q[i] - 33);
            if (s < 0) break;
            if (s > best) { best = s; st = i + 1; }
        }
    }
    if (b) {
        int64_t s = 0, best = 0;
        for (size_t i = L; i-- > 0;) {
            s += b - (q[i] - 33);
            if (s < 0) break;
            if (s > best) { best = s; sp = i; }
        }
    }
    if (st >= sp) st = sp = 0;
    *start = st;
    *stop = sp;
}

}  // namespace

extern "C" int cls_fastq_parse(const char* text, size_t len, const cls_fastq_opts* opts, cls_fasta* out) {
    if (!out || (!text && len)) return CLS_E_INVALID_ARG;
    memset(out, 0, sizeof *out);
    cls_fastq_opts o{};
    if (opts) {
        o = *opts;
        for (uint32_t r : o.reserved) if (r) return CLS_E_INVALID_ARG;
    }
    try {
        std::string headers, bases;
        std::vector<uint64_t> hoff{0}, boff{0};
        bool truncated = false;
        size_t pos = 0;
        for (;;) {
            FqLine l[4];
            size_t next = 0;
            const FqStatus st = fq_record(text, len, pos, l, &next);
            if (st != FQ_OK) { truncated = st == FQ_BAD; break; }
            if (hoff.size() > 0xFFFFFFFFull) return CLS_E_INVALID_ARG;
            headers.append(text + l[0].s + 1, l[0].e - l[0].s - 1);
            hoff.push_back(headers.size());
            size_t a = 0, b = 0;
            fq_trim((const unsigned char*)text + l[3].s, l[1].e - l[1].s, o.trim_5p, o.trim_3p, &a, &b);
            for (size_t i = l[1].s + a; i < l[1].s + b; ++i) {  // sequence.rs:47-56
                char c = text[i];
                if (c >= 'a' && c <= 'z') c = (char)(c - 32);
                if (c == 'A' || c == 'C' || c == 'G' || c == 'T') bases.push_back(c);
            }
            boff.push_back(bases.size());
            pos = next;
        }
        out->n = (uint32_t)(hoff.size() - 1);
        out->truncated = truncated ? 1 : 0;
        out->headers = (char*)malloc(headers.size() + 1);
        out->bases = (char*)malloc(bases.size() + 1);
        out->header_off = (uint64_t*)malloc(hoff.size() * 8);
        out->base_off = (uint64_t*)malloc(boff.size() * 8);
        if (!out->headers || !out->bases || !out->header_off || !out->base_off) { cls_fasta_free(out); return CLS_E_NOMEM; }
        memcpy(out->headers, headers.data(), headers.size());
        memcpy(out->bases, bases.data(), bases.size());
        memcpy(out->header_off, hoff.data(), hoff.size() * 8);
        memcpy(out->base_off, boff.data(), boff.size() * 8);
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        cls_fasta_free(out);
        return CLS_E_NOMEM;
    } catch (...) {
        cls_fasta_free(out);
        return CLS_E_INTERNAL;
    }
}

// Record by record (4 lines at a time, whatever they hold): a cut may follow any well-formed record.
extern "C" int cls_fastq_split(const char* text, size_t len, uint32_t max_pieces, uint64_t* cuts, uint32_t* n_pieces) {
    if (!cuts || !n_pieces || max_pieces == 0 || (!text && len)) return CLS_E_INVALID_ARG;
    uint32_t np = 0;
    cuts[0] = 0;
    uint32_t next = 1;  // the next interior target: next * len / max_pieces
    auto target = [&](uint32_t i) { return (uint64_t)((unsigned __int128)i * len / max_pieces); };
    size_t pos = 0;
    while (pos < len && next < max_pieces) {
        FqLine l[4];
        size_t end = 0;
        const FqStatus st = fq_record(text, len, pos, l, &end);
        if (st == FQ_END) break;
        if (st == FQ_BAD) {  // skip the record's four lines (or what is left of them): no cut after it
            end = pos;
            for (int k = 0; k < 4 && end < len; ++k) end = fq_line(text, len, end).next;
        } else if (end < len && end >= target(next)) {
            cuts[++np] = end;
            while (next < max_pieces && target(next) <= end) ++next;
        }
        pos = end;
    }
    cuts[++np] = len;
    *n_pieces = np;
    return CLS_OK;
}
