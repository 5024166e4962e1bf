// rb_core_main.cpp -- the host model of the resident BCF walk (vcfgl_amd/csrc/misc/rb_core.h: the routines the kernels run) against a
// soft cursor (BcfIn::soft) that walks the same bytes by bcf_scan_record and the rules of bcf_format_fields, as a stand-alone program
// for the sanitizers (tests/test_rb_core_cpu.py builds it with -fsanitize=address,undefined).  Every file lies in a heap block of
// exactly its length.
//   rb_core_main CASES OUT
// CASES, one a line:
//   F <hex>               a whole file.  The model at hops_most 1, 2, 7 and 2^20 and at windows of 32, 48 and RB_WINDOW bytes must give
//                         the cursor's record offsets, heads and field table and flag nothing; bcf_shared and bcf_format_fields must
//                         read from every head what they read from the file; load_u32_any must read every float of every GL block.
//                         -> "ok <records> <fields> <fifteen> <residues>": fields with fifteen values, GL data offsets mod 4 seen (bits)
//   T <hex>               every truncation of the file behind its header -> "ok <files> <flagged> <host failed>"
//   M <seed> <count> <hex>  `count` files with one byte of a record's head (lengths, shared block, keys, descriptors) changed
//                         -> the same three sums
// For T and M: the model flags wherever the cursor fails, and where the cursor does not fail the model either agrees or flags.
// A line of OUT per case, or "MISMATCH ...".  stdout: "cases <n>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "misc/record_file.h"
#include "misc/rb_core.h"

namespace {

struct RefWalk { std::vector<int64_t> rec_off, hoff; std::vector<uint8_t> heads; std::vector<rb::Field> fields; std::vector<int64_t> field_first; };

// the cursor's walk from `start`; false: it failed (out holds the records before)
bool ref_walk(const uint8_t* buf, const size_t size, const size_t start, const size_t N, RefWalk& out) {
    out = RefWalk(); out.hoff.push_back(0); out.field_first.push_back(0);
    BcfIn c; c.buf = buf; c.size = size; c.off = start; c.soft = true;
    try {
        while (c.off < c.size) {
            const size_t o = c.off;
            BcfRecAt at;
            bcf_scan_record(c, at);
            c.off = at.shared + 20;
            const uint32_t nfs = c.u32();
            if ((size_t)(nfs & 0xFFFFFF) != N) c.fail("n_sample");
            const int n_fmt = (int)(nfs >> 24);
            std::vector<uint8_t> head(buf + o, buf + at.shared);
            if (at.shared_end > size) c.fail("shared");
            head.insert(head.end(), buf + at.shared, buf + at.shared_end);
            std::vector<rb::Field> fl;
            c.off = at.shared_end;
            std::vector<int32_t> iv; int ty, n;
            for (int k = 0; k < n_fmt; k++) {
                const size_t h0 = c.off;
                c.typed(ty, n); c.ints(ty, n, iv);
                if (iv.empty()) c.fail("key");
                c.typed(ty, n);
                const size_t bytes = (size_t)bcf_type_width(ty) * n * N;
                if (c.off + bytes > c.size) c.fail("truncated BCF record");
                head.insert(head.end(), buf + h0, buf + c.off);
                fl.push_back(rb::Field{iv[0], ty, n, (int64_t)c.off});
                c.off += bytes;
            }
            c.off = at.rec_end;
            out.rec_off.push_back((int64_t)o);
            out.heads.insert(out.heads.end(), head.begin(), head.end());
            out.hoff.push_back((int64_t)out.heads.size());
            out.fields.insert(out.fields.end(), fl.begin(), fl.end());
            out.field_first.push_back((int64_t)out.fields.size());
        }
    } catch (const BcfSoftFail&) { return false; }
    return true;
}

// (the cursor reads a key's least values as "missing" and "end of vector"; the model keeps the bytes' own value)
bool same_fields(const std::vector<rb::Field>& a, const std::vector<rb::Field>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].type != b[i].type || a[i].n != b[i].n || a[i].data_off != b[i].data_off) return false;
        if (a[i].key != b[i].key && !(b[i].key == INT32_MIN || b[i].key == INT32_MIN + 1)) return false;
    }
    return true;
}

const int64_t HOPS[4] = {1, 2, 7, 1 << 20};
const int64_t WINDOWS[3] = {rb::RB_WINDOW_LEAST, 48, rb::RB_WINDOW};

// the model on the block `text` against the cursor.  strict: the file is sound -- nothing may be flagged and the cursor may not fail
std::string compare(const uint8_t* text, const int64_t n, const size_t start, const size_t N, const int64_t head_most, const bool strict, long& flagged, long& failed) {
    RefWalk want;
    const bool host_ok = ref_walk(text, (size_t)n, start, N, want);
    if (!host_ok) failed++;
    if (strict && !host_ok) return "MISMATCH the cursor fails on a sound file";
    bool any_flag = false;
    for (const int64_t hops : HOPS) for (const int64_t window : WINDOWS) {
        rb::Walk got;
        rb::walk_model(text, n, (int64_t)start, (int64_t)N, hops, window, head_most, got);
        const std::string at = " at hops " + std::to_string((long long)hops) + " window " + std::to_string((long long)window);
        if (got.flagged()) {
            any_flag = true;
            if (strict) return "MISMATCH flagged (" + std::string(rb::why_text(got.why)) + ", record " + std::to_string((long long)got.ordinal) + ")" + at;
            continue;
        }
        if (!host_ok) return "MISMATCH the cursor fails and the model does not flag" + at;
        const char* what = got.rec_off != want.rec_off ? "offsets" : got.hoff != want.hoff ? "hoff" : got.heads != want.heads ? "heads"
                           : got.field_first != want.field_first ? "field_first" : !same_fields(got.fields, want.fields) ? "fields" : nullptr;
        if (what) return std::string("MISMATCH ") + what + at;
        const int64_t R = (int64_t)want.rec_off.size();
        if (hops < (1 << 20) && got.launches != R / hops + 1) return "MISMATCH launches" + at;
    }
    if (any_flag) flagged++;
    return "";
}

std::string sound_file(const std::vector<uint8_t>& bytes, long& records, long& fields, long& fifteen, long& residues) {
    const int64_t n = (int64_t)bytes.size();
    uint8_t* text = (uint8_t*)malloc((size_t)n);
    memcpy(text, bytes.data(), (size_t)n);
    struct Free { uint8_t* p; ~Free() { free(p); } } fr{text};
    BcfDict d; Vcf v; BcfIn c; c.buf = text; c.size = (size_t)n; c.soft = true;
    try { bcf_header(c, d, v); } catch (const BcfSoftFail&) { return "MISMATCH the header"; }
    const size_t start = c.off, N = v.samples.size();
    long flagged = 0, failed = 0;
    std::string bad = compare(text, n, start, N, rf::RF_HEAD_MOST, true, flagged, failed);
    if (!bad.empty()) return bad;
    // a head bound one byte too short for the longest shared block flags, one that fits it does not
    rb::Walk w;
    rb::walk_model(text, n, (int64_t)start, (int64_t)N, 7, rb::RB_WINDOW, rf::RF_HEAD_MOST, w);
    int64_t longest = 0;
    for (const int64_t o : w.rec_off) { const int64_t l = (int64_t)rb::rd_u32(text, o); if (l > longest) longest = l; }
    if (w.records > 0) {
        rb::Walk a, b;
        rb::walk_model(text, n, (int64_t)start, (int64_t)N, 7, rb::RB_WINDOW, longest, a);
        rb::walk_model(text, n, (int64_t)start, (int64_t)N, 7, rb::RB_WINDOW, longest - 1, b);
        if (a.flagged() || b.why != rb::W_HEAD_MOST) return "MISMATCH the head bound";
    }
    // the host routines on the head stream against the same routines on the file
    try {
        BcfIn f; f.buf = text; f.size = (size_t)n; f.off = start; f.soft = true;
        BcfIn h; h.buf = w.heads.data(); h.size = w.heads.size(); h.soft = true;
        for (size_t i = 0; f.off < f.size; i++) {
            if (i >= (size_t)w.records) return "MISMATCH fewer heads than records";
            BcfRecAt at, hat; int n_fmt, hn_fmt;
            const size_t o = f.off;
            bcf_scan_record(f, at);
            Rec r, hr;
            bcf_shared(f, d, at, N, r, n_fmt);
            const size_t head_at = h.off = (size_t)w.hoff[i];
            const uint32_t ls = h.u32(); (void)h.u32();
            hat.shared = h.off; hat.shared_end = h.off + ls; hat.rec_end = (size_t)w.hoff[i + 1];
            bcf_shared(h, d, hat, N, hr, hn_fmt);
            if (n_fmt != hn_fmt || r.pos0 != hr.pos0 || r.alleles != hr.alleles || r.chrom != hr.chrom || r.info != hr.info || r.filt != hr.filt || r.id != hr.id) return "MISMATCH bcf_shared on a head";
            struct Fl { int k; std::string key; int ty, n; size_t off; };
            std::vector<Fl> a, b;
            bcf_format_fields(f, d, n_fmt, N, [&](int k, const std::string& key, int ty, int nv, size_t off) { a.push_back(Fl{k, key, ty, nv, off}); });
            bcf_format_fields(h, d, n_fmt, N, [&](int k, const std::string& key, int ty, int nv, size_t off) { b.push_back(Fl{k, key, ty, nv, off}); },
                              (int64_t)o + (int64_t)(h.off - head_at));
            if (h.off != hat.rec_end || a.size() != b.size()) return "MISMATCH bcf_format_fields on a head";
            for (size_t k = 0; k < a.size(); k++) {
                if (a[k].key != b[k].key || a[k].ty != b[k].ty || a[k].n != b[k].n || a[k].off != b[k].off) return "MISMATCH a field read from a head";
                fields++;
                if (a[k].n == 15) fifteen++;
                if (a[k].key != "GL") continue;
                residues |= 1l << (a[k].off & 3);
                const size_t words = (size_t)a[k].n * N;                 // every float of the block, at whatever byte it begins
                for (size_t j = 0; j < words; j++) {
                    uint32_t x; memcpy(&x, text + a[k].off + 4 * j, 4);
                    if (rb::load_u32_any(text, (int64_t)(a[k].off + 4 * j), n) != x) return "MISMATCH load_u32_any";
                }
            }
            f.off = at.rec_end;
            records++;
        }
    } catch (const BcfSoftFail&) { return "MISMATCH the host routines fail on a sound file"; }
    if (records != (long)w.records) return "MISMATCH the record count";
    return "";
}

std::vector<uint8_t> unhex(const char* e) {
    std::vector<uint8_t> bytes;
    while (*e == ' ') e++;
    for (; e[0] && e[1] && e[0] != '-' && e[0] != '\n'; e += 2) { unsigned v = 0; sscanf(e, "%2x", &v); bytes.push_back((uint8_t)v); }
    return bytes;
}

// one damaged copy in a block of exactly its length
std::string damaged(const std::vector<uint8_t>& bytes, const size_t len, const long at, const uint8_t value, const size_t start, const size_t N, long& flagged, long& failed) {
    uint8_t* text = (uint8_t*)malloc(len);
    if (len) memcpy(text, bytes.data(), len);
    if (at >= 0) text[at] = value;
    const std::string bad = compare(text, (int64_t)len, start, N, rf::RF_HEAD_MOST, false, flagged, failed);
    free(text);
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: rb_core_main CASES OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    std::vector<char> line(1 << 24);
    long n_cases = 0;
    while (fgets(line.data(), (int)line.size(), in)) {
        n_cases++;
        std::string bad;
        if (line[0] == 'F') {
            long records = 0, fields = 0, fifteen = 0, residues = 0;
            bad = sound_file(unhex(line.data() + 2), records, fields, fifteen, residues);
            if (bad.empty()) { fprintf(out, "ok %ld %ld %ld %ld\n", records, fields, fifteen, residues); continue; }
        } else if (line[0] == 'T' || line[0] == 'M') {
            unsigned long long seed = 0; long count = 0; int used = 0;
            if (line[0] == 'M') sscanf(line.data() + 2, "%llu %ld%n", &seed, &count, &used);
            const std::vector<uint8_t> bytes = unhex(line.data() + 2 + used);
            BcfDict d; Vcf v; BcfIn c; c.buf = bytes.data(); c.size = bytes.size(); c.soft = true;
            bcf_header(c, d, v);
            const size_t start = c.off, N = v.samples.size();
            long files = 0, flagged = 0, failed = 0;
            if (line[0] == 'T') {
                for (size_t len = start; len <= bytes.size() && bad.empty(); len++, files++) bad = damaged(bytes, len, -1, 0, start, N, flagged, failed);
            } else {
                RefWalk w;
                if (!ref_walk(bytes.data(), bytes.size(), start, N, w)) bad = "MISMATCH the cursor fails on the file to be changed";
                std::vector<long> places;                                // the bytes of every head, where they lie in the file
                for (size_t i = 0; i < w.rec_off.size(); i++) {
                    const long lead = 8 + (long)rb::rd_u32(bytes.data(), w.rec_off[i]);
                    for (long j = 0; j < lead; j++) places.push_back((long)w.rec_off[i] + j);
                    long p = (long)w.rec_off[i] + lead;
                    for (int64_t k = w.field_first[i]; k < w.field_first[i + 1]; k++) {
                        for (; p < (long)w.fields[(size_t)k].data_off; p++) places.push_back(p);
                        p = (long)(w.fields[(size_t)k].data_off + (int64_t)bcf_type_width(w.fields[(size_t)k].type) * w.fields[(size_t)k].n * (int64_t)N);
                    }
                }
                uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
                auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
                static const uint8_t special[8] = {0x00, 0xFF, 0xF5, 0xF1, 0x11, 0x12, 0x80, 0x7F};
                for (long k = 0; k < count && bad.empty() && !places.empty(); k++, files++) {
                    // (the lengths and the descriptors are a small share of a head: half the draws go to the 8 length bytes and the last
                    // fixed word of a record and to the bytes behind the shared block)
                    long at = places[next() % places.size()];
                    if (k & 1) {
                        const size_t i = next() % w.rec_off.size();
                        const long o = (long)w.rec_off[i], lead = 8 + (long)rb::rd_u32(bytes.data(), o), hl = (long)(w.hoff[i + 1] - w.hoff[i]);
                        const uint64_t pick = next() % 3;
                        at = pick == 0 ? o + (long)(next() % 8) : pick == 1 ? o + 8 + 20 + (long)(next() % 4) : hl > lead ? places[(size_t)(w.hoff[i] + lead + (long)(next() % (uint64_t)(hl - lead)))] : o;
                    }
                    const uint8_t value = next() & 1 ? special[next() % 8] : (uint8_t)next();
                    bad = damaged(bytes, bytes.size(), at, value, start, N, flagged, failed);
                    if (!bad.empty()) bad += " (byte " + std::to_string(at) + " = " + std::to_string((int)value) + ")";
                }
            }
            if (bad.empty()) { fprintf(out, "ok %ld %ld %ld\n", files, flagged, failed); continue; }
        } else bad = "MISMATCH unknown case";
        fprintf(out, "%s\n", bad.c_str());
    }
    fclose(in); fclose(out);
    printf("cases %ld\n", n_cases);
    return 0;
}
