// rf_core_main.cpp -- the host model of the resident split (vcfgl_amd/csrc/misc/rf_core.h: the routines the kernels run) against
// scan_text + nine_columns (misc/record_file.h), as a stand-alone program for the sanitizers (tests/test_rf_core_cpu.py builds it
// with -fsanitize=address,undefined).  Every text lies in a heap block of exactly its length.
//   rf_core_main CASES OUT
// CASES: one case a line: "T <head_most> <hex of the text or ->" (one text) or "R <seed> <count>" (count random texts over the
// alphabet "\n\t#:,.A1", lengths 0 .. 300, head_most 1 MiB and 7 in turn).  OUT: a line per case, "ok <lines> <over> <records>" (R: the sums) or
// "MISMATCH ...".  Each text is split by the model at chunk sizes 1, 2, 16, 64 and RF_CHUNK.  stdout: "cases <n> RF_CHUNK <bytes>"; no
// case at all (an empty CASES) prints RF_CHUNK alone, which is how the test learns it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "misc/record_file.h"
#include "misc/rf_core.h"

namespace {

// the split by the program's own line walk: memchr for the lines, nine_columns for a record's head
void split_reference(const uint8_t* text, const int64_t total, const int64_t head_most, rf::Split& out) {
    out = rf::Split();
    out.hoff.push_back(0);
    const char* const t0 = (const char*)text;
    const char* p = t0; const char* const end = t0 + total;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        const char* he = le;
        if (le > p && p[0] != '#') {
            const char* col_at[10]; int nc;
            nine_columns(p, le, col_at, nc);
            if (nc == 9) he = col_at[9];
            if (le - p > head_most && (nc < 9 || he - p > head_most)) { out.over = true; he = le; }
        }
        out.ends.push_back(le - t0);
        out.heads.insert(out.heads.end(), (const uint8_t*)p, (const uint8_t*)he);
        out.heads.push_back((uint8_t)'\n');
        out.hoff.push_back((int64_t)out.heads.size());
        out.s_off.push_back(he - t0); out.s_len.push_back(le - he);
        out.lines++;
        p = nl ? nl + 1 : end;
    }
}

// "" when the model agrees with the reference at every chunk size, and scan_text reads from the head stream what it reads from the text
std::string check(const std::vector<uint8_t>& bytes, const int64_t head_most, long& lines, long& over, long& records) {
    const int64_t n = (int64_t)bytes.size();
    uint8_t* text = (uint8_t*)malloc((size_t)n);                       // exactly n bytes (n = 0: whatever malloc(0) gives, never read)
    if (n) memcpy(text, bytes.data(), (size_t)n);
    rf::Split want;
    split_reference(text, n, head_most, want);
    std::string bad;
    const int64_t chunks[5] = {1, 2, 16, 64, rf::RF_CHUNK};
    for (const int64_t chunk : chunks) {
        rf::Split got;
        rf::split_model(text, n, chunk, head_most, got);
        const char* what = got.lines != want.lines ? "lines" : got.ends != want.ends ? "ends" : got.over != want.over ? "over" : nullptr;
        if (!what && !got.over) what = got.hoff != want.hoff ? "hoff" : got.s_off != want.s_off ? "s_off" : got.s_len != want.s_len ? "s_len" : got.heads != want.heads ? "heads" : nullptr;
        if (what) { bad = std::string("MISMATCH ") + what + " at chunk " + std::to_string((long long)chunk); break; }
    }
    if (bad.empty() && !want.over) {
        const std::vector<uint8_t> whole(text, text + n);
        const TextLines a = scan_text(whole), b = scan_text(want.heads);
        if (a.header != b.header || a.samples != b.samples || a.lines.size() != b.lines.size()) bad = "MISMATCH scan_text on the head stream";
        size_t j = 0;
        for (size_t i = 0; bad.empty() && i < a.lines.size(); i++) {
            while (want.hoff[j] < b.lines[i].first) j++;
            const char* col_at[10]; int nc;
            const char* lb = (const char*)whole.data() + a.lines[i].first; const char* le = (const char*)whole.data() + a.lines[i].second;
            nine_columns(lb, le, col_at, nc);
            const char* hcol[10]; int hnc;
            const char* hb = (const char*)want.heads.data() + b.lines[i].first; const char* he = (const char*)want.heads.data() + b.lines[i].second;
            nine_columns(hb, he, hcol, hnc);
            if (hnc != nc || want.hoff[j] != b.lines[i].first) bad = "MISMATCH a record's columns";
            else if (nc == 9 && (hcol[9] != he || want.s_off[j] != col_at[9] - (const char*)whole.data() || want.s_len[j] != le - col_at[9])) bad = "MISMATCH a record's span";
        }
        records += (long)a.lines.size();
    }
    lines += (long)want.lines; over += want.over ? 1 : 0;
    free(text);
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: rf_core_main CASES OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    std::vector<char> line(1 << 24);
    long n_cases = 0;
    while (fgets(line.data(), (int)line.size(), in)) {
        n_cases++;
        long lines = 0, over = 0, records = 0;
        std::string bad;
        if (line[0] == 'T') {
            char* e; const long long head_most = strtoll(line.data() + 2, &e, 10);
            while (*e == ' ') e++;
            std::vector<uint8_t> bytes;
            for (; e[0] && e[1] && e[0] != '-' && e[0] != '\n'; e += 2) { unsigned v = 0; sscanf(e, "%2x", &v); bytes.push_back((uint8_t)v); }
            bad = check(bytes, head_most, lines, over, records);
        } else if (line[0] == 'R') {
            unsigned long long seed = 0; long count = 0;
            sscanf(line.data() + 2, "%llu %ld", &seed, &count);
            uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
            auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
            static const char alphabet[] = "\n\t#:,.A1";
            for (long k = 0; k < count && bad.empty(); k++) {
                std::vector<uint8_t> bytes((size_t)(next() % 301));
                const int tabby = (int)(next() % 3);                       // texts with many tabs reach the ninth one
                for (uint8_t& b : bytes) b = (uint8_t)(tabby && next() % 3 == 0 ? '\t' : alphabet[next() % 8]);
                bad = check(bytes, k & 1 ? 7 : rf::RF_HEAD_MOST, lines, over, records);
                if (!bad.empty()) bad += " (text " + std::to_string(k) + ")";
            }
        } else bad = "MISMATCH unknown case";
        if (bad.empty()) fprintf(out, "ok %ld %ld %ld\n", lines, over, records); else fprintf(out, "%s\n", bad.c_str());
    }
    fclose(in); fclose(out);
    printf("cases %ld RF_CHUNK %lld\n", n_cases, (long long)rf::RF_CHUNK);
    return 0;
}
