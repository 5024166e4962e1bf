// rf_check_main.cpp -- rf_check FILE [HEAD_MOST]: the resident split of a BGZF file of VCF text (resident_file.h) against the same
// split made by scan_text / nine_columns on the bytes zlib reads.  Compared: the header lines, the sample names, the number of record
// lines, every record's head byte for byte, and every record's sample-column span with its bytes fetched from the device.  Prints the
// counts; exit 0 when everything agrees (or when the device says a line's ninth tab is not within HEAD_MOST bytes: `over 1`, nothing
// is compared then), 1 otherwise or when the file is not resident.
#include "record_file.h"
#include "resident_file.h"

int main(int argc, char** argv) {
    if (argc < 2 || argc > 3) { fprintf(stderr, "Usage: rf_check FILE [HEAD_MOST]\n"); return 1; }
    const std::string fn = argv[1];
    const int64_t head_most = argc == 3 ? atoll(argv[2]) : rf::RF_HEAD_MOST;
    char err[256];
    RfFile* f = rf_create(0, err, sizeof err);
    if (!f) die("rf_check: %s", err);
    RfWhy why;
    if (rf_load(f, fn.c_str(), rf_default_max_bytes(f), &why) != 0) die("rf_check: %s", rf_error(f));
    if (why != RF_RESIDENT) { printf("rf_check: RF_CHUNK %lld, not resident (%d)\n", (long long)rf::RF_CHUNK, (int)why); return 1; }
    rf::Split sp; bool more = false;
    if (rf_split(f, head_most, &sp, &more) != 0) die("rf_check: %s", rf_error(f));
    const int64_t total = rf_total(f);
    if (more || sp.over) {
        printf("rf_check: RF_CHUNK %lld, total %lld, lines %lld, over %d, more lines %d\n", (long long)rf::RF_CHUNK, (long long)total, (long long)sp.lines, sp.over ? 1 : 0, more ? 1 : 0);
        rf_destroy(f);
        return 0;
    }
    const std::vector<uint8_t> raw = read_whole(fn);
    const TextLines want = scan_text(raw), got = scan_text(sp.heads);
    long bad = 0;
    auto differ = [&](const char* what, long long at) { if (bad++ < 10) fprintf(stderr, "rf_check: %s differs at %lld\n", what, at); };
    if ((int64_t)raw.size() != total) differ("the text's length", total);
    if (want.header != got.header) differ("the header lines", 0);
    if (want.samples != got.samples) differ("the sample names", 0);
    if (want.lines.size() != got.lines.size()) differ("the number of record lines", (long long)got.lines.size());
    const char* const t0 = (const char*)raw.data(); const char* const h0 = (const char*)sp.heads.data();
    std::vector<uint8_t> cols;
    int64_t span_bytes = 0;
    size_t j = 0;
    for (size_t i = 0; i < want.lines.size() && i < got.lines.size(); i++) {
        const char* lb = t0 + want.lines[i].first; const char* le = t0 + want.lines[i].second;
        const char* col_at[10]; int nc;
        nine_columns(lb, le, col_at, nc);
        const char* he = nc == 9 ? col_at[9] : le;                      // the head: up to one past the ninth tab, or the line
        const int64_t gb = got.lines[i].first, ge = got.lines[i].second;
        if (ge - gb != he - lb || memcmp(h0 + gb, lb, (size_t)(he - lb)) != 0) { differ("a head", (long long)i); continue; }
        while (j < (size_t)sp.lines && sp.hoff[j] < gb) j++;
        if (j >= (size_t)sp.lines || sp.hoff[j] != gb) { differ("a head's place in the stream", (long long)i); continue; }
        if (sp.s_off[j] != he - t0 || sp.s_len[j] != le - he) { differ("a sample-column span", (long long)i); continue; }
        cols.resize((size_t)sp.s_len[j] + 1);
        if (rf_fetch(f, sp.s_off[j], sp.s_len[j], cols.data()) != 0) die("rf_check: %s", rf_error(f));
        if (memcmp(cols.data(), he, (size_t)sp.s_len[j]) != 0) differ("a span's bytes", (long long)i);
        span_bytes += sp.s_len[j];
    }
    printf("rf_check: RF_CHUNK %lld, total %lld, lines %lld, header lines %zu, samples %zu, records %zu, head bytes %zu, span bytes %lld, over 0, differences %ld\n",
           (long long)rf::RF_CHUNK, (long long)total, (long long)sp.lines, got.header.size(), got.samples.size(), got.lines.size(), sp.heads.size(), (long long)span_bytes, bad);
    rf_destroy(f);
    return bad ? 1 : 0;
}
