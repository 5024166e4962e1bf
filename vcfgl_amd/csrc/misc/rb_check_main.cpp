// rb_check_main.cpp -- rb_check FILE [HOPS_MOST] [HEAD_MOST]: the resident walk of a BGZF file of BCF (resident_file.h, rb_core.h)
// against the walk of bcf_scan_record / bcf_format_fields on the bytes zlib reads.  Compared: the record count, every record's offset,
// every head byte for byte (the two lengths, the shared block, the fields' keys and descriptors), every field's (key, type, n, data
// offset) as bcf_format_fields reads them from the head, and the bytes of every GL block fetched from the device.  Prints the counts
// and the two bounds it used; exit 0 when everything agrees (or when the device hands the file back: `flagged 1` with the record and
// the reason, nothing is compared then), 1 otherwise or when the file is not resident.
#include "record_file.h"
#include "resident_file.h"

int main(int argc, char** argv) {
    if (argc < 2 || argc > 4) { fprintf(stderr, "Usage: rb_check FILE [HOPS_MOST] [HEAD_MOST]\n"); return 1; }
    const std::string fn = argv[1];
    const int64_t hops_most = argc >= 3 ? atoll(argv[2]) : rb::RB_HOPS_MOST, head_most = argc >= 4 ? atoll(argv[3]) : rf::RF_HEAD_MOST;
    char err[256];
    RfFile* f = rf_create(0, err, sizeof err);
    if (!f) die("rb_check: %s", err);
    RfWhy why;
    if (rf_load(f, fn.c_str(), rf_default_max_bytes(f), &why) != 0) die("rb_check: %s", rf_error(f));
    if (why != RF_RESIDENT) { printf("rb_check: not resident (%d)\n", (int)why); return 1; }
    std::vector<uint8_t> hdr; bool fits = false;
    if (rf_bcf_header(f, &hdr, &fits) != 0) die("rb_check: %s", rf_error(f));
    if (!fits) { printf("rb_check: not BCF, or a header that does not fit the file\n"); return 1; }
    BcfDict d; Vcf v;
    { BcfIn c; c.buf = hdr.data(); c.size = hdr.size(); bcf_header(c, d, v); }
    const size_t N = v.samples.size();
    RbSplit sp;
    if (rf_bcf_split(f, (int64_t)hdr.size(), (int64_t)N, hops_most, head_most, &sp) != 0) die("rb_check: %s", rf_error(f));
    const int64_t total = rf_total(f);
    const long long launches = (long long)rf_stats(f)->chain_launches;
    if (sp.more_records || sp.why != rb::OK) {
        printf("rb_check: hops_most %lld, head_most %lld, total %lld, launches %lld, records %lld, fields 0, flagged 1 (record %lld: %s), differences 0\n", (long long)hops_most,
               (long long)head_most, (long long)total, launches, (long long)sp.records, (long long)sp.ordinal + 1, sp.more_records ? "too many records" : rb::why_text(sp.why));
        rf_destroy(f);
        return 0;
    }
    const std::vector<uint8_t> raw = read_whole(fn);
    long bad = 0;
    auto differ = [&](const char* what, long long at) { if (bad++ < 10) fprintf(stderr, "rb_check: %s differs at %lld\n", what, at); };
    if ((int64_t)raw.size() != total) differ("the file's length", total);
    if (raw.size() < hdr.size() || memcmp(raw.data(), hdr.data(), hdr.size()) != 0) differ("the header", 0);
    struct Fld { std::string key; int ty, n; size_t data_off; bool operator==(const Fld& o) const { return key == o.key && ty == o.ty && n == o.n && data_off == o.data_off; } };
    BcfIn c; c.buf = raw.data(); c.size = raw.size(); c.off = hdr.size();
    BcfIn h; h.buf = sp.heads.data(); h.size = sp.heads.size();
    size_t i = 0; long long n_fields = 0, gl_bytes = 0;
    std::vector<uint8_t> block;
    for (; c.off < c.size; i++) {
        const size_t o = c.off;
        BcfRecAt at;
        bcf_scan_record(c, at);
        if (i >= (size_t)sp.records) { c.off = at.rec_end; continue; }
        if (sp.rec_off[i] != (int64_t)o) differ("a record's offset", (long long)i);
        const int n_fmt = (int)(rb::rd_u32(raw.data(), (int64_t)at.shared + 20) >> 24);
        std::vector<Fld> want, got;
        c.off = at.shared_end;
        bcf_format_fields(c, d, n_fmt, N, [&](int, const std::string& key, int ty, int n, size_t data_off) { want.push_back(Fld{key, ty, n, data_off}); });
        // the head the host would cut from its own bytes
        std::vector<uint8_t> head(raw.begin() + (long)o, raw.begin() + (long)at.shared_end);
        { size_t p = at.shared_end; for (const Fld& w : want) { head.insert(head.end(), raw.begin() + (long)p, raw.begin() + (long)w.data_off); p = w.data_off + (size_t)bcf_type_width(w.ty) * w.n * N; } }
        const size_t ha = (size_t)sp.hoff[i], hb = (size_t)sp.hoff[i + 1];
        if (hb - ha != head.size() || hb > sp.heads.size() || memcmp(sp.heads.data() + ha, head.data(), head.size()) != 0) { differ("a head", (long long)i); c.off = at.rec_end; continue; }
        h.off = ha + (at.shared_end - o);
        bcf_format_fields(h, d, n_fmt, N, [&](int, const std::string& key, int ty, int n, size_t data_off) { got.push_back(Fld{key, ty, n, data_off}); }, sp.rec_off[i] + (int64_t)(at.shared_end - o));
        if (h.off != hb) differ("a head's length by its fields", (long long)i);
        if (!(want == got)) differ("a field table", (long long)i);
        n_fields += (long long)got.size();
        for (const Fld& g : got) if (g.key == "GL") {
            const size_t len = (size_t)bcf_type_width(g.ty) * g.n * N;
            block.resize(len + 1);
            if (rf_fetch(f, (int64_t)g.data_off, (int64_t)len, block.data()) != 0) die("rb_check: %s", rf_error(f));
            if (g.data_off + len > raw.size() || memcmp(block.data(), raw.data() + g.data_off, len) != 0) differ("a GL block's bytes", (long long)i);
            gl_bytes += (long long)len;
        }
        c.off = at.rec_end;
    }
    if ((int64_t)i != sp.records) differ("the number of records", (long long)sp.records);
    printf("rb_check: hops_most %lld, head_most %lld, total %lld, launches %lld, records %lld, fields %lld, flagged 0, head bytes %zu, GL bytes %lld, differences %ld\n",
           (long long)hops_most, (long long)head_most, (long long)total, launches, (long long)sp.records, n_fields, sp.heads.size(), gl_bytes, bad);
    rf_destroy(f);
    return bad ? 1 : 0;
}
