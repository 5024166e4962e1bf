// vcf_input.h -- input side of the host program: VCF text, gzip / bgzip'd VCF or BCF (raw or BGZF) -> Vcf; --device-input 1 and
// --device-inflate 1 hand the sample columns / the BGZF members to the first device of the run, --device-bcf-input 1 the GT vectors of BCF records
#pragma once
#include <atomic>
#include "cli_args.h"
#include "../vgl_bcfin_core.h"

// ---------------------------------------------------------------------------------------
struct Rec {
    std::string chrom, id, qual, filt, info;
    long pos0;
    std::vector<std::string> alleles;
    std::vector<int8_t> gt;            // 2 per sample, allele index or -1
    std::vector<std::string> gt_str;   // GT tokens as written in the input (for -printTruth)
    char ref_char;
    const uint8_t* dev_row = nullptr;  // --device-input 1 / --device-bcf-input 1: the packed row the device made (Vcf::gt_rows), gt stays empty
    int32_t dev_sum = 0;               //                   and its allele sum
    int8_t in_status = -1;             // --dump-gt: VGL_VCFIN_OK / VGL_VCFIN_HOST of the line (VGL_BCFIN_* of a BCF record)
};

// --device-input: how read_vcf is to parse the sample columns, and what it did (the [input] line of --verbose 1)
struct InputOpt {
    int device_input = 0, source = 0, device = 0, tile_sites = 4096; bool classify = false;
    int device_inflate = 0;                                  // --device-inflate 1: a BGZF file's members are inflated on `device`
    int device_bcf_input = 0;                                // --device-bcf-input 1: the GT vectors of BCF records are decoded on `device`
    bool classify_bcf = false;                               // --dump-gt FILE SOURCE 3: read_bcf also notes the status the device would give each record
    std::function<vgl_inflate_host*()> inflater;            // the host object, created beside the file read (waits for its creation; dies without a device)
};
struct InputStats {
    double t_read = 0, t_scan = 0, t_fixed = 0, t_dev = 0, t_host = 0; long lines_dev = 0, lines_host = 0; int64_t text_up = 0;
    // --device-inflate 1: members inflated on the device, compressed bytes sent up, inflated bytes received, why zlib read the file after all
    long members_dev = 0; int64_t inflate_up = 0, inflate_down = 0; const char* fallback = nullptr; double t_inflate = 0;
    // --device-bcf-input 1: records decoded on the device, those of them decoded again on the host, GT bytes sent up, why read_bcf read the
    // file after all; header and record chain, shared blocks, device decode and wait, host GT loop
    long bcf_dev = 0, bcf_host = 0; int64_t gt_up = 0; const char* bcf_fallback = nullptr; double bt_scan = 0, bt_shared = 0, bt_dev = 0, bt_host = 0;
};

struct Vcf {
    std::vector<std::string> header;   // '##' lines
    std::vector<std::string> samples;
    std::map<std::string, long> contig_len;
    std::vector<Rec> recs;
    std::vector<uint8_t> gt_rows;      // --device-input 1 / --device-bcf-input 1: one row of packed true genotypes per record (Rec::dev_row points here)
};

// ---------------------------------------------------------------------------------------
// BCF 2.x input (raw or BGZF; zlib reads the gzip members): header text, then records decoded back
// into the same Rec the text reader fills -- QUAL / FILTER / INFO as VCF text, GT as allele indices.
// The reader is four parts -- bcf_header, bcf_scan_record, bcf_shared, bcf_formats (+ bcf_gt) -- that read_bcf calls back to back
// and --device-bcf-input 1 calls apart (read_bcf_device).
struct BcfSoftFail {};                 // what a soft cursor throws where a hard one exits
struct BcfDict { std::map<int, std::string> dict, contig; std::map<std::string, int> info_is_flag; };
// a cursor over the file's bytes (it owns nothing: one per thread)
struct BcfIn {
    const uint8_t* buf = nullptr; size_t size = 0, off = 0;
    bool soft = false;                 // --device-bcf-input 1 looks at the file before it decides who reads it: nothing exits
    template <class... A> [[noreturn]] void fail(const char* fmt, A... a) const { if (soft) throw BcfSoftFail(); die(fmt, a...); }
    uint32_t u32() { if (off + 4 > size) fail("truncated BCF record"); uint32_t v; memcpy(&v, buf + off, 4); off += 4; return v; }
    void typed(int& type, int& n) {
        if (off >= size) fail("truncated BCF record");
        const uint8_t b = buf[off++]; type = b & 15; n = b >> 4;
        if (n == 15) { int t2, n2; typed(t2, n2); std::vector<int32_t> v; ints(t2, n2, v); if (v.empty() || v[0] < 0) fail("bad BCF vector length"); n = v[0]; }
    }
    void ints(int type, int n, std::vector<int32_t>& out) {          // missing -> INT32_MIN, end-of-vector -> INT32_MIN + 1
        const int w = type == 1 ? 1 : type == 2 ? 2 : type == 3 ? 4 : 0;
        if (!w) fail("BCF: integer vector expected (type %d)", type);
        if (off + (size_t)w * n > size) fail("truncated BCF record");
        out.clear();
        for (int i = 0; i < n; i++, off += w) {
            int32_t v;
            if (w == 1) { const int8_t x = (int8_t)buf[off]; v = x == -128 ? INT32_MIN : x == -127 ? INT32_MIN + 1 : x; }
            else if (w == 2) { int16_t x; memcpy(&x, buf + off, 2); v = x == -32768 ? INT32_MIN : x == -32767 ? INT32_MIN + 1 : x; }
            else memcpy(&v, buf + off, 4);
            out.push_back(v);
        }
    }
    std::string str(int n) { if (off + n > size) fail("truncated BCF record"); std::string r((const char*)buf + off, n); off += n; return r; }
    static std::string attr(const std::string& h, const char* key) {
        const std::string k = std::string(key) + "=";
        size_t a = h.find("<" + k); if (a == std::string::npos) a = h.find("," + k); if (a == std::string::npos) return "";
        a += k.size() + 1;
        return h.substr(a, h.find_first_of(",>", a) - a);
    }
};
// where a record lies: its shared block (behind the two lengths), its per-sample block, the next record
struct BcfRecAt { size_t shared = 0, shared_end = 0, rec_end = 0; };
// where a record's GT values lie: N vectors of n values of BCF type `type`, from offset `begin` of the file's bytes
struct BcfGtAt { int64_t begin = -1; int type = 0, n = 0; };

// part 1: the header -> the dictionaries, Vcf::header / samples / contig_len; the cursor is left at the first record
static void bcf_header(BcfIn& in, BcfDict& d, Vcf& v) {
    if (in.size < 9 || memcmp(in.buf, "BCF\2", 4) != 0) in.fail("not a BCF2 file");
    in.off = 5;
    const uint32_t l_text = in.u32();
    if (in.off + l_text > in.size) in.fail("truncated BCF header");
    std::string text((const char*)in.buf + in.off, l_text); in.off += l_text;
    while (!text.empty() && (text.back() == '\0' || text.back() == '\n')) text.pop_back();
    std::vector<std::string> lines, f; split(text, '\n', lines);
    int nd = 0, nc = 0; bool have_pass = false;
    for (const std::string& h : lines) if (h.compare(0, 10, "##FILTER=<") == 0 && BcfIn::attr(h, "ID") == "PASS") have_pass = true;
    if (!have_pass) { d.dict[0] = "PASS"; nd = 1; }
    for (const std::string& h : lines) {
        if (h.compare(0, 2, "##") != 0) { if (!h.empty() && h[0] == '#') { split(h, '\t', f); for (size_t i = 9; i < f.size(); i++) v.samples.push_back(f[i]); } continue; }
        v.header.push_back(h);
        const bool fil = h.compare(0, 10, "##FILTER=<") == 0, inf = h.compare(0, 8, "##INFO=<") == 0, fmt = h.compare(0, 10, "##FORMAT=<") == 0;
        const bool ctg = h.compare(0, 10, "##contig=<") == 0;
        if (!(fil || inf || fmt || ctg)) continue;
        const std::string id = BcfIn::attr(h, "ID"), idx_s = BcfIn::attr(h, "IDX");
        if (ctg) {
            const int idx = idx_s.empty() ? nc : atoi(idx_s.c_str());
            d.contig[idx] = id; nc = std::max(nc, idx + 1);
            const std::string len = BcfIn::attr(h, "length"); v.contig_len[id] = len.empty() ? -1 : atol(len.c_str());
            continue;
        }
        int idx = -1;
        for (auto& kv : d.dict) if (kv.second == id) idx = kv.first;
        if (idx < 0) idx = idx_s.empty() ? nd : atoi(idx_s.c_str());
        d.dict[idx] = id; nd = std::max(nd, idx + 1);
        if (inf) d.info_is_flag[id] = BcfIn::attr(h, "Type") == "Flag";
    }
}

// part 2: the two lengths in front of a record; the cursor is left at the shared block
static void bcf_scan_record(BcfIn& in, BcfRecAt& at) {
    const uint32_t l_shared = in.u32(), l_indiv = in.u32();
    at.shared = in.off; at.shared_end = in.off + l_shared; at.rec_end = in.off + (size_t)l_shared + l_indiv;
    if (at.rec_end > in.size) in.fail("truncated BCF record");
}

// part 3: the shared block at the cursor -> Rec; n_fmt = the number of FORMAT fields that follow
static void bcf_shared(BcfIn& in, const BcfDict& d, const BcfRecAt& at, const size_t N, Rec& r, int& n_fmt) {
    std::vector<int32_t> iv; int type, n;
    const int32_t chrom = (int32_t)in.u32(); r.pos0 = (int32_t)in.u32(); (void)in.u32();
    const uint32_t qual = in.u32(), nai = in.u32(), nfs = in.u32();
    const int n_allele = nai >> 16, n_info = nai & 0xFFFF; const size_t n_sample = nfs & 0xFFFFFF;
    n_fmt = nfs >> 24;
    const auto ctg = d.contig.find(chrom);
    if (ctg == d.contig.end()) in.fail("BCF record with an undefined contig index %d", chrom);
    if (n_sample != N) in.fail("Record at position %ld has %zu samples, the header names %zu samples.", r.pos0 + 1, n_sample, N);
    r.chrom = ctg->second;
    if (qual == VGL_FLOAT_MISSING_BITS) r.qual = "."; else { float q; memcpy(&q, &qual, 4); put_float(r.qual, q); }
    in.typed(type, n); r.id = (type == 7) ? in.str(n) : "."; if (r.id.empty()) r.id = ".";
    for (int i = 0; i < n_allele; i++) { in.typed(type, n); if (type != 7) in.fail("BCF: allele string expected"); r.alleles.push_back(in.str(n)); }
    if (r.alleles.empty() || r.alleles[0].empty()) in.fail("Empty REF at position %ld.", r.pos0 + 1);
    r.ref_char = r.alleles[0][0];
    in.typed(type, n);
    if (type == 0 || n == 0) r.filt = ".";
    else { in.ints(type, n, iv); for (size_t i = 0; i < iv.size(); i++) { if (i) r.filt += ';'; const auto k = d.dict.find(iv[i]); if (k == d.dict.end()) in.fail("BCF: undefined FILTER index"); r.filt += k->second; } }
    for (int i = 0; i < n_info; i++) {
        in.typed(type, n); in.ints(type, n, iv);
        const auto k = iv.empty() ? d.dict.end() : d.dict.find(iv[0]);
        if (k == d.dict.end()) in.fail("BCF: undefined INFO key");
        if (!r.info.empty()) r.info += ';';
        r.info += k->second;
        in.typed(type, n);
        if (type == 0 || n == 0) continue;                              // flag
        r.info += '=';
        if (type == 7) r.info += in.str(n);
        else if (type == 5) { for (int j = 0; j < n; j++) { const uint32_t b = in.u32(); if (b == 0x7F800002u) continue; if (j) r.info += ','; float x; memcpy(&x, &b, 4); put_float(r.info, x); } }
        else { in.ints(type, n, iv); bool first = true; for (int32_t x : iv) { if (x == INT32_MIN + 1) continue; if (!first) r.info += ','; first = false; put_int(r.info, x); } }
    }
    if (r.info.empty()) r.info = ".";
    if (in.off != at.shared_end) in.fail("BCF record: shared block length mismatch at position %ld", r.pos0 + 1);
}

// part 4: the GT vectors of N samples at the cursor (n values of `type` each) -> Rec::gt (and the tokens as -printTruth writes them)
static void bcf_gt(BcfIn& in, const int type, const int n, const size_t N, const bool keep_gt_text, Rec& r) {
    std::vector<int32_t> iv;
    for (size_t s = 0; s < N; s++) {
        in.ints(type, n, iv);
        int8_t a[2] = {-1, -1}; std::string txt;
        for (int j = 0; j < n && iv[j] != INT32_MIN + 1; j++) {
            const int al = (iv[j] >> 1) - 1;
            if (j < 2) a[j] = (int8_t)al;
            if (keep_gt_text) { if (j) txt += (iv[j] & 1) ? '|' : '/'; if (al < 0) txt += '.'; else { char t[16]; snprintf(t, sizeof t, "%d", al); txt += t; } }
        }
        if (n == 1 || (n >= 2 && iv[1] == INT32_MIN + 1)) a[1] = a[0];     // haploid call: both alleles, as the text reader does
        r.gt[2 * s] = a[0]; r.gt[2 * s + 1] = a[1];
        if (keep_gt_text) r.gt_str.push_back(txt.empty() ? "." : txt);
    }
}

// the n_fmt FORMAT fields at the cursor: GT is decoded into Rec::gt where it stands (decode) or only found; the others are skipped.
// where = the last GT field's values
static void bcf_formats(BcfIn& in, const BcfDict& d, const size_t N, const int n_fmt, const bool decode, const bool keep_gt_text, Rec& r, BcfGtAt& where) {
    std::vector<int32_t> iv; int type, n;
    bool have_gt = false;
    if (decode) r.gt.assign(2 * N, -1);
    for (int k = 0; k < n_fmt; k++) {
        in.typed(type, n); in.ints(type, n, iv);
        const auto key = iv.empty() ? d.dict.end() : d.dict.find(iv[0]);
        if (key == d.dict.end()) in.fail("BCF: undefined FORMAT key");
        const bool is_gt = key->second == "GT";
        in.typed(type, n);
        const size_t w = type == 1 ? 1 : type == 2 ? 2 : (type == 3 || type == 5) ? 4 : type == 7 ? 1 : 0;
        if (!is_gt) { if (in.off + w * n * N > in.size) in.fail("truncated BCF record"); in.off += w * n * N; continue; }
        if (!decode && have_gt) in.fail("BCF: a second GT field");                       // (soft cursors only: the hard reader decodes both)
        have_gt = true;
        where.begin = (int64_t)in.off; where.type = type; where.n = n;
        if (decode) { bcf_gt(in, type, n, N, keep_gt_text, r); continue; }
        // found only: what decoding N vectors would exit on is a failure here too
        if (N > 0 && (type < 1 || type > 3)) in.fail("BCF: integer vector expected (type %d)", type);
        if (in.off + w * n * N > in.size) in.fail("truncated BCF record");
        in.off += w * n * N;
    }
    if (!have_gt) in.fail("Could not find GT tag at position %ld.", r.pos0 + 1);
}

static bool allele_table(const Rec& r, const int source, int8_t ra[5]);

// classify_source >= 0 (--dump-gt FILE SOURCE 3): every record also gets the status the device decoder would give it, from the shared
// per-sample rule (vgl_bcfin_core.h) on the host
static Vcf read_bcf(std::vector<uint8_t>&& raw, bool keep_gt_text, const int classify_source = -1) {
    BcfDict d; BcfIn in; in.buf = raw.data(); in.size = raw.size();
    Vcf v;
    bcf_header(in, d, v);
    const size_t N = v.samples.size();
    std::vector<uint8_t> row(classify_source >= 0 ? N : 0);
    while (in.off < in.size) {
        BcfRecAt at; BcfGtAt gt; int n_fmt;
        bcf_scan_record(in, at);
        Rec r;
        bcf_shared(in, d, at, N, r, n_fmt);
        bcf_formats(in, d, N, n_fmt, true, keep_gt_text, r, gt);
        if (classify_source >= 0) {
            int8_t ra[5]; int32_t sum;
            r.in_status = (int8_t)(allele_table(r, classify_source, ra)
                                       ? vgl_bcfin::record(in.buf + gt.begin, gt.type, gt.n, (int)r.alleles.size(), ra, (int64_t)N, row.data(), &sum) : VGL_BCFIN_HOST);
        }
        in.off = at.rec_end;
        v.recs.push_back(std::move(r));
    }
    return v;
}

// keep_gt_text: the GT tokens as written are needed only by -printTruth
// The first nine columns of one record line [lb, le) -> Rec, the index of GT in FORMAT and the start of the sample columns.
// strict: exits on a line without ten columns or without GT; otherwise such a line returns false (r is then to be discarded).
static bool parse_fixed(const char* lb, const char* le, const bool strict, Rec& r, int& gti, const char*& samples) {
    const char* col_at[10]; int nc = 0; col_at[0] = lb;
    for (const char* q = lb; q < le && nc < 9; q++) if (*q == '\t') col_at[++nc] = q + 1;
    if (nc < 9) { if (!strict) return false; die("VCF record with fewer than 10 columns (a FORMAT/GT column is required)"); }
    auto col = [&](int k) { return std::string(col_at[k], (size_t)(col_at[k + 1] - 1 - col_at[k])); };
    std::vector<std::string> g, fmt;
    r.chrom = col(0); r.pos0 = atol(col(1).c_str()) - 1; r.id = col(2); r.qual = col(5); r.filt = col(6); r.info = col(7);
    const std::string ref = col(3), alt = col(4);
    r.alleles.push_back(ref);
    if (alt != ".") { split(alt, ',', g); for (auto& x : g) r.alleles.push_back(x); }
    if (ref.empty()) { if (!strict) return false; die("Empty REF at position %ld.", r.pos0 + 1); }
    r.ref_char = ref[0];
    split(col(8), ':', fmt);
    gti = -1; for (size_t i = 0; i < fmt.size(); i++) if (fmt[i] == "GT") gti = (int)i;
    if (gti < 0) { if (!strict) return false; die("Could not find GT tag at position %ld.", r.pos0 + 1); }
    samples = col_at[9];
    return true;
}

// The sample columns [p, le) of a record line -> Rec::gt (and the tokens as written)
static void parse_samples(const char* p, const char* le, const int gti, const size_t n_hdr, const bool keep_gt_text, Rec& r) {
    r.gt.assign(2 * n_hdr, -1);
    const char* const end = le;
    size_t s = 0;
    while (true) {                                       // p at the start of a sample column
        const char* ce = (const char*)memchr(p, '\t', (size_t)(end - p)); if (!ce) ce = end;
        if (s >= n_hdr) { s++; if (ce == end) break; p = ce + 1; continue; }
        const char* t = p;                               // the gti-th ':'-separated subfield; trailing ones may be dropped
        for (int k = 0; k < gti && t; k++) { t = (const char*)memchr(t, ':', (size_t)(ce - t)); if (t) t++; }
        const char* te = t ? (const char*)memchr(t, ':', (size_t)(ce - t)) : nullptr; if (t && !te) te = ce;
        int8_t a0 = -1, a1 = -1;
        if (t) {
            const char* sep = t; while (sep < te && *sep != '|' && *sep != '/') sep++;
            auto allele = [](const char* b, const char* e) -> int8_t { return (b == e || *b == '.') ? (int8_t)-1 : (int8_t)atoi(std::string(b, e).c_str()); };
            a0 = allele(t, sep);
            a1 = (sep == te) ? a0 : allele(sep + 1, te);
            if (keep_gt_text) r.gt_str.emplace_back(t, te);
        } else if (keep_gt_text) r.gt_str.emplace_back(".");
        r.gt[2 * s] = a0; r.gt[2 * s + 1] = a1;
        s++;
        if (ce == end) break;
        p = ce + 1;
    }
    if (s != n_hdr) die("Record at position %ld has %zu sample columns, the header names %zu samples.", r.pos0 + 1, s, n_hdr);
}

// one record line [lb, le) -> Rec (thread safe: records are parsed in parallel)
static void parse_record(const char* lb, const char* le, const size_t n_hdr, const bool keep_gt_text, Rec& r) {
    int gti; const char* p;
    parse_fixed(lb, le, true, r, gti, p);
    parse_samples(p, le, gti, n_hdr, keep_gt_text, r);
}

// --dump-gt: the status the device parser gives the sample columns [p, le) (include/vcfgl_hip.h: the plain grammar), on the host
static int classify_samples(const char* p, const char* le, const int gti, const int n_alleles, const size_t n_hdr) {
    size_t s = 0; bool plain = true;
    auto allele = [&](const char*& q, const char* te) {          // '.' or one or two digits below n_alleles
        if (q == te) return false;
        if (*q == '.') { q++; return true; }
        if (*q < '0' || *q > '9') return false;
        int v = *q++ - '0';
        if (q < te && *q >= '0' && *q <= '9') v = v * 10 + (*q++ - '0');
        return v < n_alleles;
    };
    while (true) {
        const char* ce = (const char*)memchr(p, '\t', (size_t)(le - p)); if (!ce) ce = le;
        const char* t = p;
        for (int k = 0; k < gti && t; k++) { t = (const char*)memchr(t, ':', (size_t)(ce - t)); if (t) t++; }
        if (t) {
            const char* te = (const char*)memchr(t, ':', (size_t)(ce - t)); if (!te) te = ce;
            const char* q = t;
            if (!allele(q, te)) plain = false;
            else if (q != te) { if (*q != '|' && *q != '/') plain = false; else { q++; if (!allele(q, te) || q != te) plain = false; } }
        }
        s++;
        if (ce == le) break;
        p = ce + 1;
    }
    return (plain && s == n_hdr) ? VGL_VCFIN_OK : VGL_VCFIN_HOST;
}

// allele_char_to_int, vcfgl.cpp:20-50
static int allele_to_int(const std::string& a) {
    if (a.size() > 1) return (a == "<*>" || a == "<NON_REF>") ? 4 : -1;
    switch (a[0]) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

// make_site's allele table ra[] for a record, without its exits: false where make_site would refuse the record
static bool allele_table(const Rec& r, const int source, int8_t ra[5]) {
    for (int i = 0; i < 5; i++) ra[i] = -1;
    const int n = (int)r.alleles.size();
    if (n > 5 || (source == 0 && n > 2)) return false;
    for (int i = 0; i < n; i++) {
        if (source == 1) { const int x = r.alleles[i].empty() ? -1 : allele_to_int(r.alleles[i]); if (x == -1) return false; ra[i] = (int8_t)x; }
        else { const int x = (r.alleles[i].empty() ? 0 : r.alleles[i][0]) - '0'; if (x != 0 && x != 1) return false; ra[i] = (int8_t)x; }
    }
    return true;
}

// --device-input 1: the record lines' first nine columns on `threads` host threads, their sample columns on the device in batches of
// at most tile_sites lines (vgl_vcfin_host_*: one batch is copied up and parsed while the next is put together), and the host's own
// parser for every line the device hands back (VGL_VCFIN_HOST) or the fixed columns cannot describe -- its exits and messages are
// therefore those of --device-input 0.
static void parse_lines_device(const uint8_t* raw, const std::vector<std::pair<const char*, const char*>>& rec_lines, const size_t n_hdr,
                               const bool keep_gt_text, const int threads, const InputOpt& opt, Vcf& v, InputStats& st) {
    const int n = (int)rec_lines.size();
    const int N = (int)n_hdr;
    double t0 = now_s();
    std::vector<int64_t> lb((size_t)n), le((size_t)n);
    std::vector<int32_t> gti((size_t)n), nal((size_t)n);
    std::vector<int8_t> amap((size_t)n * 5);
    std::vector<uint8_t> sent((size_t)n, 0);
    vsink::parallel_for(n, threads, [&](int i) {
        Rec& r = v.recs[i];
        int g = -1; const char* p = nullptr;
        if (parse_fixed(rec_lines[i].first, rec_lines[i].second, false, r, g, p) && allele_table(r, opt.source, &amap[(size_t)i * 5])) {
            lb[i] = p - (const char*)raw; le[i] = rec_lines[i].second - (const char*)raw; gti[i] = g; nal[i] = (int32_t)r.alleles.size();
            sent[i] = 1;
        } else { r = Rec(); parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); r.in_status = VGL_VCFIN_HOST; }
    });
    st.t_fixed = now_s() - t0; t0 = now_s();
    const int TS = std::max(1, opt.tile_sites);
    const int nb = (n + TS - 1) / TS;
    // a batch: the sent lines among TS consecutive ones, and the text from the first one's sample columns to the last one's end
    struct Batch { std::vector<int> idx; int64_t t0 = 0, t1 = 0; };
    std::vector<Batch> batches((size_t)nb);
    int64_t max_text = 1; int max_lines = 1;
    for (int b = 0; b < nb; b++) {
        Batch& B = batches[b];
        for (int i = b * TS; i < std::min(n, (b + 1) * TS); i++) if (sent[i]) B.idx.push_back(i);
        if (B.idx.empty()) continue;
        B.t0 = lb[B.idx.front()]; B.t1 = le[B.idx.back()];
        max_text = std::max(max_text, B.t1 - B.t0); max_lines = std::max(max_lines, (int)B.idx.size());
    }
    v.gt_rows.resize((size_t)n * (size_t)N);
    std::vector<int> again;                                          // lines the device handed back
    vgl_vcfin_host* h = nullptr;
    if (vgl_vcfin_host_create(opt.device, N, max_lines, max_text, &h) != VGL_OK) die("--device-input 1: %s", vgl_last_error());
    std::vector<int64_t> blb[2], ble[2]; std::vector<int32_t> bg[2], bn[2]; std::vector<int8_t> bm[2];
    int32_t ticket[2] = {-1, -1};
    auto submit = [&](int b) {
        const Batch& B = batches[b]; const int k = b & 1; const size_t m = B.idx.size();
        blb[k].resize(m); ble[k].resize(m); bg[k].resize(m); bn[k].resize(m); bm[k].resize(m * 5);
        for (size_t j = 0; j < m; j++) {
            const int i = B.idx[j];
            blb[k][j] = lb[i] - B.t0; ble[k][j] = le[i] - B.t0; bg[k][j] = gti[i]; bn[k][j] = nal[i]; memcpy(&bm[k][j * 5], &amap[(size_t)i * 5], 5);
        }
        if (vgl_vcfin_host_submit(h, raw + B.t0, B.t1 - B.t0, (int32_t)m, blb[k].data(), ble[k].data(), bg[k].data(), bn[k].data(), bm[k].data(), &ticket[k]) != VGL_OK)
            die("--device-input 1: %s", vgl_last_error());
        st.text_up += m ? B.t1 - B.t0 : 0; st.lines_dev += (long)m;
    };
    auto retire = [&](int b) {
        const Batch& B = batches[b];
        const uint8_t* rows; const int32_t* sums; const int32_t* status;
        if (vgl_vcfin_host_wait(h, ticket[b & 1], &rows, &sums, &status) != VGL_OK) die("--device-input 1: %s", vgl_last_error());
        for (size_t j = 0; j < B.idx.size(); j++) {
            const int i = B.idx[j];
            if (status[j] != VGL_VCFIN_OK) { again.push_back(i); continue; }
            uint8_t* dst = &v.gt_rows[(size_t)i * (size_t)N];
            memcpy(dst, rows + j * (size_t)N, (size_t)N);
            v.recs[i].dev_row = dst; v.recs[i].dev_sum = sums[j]; v.recs[i].in_status = VGL_VCFIN_OK;
        }
    };
    two_in_flight(nb, submit, retire);
    vgl_vcfin_host_destroy(h);
    st.t_dev = now_s() - t0; t0 = now_s();
    st.lines_host = (long)again.size();
    vsink::parallel_for((int)again.size(), threads, [&](int k) {
        const int i = again[k]; Rec& r = v.recs[i];
        r = Rec(); parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); r.in_status = VGL_VCFIN_HOST;
    });
    // -printTruth 1 writes the GT tokens as they stand in the input: collected on the host, as with --device-input 0
    if (keep_gt_text) vsink::parallel_for(n, threads, [&](int i) {
        Rec& r = v.recs[i];
        if (r.dev_row) { parse_samples((const char*)raw + lb[i], rec_lines[i].second, gti[i], n_hdr, true, r); r.gt.clear(); r.gt.shrink_to_fit(); }
    });
    st.t_host = now_s() - t0;
}

// --device-bcf-input 1: the header and the l_shared / l_indiv chain on one thread, then per record on `threads` host threads the shared
// block -> Rec and a walk over the FORMAT field headers that finds GT's values; only those slices are copied into the staging
// (vgl_bcfin_host_*: the other FORMAT fields never cross the link), in batches of at most tile_sites records, batch b submitted before
// batch b - 1 is retired.  Rows go to Vcf::gt_rows / Rec::dev_row / dev_sum, which make_site copies.  A record the device hands back
// (VGL_BCFIN_HOST) or whose alleles allele_table refuses gets the host's own GT loop, bcf_gt -- the exits of make_site stay what they
// are.  false, with the reason in st.bcf_fallback and v as it was, when the file holds anything read_bcf exits on (or a second GT field,
// or more records than an int counts): read_bcf then reads the whole file, so that its messages and their order are those of
// --device-bcf-input 0.
static bool read_bcf_device(const std::vector<uint8_t>& raw, const bool keep_gt_text, const int threads, const InputOpt& opt, Vcf& v, InputStats& st) {
    double t0 = now_s();
    BcfDict d; BcfIn in; in.buf = raw.data(); in.size = raw.size(); in.soft = true;
    std::vector<BcfRecAt> at;
    auto give_up = [&](const char* why) { v = Vcf(); st.bcf_fallback = why; return false; };
    try {
        bcf_header(in, d, v);
        while (in.off < in.size) { BcfRecAt a; bcf_scan_record(in, a); at.push_back(a); in.off = a.rec_end; }
    } catch (const BcfSoftFail&) { return give_up("the header or the chain of record lengths is damaged"); }
    const size_t N = v.samples.size();
    if (N == 0 || N > (size_t)INT32_MAX) return give_up("the header names no sample");
    if (at.size() > (size_t)INT32_MAX) return give_up("more records than one run counts");
    const int n = (int)at.size();
    st.bt_scan = now_s() - t0; t0 = now_s();
    v.recs.resize((size_t)n);
    std::vector<BcfGtAt> gt((size_t)n);
    std::vector<int8_t> amap((size_t)n * 5);
    std::vector<uint8_t> sent((size_t)n, 0);
    std::atomic<bool> failed(false);
    vsink::parallel_for(n, threads, [&](int i) {
        if (failed.load(std::memory_order_relaxed)) return;
        BcfIn c = in; c.off = at[i].shared;
        Rec& r = v.recs[i];
        try { int n_fmt; bcf_shared(c, d, at[i], N, r, n_fmt); bcf_formats(c, d, N, n_fmt, false, false, r, gt[i]); }
        catch (const BcfSoftFail&) { failed.store(true, std::memory_order_relaxed); return; }
        sent[i] = allele_table(r, opt.source, &amap[(size_t)i * 5]) ? 1 : 0;
    });
    if (failed.load()) return give_up("a record holds what the host reader exits on");
    st.bt_shared = now_s() - t0; t0 = now_s();
    auto slice_bytes = [&](int i) { const int w = vgl_bcfin::width(gt[i].type); return (w && gt[i].n >= 1) ? (int64_t)N * gt[i].n * w : (int64_t)0; };
    const int TS = std::max(1, opt.tile_sites);
    const int nb = (n + TS - 1) / TS;
    struct Batch { std::vector<int> idx; int64_t bytes = 0; };      // the sent records among TS consecutive ones, and their GT bytes
    std::vector<Batch> batches((size_t)nb);
    int64_t max_bytes = 1; int max_recs = 1;
    for (int b = 0; b < nb; b++) {
        Batch& B = batches[b];
        for (int i = b * TS; i < std::min(n, (b + 1) * TS); i++) if (sent[i]) { B.idx.push_back(i); B.bytes += slice_bytes(i); }
        max_bytes = std::max(max_bytes, B.bytes); max_recs = std::max(max_recs, (int)B.idx.size());
    }
    v.gt_rows.resize((size_t)n * N);
    std::vector<int> again;                                          // records whose GT the host decodes: handed back, or never sent
    for (int i = 0; i < n; i++) if (!sent[i]) again.push_back(i);
    vgl_bcfin_host* h = nullptr;
    if (vgl_bcfin_host_create(opt.device, (int32_t)N, max_recs, max_bytes, &h) != VGL_OK) die("--device-bcf-input 1: %s", vgl_last_error());
    std::vector<int64_t> bb[2]; std::vector<int32_t> bt[2], bn[2], ba[2]; std::vector<int8_t> bm[2];
    int32_t ticket[2] = {-1, -1};
    auto submit = [&](int b) {
        const Batch& B = batches[b]; const int k = b & 1; const size_t m = B.idx.size();
        bb[k].resize(m); bt[k].resize(m); bn[k].resize(m); ba[k].resize(m); bm[k].resize(m * 5);
        for (size_t j = 0; j < m; j++) {
            const int i = B.idx[j];
            bb[k][j] = gt[i].begin; bt[k][j] = gt[i].type; bn[k][j] = gt[i].n; ba[k][j] = (int32_t)v.recs[i].alleles.size(); memcpy(&bm[k][j * 5], &amap[(size_t)i * 5], 5);
        }
        if (vgl_bcfin_host_submit(h, raw.data(), (int64_t)raw.size(), (int32_t)m, bb[k].data(), bt[k].data(), bn[k].data(), ba[k].data(), bm[k].data(), &ticket[k]) != VGL_OK)
            die("--device-bcf-input 1: %s", vgl_last_error());
        st.gt_up += B.bytes; st.bcf_dev += (long)m;
    };
    auto retire = [&](int b) {
        const Batch& B = batches[b];
        const uint8_t* rows; const int32_t* sums; const int32_t* status;
        if (vgl_bcfin_host_wait(h, ticket[b & 1], &rows, &sums, &status) != VGL_OK) die("--device-bcf-input 1: %s", vgl_last_error());
        for (size_t j = 0; j < B.idx.size(); j++) {
            const int i = B.idx[j];
            if (status[j] != VGL_BCFIN_OK) { again.push_back(i); st.bcf_host++; continue; }
            uint8_t* dst = &v.gt_rows[(size_t)i * N];
            memcpy(dst, rows + j * N, N);
            v.recs[i].dev_row = dst; v.recs[i].dev_sum = sums[j]; v.recs[i].in_status = VGL_BCFIN_OK;
        }
    };
    two_in_flight(nb, submit, retire);
    vgl_bcfin_host_destroy(h);
    st.bt_dev = now_s() - t0; t0 = now_s();
    // today's loop for the records left to the host; with -printTruth 1 also for the others: the GT tokens are built on the host as
    // with --device-bcf-input 0 (the flag does not make that faster)
    BcfIn hard = in; hard.soft = false;
    vsink::parallel_for((int)again.size(), threads, [&](int k) {
        const int i = again[k]; Rec& r = v.recs[i];
        BcfIn c = hard; c.off = (size_t)gt[i].begin;
        r.gt.assign(2 * N, -1); bcf_gt(c, gt[i].type, gt[i].n, N, keep_gt_text, r); r.in_status = VGL_BCFIN_HOST;
    });
    if (keep_gt_text) vsink::parallel_for(n, threads, [&](int i) {
        Rec& r = v.recs[i];
        if (!r.dev_row) return;
        BcfIn c = hard; c.off = (size_t)gt[i].begin;
        r.gt.assign(2 * N, -1); bcf_gt(c, gt[i].type, gt[i].n, N, true, r); r.gt.clear(); r.gt.shrink_to_fit();
    });
    st.bt_host = now_s() - t0;
    return true;
}

// keep_gt_text: the GT tokens as written are needed only by -printTruth.  The (decompressed) file is read whole,
// the header lines are taken in order and the record lines are parsed on `threads` threads.
// --device-inflate 1: the file as it lies on the disk, its members listed by vgl_bgzf_index and inflated on the device in batches of
// 512 (the compressor's batch: 32 MiB of output at most), two batches in flight.  false, with the reason in st.fallback, when the
// file is not a series of BGZF members or a member came back VGL_INFLATE_HOST: zlib then reads the whole file as without the flag,
// so that a damaged file gives what it gives today.  A device error ends the run.
static const int INFLATE_BATCH = 512;
static bool inflate_on_device(const std::string& fn, const InputOpt& opt, std::vector<uint8_t>& raw, InputStats& st) {
    std::vector<uint8_t> file;
    {
        FILE* f = fopen(fn.c_str(), "rb");
        if (!f) die("Could not open file: %s", fn.c_str());
        std::vector<uint8_t> chunk(1 << 22);
        size_t k;
        while ((k = fread(chunk.data(), 1, chunk.size(), f)) > 0) file.insert(file.end(), chunk.begin(), chunk.begin() + k);
        fclose(f);
    }
    vgl_inflate_host* h = opt.inflater();                 // (without a device the run ends here, whatever the file holds)
    const double t0 = now_s();
    const int64_t cap = (int64_t)file.size() / 28 + 1;
    std::vector<int64_t> begin((size_t)cap); std::vector<int32_t> csize((size_t)cap), isize((size_t)cap);
    int64_t n = 0;
    if (file.empty() || vgl_bgzf_index(file.data(), (int64_t)file.size(), cap, begin.data(), csize.data(), isize.data(), &n) != VGL_OK) {
        st.fallback = "the file is not a series of BGZF members"; st.t_inflate = now_s() - t0;
        return false;
    }
    int64_t total = 0;
    for (int64_t m = 0; m < n; m++) total += isize[(size_t)m];
    raw.resize((size_t)total);
    const int64_t n_batches = (n + INFLATE_BATCH - 1) / INFLATE_BATCH;
    int32_t ticket[2] = {0, 0};
    bool ok = true;
    int64_t out_at = 0;
    auto submit = [&](int64_t b) {
        const int64_t m0 = b * INFLATE_BATCH, m1 = std::min(n, m0 + INFLATE_BATCH);
        const int64_t lo = begin[(size_t)m0], hi = begin[(size_t)m1 - 1] + csize[(size_t)m1 - 1];
        std::vector<int64_t> rel((size_t)(m1 - m0));
        for (int64_t m = m0; m < m1; m++) rel[(size_t)(m - m0)] = begin[(size_t)m] - lo;
        if (vgl_inflate_host_submit(h, file.data() + lo, hi - lo, (int32_t)(m1 - m0), rel.data(), csize.data() + m0, isize.data() + m0, &ticket[b & 1]) != VGL_OK)
            die("--device-inflate 1: %s", vgl_last_error());
        st.inflate_up += hi - lo;
    };
    auto retire = [&](int64_t b) {
        const uint8_t* out; int64_t out_n; const int32_t* status;
        if (vgl_inflate_host_wait(h, ticket[b & 1], &out, &out_n, &status) != VGL_OK) die("--device-inflate 1: %s", vgl_last_error());
        const int64_t m0 = b * INFLATE_BATCH, m1 = std::min(n, m0 + INFLATE_BATCH);
        for (int64_t m = m0; m < m1; m++) if (status[m - m0] != VGL_INFLATE_OK) ok = false;
        if (out_at + out_n > total) die("--device-inflate 1: a batch returned more bytes than its members' ISIZE fields hold");
        if (out_n > 0) memcpy(raw.data() + out_at, out, (size_t)out_n);
        out_at += out_n; st.inflate_down += out_n; st.members_dev += (long)(m1 - m0);
    };
    two_in_flight(n_batches, submit, retire);
    st.t_inflate = now_s() - t0;
    if (!ok) { st.fallback = "a member was left to the host (VGL_INFLATE_HOST)"; raw.clear(); return false; }
    return true;
}

static Vcf read_vcf(const std::string& fn, bool keep_gt_text, int threads, const InputOpt& opt = InputOpt(), InputStats* stats = nullptr) {
    InputStats st; double t0 = now_s();
    std::vector<uint8_t> raw;
    if (!opt.device_inflate || !inflate_on_device(fn, opt, raw, st)) raw = read_whole(fn);
    if (raw.size() >= 3 && !memcmp(raw.data(), "BCF", 3)) {
        if (opt.device_input) die("--device-input 1 is not supported with BCF input (its genotypes are binary already: there is no text to parse).");
        st.t_read = now_s() - t0;
        if (opt.device_bcf_input) {
            Vcf v;
            const bool done = read_bcf_device(raw, keep_gt_text, threads, opt, v, st);
            if (stats) *stats = st;
            if (done) return v;
        }
        if (stats) *stats = st;
        return read_bcf(std::move(raw), keep_gt_text, opt.classify_bcf ? opt.source : -1);
    }
    if (opt.device_bcf_input) die("--device-bcf-input 1 needs BCF input (the genotype columns of VCF text are what --device-input 1 parses).");
    st.t_read = now_s() - t0; t0 = now_s();
    Vcf v;
    std::vector<std::string> f;
    std::vector<std::pair<const char*, const char*>> rec_lines;
    const char* p = (const char*)raw.data(); const char* const end = p + raw.size();
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (le > p) {
            if (le - p >= 2 && p[0] == '#' && p[1] == '#') {
                const std::string line(p, le);
                v.header.push_back(line);
                if (line.compare(0, 10, "##contig=<") == 0) {
                    size_t a = line.find("ID="), l = line.find("length=");
                    if (a != std::string::npos) {
                        std::string id = line.substr(a + 3, line.find_first_of(",>", a) - a - 3);
                        v.contig_len[id] = (l != std::string::npos) ? atol(line.c_str() + l + 7) : -1;
                    }
                }
            } else if (p[0] == '#') { split(std::string(p, le), '\t', f); for (size_t i = 9; i < f.size(); i++) v.samples.push_back(f[i]); }
            else rec_lines.emplace_back(p, le);
        }
        p = nl ? nl + 1 : end;
    }
    st.t_scan = now_s() - t0; t0 = now_s();
    v.recs.resize(rec_lines.size());
    const size_t n_hdr = v.samples.size();
    if (opt.device_input && n_hdr > 0) parse_lines_device(raw.data(), rec_lines, n_hdr, keep_gt_text, threads, opt, v, st);
    else {
        vsink::parallel_for((int)rec_lines.size(), threads, [&](int i) {
            Rec& r = v.recs[i];
            if (!opt.classify) { parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); return; }
            int gti; const char* sp;
            parse_fixed(rec_lines[i].first, rec_lines[i].second, true, r, gti, sp);
            parse_samples(sp, rec_lines[i].second, gti, n_hdr, keep_gt_text, r);
            r.in_status = (int8_t)classify_samples(sp, rec_lines[i].second, gti, (int)r.alleles.size(), n_hdr);
        });
        st.t_host = now_s() - t0; st.lines_host = (long)rec_lines.size();
    }
    if (stats) *stats = st;
    return v;
}

// the first device the run selected: it warms the HIP runtime, parses / inflates the input and compresses BGZF streams
static int first_device(const Args& a) { return a.devices.empty() ? a.device : a.devices[0]; }
// --device-bgzf 1: that device compresses every BGZF stream of the run (-1: zlib on the host)
static int bgzf_device(const Args& a) { return a.device_bgzf ? first_device(a) : -1; }

// host threads for parsing and record encoding: --encode-threads, else --threads when given, else up to 8 of the
// machine's threads -- the bytes written do not depend on it
static int encode_threads(const Args& a) {
    if (a.enc_threads > 0) return a.enc_threads;
    if (a.threads_given) return a.threads;
    return (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
}

// The run's input.  The HIP runtime initialises (about 0.07 s) while the file is read and parsed
// (on the first device the run selected: a primary context on GPU 0 would otherwise be created for a run that never uses it;
//  a failure here is not swallowed for good -- vgl_ctx_create on the same device reports it later)
static Vcf read_input(const Args& a, const int threads, InputStats& stats) {
    std::thread hip_warm;
    const int warm_dev = first_device(a);
    // --device-inflate 1: the inflater's page-locked staging and device buffers are made on that thread too, while the file is read
    vgl_inflate_host* inflater = nullptr; int inflater_rc = VGL_OK; std::string inflater_err;
    const bool want_inflater = a.device_inflate == 1;
    if (!a.depth_inf || a.device_inf) hip_warm = std::thread([warm_dev, want_inflater, &inflater, &inflater_rc, &inflater_err] {
        vgl_host_free(vgl_host_alloc_on(warm_dev, 4096));
        if (want_inflater && (inflater_rc = vgl_inflate_host_create(warm_dev, INFLATE_BATCH, &inflater)) != VGL_OK) inflater_err = vgl_last_error();
    });
    InputOpt in_opt; in_opt.device_inflate = a.device_inflate;
    in_opt.inflater = [&]() -> vgl_inflate_host* {
        if (hip_warm.joinable()) hip_warm.join();
        if (inflater_rc != VGL_OK || !inflater) die("--device-inflate 1: %s", inflater_err.c_str());
        return inflater;
    };
    in_opt.device_input = a.device_input; in_opt.device_bcf_input = a.device_bcf_input; in_opt.source = a.source; in_opt.device = warm_dev; in_opt.tile_sites = a.tile_sites > 0 ? a.tile_sites : 4096;
    Vcf vcf = read_vcf(a.in_fn, a.print_truth != 0, threads, in_opt, &stats);
    if (hip_warm.joinable()) hip_warm.join();
    if (inflater) vgl_inflate_host_destroy(inflater);
    return vcf;
}
