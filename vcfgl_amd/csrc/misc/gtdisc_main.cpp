// gtdisc_main.cpp -- gtdiscordance_hip: the reference's misc/gtDiscordance (a call file against -printTruth's file) for this platform.
//   gtdiscordance_hip -t truth -i call -o out [-doGQ 0..8] [-perSite 0|1] [--on-device 0|1] [--device INT] [--batch-records INT] [--verbose 0|1] [--device-inflate 0|1] [--bcf-direct 0|1]
//                     [--resident 0|1] [--resident-max-bytes INT]
// Both files are read whole (plain, gzip or bgzip text through zlib; BCF records are decoded into the same text lines on the host, or
// under --bcf-direct 1 left as they are and judged from their typed vectors by the rules of gtdbcf_core.h), their
// first nine columns are parsed on the host and the records matched by the tool's sequential merge on POS.  Every matched pair is then
// judged by the PLAIN grammar of gtdisc_core.h -- on the device in batches (--on-device 1: gtdisc.hip) or by the same routines on the
// host (--on-device 0) -- and a record outside that grammar is redone whole by the permissive reader below, which owns every message.
// Both paths therefore write the same bytes.  A run that has to stop does so at the record the tool would stop at: what the records
// before it gave is written first.
// --resident 1 (with --device-inflate 1 and --on-device 1): each file of the pair that is a clean series of BGZF members is inflated
// into device memory and stays there (resident_file.h), the truth file first, the call file within what is left of
// --resident-max-bytes.  Of VCF text the heads alone come down (the # lines, the first nine columns of every other line), of BCF under
// --bcf-direct 1 the records' heads (lengths, shared block, FORMAT keys and descriptors); the nine columns, the merge and every stop
// decided from them are the host code below on those bytes, and the batches' descriptors point into the file where the inflater wrote
// it.  A record the device hands back has its sample columns (BCF: its bytes) copied down for the permissive reader.  A file that
// cannot be resident is read as with --resident 0 -- the other one may still be -- and its [input] line of --verbose 1 says why.
#include <strings.h>
#include "record_file.h"
#include "batch_plan.h"
#include "gtdisc_dev.h"
#include "resident_file.h"

namespace {

struct Opt {
    std::string truth, call, out;
    int do_gq = 0, per_site = 0, on_device = 1, device = 0, batch = 4096, verbose = 0, device_inflate = 0, bcf_direct = 0, resident = 0;
    int64_t resident_max = -1;         // --resident-max-bytes (-1: the device's free memory less 1 GiB)
};

// (--resident 0|1 [0] and --resident-max-bytes INT are taken and not listed here: README and DESIGN.md 4.32 describe them)
const char GTD_USAGE[] =
    "Usage: gtdiscordance_hip -t <truth> -i <call> -o <output.tsv>\n"
    "Options:\n"
    "  -t, --truth <file>        truth file (VCF text, gzip / bgzip'd, or BCF)\n"
    "  -i, --input <file>        input file, to be compared with truth file, typically a genotype call file\n"
    "  -o, --output <file>       output\n"
    "  -doGQ 1                   print the discordance indicator and GQ scores for each sample at each site\n"
    "  -doGQ 2                   print the discordance indicator and GQ scores for each sample at each site, with extra info\n"
    "  -doGQ 3                   print tidy gq summary\n"
    "  -doGQ 4                   print tidy gq summary with hom/het details\n"
    "  -doGQ 5                   per-sample doGQ 3\n"
    "  -doGQ 6                   per-sample doGQ 4\n"
    "  -doGQ 7                   per-sample doGQ 4, for the sites with missing GQ assume highest GQ value\n"
    "  -doGQ 8                   doGQ 7, but for the genotype calling files without GQ tags sets GQ to second lowest PL\n"
    "  -perSite 1                print position, sample, discordance indicator and hom/het type of every compared call to stdout\n"
    "  --on-device 0|1 [1]       1: the sample columns are parsed, tallied and listed on the GPU; 0: on the host, no GPU touched\n"
    "  --device INT [0]          the GPU\n"
    "  --batch-records INT [4096] call records per device batch\n"
    "  --verbose 0|1 [0]         record counts, bytes sent up and stage times\n"
    "  --device-inflate 0|1 [0]  " DEVICE_INFLATE_HELP "\n"
    "  --bcf-direct 0|1 [0]      1: a BCF file is not turned into text: its typed GT / GQ / PL vectors are judged as they lie in the file\n"
    "  -h, --help                print help\n\n";

Opt parse_opt(int argc, char** argv) {
    Opt o;
    if (argc <= 1) { fputs(GTD_USAGE, stderr); exit(0); }
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) { fputs(GTD_USAGE, stderr); exit(0); }
        if (i + 1 >= argc) die("Missing value for arg:%s", a);
        const char* v = argv[++i];
        if (!strcmp(a, "-i") || !strcmp(a, "--input")) o.call = v;
        else if (!strcmp(a, "-t") || !strcmp(a, "--truth")) o.truth = v;
        else if (!strcmp(a, "-o") || !strcmp(a, "--output")) o.out = v;
        else if (!strcasecmp(a, "-doGQ")) { o.do_gq = atoi(v); if (o.do_gq < 0 || o.do_gq > 8) die("Unknown doGq:%d", o.do_gq); }
        else if (!strcasecmp(a, "-perSite")) o.per_site = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--on-device")) o.on_device = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device")) o.device = option_int(a, v, 0, 1 << 20);
        else if (!strcmp(a, "--batch-records")) o.batch = option_int(a, v, 1, 1 << 24);
        else if (!strcmp(a, "--verbose")) o.verbose = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device-inflate")) o.device_inflate = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--bcf-direct")) o.bcf_direct = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident")) o.resident = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident-max-bytes")) {
            char* e; const long long x = strtoll(v, &e, 10);
            if (e == v || *e || x < 0) die("%s takes an integer of at least 0, not '%s'", a, v);
            o.resident_max = x;
        }
        else die("Unknown arg:%s", a);
    }
    if (o.call.empty()) die("Input file not specified. Please use -i/--input <file>.");
    if (o.truth.empty()) die("Truth file not specified. Please use -t/--truth <file>.");
    if (o.out.empty()) die("Output file not specified. Please use -o/--output <file>.");
    if (o.resident && !(o.device_inflate && o.on_device)) die("--resident 1 needs --device-inflate 1 and --on-device 1.");
    return o;
}

// ---- the two files ---------------------------------------------------------------------------------------------------------------
// where the integer GT / GQ / PL vectors of a record lie in the file's bytes (the last field of a key counts; a field of another type
// counts as absent)
struct BcfFields {
    size_t at = 0, rec_end = 0;        // the record's first byte (its two lengths) and the byte behind it
    int64_t off[3] = {0, 0, 0}; int type[3] = {0, 0, 0}, n[3] = {0, 0, 0}; bool have[3] = {false, false, false};      // GT, GQ, PL
    bool as_text = false;              // --bcf-direct 1: the record's whole line stands in Input::text after all
};
enum { F_GT = 0, F_GQ = 1, F_PL = 2 };

struct Input {
    std::vector<uint8_t> text;                                   // the file's text, or the lines made from its BCF records
    std::vector<std::string> header, samples;
    std::vector<std::pair<int64_t, int64_t>> lines;              // [begin, end) of every record line
    // --bcf-direct 1, a BCF file: its bytes as read, its dictionaries and where every record's vectors lie
    bool direct = false;
    std::vector<uint8_t> bcf; BcfDict dict; std::vector<BcfFields> brecs;
    // --resident 1, a resident file: its bytes lie in device memory.  VCF text: `text` is the head stream and record i is line
    // line_of[i] of the file, whose sample columns the split names.  BCF: `bcf` is empty, brecs hold offsets into the file
    RfFile* rf = nullptr; rf::Split split; std::vector<size_t> line_of;
    bool has_format(const char* id) const {
        const std::string k = std::string("##FORMAT=<ID=") + id + ",";
        for (const std::string& h : header) if (h.compare(0, k.size(), k) == 0) return true;
        return false;
    }
    bool vectors(const size_t i) const { return direct && !brecs[i].as_text; }     // record i is judged from its typed vectors
};

// the record at the cursor: its shared block -> r, its FORMAT field headers -> f; the cursor is left behind the record.
// One body for both sources.  heads == nullptr: the cursor walks the file's bytes.  Else (a resident BCF file) it walks the head
// stream -- per record the two lengths, the shared block and the fields' keys and descriptors, bytes identical to the file's -- and
// record i's place in the file gives f.at and the fields' data offsets (bcf_format_fields)
void bcf_walk(BcfIn& c, const BcfDict& d, const size_t N, Rec& r, BcfFields& f, const RbSplit* heads = nullptr, const size_t i = 0) {
    BcfRecAt at; int n_fmt;
    const size_t head_at = c.off;
    size_t file_end = 0;
    if (!heads) { f.at = c.off; bcf_scan_record(c, at); }
    else {                                                             // (the device has made the checks of bcf_scan_record)
        if (i >= (size_t)heads->records || (int64_t)head_at != heads->hoff[i]) die("--resident 1: the head stream does not follow its records.");
        f.at = (size_t)heads->rec_off[i];
        const uint32_t l_shared = c.u32(), l_indiv = c.u32();
        at.shared = c.off; at.shared_end = c.off + l_shared; at.rec_end = (size_t)heads->hoff[i + 1];
        file_end = f.at + 8 + (size_t)l_shared + l_indiv;
    }
    bcf_shared(c, d, at, N, r, n_fmt);
    bcf_format_fields(c, d, n_fmt, N, [&](int, const std::string& key, int type, int n, size_t data_off) {
        if (type < 1 || type > 3) return;                               // (the walker has checked that the vectors lie inside the file)
        const int k = key == "GT" ? F_GT : key == "GQ" ? F_GQ : key == "PL" ? F_PL : -1;
        if (k < 0) return;
        f.off[k] = (int64_t)data_off; f.type[k] = type; f.n[k] = n; f.have[k] = true;
    }, heads ? heads->rec_off[i] + (int64_t)(c.off - head_at) : (int64_t)-1);
    if (heads && c.off != at.rec_end) die("--resident 1: a record's head is not as long as the device made it.");
    if (!f.have[F_GT]) die("Could not find GT tag at position %ld.", r.pos0 + 1);
    c.off = at.rec_end; f.rec_end = heads ? file_end : at.rec_end;
}
// the first nine columns a VCF writer would give the record (the columns nothing reads are '.')
void bcf_nine(const Rec& r, const BcfFields& f, std::string& out) {
    out += r.chrom; out += '\t'; out += std::to_string(r.pos0 + 1); out += "\t.\t"; out += r.alleles[0]; out += '\t';
    if (r.alleles.size() == 1) out += '.';
    for (size_t a = 1; a < r.alleles.size(); a++) { if (a > 1) out += ','; out += r.alleles[a]; }
    out += "\t.\t.\t.\tGT"; if (f.have[F_GQ]) out += ":GQ"; if (f.have[F_PL]) out += ":PL";
}
// its sample columns, each behind a tab
void bcf_columns(const BcfIn& c, const BcfFields& f, const size_t N, std::string& out) {
    std::vector<int32_t> vec[3]; char num[16];
    for (int k = 0; k < 3; k++) if (f.have[k]) { BcfIn v = c; v.off = (size_t)f.off[k]; v.ints(f.type[k], (int)(f.n[k] * N), vec[k]); }
    const std::vector<int32_t>& gt = vec[F_GT]; const std::vector<int32_t>& gq = vec[F_GQ]; const std::vector<int32_t>& pl = vec[F_PL];
    const int n_gt = f.n[F_GT], n_gq = f.n[F_GQ], n_pl = f.n[F_PL];
    auto put = [&](int32_t x) { if (x == INT32_MIN) out += '.'; else { snprintf(num, sizeof num, "%d", x); out += num; } };
    for (size_t s = 0; s < N; s++) {
        out += '\t';
        int j = 0;
        for (; j < n_gt && gt[s * n_gt + j] != INT32_MIN + 1; j++) {
            const int32_t x = gt[s * n_gt + j];
            if (j) out += (x & 1) ? '|' : '/';
            if ((x >> 1) - 1 < 0) out += '.'; else put((x >> 1) - 1);
        }
        if (j == 0) out += '.';
        if (f.have[F_GQ]) { out += ':'; if (n_gq < 1 || gq[s * n_gq] == INT32_MIN + 1) out += '.'; else put(gq[s * n_gq]); }
        if (f.have[F_PL]) {
            out += ':';
            int g = 0;
            for (; g < n_pl && pl[s * n_pl + g] != INT32_MIN + 1; g++) { if (g) out += ','; put(pl[s * n_pl + g]); }
            if (g == 0) out += '.';
        }
    }
}
// the record at byte `at` of the file -> the line a VCF writer would give GT, GQ and PL (no newline)
void bcf_one_line(const std::vector<uint8_t>& raw, const BcfDict& d, const size_t N, const size_t at, std::string& out) {
    BcfIn c; c.buf = raw.data(); c.size = raw.size(); c.off = at;
    Rec r; BcfFields f;
    bcf_walk(c, d, N, r, f);
    bcf_nine(r, f, out); bcf_columns(c, f, N, out);
}

// BCF records -> text.  direct false: the lines of every record.  direct true (--bcf-direct 1): the file's bytes stay as read; the
// text holds a record's first nine columns and a tab -- what parse_nine reads -- and its sample columns are written only on demand
// (Input::line_of).  A record whose first nine columns would not stand where a reader of the line looks for them (a tab inside a
// name), or whose line could pass 2 GiB, gets its whole line here as without the flag.
// A resident file (heads, always direct): raw is the file's header, the cursor then walks the head stream, and a record that gets its
// whole line has its bytes copied down for it.
void bcf_lines(std::vector<uint8_t>& raw, Input& in, const bool direct, const RbSplit* heads = nullptr) {
    BcfIn c; c.buf = raw.data(); c.size = raw.size();
    Vcf v;
    bcf_header(c, in.dict, v);
    if (heads) { c.buf = heads->heads.data(); c.size = heads->heads.size(); c.off = 0; }
    in.header = v.header; in.samples = v.samples;
    const size_t N = v.samples.size();
    std::string out;
    std::vector<uint8_t> rec_bytes;
    for (size_t i = 0; c.off < c.size; i++) {
        Rec r; BcfFields f;
        bcf_walk(c, in.dict, N, r, f, heads, i);
        const int64_t begin = (int64_t)out.size();
        bcf_nine(r, f, out);
        if (direct) {
            int tabs = 0;
            for (size_t q = (size_t)begin; q < out.size(); q++) tabs += out[q] == '\t';
            const double bound = (double)N * (12.0 * ((double)f.n[F_GT] + 1.0 + (double)f.n[F_PL]) + 4.0);
            f.as_text = tabs != 8 || bound > (double)(INT32_MAX / 2);
        }
        if (heads && f.as_text) {
            rec_bytes.resize(f.rec_end - f.at);
            if (rf_fetch(in.rf, (int64_t)f.at, (int64_t)rec_bytes.size(), rec_bytes.data()) != 0) die("--resident 1: %s", rf_error(in.rf));
            out.resize((size_t)begin);
            bcf_one_line(rec_bytes, in.dict, N, 0, out);
        }
        else if (!direct || f.as_text) bcf_columns(c, f, N, out); else out += '\t';
        in.lines.emplace_back(begin, (int64_t)out.size());
        out += '\n';
        if (direct) in.brecs.push_back(f);
    }
    in.text.assign(out.begin(), out.end());
    if (direct) { in.direct = true; if (!heads) in.bcf = std::move(raw); }
}

// the file's bytes as the reader gave them -> the Input
void input_of_bytes(std::vector<uint8_t>& raw, Input& in, const bool bcf_direct) {
    if (raw.size() >= 3 && !memcmp(raw.data(), "BCF", 3)) { bcf_lines(raw, in, bcf_direct); return; }
    in.text = std::move(raw);
    TextLines tl = scan_text(in.text);
    in.header = std::move(tl.header); in.samples = std::move(tl.samples); in.lines = std::move(tl.lines);
}

void read_input_file(FileReader& reader, const std::string& fn, const bool bcf_direct, Input& in) {
    std::vector<uint8_t> raw = reader.read(fn);
    input_of_bytes(raw, in, bcf_direct);
}

// --resident 1, a resident file that begins as BCF: its header and the split of its records (resident_file.h).  nullptr: hdr and
// bsplit hold them; else why the bytes come down whole
const char* load_resident_bcf(RfFile* rf, std::vector<uint8_t>& hdr, RbSplit& bsplit, std::string& why) {
    auto failed = [&]() { die("--resident 1: %s", rf_error(rf)); };
    bool fits = false;
    if (rf_bcf_header(rf, &hdr, &fits) != 0) failed();
    if (!fits) { why = "the header does not fit the file"; return why.c_str(); }
    int64_t n_samples = -1;
    try { BcfDict d; Vcf v; BcfIn c; c.buf = hdr.data(); c.size = hdr.size(); c.soft = true; bcf_header(c, d, v); n_samples = (int64_t)v.samples.size(); }
    catch (const BcfSoftFail&) { why = "the header could not be read"; return why.c_str(); }
    if (rf_bcf_split(rf, (int64_t)hdr.size(), n_samples, rb::RB_HOPS_MOST, rf::RF_HEAD_MOST, &bsplit) != 0) failed();
    if (bsplit.more_records) why = "the file has more records than the offsets scan takes (INT32_MAX - 1024)";
    else if (bsplit.why != rb::OK) { char b[256]; snprintf(b, sizeof b, "record %lld: %s", (long long)bsplit.ordinal + 1, rb::why_text(bsplit.why)); why = b; }
    else return nullptr;
    return why.c_str();
}

// --resident 1: one file of the pair into device memory and its split.  `left` is what --resident-max-bytes leaves this file (-1: the
// device's free memory less 1 GiB, as it is now) and is brought down by what the file takes.  The file is resident (in.rf) or read
// as --resident 0 reads it; the [input] line says which, and why
void read_input_resident(FileReader& reader, const Opt& o, const std::string& fn, int64_t& left, Input& in) {
    char err[256];
    { FILE* fp = fopen(fn.c_str(), "rb"); if (!fp) die("Could not open file: %s", fn.c_str()); fclose(fp); }   // the file first, as without the flag
    RfFile* rf = rf_create(o.device, err, sizeof err);
    if (!rf) die("--resident 1: %s (device %d)", err, o.device);
    const int64_t most = left >= 0 ? left : rf_default_max_bytes(rf);
    auto failed = [&]() { const std::string why = rf_error(rf); if (why.compare(0, 14, "Could not open") == 0) die("%s", why.c_str()); die("--resident 1: %s", why.c_str()); };
    RfWhy why;
    if (rf_load(rf, fn.c_str(), most, &why) != 0) failed();
    const char* reason = nullptr;
    std::vector<uint8_t> raw, hdr; RbSplit bsplit; std::string bcf_why;
    bool have = false, is_bcf = false;                                 // have: raw was copied down from the device
    if (why == RF_NOT_BGZF) reason = "the file is not a series of BGZF members";
    else if (why == RF_MEMBER_HOST) reason = "a member was left to the host (VGL_INFLATE_HOST)";
    else if (why == RF_TOO_LARGE) reason = "the inflated and the compressed bytes exceed what --resident-max-bytes leaves";
    else {
        const int64_t total = rf_total(rf);
        uint8_t first[3] = {0, 0, 0};
        if (rf_fetch(rf, 0, std::min<int64_t>(3, total), first) != 0) failed();
        bool more_lines = false;
        is_bcf = total >= 3 && !memcmp(first, "BCF", 3);
        if (is_bcf && !o.bcf_direct) reason = "the file is BCF and --bcf-direct is 0";
        else if (is_bcf) reason = load_resident_bcf(rf, hdr, bsplit, bcf_why);
        else {
            if (rf_split(rf, rf::RF_HEAD_MOST, &in.split, &more_lines) != 0) failed();
            if (more_lines) reason = "the file has more lines than the offsets scan takes (INT32_MAX - 1024)";
            else if (in.split.over) reason = "a line's ninth tab is not within RF_HEAD_MOST bytes";
        }
        if (reason) {                                                  // the inflated bytes are on the device: they come down whole
            raw.resize((size_t)total);
            if (rf_fetch(rf, 0, total, raw.data()) != 0) failed();
            have = true;
        }
    }
    const RfStats st = *rf_stats(rf);
    if (o.verbose && is_bcf)
        fprintf(stderr, "[input] %s: resident %d%s%s%s, members %lld, records %lld, head bytes received %lld, compressed bytes sent up %lld; upload %.3f s, inflate %.3f s, chain %.3f s, heads %.3f s\n",
                fn.c_str(), reason ? 0 : 1, reason ? " (" : "", reason ? reason : "", reason ? ")" : "", (long long)st.members, (long long)st.records,
                (long long)st.head_bytes, (long long)st.compressed_up, st.t_upload, st.t_inflate, st.t_chain, st.t_heads);
    else if (o.verbose)
        fprintf(stderr, "[input] %s: resident %d%s%s%s, RF_CHUNK %lld, members %lld, lines %lld, head bytes received %lld, compressed bytes sent up %lld; upload %.3f s, inflate %.3f s, split %.3f s\n",
                fn.c_str(), reason ? 0 : 1, reason ? " (" : "", reason ? reason : "", reason ? ")" : "", (long long)rf::RF_CHUNK, (long long)st.members, (long long)st.lines,
                (long long)st.head_bytes, (long long)st.compressed_up, st.t_upload, st.t_inflate, st.t_split);
    if (o.verbose && have) FileReader::report(fn, (long)st.members, st.compressed_up, st.total, st.t_inflate, nullptr);
    if (reason) {
        rf_destroy(rf); in.split = rf::Split();
        if (!have) raw = reader.read(fn);
        input_of_bytes(raw, in, o.bcf_direct != 0);
        return;
    }
    in.rf = rf;
    if (left >= 0) left = std::max<int64_t>(0, left - (st.total + st.compressed_up));
    if (is_bcf) { bcf_lines(hdr, in, true, &bsplit); return; }
    in.text = std::move(in.split.heads);
    TextLines tl = scan_text(in.text);
    in.header = std::move(tl.header); in.samples = std::move(tl.samples); in.lines = std::move(tl.lines);
    in.line_of.resize(in.lines.size());
    size_t ln = 0;                                                     // record i is line ln of the file
    for (size_t i = 0; i < in.lines.size(); i++) { while (in.split.hoff[ln] < in.lines[i].first) ln++; in.line_of[i] = ln; }
}

// the first nine columns of a record line
struct Fixed {
    std::string bad;                   // why the line cannot be compared (the run stops when it gets there)
    int64_t pos = 0, s_off = 0, s_len = 0;
    std::string first;                 // the first character of every allele
    int gti = -1, gqi = -1, pli = -1;
    uint64_t map() const { uint64_t m = 0; for (size_t a = 0; a < 16; a++) m |= (uint64_t)(a < first.size() ? gtd::base_of((uint8_t)first[a]) : 15u) << (4 * a); return m; }
};

Fixed parse_nine(const Input& in, const size_t i, const char* which) {
    Fixed f;
    const char* const t0 = (const char*)in.text.data();
    const char* lb = t0 + in.lines[i].first; const char* le = t0 + in.lines[i].second;
    const char* col_at[10]; int nc;
    nine_columns(lb, le, col_at, nc);
    char msg[256];
    f.pos = pos_column(col_at, nc);
    if (nc < 9) { snprintf(msg, sizeof msg, "Record %zu of the %s file has fewer than 10 columns (a FORMAT/GT column is required).", i + 1, which); f.bad = msg; return f; }
    auto col = [&](int k) { return std::string(col_at[k], (size_t)(col_at[k + 1] - 1 - col_at[k])); };
    const std::string ref = col(3), alt = col(4);
    std::vector<std::string> g;
    if (ref.empty()) { snprintf(msg, sizeof msg, "Empty REF at position %lld of the %s file.", (long long)f.pos, which); f.bad = msg; return f; }
    f.first += ref[0];
    if (alt != ".") { split(alt, ',', g); for (auto& x : g) f.first += x.empty() ? '?' : x[0]; }
    const char* const fmt_end = col_at[9] - 1;
    f.gti = format_key_index(col_at[8], fmt_end, "GT"); f.gqi = format_key_index(col_at[8], fmt_end, "GQ"); f.pli = format_key_index(col_at[8], fmt_end, "PL");
    if (f.gti < 0) { snprintf(msg, sizeof msg, "Could not find GT tag at position %lld of the %s file.", (long long)f.pos, which); f.bad = msg; return f; }
    f.s_off = col_at[9] - t0; f.s_len = le - col_at[9];
    if (in.rf && !in.direct) { f.s_off = in.split.s_off[in.line_of[i]]; f.s_len = in.split.s_len[in.line_of[i]]; }      // (the line's head ends behind its ninth tab)
    if (f.s_len > INT32_MAX) { snprintf(msg, sizeof msg, "The record at position %lld of the %s file is longer than 2 GiB.", (long long)f.pos, which); f.bad = msg; }
    return f;
}

// a call record and the truth record it is compared with
struct Pair { size_t ci, ti; int32_t nsites1; gtd::Rec rec; gtd::BSide tside, cside; };    // (a side with have == 0 is text; offsets of a BCF side count from the file's first byte)

// ---- the run's state -------------------------------------------------------------------------------------------------------------
struct Run {
    Opt o;
    Input truth, call;
    std::vector<Fixed> tf, cf;
    std::vector<Pair> pairs;
    std::string stop;                  // why the run ends behind the last pair (empty: it does not)
    int32_t N = 0;
    int list = 0;
    std::vector<int64_t> table;        // cells and call-missing counts the host tallied
    FILE* out_fp = nullptr;
    std::string list_buf, site_buf;
    GtdDev* dev = nullptr;
    long n_host = 0, n_timed = 0; int64_t text_up = 0;
    long n_direct[2] = {0, 0}; int64_t vec_up = 0; double ms_stage = 0, ms_decode = 0; long n_batches = 0;      // --bcf-direct 1
    double t_read = 0, t_nine = 0, t_dev = 0, t_host = 0;

    void flush(bool all) {
        if (all || list_buf.size() > (1u << 22)) { if (!list_buf.empty()) fwrite(list_buf.data(), 1, list_buf.size(), out_fp); list_buf.clear(); }
        if (all || site_buf.size() > (1u << 22)) { if (!site_buf.empty()) fwrite(site_buf.data(), 1, site_buf.size(), stdout); site_buf.clear(); }
    }
    // the run ends here: what the records so far gave is written, nothing stays in flight on the device
    [[noreturn]] void stop_run(const char* fmt, ...) {
        if (dev) gtd_dev_quiesce(dev);
        flush(true); fflush(out_fp);
        va_list ap; va_start(ap, fmt); die_v(fmt, ap);
    }
    void count(const int32_t s, const uint32_t cell, const uint32_t gq) { table[((size_t)s * gtd::N_CELLS + cell) * gtd::N_GQ + gq]++; }
    void call_missing(const int32_t s) { table[(size_t)N * gtd::N_CELLS * gtd::N_GQ + s]++; }
    void lines(const Pair& p, const int32_t s, const uint32_t cell, const uint32_t gq) {
        uint8_t b[gtd::LINE_BOUND];
        if (list) { gtd::Emit<true> e{b, 0u, (uint32_t)sizeof b}; gtd::list_line(e, list, p.nsites1, (uint32_t)s, cell, gq); list_buf.append((const char*)b, e.n); }
        if (o.per_site) { gtd::Emit<true> e{b, 0u, (uint32_t)sizeof b}; gtd::site_line(e, p.rec.pos, (uint32_t)s, cell); site_buf.append((const char*)b, e.n); }
    }
    typedef std::pair<const char*, const char*> Span;
    Span sample_columns(const Input& in, size_t i, const Fixed& F, std::string& line);
    void record_permissive(const Pair& p);
    void record_host(const Pair& p, std::vector<uint8_t>& planes);
};

// ---- the permissive reader: one record by the tool's own rules, with the run's messages --------------------------------------------
typedef std::pair<const char*, const char*> Span;
void split_cols(const char* b, const char* e, std::vector<Span>& out) {
    out.clear();
    for (;;) { const char* t = (const char*)memchr(b, '\t', (size_t)(e - b)); if (!t) { out.emplace_back(b, e); return; } out.emplace_back(b, t); b = t + 1; }
}
bool nth_field(Span c, const int k, Span& f) {
    const char* b = c.first;
    for (int i = 0; i < k; i++) { b = (const char*)memchr(b, ':', (size_t)(c.second - b)); if (!b) return false; b++; }
    const char* e = (const char*)memchr(b, ':', (size_t)(c.second - b));
    f = Span(b, e ? e : c.second);
    return true;
}
// an integer of at most nine digits, with or without '-'
bool host_int(const char* b, const char* e, long& v) {
    const bool neg = b < e && *b == '-'; if (neg) b++;
    if (b == e || e - b > 9) return false;
    v = 0;
    for (; b < e; b++) { if (*b < '0' || *b > '9') return false; v = v * 10 + (*b - '0'); }
    if (neg) v = -v;
    return true;
}
// two alleles, each '.' or an index: a0 / a1 = -1 for '.'
bool host_gt(Span f, long& a0, long& a1) {
    const char* s = f.first; while (s < f.second && *s != '/' && *s != '|') s++;
    if (s == f.second) return false;
    auto one = [](const char* b, const char* e, long& a) { if (e - b == 1 && *b == '.') { a = -1; return true; } return host_int(b, e, a) && a >= 0; };
    return one(f.first, s, a0) && one(s + 1, f.second, a1);
}

// the sample columns of record i: where they stand in the text, or the line bcf_lines would have made of the record's vectors.  Of a
// resident file they are copied down: the columns of a text line, the bytes of a BCF record
Span Run::sample_columns(const Input& in, const size_t i, const Fixed& F, std::string& line) {
    const char* t0 = (const char*)in.text.data();
    if (in.rf && !in.direct) {
        line.resize((size_t)F.s_len);
        if (rf_fetch(in.rf, F.s_off, F.s_len, (uint8_t*)&line[0]) != 0) stop_run("--resident 1: %s", rf_error(in.rf));
        return Span(line.data(), line.data() + line.size());
    }
    if (!in.vectors(i)) return Span(t0 + F.s_off, t0 + F.s_off + F.s_len);
    if (in.rf) {
        const BcfFields& f = in.brecs[i];
        std::vector<uint8_t> rec(f.rec_end - f.at);
        if (rf_fetch(in.rf, (int64_t)f.at, (int64_t)rec.size(), rec.data()) != 0) stop_run("--resident 1: %s", rf_error(in.rf));
        bcf_one_line(rec, in.dict, in.samples.size(), 0, line);
    }
    else bcf_one_line(in.bcf, in.dict, in.samples.size(), in.brecs[i].at, line);
    const char* col_at[10]; int nc;
    nine_columns(line.data(), line.data() + line.size(), col_at, nc);
    return nc < 9 ? Span(line.data() + line.size(), line.data() + line.size()) : Span(col_at[9], line.data() + line.size());
}

void Run::record_permissive(const Pair& p) {
    const Fixed& T = tf[p.ti]; const Fixed& C = cf[p.ci];
    const gtd::Rec& r = p.rec;
    const long long pos = (long long)r.pos;
    std::vector<Span> tc, cc;
    std::string t_line, c_line;                                    // (the line of a record that was judged from its vectors is written now)
    const Span ts = sample_columns(truth, p.ti, T, t_line), cs = sample_columns(call, p.ci, C, c_line);
    split_cols(ts.first, ts.second, tc); split_cols(cs.first, cs.second, cc);
    if (tc.size() != (size_t)N) stop_run("The truth record at position %lld has %zu sample columns, the header names %d samples.", pos, tc.size(), N);
    if (cc.size() != (size_t)N) stop_run("The call record at position %lld has %zu sample columns, the header names %d samples.", pos, cc.size(), N);
    std::vector<int> pl_gq;
    if (r.gq_mode == gtd::GQ_PL && r.c_nal > 1) {                 // the tool's loop over every sample before it looks at a genotype
        pl_gq.resize((size_t)N);
        for (int32_t s = 0; s < N; s++) {
            Span f;
            if (!nth_field(cc[s], r.c_pli, f)) stop_run("Sample %d at position %lld has no PL field.", s, pos);
            gtd::PlWalk w; int n = 0;
            for (const char* b = f.first;; n++) {
                const char* e = (const char*)memchr(b, ',', (size_t)(f.second - b)); if (!e) e = f.second;
                long v;
                if (e - b == 1 && *b == '.') w.add(-1);
                else if (!host_int(b, e, v)) stop_run("Sample %d at position %lld: PL value '%s' is not an integer.", s, pos, std::string(b, e).c_str());
                else if (v < 0) { if (v < w.second) w.second = (int)v; }      // (the tool takes it for the second best; GQ is then refused below)
                else w.add((int)v);
                if (e == f.second) { n++; break; }
                b = e + 1;
            }
            if (n != r.nG) stop_run("Sample %d at position %lld has %d PL values; %d alleles take %d.", s, pos, n, r.c_nal, r.nG);
            if (!w.zero) stop_run("Sample %d at position %lld: no PL value is 0 or missing (-doGQ 8 takes the lowest PL for 0).", s, pos);
            pl_gq[s] = w.gq();
        }
    }
    for (int32_t s = 0; s < N; s++) {
        Span tg, cg; long t0, t1, c0, c1;
        if (!nth_field(tc[s], r.t_gti, tg) || !host_gt(tg, t0, t1))
            stop_run("Sample %d at position %lld: the true genotype '%s' is not a diploid genotype.", s, pos, std::string(tc[s].first, tc[s].second).c_str());
        if (!nth_field(cc[s], r.c_gti, cg) || !host_gt(cg, c0, c1))
            stop_run("Sample %d at position %lld: the called genotype '%s' is not a diploid genotype.", s, pos, std::string(cc[s].first, cc[s].second).c_str());
        if (t0 < 0 || t1 < 0) stop_run("Sample %d at position %lld: the true genotype is missing.", s, pos);
        if (c0 < 0 || c1 < 0) { call_missing(s); continue; }
        auto base = [&](const Fixed& F, long a, const char* which) {
            const uint32_t b = a < (long)F.first.size() ? gtd::base_of((uint8_t)F.first[(size_t)a]) : 15u;
            if (b > 3u) stop_run("Sample %d at position %lld: allele %ld of the %s genotype is not an allele that starts with one of ACGTacgt0123.", s, pos, a, which);
            return b;
        };
        const uint32_t tb = base(T, t0, "true") | base(T, t1, "true") << 4;
        const uint32_t cb = base(C, c0, "called") | base(C, c1, "called") << 4;
        long gq = 0;
        if (r.gq_mode == gtd::GQ_MAX || (r.gq_mode == gtd::GQ_PL && r.c_nal == 1)) gq = gtd::MAX_GQ;
        else if (r.gq_mode == gtd::GQ_PL) gq = pl_gq[s];
        else if (r.gq_mode == gtd::GQ_TAG) {
            Span f;
            if (!nth_field(cc[s], r.c_gqi, f) || !host_int(f.first, f.second, gq)) gq = 0;
        }
        if (r.gq_mode != gtd::GQ_NONE && (gq < 1 || gq > gtd::MAX_GQ)) stop_run("Sample %d at position %lld: GQ is not a value in 1 .. 127.", s, pos);
        const uint32_t cell = gtd::classify(tb, cb);
        count(s, cell, (uint32_t)gq);
        lines(p, s, cell, (uint32_t)gq);
    }
}

// --on-device 0: the plain grammar by the routines the kernels run, a column at a time; the permissive reader for the rest
void Run::record_host(const Pair& p, std::vector<uint8_t>& planes) {
    uint8_t* tb = planes.data(); uint8_t* cb = tb + N; uint8_t* gq = cb + N;
    int st;
    if (!p.tside.have && !p.cside.have) st = gtd::record_plain(truth.text.data(), call.text.data(), p.rec, N, tb, cb, gq);
    else {                                                           // a side at a time: the column walk for text, the typed vectors for BCF
        st = p.tside.have ? gtd::bcf_side_plain(truth.bcf.data(), (int64_t)truth.bcf.size(), p.tside, false, p.rec.gq_mode, p.rec.nG, N, tb, cb, gq)
                          : gtd::side_plain(truth.text.data(), 0, p.rec, N, tb, cb, gq);
        if (st == gtd::ST_OK)
            st = p.cside.have ? gtd::bcf_side_plain(call.bcf.data(), (int64_t)call.bcf.size(), p.cside, true, p.rec.gq_mode, p.rec.nG, N, tb, cb, gq)
                              : gtd::side_plain(call.text.data(), 1, p.rec, N, tb, cb, gq);
    }
    if (st != gtd::ST_OK) { n_host++; record_permissive(p); return; }
    for (int32_t s = 0; s < N; s++) {
        if (cb[s] == gtd::CALL_MISSING) { call_missing(s); continue; }
        const uint32_t cell = gtd::classify(tb[s], cb[s]);
        count(s, cell, gq[s]);
        if (list || o.per_site) lines(p, s, cell, gq[s]);
    }
}

// the descriptor of record i of a file: its vectors where they are judged as they lie, have == 0 (text) otherwise
gtd::BSide bcf_side(const Input& in, const size_t i, const int32_t nal, const uint64_t map) {
    gtd::BSide b;
    memset(&b, 0, sizeof b);
    if (in.rf && in.direct && !in.vectors(i)) { b.have = gtd::B_GT; b.nal = nal; return b; }     // its line stands in the host's text alone: a side that never
    if (!in.vectors(i)) return b;                                                                // fits (type 0), so the record comes back for the host reader
    const BcfFields& f = in.brecs[i];
    b.gt_off = f.off[F_GT]; b.gt_type = f.type[F_GT]; b.gt_n = f.n[F_GT];
    if (f.have[F_GQ]) { b.gq_off = f.off[F_GQ]; b.gq_type = f.type[F_GQ]; b.gq_n = f.n[F_GQ]; b.have |= gtd::B_GQ; }
    if (f.have[F_PL]) { b.pl_off = f.off[F_PL]; b.pl_type = f.type[F_PL]; b.pl_n = f.n[F_PL]; b.have |= gtd::B_PL; }
    b.have |= gtd::B_GT; b.nal = nal; b.map = map;
    return b;
}

// ---- the tables of the tool's lines 629-833 ------------------------------------------------------------------------------------------
void write_tables(Run& R, const long nsites1, const long nsites2) {
    const int N = R.N, mode = R.o.do_gq;
    FILE* f = R.out_fp;
    enum { HH0, HH1, TT0, TT1, HT, TH };
    auto cell = [&](int s, int c, int k) -> long long { return k < gtd::N_GQ ? (long long)R.table[((size_t)s * gtd::N_CELLS + c) * gtd::N_GQ + k] : 0; };
    std::vector<long long> compared((size_t)N, 0);
    for (int s = 0; s < N; s++) for (int c = 0; c < gtd::N_CELLS; c++) for (int k = 0; k < gtd::N_GQ; k++) compared[s] += cell(s, c, k);
    if (mode == 0) {
        for (int s = 0; s < N; s++) {
            long long c[gtd::N_CELLS];
            for (int j = 0; j < gtd::N_CELLS; j++) { c[j] = 0; for (int k = 0; k < gtd::N_GQ; k++) c[j] += cell(s, j, k); }
            const long long cmp = compared[s], disc = c[HH1] + c[TT1] + c[HT] + c[TH], mis = (long long)R.table[(size_t)N * gtd::N_CELLS * gtd::N_GQ + s];
            const double n = (double)cmp;
            fprintf(f, "%s\t%ld\t%ld\t%lld\t%lld\t%lld\t%ld\t%lld\t%f\t%f\t%f\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%f\t%f\t%f\t%f\t%f\t%f\n",
                    R.truth.samples[s].c_str(), nsites1, nsites2, cmp, mis, disc, nsites1 - nsites2, cmp - disc,
                    (double)(1.0 - ((double)cmp / (double)nsites1)), (double)disc / n, (double)(cmp - disc) / n,
                    c[HH0], c[TT0], c[HH1], c[HT], c[TH], c[TT1],
                    (double)c[HH0] / n, (double)c[TT0] / n, (double)c[HH1] / n, (double)c[HT] / n, (double)c[TH] / n, (double)c[TT1] / n);
        }
        return;
    }
    // the eight counts of a -doGQ 4 row: discordant (all, hom->hom, hom->het, het->hom, het->het), concordant (all, hom->hom, het->het)
    auto row = [&](int s0, int s1, int k, long long r[8]) {
        for (int j = 0; j < 8; j++) r[j] = 0;
        for (int s = s0; s < s1; s++) {
            r[1] += cell(s, HH1, k); r[2] += cell(s, HT, k); r[3] += cell(s, TH, k); r[4] += cell(s, TT1, k);
            r[6] += cell(s, HH0, k); r[7] += cell(s, TT0, k);
        }
        r[0] = r[1] + r[2] + r[3] + r[4]; r[5] = r[6] + r[7];
    };
    long long r[8];
    if (mode == 3 || mode == 4) {
        for (int k = 1; k < 130; k++) {
            row(0, N, k, r);
            if (mode == 3) fprintf(f, "%d\t%lld\t%lld\n", k, r[0], r[5]);
            else fprintf(f, "%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", k, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
        }
    } else if (mode >= 5) {
        for (int s = 0; s < N; s++) for (int k = 1; k < 130; k++) {
            row(s, s + 1, k, r);
            if (mode == 5) fprintf(f, "%d\t%d\t%lld\t%lld\t%lld\n", s, k, r[0], r[5], compared[s]);
            else fprintf(f, "%d\t%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", s, k, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], compared[s]);
        }
    }
}

// ---- --on-device 1 ---------------------------------------------------------------------------------------------------------------
void run_device(Run& R) {
    const size_t K = R.pairs.size();
    const int32_t N = R.N;
    // a batch's listing is bounded by LINE_BOUND bytes a call: no more records than 64 MiB of it (one at least)
    int64_t B = R.o.batch;
    const int64_t per_rec = (int64_t)N * ((R.list || R.o.per_site) ? gtd::LINE_BOUND : 3);
    B = std::max<int64_t>(1, std::min<int64_t>(B, (64ll << 20) / std::max<int64_t>(per_rec, 1)));
    // --bcf-direct 1: a BCF side sends the vectors its record needs -- GT, GQ under GQ_TAG, PL under GQ_PL with more than one allele --
    // each at a 16-byte boundary of the staging (so at a 4-byte one), where a lane can take several samples with one load
    const bool direct = R.truth.direct || R.call.direct;
    // --resident 1: a resident side is read where the inflater wrote it, costs a batch nothing and its offsets count from the file
    const bool resident = R.truth.rf || R.call.rf;
    auto up16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
    auto vec_bytes = [&](int type, int32_t n) { return (int64_t)gtd::bcf_width(type) * n * N; };
    auto needs = [](const gtd::BSide& b, const gtd::Rec& r, bool call, bool& gq, bool& pl) {
        gq = call && r.gq_mode == gtd::GQ_TAG && (b.have & gtd::B_GQ); pl = call && r.gq_mode == gtd::GQ_PL && r.c_nal > 1 && (b.have & gtd::B_PL);
    };
    auto side_cost = [&](const Pair& p, bool call) -> int64_t {
        const gtd::BSide& b = call ? p.cside : p.tside;
        if ((call ? R.call : R.truth).rf) return 0;
        if (!b.have) return call ? p.rec.c_len : p.rec.t_len;
        bool gq, pl; needs(b, p.rec, call, gq, pl);
        return 16 + up16(vec_bytes(b.gt_type, b.gt_n)) + (gq ? 16 + up16(vec_bytes(b.gq_type, b.gq_n)) : 0) + (pl ? 16 + up16(vec_bytes(b.pl_type, b.pl_n)) : 0);
    };
    const BatchPlan plan = plan_batches(K, B, {BATCH_NO_CAP}, [&](size_t j, size_t) { return side_cost(R.pairs[j], false) + side_cost(R.pairs[j], true); });
    const std::vector<std::pair<size_t, size_t>>& batches = plan.ranges;     // blocks of B records: the text has no cap of its own
    const int64_t nb = (int64_t)batches.size();
    const int64_t max_text = std::max<int64_t>(1, plan.max_cost[0]);
    char err[256];
    R.dev = gtd_dev_create(R.o.device, N, (int32_t)std::min<int64_t>(B, std::max<size_t>(K, 1)), max_text, R.list, R.o.per_site, direct ? 1 : 0, resident ? 1 : 0, err, sizeof err);
    if (!R.dev) R.stop_run("--on-device 1: %s (device %d; --on-device 0 compares on the host)", err, R.o.device);
    auto submit = [&](int64_t b) {
        const double t0 = now_s();
        const int slot = (int)(b & 1);
        uint8_t* text = gtd_dev_text(R.dev, slot); gtd::Rec* recs = gtd_dev_recs(R.dev, slot);
        gtd::BSide* sides = direct ? gtd_dev_sides(R.dev, slot) : nullptr;
        int64_t at = 0, vec = 0, txt = 0; int32_t n = 0;
        auto vector_up = [&](const Input& in, int64_t& off, int type, int32_t n_val) {
            const int64_t bytes = vec_bytes(type, n_val);
            at = up16(at);
            memcpy(text + at, in.bcf.data() + off, (size_t)bytes); off = at; at += bytes; vec += bytes;
        };
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            const Pair& p = R.pairs[j];
            gtd::Rec r = p.rec;
            gtd::BSide ts = p.tside, cs = p.cside; bool gq, pl;
            if (R.truth.rf) {}
            else if (ts.have) vector_up(R.truth, ts.gt_off, ts.gt_type, ts.gt_n);
            else { memcpy(text + at, R.truth.text.data() + p.rec.t_off, (size_t)r.t_len); r.t_off = at; at += r.t_len; txt += r.t_len; }
            if (R.call.rf) {
                if (cs.have) { needs(cs, r, true, gq, pl); if (!gq) cs.have &= ~(uint32_t)gtd::B_GQ; if (!pl) cs.have &= ~(uint32_t)gtd::B_PL; }      // (as a staged side says it)
            } else if (cs.have) {
                needs(cs, r, true, gq, pl);
                vector_up(R.call, cs.gt_off, cs.gt_type, cs.gt_n);
                if (gq) vector_up(R.call, cs.gq_off, cs.gq_type, cs.gq_n); else cs.have &= ~(uint32_t)gtd::B_GQ;      // (not staged: not to be read)
                if (pl) vector_up(R.call, cs.pl_off, cs.pl_type, cs.pl_n); else cs.have &= ~(uint32_t)gtd::B_PL;
            } else { memcpy(text + at, R.call.text.data() + p.rec.c_off, (size_t)r.c_len); r.c_off = at; at += r.c_len; txt += r.c_len; }
            recs[n] = r;
            if (direct) { sides[2 * n] = ts; sides[2 * n + 1] = cs; }
        }
        const int rc = !resident ? gtd_dev_submit(R.dev, slot, n, at)
                                 : gtd_dev_submit_resident(R.dev, slot, n, at, R.truth.rf ? rf_device_text(R.truth.rf) : nullptr, R.truth.rf ? rf_total(R.truth.rf) : 0,
                                                           R.call.rf ? rf_device_text(R.call.rf) : nullptr, R.call.rf ? rf_total(R.call.rf) : 0);
        if (rc != 0) R.stop_run("--on-device 1: %s", gtd_dev_error(R.dev));
        R.text_up += txt; R.vec_up += vec;                                    // (the padding in front of a vector is neither)
         R.n_batches += direct; R.n_timed += n > 0; R.t_dev += now_s() - t0;
    };
    auto retire = [&](int64_t b) {
        double t0 = now_s();
        GtdBatchOut out;
        if (gtd_dev_wait(R.dev, (int)(b & 1), &out) != 0) R.stop_run("--on-device 1: %s", gtd_dev_error(R.dev));
        R.t_dev += now_s() - t0; t0 = now_s();
        int32_t n = 0;
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            if (out.status[n] != gtd::ST_OK) { R.n_host++; R.record_permissive(R.pairs[j]); continue; }
            if (R.list) R.list_buf.append((const char*)out.list_text + out.list_off[n], (size_t)(out.list_off[n + 1] - out.list_off[n]));
            if (R.o.per_site) R.site_buf.append((const char*)out.site_text + out.site_off[n], (size_t)(out.site_off[n + 1] - out.site_off[n]));
            R.flush(false);
        }
        R.t_host += now_s() - t0;
    };
    two_in_flight(nb, submit, retire);
    std::vector<int64_t> dt(R.table.size());
    if (gtd_dev_table(R.dev, dt.data()) != 0) R.stop_run("--on-device 1: %s", gtd_dev_error(R.dev));
    for (size_t i = 0; i + 2 < dt.size(); i++) R.table[i] += dt[i];
    if (direct || resident) gtd_dev_times(R.dev, &R.ms_stage, &R.ms_decode);
}

}  // namespace

int main(int argc, char** argv) {
    Run R;
    R.o = parse_opt(argc, argv);
    const Opt& o = R.o;
    double t0 = now_s();
    {
        FileReader reader; reader.device_inflate = o.device_inflate; reader.device = o.device; reader.verbose = o.verbose;
        int64_t left = o.resident_max;                                 // the truth file first; the call file gets what is left
        if (o.resident) { read_input_resident(reader, o, o.truth, left, R.truth); read_input_resident(reader, o, o.call, left, R.call); }
        else { read_input_file(reader, o.truth, o.bcf_direct != 0, R.truth); read_input_file(reader, o.call, o.bcf_direct != 0, R.call); }
    }
    R.out_fp = fopen(o.out.c_str(), "w");
    if (!R.out_fp) die("Could not open output file %s for writing", o.out.c_str());
    R.t_read = now_s() - t0; t0 = now_s();
    if (R.truth.samples.empty()) die("The truth file %s names no sample.", o.truth.c_str());
    if (R.truth.samples.size() != R.call.samples.size())
        die("The truth file names %zu samples and the call file %zu: samples are assumed to appear in the same order and quantity in both files.", R.truth.samples.size(), R.call.samples.size());
    if (R.truth.samples.size() > (size_t)(INT32_MAX / gtd::LINE_BOUND)) die("Too many samples.");
    R.N = (int32_t)R.truth.samples.size();
    R.list = o.do_gq == 1 ? gtd::LIST_GQ : o.do_gq == 2 ? gtd::LIST_GQ_TYPE : gtd::LIST_NONE;
    const bool has_gq = R.call.has_format("GQ"), has_pl = R.call.has_format("PL");
    if (o.do_gq == 7 && !has_gq) die("-doGQ 7 needs a call file whose header declares the GQ tag.");
    if (o.do_gq == 8 && !has_gq && !has_pl) die("-doGQ 8 is only supported for genotype calling files with GQ or PL tags");
    R.table.assign((size_t)vgl_disc_table_len(R.N), 0);

    // the first nine columns, then the tool's merge on POS: nsites1 counts the truth records read so far
    const size_t nT = R.truth.lines.size(), nC = R.call.lines.size();
    R.tf.resize(nT); R.cf.resize(nC);
    for (size_t i = 0; i < nT; i++) R.tf[i] = parse_nine(R.truth, i, "truth");
    for (size_t i = 0; i < nC; i++) R.cf[i] = parse_nine(R.call, i, "call");
    size_t ti = 0; long nsites1 = 1; char msg[320];
    for (size_t ci = 0; ci < nC && R.stop.empty(); ci++) {
        const Fixed& C = R.cf[ci];
        if (!C.bad.empty()) { R.stop = C.bad; break; }
        while (ti < nT && R.tf[ti].bad.empty() && C.pos > R.tf[ti].pos) { ti++; nsites1++; }
        if (ti < nT && !R.tf[ti].bad.empty()) { R.stop = R.tf[ti].bad; break; }
        if (ti >= nT || C.pos != R.tf[ti].pos) {
            snprintf(msg, sizeof msg, "The call file has a record at position %lld and the truth file has none: the truth file must hold every site of the call file.", (long long)C.pos);
            R.stop = msg; break;
        }
        const Fixed& T = R.tf[ti];
        Pair p; p.ci = ci; p.ti = ti; p.nsites1 = (int32_t)nsites1;
        gtd::Rec& r = p.rec;
        memset(&r, 0, sizeof r);
        r.t_off = T.s_off; r.t_len = (int32_t)T.s_len; r.c_off = C.s_off; r.c_len = (int32_t)C.s_len;
        r.t_map = T.map(); r.c_map = C.map(); r.pos = C.pos; r.nsites1 = p.nsites1;
        r.t_nal = (int32_t)T.first.size(); r.c_nal = (int32_t)C.first.size();
        r.t_gti = T.gti; r.c_gti = C.gti; r.c_gqi = C.gqi; r.c_pli = C.pli;
        r.nG = gtd::n_genotypes(r.c_nal);
        if (o.do_gq == 0) r.gq_mode = gtd::GQ_NONE;
        else if (o.do_gq <= 6) {
            r.gq_mode = gtd::GQ_TAG;
            if (C.gqi < 0) { snprintf(msg, sizeof msg, "The call record at position %lld has no GQ tag (-doGQ %d reads it; -doGQ 7 assumes the highest GQ there).", (long long)C.pos, o.do_gq); R.stop = msg; break; }
        } else if (o.do_gq == 7 || has_gq) r.gq_mode = C.gqi >= 0 ? gtd::GQ_TAG : gtd::GQ_MAX;
        else {
            r.gq_mode = gtd::GQ_PL;
            if (C.pli < 0) { snprintf(msg, sizeof msg, "The call record at position %lld has no PL tag (-doGQ 8 on a call file without GQ reads it).", (long long)C.pos); R.stop = msg; break; }
            if (r.c_nal > 5) { snprintf(msg, sizeof msg, "The call record at position %lld has %d alleles: -doGQ 8 reads PL for at most 5.", (long long)C.pos, r.c_nal); R.stop = msg; break; }
        }
        p.tside = bcf_side(R.truth, ti, r.t_nal, r.t_map); p.cside = bcf_side(R.call, ci, r.c_nal, r.c_map);
        R.n_direct[0] += R.truth.vectors(ti); R.n_direct[1] += R.call.vectors(ci);      // (not a resident record whose line stands as text: its side never fits)
        R.pairs.push_back(p);
    }
    const long nsites2 = (long)R.pairs.size();
    if (R.stop.empty() && nT > 0) nsites1 += (long)(nT - 1 - ti);
    R.t_nine = now_s() - t0;

    if (o.on_device) run_device(R);
    else {
        t0 = now_s();
        std::vector<uint8_t> planes(3 * (size_t)R.N);
        for (const Pair& p : R.pairs) { R.record_host(p, planes); R.flush(false); }
        R.t_host = now_s() - t0;
    }
    if (!R.stop.empty()) R.stop_run("%s", R.stop.c_str());
    R.flush(true);

    fprintf(stderr, "Comparing the genotypes in the truth file %s and the call file %s\n", o.truth.c_str(), o.call.c_str());
    fprintf(stderr, "Number of sites in truth file: %ld\n", nsites1);
    fprintf(stderr, "Number of sites in the truth file not in the call file: %ld\n", nsites1 - nsites2);
    fprintf(stderr, "Number of sites used in comparison: %ld\n", nsites2);
    if (R.list == gtd::LIST_NONE) write_tables(R, nsites1, nsites2);
    if (o.verbose)
        fprintf(stderr, "[gtdisc] on-device %d: records %ld, redone on the host %ld, text bytes sent up %lld; read %.3f s, nine columns and merge %.3f s, device %.3f s, host %.3f s\n",
                o.on_device, nsites2, R.n_host, (long long)R.text_up, R.t_read, R.t_nine, R.t_dev, R.t_host);
    if (o.verbose && o.bcf_direct)
        fprintf(stderr, "[bcf] bcf-direct 1: records judged from their vectors: truth %ld, call %ld; redone on the host %ld; vector bytes sent up %lld, text bytes sent up %lld; "
                        "device stage %.3f ms over %ld batches (hipEvent pairs), of which k_gtd_bcf_decode %.3f ms\n",
                R.n_direct[0], R.n_direct[1], R.n_host, (long long)R.vec_up, (long long)R.text_up, R.ms_stage, R.n_batches, R.ms_decode);
    if (o.verbose && o.resident)
        fprintf(stderr, "[resident] truth %d, call %d: device stage %.3f ms over %ld batches (hipEvent pairs), of which %s %.3f ms\n",
                R.truth.rf ? 1 : 0, R.call.rf ? 1 : 0, R.ms_stage, R.n_timed, (R.truth.direct || R.call.direct) ? "k_gtd_bcf_decode" : "k_gtd_parse", R.ms_decode);
    fprintf(stderr, "\n\nFinished running gtDiscordance\n\t-> Output file: %s\n", o.out.c_str());
    if (R.dev) gtd_dev_destroy(R.dev);
    if (R.truth.rf) rf_destroy(R.truth.rf);
    if (R.call.rf) rf_destroy(R.call.rf);
    fclose(R.out_fp);
    fflush(stdout);
    return 0;
}
