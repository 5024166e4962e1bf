// fetchgl_main.cpp -- fetchgl_hip: the reference's misc/fetchGl (one genotype's FORMAT/GL of every sample, as CSV) for this platform.
//   fetchgl_hip -i file -gt XY [-o out.csv] [--on-device 0|1] [--device INT] [--batch-records INT] [--messages 0|1] [--verbose 0|1]
//               [--device-inflate 0|1] [--resident 0|1] [--resident-max-bytes INT] [--resident-bcf 0|1]
// The file is read whole (plain, gzip or bgzip text through zlib, or BCF inside either; --device-inflate 1: BGZF members on the GPU,
// record_file.h).  --resident 1 (with --device-inflate 1 and --on-device 1): a BGZF file of VCF text is inflated into device memory
// and stays there (resident_file.h) -- the device finds the lines, only their heads (the first nine columns) come down for the notes
// below, and the batches' descriptors point into the resident text; a record the device hands back has its sample columns copied
// down for the strtod reader.  Whatever keeps the file from being resident (not BGZF, a member left to the host, BCF, too large, a
// line whose ninth tab is too far, too many lines) is named in the [input] line, and the run goes on as with --resident 0.
// --resident-bcf 1 (with --resident 1) does the same for a BGZF file of BCF: the device follows the records' lengths and walks their
// FORMAT fields (rb_core.h), the head of each record (its lengths, its shared block, the fields' keys and descriptors) comes down for
// the notes, and the batches' descriptors point at the GL vectors where the inflater wrote them.  A record the walk is not sure of
// hands the whole file back to the host reader, and the [input] line says which record and why.
// The host finds the records, reads the first nine columns of each (for BCF: the shared block and the FORMAT field headers), finds GL
// and the genotype's index g, and keeps a small note per record.  The records that get a CSV line are then read by the rules of fgl_core.h -- on the device in batches
// (--on-device 1: fetchgl.hip) or by the same routines on the host (--on-device 0) -- and a record those rules hand back (a token
// outside the device grammar, a value index outside the record's values, a wrong column count) is redone whole by the strtod reader
// below, which owns every message.  Both paths therefore write the same bytes.  A run that has to stop does so at the record where the
// host path stops: the lines and messages of the records before it are written first.
#include "record_file.h"
#include "batch_plan.h"
#include "fgl_dev.h"
#include "resident_file.h"

namespace {

struct Opt {
    std::string in, gt, out;
    int on_device = 1, device = 0, batch = 4096, messages = 1, verbose = 0;
    int device_inflate = 0, resident = 0, resident_bcf = 0;
    int64_t resident_max = -1;         // --resident-max-bytes (-1: the device's free memory less 1 GiB)
};

const char FGL_USAGE[] =
    "Usage: fetchgl_hip -i <input vcf> -gt <genotype to fetch>\n"
    "Example: fetchgl_hip -i input.vcf -gt AA\n"
    "Options:\n"
    "  -i, --input <file>        record file (VCF text, gzip / bgzip'd, or BCF)\n"
    "  -gt, --genotype XY        the genotype: two characters, each the first character of an allele's name\n"
    "  -o <file>                 the CSV goes to <file> [stdout]\n"
    "  --on-device 0|1 [1]       1: the sample columns are parsed and the CSV lines formatted on the GPU; 0: on the host, no GPU touched\n"
    "  --device INT [0]          the GPU\n"
    "  --batch-records INT [4096] records per device batch (and no more than 64 MiB of text in one)\n"
    "  --messages 0|1 [1]        the tool's per-record lines on stderr\n"
    "  --verbose 0|1 [0]         record counts, bytes sent up and received, stage times\n"
    "  --device-inflate 0|1 [0]  " DEVICE_INFLATE_HELP "\n"
    "  --resident 0|1 [0]        1: a BGZF file of VCF text stays in GPU memory once inflated: the GPU finds the lines, their first nine\n"
    "                            columns alone come down, the sample columns are parsed where they lie (needs --device-inflate 1 and\n"
    "                            --on-device 1; any other file is read as with 0, the reason is in the [input] line of --verbose 1)\n"
    "  --resident-max-bytes INT  the most bytes, inflated and compressed together, a resident file may take [the GPU's free memory less 1 GiB]\n"
    "  --resident-bcf 0|1 [0]    1: a BGZF file of BCF stays in GPU memory too: the GPU follows the records and walks their FORMAT fields, the\n"
    "                            shared blocks and field headers alone come down, the GL vectors are read where they lie (needs --resident 1;\n"
    "                            a file the walk is not sure of is read as with 0, the record and the reason are in the [input] line)\n"
    "  -h, --help                print help\n\n";

Opt parse_opt(int argc, char** argv) {
    Opt o;
    if (argc <= 1) { fputs(FGL_USAGE, stderr); exit(0); }
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) { fputs(FGL_USAGE, stderr); exit(0); }
        if (i + 1 >= argc) die("Missing value for arg:%s", a);
        const char* v = argv[++i];
        if (!strcmp(a, "-i") || !strcmp(a, "--input")) o.in = v;
        else if (!strcmp(a, "-gt") || !strcmp(a, "--genotype")) o.gt = v;
        else if (!strcmp(a, "-o")) o.out = v;
        else if (!strcmp(a, "--on-device")) o.on_device = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device")) o.device = option_int(a, v, 0, 1 << 20);
        else if (!strcmp(a, "--batch-records")) o.batch = option_int(a, v, 1, 1 << 24);
        else if (!strcmp(a, "--messages")) o.messages = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--verbose")) o.verbose = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device-inflate")) o.device_inflate = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident")) o.resident = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident-bcf")) o.resident_bcf = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident-max-bytes")) {
            char* e; const long long x = strtoll(v, &e, 10);
            if (e == v || *e || x < 0) die("%s takes an integer of at least 0, not '%s'", a, v);
            o.resident_max = x;
        }
        else die("Unknown arg:%s", a);
    }
    if (o.in.empty()) die("Input file not specified. Exiting...");
    if (o.gt.empty()) die("Genotype to fetch not specified. Exiting...");
    if (o.gt.size() != 2) die("A genotype is exactly two characters, not '%s'.", o.gt.c_str());
    if (o.resident && !(o.device_inflate && o.on_device)) die("--resident 1 needs --device-inflate 1 and --on-device 1.");
    if (o.resident_bcf && !o.resident) die("--resident-bcf 1 needs --resident 1 (and with it --device-inflate 1 and --on-device 1).");
    return o;
}

// what the host keeps of a record: where its sample columns (BCF: its GL vectors) lie, GL's place, the two alleles
struct Note {
    int64_t pos = 0, off = 0;             // off: into raw, or (a resident file) into the file
    int32_t len = 0;                   // text: bytes of the sample columns; BCF: the vector length
    int32_t k = 0;
    int16_t a0 = -1, a1 = -1;
    bool halt = false;                 // the run stops at this record, behind its message
    bool found() const { return a0 >= 0 && a1 >= 0; }
    bool line() const { return found() && !halt; }
    int32_t g() const { return fgl::genotype_of(a0, a1); }
};

struct Run {
    Opt o;
    std::vector<uint8_t> raw;          // the file's bytes, inflated
    bool bcf = false;
    std::vector<std::string> header, samples;
    std::vector<Note> notes;           // the records in file order, up to the one the run stops at
    std::string stop;                  // why the run ends behind the last note (empty: it does not)
    int64_t N = 0;
    FILE* out_fp = nullptr;
    std::string csv_buf, msg_buf;
    FglDev* dev = nullptr;
    RfFile* rf = nullptr;              // --resident 1: the file's text in device memory (raw is then the head stream)
    rf::Split split;
    std::vector<uint8_t> bcf_head;     // --resident-bcf 1: the header of a resident BCF file (raw is then the records' head stream)
    RbSplit bsplit;
    long n_lines = 0, n_host = 0; int64_t up = 0, down = 0;
    double t_read = 0, t_nine = 0, t_dev = 0, t_host = 0;

    void flush(bool all) {
        if (all || csv_buf.size() > (1u << 22)) { if (!csv_buf.empty()) fwrite(csv_buf.data(), 1, csv_buf.size(), out_fp); csv_buf.clear(); }
        if (all || msg_buf.size() > (1u << 20)) { if (!msg_buf.empty()) fwrite(msg_buf.data(), 1, msg_buf.size(), stderr); msg_buf.clear(); }
    }
    // the run ends here: what the records so far gave is written, nothing stays in flight on the device
    [[noreturn]] void stop_run(const char* fmt, ...) {
        if (dev) fgl_dev_quiesce(dev);
        flush(true); fflush(out_fp);
        va_list ap; va_start(ap, fmt); die_v(fmt, ap);
    }
    // the tool's line on stderr for a record
    void message(const Note& n) {
        if (!o.messages) return;
        char b[256];
        if (!n.found()) snprintf(b, sizeof b, "Requested genotype %s not found at position %lld. Skipping...\n", o.gt.c_str(), (long long)n.pos);
        else snprintf(b, sizeof b, "Requested genotype's first allele corresponds to allele %d and second allele corresponds to allele %d at position %lld.\n",
                      (int)n.a0, (int)n.a1, (long long)n.pos);
        msg_buf += b;
    }
    void put_line(const Note& n, const uint32_t* plane) {
        uint8_t b[fgl::VALUE_BOUND];
        { vgl_fetchgl::Emit<true> e{b, 0u, (uint32_t)sizeof b}; fgl::put_pos(e, (uint64_t)n.pos); csv_buf.append((const char*)b, e.n); }
        for (int64_t s = 0; s < N; s++) { vgl_fetchgl::Emit<true> e{b, 0u, (uint32_t)sizeof b}; fgl::put_value(e, plane[s], s == N - 1); csv_buf.append((const char*)b, e.n); }
        n_lines++;
    }
    void record_strtod(const Note& n, const char* t, std::vector<uint32_t>& plane);
    // a record for the strtod reader: its sample columns where the host holds them, or copied down from the resident text
    void record_redo(const Note& n, std::vector<uint32_t>& plane) {
        if (!rf) { record_strtod(n, (const char*)raw.data() + n.off, plane); return; }
        if (bcf) {                                                     // a resident BCF record the device handed back: its GL block, by the host's rule
            std::vector<uint8_t> block((size_t)N * (size_t)n.len * 4);
            if (rf_fetch(rf, n.off, (int64_t)block.size(), block.data()) != 0) stop_run("--resident-bcf 1: %s", rf_error(rf));
            pick_bcf(n, block.data(), plane);
            return;
        }
        std::vector<uint8_t> cols((size_t)n.len + 1);
        if (rf_fetch(rf, n.off, n.len, cols.data()) != 0) stop_run("--resident 1: %s", rf_error(rf));
        record_strtod(n, (const char*)cols.data(), plane);
    }
    void pick_bcf(const Note& n, const uint8_t* v, std::vector<uint32_t>& plane) {
        for (int64_t s = 0; s < N; s++) memcpy(&plane[s], v + ((size_t)s * n.len + n.g()) * 4, 4);
        put_line(n, plane.data());
    }
    bool load_resident(FileReader& reader);
    const char* load_resident_bcf(std::string& why);
    void record_host(const Note& n, std::vector<uint32_t>& plane);
    void notes_text();
    void notes_bcf();
};

// ---- the strtod reader: one record of VCF text by the tool's own reading of its values, with the run's messages ---------------------
void Run::record_strtod(const Note& n, const char* const t, std::vector<uint32_t>& plane) {
    const char* const end = t + n.len;
    const long long pos = (long long)n.pos;
    const int32_t g = n.g();
    std::vector<std::pair<const char*, const char*>> field;            // the GL field of every column (empty pair: one missing value)
    for (const char* p = t;;) {
        const char* ce = (const char*)memchr(p, '\t', (size_t)(end - p)); if (!ce) ce = end;
        const char* b = p;
        for (int f = 0; f < n.k && b; f++) { b = (const char*)memchr(b, ':', (size_t)(ce - b)); if (b) b++; }
        if (!b) field.emplace_back(nullptr, nullptr);
        else { const char* e = (const char*)memchr(b, ':', (size_t)(ce - b)); field.emplace_back(b, e ? e : ce); }
        if (ce == end) break;
        p = ce + 1;
    }
    if ((int64_t)field.size() != N) stop_run("The record at position %lld has %zu sample columns, the header names %lld samples.", pos, field.size(), (long long)N);
    int64_t n_gls = 0;
    for (const auto& f : field) { int64_t c = 1; for (const char* q = f.first; q && q < f.second; q++) c += *q == ','; n_gls = std::max(n_gls, c); }
    if (g >= n_gls)
        stop_run("The genotype %s is value %d of FORMAT/GL at position %lld, and the record's samples carry at most %lld values (the tool reads outside its buffer there).",
                 o.gt.c_str(), g, pos, (long long)n_gls);
    for (int64_t s = 0; s < N; s++) {
        const char* b = field[s].first; const char* const fe = field[s].second;
        if (!b) { plane[s] = g == 0 ? fgl::MISSING_BITS : fgl::END_BITS; continue; }
        int32_t i = 0;
        const char* e = nullptr;
        for (;; i++) {
            e = (const char*)memchr(b, ',', (size_t)(fe - b)); if (!e) e = fe;
            if (i == g || e == fe) break;
            b = e + 1;
        }
        if (i < g) { plane[s] = fgl::END_BITS; continue; }
        const std::string tok(b, e);
        if (tok == ".") { plane[s] = fgl::MISSING_BITS; continue; }
        char* te = nullptr;
        const double d = strtod(tok.c_str(), &te);
        if (tok.empty() || te != tok.c_str() + tok.size())
            stop_run("Sample %lld at position %lld: the GL value '%s' is not a number.", (long long)s, pos, tok.c_str());
        const float f = (float)d;
        memcpy(&plane[s], &f, 4);
    }
    put_line(n, plane.data());
}

// --on-device 0: the routines the kernels run, a column at a time; the strtod reader for what they hand back
void Run::record_host(const Note& n, std::vector<uint32_t>& plane) {
    if (bcf) { pick_bcf(n, raw.data() + n.off, plane); return; }
    fgl::Rec r; memset(&r, 0, sizeof r);
    r.off = n.off; r.len = n.len; r.k = n.k; r.g = n.g(); r.pos = n.pos;
    const int st = fgl::record_plain(raw.data(), r, N, plane.data(), nullptr);
    if (st == fgl::ST_OK) { put_line(n, plane.data()); return; }
    if (st == fgl::ST_HOST) n_host++;
    record_redo(n, plane);
    if (st == fgl::ST_RANGE) stop_run("The record at position %lld was refused by the column rules and taken by the strtod reader.", (long long)n.pos);
}

// ---- the notes: the first nine columns of every record line ---------------------------------------------------------------------------
bool header_defines_gl(const std::vector<std::string>& header, std::string* type) {
    for (const std::string& h : header) if (h.compare(0, 10, "##FORMAT=<") == 0 && BcfIn::attr(h, "ID") == "GL") { if (type) *type = BcfIn::attr(h, "Type"); return true; }
    return false;
}

void match_alleles(const Opt& o, const char first, const int j, Note& n) {
    if (first == o.gt[0]) n.a0 = (int16_t)j;
    if (first == o.gt[1]) n.a1 = (int16_t)j;
}

void Run::notes_text() {
    const char* const t0 = (const char*)raw.data();
    TextLines tl = scan_text(raw);
    header = std::move(tl.header); samples = std::move(tl.samples);
    const std::vector<std::pair<int64_t, int64_t>>& lines = tl.lines;
    N = (int64_t)samples.size();
    const bool defined = header_defines_gl(header, nullptr);
    char msg[256];
    notes.reserve(lines.size());
    size_t ln = 0;                                                     // --resident 1: raw is the head stream, and record i is line ln of the file
    for (size_t i = 0; i < lines.size(); i++) {
        if (rf) while (split.hoff[ln] < lines[i].first) ln++;
        const char* lb = t0 + lines[i].first; const char* le = t0 + lines[i].second;
        const char* col_at[10]; int nc;
        nine_columns(lb, le, col_at, nc);
        Note n;
        n.pos = pos_column(col_at, nc);
        if (nc < 9) { snprintf(msg, sizeof msg, "Record %zu has fewer than 10 columns (a FORMAT/GL column is required).", i + 1); stop = msg; return; }
        // GL must be readable before anything else
        n.k = format_key_index(col_at[8], col_at[9] - 1, "GL");
        if (!defined || n.k < 0) { snprintf(msg, sizeof msg, "Could not read GL tag at position %lld. Exiting...", (long long)n.pos); stop = msg; return; }
        const char* const ref = col_at[3]; const char* const alt = col_at[4]; const char* const alt_end = col_at[5] - 1;
        int j = 0;
        match_alleles(o, ref < col_at[4] - 1 ? ref[0] : '\0', j++, n);
        if (!(alt_end - alt == 1 && alt[0] == '.'))
            for (const char* b = alt;; ) {
                const char* e = (const char*)memchr(b, ',', (size_t)(alt_end - b)); if (!e) e = alt_end;
                if (j < INT16_MAX) match_alleles(o, e > b ? b[0] : '\0', j, n);
                j++;
                if (e == alt_end) break;
                b = e + 1;
            }
        n.off = rf ? split.s_off[ln] : col_at[9] - t0;
        const int64_t len = rf ? split.s_len[ln] : le - col_at[9];
        if (len > INT32_MAX) { snprintf(msg, sizeof msg, "The record at position %lld is longer than 2 GiB.", (long long)n.pos); stop = msg; return; }
        n.len = (int32_t)len;
        notes.push_back(n);
    }
}

// --resident 1: the file into device memory and its split (resident_file.h).  true: the file is resident and raw is its head stream;
// false: raw holds the file's bytes as --resident 0 reads them, and the [input] line says why
bool Run::load_resident(FileReader& reader) {
    char err[256];
    { FILE* fp = fopen(o.in.c_str(), "rb"); if (!fp) die("Could not open file: %s", o.in.c_str()); fclose(fp); }   // the file first, as without the flag
    rf = rf_create(o.device, err, sizeof err);
    if (!rf) die("--resident 1: %s (device %d)", err, o.device);
    const int64_t most = o.resident_max >= 0 ? o.resident_max : rf_default_max_bytes(rf);
    auto failed = [&]() { const std::string why = rf_error(rf); if (why.compare(0, 14, "Could not open") == 0) die("%s", why.c_str()); die("--resident 1: %s", why.c_str()); };
    RfWhy why;
    if (rf_load(rf, o.in.c_str(), most, &why) != 0) failed();
    const char* reason = nullptr;
    bool have = false;                                                 // raw was copied down from the device
    bool is_bcf = false; std::string bcf_why;
    if (why == RF_NOT_BGZF) reason = "the file is not a series of BGZF members";
    else if (why == RF_MEMBER_HOST) reason = "a member was left to the host (VGL_INFLATE_HOST)";
    else if (why == RF_TOO_LARGE) reason = "the inflated and the compressed bytes exceed --resident-max-bytes";
    else {
        const int64_t total = rf_total(rf);
        uint8_t first[3] = {0, 0, 0};
        if (rf_fetch(rf, 0, std::min<int64_t>(3, total), first) != 0) failed();
        bool more_lines = false;
        if (total >= 3 && !memcmp(first, "BCF", 3) && o.resident_bcf) { is_bcf = true; reason = load_resident_bcf(bcf_why); }
        else if (total >= 3 && !memcmp(first, "BCF", 3)) reason = "the file is BCF";
        else {
            if (rf_split(rf, rf::RF_HEAD_MOST, &split, &more_lines) != 0) failed();
            if (more_lines) reason = "the file has more lines than the offsets scan takes (INT32_MAX - 1024)";
            else if (split.over) reason = "a line's ninth tab is not within RF_HEAD_MOST bytes";
        }
        if (reason) {                                                  // the inflated bytes are on the device: they come down whole
            raw.resize((size_t)total);
            if (rf_fetch(rf, 0, total, raw.data()) != 0) failed();
            have = true;
        }
    }
    const RfStats st = *rf_stats(rf);
    if (o.resident_bcf && reason && !have) {                           // nothing was inflated: zlib reads the first three bytes, so that the
        uint8_t first[3] = {0, 0, 0};                                  // [input] lines come in the order of --resident 1
        gzFile fp = gzopen(o.in.c_str(), "r");
        if (fp) { is_bcf = gzread(fp, first, 3) == 3 && !memcmp(first, "BCF", 3); gzclose(fp); }
    }
    if (o.verbose && is_bcf)                                           // --resident-bcf 1: a BCF file has a line of its own
        fprintf(stderr, "[input] %s: resident-bcf %d%s%s%s, members %lld, records %lld, head bytes received %lld, compressed bytes sent up %lld; upload %.3f s, inflate %.3f s, chain %.3f s, heads %.3f s\n",
                o.in.c_str(), reason ? 0 : 1, reason ? " (" : "", reason ? reason : "", reason ? ")" : "", (long long)st.members, (long long)st.records,
                (long long)st.head_bytes, (long long)st.compressed_up, st.t_upload, st.t_inflate, st.t_chain, st.t_heads);
    else if (o.verbose)
        fprintf(stderr, "[input] %s: resident %d%s%s%s, RF_CHUNK %lld, members %lld, lines %lld, head bytes received %lld, compressed bytes sent up %lld; upload %.3f s, inflate %.3f s, split %.3f s\n",
                o.in.c_str(), reason ? 0 : 1, reason ? " (" : "", reason ? reason : "", reason ? ")" : "", (long long)rf::RF_CHUNK, (long long)st.members, (long long)st.lines,
                (long long)st.head_bytes, (long long)st.compressed_up, st.t_upload, st.t_inflate, st.t_split);
    if (o.verbose && have) FileReader::report(o.in, (long)st.members, st.compressed_up, st.total, st.t_inflate, nullptr);
    if (!reason) { raw = std::move(is_bcf ? bsplit.heads : split.heads); bcf = is_bcf; return true; }
    rf_destroy(rf); rf = nullptr; split = rf::Split(); bsplit = RbSplit(); bcf_head.clear();
    if (!have) raw = reader.read(o.in);
    return false;
}

// --resident-bcf 1, a resident file that begins as BCF: its header and the split of its records (resident_file.h).  nullptr: bcf_head
// and bsplit hold them; else why the bytes come down whole
const char* Run::load_resident_bcf(std::string& why) {
    auto failed = [&]() { die("--resident-bcf 1: %s", rf_error(rf)); };
    bool fits = false;
    if (rf_bcf_header(rf, &bcf_head, &fits) != 0) failed();
    if (!fits) { why = "the header does not fit the file"; return why.c_str(); }
    int64_t n_samples = -1;
    try { BcfDict d; Vcf v; BcfIn c; c.buf = bcf_head.data(); c.size = bcf_head.size(); c.soft = true; bcf_header(c, d, v); n_samples = (int64_t)v.samples.size(); }
    catch (const BcfSoftFail&) { why = "the header could not be read"; return why.c_str(); }
    if (rf_bcf_split(rf, (int64_t)bcf_head.size(), n_samples, rb::RB_HOPS_MOST, rf::RF_HEAD_MOST, &bsplit) != 0) failed();
    if (bsplit.more_records) why = "the file has more records than the offsets scan takes (INT32_MAX - 1024)";
    else if (bsplit.why != rb::OK) { char b[256]; snprintf(b, sizeof b, "record %lld: %s", (long long)bsplit.ordinal + 1, rb::why_text(bsplit.why)); why = b; }
    else return nullptr;
    return why.c_str();
}

// BCF: the shared block -> POS and the alleles; the FORMAT field headers -> where GL's vectors lie
// One body for both sources.  The file's bytes in raw: the cursor walks them.  A resident file (--resident-bcf 1): the header is
// bcf_head, raw is the head stream -- per record the two lengths, the shared block and the fields' keys and descriptors, bytes
// identical to the file's -- and a field's data offset is worked out from the record's place in the file (bcf_format_fields).
void Run::notes_bcf() {
    BcfDict d; BcfIn c; c.buf = rf ? bcf_head.data() : raw.data(); c.size = rf ? bcf_head.size() : raw.size();
    Vcf v;
    bcf_header(c, d, v);
    if (rf) { c.buf = raw.data(); c.size = raw.size(); c.off = 0; }
    header = v.header; samples = v.samples;
    N = (int64_t)samples.size();
    std::string type;
    const bool defined = header_defines_gl(header, &type) && type == "Float";
    char msg[256];
    for (size_t i = 0; c.off < c.size; i++) {
        BcfRecAt at; int n_fmt;
        const size_t head_at = c.off;
        if (!rf) bcf_scan_record(c, at);
        else {                                                         // (the device has made the checks of bcf_scan_record)
            if (i >= (size_t)bsplit.records || (int64_t)head_at != bsplit.hoff[i]) stop_run("--resident-bcf 1: the head stream does not follow its records.");
            const uint32_t l_shared = c.u32(); (void)c.u32();
            at.shared = c.off; at.shared_end = c.off + l_shared; at.rec_end = (size_t)bsplit.hoff[i + 1];
        }
        Rec r;
        bcf_shared(c, d, at, (size_t)N, r, n_fmt);
        Note n; n.pos = r.pos0 + 1; n.k = -1;
        bool is_float = false;
        bcf_format_fields(c, d, n_fmt, (size_t)N, [&](int k, const std::string& key, int ty, int nv, size_t data_off) {
            if (key == "GL" && n.k < 0) { n.k = k; is_float = ty == 5 && nv >= 1; n.off = (int64_t)data_off; n.len = nv; }
        }, rf ? bsplit.rec_off[i] + (int64_t)(c.off - head_at) : (int64_t)-1);
        if (rf && c.off != at.rec_end) stop_run("--resident-bcf 1: a record's head is not as long as the device made it.");
        c.off = at.rec_end;
        if (!defined || n.k < 0 || !is_float) { snprintf(msg, sizeof msg, "Could not read GL tag at position %lld. Exiting...", (long long)n.pos); stop = msg; return; }
        for (size_t j = 0; j < r.alleles.size() && j < (size_t)INT16_MAX; j++) match_alleles(o, r.alleles[j].empty() ? '\0' : r.alleles[j][0], (int)j, n);
        if (n.found() && n.g() >= n.len) {
            n.halt = true; notes.push_back(n);                          // (its message comes first, as on the text path)
            snprintf(msg, sizeof msg, "The genotype %s is value %d of FORMAT/GL at position %lld, and the record's samples carry at most %lld values (the tool reads outside its buffer there).",
                     o.gt.c_str(), n.g(), (long long)n.pos, (long long)n.len);
            stop = msg;
            return;
        }
        notes.push_back(n);
    }
}

// ---- --on-device 1 ---------------------------------------------------------------------------------------------------------------
void run_device(Run& R, std::vector<uint32_t>& plane) {
    const std::vector<Note>& notes = R.notes;
    std::vector<size_t> sent;
    for (size_t i = 0; i < notes.size(); i++) if (notes[i].line()) sent.push_back(i);
    // (--resident 1: the text is on the device already, a batch stages descriptors alone)
    auto bytes_of = [&](const Note& n) { return R.rf ? (int64_t)0 : R.bcf ? ((int64_t)R.N * n.len * 4) : (int64_t)n.len; };
    // a batch: at most --batch-records records, 64 MiB of CSV bound and 64 MiB of text (one record at least)
    const int64_t TEXT_MOST = 64ll << 20;
    const int64_t B = std::max<int64_t>(1, std::min<int64_t>(R.o.batch, TEXT_MOST / fgl_dev_line_bound((int32_t)R.N)));
    const BatchPlan plan = plan_batches(sent.size(), B, {TEXT_MOST}, [&](size_t j, size_t) { return bytes_of(notes[sent[j]]); });
    const std::vector<std::pair<size_t, size_t>>& batches = plan.ranges;     // [j0, j1) of sent
    const int64_t max_text = std::max<int64_t>(1, plan.max_cost[0]), max_recs = std::max<int64_t>(1, plan.max_recs);
    char err[256];
    R.dev = fgl_dev_create(R.o.device, (int32_t)R.N, (int32_t)max_recs, max_text, err, sizeof err);
    if (!R.dev) { R.notes.clear(); R.stop_run("--on-device 1: %s (device %d; --on-device 0 reads on the host)", err, R.o.device); }
    auto submit = [&](int64_t b) {
        const double t0 = now_s();
        const int slot = (int)(b & 1);
        uint8_t* text = fgl_dev_text(R.dev, slot); fgl::Rec* recs = fgl_dev_recs(R.dev, slot);
        int64_t at = 0; int32_t n = 0;
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            const Note& nt = notes[sent[j]];
            fgl::Rec r; memset(&r, 0, sizeof r);
            r.off = R.rf ? nt.off : at; r.len = nt.len; r.k = nt.k; r.g = nt.g(); r.pos = nt.pos;
            if (!R.rf) { memcpy(text + at, R.raw.data() + nt.off, (size_t)bytes_of(nt)); at += bytes_of(nt); }
            recs[n] = r;
        }
        const int rc = R.rf ? fgl_dev_submit_resident(R.dev, slot, n, rf_device_text(R.rf), rf_total(R.rf), R.bcf ? 1 : 0) : fgl_dev_submit(R.dev, slot, n, at, R.bcf ? 1 : 0);
        if (rc != 0) R.stop_run("--on-device 1: %s", fgl_dev_error(R.dev));
        R.up += at + (int64_t)n * (int64_t)sizeof(fgl::Rec); R.t_dev += now_s() - t0;
    };
    size_t cur = 0;                                                    // the next record in file order
    auto retire = [&](int64_t b) {
        double t0 = now_s();
        FglBatchOut out;
        if (fgl_dev_wait(R.dev, (int)(b & 1), &out) != 0) R.stop_run("--on-device 1: %s", fgl_dev_error(R.dev));
        R.t_dev += now_s() - t0; t0 = now_s();
        int32_t n = 0;
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            for (; cur < sent[j]; cur++) R.message(notes[cur]);
            const Note& nt = notes[cur++];
            R.message(nt);
            if (out.status[n] == fgl::ST_OK) { R.csv_buf.append((const char*)out.csv + out.off[n], (size_t)(out.off[n + 1] - out.off[n])); R.n_lines++; }
            else {
                if (out.status[n] == fgl::ST_HOST) R.n_host++;
                R.record_redo(nt, plane);
                if (out.status[n] == fgl::ST_RANGE) R.stop_run("The record at position %lld was refused by the column rules and taken by the strtod reader.", (long long)nt.pos);
            }
            R.flush(false);
        }
        R.down += out.off[n] + (int64_t)n * 12 + 8;
        R.t_host += now_s() - t0;
    };
    two_in_flight((int64_t)batches.size(), submit, retire);
    for (; cur < notes.size(); cur++) R.message(notes[cur]);
}

}  // namespace

int main(int argc, char** argv) {
    Run R;
    R.o = parse_opt(argc, argv);
    const Opt& o = R.o;
    double t0 = now_s();
    FileReader reader; reader.device_inflate = o.device_inflate; reader.device = o.device; reader.verbose = o.verbose;
    if (o.resident) R.load_resident(reader);
    else R.raw = reader.read(o.in);
    R.out_fp = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
    if (!R.out_fp) die("Could not open output file %s for writing", o.out.c_str());
    R.t_read = now_s() - t0; t0 = now_s();
    if (!R.rf) R.bcf = R.raw.size() >= 3 && !memcmp(R.raw.data(), "BCF", 3);
    if (R.bcf) R.notes_bcf(); else R.notes_text();
    if (R.N <= 0) die("The file %s names no sample.", o.in.c_str());
    if (R.N > (int64_t)(INT32_MAX / fgl::VALUE_BOUND)) die("Too many samples.");
    R.t_nine = now_s() - t0;

    std::vector<uint32_t> plane((size_t)R.N);
    if (o.on_device) run_device(R, plane);
    else {
        t0 = now_s();
        for (const Note& n : R.notes) { R.message(n); if (n.line()) R.record_host(n, plane); R.flush(false); }
        R.t_host = now_s() - t0;
    }
    if (!R.stop.empty()) R.stop_run("%s", R.stop.c_str());
    R.flush(true);
    if (o.verbose)
        fprintf(stderr, "[fetchgl] on-device %d: records %zu, with a CSV line %ld, redone on the host %ld, bytes sent up %lld, received %lld; read %.3f s, nine columns %.3f s, device %.3f s, host %.3f s\n",
                o.on_device, R.notes.size(), R.n_lines, R.n_host, (long long)R.up, (long long)R.down, R.t_read, R.t_nine, R.t_dev, R.t_host);
    if (R.dev) fgl_dev_destroy(R.dev);
    if (R.rf) rf_destroy(R.rf);
    if (R.out_fp != stdout) fclose(R.out_fp);
    fflush(stdout);
    return 0;
}
