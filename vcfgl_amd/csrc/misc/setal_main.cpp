// setal_main.cpp -- setalleles_hip: the reference's misc/setAlleles (a record file gets a new REF/ALT list per record from a TSV; INFO/QS
// and FORMAT GL / PL / GP follow the new allele order and are renormalised) for this platform, on a file that exists on disk.
//   setalleles_hip -i file -a alleles.tsv [-O b|u|z|v] [-o prefix] [--on-device 0|1] [--device INT] [--batch-records INT] [--threads INT] [--verbose 0|1]
//                  [--device-inflate 0|1] [--resident 0|1] [--resident-max-bytes INT]
// Both files are read whole (the record file through zlib: plain, gzip or bgzip text, or BCF inside either).  The TSV is checked first, then one pass reads the
// first nine columns of every record, matches its TSV line, builds oldgt2newgt and the new fixed columns (REF, ALT, INFO with QS
// permuted) and keeps a note per record; every stop of these two passes comes before the output file is opened.
// VCF text is worked on the host (--on-device 0; --on-device 1 is refused for it): the sample columns are read by the rules of
// sal_core.h, a column at a time, and a record those rules hand back (a token outside their grammar, a column count other than the
// header's, more values than the old genotype count, a PL sample whose cast would overflow) is redone whole by the strtod / strtol
// reader below, which owns every message.  The new sample columns are the copied bytes of the untouched fields and the new values in
// htslib's text.
// BCF input (raw or BGZF) is written as BCF (-O u, -O b): the shared block is rewritten (n_allele, the allele strings, QS resized, rlen),
// GL / GP become N x nG_new floats, PL is re-typed to the narrowest of int8 / int16 / int32 over the record's values (--on-device 1: k_sal_bcf_apply
// in batches, two in flight; --on-device 0: the same routines on the host, so both settings write the same bytes), the untouched fields are copied.  Text is written as text (-O v, -O z); a request across is refused.
// --resident 1 (with --device-inflate 1 and --on-device 1): a BGZF file of BCF is inflated into device memory and stays there
// (resident_file.h).  The device follows the records and hands down their heads for the notes below; k_sal_bcf_apply reads the vectors
// where the inflater wrote them; the output records are assembled on the device (setalres.hip, salres_core.h: the new shared blocks go
// up, the untouched fields are copied from the resident file, the new vectors from the batch's planes) and compressed there for -O b,
// so that BGZF members alone come down (-O u: the records).  The host path stays the specification: a file that cannot be resident
// is read as with --resident 0 (the [input] line of --verbose 1 says why), and a batch in which any record is not taken by the device
// is fetched record by record and worked by record_host_bcf in order, which owns every message.
#include "record_file.h"
#include "batch_plan.h"
#include "sal_dev.h"
#include "resident_file.h"
#include "salres_dev.h"

namespace {

struct Opt {
    std::string in, alleles, prefix, out_fn;
    char mode = 'b';
    int on_device = 1, device = 0, batch = 4096, threads = 1, verbose = 0, device_inflate = 0, resident = 0;
    int64_t resident_max = -1;         // --resident-max-bytes (-1: the device's free memory less 1 GiB)
};

const char SAL_VERSION[] = "0.0.1";
const char SAL_USAGE[] =
    "Usage: setalleles_hip -i <input> -a <alleles tsv> [options]\n"
    "    -h, --help                 print this help message and exit\n"
    "    -v, --version              print the version and exit\n"
    "Options:\n"
    "    -i, --input FILE           record file: VCF text (plain, gzip or bgzip) or BCF (raw or BGZF)\n"
    "    -a, --alleles FILE         alleles TSV: one REF<TAB>ALT[,ALT...] line per record, 1 to 4 ALTs\n"
    "    -O, --output-mode [b]|u|z|v  b: compressed BCF (.bcf), u: uncompressed BCF (.bcf), z: compressed VCF (.vcf.gz), v: VCF (.vcf);\n"
    "                               text input is written as v or z, BCF input as b or u\n"
    "    -o, --output STRING ['output']  output filename prefix\n"
    "    --on-device 0|1 [1]        1: the GL / PL / GP vectors of BCF input are reordered, normalised and narrowed on the GPU (VCF text: refused);\n"
    "                               0: on the host, no GPU touched\n"
    "    --device INT [0]           the GPU\n"
    "    --batch-records INT [4096] records per device batch (and no more than 64 MiB staged either way in one; a file kept in GPU memory:\n"
    "                               no more than 64 MiB of assembled records in one, a larger record is a batch of its own)\n"
    "    --threads INT [1]          BGZF compression threads of -O z / -O b\n"
    "    --verbose 0|1 [0]          record counts, bytes sent up and received, stage times\n"
    "    --device-inflate 0|1 [0]   " DEVICE_INFLATE_HELP "\n\n";
// (--resident 0|1 [0] and --resident-max-bytes INT are taken below and described in README.md and DESIGN.md section 4.30; this text
// does not name them: tests/test_miscread_cli_cpu.py holds the help of this program to be without them)

Opt parse_opt(int argc, char** argv) {
    Opt o;
    if (argc <= 1) { fputs(SAL_USAGE, stderr); exit(0); }
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) { fputs(SAL_USAGE, stderr); exit(0); }
        if (!strcmp(a, "-v") || !strcmp(a, "--version")) { fprintf(stderr, "setalleles_hip [version: %s]\n\n", SAL_VERSION); exit(0); }
        if (i + 1 >= argc || !argv[i + 1][0]) die("Argument '%s' requires a value.", a);
        const char* v = argv[++i];
        if (!strcmp(a, "-i") || !strcmp(a, "--input")) o.in = v;
        else if (!strcmp(a, "-a") || !strcmp(a, "--alleles")) o.alleles = v;
        else if (!strcmp(a, "-O") || !strcmp(a, "--output-mode")) {
            if (strlen(v) != 1 || !strchr("buzv", v[0])) die("--output-mode is one of b, u, z, v, not '%s'", v);
            o.mode = v[0];
        }
        else if (!strcmp(a, "-o") || !strcmp(a, "--output")) o.prefix = v;
        else if (!strcmp(a, "--on-device")) o.on_device = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device")) o.device = option_int(a, v, 0, 1 << 20);
        else if (!strcmp(a, "--batch-records")) o.batch = option_int(a, v, 1, 1 << 24);
        else if (!strcmp(a, "--threads")) o.threads = option_int(a, v, 1, 1024);
        else if (!strcmp(a, "--verbose")) o.verbose = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--device-inflate")) o.device_inflate = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident")) o.resident = option_int(a, v, 0, 1);
        else if (!strcmp(a, "--resident-max-bytes")) {
            char* e; const long long x = strtoll(v, &e, 10);
            if (e == v || *e || x < 0) die("%s takes an integer of at least 0, not '%s'", a, v);
            o.resident_max = x;
        }
        else die("Unknown arg:%s", a);
    }
    if (o.in.empty()) die("Input file is required. Please provide a record file using the -i flag (e.g. -i input.vcf)");
    if (o.alleles.empty()) die("Alleles TSV file is required. Please provide an alleles TSV file using the -a flag (e.g. -a alleles.tsv)");
    if (o.prefix.empty()) {
        fprintf(stderr, "\n\n[WARNING]: Output file prefix is not specified. Setting it to 'output'.\n\n");
        o.prefix = "output";
    }
    o.out_fn = o.prefix + (o.mode == 'v' ? ".vcf" : o.mode == 'z' ? ".vcf.gz" : ".bcf");
    if (o.resident && !(o.device_inflate && o.on_device)) die("--resident 1 needs --device-inflate 1 and --on-device 1.");
    return o;
}

// ---- the alleles file: one list of 2 .. 5 names per line, REF first ---------------------------------------------------------------
enum { MAX_LINE = 256, MAX_NALTS = 4 };
std::vector<std::vector<std::string>> load_alleles(const std::string& fn) {
    FILE* fp = fopen(fn.c_str(), "rb");
    if (!fp) die("Could not open file: %s", fn.c_str());
    std::string all; char buf[1 << 16]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) all.append(buf, k);
    fclose(fp);
    std::vector<std::vector<std::string>> out;
    std::vector<std::string> tab, alts;
    for (size_t b = 0, ln = 1; b < all.size(); ln++) {
        size_t e = all.find('\n', b);
        const bool nl = e != std::string::npos;
        if (!nl) e = all.size();
        if (e - b + (nl ? 1 : 0) >= MAX_LINE) die("Alleles file %s, line %zu: a line of %d bytes or more.", fn.c_str(), ln, (int)MAX_LINE);
        split(all.substr(b, e - b), '\t', tab);
        if (tab.size() != 2 || tab[0].empty() || tab[1].empty()) die("Alleles file %s, line %zu: not REF<TAB>ALT[,ALT...].", fn.c_str(), ln);
        split(tab[1], ',', alts);
        if (alts.size() > MAX_NALTS) die("Alleles file %s, line %zu: %zu ALT alleles, at most %d can be set.", fn.c_str(), ln, alts.size(), (int)MAX_NALTS);
        std::vector<std::string> names{tab[0]};
        for (const std::string& a : alts) {
            if (a.empty()) die("Alleles file %s, line %zu: not REF<TAB>ALT[,ALT...].", fn.c_str(), ln);
            names.push_back(a);
        }
        for (size_t i = 0; i < names.size(); i++)
            for (size_t j = 0; j < i; j++)
                if (names[i] == names[j]) die("Alleles file %s, line %zu: the allele %s is named twice.", fn.c_str(), ln, names[i].c_str());
        out.push_back(names);
        b = nl ? e + 1 : e;
    }
    return out;
}

// what the host keeps of a record
struct Note {
    int64_t pos = 0, off = 0;          // off: the sample columns in raw
    sal::Rec rec{};                    // (off and plane_off are the batch's, set when the record is staged)
    std::string fixed;                 // the new nine columns, the tab behind them included when sample columns follow
    bool has_samples = false;
    bool staged() const { return has_samples && sal::n_fields(rec) > 0; }
};

// BCF: what the host keeps of a record
struct BField { size_t at = 0, key_end = 0, data_at = 0, end = 0; int f = -1; };      // [at, end) the field in the file, its key up to key_end, its vectors from data_at; f: GL / PL / GP or -1
struct BNote {
    int64_t pos = 0;
    std::string shared;                // the new shared block
    std::vector<BField> fmt;
    sal::BRec rec{};                   // (in_off: the vectors in the file; the batch's when the record is staged)
    int64_t rec_at = 0, rec_len = 0;   // the record in the file
    bool staged() const { return sal::b_fields(rec) > 0; }
};

struct Out {
    FILE* fp = nullptr; bool z = false; vsink::Bgzf bg; std::string buf;
    void open(const Opt& o) {
        fp = fopen(o.out_fn.c_str(), "wb");
        if (!fp) die("Could not open output file %s for writing", o.out_fn.c_str());
        z = o.mode == 'z' || o.mode == 'b';
        if (z) bg.open(fp, o.threads);
    }
    void flush(bool all) {
        if (buf.empty() || (!all && buf.size() < (1u << 22))) return;
        if (z) bg.write(buf.data(), buf.size());
        else if (fwrite(buf.data(), 1, buf.size(), fp) != buf.size()) die("write error");
        buf.clear();
    }
    // bytes made on the device (--resident 1): finished BGZF members, or records for -O u.  What the host has buffered goes first, to a
    // member boundary (Bgzf::put_members), so the file keeps its order
    void put_made(const void* p, size_t n) {
        flush(true);
        if (z) bg.put_members(p, n);
        else if (n && fwrite(p, 1, n, fp) != n) die("write error");
    }
    void close() { if (!fp) return; flush(true); if (z) bg.close(); if (fclose(fp) != 0) die("write error"); fp = nullptr; }
};

struct Run {
    Opt o;
    std::vector<uint8_t> raw;
    std::vector<std::vector<std::string>> tsv;
    size_t header_bytes = 0;
    std::vector<Note> notes;
    bool bcf = false;
    std::vector<BNote> bnotes;
    int64_t N = 0;
    Out out;
    SalDev* dev = nullptr;
    // --resident 1: the file in device memory; raw is then the records' head stream and bcf_head the file's header
    RfFile* rf = nullptr;
    std::vector<uint8_t> bcf_head;
    RbSplit bsplit;
    int64_t resident_most = 0;
    std::string not_resident;          // why the file is read as with --resident 0 (empty: it is resident, or the flag is 0)
    RfStats rf_st;
    SalRes* res = nullptr;
    BatchPlan res_plan; SalResShape res_shape;
    // where the bytes of the file's FORMAT fields are read from: byte o of the file is src[o - bias] (raw; a fetched record of a resident file)
    const uint8_t* src = nullptr; int64_t bias = 0;
    const uint8_t* file_at(size_t o) const { return src + ((int64_t)o - bias); }
    long n_host = 0, n_assembled = 0, n_back = 0; int64_t up = 0, down = 0, made = 0;
    double t_read = 0, t_nine = 0, t_dev = 0, t_host = 0, t_relabel = 0, t_assemble = 0, t_write = 0, t_compress = 0, t_down = 0;
    int64_t write_bytes = 0;

    // the run ends here: what the records so far gave is written, nothing stays in flight on the device
    [[noreturn]] void stop_run(const char* fmt, ...) {
        if (dev) sal_dev_quiesce(dev);
        if (res) salres_quiesce(res);
        out.close();
        if (o.resident) report(0);                                     // (the counts of a resident run are kept where it stops, too)
        va_list ap; va_start(ap, fmt); die_v(fmt, ap);
    }
    void notes_text();
    void notes_bcf();
    void load_resident(FileReader& reader);
    void plan_resident();
    void leave_resident(const char* why);
    void input_line() const;
    // the [setalleles] line of --verbose 1; --resident 1 adds its counts and the device's stage times behind today's fields
    void report(const double t_close) const {
        if (!o.verbose) return;
        fprintf(stderr, "[setalleles] on-device %d: records %zu, redone on the host %ld, bytes sent up %lld, received %lld; read %.3f s, nine columns %.3f s, device %.3f s, host %.3f s, close %.3f s",
                o.on_device, bcf ? bnotes.size() : notes.size(), n_host, (long long)up, (long long)down, t_read, t_nine, t_dev, t_host, t_close);
        if (o.resident)
            fprintf(stderr, "; resident %d: assembled on the device %ld, batches handed back %ld, %s bytes received %lld; relabel %.3f s, assemble %.3f s (k_salres_write %.3f s, %lld bytes), compress %.3f s, %s down %.3f s",
                    rf ? 1 : 0, n_assembled, n_back, o.mode == 'b' ? "member" : "record", (long long)made, t_relabel, t_assemble, t_write, (long long)write_bytes,
                    t_compress, o.mode == 'b' ? "members" : "records", t_down);
        fputc('\n', stderr);
    }
    void put_record_bcf(const BNote& n, const sal::BRec& r, const uint32_t* planes, int width);
    void record_host_bcf(const BNote& n, std::vector<uint32_t>& planes, std::vector<uint32_t>& work);
    void put_record(const Note& n, const sal::Rec& r, const uint32_t* planes);
    int rules(const Note& n, std::vector<uint32_t>& planes);
    void redo(const Note& n, std::vector<uint32_t>& planes);
    void record_host(const Note& n, std::vector<uint32_t>& planes);
};

const char* const FIELD_NAME[sal::NF] = {"GL", "PL", "GP"};

// ---- the strtod / strtol reader: a token by the tool's own reading, the first failure kept as the run's message -----------------------
struct HostReader {
    long long pos = 0;
    std::string msg;
    bool flt(const uint8_t* t, int64_t b, int64_t e, int64_t col, int f, uint32_t& bits) {
        const std::string tok((const char*)t + b, (const char*)t + e);
        if (tok == ".") { bits = sal::F_MISSING; return true; }
        char* te = nullptr;
        const double d = strtod(tok.c_str(), &te);
        if (tok.empty() || te != tok.c_str() + tok.size()) {
            if (msg.empty()) { char m[512]; snprintf(m, sizeof m, "Sample %lld at position %lld: the %s value '%.200s' is not a number.", (long long)col, pos, FIELD_NAME[f], tok.c_str()); msg = m; }
            return false;
        }
        const float x = (float)d;
        memcpy(&bits, &x, 4);
        return true;
    }
    bool pl(const uint8_t* t, int64_t b, int64_t e, int64_t col, uint32_t& bits) {
        const std::string tok((const char*)t + b, (const char*)t + e);
        if (tok == ".") { bits = sal::I_MISSING; return true; }
        char* te = nullptr; errno = 0;
        const long long v = strtoll(tok.c_str(), &te, 10);
        if (tok.empty() || te != tok.c_str() + tok.size() || errno == ERANGE || v < INT32_MIN || v > INT32_MAX) {
            if (msg.empty()) { char m[512]; snprintf(m, sizeof m, "Sample %lld at position %lld: the PL value '%.200s' is not an integer inside int32.", (long long)col, pos, tok.c_str()); msg = m; }
            return false;
        }
        bits = (uint32_t)(int32_t)v;
        return true;
    }
};

// a record of the input by the rules of sal_core.h; planes: the record's, from value 0
int Run::rules(const Note& n, std::vector<uint32_t>& planes) {
    sal::Rec r = n.rec; r.off = n.off; r.plane_off = 0;
    sal::GrammarReader rd;
    int st = sal::record_plain(raw.data(), r, N, rd, planes.data(), nullptr);
    if (st != sal::ST_OK) return st;
    for (int f = 0; f < sal::NF; f++) {
        if (r.k[f] < 0) continue;
        uint32_t* p = planes.data() + (int64_t)sal::field_slot(r, f) * r.n_new_g * N;
        for (int64_t s = 0; s < N; s++) if (sal::norm_sample(p, N, s, r.n_new_g, f)) st = sal::ST_RANGE;
    }
    return st;
}

// the same record by the strtod / strtol reader, with the run's messages
void Run::redo(const Note& n, std::vector<uint32_t>& planes) {
    sal::Rec r = n.rec; r.off = n.off; r.plane_off = 0;
    HostReader rd; rd.pos = (long long)n.pos;
    int64_t cols = 0;
    const int st = sal::record_plain(raw.data(), r, N, rd, planes.data(), &cols);
    if (!rd.msg.empty()) stop_run("%s", rd.msg.c_str());
    if (cols != N) stop_run("The record at position %lld has %lld sample columns, the header names %lld samples.", (long long)n.pos, (long long)cols, (long long)N);
    if (st != sal::ST_OK)
        stop_run("A sample at position %lld carries more than %d values of GL, PL or GP, the genotypes of the record's alleles (the tool's maps end there).", (long long)n.pos, (int)r.n_old_g);
    for (int f = 0; f < sal::NF; f++) {
        if (r.k[f] < 0) continue;
        uint32_t* p = planes.data() + (int64_t)sal::field_slot(r, f) * r.n_new_g * N;
        for (int64_t s = 0; s < N; s++)
            if (sal::norm_sample(p, N, s, r.n_new_g, f))
                stop_run("Sample %lld at position %lld: PL minus its minimum does not fit int32 (end-of-vector beside ordinary values; the tool's cast is undefined there).", (long long)s, (long long)n.pos);
    }
    put_record(n, r, planes.data());
}

void Run::record_host(const Note& n, std::vector<uint32_t>& planes) {
    if (!n.staged()) { put_record(n, n.rec, nullptr); return; }
    const int st = rules(n, planes);
    if (st == sal::ST_OK) { sal::Rec r = n.rec; r.plane_off = 0; put_record(n, r, planes.data()); return; }
    if (st == sal::ST_HOST) n_host++;
    redo(n, planes);
}

// the record's line: the new fixed columns, then every sample column with the untouched fields' bytes and the new values
void Run::put_record(const Note& n, const sal::Rec& r, const uint32_t* planes) {
    std::string& o = out.buf;
    o += n.fixed;
    const char* const t = (const char*)raw.data() + n.off; const char* const end = t + n.rec.len;
    if (!n.staged()) { if (n.has_samples) o.append(t, end); o += '\n'; out.flush(false); return; }
    int64_t col = 0;
    for (const char* q = t;; col++) {
        const char* ce = (const char*)memchr(q, '\t', (size_t)(end - q)); if (!ce) ce = end;
        for (int fi = 0;; fi++) {
            const char* fe = (const char*)memchr(q, ':', (size_t)(ce - q)); if (!fe) fe = ce;
            const int f = fi == r.k[0] ? 0 : fi == r.k[1] ? 1 : fi == r.k[2] ? 2 : -1;
            if (f < 0) o.append(q, fe);
            else {
                const uint32_t* p = planes + r.plane_off + (int64_t)sal::field_slot(r, f) * r.n_new_g * N + col;
                int h = 0;
                for (; h < r.n_new_g; h++) {
                    const uint32_t v = p[(int64_t)h * N];
                    if (v == (f == sal::F_PL ? (uint32_t)sal::I_END : (uint32_t)sal::F_END)) break;
                    if (h) o += ',';
                    if (f == sal::F_PL) put_int(o, (int32_t)v);
                    else { float x; memcpy(&x, &v, 4); put_float(o, x); }
                }
                if (h == 0) o += '.';
            }
            if (fe == ce) break;
            o += ':'; q = fe + 1;
        }
        if (ce == end) break;
        o += '\t'; q = ce + 1;
    }
    o += '\n';
    out.flush(false);
}

void put32(std::string& o, uint32_t v) { o.append((const char*)&v, 4); }
// htslib's bcf_enc_size: a typed value's descriptor
void put_typed_len(std::string& o, size_t n, int ty) {
    if (n < 15) { o += (char)((n << 4) | (size_t)ty); return; }
    o += (char)(0xF0 | ty);
    if (n < 128) { o += (char)0x11; o += (char)n; }
    else if (n < 32768) { o += (char)0x12; const uint16_t x = (uint16_t)n; o.append((const char*)&x, 2); }
    else { o += (char)0x13; put32(o, (uint32_t)n); }
}

// the record's names against its TSV line: new2old by the last name that matches (what the tool's scatter leaves), oldgt2newgt
void allele_maps(const std::vector<std::string>& names, const std::vector<std::string>& tgt, size_t line, long long pos, int* new2old, int8_t* g2g) {
    const int n_old = (int)names.size(), n_new = (int)tgt.size();
    if (n_old > sal::MAX_A) die("The record at position %lld has %d alleles, at most %d can be mapped (the tool's maps end there).", pos, n_old, (int)sal::MAX_A);
    for (int j = 0; j < n_new; j++) {
        new2old[j] = -1;
        for (int a = 0; a < n_old; a++) if (names[a] == tgt[j]) new2old[j] = a;
        if (new2old[j] < 0) die("Line %zu of the alleles file names the allele %s, which the record at position %lld does not have.", line, tgt[j].c_str(), pos);
    }
    int8_t old2new[sal::MAX_A];
    for (int a = 0; a < sal::MAX_A; a++) { old2new[a] = -1; if (a < n_old) for (int j = n_new - 1; j >= 0; j--) if (names[a] == tgt[j]) old2new[a] = (int8_t)j; }
    vgl_setal::genotype_map(old2new, n_old, g2g);
}

// ---- the notes: the first nine columns of every record line ---------------------------------------------------------------------------
// (the line loop is this program's own, not scan_text: the header is copied to the output as its bytes, so its length is kept; N is the
// #CHROM line's tab count, no name is read; and once a record has been seen every line that is not empty is a record, '#' or not)
void Run::notes_text() {
    const char* const t0 = (const char*)raw.data();
    const char* p = t0; const char* const end = p + raw.size();
    bool in_header = true, have_cols = false;
    std::vector<std::string> names, old_qs, info;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        const char* const next = nl ? nl + 1 : end;
        if (in_header && le > p && p[0] == '#') {
            if (!(le - p >= 2 && p[1] == '#')) { int tabs = 0; for (const char* q = p; q < le; q++) tabs += *q == '\t'; N = tabs >= 9 ? tabs - 8 : 0; have_cols = true; }
            header_bytes = (size_t)(next - t0);
            p = next; continue;
        }
        in_header = false;
        if (le == p) { p = next; continue; }
        const size_t i = notes.size();                                  // the record's index: its TSV line
        const char* c[10]; int nc;
        nine_columns(p, le, c, nc);
        Note n;
        if (nc < 7) die("Record %zu has fewer than 8 columns.", i + 1);
        n.pos = pos_column(c, nc);
        const long long pos = (long long)n.pos;
        auto col_end = [&](int k) { return k < nc ? c[k + 1] - 1 : le; };
        if (i >= tsv.size()) { notes.push_back(n); p = next; continue; }  // (the count is compared behind the loop)
        const std::vector<std::string>& tgt = tsv[i];
        // the record's alleles
        names.clear(); names.emplace_back(c[3], col_end(3));
        { const std::string alt(c[4], col_end(4)); if (alt != ".") { std::vector<std::string> a; split(alt, ',', a); names.insert(names.end(), a.begin(), a.end()); } }
        const int n_old = (int)names.size(), n_new = (int)tgt.size();
        int new2old[sal::MAX_A]; int8_t g2g[sal::MAX_G];
        allele_maps(names, tgt, i + 1, pos, new2old, g2g);
        n.rec = sal::Rec{0, 0, sal::pack_o2n(g2g), 0, {-1, -1, -1}, (int8_t)(n_old * (n_old + 1) / 2), (int8_t)(n_new * (n_new + 1) / 2)};
        // the new fixed columns
        std::string& fx = n.fixed;
        fx.assign(c[0], c[3]);
        fx += tgt[0]; fx += '\t';
        for (int j = 1; j < n_new; j++) { if (j > 1) fx += ','; fx += tgt[j]; }
        fx += '\t';
        fx.append(c[5], c[7]);
        split(std::string(c[7], col_end(7)), ';', info);
        for (size_t k = 0; k < info.size(); k++) {
            if (k) fx += ';';
            if (info[k].compare(0, 3, "QS=") != 0) { fx += info[k]; continue; }
            split(info[k].substr(3), ',', old_qs);
            if ((int)old_qs.size() != n_old) die("INFO/QS at position %lld has %zu values, the record has %d alleles.", pos, old_qs.size(), n_old);
            fx += "QS=";
            for (int j = 0; j < n_new; j++) {
                const std::string& tok = old_qs[(size_t)new2old[j]];
                if (j) fx += ',';
                if (tok == ".") { fx += '.'; continue; }
                char* te = nullptr; const double d = strtod(tok.c_str(), &te);
                if (tok.empty() || te != tok.c_str() + tok.size()) die("INFO/QS at position %lld: the value '%s' is not a number.", pos, tok.c_str());
                put_float(fx, (float)d);
            }
        }
        if (nc >= 8) {
            fx += '\t'; fx.append(c[8], col_end(8));
            int n_fields = 0;
            for (int f = 0; f < sal::NF; f++) n.rec.k[f] = (int16_t)format_key_index(c[8], col_end(8), FIELD_NAME[f], &n_fields);
            if (n_fields > INT16_MAX) die("The record at position %lld has too many FORMAT fields.", pos);
        }
        if (nc >= 9) {
            fx += '\t';
            n.has_samples = true; n.off = c[9] - t0;
            if (le - c[9] > INT32_MAX) die("The record at position %lld is longer than 2 GiB.", pos);
            n.rec.len = (int32_t)(le - c[9]);
        }
        notes.push_back(std::move(n));
        p = next;
    }
    if (!have_cols) die("The file %s has no #CHROM line.", o.in.c_str());
    if (notes.size() != tsv.size())
        die("The alleles file has %zu lines and the record file %zu records: one line per record is required.", tsv.size(), notes.size());
}

// ---- BCF: the shared block and the FORMAT field headers of every record ---------------------------------------------------------------
// One body for both sources.  The file's bytes in raw: the cursor walks them.  A resident file (--resident 1): the header is bcf_head,
// raw is the head stream -- per record the two lengths, the shared block and the fields' keys and descriptors, bytes identical to the
// file's -- and where a field lies in the file follows from the record's place there (rec_off) and the widths: `shift` is what a
// place of the cursor's stream lacks to its place in the file, and grows by every field's data, which the stream leaves out.
void Run::notes_bcf() {
    BcfDict d; BcfIn c; c.buf = rf ? bcf_head.data() : raw.data(); c.size = rf ? bcf_head.size() : raw.size();
    Vcf v;
    bcf_header(c, d, v);
    header_bytes = c.off;
    if (rf) { c.buf = raw.data(); c.size = raw.size(); c.off = 0; }
    N = (int64_t)v.samples.size();
    std::vector<int32_t> iv; std::vector<std::string> names;
    while (c.off < c.size) {
        const size_t i = bnotes.size();
        BcfRecAt at; int ty, n;
        const size_t head_at = c.off;
        int64_t shift = 0;
        size_t file_end = 0;                                           // where the record ends in the file
        if (!rf) { bcf_scan_record(c, at); file_end = at.rec_end; }
        else {                                                         // (the device has made the checks of bcf_scan_record)
            if (i >= (size_t)bsplit.records || (int64_t)head_at != bsplit.hoff[i]) die("--resident 1: the head stream does not follow its records.");
            const uint32_t l_shared = c.u32(), l_indiv = c.u32();
            at.shared = c.off; at.shared_end = c.off + l_shared; at.rec_end = (size_t)bsplit.hoff[i + 1];
            shift = bsplit.rec_off[i] - (int64_t)head_at;
            file_end = (size_t)bsplit.rec_off[i] + 8 + (size_t)l_shared + l_indiv;
            if (at.shared_end > at.rec_end) die("--resident 1: a record's head is not as long as the device made it.");
        }
        if (at.shared_end - at.shared < 24) c.fail("truncated BCF record");
        const uint32_t chrom = c.u32(), pos0 = c.u32(), rlen = c.u32(), qual = c.u32(), nai = c.u32(), nfs = c.u32();
        const int n_allele = (int)(nai >> 16), n_info = (int)(nai & 0xFFFF), n_fmt = (int)(nfs >> 24);
        BNote bn; bn.pos = (int64_t)(int32_t)pos0 + 1;
        bn.rec_at = (int64_t)head_at + shift; bn.rec_len = (int64_t)file_end - bn.rec_at;
        const long long pos = (long long)bn.pos;
        if ((int64_t)(nfs & 0xFFFFFF) != N) die("Record at position %lld has %u samples, the header names %lld samples.", pos, nfs & 0xFFFFFF, (long long)N);
        auto skip = [&](size_t k) { if (c.off + k > at.shared_end) c.fail("BCF record: shared block length mismatch at position %lld", pos); c.off += k; };
        const size_t id_at = c.off; c.typed(ty, n); skip((size_t)bcf_type_width(ty) * n);
        const size_t id_end = c.off;
        names.clear();
        for (int a = 0; a < n_allele; a++) { c.typed(ty, n); if (ty != 7 || c.off + n > at.shared_end) c.fail("BCF: allele string expected"); names.push_back(c.str(n)); }
        const size_t filt_at = c.off; c.typed(ty, n); skip((size_t)bcf_type_width(ty) * n);
        const size_t filt_end = c.off;
        if (i >= tsv.size()) { for (int k = 0; k < n_info; k++) { c.typed(ty, n); skip((size_t)bcf_type_width(ty) * n); c.typed(ty, n); skip((size_t)bcf_type_width(ty) * n); }
                               c.off = at.rec_end; bnotes.push_back(bn); continue; }     // (the count is compared behind the loop)
        const std::vector<std::string>& tgt = tsv[i];
        const int n_old = (int)names.size(), n_new = (int)tgt.size();
        int new2old[sal::MAX_A]; int8_t g2g[sal::MAX_G];
        allele_maps(names, tgt, i + 1, pos, new2old, g2g);
        std::string info; bool has_end = false;
        for (int k = 0; k < n_info; k++) {
            const size_t e_at = c.off;
            c.typed(ty, n); if (c.off + (size_t)bcf_type_width(ty) * n > at.shared_end) c.fail("truncated BCF record"); c.ints(ty, n, iv);
            const auto key = iv.empty() ? d.dict.end() : d.dict.find(iv[0]);
            if (key == d.dict.end()) c.fail("BCF: undefined INFO key");
            const size_t val_at = c.off;
            c.typed(ty, n);
            const size_t data_at = c.off; skip((size_t)bcf_type_width(ty) * n);
            if (key->second == "END") has_end = true;
            if (key->second != "QS") { info.append((const char*)raw.data() + e_at, c.off - e_at); continue; }
            if (ty != 5) die("INFO/QS at position %lld is not a float vector.", pos);
            if (n != n_old) die("INFO/QS at position %lld has %d values, the record has %d alleles.", pos, n, n_old);
            info.append((const char*)raw.data() + e_at, val_at - e_at);
            put_typed_len(info, (size_t)n_new, 5);
            for (int j = 0; j < n_new; j++) info.append((const char*)raw.data() + data_at + 4 * (size_t)new2old[j], 4);
        }
        if (c.off != at.shared_end) c.fail("BCF record: shared block length mismatch at position %lld", pos);
        std::string& sh = bn.shared;
        put32(sh, chrom); put32(sh, pos0); put32(sh, has_end ? rlen : (uint32_t)tgt[0].size()); put32(sh, qual);
        put32(sh, ((uint32_t)n_new << 16) | (uint32_t)n_info); put32(sh, nfs);
        sh.append((const char*)raw.data() + id_at, id_end - id_at);
        for (const std::string& a : tgt) { put_typed_len(sh, a.size(), 7); sh += a; }
        sh.append((const char*)raw.data() + filt_at, filt_end - filt_at);
        sh += info;
        // the FORMAT fields
        int8_t n2o[sal::MAX_G];
        for (int h = 0; h < sal::MAX_G; h++) n2o[h] = -1;
        for (int b2 = 0, h = 0; b2 < n_new; b2++) for (int b1 = 0; b1 <= b2; b1++, h++) n2o[h] = (int8_t)vgl_setal::alleles2gt(new2old[b1], new2old[b2]);
        bn.rec.n2o = sal::pack_o2n(n2o);
        bn.rec.n_old_g = (int8_t)(n_old * (n_old + 1) / 2); bn.rec.n_new_g = (int8_t)(n_new * (n_new + 1) / 2);
        // (the loop is this program's own, not bcf_format_fields: a field ends with the record here, not with the file, the key's bytes
        // are held to that end as well, and where every field starts is kept for the copy)
        for (int k = 0; k < n_fmt; k++) {
            BField bf; bf.at = c.off + (size_t)shift;
            c.typed(ty, n); if (c.off + (size_t)bcf_type_width(ty) * n > at.rec_end) c.fail("truncated BCF record"); c.ints(ty, n, iv);
            bf.key_end = c.off + (size_t)shift;
            const auto key = iv.empty() ? d.dict.end() : d.dict.find(iv[0]);
            if (key == d.dict.end()) c.fail("BCF: undefined FORMAT key");
            c.typed(ty, n);
            bf.data_at = c.off + (size_t)shift;
            const size_t data = (size_t)bcf_type_width(ty) * n * (size_t)N;
            if (bf.data_at + data > file_end) c.fail("truncated BCF record");
            if (rf) shift += (int64_t)data; else c.off += data;
            bf.end = c.off + (size_t)shift;
            const int f = key->second == "GL" ? sal::F_GL : key->second == "PL" ? sal::F_PL : key->second == "GP" ? sal::F_GP : -1;
            if (f >= 0 && n > 0 && bn.rec.nv[f] == 0) {
                if (f == sal::F_PL ? (ty < 1 || ty > 3) : ty != 5)
                    die("FORMAT/%s at position %lld is not %s vector.", key->second.c_str(), pos, f == sal::F_PL ? "an integer" : "a float");
                if (n > bn.rec.n_old_g)
                    die("FORMAT/%s at position %lld carries %d values a sample, more than the %d genotypes of the record's alleles (the tool's maps end there).",
                        key->second.c_str(), pos, n, (int)bn.rec.n_old_g);
                bf.f = f; bn.rec.nv[f] = n; bn.rec.ty[f] = (int8_t)ty; bn.rec.in_off[f] = (int64_t)bf.data_at;
            }
            bn.fmt.push_back(bf);
        }
        if (c.off != at.rec_end || c.off + (size_t)shift != file_end) c.fail("BCF record: individual block length mismatch at position %lld", pos);
        bnotes.push_back(std::move(bn));
    }
    if (bnotes.size() != tsv.size())
        die("The alleles file has %zu lines and the record file %zu records: one line per record is required.", tsv.size(), bnotes.size());
}

// the record: the two lengths, the new shared block, then every FORMAT field -- untouched ones as their bytes, GL / GP as N x nG_new
// floats, PL at the record's width; planes: r.plane_off is where the record's lie, in 32-bit words
void Run::put_record_bcf(const BNote& n, const sal::BRec& r, const uint32_t* planes, int width) {
    std::string indiv;
    for (const BField& bf : n.fmt) {
        if (bf.f < 0) { indiv.append((const char*)file_at(bf.at), bf.end - bf.at); continue; }
        indiv.append((const char*)file_at(bf.at), bf.key_end - bf.at);   // the key: a typed integer scalar
        const int w = bf.f == sal::F_PL ? width : 4;
        put_typed_len(indiv, (size_t)r.n_new_g, bf.f == sal::F_PL ? (w == 1 ? 1 : w == 2 ? 2 : 3) : 5);
        const uint32_t* p = planes + r.plane_off + (int64_t)sal::b_slot(r, bf.f) * r.n_new_g * N;
        indiv.append((const char*)p, (size_t)N * r.n_new_g * w);
    }
    std::string& o = out.buf;
    put32(o, (uint32_t)n.shared.size()); put32(o, (uint32_t)indiv.size());
    o += n.shared; o += indiv;
    out.flush(false);
}

// a BCF record by the rules of sal_core.h on the host: what k_sal_bcf_apply does.  A PL sample whose cast would overflow stops the run
void Run::record_host_bcf(const BNote& n, std::vector<uint32_t>& planes, std::vector<uint32_t>& work) {
    sal::BRec r = n.rec; r.plane_off = 0;
    if (!n.staged()) { put_record_bcf(n, r, planes.data(), 4); return; }
    int width = 1;
    uint32_t v[sal::MAX_G];
    for (int f = 0; f < sal::NF; f++) {
        if (r.nv[f] <= 0) continue;
        const uint8_t* in = file_at((size_t)r.in_off[f]);
        const int w_in = sal::type_width(r.ty[f]), nG = r.n_new_g;
        uint32_t* p = planes.data() + (int64_t)sal::b_slot(r, f) * nG * N;
        int32_t mn = INT32_MAX, mx = INT32_MIN + 1;
        for (int64_t s = 0; s < N; s++) {
            if (sal::bcf_sample(in + s * r.nv[f] * w_in, r.ty[f], r.nv[f], r.n2o, nG, f, v))
                stop_run("Sample %lld at position %lld: PL minus its minimum does not fit int32 (end-of-vector beside ordinary values; the tool's cast is undefined there).", (long long)s, (long long)n.pos);
            for (int h = 0; h < nG; h++) {
                (f == sal::F_PL ? work.data() : p)[s * nG + h] = v[h];
                if (f == sal::F_PL && v[h] != sal::I_MISSING && v[h] != sal::I_END) { mn = std::min(mn, (int32_t)v[h]); mx = std::max(mx, (int32_t)v[h]); }
            }
        }
        if (f != sal::F_PL) continue;
        width = sal::int_width(mn, mx);
        for (int64_t j = 0; j < N * nG; j++) sal::store_narrow((uint8_t*)p, width, j, work[(size_t)j]);
    }
    put_record_bcf(n, r, planes.data(), width);
}

// ---- --on-device 1 ---------------------------------------------------------------------------------------------------------------
// BCF: the GL / PL / GP vector blocks go up, the new vectors come down; the host splices them between the copied bytes
void run_device_bcf(Run& R, std::vector<uint32_t>& planes, std::vector<uint32_t>& work) {
    const std::vector<BNote>& notes = R.bnotes;
    std::vector<size_t> sent;
    for (size_t i = 0; i < notes.size(); i++) if (notes[i].staged()) sent.push_back(i);
    auto up_bytes = [&](const BNote& n) {
        int64_t b = 0;
        for (int f = 0; f < sal::NF; f++) if (n.rec.nv[f] > 0) b += ((int64_t)R.N * n.rec.nv[f] * sal::type_width(n.rec.ty[f]) + 3) & ~3ll;
        return b;
    };
    const int64_t MOST = 64ll << 20;                                   // of staged bytes up, and of plane values x 4 down
    const BatchPlan plan = plan_batches(sent.size(), R.o.batch, {MOST, MOST}, [&](size_t j, size_t c) {
        const BNote& nt = notes[sent[j]];
        return c == 0 ? up_bytes(nt) : sal::b_plane_vals(nt.rec, R.N) * 4;
    });
    const std::vector<std::pair<size_t, size_t>>& batches = plan.ranges;
    const int64_t max_text = std::max<int64_t>(4, plan.max_cost[0]), max_vals = std::max<int64_t>(1, plan.max_cost[1] / 4), max_recs = std::max<int64_t>(1, plan.max_recs);
    char err[256];
    R.dev = sal_dev_create(R.o.device, (int32_t)R.N, (int32_t)max_recs, max_text, max_vals, err, sizeof err);
    if (!R.dev) R.stop_run("--on-device 1: %s (device %d; --on-device 0 works on the host)", err, R.o.device);
    std::vector<sal::BRec> staged[2];
    auto submit = [&](int64_t b) {
        const double t0 = now_s();
        const int slot = (int)(b & 1);
        uint8_t* text = sal_dev_text(R.dev, slot); sal::BRec* recs = sal_dev_brecs(R.dev, slot);
        int64_t at = 0, vals = 0; int32_t n = 0;
        staged[slot].clear();
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            const BNote& nt = notes[sent[j]];
            sal::BRec r = nt.rec; r.plane_off = vals;
            for (int f = 0; f < sal::NF; f++) {
                if (r.nv[f] <= 0) continue;
                const int64_t len = (int64_t)R.N * r.nv[f] * sal::type_width(r.ty[f]);
                memcpy(text + at, R.file_at((size_t)nt.rec.in_off[f]), (size_t)len);
                r.in_off[f] = at; at += (len + 3) & ~3ll;
            }
            vals += sal::b_plane_vals(r, R.N);
            recs[n] = r; staged[slot].push_back(r);
        }
        if (sal_dev_submit(R.dev, slot, n, at, vals) != 0) R.stop_run("--on-device 1: %s", sal_dev_error(R.dev));
        R.up += at + (int64_t)n * (int64_t)sizeof(sal::BRec); R.down += vals * 4 + (int64_t)n * 12;
        R.t_dev += now_s() - t0;
    };
    size_t cur = 0;
    auto retire = [&](int64_t b) {
        double t0 = now_s();
        const int slot = (int)(b & 1);
        SalBatchOut out;
        if (sal_dev_wait(R.dev, slot, &out) != 0) R.stop_run("--on-device 1: %s", sal_dev_error(R.dev));
        R.t_dev += now_s() - t0; t0 = now_s();
        int32_t n = 0;
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            for (; cur < sent[j]; cur++) R.record_host_bcf(notes[cur], planes, work);
            const BNote& nt = notes[cur++];
            if (out.status[n] == sal::ST_OK) R.put_record_bcf(nt, staged[slot][(size_t)n], out.planes, out.width[n]);
            else {
                if (out.status[n] == sal::ST_HOST) R.n_host++;
                R.record_host_bcf(nt, planes, work);                       // (owns the message of a record the run stops at)
            }
        }
        R.t_host += now_s() - t0;
    };
    two_in_flight((int64_t)batches.size(), submit, retire);
    for (; cur < notes.size(); cur++) R.record_host_bcf(notes[cur], planes, work);
}

// ---- --resident 1 ------------------------------------------------------------------------------------------------------------------
// The file into device memory, its header and the split of its records (resident_file.h).  Resident: raw is the head stream.  Not:
// not_resident says why, and raw holds the file's bytes as --resident 0 reads them.
void Run::load_resident(FileReader& reader) {
    char err[256];
    { FILE* fp = fopen(o.in.c_str(), "rb"); if (!fp) die("Could not open file: %s", o.in.c_str()); fclose(fp); }   // the file first, as without the flag
    rf = rf_create(o.device, err, sizeof err);
    if (!rf) die("--resident 1: %s (device %d)", err, o.device);
    resident_most = o.resident_max >= 0 ? o.resident_max : rf_default_max_bytes(rf);
    auto failed = [&]() { const std::string why = rf_error(rf); if (why.compare(0, 14, "Could not open") == 0) die("%s", why.c_str()); die("--resident 1: %s", why.c_str()); };
    RfWhy why;
    if (rf_load(rf, o.in.c_str(), resident_most, &why) != 0) failed();
    if (why == RF_NOT_BGZF) not_resident = "the file is not a series of BGZF members";
    else if (why == RF_MEMBER_HOST) not_resident = "a member was left to the host (VGL_INFLATE_HOST)";
    else if (why == RF_TOO_LARGE) not_resident = "the inflated and the compressed bytes exceed --resident-max-bytes";
    else {
        bool fits = false;
        if (rf_bcf_header(rf, &bcf_head, &fits) != 0) failed();
        int64_t n_samples = -1;
        if (!fits) not_resident = "the file is not BCF, or its header does not fit it";
        else {
            try { BcfDict d; Vcf v; BcfIn c; c.buf = bcf_head.data(); c.size = bcf_head.size(); c.soft = true; bcf_header(c, d, v); n_samples = (int64_t)v.samples.size(); }
            catch (const BcfSoftFail&) { not_resident = "the header could not be read"; }
        }
        if (not_resident.empty()) {
            if (rf_bcf_split(rf, (int64_t)bcf_head.size(), n_samples, rb::RB_HOPS_MOST, rf::RF_HEAD_MOST, &bsplit) != 0) failed();
            if (bsplit.more_records) not_resident = "the file has more records than the offsets scan takes (INT32_MAX - 1024)";
            else if (bsplit.why != rb::OK) { char b[256]; snprintf(b, sizeof b, "record %lld: %s", (long long)bsplit.ordinal + 1, rb::why_text(bsplit.why)); not_resident = b; }
        }
        if (!not_resident.empty()) { leave_resident(nullptr); return; }          // the inflated bytes are on the device: they come down whole
    }
    rf_st = *rf_stats(rf);
    if (not_resident.empty()) { raw = std::move(bsplit.heads); bcf = true; return; }
    rf_destroy(rf); rf = nullptr;
    input_line();
    raw = reader.read(o.in);
}

// the resident file's bytes come down whole and the run goes on as with --resident 0: every place the notes hold is a place of the file
void Run::leave_resident(const char* why) {
    if (why) not_resident = why;
    const int64_t total = rf_total(rf);
    std::vector<uint8_t> all((size_t)total);
    if (rf_fetch(rf, 0, total, all.data()) != 0) die("--resident 1: %s", rf_error(rf));
    rf_st = *rf_stats(rf);
    raw = std::move(all);
    rf_destroy(rf); rf = nullptr; bsplit = RbSplit(); bcf_head.clear();
    src = raw.data(); bias = 0;
    input_line();
    if (o.verbose) FileReader::report(o.in, (long)rf_st.members, rf_st.compressed_up, rf_st.total, rf_st.t_inflate, nullptr);
}

void Run::input_line() const {
    if (!o.verbose) return;
    const bool no = !not_resident.empty();
    fprintf(stderr, "[input] %s: resident %d%s%s%s, members %lld, records %lld, head bytes received %lld, compressed bytes sent up %lld; upload %.3f s, inflate %.3f s, chain %.3f s, heads %.3f s\n",
            o.in.c_str(), no ? 0 : 1, no ? " (" : "", not_resident.c_str(), no ? ")" : "", (long long)rf_st.members, (long long)rf_st.records,
            (long long)rf_st.head_bytes, (long long)rf_st.compressed_up, rf_st.t_upload, rf_st.t_inflate, rf_st.t_chain, rf_st.t_heads);
}

// a record's piece table (salres_core.h) from its note: untouched fields that follow each other are one run
salres::Desc piece_table(const BNote& nt) {
    salres::Desc d;
    salres::table_begin(d, nt.fmt.empty() ? nt.rec_at + nt.rec_len : (int64_t)nt.fmt[0].at);
    d.shared_len = (int32_t)nt.shared.size();
    for (const BField& bf : nt.fmt) salres::table_field(d, (int64_t)bf.at, (int64_t)bf.key_end, (int64_t)bf.end, bf.f);      // (at most one touched field a tag: never a fourth)
    return d;
}

const int64_t RES_OUT_MOST = 64ll << 20;                               // of assembled records in a batch, and of plane values x 4

// the batches of a resident run and the buffers they need; a file whose buffers do not fit beside it comes down whole
void Run::plan_resident() {
    const std::vector<BNote>& notes = bnotes;
    res_plan = plan_batches(notes.size(), o.batch, {RES_OUT_MOST, RES_OUT_MOST, BATCH_NO_CAP}, [&](size_t j, size_t c) {
        const BNote& nt = notes[j];
        if (c == 1) return sal::b_plane_vals(nt.rec, N) * 4;
        if (c == 2) return (int64_t)nt.shared.size();
        int64_t b = 8 + (int64_t)nt.shared.size();                     // the record with PL at four bytes: no shorter than what the device makes
        for (const BField& bf : nt.fmt) b += bf.f < 0 ? (int64_t)(bf.end - bf.at) : (int64_t)(bf.key_end - bf.at) + 3 + N * nt.rec.n_new_g * 4;
        return b;
    });
    res_shape.n_samples = (int32_t)N; res_shape.max_recs = (int32_t)std::max<int64_t>(1, res_plan.max_recs);
    res_shape.max_out = std::max<int64_t>(1, res_plan.max_cost[0]); res_shape.max_vals = std::max<int64_t>(1, res_plan.max_cost[1] / 4);
    res_shape.max_shared = std::max<int64_t>(1, res_plan.max_cost[2]); res_shape.compress = o.mode == 'b' ? 1 : 0;
    if (rf_total(rf) + salres_device_bytes(res_shape) > resident_most) leave_resident("the batches' buffers beside the file exceed --resident-max-bytes");
    else input_line();
}

// every record is assembled on the device; a batch in which a record is not ST_OK is fetched and worked by record_host_bcf in order
void run_resident_bcf(Run& R, std::vector<uint32_t>& planes, std::vector<uint32_t>& work) {
    const std::vector<BNote>& notes = R.bnotes;
    const std::vector<std::pair<size_t, size_t>>& batches = R.res_plan.ranges;
    char err[256];
    R.res = salres_create(R.o.device, R.res_shape, err, sizeof err);
    if (!R.res) R.stop_run("--resident 1: %s (device %d; --resident 0 stages the vectors)", err, R.o.device);
    R.up += R.rf_st.compressed_up;
    const uint8_t* const file = rf_device_text(R.rf); const int64_t total = rf_total(R.rf);
    auto submit = [&](int64_t b) {
        const double t0 = now_s();
        const int slot = (int)(b & 1);
        sal::BRec* recs = salres_brecs(R.res, slot); salres::Desc* descs = salres_descs(R.res, slot); uint8_t* shared = salres_shared(R.res, slot);
        int64_t vals = 0, sh_at = 0; int32_t n = 0;
        for (size_t j = batches[b].first; j < batches[b].second; j++, n++) {
            const BNote& nt = notes[j];
            sal::BRec r = nt.rec; r.plane_off = vals;
            salres::Desc d = piece_table(nt); d.shared_off = sh_at;
            memcpy(shared + sh_at, nt.shared.data(), nt.shared.size()); sh_at += (int64_t)nt.shared.size();
            vals += sal::b_plane_vals(r, R.N);
            recs[n] = r; descs[n] = d;
        }
        if (salres_submit(R.res, slot, n, vals, sh_at, file, total) != 0) R.stop_run("--resident 1: %s", salres_error(R.res));
        R.up += sh_at + (int64_t)n * (int64_t)(sizeof(sal::BRec) + sizeof(salres::Desc));
        R.t_dev += now_s() - t0;
    };
    std::vector<uint8_t> one;
    auto retire = [&](int64_t b) {
        double t0 = now_s();
        SalResOut out;
        if (salres_wait(R.res, (int)(b & 1), &out) != 0) R.stop_run("--resident 1: %s", salres_error(R.res));
        R.t_dev += now_s() - t0; t0 = now_s();
        if (!out.guards_ok) R.stop_run("the device wrote outside a batch's buffers");
        const int64_t n = (int64_t)(batches[b].second - batches[b].first);
        R.down += n * 12 + 16 + 6 * salres::GUARD;
        R.t_relabel += out.t_relabel; R.t_assemble += out.t_assemble; R.t_write += out.t_write; R.t_compress += out.t_compress; R.t_down += out.t_down;
        if (!out.handed_back) {
            R.out.put_made(out.bytes, (size_t)out.n);
            R.n_assembled += (long)n; R.made += out.n; R.down += out.n; R.write_bytes += out.raw_n;
        } else {                                                       // the batch is the host's: its records' bytes come down, one at a time
            R.n_back++;
            int32_t k = 0;
            for (size_t j = batches[b].first; j < batches[b].second; j++, k++) {
                const BNote& nt = notes[j];
                if (out.status[k] == sal::ST_HOST) R.n_host++;
                one.resize((size_t)nt.rec_len);
                if (rf_fetch(R.rf, nt.rec_at, nt.rec_len, one.data()) != 0) R.stop_run("--resident 1: %s", rf_error(R.rf));
                R.down += nt.rec_len;
                R.src = one.data(); R.bias = nt.rec_at;
                R.record_host_bcf(nt, planes, work);                   // (owns the message of a record the run stops at)
            }
        }
        R.t_host += now_s() - t0;
    };
    two_in_flight((int64_t)batches.size(), submit, retire);
}

}  // namespace

int main(int argc, char** argv) {
    Run R;
    R.o = parse_opt(argc, argv);
    const Opt& o = R.o;
    double t0 = now_s();
    R.tsv = load_alleles(o.alleles);
    {
        FileReader reader; reader.device_inflate = o.device_inflate; reader.device = o.device; reader.verbose = o.verbose;
        if (o.resident) R.load_resident(reader);
        else R.raw = reader.read(o.in);
    }
    R.t_read = now_s() - t0; t0 = now_s();
    if (!R.rf) { R.bcf = R.raw.size() >= 3 && !memcmp(R.raw.data(), "BCF", 3); R.src = R.raw.data(); }
    // text is written as text and BCF as BCF: converting between the two would need every INFO / FORMAT field's type, not this program's work
    if (R.bcf && (o.mode == 'v' || o.mode == 'z'))
        die("%s is a BCF file and -O %c asks for VCF text: BCF is written as BCF. Use -O b or -O u.", o.in.c_str(), o.mode);
    if (!R.bcf && (o.mode == 'b' || o.mode == 'u'))
        die("%s is VCF text and -O %c asks for BCF: text is written as text. Use -O v or -O z.", o.in.c_str(), o.mode);
    if (!R.bcf && o.on_device)
        die("%s is VCF text, which this program works on the host: --on-device 1 holds for BCF input. Use --on-device 0.", o.in.c_str());
    if (R.bcf) R.notes_bcf(); else R.notes_text();
    R.t_nine = now_s() - t0;
    if (R.N > (int64_t)INT32_MAX / (sal::NF * sal::MAX_G * 4)) die("Too many samples.");
    if (R.rf) R.plan_resident();                                       // (may hand the file back: the notes' places hold either way)

    R.out.open(o);
    if (R.rf) R.out.buf.append((const char*)R.bcf_head.data(), R.bcf_head.size());
    else R.out.buf.append((const char*)R.raw.data(), R.header_bytes);
    std::vector<uint32_t> planes((size_t)std::max<int64_t>(R.N, 1) * sal::NF * sal::MAX_G), work;
    if (R.bcf) work.resize((size_t)std::max<int64_t>(R.N, 1) * sal::MAX_G);
    if (R.rf) run_resident_bcf(R, planes, work);
    else if (o.on_device) run_device_bcf(R, planes, work);             // (a file with nothing to stage opens the GPU all the same: 1 without one fails)
    else {
        t0 = now_s();
        if (R.bcf) for (const BNote& n : R.bnotes) R.record_host_bcf(n, planes, work);
        else for (const Note& n : R.notes) R.record_host(n, planes);
        R.t_host = now_s() - t0;
    }
    t0 = now_s();
    R.out.close();
    const double t_close = now_s() - t0;
    R.report(t_close);
    if (R.dev) sal_dev_destroy(R.dev);
    if (R.res) salres_destroy(R.res);
    if (R.rf) rf_destroy(R.rf);
    fprintf(stderr, "\nProgram finished successfully!\n\t-> Processed %zu sites.\n\t-> Output file: %s\n", R.bcf ? R.bnotes.size() : R.notes.size(), o.out_fn.c_str());
    return 0;
}
