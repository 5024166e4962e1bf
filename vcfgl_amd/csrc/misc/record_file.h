// record_file.h -- what the mains of the misc programs share of reading a record file (gtdisc_main.cpp, fetchgl_main.cpp, setal_main.cpp):
// the lines of VCF text, the first nine columns of a record line, a key's place in the FORMAT column, the FORMAT fields of a BCF record,
// and the integer options of the command lines.  The file's bytes come from FileReader below: read_whole (host/host_util.h), or the
// device inflater of vcfgl_hip (--device-inflate 1).  Every refusal of a record stays with the program that words it.
#pragma once
#include "../host/vcf_input.h"

// --device-inflate 0|1 of the three programs: how a record file's bytes are read.  0: read_whole, zlib on one host thread.  1: the
// file as it lies on the disk, its BGZF members inflated on `device` by the reader of vcfgl_hip (inflate_on_device, host/vcf_input.h:
// 512 members a batch, two batches in flight); zlib stays the specification -- a file that is not a clean series of BGZF members, or
// of which a member came back VGL_INFLATE_HOST, is read whole by zlib as with 0, so a damaged file gives what it gives today.
// Without a device the run ends with the library's message.  One reader serves every file of a run (gtdiscordance_hip reads two).
#define DEVICE_INFLATE_HELP "1: the file's BGZF members are inflated on the GPU (any other file: zlib, as with 0); the one thing that opens the GPU under --on-device 0"
struct FileReader {
    int device_inflate = 0, device = 0, verbose = 0;
    vgl_inflate_host* h = nullptr;
    FileReader() = default;
    FileReader(const FileReader&) = delete;
    FileReader& operator=(const FileReader&) = delete;
    ~FileReader() { if (h) vgl_inflate_host_destroy(h); }

    // the [input] line of --verbose 1
    static void report(const std::string& fn, const long members, const int64_t up, const int64_t down, const double t_inflate, const char* fallback) {
        fprintf(stderr, "[input] %s: device-inflate 1, members inflated on the device %ld, bytes sent up %lld, received %lld, inflate %.3f s, read by the host: %s%s%s\n",
                fn.c_str(), members, (long long)up, (long long)down, t_inflate, fallback ? "yes (" : "no", fallback ? fallback : "", fallback ? ")" : "");
    }
    std::vector<uint8_t> read(const std::string& fn) {
        if (!device_inflate) return read_whole(fn);
        InputOpt opt; opt.device_inflate = 1; opt.device = device;
        opt.inflater = [this]() -> vgl_inflate_host* {
            if (!h && vgl_inflate_host_create(device, INFLATE_BATCH, &h) != VGL_OK) die("--device-inflate 1: %s", vgl_last_error());
            return h;
        };
        InputStats st;
        std::vector<uint8_t> raw;
        const bool done = inflate_on_device(fn, opt, raw, st);
        if (!done) raw = read_whole(fn);
        if (verbose) report(fn, done ? st.members_dev : 0, st.inflate_up, done ? st.inflate_down : 0, st.t_inflate, st.fallback);
        return raw;
    }
};

// VCF text: the ## lines, the sample names of the #CHROM line and [begin, end) of every record line; empty lines are skipped
struct TextLines {
    std::vector<std::string> header, samples;
    std::vector<std::pair<int64_t, int64_t>> lines;
};
static TextLines scan_text(const std::vector<uint8_t>& text) {
    TextLines out;
    const char* const t0 = (const char*)text.data();
    const char* p = t0; const char* const end = p + text.size();
    std::vector<std::string> f;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (le > p) {
            if (le - p >= 2 && p[0] == '#' && p[1] == '#') out.header.emplace_back(p, le);
            else if (p[0] == '#') { split(std::string(p, le), '\t', f); for (size_t i = 9; i < f.size(); i++) out.samples.push_back(f[i]); }
            else out.lines.emplace_back(p - t0, le - t0);
        }
        p = nl ? nl + 1 : end;
    }
    return out;
}

// the record line [lb, le): col_at[k] = where column k starts, for k = 0 .. nc; nc = 9 when the line has sample columns
static void nine_columns(const char* lb, const char* le, const char* col_at[10], int& nc) {
    nc = 0; col_at[0] = lb;
    for (const char* q = lb; q < le && nc < 9; q++) if (*q == '\t') col_at[++nc] = q + 1;
}
// POS, column 1 (0 for a line of one column)
static int64_t pos_column(const char* const col_at[10], const int nc) {
    return nc >= 1 ? atoll(std::string(col_at[1], col_at[2 > nc ? nc : 2]).c_str()) : 0;
}

// the FORMAT column [b, e): the index of the first field that is `key`, or -1; n_fields = the number of its fields
static int format_key_index(const char* b, const char* const e, const char* key, int* n_fields = nullptr) {
    const size_t kl = strlen(key);
    int k = 0, found = -1;
    for (const char* q = b;; q++)
        if (q == e || *q == ':') {
            if ((size_t)(q - b) == kl && !memcmp(b, key, kl) && found < 0) found = k;
            k++;
            if (q == e) break;
            b = q + 1;
        }
    if (n_fields) *n_fields = k;
    return found;
}

// bytes of one value of a BCF typed vector (0: no such type)
static inline int bcf_type_width(const int ty) { return ty == 1 ? 1 : ty == 2 ? 2 : (ty == 3 || ty == 5) ? 4 : ty == 7 ? 1 : 0; }

// the n_fmt FORMAT fields of the BCF record at the cursor, N samples: f(k, key, type, n, data_off) for field k, whose N vectors of n
// values of `type` lie from byte data_off of the file; the cursor is left behind the last field.  A key outside the dictionary and a
// field that runs past the file's end stop the program.  file_at < 0: the cursor is over the file.  file_at >= 0: the cursor is over
// the fields' keys and descriptors alone, back to back (the head of a resident record, resident_file.h), the first of which lies at
// byte file_at of the file: data_off is then file_at + the header bytes so far + the data bytes of the fields before
template <typename F> static void bcf_format_fields(BcfIn& c, const BcfDict& d, const int n_fmt, const size_t N, F f, const int64_t file_at = -1) {
    std::vector<int32_t> iv; int ty, n;
    const size_t first = c.off; size_t data_before = 0;
    for (int k = 0; k < n_fmt; k++) {
        c.typed(ty, n); c.ints(ty, n, iv);
        const auto key = iv.empty() ? d.dict.end() : d.dict.find(iv[0]);
        if (key == d.dict.end()) c.fail("BCF: undefined FORMAT key");
        c.typed(ty, n);
        const size_t bytes = (size_t)bcf_type_width(ty) * n * N;
        if (file_at >= 0) { f(k, key->second, ty, n, (size_t)file_at + (c.off - first) + data_before); data_before += bytes; continue; }
        if (c.off + bytes > c.size) c.fail("truncated BCF record");
        f(k, key->second, ty, n, c.off);
        c.off += bytes;
    }
}

// the value v of option a: an integer in lo .. hi
static int option_int(const char* a, const char* v, const int lo, const int hi) {
    char* e; const long x = strtol(v, &e, 10);
    if (e == v || *e || x < lo || x > hi) die("%s takes an integer in %d .. %d, not '%s'", a, lo, hi, v);
    return (int)x;
}
