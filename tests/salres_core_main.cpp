// salres_core_main.cpp -- the rules by which setalleles_hip --resident 1 assembles its output records (vcfgl_amd/csrc/misc/salres_core.h:
// what k_salres_plan and k_salres_write run) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer.
//   salres_core_main records IN.bcf WANT.bcf N GL PL GP
//       IN: a raw BCF file; WANT: what setalleles_hip --on-device 0 -O u made of it (put_record_bcf's bytes); N samples; the dictionary
//       ids of GL, PL and GP.  Per record the piece table is built from the record's head (rb::format_walk over IN, table_field), the
//       new shared block and the planes are taken out of WANT's record, and the planned length and the bytes write_record makes -- lane
//       by lane, at 1, 64 and 256 lanes, the output and the file shifted through all 16 residues mod 16 -- must be WANT's record.
//       IN, the planes, the shared bytes and the output live in heap blocks of exactly their length; the last record ends at IN's last byte.
//   salres_core_main runs
//       copy_run over source and destination residues 0 .. 15 and runs of 0, 1, 15, 16, 17 and 4099 bytes, the source's run ending at
//       the end of its block (and once more with 40 bytes behind it: the path of two aligned loads), the destination a block of exactly
//       d + n bytes whose first d bytes must stay as they were
// Prints "ok <count>" and returns 0, or says what differs and returns 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "misc/salres_core.h"
#include "misc/rb_core.h"

namespace {

[[noreturn]] void bad(const char* what, long a = 0, long b = 0) { printf("MISMATCH %s %ld %ld\n", what, a, b); exit(1); }

std::vector<uint8_t> slurp(const char* fn) {
    FILE* fp = fopen(fn, "rb");
    if (!fp) bad("open");
    std::vector<uint8_t> v; uint8_t buf[1 << 16]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(fp);
    return v;
}

// a heap block of exactly n bytes (n = 0: one byte that is never touched)
struct Block {
    uint8_t* p; size_t n;
    explicit Block(size_t n_) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) {}
    Block(const Block&) = delete;
    ~Block() { free(p); }
};

struct Field { int64_t at, key_end, data, end; int32_t key, type; int64_t n; };
struct Record { int64_t at, end; uint32_t l_shared; std::vector<Field> fields; };

std::vector<Record> walk(const std::vector<uint8_t>& file, const int64_t N) {
    const int64_t total = (int64_t)file.size();
    if (total < 9 || memcmp(file.data(), "BCF\2", 4) != 0) bad("header");
    std::vector<Record> out;
    for (int64_t o = 9 + (int64_t)rb::rd_u32(file.data(), 5); o < total;) {
        Record r; r.at = o;
        int64_t head_len;
        const int st = rb::format_walk(file.data(), total, o, N, rf::RF_HEAD_MOST, head_len, [&](int, int64_t hdr_at, int64_t hdr_len, int32_t key, int32_t type, int64_t n, int64_t data_off) {
            const rb::Typed k = rb::typed_at(file.data(), hdr_at, total);
            r.fields.push_back(Field{hdr_at, hdr_at + k.len + k.n * rb::int_width(k.type), data_off, data_off + (int64_t)rb::type_width(type) * n * N, key, type, n});
        });
        if (st != rb::OK) bad("walk", (long)out.size(), st);
        uint32_t l_shared; int64_t rec_end;
        rb::record_step(file.data(), total, o, l_shared, rec_end);
        r.l_shared = l_shared; r.end = rec_end;
        out.push_back(r);
        o = rec_end;
    }
    return out;
}

int records(int argc, char** argv) {
    if (argc != 8) bad("usage");
    const std::vector<uint8_t> in_v = slurp(argv[2]), want = slurp(argv[3]);
    const int64_t N = atoll(argv[4]);
    const int key_of[sal::NF] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
    const std::vector<Record> ri = walk(in_v, N), rw = walk(want, N);
    if (ri.size() != rw.size()) bad("record count", (long)ri.size(), (long)rw.size());
    if (!ri.empty() && ri.back().end != (int64_t)in_v.size()) bad("the last record does not end the file");
    long n_checked = 0, n_touched = 0;
    for (int res = 0; res < 16; res++) {
        const int shift = (res * 7) & 15;                              // the file's own shift: `shift` bytes in front of it
        Block file((size_t)shift + in_v.size());
        memset(file.p, 0xEE, (size_t)shift); memcpy(file.p + shift, in_v.data(), in_v.size());
        for (size_t i = 0; i < ri.size(); i++) {
            const Record& a = ri[i]; const Record& w = rw[i];
            // the piece table from the head, by the program's rule: the first field of a tag that has values is touched
            salres::Desc d;
            sal::BRec r; memset(&r, 0, sizeof r);
            int pl_width = 4;
            salres::table_begin(d, shift + (a.fields.empty() ? a.end : a.fields[0].at));
            std::vector<int> f_of(a.fields.size(), -1);
            for (size_t k = 0; k < a.fields.size(); k++) {
                const Field& fd = a.fields[k];
                int f = -1;
                for (int t = 0; t < sal::NF; t++) if (fd.key == key_of[t] && fd.n > 0 && r.nv[t] == 0) f = t;
                if (f >= 0) { r.nv[f] = (int32_t)fd.n; r.ty[f] = (int8_t)fd.type; }
                f_of[k] = f;
                if (!salres::table_field(d, shift + fd.at, shift + fd.key_end, shift + fd.end, f)) bad("a fourth touched field", (long)i);
            }
            if (a.fields.size() != w.fields.size()) bad("field count", (long)i);
            // what the relabelling stage and the host hand the writer: the planes and the new shared block, out of WANT's record
            int n_new_g = 1, n_old_g = 1;
            for (size_t k = 0; k < a.fields.size(); k++) if (f_of[k] >= 0) { n_new_g = (int)w.fields[k].n; if (a.fields[k].n > n_old_g) n_old_g = (int)a.fields[k].n; }
            r.n_new_g = (int8_t)n_new_g; r.n_old_g = (int8_t)n_old_g;
            for (int h = 0; h < n_new_g; h++) r.n2o |= (uint64_t)1 << (4 * h);
            const int64_t lead = 5;                                    // plane words of another record in front
            r.plane_off = lead;
            const int64_t vals = lead + sal::b_plane_vals(r, N);
            Block planes((size_t)vals * 4);
            memset(planes.p, 0xDD, planes.n);
            for (size_t k = 0; k < a.fields.size(); k++) {
                const int f = f_of[k];
                if (f < 0) continue;
                n_touched++;
                const Field& fw = w.fields[k];
                if (f == sal::F_PL) pl_width = rb::type_width(fw.type);
                else if (fw.type != 5) bad("a float field's type", (long)i);
                memcpy(planes.p + (r.plane_off + (int64_t)sal::b_slot(r, f) * n_new_g * N) * 4, want.data() + fw.data, (size_t)(fw.end - fw.data));
            }
            const int64_t sh_lead = 3;
            Block shared((size_t)(sh_lead + w.l_shared));
            memset(shared.p, 0xCC, (size_t)sh_lead); memcpy(shared.p + sh_lead, want.data() + w.at + 8, w.l_shared);
            d.shared_off = sh_lead; d.shared_len = (int32_t)w.l_shared;
            const salres::Sources S{file.p, (int64_t)file.n, shared.p, (int64_t)shared.n, planes.p, vals};
            if (!salres::check(d, r, N, pl_width, S)) bad("check", (long)i);
            const int64_t len = salres::record_len(d, r, N, pl_width);
            if (len != w.end - w.at) bad("planned length", (long)len, (long)(w.end - w.at));
            for (const int n_lanes : {1, 64, 256}) {
                Block out((size_t)(res + len));
                memset(out.p, 0xAB, out.n);
                for (int lane = 0; lane < n_lanes; lane++)
                    if (!salres::write_record(out.p, res, res + len, d, r, N, pl_width, S, lane, n_lanes)) bad("write_record refused", (long)i);
                for (int j = 0; j < res; j++) if (out.p[j] != 0xAB) bad("a byte in front of the record", (long)i, j);
                if (memcmp(out.p + res, want.data() + w.at, (size_t)len) != 0) {
                    int64_t j = 0; while (out.p[res + j] == want[(size_t)(w.at + j)]) j++;
                    bad("record bytes", (long)i, (long)j);
                }
                n_checked++;
            }
            // a descriptor that does not hold is refused and nothing is written
            {
                Block out((size_t)len); memset(out.p, 0xAB, out.n);
                salres::Desc e = d; e.run_len[0] += 1;
                bool refused = !salres::write_record(out.p, 0, len, e, r, N, pl_width, S, 0, 1);
                e = d; e.run_off[d.n_touched] = (int64_t)file.n; e.run_len[d.n_touched] = 1;
                refused = refused && !salres::write_record(out.p, 0, len + 1, e, r, N, pl_width, S, 0, 1);
                e = d; e.shared_off = (int64_t)shared.n - e.shared_len + 1;
                refused = refused && !salres::write_record(out.p, 0, len, e, r, N, pl_width, S, 0, 1);
                if (d.n_touched > 0) { sal::BRec q = r; q.plane_off = vals; refused = refused && !salres::write_record(out.p, 0, len, d, q, N, pl_width, S, 0, 1); }
                for (size_t j = 0; j < out.n; j++) if (out.p[j] != 0xAB) bad("a refused record was written", (long)i);
                if (!refused) bad("a descriptor that does not hold was taken", (long)i);
            }
        }
    }
    printf("ok %ld records %zu touched %ld\n", n_checked, ri.size(), n_touched / 16);
    return 0;
}

int runs() {
    long n_checked = 0;
    const int64_t lens[] = {0, 1, 15, 16, 17, 4099};
    for (const int64_t n : lens)
        for (int s = 0; s < 16; s++)
            for (int d = 0; d < 16; d++)
                for (const int behind : {0, 40})
                    for (const int n_lanes : {1, 64, 256}) {
                        Block src((size_t)(s + n + behind)), dst((size_t)(d + n));
                        for (size_t j = 0; j < src.n; j++) src.p[j] = (uint8_t)(j * 131 + 7 * s + 1);
                        memset(dst.p, 0xAB, dst.n);
                        for (int lane = 0; lane < n_lanes; lane++) salres::copy_run(dst.p, d, src.p, s, (int64_t)src.n, n, lane, n_lanes);
                        for (int j = 0; j < d; j++) if (dst.p[j] != 0xAB) bad("a byte in front of the run", (long)n, j);
                        if (n && memcmp(dst.p + d, src.p + s, (size_t)n) != 0) bad("run bytes", (long)n, s * 16 + d);
                        n_checked++;
                    }
    printf("ok %ld\n", n_checked);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "records")) return records(argc, argv);
    if (argc == 2 && !strcmp(argv[1], "runs")) return runs();
    bad("usage");
}
