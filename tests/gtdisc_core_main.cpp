// gtdisc_core_main.cpp -- the rules of vcfgl_amd/csrc/misc/gtdisc_core.h on the host, for the sanitizers (tests/test_gtdisc_core_cpu.py).
//   gtdisc_core_main CASES OUT
// CASES: one case a line, fields separated by one blank, text as hexadecimal digits ("-" for none):
//   T t_gti t_nal t_map TEXT                            gtd::sample_true on a region of exactly the text's length
//   C c_gti c_gqi c_pli c_nal c_map gq_mode TEXT         gtd::sample_call likewise
//   R N t_gti t_nal t_map c_gti c_gqi c_pli c_nal c_map gq_mode TRUTH CALL   gtd::record_plain on two regions of exactly their lengths
//   L list nsites1 i cell gq pos                         the listing line and the per-site line, each into an allocation of exactly its
//                                                        planned size
// OUT: one line a case: "host", or the values ("ok tb", "ok cb gq", "ok" and the three planes in hex, the two lines).
// Every region is a heap block of its own with no byte to spare: a read at or past its end is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "misc/gtdisc_core.h"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (!strcmp(s, "-")) return out;
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (; s[0] && s[1]; s += 2) out.push_back((uint8_t)(nib(s[0]) << 4 | nib(s[1])));
    return out;
}
// a heap block of exactly the bytes (one byte for none: its address is never read)
static uint8_t* exact(const std::vector<uint8_t>& v) {
    uint8_t* p = (uint8_t*)malloc(v.empty() ? 1 : v.size());
    if (!v.empty()) memcpy(p, v.data(), v.size());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    std::vector<char> line(1 << 20), a(1 << 20), b(1 << 20);
    long cases = 0; unsigned longest = 0;
    while (fgets(line.data(), (int)line.size(), in)) {
        cases++;
        gtd::Rec r; memset(&r, 0, sizeof r);
        unsigned long long tm = 0, cm = 0; long long pos = 0;
        int N = 0, list = 0, nsites1 = 0, i = 0, cell = 0, gq = 0;
        if (line[0] == 'T' && sscanf(line.data(), "T %d %d %llx %s", &r.t_gti, &r.t_nal, &tm, a.data()) == 4) {
            r.t_map = tm;
            const std::vector<uint8_t> v = unhex(a.data());
            uint8_t* p = exact(v); uint32_t tb = 0;
            if (gtd::sample_true(p, 0, (int64_t)v.size(), r, tb)) fprintf(out, "ok %u\n", tb); else fprintf(out, "host\n");
            free(p);
        } else if (line[0] == 'C' && sscanf(line.data(), "C %d %d %d %d %llx %d %s", &r.c_gti, &r.c_gqi, &r.c_pli, &r.c_nal, &cm, &r.gq_mode, a.data()) == 7) {
            r.c_map = cm; r.nG = gtd::n_genotypes(r.c_nal);
            const std::vector<uint8_t> v = unhex(a.data());
            uint8_t* p = exact(v); uint32_t cb = 0, g = 0;
            if (gtd::sample_call(p, 0, (int64_t)v.size(), r, cb, g)) fprintf(out, "ok %u %u\n", cb, g); else fprintf(out, "host\n");
            free(p);
        } else if (line[0] == 'R' && sscanf(line.data(), "R %d %d %d %llx %d %d %d %d %llx %d %s %s", &N, &r.t_gti, &r.t_nal, &tm, &r.c_gti, &r.c_gqi, &r.c_pli,
                                            &r.c_nal, &cm, &r.gq_mode, a.data(), b.data()) == 12) {
            r.t_map = tm; r.c_map = cm; r.nG = gtd::n_genotypes(r.c_nal);
            const std::vector<uint8_t> tv = unhex(a.data()), cv = unhex(b.data());
            uint8_t* tp = exact(tv); uint8_t* cp = exact(cv);
            r.t_off = 0; r.t_len = (int32_t)tv.size(); r.c_off = 0; r.c_len = (int32_t)cv.size();
            uint8_t* planes = (uint8_t*)malloc(3 * (size_t)N + 1);
            if (gtd::record_plain(tp, cp, r, N, planes, planes + N, planes + 2 * N) != gtd::ST_OK) fprintf(out, "host\n");
            else { fprintf(out, "ok "); for (int k = 0; k < 3 * N; k++) fprintf(out, "%02x", planes[k]); fprintf(out, "\n"); }
            free(planes); free(tp); free(cp);
        } else if (line[0] == 'L' && sscanf(line.data(), "L %d %d %d %d %d %lld", &list, &nsites1, &i, &cell, &gq, &pos) == 6) {
            const uint32_t n0 = gtd::list_len(list, nsites1, (uint32_t)i, (uint32_t)cell, (uint32_t)gq), n1 = gtd::site_len(pos, (uint32_t)i, (uint32_t)cell);
            if (n0 > (unsigned)gtd::LINE_BOUND || n1 > (unsigned)gtd::LINE_BOUND) return 3;
            if (n0 > longest) longest = n0;
            if (n1 > longest) longest = n1;
            uint8_t* p0 = (uint8_t*)malloc(n0); uint8_t* p1 = (uint8_t*)malloc(n1);
            gtd::Emit<true> e0{p0, 0u, n0}, e1{p1, 0u, n1};
            gtd::list_line(e0, list, nsites1, (uint32_t)i, (uint32_t)cell, (uint32_t)gq);
            gtd::site_line(e1, pos, (uint32_t)i, (uint32_t)cell);
            if (e0.n != n0 || e1.n != n1) return 4;
            fwrite(p0, 1, n0 - 1, out); fputc('|', out); fwrite(p1, 1, n1, out);      // (the listing line's '\n' becomes '|': one output line a case)
            free(p0); free(p1);
        } else return 5;
    }
    fclose(in); fclose(out);
    printf("cases %ld longest %u\n", cases, longest);
    return 0;
}
