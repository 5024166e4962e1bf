// gtdbcf_core_main.cpp -- the rules of vcfgl_amd/csrc/misc/gtdbcf_core.h on the host, for the sanitizers (tests/test_gtdbcf_core_cpu.py).
//   gtdbcf_core_main CASES OUT
// CASES: one case a line, fields separated by one blank, bytes as hexadecimal digits ("-" for none); a vector is TYPE N_VALUES BYTES,
// type 0 for an absent field:
//   T N s nal map  GT                       gtd::bcf_sample_true of sample s of N
//   C N s gq_mode nal map  GT GQ PL         gtd::bcf_sample_call likewise
//   S call N gq_mode nal map n_bytes  gt_off gt_type gt_n  gq_off gq_type gq_n  pl_off pl_type pl_n  BYTES
//                                           gtd::bcf_side_plain on one block of exactly BYTES, told that it has n_bytes bytes
// OUT: one line a case: "host", or "ok tb", "ok cb gq", "ok" and the planes in hex.
// Every vector of T and C is a heap block of its own with no byte to spare (the descriptor's offsets are the distances of the GQ and PL
// blocks from the GT block): a read before or past a vector is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "misc/gtdbcf_core.h"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (!strcmp(s, "-")) return out;
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (; s[0] && s[1]; s += 2) out.push_back((uint8_t)(nib(s[0]) << 4 | nib(s[1])));
    return out;
}
static uint8_t* exact(const std::vector<uint8_t>& v) {
    uint8_t* p = (uint8_t*)malloc(v.empty() ? 1 : v.size());
    if (!v.empty()) memcpy(p, v.data(), v.size());
    return p;
}
static void hex(FILE* f, const std::vector<uint8_t>& v) { for (uint8_t x : v) fprintf(f, "%02x", x); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    std::vector<char> line(1 << 20), a(1 << 20), b(1 << 20), c(1 << 20);
    long cases = 0;
    while (fgets(line.data(), (int)line.size(), in)) {
        cases++;
        gtd::BSide B; memset(&B, 0, sizeof B);
        unsigned long long map = 0; long long N = 0, s = 0, n_bytes = 0, o0 = 0, o1 = 0, o2 = 0;
        int mode = 0, call = 0;
        if (line[0] == 'T' && sscanf(line.data(), "T %lld %lld %d %llx %d %d %s", &N, &s, &B.nal, &map, &B.gt_type, &B.gt_n, a.data()) == 7) {
            B.map = map; B.have = gtd::B_GT;
            const std::vector<uint8_t> v = unhex(a.data());
            if ((long long)v.size() != N * B.gt_n * gtd::bcf_width(B.gt_type)) return 3;
            uint8_t* p = exact(v); uint32_t tb = 0;
            if (gtd::bcf_sample_true(p, B, s, tb)) fprintf(out, "ok %u\n", tb); else fprintf(out, "host\n");
            free(p);
        } else if (line[0] == 'C' && sscanf(line.data(), "C %lld %lld %d %d %llx %d %d %s %d %d %s %d %d %s", &N, &s, &mode, &B.nal, &map, &B.gt_type, &B.gt_n, a.data(),
                                            &B.gq_type, &B.gq_n, b.data(), &B.pl_type, &B.pl_n, c.data()) == 14) {
            B.map = map; B.have = gtd::B_GT | (B.gq_type ? gtd::B_GQ : 0) | (B.pl_type ? gtd::B_PL : 0);
            const std::vector<uint8_t> v = unhex(a.data()), q = unhex(b.data()), l = unhex(c.data());
            if ((long long)v.size() != N * B.gt_n * gtd::bcf_width(B.gt_type) || (long long)q.size() != N * B.gq_n * gtd::bcf_width(B.gq_type) ||
                (long long)l.size() != N * B.pl_n * gtd::bcf_width(B.pl_type)) return 3;
            uint8_t* p = exact(v); uint8_t* pq = exact(q); uint8_t* pl = exact(l);
            B.gq_off = (int64_t)((intptr_t)pq - (intptr_t)p); B.pl_off = (int64_t)((intptr_t)pl - (intptr_t)p);
            uint32_t cb = 0, g = 0;
            if (gtd::bcf_sample_call(p, B, s, mode, gtd::n_genotypes(B.nal), cb, g)) fprintf(out, "ok %u %u\n", cb, g); else fprintf(out, "host\n");
            free(p); free(pq); free(pl);
        } else if (line[0] == 'S' && sscanf(line.data(), "S %d %lld %d %d %llx %lld %lld %d %d %lld %d %d %lld %d %d %s", &call, &N, &mode, &B.nal, &map, &n_bytes, &o0, &B.gt_type, &B.gt_n,
                                            &o1, &B.gq_type, &B.gq_n, &o2, &B.pl_type, &B.pl_n, a.data()) == 16) {
            B.map = map; B.have = gtd::B_GT | (B.gq_type ? gtd::B_GQ : 0) | (B.pl_type ? gtd::B_PL : 0);
            B.gt_off = o0; B.gq_off = o1; B.pl_off = o2;
            const std::vector<uint8_t> v = unhex(a.data());
            uint8_t* p = exact(v);
            std::vector<uint8_t> tb((size_t)N), cb((size_t)N), gq((size_t)N);
            if (gtd::bcf_side_plain(p, n_bytes, B, call != 0, mode, gtd::n_genotypes(B.nal), N, tb.data(), cb.data(), gq.data()) != gtd::ST_OK) fprintf(out, "host\n");
            else { fprintf(out, "ok "); if (call) { hex(out, cb); fprintf(out, " "); hex(out, gq); } else hex(out, tb); fprintf(out, "\n"); }
            free(p);
        } else return 3;
    }
    fclose(out); fclose(in);
    printf("cases %ld\n", cases);
    return 0;
}
