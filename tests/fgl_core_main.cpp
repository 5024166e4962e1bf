// fgl_core_main.cpp -- the rules of vcfgl_amd/csrc/misc/fgl_core.h on the host, for the sanitizers (tests/test_fgl_core_cpu.py).
//   fgl_core_main CASES OUT
// CASES: one case a line, fields separated by one blank, text as hexadecimal digits ("-" for none):
//   P TOKEN            fgl::parse_token on a region of exactly the token's length; a token it takes (other than ".") is also given to
//                      strtod and cast to float: the bits must be equal
//   R N k g REGION     fgl::record_plain on a region of exactly the text's length
//   V bits             fgl::put_value into an allocation of exactly fgl::value_len bytes
// OUT: one line a case: P "host" | "ok BITS" | "MISMATCH BITS STRTOD"; R "host" | "range N_GLS" | "ok N_GLS BITS..."; V the text.
// Every region is a heap block of its own with no byte to spare: a read at or past its end is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "misc/fgl_core.h"

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
    std::vector<char> line(1 << 20), a(1 << 20);
    long cases = 0, taken = 0; unsigned longest = 0;
    while (fgets(line.data(), (int)line.size(), in)) {
        cases++;
        int N = 0, k = 0, g = 0; unsigned bits = 0;
        if (line[0] == 'P' && sscanf(line.data(), "P %s", a.data()) == 1) {
            const std::vector<uint8_t> v = unhex(a.data());
            uint8_t* p = exact(v); uint32_t b = 0;
            if (!fgl::parse_token(p, 0, (int64_t)v.size(), b)) fprintf(out, "host\n");
            else {
                taken++;
                const std::string tok(v.begin(), v.end());
                uint32_t want = b;
                if (tok != ".") {
                    char* e = nullptr;
                    const double d = strtod(tok.c_str(), &e);
                    if (e != tok.c_str() + tok.size()) return 3;              // the grammar took what strtod does not take whole
                    const float f = (float)d;
                    memcpy(&want, &f, 4);
                }
                if (want == b) fprintf(out, "ok %08x\n", b); else fprintf(out, "MISMATCH %08x %08x\n", b, want);
            }
            free(p);
        } else if (line[0] == 'R' && sscanf(line.data(), "R %d %d %d %s", &N, &k, &g, a.data()) == 4) {
            const std::vector<uint8_t> v = unhex(a.data());
            uint8_t* p = exact(v);
            fgl::Rec r; memset(&r, 0, sizeof r);
            r.off = 0; r.len = (int32_t)v.size(); r.k = k; r.g = g; r.pos = 1;
            uint32_t* plane = (uint32_t*)malloc(4 * (size_t)N + 4);
            int32_t n_gls = 0;
            const int st = fgl::record_plain(p, r, N, plane, &n_gls);
            if (st == fgl::ST_HOST) fprintf(out, "host\n");
            else if (st == fgl::ST_RANGE) fprintf(out, "range %d\n", n_gls);
            else { fprintf(out, "ok %d", n_gls); for (int s = 0; s < N; s++) fprintf(out, " %08x", plane[s]); fprintf(out, "\n"); }
            free(plane); free(p);
        } else if (line[0] == 'V' && sscanf(line.data(), "V %x", &bits) == 1) {
            const uint32_t n = fgl::value_len(bits);
            if (n > (unsigned)fgl::VALUE_BOUND) return 4;
            if (n > longest) longest = n;
            uint8_t* p = (uint8_t*)malloc(n);
            vgl_fetchgl::Emit<true> e{p, 0u, n};
            fgl::put_value(e, bits, true);
            if (e.n != n) return 5;
            fwrite(p, 1, n, out);                                              // (ends in '\n')
            free(p);
        } else return 6;
    }
    fclose(in); fclose(out);
    printf("cases %ld taken %ld longest %u\n", cases, taken, longest);
    return 0;
}
