// sal_core_main.cpp -- the rules of setalleles_hip (vcfgl_amd/csrc/misc/sal_core.h) as a host program of its own, built with
// -fsanitize=address,undefined by tests/test_sal_core_cpu.py.  Every text lies in a heap block of exactly its length.
//   sal_core_main cases.txt out.txt       one case per line, one result line per case:
//   P <hex token>                         sal::parse_pl_token -> the int32, or "host"; compared here with strtol ("MISMATCH ..." if they differ)
//   N <field> <n> <hex bits> ...          norm_flt / norm_pl of one sample's n values -> the new bits, or "over"
//   W <min> <max>                         int_width
//   B <field> <type> <nv> <n_new_g> <hex n2o> <hex vector>
//                                         bcf_sample on one sample's old BCF vector (a block of exactly nv values) -> the new bits, or "over";
//                                         then store_narrow at every width into blocks of exactly n_new_g values, read back widened
//   R <N> <kGL> <kPL> <kGP> <n_old_g> <n_new_g> <hex o2n> <hex region>
//                                         record_plain by the grammar reader, then norm_sample: "status cols" and, for status 0, the planes
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "misc/sal_core.h"

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> b;
    if (h == "-") return b;
    for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return b;
}

// the bytes in a heap block of exactly their length (a zero-length block is still a block)
struct Exact {
    uint8_t* p; size_t n;
    explicit Exact(const std::vector<uint8_t>& b) : p((uint8_t*)malloc(b.size() ? b.size() : 1)), n(b.size()) { if (n) memcpy(p, b.data(), n); }
    ~Exact() { free(p); }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    std::string line; long cases = 0; int c;
    auto next_line = [&]() { line.clear(); while ((c = fgetc(in)) != EOF && c != '\n') line += (char)c; return c != EOF || !line.empty(); };
    while (next_line()) {
        std::istringstream ss(line);
        std::string kind; ss >> kind;
        cases++;
        if (kind == "P") {
            std::string h; ss >> h;
            const std::vector<uint8_t> tok = unhex(h);
            Exact x(tok);
            uint32_t bits = 0;
            const bool ok = sal::parse_pl_token(x.p, 0, (int64_t)x.n, bits);
            if (!ok) { fprintf(out, "host\n"); continue; }
            const std::string s(tok.begin(), tok.end());
            long long want;
            if (s == ".") want = INT32_MIN;
            else { char* e; errno = 0; want = strtoll(s.c_str(), &e, 10); if (*e || errno) { fprintf(out, "MISMATCH strtol refuses\n"); continue; } }
            if (want != (long long)(int32_t)bits) fprintf(out, "MISMATCH %lld\n", want); else fprintf(out, "%d\n", (int32_t)bits);
        } else if (kind == "N") {
            int f, n; ss >> f >> n;
            uint32_t* v = (uint32_t*)malloc(sizeof(uint32_t) * sal::MAX_G);     // (norm_* touch v[g] for g < n only)
            for (int g = 0; g < sal::MAX_G; g++) v[g] = 0xDEADBEEFu;
            for (int g = 0; g < n; g++) { std::string h; ss >> h; v[g] = (uint32_t)strtoul(h.c_str(), nullptr, 16); }
            bool over = false;
            if (f == sal::F_PL) over = sal::norm_pl(v, n); else sal::norm_flt(v, n, f == sal::F_GP);
            bool clean = true;
            for (int g = n; g < sal::MAX_G; g++) clean = clean && v[g] == 0xDEADBEEFu;
            if (!clean) fprintf(out, "MISMATCH touched behind n\n");
            else if (over) fprintf(out, "over\n");
            else { for (int g = 0; g < n; g++) fprintf(out, "%s%08x", g ? " " : "", v[g]); fprintf(out, "\n"); }
            free(v);
        } else if (kind == "W") {
            long long mn, mx; ss >> mn >> mx;
            fprintf(out, "%d\n", sal::int_width((int32_t)mn, (int32_t)mx));
        } else if (kind == "B") {
            int f, ty, nv, nn; std::string ho, hv;
            ss >> f >> ty >> nv >> nn >> ho >> hv;
            Exact x(unhex(hv));
            if ((size_t)nv * (size_t)sal::type_width(ty) != x.n) { fprintf(out, "MISMATCH vector length\n"); continue; }
            uint32_t v[sal::MAX_G];
            const bool over = sal::bcf_sample(x.p, ty, nv, strtoull(ho.c_str(), nullptr, 16), nn, f, v);
            if (over) { fprintf(out, "over\n"); continue; }
            bool same = true;
            if (f == sal::F_PL)
                for (int w = 1; w <= 4; w <<= 1) {
                    int32_t mn = INT32_MAX, mx = INT32_MIN + 1;
                    for (int h = 0; h < nn; h++) if (v[h] != sal::I_MISSING && v[h] != sal::I_END) { if ((int32_t)v[h] < mn) mn = (int32_t)v[h]; if ((int32_t)v[h] > mx) mx = (int32_t)v[h]; }
                    if (w < sal::int_width(mn, mx)) continue;
                    uint8_t* b = (uint8_t*)malloc((size_t)nn * w);
                    for (int h = 0; h < nn; h++) sal::store_narrow(b, w, h, v[h]);
                    for (int h = 0; h < nn; h++) same = same && sal::bcf_load(b, w == 1 ? 1 : w == 2 ? 2 : 3, h) == v[h];
                    free(b);
                }
            if (!same) { fprintf(out, "MISMATCH narrowing\n"); continue; }
            for (int h = 0; h < nn; h++) fprintf(out, "%s%08x", h ? " " : "", v[h]);
            fprintf(out, "\n");
        } else if (kind == "R") {
            long long N; int k0, k1, k2, no, nn; std::string ho, hr;
            ss >> N >> k0 >> k1 >> k2 >> no >> nn >> ho >> hr;
            Exact x(unhex(hr));
            sal::Rec r{0, 0, strtoull(ho.c_str(), nullptr, 16), (int32_t)x.n, {(int16_t)k0, (int16_t)k1, (int16_t)k2}, (int8_t)no, (int8_t)nn};
            if (!sal::rec_sane(r)) { fprintf(out, "insane\n"); continue; }
            const size_t vals = (size_t)sal::plane_vals(r, N);
            uint32_t* planes = (uint32_t*)malloc(sizeof(uint32_t) * (vals ? vals : 1));
            for (size_t i = 0; i < vals; i++) planes[i] = 0xDEADBEEFu;
            sal::GrammarReader rd; int64_t cols = 0;
            int st = sal::record_plain(x.p, r, N, rd, planes, &cols);
            if (st == sal::ST_OK)
                for (int f = 0; f < sal::NF; f++)
                    if (r.k[f] >= 0)
                        for (int64_t s = 0; s < N; s++)
                            if (sal::norm_sample(planes + (int64_t)sal::field_slot(r, f) * r.n_new_g * N, N, s, r.n_new_g, f)) st = sal::ST_RANGE;
            fprintf(out, "%d %lld", st, (long long)cols);
            if (st == sal::ST_OK) for (size_t i = 0; i < vals; i++) fprintf(out, " %08x", planes[i]);
            fprintf(out, "\n");
            free(planes);
        } else { fprintf(out, "?\n"); }
    }
    fclose(in); fclose(out);
    printf("cases %ld\n", cases);
    return 0;
}
