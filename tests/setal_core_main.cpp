// setal_core_main.cpp -- vgl_setal_core.h on the host, for the sanitizers (tests/test_setal_core_cpu.py).
// Every (old allele list, target list) of 2 .. 5 distinct alleles out of A, C, G, T, <*> in every order: the header's maps and plan
// against a second, straightforward implementation written the way the tool is (search the list, scatter, loop), and the per-sample
// routines on values gathered through the plan against the same values scattered through the straightforward map.
// Special samples: missing ones, -inf entries, all kept genotypes -inf, one-byte PL 255, a GP sum whose float order matters.
// Prints "pairs <n> subsets <n> refused <n> samples <n>"; exits 1 with a message at the first difference.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vgl_setal_core.h"

namespace sa = vgl_setal;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

static void die(const char* what, const std::vector<int>& o, const std::vector<int>& t) {
    fprintf(stderr, "%s: old", what);
    for (int x : o) fprintf(stderr, " %d", x);
    fprintf(stderr, " target");
    for (int x : t) fprintf(stderr, " %d", x);
    fprintf(stderr, "\n");
    exit(1);
}

// ---- the straightforward side ------------------------------------------------------------------------------------------------------
static int ref_gt(int a, int b) { if (a > b) { int x = a; a = b; b = x; } return b * (b + 1) / 2 + a; }
static void ref_maps(const std::vector<int>& o, const std::vector<int>& t, int* o2n, int* g2g) {
    for (size_t a = 0; a < o.size(); a++) { o2n[a] = -1; for (size_t j = 0; j < t.size(); j++) if (t[j] == o[a]) { o2n[a] = (int)j; break; } }
    for (int g = 0; g < 15; g++) g2g[g] = -1;
    for (int a2 = 0, g = 0; a2 < (int)o.size(); a2++)
        for (int a1 = 0; a1 <= a2; a1++, g++)
            if (o2n[a1] != -1 && o2n[a2] != -1) g2g[g] = ref_gt(o2n[a1], o2n[a2]);
}
static bool bits_nan(uint32_t b) { float f; memcpy(&f, &b, 4); return f != f; }
static void ref_gl(std::vector<uint32_t>& v) {
    for (uint32_t b : v) if (bits_nan(b)) return;
    float mx = -INFINITY;
    for (uint32_t b : v) { float f; memcpy(&f, &b, 4); if (f > mx) mx = f; }
    for (uint32_t& b : v) { float f; memcpy(&f, &b, 4); f -= mx; memcpy(&b, &f, 4); }
}
static void ref_pl(std::vector<uint32_t>& v) {
    for (uint32_t b : v) if ((int32_t)b == INT32_MIN) return;
    float mn = INFINITY;
    for (uint32_t b : v) if ((float)(int32_t)b < mn) mn = (float)(int32_t)b;
    for (uint32_t& b : v) { const float t = (float)(int32_t)b - mn; b = (uint32_t)(int32_t)t; }
}
static void ref_gp(std::vector<uint32_t>& v) {
    for (uint32_t b : v) if (bits_nan(b)) return;
    volatile float sum = 0.0f;
    for (uint32_t b : v) { float f; memcpy(&f, &b, 4); sum = sum + f; }
    for (uint32_t& b : v) { float f; memcpy(&f, &b, 4); volatile float q = f / sum; f = q; memcpy(&b, &f, 4); }
}
static void ref_u8(std::vector<uint32_t>& v, bool missing) {
    if (missing) return;
    uint32_t mn = v[0];
    for (uint32_t b : v) if (b < mn) mn = b;
    for (uint32_t& b : v) b -= mn;
}

// both bit patterns equal, or both NaN results of arithmetic (the sign of an invalid operation's NaN is the machine's)
static bool same(uint32_t a, uint32_t b) { return a == b || (bits_nan(a) && bits_nan(b) && (a & 0x7FFFFFFFu) == (b & 0x7FFFFFFFu)); }

static long n_samples_done = 0;
// one sample through both sides: old values `ov` (nGo of them) of kind k (0 GL, 1 PL, 2 GP, 3 one-byte PL)
static void sample(const sa::SitePlan& P, const int* g2g, int nGo, int nGn, const uint32_t* ov, int k, bool u8_missing,
                   const std::vector<int>& o, const std::vector<int>& t) {
    uint32_t v[sa::MAX_G];
    for (int h = 0; h < sa::MAX_G; h++) v[h] = h < nGn ? ov[P.new2old[h]] : 0xDEADBEEFu;
    if (k == 0) sa::norm_gl(v, nGn); else if (k == 1) sa::norm_pl(v, nGn); else if (k == 2) sa::norm_gp(v, nGn); else sa::norm_pl_u8(v, nGn, u8_missing);
    std::vector<uint32_t> w((size_t)nGn, 0xDEADBEEFu);
    for (int g = 0; g < nGo; g++) if (g2g[g] != -1) w[(size_t)g2g[g]] = ov[g];
    if (k == 0) ref_gl(w); else if (k == 1) ref_pl(w); else if (k == 2) ref_gp(w); else ref_u8(w, u8_missing);
    for (int h = 0; h < nGn; h++) if (!same(v[h], w[(size_t)h])) { fprintf(stderr, "kind %d genotype %d: %08x vs %08x\n", k, h, v[h], w[(size_t)h]); die("sample", o, t); }
    for (int h = nGn; h < sa::MAX_G; h++) if (v[h] != 0xDEADBEEFu) die("a routine wrote behind its count", o, t);
    n_samples_done++;
}

static uint32_t fbits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static void samples_of(const sa::SitePlan& P, const int* g2g, int nGo, int nGn, const std::vector<int>& o, const std::vector<int>& t) {
    uint32_t ov[sa::MAX_G];
    // GL: random negatives with a zero; with -inf entries; all -inf; missing
    for (int rep = 0; rep < 4; rep++) {
        for (int g = 0; g < nGo; g++) ov[g] = fbits(-(float)(rnd() % 100000) / 977.0f);
        ov[rnd() % (uint32_t)nGo] = fbits(0.0f);
        if (rep == 1) for (int g = 0; g < nGo; g++) if (rnd() & 1u) ov[g] = fbits(-INFINITY);
        if (rep == 2) for (int g = 0; g < nGo; g++) ov[g] = fbits(-INFINITY);
        if (rep == 3) for (int g = 0; g < nGo; g++) ov[g] = sa::FLOAT_MISSING_BITS;
        sample(P, g2g, nGo, nGn, ov, 0, false, o, t);
    }
    // PL: 0 .. 255 with a zero; large values; missing
    for (int rep = 0; rep < 3; rep++) {
        for (int g = 0; g < nGo; g++) ov[g] = rep == 1 ? rnd() % 2000000u : rnd() % 256u;
        if (rep == 0) ov[rnd() % (uint32_t)nGo] = 0;
        if (rep == 2) for (int g = 0; g < nGo; g++) ov[g] = sa::INT32_MISSING_BITS;
        sample(P, g2g, nGo, nGn, ov, 1, false, o, t);
    }
    // GP: random probabilities; a sum whose float order matters (one large value among many small ones); zeros; missing
    for (int rep = 0; rep < 4; rep++) {
        for (int g = 0; g < nGo; g++) ov[g] = fbits((float)(rnd() % 1000003u) / 1000003.0f);
        if (rep == 1) { for (int g = 0; g < nGo; g++) ov[g] = fbits(5.9604645e-8f * (float)(1 + rnd() % 3)); ov[rnd() % (uint32_t)nGo] = fbits(1.0f); }
        if (rep == 2) for (int g = 0; g < nGo; g++) ov[g] = fbits(0.0f);
        if (rep == 3) for (int g = 0; g < nGo; g++) ov[g] = sa::FLOAT_MISSING_BITS;
        sample(P, g2g, nGo, nGn, ov, 2, false, o, t);
    }
    // the one-byte PL: with 255 (capped) entries; all 255 with and without reads
    for (int rep = 0; rep < 3; rep++) {
        for (int g = 0; g < nGo; g++) ov[g] = (rnd() & 3u) ? rnd() % 256u : 255u;
        if (rep >= 1) for (int g = 0; g < nGo; g++) ov[g] = 255u;
        sample(P, g2g, nGo, nGn, ov, 3, rep == 2, o, t);
    }
}

// every ordered selection of n distinct codes out of 0 .. 4
static void selections(int n, std::vector<std::vector<int>>& out) {
    std::vector<int> cur;
    struct R { static void go(int n, std::vector<int>& cur, std::vector<std::vector<int>>& out) {
        if ((int)cur.size() == n) { out.push_back(cur); return; }
        for (int c = 0; c < 5; c++) { bool used = false; for (int x : cur) used = used || x == c; if (!used) { cur.push_back(c); go(n, cur, out); cur.pop_back(); } }
    } };
    R::go(n, cur, out);
}

int main() {
    long pairs = 0, subsets = 0, refused = 0;
    for (int no = 2; no <= 5; no++) for (int nn = 2; nn <= 5; nn++) {
        std::vector<std::vector<int>> olds, news;
        selections(no, olds); selections(nn, news);
        for (const auto& o : olds) for (const auto& t : news) {
            pairs++;
            // exactly sized allocations: a read or write behind either list is the sanitizer's to report
            int8_t* a2b = (int8_t*)malloc(5); int8_t* entry = (int8_t*)malloc(8);
            for (int k = 0; k < 5; k++) a2b[k] = k < no ? (int8_t)o[(size_t)k] : (int8_t)-1;
            entry[0] = (int8_t)nn; entry[6] = entry[7] = 0;
            for (int k = 0; k < 5; k++) entry[1 + k] = k < nn ? (int8_t)t[(size_t)k] : (int8_t)-1;
            int o2n[5], g2g[15];
            ref_maps(o, t, o2n, g2g);
            int8_t m1[sa::MAX_A], m2[sa::MAX_G];
            sa::allele_map(a2b, no, entry + 1, nn, m1);
            sa::genotype_map(m1, no, m2);
            for (int a = 0; a < 5; a++) if (m1[a] != (a < no ? o2n[a] : -1)) die("allele_map", o, t);
            for (int g = 0; g < 15; g++) if (m2[g] != g2g[g]) die("genotype_map", o, t);
            bool subset = true;
            for (int x : t) { bool in = false; for (int y : o) in = in || x == y; subset = subset && in; }
            sa::SitePlan P;
            const bool ok = sa::site_plan(a2b, no, entry, P);
            if (ok != subset) die("site_plan: accepted / refused", o, t);
            if (!ok) { refused++; if (P.n_new != 0) die("site_plan: a refused site has a count", o, t); free(a2b); free(entry); continue; }
            subsets++;
            const int nGo = no * (no + 1) / 2, nGn = nn * (nn + 1) / 2;
            if (P.n_new != nn || P.n_old != no) die("site_plan: counts", o, t);
            // the gather map is the inverse of the scatter map
            for (int h = 0; h < 15; h++) {
                if (h >= nGn) { if (P.new2old[h] != -1) die("site_plan: new2old behind the count", o, t); continue; }
                const int g = P.new2old[h];
                if (g < 0 || g >= nGo || g2g[g] != h) die("site_plan: new2old", o, t);
            }
            for (int j = 0; j < 5; j++) {
                if (P.a2b_new[j] != (j < nn ? t[(size_t)j] : -1)) die("site_plan: a2b_new", o, t);
                if (j < nn ? (P.qs_src[j] < 0 || o2n[P.qs_src[j]] != j) : P.qs_src[j] != -1) die("site_plan: qs_src", o, t);
            }
            samples_of(P, g2g, nGo, nGn, o, t);
            free(a2b); free(entry);
        }
    }
    // bad entries: counts outside 2 .. 5, an allele outside 0 .. 4, a duplicate
    {
        const int8_t a2b[5] = {0, 1, 2, 3, 4};
        const int8_t bad[5][8] = {{1, 0, -1, -1, -1, -1, 0, 0}, {6, 0, 1, 2, 3, 4, 0, 0}, {2, 0, 5, -1, -1, -1, 0, 0}, {3, 0, 1, 0, -1, -1, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
        for (const auto& e : bad) { sa::SitePlan P; if (sa::site_plan(a2b, 5, e, P) || P.n_new != 0) { fprintf(stderr, "a bad entry was accepted\n"); return 1; } }
    }
    printf("pairs %ld subsets %ld refused %ld samples %ld\n", pairs, subsets, refused, n_samples_done);
    return 0;
}
