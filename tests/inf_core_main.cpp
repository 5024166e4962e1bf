// inf_core_main.cpp -- vcfgl_amd/csrc/vgl_inf_core.h on the CPU (built by tests/test_inf_core_cpu.py with the host sanitizers): every
// vector of allele counts in {0 .. 3}^4 but the all-zero one, under every -doUnobserved 0 .. 5, through the header's closed form (the
// map as a struct and as the packed word the kernels keep) and through a second, straightforward implementation (the insertion sort spelled out, the list built entry by entry, positions found
// by searching the list); and for every such site every pair of bases that occur in it, the true genotype both ways.
// Prints "sites <n> pairs <n>"; any difference is printed and makes the exit status 1.
#include <stdio.h>
#include <string.h>

#include "vgl_inf_core.h"

struct RefSite { int alleles[5]; int n_alleles, n_obs; };

static RefSite ref_site(const int ac[4], int do_unobserved) {
    int order[4] = {0, 1, 2, 3};
    RefSite r;
    r.n_obs = 0;
    for (int i = 0; i < 4; ++i) {
        if (ac[i] > 0) r.n_obs++;
        for (int j = i; j > 0 && ac[order[j]] > ac[order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    }
    r.n_alleles = 0;
    for (int k = 0; k < 5; ++k) r.alleles[k] = -1;
    for (int i = 0; i < r.n_obs; ++i) r.alleles[r.n_alleles++] = order[i];
    if (do_unobserved >= 3) for (int i = r.n_obs; i < 4; ++i) r.alleles[r.n_alleles++] = order[i];
    if (do_unobserved == 1 || do_unobserved == 2 || do_unobserved == 4 || do_unobserved == 5) r.alleles[r.n_alleles++] = 4;
    return r;
}
static int ref_find(const RefSite& r, int base) { for (int k = 0; k < r.n_alleles; ++k) if (r.alleles[k] == base) return k; return -1; }
static int ref_gt(int a, int b) { if (a > b) { const int t = a; a = b; b = t; } return b * (b + 1) / 2 + a; }

int main() {
    long sites = 0, pairs = 0, bad = 0;
    for (int code = 1; code < 256; ++code) {
        const int32_t ac[4] = {code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3};
        const int iac[4] = {ac[0], ac[1], ac[2], ac[3]};
        for (int d = 0; d <= 5; ++d) {
            vgl_inf::SiteMap M;
            int8_t a2b[vgl_inf::MAX_A];
            memset(&M, 0x55, sizeof M); memset(a2b, 0x55, sizeof a2b);
            vgl_inf::site_map(ac, d, M, a2b);
            const RefSite r = ref_site(iac, d);
            ++sites;
            bool ok = M.n_alleles == r.n_alleles && M.n_obs == r.n_obs && M.n_alleles <= vgl_inf::max_alleles(d) &&
                      M.n_alleles * (M.n_alleles + 1) / 2 <= vgl_inf::max_genotypes(d);
            for (int k = 0; k < 5; ++k) ok = ok && a2b[k] == r.alleles[k];
            for (int b = 0; b < 4; ++b) ok = ok && M.idx[b] == ref_find(r, b) && vgl_inf::allele_index(M, b) == ref_find(r, b);
            const uint64_t W = vgl_inf::pack_map(M);
            ok = ok && vgl_inf::packed_n_alleles(W) == r.n_alleles;
            if (!ok) { ++bad; printf("site map differs: ac %d %d %d %d doUnobserved %d\n", iac[0], iac[1], iac[2], iac[3], d); continue; }
            for (int b0 = 0; b0 < 4; ++b0) for (int b1 = 0; b1 < 4; ++b1) {
                if (!ac[b0] || !ac[b1]) continue;
                ++pairs;
                const int got = vgl_inf::true_genotype(M, b0, b1), want = ref_gt(ref_find(r, b0), ref_find(r, b1));
                if (got != want || vgl_inf::packed_true_genotype(W, b0, b1) != want || got < 0 || got >= M.n_alleles * (M.n_alleles + 1) / 2) {
                    ++bad; printf("genotype differs: ac %d %d %d %d doUnobserved %d bases %d %d: %d, expected %d\n", iac[0], iac[1], iac[2], iac[3], d, b0, b1, got, want);
                }
            }
        }
    }
    printf("sites %ld pairs %ld\n", sites, pairs);
    return bad ? 1 : 0;
}
