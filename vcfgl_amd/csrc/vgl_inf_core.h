// vgl_inf_core.h -- the per-site allele list and the per-sample true genotype of vgl_inf.hip (k_inf_site, k_inf_fill) as code that
// compiles for the host and for the device; a host program around this header (tests/test_inf_core_cpu.py) runs it under the host
// sanitizers.
// What simulate_record_true_values (vcfgl.cpp:1089-1262) does to a record under --depth inf: no read is drawn, the alleles of the
// record are those its samples carry, ordered by how often they occur, and every sample gets its true genotype with certainty.
//   order           the four bases by descending allele count; vcfgl.cpp:1106-1116 is an insertion sort that swaps only on strictly
//                   greater, i.e. a stable sort: ties keep A < C < G < T.  Hence the closed form used here:
//                   rank[b] = #{c : ac[c] > ac[b]} + #{c < b : ac[c] == ac[b]}
//   n_alleles_obs   the number of non-zero counts (a base without a count sorts behind every base with one)
//   the list        -doUnobserved 0 / 1 / 2: the observed bases; 3 / 4 / 5: all four.  1, 2, 4, 5 append the unobserved allele (4)
//   idx[b]          the position of base b in the list, or -1
//   tg              bcf_alleles2gt(idx[b0], idx[b1]) of a sample's two bases
// Plain C++ only.
#ifndef VGL_INF_CORE_H
#define VGL_INF_CORE_H
#include <stdint.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif
#if defined(__clang__)
#define VGL_INF_UNROLL _Pragma("unroll")
#else
#define VGL_INF_UNROLL
#endif

namespace vgl_inf {

enum { MAX_A = 5, MAX_G = 15 };

// bcf_alleles2gt
VGL_HD int alleles2gt(int a, int b) { return b > a ? b * (b + 1) / 2 + a : a * (a + 1) / 2 + b; }

VGL_HD bool adds_unobserved(int do_unobserved) { return do_unobserved == 1 || do_unobserved == 2 || do_unobserved == 4 || do_unobserved == 5; }
VGL_HD bool explodes_acgt(int do_unobserved) { return do_unobserved >= 3; }
// the most alleles / genotypes a site of such a run can have (vgl_max_alleles, vgl_max_genotypes)
VGL_HD int max_alleles(int do_unobserved) { return adds_unobserved(do_unobserved) ? 5 : 4; }
VGL_HD int max_genotypes(int do_unobserved) { return adds_unobserved(do_unobserved) ? 15 : 10; }

// the map of one site; k_inf_site leaves it in the workspace as one 64-bit word (pack_map)
struct SiteMap {
    int8_t idx[4];              // base -> position in the allele list; -1 = not in it
    int8_t n_alleles;           // 1 .. 5
    int8_t n_obs;               // 1 .. 4 (0: no sample)
    int8_t pad[2];
};

// The map of one site from its allele counts ac[0 .. 4) = A, C, G, T; a2b[0 .. 5) = alleles2acgt (4 = unobserved, -1 behind the count).
VGL_HD void site_map(const int32_t* ac, int do_unobserved, SiteMap& M, int8_t* a2b) {
    const int c[4] = {ac[0], ac[1], ac[2], ac[3]};
    int n_obs = 0;
    VGL_INF_UNROLL
    for (int b = 0; b < 4; ++b) n_obs += c[b] > 0 ? 1 : 0;
    const int n_acgt = explodes_acgt(do_unobserved) ? 4 : n_obs;
    const bool unobs = adds_unobserved(do_unobserved);
    VGL_INF_UNROLL
    for (int k = 0; k < MAX_A; ++k) a2b[k] = (int8_t)((k == n_acgt && unobs) ? 4 : -1);
    VGL_INF_UNROLL
    for (int b = 0; b < 4; ++b) {
        int rank = 0;
        VGL_INF_UNROLL
        for (int o = 0; o < 4; ++o) rank += (c[o] > c[b] || (o < b && c[o] == c[b])) ? 1 : 0;
        M.idx[b] = (int8_t)(rank < n_acgt ? rank : -1);
        VGL_INF_UNROLL
        for (int k = 0; k < 4; ++k)
            if (k == rank && rank < n_acgt) a2b[k] = (int8_t)b;
    }
    M.n_alleles = (int8_t)(n_acgt + (unobs ? 1 : 0));
    M.n_obs = (int8_t)n_obs;
    M.pad[0] = M.pad[1] = 0;
}

// the list position of base b (0 .. 3) without a variable index into M
VGL_HD int allele_index(const SiteMap& M, int b) {
    int r = M.idx[0];
    r = b == 1 ? M.idx[1] : r;
    r = b == 2 ? M.idx[2] : r;
    r = b == 3 ? M.idx[3] : r;
    return r;
}

// the true genotype of a sample with the bases b0, b1 (0 .. 3, both in the list)
VGL_HD int true_genotype(const SiteMap& M, int b0, int b1) { return alleles2gt(allele_index(M, b0), allele_index(M, b1)); }

// The map as a word -- byte b: idx[b], byte 4: n_alleles, byte 5: n_obs -- and the two things k_inf_fill reads from it.  (A lane
// keeps the word in a register pair and shifts; a SiteMap copied per lane is an 8-byte private array.)
VGL_HD uint64_t pack_map(const SiteMap& M) {
    uint64_t w = 0;
    VGL_INF_UNROLL
    for (int b = 0; b < 4; ++b) w |= (uint64_t)(uint8_t)M.idx[b] << (8 * b);
    return w | (uint64_t)(uint8_t)M.n_alleles << 32 | (uint64_t)(uint8_t)M.n_obs << 40;
}
VGL_HD int packed_n_alleles(uint64_t w) { return (int)(int8_t)(w >> 32); }
VGL_HD int packed_true_genotype(uint64_t w, int b0, int b1) { return alleles2gt((int)(int8_t)(w >> (8 * b0)), (int)(int8_t)(w >> (8 * b1))); }

}  // namespace vgl_inf
#endif
