// vgl_setal_core.h -- the per-site maps and per-sample routines of vgl_setal.hip (k_setal_plan, k_setal_apply) as code that compiles
// for the host and for the device; a host program around this header (tests/test_setal_core_cpu.py) runs it under the host sanitizers.
// What misc/setAlleles does to a record when it is given a new REF/ALT list (alleles as 0 .. 4 = A, C, G, T, the unobserved allele):
//   old2new[a]      the index of old allele a in the new list, or -1
//   oldgt2newgt[g]  bcf_alleles2gt(old2new[a1], old2new[a2]) for g = a2 (a2 + 1) / 2 + a1 when both are >= 0, else -1
//   QS              new[old2new[a]] = old[a]
//   GL, PL, GP      per sample: new[oldgt2newgt[g]] = old[g], then renormalised (norm_gl, norm_pl, norm_gp below)
// The kernels gather instead of scattering: with distinct alleles on either side the defined part of oldgt2newgt is one-to-one, so
// new[h] = old[newgt2oldgt[h]] is the same assignment, and a lane can load its values in the new order with constant register
// indices.  newgt2oldgt[h] = -1 marks a new genotype with an allele the record does not have: the tool reads uninitialised memory
// there, the library refuses the site (site_plan returns false).
// Values travel as their 32 bits: the missing pattern 0x7F800001 is a signalling NaN that arithmetic would quiet.
// Plain C++ only.
#ifndef VGL_SETAL_CORE_H
#define VGL_SETAL_CORE_H
#include <stdint.h>
#include <string.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif
#if defined(__clang__)
#define VGL_SA_UNROLL _Pragma("unroll")
#else
#define VGL_SA_UNROLL
#endif

namespace vgl_setal {

enum : uint32_t { FLOAT_MISSING_BITS = 0x7F800001u, INT32_MISSING_BITS = 0x80000000u, U8_MISSING = 255u };
enum { MAX_A = 5, MAX_G = 15 };

VGL_HD float sa_float(uint32_t b) { float f; memcpy(&f, &b, sizeof f); return f; }
VGL_HD uint32_t sa_bits(float f) { uint32_t b; memcpy(&b, &f, sizeof b); return b; }
VGL_HD bool sa_isnan(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

// bcf_alleles2gt
VGL_HD int alleles2gt(int a, int b) { return b > a ? b * (b + 1) / 2 + a : a * (a + 1) / 2 + b; }

// what k_setal_plan leaves in the workspace for one site (32 bytes)
struct SitePlan {
    int8_t new2old[MAX_G];      // newgt2oldgt; -1 = none
    int8_t n_new;               // new allele count 2 .. 5; 0 = the site is left alone (skipped, or refused)
    int8_t n_old;               // the record's allele count
    int8_t a2b_new[MAX_A];      // the new alleles2acgt, -1 behind n_new
    int8_t qs_src[MAX_A];       // QS: new[j] = old[qs_src[j]]
    int8_t pad[5];
};

// old2new of the record's alleles (a2b_old[0 .. n_old)) against the target list (tgt[0 .. n_new)): the first position that holds it
VGL_HD void allele_map(const int8_t* a2b_old, int n_old, const int8_t* tgt, int n_new, int8_t* old2new) {
    VGL_SA_UNROLL
    for (int a = 0; a < MAX_A; ++a) {
        int m = -1;
        VGL_SA_UNROLL
        for (int j = MAX_A - 1; j >= 0; --j)
            if (a < n_old && j < n_new && tgt[j] == a2b_old[a]) m = j;
        old2new[a] = (int8_t)m;
    }
}

// oldgt2newgt for the n_old (n_old + 1) / 2 genotypes of the record, -1 elsewhere
VGL_HD void genotype_map(const int8_t* old2new, int n_old, int8_t* oldgt2newgt) {
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g) oldgt2newgt[g] = -1;
    int g = 0;
    VGL_SA_UNROLL
    for (int a2 = 0; a2 < MAX_A; ++a2) {
        VGL_SA_UNROLL
        for (int a1 = 0; a1 <= a2; ++a1, ++g) {
            if (a2 >= n_old) continue;
            const int n1 = old2new[a1], n2 = old2new[a2];
            if (n1 >= 0 && n2 >= 0) oldgt2newgt[g] = (int8_t)alleles2gt(n1, n2);
        }
    }
}

// The plan of one site.  False when the target is not a list of 2 .. 5 distinct alleles of 0 .. 4 that the record all has (P.n_new = 0
// then); true otherwise, with P filled in.
VGL_HD bool site_plan(const int8_t* a2b_old, int n_old, const int8_t* entry, SitePlan& P) {
    memset(&P, 0xFF, sizeof P);
    P.n_new = 0; P.n_old = (int8_t)n_old;
    const int n_new = entry[0];
    if (n_old < 1 || n_old > MAX_A || n_new < 2 || n_new > MAX_A) return false;
    int8_t tgt[MAX_A];
    VGL_SA_UNROLL
    for (int j = 0; j < MAX_A; ++j) tgt[j] = j < n_new ? entry[1 + j] : (int8_t)-1;
    int8_t new2old_a[MAX_A];
    bool ok = true;
    VGL_SA_UNROLL
    for (int j = 0; j < MAX_A; ++j) {
        int m = -1, hits = 0;
        VGL_SA_UNROLL
        for (int a = MAX_A - 1; a >= 0; --a)
            if (a < n_old && tgt[j] == a2b_old[a]) m = a;
        VGL_SA_UNROLL
        for (int k = 0; k < MAX_A; ++k)
            if (k < j && tgt[k] == tgt[j]) hits++;
        new2old_a[j] = (int8_t)m;
        if (j < n_new && (tgt[j] < 0 || tgt[j] > 4 || m < 0 || hits)) ok = false;
    }
    if (!ok) return false;
    int h = 0;
    VGL_SA_UNROLL
    for (int b2 = 0; b2 < MAX_A; ++b2) {
        VGL_SA_UNROLL
        for (int b1 = 0; b1 <= b2; ++b1, ++h)
            if (b2 < n_new) P.new2old[h] = (int8_t)alleles2gt(new2old_a[b1], new2old_a[b2]);
    }
    VGL_SA_UNROLL
    for (int j = 0; j < MAX_A; ++j) {
        P.a2b_new[j] = tgt[j];
        P.qs_src[j] = j < n_new ? new2old_a[j] : (int8_t)-1;
    }
    P.n_new = (int8_t)n_new;
    return true;
}

// ---- the per-sample routines: v[0 .. n) in the new genotype order, as bits --------------------------------------------------------
// GL: a NaN among the new values = a missing sample, left as it is; otherwise the float maximum is subtracted from each
VGL_HD void norm_gl(uint32_t* v, int n) {
    bool miss = false;
    float mx = sa_float(0xFF800000u);                               // -inf
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) { miss = miss || sa_isnan(v[g]); const float x = sa_float(v[g]); if (x > mx) mx = x; }
    if (miss) return;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) v[g] = sa_bits(sa_float(v[g]) - mx);
}

// PL: INT32_MIN among the new values = missing; otherwise (int32)((float)pl - (float)min)
VGL_HD void norm_pl(uint32_t* v, int n) {
    bool miss = false;
    float mn = sa_float(0x7F800000u);                               // +inf
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) { miss = miss || v[g] == INT32_MISSING_BITS; const float x = (float)(int32_t)v[g]; if (x < mn) mn = x; }
    if (miss) return;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) v[g] = (uint32_t)(int32_t)((float)(int32_t)v[g] - mn);
}

// GP: a NaN among the new values = missing; otherwise each is divided by the float sum taken in ascending genotype order
VGL_HD void norm_gp(uint32_t* v, int n) {
    bool miss = false;
    float sum = 0.0f;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) { miss = miss || sa_isnan(v[g]); sum += sa_float(v[g]); }
    if (miss) return;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) v[g] = sa_bits(sa_float(v[g]) / sum);
}

// the one-byte PL (values 0 .. 255 in v): 255 cannot tell a capped value from a missing one, so `missing` is the caller's fmt_dp == 0
VGL_HD void norm_pl_u8(uint32_t* v, int n, bool missing) {
    if (missing) return;
    uint32_t mn = 255u;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n && v[g] < mn) mn = v[g];
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) v[g] = (v[g] - mn) & 0xFFu;
}

}  // namespace vgl_setal
#endif
