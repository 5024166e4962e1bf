// vgl_disc.hip -- genotype calls and their discordance against the truth, tallied on the device (ABI 7 additions: vgl_disc_table_len,
// vgl_disc_tally_device; the context's vgl_ctx_discordance runs the same kernel behind every tile's likelihood kernel).
// What misc/gtDiscordance computes from a call file and -printTruth's file, from the arrays of a tile instead.  Per kept site
// (site_status >= 0) and sample:
//   call missing   fmt_dp == 0, a true allele outside A/C/G/T (VGL_GT_MISSING), or a site without a genotype of two A/C/G/T alleles:
//                  callmis[sample] goes up and nothing else is counted
//   call           the lowest g < nG(site) with the smallest PL among the genotypes whose two alleles both map to A/C/G/T through
//                  alleles2acgt (one with the unobserved allele is never called); g = b (b + 1) / 2 + a, a <= b
//   GQ             gtDiscordance -doGQ 8: the smallest PL over ALL g < nG(site) that is not 0, capped at 127; 127 without one (1 ... 127)
//   PL             one byte (pl_u8) or int32 (pl); an int32 value outside [0, 255] (VGL_INT32_MISSING included) counts as 255, which is
//                  what pl_u8 holds for it -- both forms give the same table
//   cell           true bases (the nibbles of gt) against called bases as unordered pairs: 0 hom->hom concordant, 1 hom->hom
//                  discordant, 2 het->het concordant, 3 het->het discordant, 4 hom->het, 5 het->hom (VGL_DISC_*)
// The table (int64): cell[sample][6][128] by GQ, callmis[sample], sites[2] = kept, skipped (site_status < 0).  Counts are integer sums:
// the table does not depend on how sites are cut into tiles, nor on the order of the additions.
//   k_disc_tally   a workgroup of 16 wavefronts owns 64 consecutive samples over a run of sites: a wavefront takes a site, its lanes the
//                  samples (a plane row, or the sample-major slab of the 64 samples, is one contiguous run).  The site's allele table is
//                  wave-uniform.  Counts go to an LDS histogram [cell][GQ][sample] of 16-bit counters, two to a word, 96 KB -- a counter
//                  belongs to one sample and a run has at most 32768 sites, so it cannot wrap; lanes of one wavefront hit 32 different
//                  words.  Once per workgroup the non-zero counters are added to the table with 64-bit atomics.  No global atomic per call.
//                  With an error word (the context's), a tile whose VGL_DEVERR_CAPACITY bit is up is not counted: it is run again.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_device.h"

namespace {

constexpr int NT = 1024;                 // lanes per workgroup
constexpr int SG = 64;                   // samples per workgroup = lanes of a wavefront
constexpr int NCELL = 6, NGQ = 128;
constexpr int HIST = NCELL * NGQ * SG;   // 16-bit counters
constexpr int MAX_RUN = 32768;           // sites per workgroup: below 2^16
constexpr size_t LDS_BYTES = (size_t)HIST * 2 + (SG + 2) * sizeof(uint32_t);

struct DiscArgs {
    int32_t N, n_sites, G, run;
    const int32_t* site_status;
    const int32_t* n_alleles;
    const int8_t* a2b;                  // alleles2acgt [n_sites][5]
    const int32_t* dp;
    const void* pl;
    const uint8_t* gt;
    const uint32_t* errflag;            // may be null
    unsigned long long* table;
};

template <bool U8, bool SM>
__global__ __launch_bounds__(NT) void k_disc_tally(DiscArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];       // [HIST / 2] counters, [SG] call-missing, [2] sites
    if (A.errflag && (*A.errflag & VGL_DEVERR_CAPACITY)) return;
    uint32_t* const s_mis = s_h + HIST / 2;
    uint32_t* const s_sites = s_mis + SG;
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < HIST / 2 + SG + 2; k += NT) s_h[k] = 0u;
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const int N = A.N;
    const int s = (int)blockIdx.x * SG + lane;
    const int i0 = (int)blockIdx.y * A.run;
    const int i1 = (A.n_sites - i0 < A.run) ? A.n_sites : i0 + A.run;
    uint32_t mis = 0;
    const int wv0 = __builtin_amdgcn_readfirstlane(wv);                   // (the site index is wave-uniform: its status and allele table come by scalar loads)
    for (int i = i0 + wv0; i < i1; i += NT / 64) {
        const int st = A.site_status[i];
        int nA = A.n_alleles[i];
        uint32_t codes = 0;                                              // a nibble per allele: its base, 15 = none of A/C/G/T
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int b = A.a2b[(size_t)i * 5 + k];
            codes |= (uint32_t)((b >= 0 && b <= 3) ? b : 15) << (4 * k);
        }
        if (st < 0 || s >= N) continue;
        nA = nA < 0 ? 0 : (nA > 5 ? 5 : nA);
        const size_t ev = (size_t)i * N + s;
        const int32_t dp = A.dp[ev];
        const uint32_t gt = A.gt[ev];
        const uint32_t t0 = gt & 15u, t1 = gt >> 4;
        if (dp == 0 || t0 > 3u || t1 > 3u) { ++mis; continue; }
        const int nG = nA * (nA + 1) / 2;
        if (nG > A.G) { ++mis; continue; }                                 // (a site wider than the caller's planes: never read past them)
        uint32_t bestv = 256u, bestc = 0u, gqmin = 255u;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
#pragma unroll
            for (int a = 0; a <= b; ++a) {
                const int g = b * (b + 1) / 2 + a;
                if (b < nA) {
                    const size_t at = SM ? ((size_t)i * A.G * N + (size_t)s * nG + g) : (((size_t)i * A.G + g) * N + s);
                    uint32_t v;
                    if (U8) v = ((const uint8_t*)A.pl)[at];
                    else { v = (uint32_t)((const int32_t*)A.pl)[at]; v = v > 255u ? 255u : v; }
                    const uint32_t ca = codes >> (4 * a) & 15u, cb = codes >> (4 * b) & 15u;
                    if (ca < 4u && cb < 4u && v < bestv) { bestv = v; bestc = ca | cb << 2; }
                    if (v != 0u && v < gqmin) gqmin = v;
                }
            }
        }
        if (bestv == 256u) { ++mis; continue; }
        const uint32_t gq = gqmin > 127u ? 127u : gqmin;
        const uint32_t c0 = bestc & 3u, c1 = bestc >> 2;
        const bool thom = t0 == t1, chom = c0 == c1;
        uint32_t cell;
        if (thom && chom) cell = t0 == c0 ? 0u : 1u;
        else if (!thom && !chom) cell = ((t0 == c0 && t1 == c1) || (t0 == c1 && t1 == c0)) ? 2u : 3u;
        else cell = thom ? 4u : 5u;
        const uint32_t idx = (cell * NGQ + gq) * SG + (uint32_t)lane;
        atomicAdd(&s_h[idx >> 1], 1u << (16u * (idx & 1u)));
    }
    if (mis) atomicAdd(&s_mis[lane], mis);
    if (blockIdx.x == 0) {                                               // the run's site counts, once
        uint32_t kept = 0, skipped = 0;
        for (int i = i0 + tid; i < i1; i += NT) { if (A.site_status[i] >= 0) ++kept; else ++skipped; }
        if (kept) atomicAdd(&s_sites[0], kept);
        if (skipped) atomicAdd(&s_sites[1], skipped);
    }
    __syncthreads();
    for (int w = tid; w < HIST / 2; w += NT) {
        const uint32_t word = s_h[w];
        if (!word) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t n = word >> (16 * h) & 0xffffu;
            const int idx = 2 * w + h, ls = idx & (SG - 1), cg = idx >> 6;   // cg = cell * 128 + GQ
            const int sm = (int)blockIdx.x * SG + ls;
            if (n && sm < N) atomicAdd(&A.table[(size_t)sm * (NCELL * NGQ) + cg], (unsigned long long)n);
        }
    }
    if (tid < SG) {
        const int sm = (int)blockIdx.x * SG + tid;
        if (s_mis[tid] && sm < N) atomicAdd(&A.table[(size_t)N * (NCELL * NGQ) + sm], (unsigned long long)s_mis[tid]);
    }
    if (tid < 2 && s_sites[tid]) atomicAdd(&A.table[(size_t)N * (NCELL * NGQ + 1) + tid], (unsigned long long)s_sites[tid]);
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_disc_table_len(int32_t n_samples) {
    if (n_samples < 0) return -1;
    return (int64_t)n_samples * (NCELL * NGQ + 1) + 2;
}

// the stateless entry and the context's: errflag != NULL skips a tile whose capacity flag is up
extern "C" int vgl_disc_tally_impl(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout,
                                   const int32_t* site_status, const int32_t* n_alleles, const int8_t* alleles2acgt, const int32_t* fmt_dp,
                                   const uint8_t* pl_u8, const int32_t* pl, const uint8_t* gt, int64_t* table, const uint32_t* errflag,
                                   void* hip_stream) {
    if (n_samples <= 0 || n_sites < 0 || max_genotypes < 1 || max_genotypes > 15)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_disc_tally_device: bad n_samples, n_sites or max_genotypes");
    if (layout != VGL_LAYOUT_PLANES && layout != VGL_LAYOUT_SAMPLE_MAJOR)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_disc_tally_device: layout must be VGL_LAYOUT_PLANES or VGL_LAYOUT_SAMPLE_MAJOR");
    if ((pl_u8 != nullptr) == (pl != nullptr)) return vgl_pack_set_error(VGL_E_ARG, "vgl_disc_tally_device: exactly one of pl_u8 and pl is given");
    if (!site_status || !n_alleles || !alleles2acgt || !fmt_dp || !gt || !table) return vgl_pack_set_error(VGL_E_ARG, "vgl_disc_tally_device: null argument");
    if (n_sites == 0) return VGL_OK;
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_disc_tally_device: hipSetDevice failed");
    DiscArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.G = max_genotypes;
    A.site_status = site_status; A.n_alleles = n_alleles; A.a2b = alleles2acgt; A.dp = fmt_dp; A.gt = gt;
    A.pl = pl_u8 ? (const void*)pl_u8 : (const void*)pl; A.errflag = errflag; A.table = (unsigned long long*)table;
    // about two workgroups per CU where the tile has them, runs of at least 16 sites (a workgroup clears and scans 96 KB of LDS)
    const int groups = (n_samples + SG - 1) / SG;
    int runs = 512 / groups;
    const int most = (n_sites + 15) / 16;
    if (runs > most) runs = most;
    if (runs < 1) runs = 1;
    int run = (n_sites + runs - 1) / runs;
    if (run > MAX_RUN) run = MAX_RUN;
    runs = (n_sites + run - 1) / run;
    if (runs > 65535) return vgl_pack_set_error(VGL_E_ARG, "vgl_disc_tally_device: too many sites for one call");
    A.run = run;
    const dim3 grid((unsigned)groups, (unsigned)runs);
    hipStream_t st = (hipStream_t)hip_stream;
    const bool sm = layout == VGL_LAYOUT_SAMPLE_MAJOR;
    if (pl_u8) {
        if (sm) hipLaunchKernelGGL((k_disc_tally<true, true>), grid, dim3(NT), LDS_BYTES, st, A);
        else hipLaunchKernelGGL((k_disc_tally<true, false>), grid, dim3(NT), LDS_BYTES, st, A);
    } else {
        if (sm) hipLaunchKernelGGL((k_disc_tally<false, true>), grid, dim3(NT), LDS_BYTES, st, A);
        else hipLaunchKernelGGL((k_disc_tally<false, false>), grid, dim3(NT), LDS_BYTES, st, A);
    }
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_disc_tally_device: the launch failed");
    return VGL_OK;
}

extern "C" int vgl_disc_tally_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout,
                                     const int32_t* site_status, const int32_t* n_alleles, const int8_t* alleles2acgt, const int32_t* fmt_dp,
                                     const uint8_t* pl_u8, const int32_t* pl, const uint8_t* gt, int64_t* table, void* hip_stream) {
    return vgl_disc_tally_impl(device, n_samples, n_sites, max_genotypes, layout, site_status, n_alleles, alleles2acgt, fmt_dp, pl_u8, pl, gt, table,
                               nullptr, hip_stream);
}
