// vgl_inf.hip -- the records of --depth inf on the device (ABI 7 additions: vgl_inf_workspace_bytes, vgl_inf_fill_device).
// simulate_record_true_values (vcfgl.cpp:1089-1262): no read is drawn.  A tile's packed true genotypes become its records' allele
// lists (vgl_inf_core.h has the order and the maps) and, per sample, GL 0 / GP 1 / PL 0 at the true genotype and -inf / 0 / 255 at
// every other one.
//   k_inf_site      a sub-group of L = min(64, pow2 >= N) lanes per site counts A / C / G / T over the site's 2 N nibbles (lane l takes
//                   samples l, l + L, ...; the counts are summed across the sub-group with wavefront shuffles): 64 sites per wavefront at
//                   N = 1, one site per wavefront from N = 33 on.  The sub-group's first lane writes site_status, n_alleles,
//                   n_alleles_obs, alleles2acgt and the site's map (vgl_inf::pack_map, one 64-bit word) into the workspace.  A nibble outside
//                   0 .. 3 makes the site bad: one atomicMin per bad site on *bad_site.
//   k_inf_fill<SM>  one launch for all of GL, GP, PL and the one-byte PL (each optional).
//                   VGL_LAYOUT_PLANES  x[(i G + g) N + s]: a lane per (site, sample) writes its G values; the 64 lanes of a wavefront
//                     write 64 consecutive elements of every plane.  Planes g >= nG(site) get the missing value.
//                   VGL_LAYOUT_SAMPLE_MAJOR  x[i G N + s nG(i) + g]: a lane per value v = s nG + g < N nG of the slab, so that a
//                     wavefront's stores are 64 consecutive elements; nothing behind N nG is written.
//                   The arrays of a bad site are unspecified (written from its nibbles' low two bits, inside the site's own slab).
// The kernels are bound by their stores: one byte of gt is read per sample, up to 13 bytes are written per genotype.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_inf_core.h"

namespace {

namespace inf = vgl_inf;

constexpr int NT = 256;                 // lanes per workgroup

struct InfArgs {
    int32_t N, n_sites, G, do_unobserved, sub;      // sub: lanes per site in k_inf_site
    int64_t site0;                                  // absolute index of the tile's first site (bad_abs)
    const uint8_t* gt;
    int32_t* site_status; int32_t* n_alleles; int32_t* n_alleles_obs; int8_t* a2b;
    uint32_t* gl; uint32_t* gp; int32_t* pl; uint8_t* pl_u8;
    int32_t* bad_site;
    unsigned long long* bad_abs;                    // a context's word: the smallest bad absolute site, or NULL
    uint64_t* map;
};

__global__ __launch_bounds__(NT) void k_inf_site(InfArgs A) {
    const int L = A.sub;
    const int64_t i = ((int64_t)blockIdx.x * NT + threadIdx.x) / L;
    const int lane = threadIdx.x & (L - 1);
    const bool live = i < A.n_sites;
    int32_t ac0 = 0, ac1 = 0, ac2 = 0, ac3 = 0, bad = 0;
    if (live) {
        const uint8_t* row = A.gt + (size_t)i * A.N;
        for (int s = lane; s < A.N; s += L) {
            const int b = row[s], b0 = b & 0xF, b1 = b >> 4;
            bad |= (b0 > 3 || b1 > 3) ? 1 : 0;
            ac0 += (b0 == 0) + (b1 == 0); ac1 += (b0 == 1) + (b1 == 1); ac2 += (b0 == 2) + (b1 == 2); ac3 += (b0 == 3) + (b1 == 3);
        }
    }
    // (every lane of the wavefront takes part in the shuffles; a partner is always inside the aligned sub-group of L lanes)
    for (int off = L >> 1; off > 0; off >>= 1) {
        ac0 += __shfl_xor(ac0, off, 64); ac1 += __shfl_xor(ac1, off, 64); ac2 += __shfl_xor(ac2, off, 64); ac3 += __shfl_xor(ac3, off, 64);
        bad |= __shfl_xor(bad, off, 64);
    }
    if (!live || lane != 0) return;
    const int32_t ac[4] = {ac0, ac1, ac2, ac3};
    inf::SiteMap M;
    int8_t a2b[inf::MAX_A];
    inf::site_map(ac, A.do_unobserved, M, a2b);
    A.map[i] = inf::pack_map(M);
    A.site_status[i] = VGL_SITE_OK;
    A.n_alleles[i] = M.n_alleles;
    A.n_alleles_obs[i] = M.n_obs;
#pragma unroll
    for (int k = 0; k < inf::MAX_A; ++k) A.a2b[(size_t)i * 5 + k] = a2b[k];
    if (bad) {
        atomicMin(A.bad_site, (int32_t)i);
        if (A.bad_abs) atomicMin(A.bad_abs, (unsigned long long)(A.site0 + i));
    }
}

__device__ __forceinline__ int true_gt(uint64_t M, int b) { return inf::packed_true_genotype(M, b & 3, (b >> 4) & 3); }

// VGL_LAYOUT_PLANES: grid (n_sites, ceil(N / NT)), a lane per (site, sample)
__device__ __forceinline__ void fill_planes(const InfArgs& A) {
    const int64_t i = blockIdx.x;
    const int s = blockIdx.y * NT + threadIdx.x;
    if (s >= A.N) return;
    const uint64_t M = A.map[i];
    const int nA = inf::packed_n_alleles(M), nG = nA * (nA + 1) / 2;
    const int tg = true_gt(M, A.gt[(size_t)i * A.N + s]);
    const size_t base = (size_t)i * A.G * A.N + (size_t)s;
    for (int g = 0; g < A.G; ++g) {
        const size_t at = base + (size_t)g * A.N;
        const bool in = g < nG, hit = g == tg;
        if (A.gl) A.gl[at] = !in ? VGL_FLOAT_MISSING_BITS : hit ? 0x00000000u : 0xFF800000u;
        if (A.gp) A.gp[at] = !in ? VGL_FLOAT_MISSING_BITS : hit ? 0x3F800000u : 0x00000000u;
        if (A.pl) A.pl[at] = !in ? VGL_INT32_MISSING : hit ? 0 : 255;
        if (A.pl_u8) A.pl_u8[at] = (uint8_t)((in && hit) ? 0 : 255);
    }
}

// VGL_LAYOUT_SAMPLE_MAJOR: grid (n_sites, ceil(N G / NT)), a lane per value of the slab
__device__ __forceinline__ void fill_sm(const InfArgs& A) {
    const int64_t i = blockIdx.x;
    const uint64_t M = A.map[i];
    const uint32_t nA = (uint32_t)inf::packed_n_alleles(M), nG = nA * (nA + 1) / 2;
    const uint32_t v = blockIdx.y * (uint32_t)NT + threadIdx.x;
    if (v >= (uint32_t)A.N * nG) return;
    const uint32_t s = v / nG, g = v - s * nG;
    const bool hit = (int)g == true_gt(M, A.gt[(size_t)i * A.N + s]);
    const size_t at = (size_t)i * A.G * A.N + v;
    if (A.gl) A.gl[at] = hit ? 0x00000000u : 0xFF800000u;
    if (A.gp) A.gp[at] = hit ? 0x3F800000u : 0x00000000u;
    if (A.pl) A.pl[at] = hit ? 0 : 255;
    if (A.pl_u8) A.pl_u8[at] = (uint8_t)(hit ? 0 : 255);
}

template <bool SM>
__global__ __launch_bounds__(NT) void k_inf_fill(InfArgs A) {
    if (SM) fill_sm(A); else fill_planes(A);
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_inf_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    return ((int64_t)n_sites * (int64_t)sizeof(uint64_t) + 255) / 256 * 256;
}

// vgl_inf_fill_device with a context's extras (hostlib: not exported): site0 and the word that takes the smallest bad absolute site
extern "C" int vgl_inf_fill_impl(int32_t device, int32_t n_samples, int32_t n_sites, int32_t do_unobserved, int32_t max_genotypes, int32_t max_alleles,
                                 int32_t layout, const uint8_t* gt, int32_t* site_status, int32_t* n_alleles, int32_t* n_alleles_obs, int8_t* alleles2acgt,
                                 float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site, void* workspace, int64_t workspace_bytes,
                                 int64_t site0, unsigned long long* bad_abs, void* hip_stream) {
    if (n_samples <= 0 || n_sites < 0 || do_unobserved < 0 || do_unobserved > 5)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: bad n_samples, n_sites or do_unobserved");
    if (max_genotypes != inf::max_genotypes(do_unobserved) || max_alleles != inf::max_alleles(do_unobserved))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: max_genotypes / max_alleles must be what do_unobserved gives (10 / 4 for 0 and 3, else 15 / 5)");
    if (layout != VGL_LAYOUT_PLANES && layout != VGL_LAYOUT_SAMPLE_MAJOR)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: layout must be VGL_LAYOUT_PLANES or VGL_LAYOUT_SAMPLE_MAJOR");
    if (n_sites == 0) return VGL_OK;
    if (!gt || !site_status || !n_alleles || !n_alleles_obs || !alleles2acgt || !bad_site) return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: null argument");
    const int64_t need = vgl_inf_workspace_bytes(n_samples, n_sites);
    if (need < 0 || !workspace || workspace_bytes < need)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: workspace smaller than vgl_inf_workspace_bytes()");
    const bool sm = layout == VGL_LAYOUT_SAMPLE_MAJOR;
    const int64_t per_site = sm ? (int64_t)n_samples * max_genotypes : (int64_t)n_samples;
    const int64_t chunks = (per_site + NT - 1) / NT;
    if (chunks > 65535) return vgl_pack_set_error(VGL_E_ARG, "vgl_inf_fill_device: too many samples for one call");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inf_fill_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    InfArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.G = max_genotypes; A.do_unobserved = do_unobserved; A.site0 = site0;
    A.sub = 1;
    while (A.sub < 64 && A.sub < n_samples) A.sub <<= 1;
    A.gt = gt; A.site_status = site_status; A.n_alleles = n_alleles; A.n_alleles_obs = n_alleles_obs; A.a2b = alleles2acgt;
    A.gl = (uint32_t*)gl; A.gp = (uint32_t*)gp; A.pl = pl; A.pl_u8 = pl_u8; A.bad_site = bad_site; A.bad_abs = bad_abs; A.map = (uint64_t*)workspace;
    const int sites_per_group = NT / A.sub;
    hipLaunchKernelGGL(k_inf_site, dim3((unsigned)((n_sites + sites_per_group - 1) / sites_per_group)), dim3(NT), 0, st, A);
    if (gl || gp || pl || pl_u8) {
        const dim3 grid((unsigned)n_sites, (unsigned)chunks);
        if (sm) hipLaunchKernelGGL(k_inf_fill<true>, grid, dim3(NT), 0, st, A);
        else hipLaunchKernelGGL(k_inf_fill<false>, grid, dim3(NT), 0, st, A);
    }
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inf_fill_device: a launch failed");
    return VGL_OK;
}

extern "C" int vgl_inf_fill_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t do_unobserved, int32_t max_genotypes, int32_t max_alleles,
                                   int32_t layout, const uint8_t* gt, int32_t* site_status, int32_t* n_alleles, int32_t* n_alleles_obs, int8_t* alleles2acgt,
                                   float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site, void* workspace, int64_t workspace_bytes,
                                   void* hip_stream) {
    return vgl_inf_fill_impl(device, n_samples, n_sites, do_unobserved, max_genotypes, max_alleles, layout, gt, site_status, n_alleles, n_alleles_obs, alleles2acgt,
                             gl, pl, gp, pl_u8, bad_site, workspace, workspace_bytes, 0, nullptr, hip_stream);
}
