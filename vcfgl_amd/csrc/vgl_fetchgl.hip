// vgl_fetchgl.hip -- one genotype's FORMAT/GL of every sample as CSV text on the device (ABI 7 additions: vgl_fetchgl_bound,
// vgl_fetchgl_workspace_bytes, vgl_fetchgl_format_device).
// What misc/fetchGl prints behind "POS," for a record of the output file, from the arrays of a tile instead.  For every site i with
// site_status[i] >= 0 where both requested alleles a and b (0 .. 4 = A, C, G, T, unobserved) occur among the site's n_alleles[i]
// entries of alleles2acgt -- at indices j0 and j1, g = max (max + 1) / 2 + min -- the output is
//     value(0) "," value(1) "," ... value(N-1) "\n"              value(s) = GL of genotype g of sample s
// Every other site produces no bytes.  A value is formatted by vgl_fetchgl_core.h (fmt_value: "MISSING", "END", glibc's %f of the
// simulated float or of the float its VCF text reads back as).  Both GL layouts: planes gl[(i G + g) N + s] -- a genotype's row is one
// contiguous run for the 64 lanes of a wavefront -- and VGL_LAYOUT_SAMPLE_MAJOR gl[i G N + s nG(i) + g].  A site whose nG(i) exceeds
// max_genotypes has no line (never a read past the caller's planes).
// Three passes, the shape of vgl_text.hip (plan, scan, write):
//   k_fetchgl_plan   one workgroup per site: the site's status, allele count and allele table are wave-uniform; every lane formats its
//                    sample's value without storing it (the length plus the separator), a workgroup scan gives each column's offset
//                    inside the site (workspace, uint32 per (site, sample)) and the site's length
//   k_text_scan      vgl_text.hip's, through vgl_text_scan_launch: offsets[0 .. n_sites], offsets[n_sites] = total
//   k_fetchgl_write  one lane per (site, sample): the same formatter again, storing at its offset; nothing is written when the total
//                    exceeds dst_cap (the caller reads offsets[n_sites] to learn the size it needs)
// Bytes are written with ordinary byte stores, each lane inside its own column.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_fetchgl_core.h"

namespace {

namespace fg = vgl_fetchgl;

constexpr int NT = 256;                 // lanes per workgroup (plan: one workgroup per site, samples in chunks of NT)

struct FetchArgs {
    int32_t N, n_sites, G, a, b, mode;
    const int32_t* site_status;
    const int32_t* n_alleles;
    const int8_t* a2b;                  // alleles2acgt [n_sites][5]
    const uint32_t* gl;
    uint8_t* dst;
    int64_t cap;
    int64_t* off;
    uint32_t* ws;
};

// the element of site i's genotype (wave-uniform) where sample 0's value lies and the step to the next sample's; false: no line
template <bool SM>
__device__ bool site_row(const FetchArgs& A, int64_t i, size_t& at0, int& step) {
    if (A.site_status[i] < 0) return false;
    int nA = A.n_alleles[i];
    nA = nA < 0 ? 0 : (nA > 5 ? 5 : nA);
    int8_t t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = A.a2b[(size_t)i * 5 + k];
    const int g = fg::genotype_index(t, nA, A.a, A.b);
    const int nG = nA * (nA + 1) / 2;
    if (g < 0 || nG > A.G) return false;
    if (SM) { at0 = (size_t)i * A.G * A.N + (size_t)g; step = nG; }
    else { at0 = ((size_t)i * A.G + (size_t)g) * A.N; step = 1; }
    return true;
}

template <bool SM>
__global__ __launch_bounds__(NT) void k_fetchgl_plan(FetchArgs A) {
    __shared__ uint32_t part[NT / 64];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    size_t at0 = 0; int step = 1;
    if (!site_row<SM>(A, i, at0, step)) { if (tid == 0) A.off[i] = 0; return; }
    uint32_t carry = 0;
    for (int s0 = 0; s0 < A.N; s0 += NT) {
        const int s = s0 + tid;
        uint32_t len = 0;
        if (s < A.N) { fg::Emit<false> e{nullptr, 0, 0}; fg::fmt_value(e, A.gl[at0 + (size_t)s * step], A.mode); len = e.n + 1u; }
        uint32_t x = len;                                   // inclusive scan in the wavefront
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) part[wv] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) { const uint32_t p = part[w]; if (w < wv) before += p; total += p; }
        if (s < A.N) A.ws[i * A.N + s] = carry + before + x - len;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) A.off[i] = (int64_t)carry;
}

// grid (n_sites, ceil(N / NT)): lane = one sample's value of one site
template <bool SM>
__global__ __launch_bounds__(NT) void k_fetchgl_write(FetchArgs A) {
    const int64_t i = blockIdx.x;
    const int s = blockIdx.y * NT + threadIdx.x;
    if (A.off[A.n_sites] > A.cap) return;                   // does not fit: nothing is written
    const int64_t b = A.off[i], end = A.off[i + 1];
    if (end <= b || s >= A.N) return;                       // a site without a line
    size_t at0 = 0; int step = 1;
    if (!site_row<SM>(A, i, at0, step)) return;
    const int64_t c0 = b + A.ws[i * A.N + s];
    const int64_t c1 = s + 1 < A.N ? b + A.ws[i * A.N + s + 1] : end;
    if (c0 >= c1 || c1 > end) return;
    fg::Emit<true> e{A.dst + c0, 0, (uint32_t)(c1 - c0)};
    fg::fmt_value(e, A.gl[at0 + (size_t)s * step], A.mode);
    e.put(s + 1 < A.N ? ',' : '\n');
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()
extern "C" int vgl_text_scan_launch(int32_t n_sites, int64_t* offsets, void* hip_stream);      // vgl_text.hip (not exported)

extern "C" int64_t vgl_fetchgl_bound(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    int64_t r;
    if (__builtin_mul_overflow((int64_t)n_sites * n_samples, (int64_t)(fg::MAX_VALUE_LEN + 1), &r)) return -1;
    return r;
}

extern "C" int64_t vgl_fetchgl_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    return (int64_t)n_samples * n_sites * (int64_t)sizeof(uint32_t);
}

extern "C" int vgl_fetchgl_format_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout,
                                         const int32_t* site_status, const int32_t* n_alleles, const int8_t* alleles2acgt, const float* gl,
                                         int32_t a, int32_t b, int32_t value_mode, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                         void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (n_samples <= 0 || n_sites < 0 || max_genotypes < 1 || max_genotypes > 15 || dst_cap < 0)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: bad n_samples, n_sites, max_genotypes or dst_cap");
    if (layout != VGL_LAYOUT_PLANES && layout != VGL_LAYOUT_SAMPLE_MAJOR)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: layout must be VGL_LAYOUT_PLANES or VGL_LAYOUT_SAMPLE_MAJOR");
    if (a < 0 || a > 4 || b < 0 || b > 4) return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: alleles are 0 .. 4 (A, C, G, T, unobserved)");
    if (value_mode != VGL_FETCHGL_FLOAT && value_mode != VGL_FETCHGL_TEXT)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: value_mode must be VGL_FETCHGL_FLOAT or VGL_FETCHGL_TEXT");
    if (!offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: null offsets");
    if (n_sites > 0 && (!site_status || !n_alleles || !alleles2acgt || !gl || (dst_cap > 0 && !dst)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: null argument");
    if (n_sites > 0 && (!workspace || workspace_bytes < vgl_fetchgl_workspace_bytes(n_samples, n_sites)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: workspace smaller than vgl_fetchgl_workspace_bytes()");
    // a site's text is addressed with 32-bit offsets inside the site
    if ((int64_t)n_samples * (fg::MAX_VALUE_LEN + 1) > (int64_t)UINT32_MAX)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: too many samples for one line");
    if ((n_samples + NT - 1) / NT > 65535) return vgl_pack_set_error(VGL_E_ARG, "vgl_fetchgl_format_device: too many samples for one call");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_fetchgl_format_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_fetchgl_format_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    FetchArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.G = max_genotypes; A.a = a; A.b = b; A.mode = value_mode;
    A.site_status = site_status; A.n_alleles = n_alleles; A.a2b = alleles2acgt; A.gl = (const uint32_t*)gl;
    A.dst = dst; A.cap = dst_cap; A.off = offsets; A.ws = (uint32_t*)workspace;
    const bool sm = layout == VGL_LAYOUT_SAMPLE_MAJOR;
    const dim3 wgrid((unsigned)n_sites, (unsigned)((n_samples + NT - 1) / NT));
    if (sm) hipLaunchKernelGGL(k_fetchgl_plan<true>, dim3((unsigned)n_sites), dim3(NT), 0, st, A);
    else hipLaunchKernelGGL(k_fetchgl_plan<false>, dim3((unsigned)n_sites), dim3(NT), 0, st, A);
    if (vgl_text_scan_launch(n_sites, offsets, hip_stream)) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_fetchgl_format_device: a launch failed");
    if (sm) hipLaunchKernelGGL(k_fetchgl_write<true>, wgrid, dim3(NT), 0, st, A);
    else hipLaunchKernelGGL(k_fetchgl_write<false>, wgrid, dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_fetchgl_format_device: a launch failed");
    return VGL_OK;
}
