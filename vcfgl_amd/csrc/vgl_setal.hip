// vgl_setal.hip -- a prescribed REF/ALT list for every record of a tile, on the device (ABI 7 additions: vgl_setal_workspace_bytes,
// vgl_setal_apply_device).
// What misc/setAlleles does to a record file, done to the arrays of a tile before any writer reads them: INFO/QS, FORMAT/GL, PL, GP and
// the one-byte PL are re-indexed to the site's target list and renormalised (vgl_setal_core.h has the maps and the per-sample
// routines), n_alleles and alleles2acgt become the target's.  DP, I16, n_alleles_obs and the AD tags are not touched.
// A target entry is 8 bytes: [n_new (2 .. 5), a0 .. a4 (0 .. 4 = A, C, G, T, unobserved; -1 behind n_new), 2 pad].
//   k_setal_plan    one thread per site: the site's plan (vgl_setal::SitePlan, 32 bytes) into the workspace and the permuted QS.  A site
//                   with site_status < 0 gets n_new = 0 (left alone).  A target that is not 2 .. 5 distinct alleles which the record all
//                   has -- the tool's undefined case -- also gets n_new = 0, and the smallest such site index goes to *bad_site with
//                   one atomicMin per site.  So does a site whose old or new genotype count exceeds max_genotypes.
//   k_setal_apply   one launch per array (GL, PL, GP, the one-byte PL), one lane per (site, sample): the lane gathers its values in the
//                   new genotype order, normalises them and stores them.
//                   VGL_LAYOUT_PLANES  x[(i G + g) N + s] in place: a lane touches only its own column s, it has loaded all its
//                     old values before its first store, and 64 lanes of a wavefront read and write 64 consecutive elements of a
//                     plane.  Planes g >= nG_new get the missing pattern.
//                   VGL_LAYOUT_SAMPLE_MAJOR  x[i G N + s nG(i) + g]: the per-sample stride changes from nG_old to nG_new, so one
//                     sample's new place is another's old one -- not in place.  A workgroup takes CH consecutive samples: their old
//                     values are one contiguous run, loaded into LDS with consecutive lanes on consecutive elements; every lane picks
//                     its values out of LDS, normalises, and puts them back at the new stride; the run goes out as contiguous
//                     stores into the workspace, at the place it will have in the array.
//   k_setal_copy    VGL_LAYOUT_SAMPLE_MAJOR: the new runs (N nG_new elements of every changed site) from the workspace back into the array
//   k_setal_commit  one thread per site, behind the last array: n_alleles and alleles2acgt from the plan
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_setal_core.h"

namespace {

namespace sa = vgl_setal;

constexpr int NT = 256;                 // lanes per workgroup
constexpr int CH = 256;                 // samples of a workgroup's LDS chunk (sample-major)
enum { KIND_GL = 0, KIND_PL = 1, KIND_GP = 2, KIND_U8 = 3 };

struct SetalArgs {
    int32_t N, n_sites, G, A, kind;
    const int8_t* targets;              // [n_sites][8]
    const int32_t* site_status;
    int32_t* n_alleles;
    int8_t* a2b;                        // alleles2acgt [n_sites][5]
    float* qs;                          // [n_sites][A] or NULL
    const int32_t* fmt_dp;              // [n_sites][N] (KIND_U8)
    void* x;                            // the array of this launch
    void* out;                          // sample-major: the workspace array
    int32_t* bad_site;
    sa::SitePlan* plan;
};

__device__ __forceinline__ uint32_t load_elem(const void* p, size_t at, bool u8) {
    return u8 ? (uint32_t)((const uint8_t*)p)[at] : ((const uint32_t*)p)[at];
}
__device__ __forceinline__ void store_elem(void* p, size_t at, uint32_t v, bool u8) {
    if (u8) ((uint8_t*)p)[at] = (uint8_t)v; else ((uint32_t*)p)[at] = v;
}
__device__ __forceinline__ uint32_t missing_of(int kind) {
    return kind == KIND_PL ? (uint32_t)sa::INT32_MISSING_BITS : kind == KIND_U8 ? (uint32_t)sa::U8_MISSING : (uint32_t)sa::FLOAT_MISSING_BITS;
}
__device__ __forceinline__ void normalise(uint32_t* v, int n, int kind, bool u8_missing) {
    if (kind == KIND_GL) sa::norm_gl(v, n);
    else if (kind == KIND_PL) sa::norm_pl(v, n);
    else if (kind == KIND_GP) sa::norm_gp(v, n);
    else sa::norm_pl_u8(v, n, u8_missing);
}

__global__ __launch_bounds__(NT) void k_setal_plan(SetalArgs A) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= A.n_sites) return;
    sa::SitePlan P;
    memset(&P, 0xFF, sizeof P);
    P.n_new = 0; P.n_old = 0;
    if (A.site_status[i] >= 0) {
        int8_t old[sa::MAX_A], entry[8];
#pragma unroll
        for (int k = 0; k < sa::MAX_A; ++k) old[k] = A.a2b[(size_t)i * 5 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) entry[k] = A.targets[(size_t)i * 8 + k];
        const int n_old = A.n_alleles[i];
        bool ok = sa::site_plan(old, n_old, entry, P);
        if (ok && (n_old * (n_old + 1) / 2 > A.G || P.n_new * (P.n_new + 1) / 2 > A.G || P.n_new > A.A)) { ok = false; P.n_new = 0; }
        if (!ok) atomicMin(A.bad_site, (int32_t)i);
        else if (A.qs) {
            float q[sa::MAX_A];
#pragma unroll
            for (int a = 0; a < sa::MAX_A; ++a) q[a] = a < A.A ? A.qs[(size_t)i * A.A + a] : 0.0f;
#pragma unroll
            for (int j = 0; j < sa::MAX_A; ++j) {
                const int src = P.qs_src[j];
                float v = q[0];
#pragma unroll
                for (int a = 1; a < sa::MAX_A; ++a) v = src == a ? q[a] : v;
                if (j < P.n_new) A.qs[(size_t)i * A.A + j] = v;
            }
        }
    }
    A.plan[i] = P;
}

// VGL_LAYOUT_PLANES in place
__device__ __forceinline__ void apply_planes(const SetalArgs& A) {
    const int64_t i = blockIdx.x;
    const int s = blockIdx.y * NT + threadIdx.x;
    const sa::SitePlan P = A.plan[i];
    if (P.n_new == 0 || s >= A.N) return;
    const bool u8 = A.kind == KIND_U8;
    const int nGn = P.n_new * (P.n_new + 1) / 2;
    const size_t base = (size_t)i * A.G * A.N + (size_t)s;
    const uint32_t miss = missing_of(A.kind);
    uint32_t v[sa::MAX_G];
#pragma unroll
    for (int g = 0; g < sa::MAX_G; ++g) {
        v[g] = miss;
        if (g < nGn) { const int src = P.new2old[g]; if (src >= 0) v[g] = load_elem(A.x, base + (size_t)src * A.N, u8); }
    }
    const bool u8_missing = u8 && A.fmt_dp[(size_t)i * A.N + s] == 0;
    normalise(v, nGn, A.kind, u8_missing);
#pragma unroll
    for (int g = 0; g < sa::MAX_G; ++g)
        if (g < A.G) store_elem(A.x, base + (size_t)g * A.N, v[g], u8);
}

// VGL_LAYOUT_SAMPLE_MAJOR through LDS into the workspace array
__device__ __forceinline__ void apply_sm(const SetalArgs& A) {
    __shared__ uint32_t buf[CH * sa::MAX_G];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x;
    const sa::SitePlan P = A.plan[i];
    if (P.n_new == 0) return;
    const bool u8 = A.kind == KIND_U8;
    const int nGo = P.n_old * (P.n_old + 1) / 2, nGn = P.n_new * (P.n_new + 1) / 2;
    const int s0 = blockIdx.y * CH;
    const int cnt = A.N - s0 < CH ? A.N - s0 : CH;
    const size_t slab = (size_t)i * A.G * A.N;
    const size_t in0 = slab + (size_t)s0 * nGo, out0 = slab + (size_t)s0 * nGn;
    for (int k = tid; k < cnt * nGo; k += NT) buf[k] = load_elem(A.x, in0 + k, u8);
    __syncthreads();
    const uint32_t miss = missing_of(A.kind);
    uint32_t v[sa::MAX_G];
    if (tid < cnt) {
#pragma unroll
        for (int g = 0; g < sa::MAX_G; ++g) {
            v[g] = miss;
            if (g < nGn) { const int src = P.new2old[g]; if (src >= 0 && src < nGo) v[g] = buf[tid * nGo + src]; }
        }
        const bool u8_missing = u8 && A.fmt_dp[(size_t)i * A.N + s0 + tid] == 0;
        normalise(v, nGn, A.kind, u8_missing);
    }
    __syncthreads();
    if (tid < cnt) {
#pragma unroll
        for (int g = 0; g < sa::MAX_G; ++g)
            if (g < nGn) buf[tid * nGn + g] = v[g];
    }
    __syncthreads();
    for (int k = tid; k < cnt * nGn; k += NT) store_elem(A.out, out0 + k, buf[k], u8);
}

// grid (n_sites, ceil(N / CH)), NT = CH: one lane per (site, sample)
template <bool SM>
__global__ __launch_bounds__(NT) void k_setal_apply(SetalArgs A) {
    if (SM) apply_sm(A); else apply_planes(A);
}

// grid (n_sites, ceil(N / CH)): the new runs from the workspace array back into the array
__global__ __launch_bounds__(NT) void k_setal_copy(SetalArgs A) {
    const int64_t i = blockIdx.x;
    const int n_new = A.plan[i].n_new;
    if (n_new == 0) return;
    const bool u8 = A.kind == KIND_U8;
    const int nGn = n_new * (n_new + 1) / 2;
    const int s0 = blockIdx.y * CH;
    const int cnt = A.N - s0 < CH ? A.N - s0 : CH;
    const size_t at0 = (size_t)i * A.G * A.N + (size_t)s0 * nGn;
    for (int k = threadIdx.x; k < cnt * nGn; k += NT) store_elem(A.x, at0 + k, load_elem(A.out, at0 + k, u8), u8);
}

__global__ __launch_bounds__(NT) void k_setal_commit(SetalArgs A) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= A.n_sites) return;
    const sa::SitePlan P = A.plan[i];
    if (P.n_new == 0) return;
    A.n_alleles[i] = P.n_new;
#pragma unroll
    for (int k = 0; k < sa::MAX_A; ++k) A.a2b[(size_t)i * 5 + k] = P.a2b_new[k];
}

constexpr int64_t PLAN_ALIGN = 256;
int64_t plan_bytes(int64_t n_sites) { return (n_sites * (int64_t)sizeof(sa::SitePlan) + PLAN_ALIGN - 1) / PLAN_ALIGN * PLAN_ALIGN; }

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_setal_workspace_bytes(int32_t n_samples, int32_t n_sites, int32_t max_genotypes) {
    if (n_samples < 0 || n_sites < 0 || max_genotypes < 0) return -1;
    int64_t r;
    if (__builtin_mul_overflow((int64_t)n_samples * n_sites, (int64_t)max_genotypes * (int64_t)sizeof(uint32_t), &r)) return -1;
    return plan_bytes(n_sites) + r;
}

extern "C" int vgl_setal_apply_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t max_alleles, int32_t layout,
                                      const int8_t* targets, const int32_t* site_status, int32_t* n_alleles, int8_t* alleles2acgt, float* qs,
                                      const int32_t* fmt_dp, float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site,
                                      void* workspace, int64_t workspace_bytes, void* hip_stream) {
    static_assert(sizeof(sa::SitePlan) == 32, "SitePlan is 32 bytes");
    if (n_samples <= 0 || n_sites < 0 || max_genotypes < 1 || max_genotypes > 15 || max_alleles < 1 || max_alleles > 5)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: bad n_samples, n_sites, max_genotypes or max_alleles");
    if (layout != VGL_LAYOUT_PLANES && layout != VGL_LAYOUT_SAMPLE_MAJOR)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: layout must be VGL_LAYOUT_PLANES or VGL_LAYOUT_SAMPLE_MAJOR");
    if (n_sites == 0) return VGL_OK;
    if (!targets || !site_status || !n_alleles || !alleles2acgt || !bad_site) return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: null argument");
    if (pl_u8 && !fmt_dp) return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: pl_u8 needs fmt_dp (a sample without reads is told by fmt_dp == 0)");
    const int64_t need = vgl_setal_workspace_bytes(n_samples, n_sites, max_genotypes);
    if (need < 0 || !workspace || workspace_bytes < need)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: workspace smaller than vgl_setal_workspace_bytes()");
    const unsigned chunks = (unsigned)((n_samples + CH - 1) / CH);
    if (chunks > 65535u) return vgl_pack_set_error(VGL_E_ARG, "vgl_setal_apply_device: too many samples for one call");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_setal_apply_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    SetalArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.G = max_genotypes; A.A = max_alleles;
    A.targets = targets; A.site_status = site_status; A.n_alleles = n_alleles; A.a2b = alleles2acgt; A.qs = qs; A.fmt_dp = fmt_dp;
    A.bad_site = bad_site; A.plan = (sa::SitePlan*)workspace; A.out = (char*)workspace + plan_bytes(n_sites);
    const dim3 sgrid((unsigned)((n_sites + NT - 1) / NT)), egrid((unsigned)n_sites, chunks);
    static_assert(NT == CH, "one grid shape for both layouts");
    hipLaunchKernelGGL(k_setal_plan, sgrid, dim3(NT), 0, st, A);
    void* const arrays[4] = {gl, pl, gp, pl_u8};
    for (int kind = 0; kind < 4; ++kind) {
        if (!arrays[kind]) continue;
        A.kind = kind; A.x = arrays[kind];
        if (layout == VGL_LAYOUT_SAMPLE_MAJOR) {
            hipLaunchKernelGGL(k_setal_apply<true>, egrid, dim3(NT), 0, st, A);
            hipLaunchKernelGGL(k_setal_copy, egrid, dim3(NT), 0, st, A);
        } else hipLaunchKernelGGL(k_setal_apply<false>, egrid, dim3(NT), 0, st, A);
    }
    hipLaunchKernelGGL(k_setal_commit, sgrid, dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_setal_apply_device: a launch failed");
    return VGL_OK;
}
