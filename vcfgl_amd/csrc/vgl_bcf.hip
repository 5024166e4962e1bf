// vgl_bcf.hip -- the FORMAT part of a tile's BCF records on the device (ABI 7 additions: vgl_bcf_bound, vgl_bcf_workspace_bytes,
// vgl_bcf_encode_device).
// For every site i with site_status[i] >= 0 the output is exactly what the host writer (host/vcf_sink.h, Sink::encode_rec, binary
// branch) puts into a record's `indiv` block: for each field, in the order given,
//     enc_int1(key_id)                     0x11 id | 0x12 id16 | 0x13 id32 (the smallest integer type that holds the id)
//     size/type                            (n << 4 | bt) for n < 15, (0xF0 | bt) enc_int1(n) for n >= 15, bt alone for n = 0
//     n(i) * N values                      bt = int8 / int16 / int32 (the narrowest that holds the record's range, missing and
//                                          vector-end values left out: int8 when max <= 127 and min >= -120, int16 when max <= 32767 and
//                                          min >= -32760) or float32 (bit patterns untouched); little endian
// A skipped site (site_status < 0) produces no bytes.  The input is the tile's FORMAT arrays in VGL_LAYOUT_SAMPLE_MAJOR: value k of
// sample s of site i at base[i * site_stride + s * n(i) + k] -- the slab of a site is the array BCF stores, so both passes read it front
// to back.  Three passes, the shape of vgl_text (plan, scan, write):
//   k_bcf_plan    one workgroup per site: min / max of every integer field (16-byte loads behind an aligning head), the field's type
//                 code into the workspace (int32 per (site, field)), the site's length into offsets[i]
//   k_text_scan   (vgl_text.hip) exclusive prefix sum of the site lengths -> offsets[0 .. n_sites], offsets[n_sites] = the total
//   k_bcf_write   grid (n_sites, slices): the field headers byte by byte, the values as whole 32-bit words wherever the destination
//                 is word aligned (a site starts at any byte: a head and a tail of single bytes per field); every store is bounded by
//                 the site's own end; nothing is written when the total exceeds dst_cap
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"

namespace {

constexpr int NT = 256;                 // lanes per workgroup
constexpr int MAX_SLICES = 64;          // workgroups that share one site in k_bcf_write
constexpr int32_t I32_VEND = INT32_MIN + 1;
enum { BT_INT8 = 1, BT_INT16 = 2, BT_INT32 = 3, BT_FLOAT = 5 };

struct BcfArgs {
    int32_t nf, N, n_sites, pad;
    const int32_t* base[VGL_TEXT_MAX_FIELDS];       // float fields are copied as bit patterns
    int64_t stride[VGL_TEXT_MAX_FIELDS];
    int32_t count[VGL_TEXT_MAX_FIELDS];
    int32_t is_float[VGL_TEXT_MAX_FIELDS];
    int32_t key[VGL_TEXT_MAX_FIELDS];
    const int32_t* site_status;
    const int32_t* n_alleles;
    uint8_t* dst;
    int64_t cap;
    int64_t* off;
    int32_t* ws;                                    // [n_sites][VGL_TEXT_MAX_FIELDS] type codes
};

__host__ __device__ inline int int1_len(int32_t v) { return v <= 127 ? 2 : v <= 32767 ? 3 : 5; }
__host__ __device__ inline int size_len(int32_t n) { return n < 15 ? 1 : 1 + int1_len(n); }
__host__ __device__ inline int width_of(int bt) { return bt == BT_INT8 ? 1 : bt == BT_INT16 ? 2 : 4; }

__device__ int values_of(const BcfArgs& A, int f, int nA) {
    const int c = A.count[f];
    int n = c == VGL_TEXT_PER_G ? nA * (nA + 1) / 2 : c == VGL_TEXT_PER_A ? nA : 1;
    const int64_t fit = A.N > 0 ? A.stride[f] / A.N : 0;    // never read past the site's slab
    if (n > fit) n = (int)fit;
    return n < 0 ? 0 : n;
}

// a field's header (at most 11 bytes) in two registers
struct Hdr { uint64_t lo, hi; int len; };
__device__ void push(Hdr& h, uint64_t v, int nb) {          // nb <= 5
    if (h.len < 8) { h.lo |= v << (8 * h.len); if (h.len + nb > 8) h.hi |= v >> (8 * (8 - h.len)); }
    else h.hi |= v << (8 * (h.len - 8));
    h.len += nb;
}
__device__ void push_int1(Hdr& h, int32_t v) {
    if (v <= 127) push(h, 0x11u | (uint64_t)(uint32_t)v << 8, 2);
    else if (v <= 32767) push(h, 0x12u | (uint64_t)(uint32_t)v << 8, 3);
    else push(h, 0x13u | (uint64_t)(uint32_t)v << 8, 5);
}
__device__ Hdr header_of(int32_t key, int n, int bt) {
    Hdr h{0, 0, 0};
    push_int1(h, key);
    if (n < 15) push(h, (uint64_t)(n << 4 | bt), 1);
    else { push(h, (uint64_t)(0xF0 | bt), 1); push_int1(h, n); }
    return h;
}

__device__ inline void acc(int32_t v, int32_t& mn, int32_t& mx) {
    if (v == VGL_INT32_MISSING || v == I32_VEND) return;
    mn = v < mn ? v : mn; mx = v > mx ? v : mx;
}

__global__ __launch_bounds__(NT) void k_bcf_plan(BcfArgs A) {
    __shared__ int32_t s_mn[VGL_TEXT_MAX_FIELDS][NT / 64], s_mx[VGL_TEXT_MAX_FIELDS][NT / 64];
    __shared__ int64_t s_len[VGL_TEXT_MAX_FIELDS];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (A.site_status[i] < 0) { if (tid == 0) A.off[i] = 0; return; }
    const int nA = A.n_alleles[i];
    for (int f = 0; f < A.nf; ++f) {
        if (A.is_float[f]) continue;
        const int64_t total = (int64_t)values_of(A, f, nA) * A.N;
        const int32_t* p = A.base[f] + i * A.stride[f];
        int32_t mn = INT32_MAX, mx = INT32_MIN;
        int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);    // values in front of the first 16-byte boundary
        if (head > total) head = total;
        const int64_t nvec = (total - head) >> 2;
        if (tid < head) acc(p[tid], mn, mx);
        const int4* q = (const int4*)(p + head);
        for (int64_t v = tid; v < nvec; v += NT) { const int4 x = q[v]; acc(x.x, mn, mx); acc(x.y, mn, mx); acc(x.z, mn, mx); acc(x.w, mn, mx); }
        const int64_t t = head + 4 * nvec + tid;
        if (t < total) acc(p[t], mn, mx);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int32_t a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
            mn = a < mn ? a : mn; mx = b > mx ? b : mx;
        }
        if (lane == 0) { s_mn[f][wv] = mn; s_mx[f][wv] = mx; }
    }
    __syncthreads();
    if (tid < A.nf) {
        const int f = tid;
        int bt = BT_FLOAT;
        if (!A.is_float[f]) {
            int32_t mn = INT32_MAX, mx = INT32_MIN;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) { const int32_t a = s_mn[f][w], b = s_mx[f][w]; mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
            bt = (mx <= 127 && mn >= -120) ? BT_INT8 : (mx <= 32767 && mn >= -32760) ? BT_INT16 : BT_INT32;
        }
        const int n = values_of(A, f, nA);
        A.ws[i * VGL_TEXT_MAX_FIELDS + f] = bt;
        s_len[f] = int1_len(A.key[f]) + size_len(n) + (int64_t)n * A.N * width_of(bt);
    }
    __syncthreads();
    if (tid == 0) { int64_t L = 0; for (int f = 0; f < A.nf; ++f) L += s_len[f]; A.off[i] = L; }
}

template <int W>
__device__ inline uint32_t enc(int32_t v) {
    if (W == 1) return v == VGL_INT32_MISSING ? 0x80u : v == I32_VEND ? 0x81u : ((uint32_t)v & 0xffu);
    if (W == 2) return v == VGL_INT32_MISSING ? 0x8000u : v == I32_VEND ? 0x8001u : ((uint32_t)v & 0xffffu);
    return (uint32_t)v;
}
// bytes j .. j + 3 of a field's value array (all four inside it), as one little-endian word
template <int W>
__device__ inline uint32_t word_at(const int32_t* src, int64_t j) {
    if (W == 1) return enc<1>(src[j]) | enc<1>(src[j + 1]) << 8 | enc<1>(src[j + 2]) << 16 | enc<1>(src[j + 3]) << 24;
    if (W == 2) {
        const int64_t k = j >> 1;
        if (!(j & 1)) return enc<2>(src[k]) | enc<2>(src[k + 1]) << 16;
        return enc<2>(src[k]) >> 8 | enc<2>(src[k + 1]) << 8 | (enc<2>(src[k + 2]) & 0xffu) << 24;
    }
    const int64_t k = j >> 2; const int r = (int)(j & 3);
    if (r == 0) return (uint32_t)src[k];
    return (uint32_t)src[k] >> (8 * r) | (uint32_t)src[k + 1] << (32 - 8 * r);
}
template <int W>
__device__ inline uint8_t byte_at(const int32_t* src, int64_t j) {
    if (W == 1) return (uint8_t)enc<1>(src[j]);
    if (W == 2) return (uint8_t)(enc<2>(src[j >> 1]) >> (8 * (j & 1)));
    return (uint8_t)((uint32_t)src[j >> 2] >> (8 * (j & 3)));
}

// `nbytes` bytes of values at o (which ends at `end`): single bytes up to the first word boundary, whole words, single bytes again
template <int W>
__device__ void put_values(const int32_t* src, uint8_t* o, const uint8_t* end, int64_t nbytes, int64_t g, int64_t step) {
    if (o + nbytes > end) nbytes = end > o ? end - o : 0;   // (the plan's lengths come from the same values: never taken)
    int64_t head = (int64_t)((4u - (uint32_t)((uintptr_t)o & 3u)) & 3u);
    if (head > nbytes) head = nbytes;
    const int64_t nw = (nbytes - head) >> 2;
    if (g < head) o[g] = byte_at<W>(src, g);
    uint32_t* ow = (uint32_t*)(o + head);
    for (int64_t w = g; w < nw; w += step) ow[w] = word_at<W>(src, head + 4 * w);
    const int64_t t = head + 4 * nw + g;
    if (t < nbytes) o[t] = byte_at<W>(src, t);
}

__global__ __launch_bounds__(NT) void k_bcf_write(BcfArgs A) {
    const int64_t i = blockIdx.x;
    if (A.off[A.n_sites] > A.cap) return;                   // does not fit: nothing is written
    if (A.site_status[i] < 0) return;
    const int64_t g = (int64_t)blockIdx.y * NT + threadIdx.x, step = (int64_t)gridDim.y * NT;
    uint8_t* o = A.dst + A.off[i];
    const uint8_t* end = A.dst + A.off[i + 1];
    const int nA = A.n_alleles[i];
    for (int f = 0; f < A.nf; ++f) {
        const int n = values_of(A, f, nA), bt = A.ws[i * VGL_TEXT_MAX_FIELDS + f], w = width_of(bt);
        const Hdr h = header_of(A.key[f], n, bt);
        if (g < h.len && o + g < end) o[g] = (uint8_t)(g < 8 ? h.lo >> (8 * g) : h.hi >> (8 * (g - 8)));
        o += h.len;
        const int64_t nbytes = (int64_t)n * A.N * w;
        const int32_t* src = A.base[f] + i * A.stride[f];
        if (w == 1) put_values<1>(src, o, end, nbytes, g, step);
        else if (w == 2) put_values<2>(src, o, end, nbytes, g, step);
        else put_values<4>(src, o, end, nbytes, g, step);
        o += nbytes;
    }
}

int64_t max_values(int32_t count, int32_t max_alleles) {
    return count == VGL_TEXT_PER_G ? (int64_t)max_alleles * (max_alleles + 1) / 2 : count == VGL_TEXT_PER_A ? max_alleles : 1;
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()
extern "C" int vgl_text_scan_launch(int32_t n_sites, int64_t* offsets, void* hip_stream);   // vgl_text.hip (k_text_scan)

extern "C" int64_t vgl_bcf_bound(int32_t n_samples, int32_t n_sites, const vgl_bcf_field* fields, int32_t n_fields, int32_t max_alleles) {
    if (n_samples < 0 || n_sites < 0 || n_fields < 0 || n_fields > VGL_TEXT_MAX_FIELDS || (n_fields > 0 && !fields) || max_alleles < 1 || max_alleles > 5) return -1;
    int64_t per_site = 0;
    for (int k = 0; k < n_fields; ++k) {
        if (fields[k].key_id < 0 || fields[k].count < VGL_TEXT_ONE || fields[k].count > VGL_TEXT_PER_A) return -1;
        const int64_t n = max_values(fields[k].count, max_alleles);
        per_site += int1_len(fields[k].key_id) + size_len((int32_t)n) + n * n_samples * 4;
    }
    return (int64_t)n_sites * per_site;
}

extern "C" int64_t vgl_bcf_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    return (int64_t)n_sites * VGL_TEXT_MAX_FIELDS * (int64_t)sizeof(int32_t);
}

extern "C" int vgl_bcf_encode_device(int32_t device, const vgl_bcf_field* fields, int32_t n_fields, int32_t n_samples, int32_t n_sites,
                                     const int32_t* site_status, const int32_t* n_alleles, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                     void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (n_samples < 0 || n_sites < 0 || n_fields < 0 || n_fields > VGL_TEXT_MAX_FIELDS || (n_fields > 0 && !fields) || dst_cap < 0)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_bcf_encode_device: bad argument");
    if (!offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcf_encode_device: null offsets");
    if (n_sites > 0 && (!site_status || !n_alleles || (dst_cap > 0 && !dst)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_bcf_encode_device: null argument");
    if (n_sites > 0 && (!workspace || workspace_bytes < vgl_bcf_workspace_bytes(n_samples, n_sites)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_bcf_encode_device: workspace smaller than vgl_bcf_workspace_bytes()");
    BcfArgs A;
    memset(&A, 0, sizeof A);
    A.nf = n_fields; A.N = n_samples; A.n_sites = n_sites;
    int64_t words = 0;                                      // 32-bit values of the widest site
    for (int k = 0; k < n_fields; ++k) {
        const vgl_bcf_field& F = fields[k];
        if (F.key_id < 0 || (n_sites > 0 && n_samples > 0 && !F.base) || ((uintptr_t)F.base & 3u) || F.count < VGL_TEXT_ONE || F.count > VGL_TEXT_PER_A || F.site_stride < 0)
            return vgl_pack_set_error(VGL_E_ARG, "vgl_bcf_encode_device: bad field descriptor");
        A.base[k] = (const int32_t*)F.base; A.stride[k] = F.site_stride; A.count[k] = F.count; A.is_float[k] = F.is_float ? 1 : 0; A.key[k] = F.key_id;
        words += max_values(F.count, 5) * n_samples;
    }
    A.site_status = site_status; A.n_alleles = n_alleles; A.dst = dst; A.cap = dst_cap; A.off = offsets; A.ws = (int32_t*)workspace;
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcf_encode_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcf_encode_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    hipLaunchKernelGGL(k_bcf_plan, dim3((unsigned)n_sites), dim3(NT), 0, st, A);
    if (vgl_text_scan_launch(n_sites, offsets, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcf_encode_device: a launch failed");
    // slices of a site: about four words per lane, so that a tile of few wide sites still fills the device
    int64_t slices = (words + (int64_t)NT * 16 - 1) / ((int64_t)NT * 16);
    slices = slices < 1 ? 1 : slices > MAX_SLICES ? MAX_SLICES : slices;
    hipLaunchKernelGGL(k_bcf_write, dim3((unsigned)n_sites, (unsigned)slices), dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcf_encode_device: a launch failed");
    return VGL_OK;
}
