// vgl_text.hip -- VCF text of the sample columns of a tile's records on the device (ABI 7 additions: vgl_text_bound,
// vgl_text_workspace_bytes, vgl_text_format_device).
// For every site i with site_status[i] >= 0 the output is exactly what the host writer (host/vcf_sink.h, Sink::encode_rec, text
// branch) appends behind the eight fixed columns:
//     "\t" KEYS ( "\t" sample_0 ) ... ( "\t" sample_{N-1} ) "\n"
// KEYS = the FORMAT keys joined by ':' ("." without fields), a sample column = its fields joined by ':', a field's values by ','.
// A skipped site (site_status < 0) produces no bytes.  The input is the tile's FORMAT arrays in VGL_LAYOUT_SAMPLE_MAJOR: value k of
// sample s of site i at base[i * site_stride + s * n(i) + k], n(i) = 1, nG(i) = nA (nA + 1) / 2 or nA(i) = n_alleles[i].
// Three passes, the shape of vgl_pack / vgl_bgzf (plan, scan, write):
//   k_text_plan   one workgroup per site: every lane formats its sample's column without storing it (the length), a workgroup scan
//                 gives each column's offset inside the site (workspace, uint32 per (site, sample)) and the site's length
//   k_text_scan   one workgroup: exclusive prefix sum of the site lengths -> offsets[0 .. n_sites], offsets[n_sites] = total
//   k_text_write  one lane per (site, sample): the same formatter again, storing at its offset; nothing is written when the total
//                 exceeds dst_cap (the caller reads offsets[n_sites] to learn the size it needs)
// Number formatting follows the host program's formatter (vcfgl_main.cpp put_float / put_int, htslib's kputd) byte for byte:
//   int32   VGL_INT32_MISSING -> ".", otherwise %d
//   float32 VGL_FLOAT_MISSING_BITS -> ".", other NaN -> "nan", +-0 -> "0" / "-0", the sign of a negative value first; then
//           [1e-4, 999999]: kputd's integer form (uint64_t)(d * 1e10) plus half a unit of the 6th significant digit, 6 digits, trailing
//           zeros stripped; outside it (infinity included) glibc's %g -- the exact binary value correctly rounded to 6 significant
//           digits, ties to even (exact multi-word integer arithmetic: a float is m 2^e with m < 2^24 and e in [-149, 104], so 256 bits
//           hold every product below), trailing zeros stripped, an exponent of at least two digits.
// Bytes are written with ordinary byte stores, each lane inside its own column.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/vcfgl_hip.h"

namespace {

constexpr int NT = 256;                 // lanes per workgroup (plan: one workgroup per site, samples in chunks of NT)
constexpr int SCAN_NT = 1024;
constexpr int HDR_MAX = 128;            // "\t" + keys joined by ':'

struct TextArgs {
    int32_t nf, N, n_sites, hdr_len;
    const void* base[VGL_TEXT_MAX_FIELDS];
    int64_t stride[VGL_TEXT_MAX_FIELDS];
    int32_t count[VGL_TEXT_MAX_FIELDS];
    int32_t is_float[VGL_TEXT_MAX_FIELDS];
    const int32_t* site_status;
    const int32_t* n_alleles;
    uint8_t* dst;
    int64_t cap;
    int64_t* off;
    uint32_t* ws;
    char hdr[HDR_MAX];
};

// byte sink of one column: W = false counts only; W = true stores, never at or past `lim`
template <bool W>
struct Emit {
    uint8_t* p;
    uint32_t n, lim;
    __device__ void put(char c) { if (W && n < lim) p[n] = (uint8_t)c; n++; }
    __device__ void put_at(uint32_t at, char c) { if (W && at < lim) p[at] = (uint8_t)c; }
};

__device__ int ndig32(uint32_t u) {
    int n = 1;
    if (u >= 10u) n = 2; if (u >= 100u) n = 3; if (u >= 1000u) n = 4; if (u >= 10000u) n = 5;
    if (u >= 100000u) n = 6; if (u >= 1000000u) n = 7; if (u >= 10000000u) n = 8; if (u >= 100000000u) n = 9; if (u >= 1000000000u) n = 10;
    return n;
}

template <bool W>
__device__ void fmt_int(Emit<W>& e, int32_t v) {
    if (v == VGL_INT32_MISSING) { e.put('.'); return; }
    uint32_t u = (uint32_t)v;
    if (v < 0) { e.put('-'); u = 0u - u; }
    const int L = ndig32(u);
    if (W) { uint32_t x = u; for (int j = L - 1; j >= 0; --j) { e.put_at(e.n + (uint32_t)j, (char)('0' + x % 10u)); x /= 10u; } }
    e.n += (uint32_t)L;
}

// ---- exact 256-bit unsigned integers (8 x 32-bit limbs, little endian; every index a constant after unrolling) ------------------
struct Big { uint32_t w[8]; };

__device__ void big_mul_small(Big& a, uint32_t c) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const uint64_t t = (uint64_t)a.w[j] * c + carry; a.w[j] = (uint32_t)t; carry = t >> 32; }
}
__device__ void big_mul_pow10(Big& a, int p) {
    for (; p >= 9; p -= 9) big_mul_small(a, 1000000000u);
    uint32_t m = 1; for (int r = 0; r < p; ++r) m *= 10u;
    big_mul_small(a, m);
}
__device__ void big_mul_pow5(Big& a, int p) {
    for (; p >= 13; p -= 13) big_mul_small(a, 1220703125u);
    uint32_t m = 1; for (int r = 0; r < p; ++r) m *= 5u;
    big_mul_small(a, m);
}
__device__ uint32_t big_div10(Big& a) {                      // a /= 10, returns the remainder
    uint64_t rem = 0;
#pragma unroll
    for (int j = 7; j >= 0; --j) { const uint64_t cur = (rem << 32) | a.w[j]; a.w[j] = (uint32_t)(cur / 10u); rem = cur % 10u; }
    return (uint32_t)rem;
}
__device__ void big_shl(Big& a, int s) {
    for (; s >= 32; s -= 32) {
#pragma unroll
        for (int j = 7; j > 0; --j) a.w[j] = a.w[j - 1];
        a.w[0] = 0;
    }
    if (s > 0) {
#pragma unroll
        for (int j = 7; j > 0; --j) a.w[j] = (a.w[j] << s) | (a.w[j - 1] >> (32 - s));
        a.w[0] <<= s;
    }
}
// a >>= s; returns whether a nonzero bit was shifted out
__device__ bool big_shr_sticky(Big& a, int s) {
    bool sticky = false;
    for (; s >= 32; s -= 32) {
        sticky |= a.w[0] != 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) a.w[j] = a.w[j + 1];
        a.w[7] = 0;
    }
    if (s > 0) {
        sticky |= (a.w[0] & ((1u << s) - 1u)) != 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) a.w[j] = (a.w[j] >> s) | (a.w[j + 1] << (32 - s));
        a.w[7] >>= s;
    }
    return sticky;
}
__device__ uint32_t big_low_or_huge(const Big& a) {       // the value when it fits 32 bits, else 0xffffffff
    uint32_t hi = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) hi |= a.w[j];
    return hi ? 0xffffffffu : a.w[0];
}

enum { BELOW = 0, HALF = 1, ABOVE = 2 };

// floor(m 2^e / 10^k) (0xffffffff when it does not fit 32 bits) and where the remainder lies against half a unit
__device__ void scaled(uint32_t m, int e, int k, uint32_t& fl, int& cls) {
    Big a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a.w[j] = 0;
    a.w[0] = m;
    if (k < 0) {                                            // m 10^-k / 2^-e
        big_mul_pow10(a, -k);
        int sh = -e;
        if (sh <= 0) { big_shl(a, -sh); fl = big_low_or_huge(a); cls = BELOW; return; }
        const bool sticky = big_shr_sticky(a, sh - 1);      // one bit more than the quotient: the half bit
        const uint32_t half = a.w[0] & 1u;
        big_shr_sticky(a, 1);
        fl = big_low_or_huge(a);
        cls = half ? (sticky ? ABOVE : HALF) : BELOW;
        return;
    }
    int t = k;                                               // m 2^e = a / 10^t with a an integer
    if (e >= 0) big_shl(a, e);
    else { big_mul_pow5(a, -e); t = k - e; }
    bool sticky = false;
    uint32_t last = 0;
    for (int r = 0; r < t; ++r) { if (r) sticky |= last != 0; last = big_div10(a); }
    fl = big_low_or_huge(a);
    cls = (last > 5u || (last == 5u && sticky)) ? ABOVE : (last == 5u ? HALF : BELOW);
}

// the 6 significant digits q (100000 .. 999999) and decimal exponent X (value ~ q 10^(X - 5)) of %g for a finite positive float
__device__ void g_digits(uint32_t a, double d, uint32_t& q, int& X) {
    const uint32_t ef = a >> 23, fr = a & 0x7fffffu;
    const uint32_t m = ef ? (fr | 0x800000u) : fr;
    const int e = ef ? (int)ef - 150 : -149;
    int E = (int)floor(log10(d));
    uint32_t fl = 0; int cls = BELOW;
    for (int it = 0; it < 6; ++it) {                        // the estimate is off by at most one near powers of ten
        scaled(m, e, E - 5, fl, cls);
        if (fl >= 1000000u) { E++; continue; }
        if (fl < 100000u) { E--; continue; }
        break;
    }
    q = fl + ((cls == ABOVE || (cls == HALF && (fl & 1u))) ? 1u : 0u);
    if (q == 1000000u) { q = 100000u; E++; }
    X = E;
}

// kputd: (uint64_t)(d * 1e10) plus half a unit of the 6th significant digit (one double multiply: nothing to contract)
__device__ void kputd_digits(double d, uint32_t& q, int& X) {
    uint64_t i = (uint64_t)(d * 10000000000.0);
    if (d < 0.001) i += 5; else if (d < 0.01) i += 50; else if (d < 0.1) i += 500;
    else if (d < 1) i += 5000; else if (d < 10) i += 50000; else if (d < 100) i += 500000; else if (d < 1000) i += 5000000;
    else if (d < 10000) i += 50000000; else if (d < 100000) i += 500000000; else i += 5000000000ULL;
    int n = 1;
    for (uint64_t p = 10; n < 20 && i >= p; p *= 10) n++;   // decimal digits of i (7 .. 16 here)
    for (int j = n; j > 6; --j) i /= 10u;
    q = (uint32_t)i;
    X = n - 11;
}

template <bool W>
__device__ void fmt_float(Emit<W>& e, uint32_t bits) {
    if (bits == VGL_FLOAT_MISSING_BITS) { e.put('.'); return; }
    const uint32_t a = bits & 0x7fffffffu;
    if (a > 0x7f800000u) { e.put('n'); e.put('a'); e.put('n'); return; }
    if (bits >> 31) e.put('-');
    if (a == 0) { e.put('0'); return; }
    if (a == 0x7f800000u) { e.put('i'); e.put('n'); e.put('f'); return; }
    const double d = (double)__uint_as_float(a);
    uint32_t q; int X;
    if (d >= 0.0001 && d <= 999999) kputd_digits(d, q, X);
    else g_digits(a, d, q, X);
    uint32_t D[6];
    uint32_t t = q;
#pragma unroll
    for (int j = 5; j >= 0; --j) { D[j] = t % 10u; t /= 10u; }
    int sd = 6;                                             // significant digits left after stripping trailing zeros
#pragma unroll
    for (int j = 5; j >= 1; --j) if (sd == j + 1 && D[j] == 0) sd = j;
    if (X >= -4 && X <= 5) {                                // fixed notation (kputd always; %g at its decade boundaries)
        if (X >= 0) {
#pragma unroll
            for (int j = 0; j < 6; ++j) if (j <= X) e.put((char)('0' + D[j]));
            if (sd > X + 1) {
                e.put('.');
#pragma unroll
                for (int j = 1; j < 6; ++j) if (j > X && j < sd) e.put((char)('0' + D[j]));
            }
        } else {
            e.put('0'); e.put('.');
            for (int z = 0; z < -X - 1; ++z) e.put('0');
#pragma unroll
            for (int j = 0; j < 6; ++j) if (j < sd) e.put((char)('0' + D[j]));
        }
        return;
    }
    e.put((char)('0' + D[0]));
    if (sd > 1) {
        e.put('.');
#pragma unroll
        for (int j = 1; j < 6; ++j) if (j < sd) e.put((char)('0' + D[j]));
    }
    e.put('e'); e.put(X < 0 ? '-' : '+');
    const int ax = X < 0 ? -X : X;
    if (ax >= 100) e.put((char)('0' + ax / 100));
    e.put((char)('0' + (ax / 10) % 10)); e.put((char)('0' + ax % 10));
}

__device__ int values_of(const TextArgs& A, int f, int nA) {
    const int c = A.count[f];
    int n = c == VGL_TEXT_PER_G ? nA * (nA + 1) / 2 : c == VGL_TEXT_PER_A ? nA : 1;
    const int64_t fit = A.N > 0 ? A.stride[f] / A.N : 0;    // never read past the site's slab
    if (n > fit) n = (int)fit;
    return n < 0 ? 0 : n;
}

// "\t" + the sample's fields
template <bool W>
__device__ void column(const TextArgs& A, int64_t i, int s, int nA, Emit<W>& e) {
    e.put('\t');
    if (A.nf == 0) { e.put('.'); return; }
    for (int f = 0; f < A.nf; ++f) {
        if (f) e.put(':');
        const int n = values_of(A, f, nA);
        const int64_t at = i * A.stride[f] + (int64_t)s * n;
        for (int k = 0; k < n; ++k) {
            if (k) e.put(',');
            if (A.is_float[f]) fmt_float(e, ((const uint32_t*)A.base[f])[at + k]);
            else fmt_int(e, ((const int32_t*)A.base[f])[at + k]);
        }
    }
}

__global__ __launch_bounds__(NT) void k_text_plan(TextArgs A) {
    __shared__ uint32_t part[NT / 64];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (A.site_status[i] < 0) { if (tid == 0) A.off[i] = 0; return; }
    const int nA = A.n_alleles[i];
    uint32_t carry = 0;
    for (int s0 = 0; s0 < A.N; s0 += NT) {
        const int s = s0 + tid;
        uint32_t len = 0;
        if (s < A.N) { Emit<false> e{nullptr, 0, 0}; column(A, i, s, nA, e); len = e.n; }
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
    if (tid == 0) A.off[i] = (int64_t)A.hdr_len + carry + 1;
}

__global__ __launch_bounds__(SCAN_NT) void k_text_scan(int32_t n_sites, int64_t* off) {
    __shared__ int64_t part[SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t carry = 0;
    for (int b = 0; b < n_sites; b += SCAN_NT) {
        const int i = b + tid;
        const int64_t v = i < n_sites ? off[i] : 0;
        int64_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int64_t y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) part[wv] = x;
        __syncthreads();
        int64_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCAN_NT / 64; ++w) { const int64_t p = part[w]; if (w < wv) before += p; total += p; }
        if (i < n_sites) off[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) off[n_sites] = carry;
}

// grid (n_sites, ceil(N / NT)): lane = one sample column of one site
__global__ __launch_bounds__(NT) void k_text_write(TextArgs A) {
    const int64_t i = blockIdx.x;
    const int s = blockIdx.y * NT + threadIdx.x;
    if (A.off[A.n_sites] > A.cap) return;                   // does not fit: nothing is written
    if (A.site_status[i] < 0) return;
    const int64_t b = A.off[i], end = A.off[i + 1];
    if (s == 0) {
        for (int j = 0; j < A.hdr_len && b + j < end; ++j) A.dst[b + j] = (uint8_t)A.hdr[j];
        if (end > b) A.dst[end - 1] = '\n';
    }
    if (s >= A.N) return;
    const int64_t c0 = b + A.hdr_len + A.ws[i * A.N + s];
    const int64_t c1 = s + 1 < A.N ? b + A.hdr_len + A.ws[i * A.N + s + 1] : end - 1;
    if (c0 > c1 || c1 > end) return;
    Emit<true> e{A.dst + c0, 0, (uint32_t)(c1 - c0)};
    column(A, i, s, A.n_alleles[i], e);
}

int64_t per_sample_bound(const vgl_text_field* f, int32_t nf, int32_t max_alleles) {
    const int64_t G = (int64_t)max_alleles * (max_alleles + 1) / 2;
    int64_t b = 2;                                          // "\t" and "." (no fields)
    for (int k = 0; k < nf; ++k) {
        const int64_t n = f[k].count == VGL_TEXT_PER_G ? G : f[k].count == VGL_TEXT_PER_A ? max_alleles : 1;
        b += n * ((f[k].is_float ? 12 : 11) + 1);           // "-1.23457e-45" / "-2147483647" and a separator
    }
    return b;
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

// the site scan alone (k_text_scan: offsets[0 .. n_sites] from the site lengths in offsets[0 .. n_sites)); vgl_pileup.hip places its sites
// with it (not exported)
extern "C" int vgl_text_scan_launch(int32_t n_sites, int64_t* offsets, void* hip_stream) {
    hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(SCAN_NT), 0, (hipStream_t)hip_stream, n_sites, offsets);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}

extern "C" int64_t vgl_text_bound(int32_t n_samples, int32_t n_sites, const vgl_text_field* fields, int32_t n_fields, int32_t max_alleles) {
    if (n_samples < 0 || n_sites < 0 || n_fields < 0 || n_fields > VGL_TEXT_MAX_FIELDS || (n_fields > 0 && !fields) || max_alleles < 1 || max_alleles > 5) return -1;
    int64_t hdr = 2;
    for (int k = 0; k < n_fields; ++k) hdr += (fields[k].key ? (int64_t)strlen(fields[k].key) : 0) + 1;
    return (int64_t)n_sites * (hdr + 1 + (int64_t)n_samples * per_sample_bound(fields, n_fields, max_alleles));
}

extern "C" int64_t vgl_text_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    return (int64_t)n_samples * n_sites * (int64_t)sizeof(uint32_t);
}

extern "C" int vgl_text_format_device(int32_t device, const vgl_text_field* fields, int32_t n_fields, int32_t n_samples, int32_t n_sites,
                                      const int32_t* site_status, const int32_t* n_alleles, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                      void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (n_samples < 0 || n_sites < 0 || n_fields < 0 || n_fields > VGL_TEXT_MAX_FIELDS || (n_fields > 0 && !fields) || dst_cap < 0)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: bad argument");
    if (!offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: null offsets");
    if (n_sites > 0 && (!site_status || !n_alleles || (dst_cap > 0 && !dst)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: null argument");
    if (n_sites > 0 && n_samples > 0 && (!workspace || workspace_bytes < vgl_text_workspace_bytes(n_samples, n_sites)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: workspace smaller than vgl_text_workspace_bytes()");
    TextArgs A;
    memset(&A, 0, sizeof A);
    A.nf = n_fields; A.N = n_samples; A.n_sites = n_sites;
    std::string hdr = "\t";
    for (int k = 0; k < n_fields; ++k) {
        const vgl_text_field& F = fields[k];
        if (!F.key || !F.key[0] || (n_sites > 0 && n_samples > 0 && !F.base) || F.count < VGL_TEXT_ONE || F.count > VGL_TEXT_PER_A || F.site_stride < 0)
            return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: bad field descriptor");
        if (k) hdr += ':';
        hdr += F.key;
        A.base[k] = F.base; A.stride[k] = F.site_stride; A.count[k] = F.count; A.is_float[k] = F.is_float ? 1 : 0;
    }
    if (n_fields == 0) hdr += '.';
    if (hdr.size() > (size_t)HDR_MAX) return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: FORMAT keys longer than 127 bytes in all");
    // a site's text is addressed with 32-bit offsets inside the site
    if ((int64_t)n_samples * per_sample_bound(fields, n_fields, 5) + HDR_MAX + 1 > (int64_t)UINT32_MAX)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_text_format_device: too many samples for one record's text");
    memcpy(A.hdr, hdr.data(), hdr.size()); A.hdr_len = (int32_t)hdr.size();
    A.site_status = site_status; A.n_alleles = n_alleles; A.dst = dst; A.cap = dst_cap; A.off = offsets; A.ws = (uint32_t*)workspace;
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_text_format_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_text_format_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    hipLaunchKernelGGL(k_text_plan, dim3((unsigned)n_sites), dim3(NT), 0, st, A);
    hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(SCAN_NT), 0, st, n_sites, offsets);
    if (n_samples > 0) hipLaunchKernelGGL(k_text_write, dim3((unsigned)n_sites, (unsigned)((n_samples + NT - 1) / NT)), dim3(NT), 0, st, A);
    else hipLaunchKernelGGL(k_text_write, dim3((unsigned)n_sites, 1), dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_text_format_device: a launch failed");
    return VGL_OK;
}
