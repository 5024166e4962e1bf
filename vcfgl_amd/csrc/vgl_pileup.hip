// vgl_pileup.hip -- the N-wide part of a tile's pileup lines on the device (ABI 7 additions: vgl_pileup_bound,
// vgl_pileup_workspace_bytes, vgl_pileup_format_device).
// For every site i with site_status[i] != VGL_SITE_SKIP_EMPTY the output is exactly what the host writer (host/vcfgl_main.cpp,
// write_tile, -printPileup 1) appends behind the prefix chrom "\t" pos "\t" ref:
//     ( "\t" COL(i, s) ) for s = 0 .. N-1, then "\n"
//     COL = "0\t*\t*"                                    dp(i, s) == 0
//     COL = dp "\t" B_0 .. B_{dp-1} "\t" Q_0 .. Q_{dp-1}   otherwise
//     B_r = "ACGT"[reads[r][i][s] & 3],  Q_r = (reads[r][i][s] >> 2) + 33, or one constant byte, or (--adjust-qs 4 with --error-qs 2)
//           the adjusted score of the read's staged error probability + 33 (errprob_to_qs, vgl_common.hip.h)
// An empty site (VGL_SITE_SKIP_EMPTY) produces no bytes; every other status (VGL_SITE_SKIP_INVAR and VGL_SITE_NO_READS included) gets
// its line, since the host prints the pileup before it decides to skip a site.  Inputs: fmt_dp[i * N + s] (VGL_LAYOUT_SAMPLE_MAJOR),
// reads[(r * n_sites + i) * N + s] for r < read_capacity (the read dump of vgl_tile_out.reads).
// Three passes, the shape of vgl_text (plan, scan, write):
//   k_pileup_plan   one workgroup per site: a column's length from DP alone (dp == 0 ? 6 : 3 + digits(dp) + 2 dp, its tab included), a
//                   workgroup scan gives each column's offset inside the site (workspace, uint32 per (site, sample)) and the site's length;
//                   a dp below 0 or above read_capacity raises the call's flag word
//   k_text_scan     vgl_text.hip's site scan (vgl_text_scan_launch): offsets[0 .. n_sites], offsets[n_sites] = the total
//   k_pileup_write  one lane per (site, sample), consecutive samples in consecutive lanes (row r of the dump is read coalesced); each
//                   lane reads a read byte once and emits its base and its score into two byte streams, each assembled into dwords and
//                   stored whole where the dword lies inside the stream's own bytes (byte stores only at the two ends of a stream).
//                   Nothing is written when the flag is up (offsets[n_sites] = -1) or the total exceeds dst_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_common.hip.h"

namespace {

constexpr int NT = 256;                 // lanes per workgroup (plan: one workgroup per site, samples in chunks of NT)
constexpr int64_t WS_HEAD = 16;         // workspace: the flag word, padded; then uint32 column offsets per (site, sample)

enum { Q_OWN = 0, Q_CONST = 1, Q_ERRP = 2 };

struct PileArgs {
    int32_t N, n_sites, read_cap, qual_char;
    const int32_t* site_status;
    const int32_t* dp;
    const uint8_t* reads;
    const double* errp;                 // Q_ERRP: the staged error probabilities, same layout as reads
    uint8_t* dst;
    int64_t cap;
    int64_t* off;
    uint32_t* ws;                       // column offsets
    uint32_t* flag;                     // the call's flag word (a dp out of range)
    uint32_t* errflag;                  // Q_ERRP: where errprob_to_qs reports a --qs-bins miss
};

__device__ __forceinline__ int ndig32(uint32_t u) {
    int n = 1;
    if (u >= 10u) n = 2; if (u >= 100u) n = 3; if (u >= 1000u) n = 4; if (u >= 10000u) n = 5;
    if (u >= 100000u) n = 6; if (u >= 1000000u) n = 7; if (u >= 10000000u) n = 8; if (u >= 100000000u) n = 9; if (u >= 1000000000u) n = 10;
    return n;
}

__device__ __forceinline__ uint32_t col_len(int32_t d) { return d == 0 ? 6u : 3u + (uint32_t)ndig32((uint32_t)d) + 2u * (uint32_t)d; }

// one byte stream of a lane, [lo, end): bytes gather in a dword that is stored whole when it lies inside [lo, end); the bytes of a
// dword that starts before lo, and the last partial dword, are stored one by one (they share their dword with another stream)
struct DwordOut {
    uint8_t* p;                         // next byte
    uint8_t* lo;                        // the stream's first byte
    uint32_t acc;
    __device__ void put(uint32_t c) {
        const uint32_t k = (uint32_t)(uintptr_t)p & 3u;
        acc |= c << (8u * k);
        ++p;
        if (k == 3u) {
            uint8_t* d = p - 4;
            if (d >= lo) *(uint32_t*)d = acc;
            else for (uint8_t* q = lo; q < p; ++q) *q = (uint8_t)(acc >> (8u * ((uint32_t)(uintptr_t)q & 3u)));
            acc = 0;
        }
    }
    __device__ void flush() {
        const uint32_t k = (uint32_t)(uintptr_t)p & 3u;
        if (k == 0) return;
        uint8_t* q = p - k;
        if (q < lo) q = lo;
        for (; q < p; ++q) *q = (uint8_t)(acc >> (8u * ((uint32_t)(uintptr_t)q & 3u)));
    }
};

__global__ __launch_bounds__(NT) void k_pileup_plan(PileArgs A) {
    __shared__ uint32_t part[NT / 64];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (A.site_status[i] == VGL_SITE_SKIP_EMPTY) { if (tid == 0) A.off[i] = 0; return; }
    uint32_t carry = 0;
    for (int s0 = 0; s0 < A.N; s0 += NT) {
        const int s = s0 + tid;
        uint32_t len = 0;
        if (s < A.N) {
            int32_t d = A.dp[i * A.N + s];
            if (d < 0 || d > A.read_cap) { *A.flag = 1u; d = 0; }
            len = col_len(d);
        }
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
    if (tid == 0) A.off[i] = (int64_t)carry + 1;
}

// grid (n_sites, ceil(N / NT)): lane = one sample column of one site
template <int QM>
__device__ void write_column(const PileArgs& A, const VglDevParams* P) {
    const int64_t i = blockIdx.x;
    const int s = blockIdx.y * NT + threadIdx.x;
    if (*A.flag) {                                          // a dp out of range: nothing is written, the total reads -1
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) A.off[A.n_sites] = -1;
        return;
    }
    if (A.off[A.n_sites] > A.cap) return;                   // does not fit: nothing is written
    if (A.site_status[i] == VGL_SITE_SKIP_EMPTY) return;
    const int64_t b = A.off[i], end = A.off[i + 1];
    if (s == 0 && end > b) A.dst[end - 1] = '\n';
    if (s >= A.N) return;
    const int32_t d = A.dp[i * A.N + s];
    uint8_t* const c0 = A.dst + b + A.ws[i * A.N + s];
    DwordOut o1{c0, c0, 0u};
    o1.put('\t');
    if (d == 0) {
        o1.put('0'); o1.put('\t'); o1.put('*'); o1.put('\t'); o1.put('*');
        o1.flush();
        return;
    }
    const int L = ndig32((uint32_t)d);
    uint32_t pw = 1;
    for (int j = 1; j < L; ++j) pw *= 10u;
    for (uint32_t x = (uint32_t)d; pw; pw /= 10u) { o1.put('0' + x / pw); x %= pw; }
    o1.put('\t');
    uint8_t* const q0 = c0 + 2 + L + d;                     // the tab in front of the scores: the second stream
    DwordOut o2{q0, q0, 0u};
    o2.put('\t');
    const size_t plane = (size_t)A.n_sites * A.N;
    const size_t ev = (size_t)i * A.N + s;
    for (int r = 0; r < d; ++r) {
        const uint32_t v = A.reads[(size_t)r * plane + ev];
        o1.put((0x54474341u >> (8u * (v & 3u))) & 0xffu);  // "ACGT"
        uint32_t q;
        if (QM == Q_OWN) q = (v >> 2) + 33u;
        else if (QM == Q_CONST) q = (uint32_t)A.qual_char;
        else { int qq, aq; errprob_to_qs(*P, A.errp[(size_t)r * plane + ev], qq, aq, A.errflag); q = (uint32_t)(aq + 33) & 0xffu; }
        o2.put(q);
    }
    o1.flush();
    o2.flush();
}

__global__ __launch_bounds__(NT) void k_pileup_write(PileArgs A) {
    if (A.qual_char < 0) write_column<Q_OWN>(A, nullptr);
    else write_column<Q_CONST>(A, nullptr);
}

__global__ __launch_bounds__(NT) void k_pileup_write_errp(PileArgs A, VglDevParams P) { write_column<Q_ERRP>(A, &P); }

int64_t max_col(int32_t read_capacity) {
    int64_t digits = 1;
    for (int64_t p = 10; p <= read_capacity; p *= 10) ++digits;
    const int64_t c = 3 + digits + 2 * (int64_t)read_capacity;
    return c > 6 ? c : 6;
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()
extern "C" int vgl_text_scan_launch(int32_t n_sites, int64_t* offsets, void* hip_stream);   // vgl_text.hip (not exported)

extern "C" int64_t vgl_pileup_bound(int32_t n_samples, int32_t n_sites, int32_t read_capacity) {
    if (n_samples < 0 || n_sites < 0 || read_capacity < 0) return -1;
    return (int64_t)n_sites * (1 + (int64_t)n_samples * max_col(read_capacity));
}

extern "C" int64_t vgl_pileup_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    return WS_HEAD + (int64_t)n_samples * n_sites * (int64_t)sizeof(uint32_t);
}

// the stateless entry and the context's: errp != NULL (with P) takes every score from the read's staged error probability
extern "C" int vgl_pileup_format_impl(int32_t device, int32_t n_samples, int32_t n_sites, const int32_t* site_status, const int32_t* fmt_dp,
                                      const uint8_t* reads, int32_t read_capacity, int32_t qual_char, const double* errp, const VglDevParams* P,
                                      uint32_t* errflag, uint8_t* dst, int64_t dst_cap, int64_t* offsets, void* workspace, int64_t workspace_bytes,
                                      void* hip_stream) {
    if (n_samples < 0 || n_sites < 0 || read_capacity < 0 || dst_cap < 0 || qual_char < -1 || qual_char > 255)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: bad argument");
    if (!offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: null offsets");
    if (n_sites > 0 && (!site_status || (dst_cap > 0 && !dst) || (n_samples > 0 && (!fmt_dp || (read_capacity > 0 && !reads)))))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: null argument");
    if (n_sites > 0 && (!workspace || workspace_bytes < vgl_pileup_workspace_bytes(n_samples, n_sites)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: workspace smaller than vgl_pileup_workspace_bytes()");
    // a site's text is addressed with 32-bit offsets inside the site
    if ((int64_t)n_samples * max_col(read_capacity) + 1 > (int64_t)UINT32_MAX)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: too many samples for one site's line");
    if (errp && (!P || !errflag)) return vgl_pack_set_error(VGL_E_ARG, "vgl_pileup_format_device: internal: scores from errp need the parameters");
    PileArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.read_cap = read_capacity; A.qual_char = qual_char;
    A.site_status = site_status; A.dp = fmt_dp; A.reads = reads; A.errp = errp;
    A.dst = dst; A.cap = dst_cap; A.off = offsets;
    A.flag = (uint32_t*)workspace; A.ws = (uint32_t*)((uint8_t*)workspace + WS_HEAD); A.errflag = errflag;
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_pileup_format_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_pileup_format_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    if (hipMemsetAsync(A.flag, 0, sizeof(uint32_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_pileup_format_device: hipMemsetAsync failed");
    hipLaunchKernelGGL(k_pileup_plan, dim3((unsigned)n_sites), dim3(NT), 0, st, A);
    if (vgl_text_scan_launch(n_sites, offsets, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_pileup_format_device: k_text_scan launch failed");
    const dim3 grid((unsigned)n_sites, (unsigned)(n_samples > 0 ? (n_samples + NT - 1) / NT : 1));
    if (errp) hipLaunchKernelGGL(k_pileup_write_errp, grid, dim3(NT), 0, st, A, *P);
    else hipLaunchKernelGGL(k_pileup_write, grid, dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_pileup_format_device: a launch failed");
    return VGL_OK;
}

extern "C" int vgl_pileup_format_device(int32_t device, int32_t n_samples, int32_t n_sites, const int32_t* site_status, const int32_t* fmt_dp,
                                        const uint8_t* reads, int32_t read_capacity, int32_t qual_char, uint8_t* dst, int64_t dst_cap,
                                        int64_t* offsets, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    return vgl_pileup_format_impl(device, n_samples, n_sites, site_status, fmt_dp, reads, read_capacity, qual_char, nullptr, nullptr, nullptr,
                                  dst, dst_cap, offsets, workspace, workspace_bytes, hip_stream);
}
