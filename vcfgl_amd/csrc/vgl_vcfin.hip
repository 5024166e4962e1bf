// vgl_vcfin.hip -- the sample columns of VCF text parsed on the device (ABI 7 additions: vgl_vcfin_workspace_bytes,
// vgl_vcfin_parse_device; vgl_vcfin_host_* in hostlib/batch.h launches k_vcfin_parse through vgl_launch_vcfin_parse).  The host program's parse_record + make_site are the specification: per line, the
// GT token of every sample column becomes the packed byte (b1 << 4) | b0 that the tile calls take, b = allele_map[a] & 0xF
// (0xF for a missing allele), and the non-missing allele indices are summed.
//   token         the gti-th ':'-separated subfield of the column; a column with fewer subfields has none: both alleles missing
//   plain token   A or A S A, A = '.' or one or two decimal digits below the line's allele count, S = '|' or '/'; A alone gives
//                 a1 = a0 (a haploid call)
//   anything else (an empty allele, another byte -- '\r' included --, a third allele, a third digit, an index >= n_alleles, a
//                 number of columns that is not n_samples) gives the LINE the status VGL_VCFIN_HOST: its row is unspecified and
//                 the caller parses that line itself.  Nothing is guessed on the device.
//   k_vcfin_check the line ranges against the text: 0 <= line_begin <= line_end <= text_bytes; one flag word
//   k_vcfin_parse one workgroup of 256 lanes per line.  The sample region [line_begin, line_end) is walked in chunks of 256 x 16
//                 bytes on 16-byte address boundaries: a lane whose 16 bytes lie inside the region loads them with one 16-byte
//                 load, the lanes at the two ends read their bytes of the region one by one -- no byte outside the region is
//                 read.  Each lane builds the tab mask of its bytes; an exclusive scan of the popcounts (wave-wide with
//                 shuffles, the four wave totals through LDS, a running base across chunks) numbers the tabs, so the lane that
//                 owns the tab before column s parses that column's token (column 0: the lane that owns the region's first
//                 byte).  The token's few bytes are read from the text again, bounded by line_end (they were just loaded: L1
//                 hits), and one byte goes to gt_out[line][s], guarded by s < n_samples.  The allele sum, the status (an OR) and
//                 the column count are workgroup reductions that lane 0 stores.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_device.h"

namespace {

constexpr int NT = 256;                  // lanes per workgroup
constexpr int LB = 16;                   // bytes per lane and chunk
constexpr int CHUNK = NT * LB;
constexpr int64_t WS_BYTES = 256;        // the flag word of k_vcfin_check

using VcfinArgs = VglVcfinArgs;

__global__ void __launch_bounds__(NT) k_vcfin_check(int32_t n_lines, int64_t text_bytes, const int64_t* __restrict__ lb, const int64_t* __restrict__ le,
                                                    uint32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_lines; i += (int64_t)gridDim.x * NT) {
        const int64_t b = lb[i], e = le[i];
        bad |= b < 0 || b > e || e > text_bytes;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1u;       // (every writer stores the same word)
}

// one allele at q: '.' or one or two digits.  Returns the index (-1 missing), -2 when the bytes are not an allele
__device__ __forceinline__ int vcfin_allele(const uint8_t* __restrict__ text, int64_t& q, const int64_t le) {
    if (q >= le) return -2;
    const int c = text[q];
    if (c == '.') { q++; return -1; }
    if (c < '0' || c > '9') return -2;
    int v = c - '0'; q++;
    if (q < le) { const int d = text[q]; if (d >= '0' && d <= '9') { v = v * 10 + (d - '0'); q++; } }
    return v;
}

// the column that starts at q: its packed byte, its allele sum; false = not a plain token (the line goes to the host)
__device__ __forceinline__ bool vcfin_column(const uint8_t* __restrict__ text, int64_t q, const int64_t le, const int gti, const int nal,
                                             const int m0, const int m1, const int m2, const int m3, const int m4, uint32_t& byte, int& sum) {
    byte = 0xFFu; sum = 0;
    for (int k = 0; k < gti; k++) {                                  // skip gti subfields; the column may end first: no token
        for (;;) {
            if (q >= le) return true;
            const int c = text[q++];
            if (c == '\t') return true;
            if (c == ':') break;
        }
    }
    auto ends = [&](int64_t at) { if (at >= le) return true; const int c = text[at]; return c == '\t' || c == ':'; };
    auto map = [&](int a) { return (a < 0 ? 0xF : (a == 0 ? m0 : a == 1 ? m1 : a == 2 ? m2 : a == 3 ? m3 : m4) & 0xF); };
    const int a0 = vcfin_allele(text, q, le);
    if (a0 == -2 || a0 >= nal) return false;
    int a1 = a0;
    if (!ends(q)) {
        const int c = text[q];
        if (c != '|' && c != '/') return false;
        q++;
        a1 = vcfin_allele(text, q, le);
        if (a1 == -2 || a1 >= nal || !ends(q)) return false;
    }
    byte = (uint32_t)(map(a0) | (map(a1) << 4));
    sum = (a0 > 0 ? a0 : 0) + (a1 > 0 ? a1 : 0);
    return true;
}

__global__ void __launch_bounds__(NT) k_vcfin_parse(const VcfinArgs A) {
    __shared__ int32_t s_tot[2][NT / 64];
    __shared__ int32_t s_sum[NT / 64], s_bad[NT / 64];
    const int line = blockIdx.x;
    if (line >= A.n_lines) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = A.N;
    int64_t lb = A.line_begin[line], le = A.line_end[line];
    if (lb < 0 || lb > le || le > A.text_bytes) {                      // (refused by the entry point; never read outside the text)
        if (t == 0) { A.status_out[line] = VGL_VCFIN_HOST; A.allelesum_out[line] = 0; }
        return;
    }
    const uint8_t* __restrict__ text = A.text;
    const int gti = A.gti[line], nal = A.n_alleles[line];
    if (gti < 0 || nal < 1 || nal > 5) {                               // outside what allele_map [5] and a FORMAT index can describe: the caller's line
        if (t == 0) { A.status_out[line] = VGL_VCFIN_HOST; A.allelesum_out[line] = 0; }
        return;
    }
    const int8_t* am = A.allele_map + (size_t)line * 5;
    const int m0 = am[0], m1 = am[1], m2 = am[2], m3 = am[3], m4 = am[4];
    uint8_t* __restrict__ row = A.gt_out + (size_t)line * (size_t)N;
    // chunks on 16-byte ADDRESS boundaries: o0 = offset of the boundary at or below the region's first byte (may be negative)
    const int64_t mis = (int64_t)((uintptr_t)(text + lb) & (LB - 1));
    const int64_t o0 = lb - mis;
    const int64_t n_chunks = (le - o0 + CHUNK - 1) / CHUNK;            // 0 for an empty region at an aligned offset
    int32_t base = 0, sum = 0, bad = 0;
    if (t == 0) {                                                      // column 0 starts at the region's first byte
        uint32_t b; int s;
        if (!vcfin_column(text, lb, le, gti, nal, m0, m1, m2, m3, m4, b, s)) bad = 1;
        else { sum += s; if (0 < N) row[0] = (uint8_t)b; }
    }
    for (int64_t c = 0; c < n_chunks; c++) {
        const int64_t o = o0 + c * CHUNK + (int64_t)t * LB;            // this lane's 16 bytes: [o, o + 16)
        uint32_t w[4] = {0, 0, 0, 0};
        if (o >= lb && o + LB <= le) {
            const uint4 v = *reinterpret_cast<const uint4*>(text + o);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if (o + LB > lb && o < le) {
#pragma unroll
            for (int i = 0; i < LB; i++) { const int64_t at = o + i; if (at >= lb && at < le) w[i >> 2] |= (uint32_t)text[at] << (8 * (i & 3)); }
        }
        uint32_t mask = 0;                                             // bit i: byte i is a tab (a byte outside the region is 0 here)
#pragma unroll
        for (int i = 0; i < LB; i++) mask |= (((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == (uint32_t)'\t' ? 1u : 0u) << i;
        const int cnt = __popc(mask);
        int inc = cnt;                                                 // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d, 64); if (lane >= d) inc += y; }
        if (lane == 63) s_tot[c & 1][wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; k++) { const int x = s_tot[c & 1][k]; if (k < wave) before += x; total += x; }
        int col = base + before + inc - cnt + 1;                       // the column after this lane's first tab
        base += total;
        while (mask) {
            const int i = __ffs(mask) - 1; mask &= mask - 1;
            if (col < N) {
                uint32_t b; int s;
                if (!vcfin_column(text, o + i + 1, le, gti, nal, m0, m1, m2, m3, m4, b, s)) bad = 1;
                else { sum += s; row[col] = (uint8_t)b; }
            }
            col++;
        }
    }
    // (every lane holds the same base: the number of tabs; base + 1 columns)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sum += __shfl_down(sum, d, 64); bad |= __shfl_down(bad, d, 64); }
    if (lane == 0) { s_sum[wave] = sum; s_bad[wave] = bad; }
    __syncthreads();
    if (t == 0) {
        int S = 0, B = 0;
        for (int k = 0; k < NT / 64; k++) { S += s_sum[k]; B |= s_bad[k]; }
        if (base + 1 != N) B = 1;
        A.allelesum_out[line] = S;
        A.status_out[line] = B ? VGL_VCFIN_HOST : VGL_VCFIN_OK;
    }
}

}  // namespace

extern "C" int vgl_launch_vcfin_parse(const VglVcfinArgs* a, void* stream) {
    hipLaunchKernelGGL(k_vcfin_parse, dim3((unsigned)a->n_lines), dim3(NT), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_vcfin_workspace_bytes(int32_t n_samples, int32_t n_lines) {
    if (n_samples <= 0 || n_lines < 0) return -1;
    return WS_BYTES;
}

extern "C" int vgl_vcfin_parse_device(int32_t device, const uint8_t* text, int64_t text_bytes, int32_t n_lines, const int64_t* line_begin,
                                      const int64_t* line_end, const int32_t* gti, const int32_t* n_alleles, const int8_t* allele_map,
                                      int32_t n_samples, uint8_t* gt_out, int32_t* allelesum_out, int32_t* status_out, void* workspace,
                                      void* hip_stream) {
    if (n_lines < 0 || n_samples <= 0 || text_bytes < 0) return vgl_pack_set_error(VGL_E_ARG, "vgl_vcfin_parse_device: bad argument");
    if (n_lines > 0 && (!text || !line_begin || !line_end || !gti || !n_alleles || !allele_map || !gt_out || !allelesum_out || !status_out || !workspace))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_vcfin_parse_device: null argument");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_vcfin_parse_device: no HIP device is available");
    if (device < 0 || device >= nd || hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_vcfin_parse_device: no such device");
    if (n_lines == 0) return VGL_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    // the line ranges are device memory: one small kernel compares them with text_bytes and the call waits for its one word --
    // a range outside the text is refused before the parser is launched (the parse itself is not waited for)
    uint32_t* flag = (uint32_t*)workspace; uint32_t h_flag = 0;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_vcfin_parse_device: hipMemsetAsync failed");
    const int cg = (n_lines + NT - 1) / NT < 1024 ? (n_lines + NT - 1) / NT : 1024;
    hipLaunchKernelGGL(k_vcfin_check, dim3((unsigned)cg), dim3(NT), 0, st, n_lines, text_bytes, line_begin, line_end, flag);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_flag, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_vcfin_parse_device: the argument check failed to run");
    if (h_flag) return vgl_pack_set_error(VGL_E_ARG, "vgl_vcfin_parse_device: a line range lies outside the text (0 <= line_begin <= line_end <= text_bytes)");
    VcfinArgs A{text, text_bytes, n_lines, n_samples, line_begin, line_end, gti, n_alleles, allele_map, gt_out, allelesum_out, status_out};
    if (vgl_launch_vcfin_parse(&A, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_vcfin_parse_device: the launch failed");
    return VGL_OK;
}
