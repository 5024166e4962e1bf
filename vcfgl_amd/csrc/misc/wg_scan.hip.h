// wg_scan.hip.h -- the workgroup scan of the misc kernels: one step of it, which scan_columns (column_walk.hip.h), k_fgl_write and
// k_gtd_list_write take chunk by chunk, and k_offsets_scan, the kernel that turns a batch's per-record byte counts into offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wgscan {

// One step over a workgroup of NT lanes: inc = the inclusive sum of v inside the lane's wavefront, before = the sum over the wavefronts
// below it, total = the sum over the workgroup.  The wavefronts' totals go through s_tot[parity]: a caller that steps in a loop gives
// c & 1 in turn, so that one __syncthreads a step is enough; every lane of the workgroup takes part.
template <typename T> struct Sums { T inc, before, total; };
template <int NT, typename T>
__device__ __forceinline__ Sums<T> step(const T v, T (*s_tot)[NT / 64], const int parity) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T y = __shfl_up(inc, d, 64); if (lane >= d) inc += y; }
    if (lane == 63) s_tot[parity][wave] = inc;
    __syncthreads();
    T before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) { const T x = s_tot[parity][k]; if (k < wave) before += x; total += x; }
    return {inc, before, total};
}

constexpr int SCAN_NT = 1024;            // lanes of k_offsets_scan

// off[row][0 .. n] = the exclusive prefix sums of len[row][0 .. n), row = blockIdx.x: one workgroup a row, 1024 values a chunk
static __global__ void __launch_bounds__(SCAN_NT) k_offsets_scan(const int64_t* len_rows, int64_t* off_rows, const int32_t n) {
    __shared__ long long s_tot[2][SCAN_NT / 64];
    const int t = threadIdx.x;
    const int64_t* len = len_rows + (size_t)blockIdx.x * n;
    int64_t* off = off_rows + (size_t)blockIdx.x * ((size_t)n + 1);
    long long base = 0;
    const int n_chunks = (n + SCAN_NT - 1) / SCAN_NT;
    for (int c = 0; c < n_chunks; c++) {
        const int i = c * SCAN_NT + t;
        const long long v = i < n ? (long long)len[i] : 0;
        const Sums<long long> s = step<SCAN_NT>(v, s_tot, c & 1);
        if (i < n) off[i] = (int64_t)(base + s.before + s.inc - v);
        base += s.total;
    }
    if (t == 0) off[n] = (int64_t)base;
}

}  // namespace wgscan
