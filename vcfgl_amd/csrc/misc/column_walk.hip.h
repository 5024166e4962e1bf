// column_walk.hip.h -- the walk over the tab-separated columns of a text region that k_gtd_parse (gtdisc.hip) and k_fgl_parse
// (fetchgl.hip) share: a workgroup of NT lanes reads the region in chunks of NT x LB bytes on LB-byte address boundaries -- a lane
// whose LB bytes lie inside the region loads them at once, the lanes at the two ends read their bytes one by one, so no byte outside
// the region is read -- and a scan of the tab counts (wg_scan.hip.h) numbers the columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_scan.hip.h"

namespace colwalk {

constexpr int NT = 256;                  // lanes per workgroup
constexpr int LB = 16;                   // bytes per lane and chunk
constexpr int CHUNK = NT * LB;

// the columns of the region [lb, le): f(col, q) for every column that starts at q; returns the number of columns.  One __syncthreads
// per chunk on s_tot[parity]; every lane of the workgroup takes part.
template <typename F>
__device__ __forceinline__ int32_t scan_columns(const uint8_t* __restrict__ text, const int64_t lb, const int64_t le, int32_t (*s_tot)[NT / 64], F f) {
    const int t = threadIdx.x;
    const int64_t mis = (int64_t)((uintptr_t)(text + lb) & (LB - 1));
    const int64_t o0 = lb - mis;                                       // the 16-byte boundary at or below the region's first byte
    const int64_t n_chunks = (le - o0 + CHUNK - 1) / CHUNK;
    int32_t base = 0;
    if (t == 0) f(0, lb);                                              // column 0 starts at the region's first byte
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
        const wgscan::Sums<int> s = wgscan::step<NT>(cnt, s_tot, c & 1);
        int32_t col = base + s.before + s.inc - cnt + 1;               // the column after this lane's first tab
        base += s.total;
        while (mask) {
            const int i = __ffs(mask) - 1; mask &= mask - 1;
            f(col, o + i + 1);
            col++;
        }
    }
    return base + 1;
}

}  // namespace colwalk
