// vgl_stream.hip -- a tile's record stream assembled and compressed on the device (ABI 7 addition: vgl_stream_assemble_device; its user
// vgl_stream_host_* is in hostlib/batch.h).
// A record of the output is a host-built HEAD (the eight fixed columns of a VCF line; l_shared, l_indiv and the shared block of a BCF
// record) followed by a device-built BODY (the sample columns of vgl_text.hip, the indiv block of vgl_bcf.hip).  The bodies of a tile
// stay where they were built; the heads -- a few dozen bytes per site -- come up the link, and k_stream_gather interleaves the two:
//     record i starts at (head_offsets[i] - head_offsets[0]) + (body_offsets[i] - body_offsets[0]), head first, then body
// so the destination of every byte follows from the two prefix sums and no scan is needed.  vgl_bgzf_compress_device then cuts the
// stream into members, and only those come down.
//   k_stream_gather   one workgroup per 4 KiB of the DESTINATION (cut at 16-byte boundaries of its address): the workgroup finds the
//                     sites whose records overlap its piece by bisection on the record starts, and moves the 2 x sites segments (head,
//                     body), each clipped to the piece.  A workgroup's NT lanes work as NT / G groups of G lanes, one segment per group
//                     at a time; G = 256, 64 or 16 by the piece's mean segment length, so a 300 KB body is shared by the workgroups of
//                     all its pieces at 16 bytes per lane, and a piece of a hundred 30-byte records keeps sixteen groups busy.
//   the byte mover    the form of k_bcf_write (put_values): single bytes up to the destination's next 16-byte boundary, then 16-byte
//                     aligned stores whose source is read as aligned 32-bit words and funnel-shifted (v_alignbyte) when it is off by
//                     1 - 3 bytes, then a tail of single bytes; every store lies inside the clipped segment, so inside the record.
// Store width: the destination is a contiguous stream, so a wavefront's 16-byte stores are one 1 KiB run (the widest a vector store
// instruction writes); against 4-byte stores that is a quarter of the store instructions and of the address arithmetic per byte, which
// is what a copy with a funnel shift per word is made of.  The source side stays at 32-bit words: that is the alignment a head or a body
// is known to have after the shift, and five words per lane are contiguous across the lanes of a group.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"

namespace {

constexpr int NT = 256;                         // lanes per workgroup
constexpr int64_t PIECE = (int64_t)NT * 16;     // destination bytes per workgroup: one 16-byte store per lane
constexpr int64_t MAX_GRID = 1 << 20;           // (pieces beyond it are taken in a grid-stride loop)

// n bytes from src to dst by the G lanes of a group (g = this lane's index in it)
__device__ inline void move_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n, int g, int G) {
    int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (head > n) head = n;
    for (int64_t j = g; j < head; j += G) dst[j] = src[j];
    const int64_t nv = (n - head) >> 4;
    const uint8_t* s = src + head;
    uint4* o = (uint4*)(dst + head);
    const uint32_t r = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t* w = (const uint32_t*)(s - r);           // the aligned word that holds s[0]
    if (r == 0) {
        for (int64_t v = g; v < nv; v += G) {
            const uint32_t* p = w + 4 * v;
            o[v] = make_uint4(p[0], p[1], p[2], p[3]);
        }
    } else {
        // bytes r .. r + 15 of five aligned words: the fifth holds s[16 - r .. 15], so it is a word of the source as well
        for (int64_t v = g; v < nv; v += G) {
            const uint32_t* p = w + 4 * v;
            const uint32_t a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
            o[v] = make_uint4(__builtin_amdgcn_alignbyte(b, a, r), __builtin_amdgcn_alignbyte(c, b, r),
                              __builtin_amdgcn_alignbyte(d, c, r), __builtin_amdgcn_alignbyte(e, d, r));
        }
    }
    for (int64_t t = head + 16 * nv + g; t < n; t += G) dst[t] = src[t];
}

struct Gather {
    const uint8_t* heads; const int64_t* ho;
    const uint8_t* bodies; const int64_t* bo;
    uint8_t* dst; int64_t cap; int64_t* total;
    int64_t n;
};

__device__ inline int64_t rec_start(const Gather& A, int64_t i) { return (A.ho[i] - A.ho[0]) + (A.bo[i] - A.bo[0]); }

__global__ __launch_bounds__(NT) void k_stream_gather(Gather A) {
    const int64_t total = rec_start(A, A.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.total = total;
    if (total <= 0 || total > A.cap) return;                // nothing to move (every site empty) / does not fit: nothing is written
    const int64_t al = (int64_t)((uintptr_t)A.dst & 15u);   // pieces are cut at 16-byte boundaries of the destination's address
    const int64_t pieces = (total + al + PIECE - 1) / PIECE;
    for (int64_t c = blockIdx.x; c < pieces; c += gridDim.x) {
        const int64_t c0 = c == 0 ? 0 : c * PIECE - al;
        const int64_t c1 = (c + 1) * PIECE - al < total ? (c + 1) * PIECE - al : total;
        // lo = the last site that starts at or before c0, hi = the first that starts at or behind c1: sites lo .. hi - 1 overlap
        int64_t a = 0, b = A.n + 1;
        while (a < b) { const int64_t m = (a + b) >> 1; if (rec_start(A, m) <= c0) a = m + 1; else b = m; }
        const int64_t lo = a > 0 ? a - 1 : 0;
        b = A.n;
        while (a < b) { const int64_t m = (a + b) >> 1; if (rec_start(A, m) < c1) a = m + 1; else b = m; }
        const int64_t hi = a;
        const int64_t nseg = 2 * (hi - lo);
        const int G = nseg * 2048 <= PIECE ? NT : nseg * 512 <= PIECE ? 64 : 16;
        const int g = (int)threadIdx.x % G, q = (int)threadIdx.x / G, groups = NT / G;
        for (int64_t s = q; s < nseg; s += groups) {
            const int64_t i = lo + (s >> 1);
            const int64_t h0 = A.ho[i] - A.ho[0], hl = A.ho[i + 1] - A.ho[i], b0 = A.bo[i] - A.bo[0], bl = A.bo[i + 1] - A.bo[i];
            const bool body = s & 1;
            const int64_t d0 = h0 + b0 + (body ? hl : 0), len = body ? bl : hl;
            const uint8_t* src = body ? A.bodies + b0 : A.heads + h0;
            const int64_t x0 = d0 > c0 ? d0 : c0, x1 = d0 + len < c1 ? d0 + len : c1;      // the segment inside this piece
            if (x0 < x1) move_bytes(src + (x0 - d0), A.dst + x0, x1 - x0, g, G);
        }
    }
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int vgl_stream_assemble_device(int32_t device, int32_t n_sites, const uint8_t* heads, const int64_t* head_offsets, const uint8_t* bodies,
                                          const int64_t* body_offsets, uint8_t* dst, int64_t dst_cap, int64_t* total, void* hip_stream) {
    if (n_sites < 0 || dst_cap < 0 || !total) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_assemble_device: bad argument");
    if (n_sites > 0 && (!head_offsets || !body_offsets || (dst_cap > 0 && (!dst || !heads || !bodies))))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_assemble_device: null argument");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_assemble_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(total, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_assemble_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    Gather A{heads, head_offsets, bodies, body_offsets, dst, dst_cap, total, n_sites};
    // the total is known on the device only: one workgroup per piece of the capacity (those behind the total leave at once)
    int64_t grid = (dst_cap + 15 + PIECE - 1) / PIECE;
    grid = grid < 1 ? 1 : grid > MAX_GRID ? MAX_GRID : grid;
    hipLaunchKernelGGL(k_stream_gather, dim3((unsigned)grid), dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_assemble_device: a launch failed");
    return VGL_OK;
}
