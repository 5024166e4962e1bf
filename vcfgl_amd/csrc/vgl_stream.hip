// vgl_stream.hip -- a tile's record stream assembled and compressed on the device (ABI 7 additions: vgl_stream_assemble_device,
// vgl_stream_host_*).
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

#include <algorithm>
#include <vector>

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

// ---- host handle (vgl_stream_host_*): what the host program's writer thread uses ------------------------------------------------------
// One HIP stream orders the work of all buffers (upload, gather, compression, the size back), so the assembled stream and the BGZF
// workspace are shared; the bodies, the uploaded heads and offsets and the members are per buffer.
struct vgl_stream_host {
    int device = 0, nb = 0;
    int32_t max_sites = 0;
    int64_t max_head = 0, max_body = 0, cap = 0, ws_bytes = 0, out_cap = 0;
    hipStream_t st = nullptr, cp = nullptr;                 // assembly + compression; copies of finished members back to the host
    uint8_t* d_stream = nullptr; void* ws = nullptr;
    struct Buf {
        uint8_t* d_body = nullptr; uint8_t* d_heads = nullptr; int64_t* d_off = nullptr;    // d_off: head offsets, then body offsets
        uint8_t* h_heads = nullptr; int64_t* h_off = nullptr;                               // page-locked staging of what submit is given
        uint8_t* d_mem = nullptr; uint8_t* h_mem = nullptr; int64_t h_mem_cap = 0;          // h_mem grows to what the members take (page-locking is not free)
        int64_t* d_n = nullptr; int64_t* h_n = nullptr;                                     // {assembled total, compressed length}
        int64_t raw = 0, seq = 0; hipEvent_t done = nullptr; bool busy = false;
    };
    std::vector<Buf> b;
    int64_t next_seq = 0, wait_seq = 0;
};

extern "C" int vgl_stream_host_destroy(vgl_stream_host* h) {
    if (!h) return VGL_OK;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    if (h->cp) (void)hipStreamSynchronize(h->cp);
    for (auto& B : h->b) {
        if (B.d_body) (void)hipFree(B.d_body);
        if (B.d_heads) (void)hipFree(B.d_heads);
        if (B.d_off) (void)hipFree(B.d_off);
        if (B.h_heads) (void)hipHostFree(B.h_heads);
        if (B.h_off) (void)hipHostFree(B.h_off);
        if (B.d_mem) (void)hipFree(B.d_mem);
        if (B.h_mem) (void)hipHostFree(B.h_mem);
        if (B.d_n) (void)hipFree(B.d_n);
        if (B.h_n) (void)hipHostFree(B.h_n);
        if (B.done) (void)hipEventDestroy(B.done);
    }
    if (h->d_stream) (void)hipFree(h->d_stream);
    if (h->ws) (void)hipFree(h->ws);
    if (h->st) (void)hipStreamDestroy(h->st);
    if (h->cp) (void)hipStreamDestroy(h->cp);
    delete h;
    return VGL_OK;
}

extern "C" int vgl_stream_host_create(int32_t device, int32_t n_buffers, int32_t max_sites, int64_t max_head_bytes, int64_t max_body_bytes,
                                      vgl_stream_host** out) {
    if (!out) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_create: null out");
    *out = nullptr;
    if (n_buffers < 1 || n_buffers > 8) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_create: n_buffers outside [1, 8]");
    if (max_sites < 1) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_create: max_sites below 1");
    if (max_head_bytes < 1) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_create: max_head_bytes below 1");
    if (max_body_bytes < 1) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_create: max_body_bytes below 1");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_create: no HIP device is available");
    if (device < 0 || device >= nd) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_create: no such device");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_create: hipSetDevice failed");
    vgl_stream_host* h = new vgl_stream_host;
    h->device = device; h->nb = n_buffers; h->max_sites = max_sites; h->max_head = max_head_bytes; h->max_body = max_body_bytes;
    h->cap = max_head_bytes + max_body_bytes; h->ws_bytes = vgl_bgzf_workspace_bytes(h->cap); h->out_cap = vgl_bgzf_bound(h->cap);
    h->b.resize((size_t)n_buffers);
    const size_t off_bytes = 2 * ((size_t)max_sites + 1) * sizeof(int64_t);
    bool ok = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&h->cp, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc((void**)&h->d_stream, (size_t)h->cap) == hipSuccess && hipMalloc(&h->ws, (size_t)h->ws_bytes) == hipSuccess;
    for (auto& B : h->b)
        ok = ok && hipMalloc((void**)&B.d_body, (size_t)max_body_bytes) == hipSuccess && hipMalloc((void**)&B.d_heads, (size_t)max_head_bytes) == hipSuccess &&
             hipMalloc((void**)&B.d_off, off_bytes) == hipSuccess && hipHostMalloc((void**)&B.h_heads, (size_t)max_head_bytes, hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void**)&B.h_off, off_bytes, hipHostMallocDefault) == hipSuccess && hipMalloc((void**)&B.d_mem, (size_t)h->out_cap) == hipSuccess &&
             hipMalloc((void**)&B.d_n, 2 * sizeof(int64_t)) == hipSuccess &&
             hipHostMalloc((void**)&B.h_n, 2 * sizeof(int64_t), hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&B.done, hipEventDisableTiming) == hipSuccess;
    if (!ok) { vgl_stream_host_destroy(h); return vgl_pack_set_error(VGL_E_NOMEM, "vgl_stream_host_create: device or page-locked memory could not be allocated"); }
    *out = h;
    return VGL_OK;
}

// a failure after work was enqueued: the buffer stays free, so whatever already runs on the stream must be over before the caller can
// submit again and overwrite the page-locked staging
static int submit_failed(vgl_stream_host* h, int code, const char* msg) {
    (void)hipStreamSynchronize(h->st);
    return msg ? vgl_pack_set_error(code, msg) : code;      // (msg = NULL: the callee's message stands)
}

extern "C" uint8_t* vgl_stream_host_body(vgl_stream_host* h, int32_t k) {
    if (!h || k < 0 || k >= h->nb) { vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_body: k is out of range"); return nullptr; }
    return h->b[(size_t)k].d_body;
}

extern "C" int vgl_stream_host_submit(vgl_stream_host* h, int32_t k, int32_t n_sites, const uint8_t* heads, const int64_t* head_offsets,
                                      const int64_t* body_offsets, int32_t* ticket) {
    if (!h || !ticket) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: null handle or ticket");
    if (k < 0 || k >= h->nb) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: k is out of range");
    auto& B = h->b[(size_t)k];
    if (B.busy) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: buffer k is still in flight (vgl_stream_host_wait its ticket first)");
    if (n_sites < 0 || n_sites > h->max_sites) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: n_sites outside [0, max_sites]");
    int64_t hb = 0, bb = 0;
    if (n_sites > 0) {
        if (!head_offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: null head_offsets");
        if (!body_offsets) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: null body_offsets");
        for (int32_t i = 0; i < n_sites; i++) {
            if (head_offsets[i + 1] < head_offsets[i]) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: head_offsets is not monotone");
            if (body_offsets[i + 1] < body_offsets[i]) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: body_offsets is not monotone");
        }
        hb = head_offsets[n_sites] - head_offsets[0]; bb = body_offsets[n_sites] - body_offsets[0];
        if (hb > h->max_head) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: head_offsets spans more than max_head_bytes");
        if (body_offsets[0] < 0 || body_offsets[n_sites] > h->max_body) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: body_offsets leaves the body buffer (max_body_bytes)");
        if (hb > 0 && !heads) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_submit: null heads");
    }
    const int64_t raw = hb + bb;
    if (hipSetDevice(h->device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_submit: hipSetDevice failed");
    B.h_n[0] = 0; B.h_n[1] = 0;
    if (raw > 0) {
        // the caller's arrays are free again when this returns: page-locked copies go up the link
        const size_t no = (size_t)n_sites + 1;
        memcpy(B.h_off, head_offsets, no * sizeof(int64_t));
        memcpy(B.h_off + no, body_offsets, no * sizeof(int64_t));
        if (hb > 0) memcpy(B.h_heads, heads + head_offsets[0], (size_t)hb);
        bool ok = hipMemcpyAsync(B.d_off, B.h_off, 2 * no * sizeof(int64_t), hipMemcpyHostToDevice, h->st) == hipSuccess;
        if (hb > 0) ok = ok && hipMemcpyAsync(B.d_heads, B.h_heads, (size_t)hb, hipMemcpyHostToDevice, h->st) == hipSuccess;
        if (!ok) return submit_failed(h, VGL_E_NODEVICE, "vgl_stream_host_submit: copy to the device failed");
        int rc = vgl_stream_assemble_device(h->device, n_sites, B.d_heads, B.d_off, B.d_body + body_offsets[0], B.d_off + no, h->d_stream, raw, B.d_n, h->st);
        if (rc == VGL_OK) rc = vgl_bgzf_compress_device(h->device, h->d_stream, raw, B.d_mem, h->out_cap, B.d_n + 1, h->ws, h->ws_bytes, h->st);
        if (rc != VGL_OK) return submit_failed(h, rc, nullptr);
        if (hipMemcpyAsync(B.h_n, B.d_n, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->st) != hipSuccess)
            return submit_failed(h, VGL_E_NODEVICE, "vgl_stream_host_submit: enqueue failed");
    }
    if (hipEventRecord(B.done, h->st) != hipSuccess) return submit_failed(h, VGL_E_NODEVICE, "vgl_stream_host_submit: enqueue failed");
    B.raw = raw; B.seq = h->next_seq++; B.busy = true;
    *ticket = k;
    return VGL_OK;
}

extern "C" int vgl_stream_host_wait(vgl_stream_host* h, int32_t ticket, const uint8_t** members, int64_t* members_n, int64_t* raw_n) {
    if (!h || !members || !members_n) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_wait: null argument");
    if (ticket < 0 || ticket >= h->nb || !h->b[(size_t)ticket].busy) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_wait: bad ticket");
    auto& B = h->b[(size_t)ticket];
    if (B.seq != h->wait_seq) return vgl_pack_set_error(VGL_E_ARG, "vgl_stream_host_wait: tickets are waited for in submit order");
    if (hipSetDevice(h->device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_wait: hipSetDevice failed");
    if (hipEventSynchronize(B.done) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_wait: the assembly or compression failed");
    B.busy = false; h->wait_seq++;
    int64_t m = 0;
    if (B.raw > 0) {
        m = B.h_n[1];
        if (B.h_n[0] != B.raw) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_wait: the assembled length differs from the offsets' total");
        if (m <= 0 || m > vgl_bgzf_bound(B.raw)) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_wait: compressed size out of range");
        if (m > B.h_mem_cap) {
            const int64_t want = std::min(h->out_cap, std::max<int64_t>(m + m / 4, 1 << 20));
            if (B.h_mem) (void)hipHostFree(B.h_mem);
            B.h_mem = nullptr; B.h_mem_cap = 0;
            if (hipHostMalloc((void**)&B.h_mem, (size_t)want, hipHostMallocDefault) != hipSuccess)
                return vgl_pack_set_error(VGL_E_NOMEM, "vgl_stream_host_wait: page-locked memory for the members could not be allocated");
            B.h_mem_cap = want;
        }
        if (hipMemcpyAsync(B.h_mem, B.d_mem, (size_t)m, hipMemcpyDeviceToHost, h->cp) != hipSuccess || hipStreamSynchronize(h->cp) != hipSuccess)
            return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_stream_host_wait: copy back failed");
    }
    *members = B.h_mem; *members_n = m;
    if (raw_n) *raw_n = B.raw;
    return VGL_OK;
}
