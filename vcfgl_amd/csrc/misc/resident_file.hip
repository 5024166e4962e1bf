// resident_file.hip -- a BGZF file of VCF text inflated into one device buffer and split into lines there (a translation unit of the
// program that links it: the library gets no entry point).  The per-byte and per-line rules are rf_core.h.
//   k_rf_count      a workgroup of RF_NT lanes per chunk of RF_CHUNK bytes, a lane per piece of 16: the '\n' of the chunk.  A piece that
//                   lies whole inside the text on a 16-byte address is one load, any other is read byte by byte inside the text
//   k_offsets_scan  (wg_scan.hip.h) the counts -> the first line ordinal of every chunk
//   k_rf_ends       the same walk: a lane's count goes through a ballot / popcount prefix inside its wavefront (five ballots: a count
//                   has five bits), the wavefronts' totals through LDS, and every lane stores the places of its '\n' in order; the
//                   entry behind the last '\n' is `total` (a last line without one ends there)
//   k_rf_head_len   a lane per line: rf::classify -> head length + 1, the sample columns' offset and length; a line that cannot be
//                   classified within head_most bytes raises the file's flag
//   k_offsets_scan  the head lengths + 1 -> where every head begins in the stream
//   k_rf_head_copy  a wavefront per line: the head's bytes and a '\n' behind them
// No kernel reads outside [0, total) or stores outside the arrays it is given (every index is compared with the array's length).
// A BCF file (--resident-bcf 1) is walked by the kernels further down: k_rb_chain, k_rb_head_len, k_rb_head_copy (rb_core.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>

#include "../../../include/vcfgl_hip.h"
#include "resident_file.h"
#include "rb_core.h"
#include "wg_scan.hip.h"
#include "batch_dev.hip.h"

namespace {

using rf::RF_NT;
using rf::RF_LANE;
using rf::RF_CHUNK;

constexpr int GRID_MOST = 2048;          // workgroups of a launch; the chunks and lines beyond are taken in a grid stride

__global__ void __launch_bounds__(RF_NT) k_rf_count(const uint8_t* __restrict__ text, const int64_t total, const int64_t n_chunks, int64_t* __restrict__ counts) {
    __shared__ int32_t s_n[2][RF_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int parity = 0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x, parity ^= 1) {
        uint32_t w[4];
        rf::load_piece(text, c * RF_CHUNK + (int64_t)t * RF_LANE, total, w);
        int32_t n = __popc(rf::newline_mask(w));
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
        if (lane == 0) s_n[parity][wave] = n;
        __syncthreads();
        if (t == 0) { int32_t x = 0; for (int k = 0; k < RF_NT / 64; k++) x += s_n[parity][k]; counts[c] = x; }
    }
}

__global__ void __launch_bounds__(RF_NT) k_rf_ends(const uint8_t* __restrict__ text, const int64_t total, const int64_t n_chunks, const int64_t* __restrict__ first,
                                                  int64_t* __restrict__ ends, const int64_t n_ends) {
    __shared__ int32_t s_n[2][RF_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int parity = 0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x, parity ^= 1) {
        const int64_t o = c * RF_CHUNK + (int64_t)t * RF_LANE;
        uint32_t w[4];
        rf::load_piece(text, o, total, w);
        uint32_t mask = rf::newline_mask(w);
        const int32_t cnt = __popc(mask);                              // 0 .. 16
        int32_t pre = 0, sum = 0;
#pragma unroll
        for (int b = 0; b < 5; b++) {
            const unsigned long long has = __ballot((cnt >> b) & 1);
            pre += __popcll(has & below) << b; sum += __popcll(has) << b;
        }
        if (lane == 0) s_n[parity][wave] = sum;
        __syncthreads();
        int32_t before = 0;
#pragma unroll
        for (int k = 0; k < RF_NT / 64; k++) if (k < wave) before += s_n[parity][k];
        int64_t at = first[c] + before + pre;
        while (mask) {
            const int i = __ffs(mask) - 1; mask &= mask - 1;
            if (at >= 0 && at < n_ends) ends[at] = o + i;
            at++;
        }
    }
    if (blockIdx.x == 0 && t == 0 && n_ends > 0) ends[n_ends - 1] = total;
}

struct HeadArgs {
    const uint8_t* text; int64_t total;
    const int64_t* ends; int64_t n_lines;
    int64_t head_most;
    int64_t* hl1; int64_t* s_off; int64_t* s_len;
    int32_t* over;
};

__global__ void __launch_bounds__(RF_NT) k_rf_head_len(const HeadArgs A) {
    for (int64_t i = (int64_t)blockIdx.x * RF_NT + threadIdx.x; i < A.n_lines; i += (int64_t)gridDim.x * RF_NT) {
        int64_t b = rf::line_begin(A.ends, i), e = A.ends[i];
        if (e > A.total) e = A.total;
        if (e < 0) e = 0;
        if (b < 0) b = 0;
        if (b > e) b = e;                                              // (the ends ascend inside the text: never so)
        const rf::Head h = rf::classify(A.text, b, e, A.head_most);
        A.hl1[i] = h.head_len + 1; A.s_off[i] = h.s_off; A.s_len[i] = h.s_len;
        if (h.over) *A.over = 1;
    }
}

struct CopyArgs {
    const uint8_t* text; int64_t total;
    const int64_t* ends; const int64_t* hoff; int64_t n_lines;
    uint8_t* heads; int64_t head_bytes;
};

__global__ void __launch_bounds__(RF_NT) k_rf_head_copy(const CopyArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * (RF_NT / 64) + wave; i < A.n_lines; i += (int64_t)gridDim.x * (RF_NT / 64)) {
        const int64_t b = rf::line_begin(A.ends, i), at = A.hoff[i], n = A.hoff[i + 1] - at - 1;
        if (b < 0 || n < 0 || b + n > A.total || at < 0 || at + n + 1 > A.head_bytes) continue;     // (uniform over the wavefront)
        for (int64_t j = lane; j < n; j += 64) A.heads[at + j] = A.text[b + j];
        if (lane == 0) A.heads[at + n] = (uint8_t)'\n';
    }
}

// ---- a resident BCF file (rb_core.h) ----------------------------------------------------------------------------------------------
//   k_rb_chain      the serial part, one wavefront: the lanes load a window of RB_WINDOW bytes into LDS (a piece of 16 a lane, as
//                   k_rf_count loads it), the lengths of the records inside the window are followed from LDS, and the window is loaded
//                   again only when the next record's lengths lie outside it.  At most hops_most records a launch: their offsets go
//                   into a buffer of that many entries, and where the launch stopped goes back to the host, which launches again.
//                   Every hop moves on by RB_REC_LEAST bytes at least.
//   k_rb_head_len   a lane per record: rb::format_walk (a loop of n_fmt <= 255 fields, and of the shared block's n_allele + n_info
//                   <= 2^17 items) -> the head's length; a record the walk hands back raises the file's flag, the lowest ordinal wins
//   k_offsets_scan  the head lengths -> where every head begins in the stream
//   k_rb_head_copy  a wavefront per record: the lengths and the shared block lane by lane, then the fields' headers by walking the
//                   fields again (rb::fields_walk; the shared block was walked by k_rb_head_len and is not walked twice)
// No kernel waits for another; every store is compared with its array's length.
struct ChainArgs {
    const uint8_t* bytes; int64_t total, o0, hops_most;
    int64_t* offs; int64_t offs_cap;
    rb::ChainEnd* end;
};

__global__ void __launch_bounds__(rb::RB_WIN_LANES) k_rb_chain(const ChainArgs A) {
    __shared__ uint32_t s_win[rb::RB_WINDOW / 4];
    const int lane = threadIdx.x;
    // (every value below is the same in all lanes: the loop and its barriers are uniform)
    int64_t o = A.o0, wb = -1, taken = 0;
    int32_t why = rb::OK, done = 0;
    while (taken < A.hops_most && taken < A.offs_cap) {
        if (o == A.total) { done = 1; break; }
        if (o < 0 || o + 8 > A.total) { why = rb::W_LENGTHS; break; }
        if (wb < 0 || o < wb || o + 8 > wb + rb::RB_WINDOW) {
            wb = o & ~(int64_t)(RF_LANE - 1);
            uint32_t w[4];
            rf::load_piece(A.bytes, wb + (int64_t)lane * RF_LANE, A.total, w);
            __syncthreads();
            s_win[lane * 4 + 0] = w[0]; s_win[lane * 4 + 1] = w[1]; s_win[lane * 4 + 2] = w[2]; s_win[lane * 4 + 3] = w[3];
            __syncthreads();
        }
        uint32_t l_shared, l_indiv; int64_t rec_end;
        rb::win_lengths(s_win, o - wb, l_shared, l_indiv);
        why = rb::step_rule(o, A.total, l_shared, l_indiv, rec_end);
        if (why != rb::OK) break;
        if (lane == 0) A.offs[taken] = o;
        taken++;
        o = rec_end;
    }
    if (lane == 0) { A.end->next = o; A.end->taken = taken; A.end->done = done; A.end->why = why; }
}

struct RbHeadArgs {
    const uint8_t* bytes; int64_t total;
    const int64_t* rec_off; int64_t n_recs, N, head_most;
    int64_t* hl;
    unsigned long long* flag;
};

__global__ void __launch_bounds__(RF_NT) k_rb_head_len(const RbHeadArgs A) {
    for (int64_t i = (int64_t)blockIdx.x * RF_NT + threadIdx.x; i < A.n_recs; i += (int64_t)gridDim.x * RF_NT) {
        int64_t len = 0;
        const int st = rb::format_walk(A.bytes, A.total, A.rec_off[i], A.N, A.head_most, len, [](int, int64_t, int64_t, int32_t, int32_t, int64_t, int64_t) {});
        A.hl[i] = st == rb::OK ? len : 0;
        if (st != rb::OK) atomicMin(A.flag, rb::flag_word(i, st));
    }
}

struct RbCopyArgs {
    const uint8_t* bytes; int64_t total;
    const int64_t* rec_off; const int64_t* hoff; int64_t n_recs, N, head_most;
    uint8_t* heads; int64_t head_bytes;
};

__global__ void __launch_bounds__(RF_NT) k_rb_head_copy(const RbCopyArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * (RF_NT / 64) + wave; i < A.n_recs; i += (int64_t)gridDim.x * (RF_NT / 64)) {
        const int64_t o = A.rec_off[i], at = A.hoff[i], n = A.hoff[i + 1] - at;
        rb::Lead L;
        if (rb::record_lead(A.bytes, A.total, o, A.N, A.head_most, L) != rb::OK) continue;       // (uniform over the wavefront)
        const int64_t lead = 8 + (int64_t)L.l_shared, hi = at + n < A.head_bytes ? at + n : A.head_bytes;
        if (at < 0 || n < lead) continue;
        for (int64_t j = lane; j < lead; j += 64) if (at + j < hi) A.heads[at + j] = A.bytes[o + j];
        // the fields alone: k_rb_head_len has taken the record, its shared block is not walked again
        int64_t w = at + lead, hdr;
        rb::fields_walk(A.bytes, L.se, L.rec_end, L.n_fmt, A.N, hdr, [&](int, int64_t hdr_at, int64_t hdr_len, int32_t, int32_t, int64_t, int64_t) {
            for (int64_t j = lane; j < hdr_len; j += 64) if (w + j < hi) A.heads[w + j] = A.bytes[hdr_at + j];
            w += hdr_len;
        });
    }
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
unsigned grid_for(int64_t n) { return (unsigned)(n < 1 ? 1 : n > GRID_MOST ? GRID_MOST : n); }

const int64_t PIECE = 16ll << 20;        // bytes of the file per upload
const int64_t MEMBERS_A_CALL = 4096;     // members per vgl_inflate_members_device call (it waits for its range check)

}  // namespace

struct RfFile {
    int device = 0;
    batchdev::Stream stream;
    batchdev::Event ev[2];
    batchdev::PinMem<uint8_t> pin[2];
    batchdev::DevMem<uint8_t> d_src, d_text;
    int64_t total = 0;
    RfStats st;
    char err[512] = {0};

    ~RfFile() { if (stream.h) (void)hipStreamSynchronize(stream); }
    int refuse(const char* why) { snprintf(err, sizeof err, "%s", why); return -1; }
    int fail(const char* what, hipError_t e) { snprintf(err, sizeof err, "%s: %s", what, hipGetErrorString(e)); return -1; }
    int open(int dev) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return refuse("no HIP device is available");
        if (dev < 0 || dev >= nd) return refuse("no such device");
        device = dev;
        BATCH_HIP(this, hipSetDevice(device));
        BATCH_HIP(this, hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking));
        for (batchdev::Event& e : ev) BATCH_HIP(this, hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
        return 0;
    }
};

RfFile* rf_create(int device, char* err, size_t err_len) {
    RfFile* f = new RfFile();
    if (f->open(device) == 0) return f;
    snprintf(err, err_len, "%s", f->err);
    delete f;
    return nullptr;
}
void rf_destroy(RfFile* f) { delete f; }
const char* rf_error(RfFile* f) { return f->err; }
int64_t rf_total(const RfFile* f) { return f->total; }
const uint8_t* rf_device_text(const RfFile* f) { return f->d_text; }
const RfStats* rf_stats(const RfFile* f) { return &f->st; }

int64_t rf_default_max_bytes(RfFile* f) {
    size_t free_b = 0, all_b = 0;
    if (hipSetDevice(f->device) != hipSuccess || hipMemGetInfo(&free_b, &all_b) != hipSuccess) return 0;
    const int64_t x = (int64_t)free_b - (1ll << 30);
    return x > 0 ? x : 0;
}

int rf_load(RfFile* f, const char* path, int64_t max_bytes, RfWhy* why) {
    *why = RF_NOT_BGZF;
    f->d_src.release(); f->d_text.release(); f->total = 0; f->st = RfStats();
    BATCH_HIP(f, hipSetDevice(f->device));
    double t0 = now();
    FILE* fp = fopen(path, "rb");
    if (!fp) { snprintf(f->err, sizeof f->err, "Could not open file: %s", path); return -1; }
    struct Close { FILE* p; ~Close() { fclose(p); } } closer{fp};
    if (fseeko(fp, 0, SEEK_END) != 0) return 0;                        // (not a file that can be sized: zlib reads it)
    const int64_t size = (int64_t)ftello(fp);
    if (size < 28 || fseeko(fp, 0, SEEK_SET) != 0) return 0;
    uint8_t magic[4] = {0, 0, 0, 0};                                   // a file that does not begin as a BGZF member is not sent at all
    if (fread(magic, 1, 4, fp) != 4 || !(magic[0] == 0x1f && magic[1] == 0x8b && magic[2] == 8 && (magic[3] & 4)) || fseeko(fp, 0, SEEK_SET) != 0) return 0;
    if (size > max_bytes) { *why = RF_TOO_LARGE; return 0; }
    for (batchdev::PinMem<uint8_t>& p : f->pin) if (!p.alloc(f->device, (size_t)(size < PIECE ? size : PIECE))) {
        snprintf(f->err, sizeof f->err, "page-locked host memory could not be allocated: %s", vgl_last_error()); return -1;
    }
    if (f->d_src.alloc((size_t)size) != hipSuccess) { (void)hipGetLastError(); f->d_src.p = nullptr; *why = RF_TOO_LARGE; return 0; }
    std::vector<uint8_t> file((size_t)size);
    // a piece is copied up while the next is read
    int64_t off = 0;
    for (int k = 0; off < size; k++) {
        const int s = k & 1;
        if (k >= 2) BATCH_HIP(f, hipEventSynchronize(f->ev[s]));
        const int64_t want = size - off < PIECE ? size - off : PIECE;
        const size_t got = fread(f->pin[s], 1, (size_t)want, fp);
        if ((int64_t)got != want) { (void)hipStreamSynchronize(f->stream); return f->refuse("the file changed while it was read"); }
        memcpy(file.data() + off, f->pin[s], got);
        BATCH_HIP(f, hipMemcpyAsync(f->d_src + off, f->pin[s], got, hipMemcpyHostToDevice, f->stream));
        BATCH_HIP(f, hipEventRecord(f->ev[s], f->stream));
        off += (int64_t)got;
    }
    // the members, while the last pieces fly
    const int64_t cap = size / 28 + 1;
    std::vector<int64_t> begin((size_t)cap), out_off((size_t)cap); std::vector<int32_t> csize((size_t)cap), isize((size_t)cap);
    int64_t n = 0;
    const int rc = vgl_bgzf_index(file.data(), size, cap, begin.data(), csize.data(), isize.data(), &n);
    std::vector<uint8_t>().swap(file);
    BATCH_HIP(f, hipStreamSynchronize(f->stream));
    f->st.compressed_up = size; f->st.t_upload = now() - t0; t0 = now();
    if (rc != VGL_OK || n <= 0) { f->d_src.release(); return 0; }
    int64_t total = 0;
    for (int64_t m = 0; m < n; m++) { out_off[(size_t)m] = total; total += isize[(size_t)m]; }
    if (total + size > max_bytes) { f->d_src.release(); *why = RF_TOO_LARGE; return 0; }
    batchdev::DevMem<int64_t> d_begin, d_out; batchdev::DevMem<int32_t> d_csize, d_isize, d_status; batchdev::DevMem<uint8_t> d_ws;
    const int64_t ws = vgl_inflate_workspace_bytes(n < MEMBERS_A_CALL ? n : MEMBERS_A_CALL);
    if (f->d_text.alloc((size_t)(total > 0 ? total : 1)) != hipSuccess) { (void)hipGetLastError(); f->d_text.p = nullptr; f->d_src.release(); *why = RF_TOO_LARGE; return 0; }
    BATCH_HIP(f, d_begin.alloc((size_t)n * 8)); BATCH_HIP(f, d_out.alloc((size_t)n * 8));
    BATCH_HIP(f, d_csize.alloc((size_t)n * 4)); BATCH_HIP(f, d_isize.alloc((size_t)n * 4)); BATCH_HIP(f, d_status.alloc((size_t)n * 4));
    BATCH_HIP(f, d_ws.alloc((size_t)(ws > 0 ? ws : 1)));
    BATCH_HIP(f, hipMemcpyAsync(d_begin, begin.data(), (size_t)n * 8, hipMemcpyHostToDevice, f->stream));
    BATCH_HIP(f, hipMemcpyAsync(d_out, out_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, f->stream));
    BATCH_HIP(f, hipMemcpyAsync(d_csize, csize.data(), (size_t)n * 4, hipMemcpyHostToDevice, f->stream));
    BATCH_HIP(f, hipMemcpyAsync(d_isize, isize.data(), (size_t)n * 4, hipMemcpyHostToDevice, f->stream));
    BATCH_HIP(f, hipStreamSynchronize(f->stream));
    for (int64_t m0 = 0; m0 < n; m0 += MEMBERS_A_CALL) {
        const int64_t cnt = n - m0 < MEMBERS_A_CALL ? n - m0 : MEMBERS_A_CALL;
        if (vgl_inflate_members_device(f->device, f->d_src, size, cnt, d_begin + m0, d_csize + m0, d_out + m0, d_isize + m0, f->d_text, total,
                                       d_status + m0, d_ws, ws, (void*)f->stream.h) != VGL_OK) {
            (void)hipStreamSynchronize(f->stream);
            return f->refuse(vgl_last_error());
        }
    }
    std::vector<int32_t> status((size_t)n);
    BATCH_HIP(f, hipMemcpyAsync(status.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    BATCH_HIP(f, hipStreamSynchronize(f->stream));
    f->d_src.release();                                                // the compressed bytes have done their work
    f->st.members = n; f->st.t_inflate = now() - t0;
    for (int64_t m = 0; m < n; m++) if (status[(size_t)m] != VGL_INFLATE_OK) { f->d_text.release(); *why = RF_MEMBER_HOST; return 0; }
    f->total = total; f->st.total = total;
    *why = RF_RESIDENT;
    return 0;
}

int rf_fetch(RfFile* f, int64_t off, int64_t n, uint8_t* dst) {
    if (off < 0 || n < 0 || off + n > f->total) return f->refuse("a span outside the resident text");
    if (n == 0) return 0;
    BATCH_HIP(f, hipSetDevice(f->device));
    BATCH_HIP(f, hipMemcpyAsync(dst, f->d_text + off, (size_t)n, hipMemcpyDeviceToHost, f->stream));
    BATCH_HIP(f, hipStreamSynchronize(f->stream));
    f->st.down += n;
    return 0;
}

int rf_split(RfFile* f, int64_t head_most, rf::Split* out, bool* more_lines) {
    *out = rf::Split(); *more_lines = false;
    const int64_t total = f->total;
    if (total <= 0) return 0;
    if (head_most < 1) return f->refuse("head-most must be at least 1");
    BATCH_HIP(f, hipSetDevice(f->device));
    const double t0 = now();
    hipStream_t st = f->stream;
    const uint8_t* text = f->d_text;
    const int64_t n_chunks = (total + RF_CHUNK - 1) / RF_CHUNK;
    const int64_t SCAN_MOST = (int64_t)INT32_MAX - wgscan::SCAN_NT;    // k_offsets_scan rounds its count up to whole chunks in an int
    if (n_chunks > SCAN_MOST) { *more_lines = true; return 0; }
    batchdev::DevMem<int64_t> d_counts, d_first, d_ends, d_hl1, d_hoff, d_soff, d_slen; batchdev::DevMem<int32_t> d_over; batchdev::DevMem<uint8_t> d_heads;
    BATCH_HIP(f, d_counts.alloc((size_t)n_chunks * 8)); BATCH_HIP(f, d_first.alloc(((size_t)n_chunks + 1) * 8));
    hipLaunchKernelGGL(k_rf_count, dim3(grid_for(n_chunks)), dim3(RF_NT), 0, st, text, total, n_chunks, (int64_t*)d_counts);
    BATCH_HIP(f, hipGetLastError());
    hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(1), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)d_counts, (int64_t*)d_first, (int32_t)n_chunks);
    BATCH_HIP(f, hipGetLastError());
    int64_t n_nl = 0; uint8_t last = 0;
    BATCH_HIP(f, hipMemcpyAsync(&n_nl, d_first + n_chunks, 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(&last, text + (total - 1), 1, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipStreamSynchronize(st));
    if (n_nl < 0 || n_nl > total) return f->refuse("the newline count is outside the text's length");
    const int64_t L = n_nl + (last != (uint8_t)'\n' ? 1 : 0);
    if (L > SCAN_MOST) { *more_lines = true; return 0; }
    const int64_t n_ends = n_nl + 1;
    BATCH_HIP(f, d_ends.alloc((size_t)n_ends * 8));
    hipLaunchKernelGGL(k_rf_ends, dim3(grid_for(n_chunks)), dim3(RF_NT), 0, st, text, total, n_chunks, (const int64_t*)d_first, (int64_t*)d_ends, n_ends);
    BATCH_HIP(f, hipGetLastError());
    out->lines = L; f->st.lines = L;
    if (L == 0) { BATCH_HIP(f, hipStreamSynchronize(st)); f->st.t_split = now() - t0; out->hoff.assign(1, 0); return 0; }
    BATCH_HIP(f, d_hl1.alloc((size_t)L * 8)); BATCH_HIP(f, d_hoff.alloc(((size_t)L + 1) * 8));
    BATCH_HIP(f, d_soff.alloc((size_t)L * 8)); BATCH_HIP(f, d_slen.alloc((size_t)L * 8)); BATCH_HIP(f, d_over.alloc(4));
    BATCH_HIP(f, hipMemsetAsync(d_over, 0, 4, st));
    const HeadArgs H{text, total, d_ends, L, head_most, d_hl1, d_soff, d_slen, d_over};
    hipLaunchKernelGGL(k_rf_head_len, dim3(grid_for((L + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, H);
    BATCH_HIP(f, hipGetLastError());
    hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(1), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)d_hl1, (int64_t*)d_hoff, (int32_t)L);
    BATCH_HIP(f, hipGetLastError());
    int64_t head_bytes = 0; int32_t over = 0;
    BATCH_HIP(f, hipMemcpyAsync(&head_bytes, d_hoff + L, 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipStreamSynchronize(st));
    out->over = over != 0;
    if (out->over) { f->st.t_split = now() - t0; return 0; }
    if (head_bytes < L || head_bytes > total + L) return f->refuse("the head stream is longer than the text and its lines");
    BATCH_HIP(f, d_heads.alloc((size_t)head_bytes));
    const CopyArgs C{text, total, d_ends, d_hoff, L, d_heads, head_bytes};
    hipLaunchKernelGGL(k_rf_head_copy, dim3(grid_for((L + RF_NT / 64 - 1) / (RF_NT / 64))), dim3(RF_NT), 0, st, C);
    BATCH_HIP(f, hipGetLastError());
    out->heads.resize((size_t)head_bytes); out->hoff.resize((size_t)L + 1); out->s_off.resize((size_t)L); out->s_len.resize((size_t)L);
    BATCH_HIP(f, hipMemcpyAsync(out->heads.data(), d_heads, (size_t)head_bytes, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(out->hoff.data(), d_hoff, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(out->s_off.data(), d_soff, (size_t)L * 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(out->s_len.data(), d_slen, (size_t)L * 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipStreamSynchronize(st));
    f->st.head_bytes = head_bytes; f->st.down += head_bytes + (3 * L + 1) * 8; f->st.t_split = now() - t0;
    return 0;
}

// ---- a resident BCF file ----------------------------------------------------------------------------------------------------------
int rf_bcf_header(RfFile* f, std::vector<uint8_t>* hdr, bool* fits) {
    hdr->clear(); *fits = false;
    if (f->total < 9) return 0;
    uint8_t lead[9];
    if (rf_fetch(f, 0, 9, lead) != 0) return -1;
    if (memcmp(lead, "BCF\2", 4) != 0) return 0;
    const int64_t l_text = (int64_t)rb::rd_u32(lead, 5);
    if (9 + l_text > f->total) return 0;
    hdr->resize((size_t)(9 + l_text));
    if (rf_fetch(f, 0, 9 + l_text, hdr->data()) != 0) return -1;
    *fits = true;
    return 0;
}

int rf_bcf_split(RfFile* f, int64_t start, int64_t n_samples, int64_t hops_most, int64_t head_most, RbSplit* out) {
    *out = RbSplit();
    const int64_t total = f->total;
    if (start < 0 || start > total || n_samples < 0 || hops_most < 1 || head_most < 24) return f->refuse("a resident BCF split outside its bounds");
    BATCH_HIP(f, hipSetDevice(f->device));
    double t0 = now();
    hipStream_t st = f->stream;
    const uint8_t* bytes = f->d_text;
    const int64_t SCAN_MOST = (int64_t)INT32_MAX - wgscan::SCAN_NT;
    // the chain: hops_most records a launch
    const int64_t room = (total - start) / rb::RB_REC_LEAST + 1, cap = hops_most < room ? hops_most : room;
    batchdev::DevMem<int64_t> d_hop; batchdev::DevMem<rb::ChainEnd> d_end;
    BATCH_HIP(f, d_hop.alloc((size_t)cap * 8)); BATCH_HIP(f, d_end.alloc(sizeof(rb::ChainEnd)));
    std::vector<int64_t>& rec_off = out->rec_off;
    for (int64_t o = start;;) {
        const ChainArgs A{bytes, total, o, hops_most, d_hop, cap, d_end};
        hipLaunchKernelGGL(k_rb_chain, dim3(1), dim3(rb::RB_WIN_LANES), 0, st, A);
        BATCH_HIP(f, hipGetLastError());
        rb::ChainEnd e;
        BATCH_HIP(f, hipMemcpyAsync(&e, d_end, sizeof e, hipMemcpyDeviceToHost, st));
        BATCH_HIP(f, hipStreamSynchronize(st));
        f->st.chain_launches++;
        if (e.taken < 0 || e.taken > cap || e.next < o || e.next > total) return f->refuse("a chain launch ended outside the file");
        if (e.taken > 0) {
            const size_t at = rec_off.size();
            rec_off.resize(at + (size_t)e.taken);
            BATCH_HIP(f, hipMemcpyAsync(rec_off.data() + at, d_hop, (size_t)e.taken * 8, hipMemcpyDeviceToHost, st));
            BATCH_HIP(f, hipStreamSynchronize(st));
            f->st.down += e.taken * 8;
        }
        if ((int64_t)rec_off.size() > SCAN_MOST) { out->more_records = true; rec_off.clear(); f->st.t_chain = now() - t0; return 0; }
        if (e.why != rb::OK) { out->why = e.why; out->ordinal = (int64_t)rec_off.size(); break; }
        if (e.done) break;
        if (e.taken == 0) return f->refuse("a chain launch took no record");
        o = e.next;
    }
    const int64_t R = (int64_t)rec_off.size();
    out->records = R; f->st.records = R; f->st.t_chain = now() - t0; t0 = now();
    out->hoff.assign(1, 0);
    if (out->why != rb::OK || R == 0) return 0;
    // the heads
    batchdev::DevMem<int64_t> d_rec, d_hl, d_hoff; batchdev::DevMem<unsigned long long> d_flag; batchdev::DevMem<uint8_t> d_heads;
    BATCH_HIP(f, d_rec.alloc((size_t)R * 8)); BATCH_HIP(f, d_hl.alloc((size_t)R * 8)); BATCH_HIP(f, d_hoff.alloc(((size_t)R + 1) * 8)); BATCH_HIP(f, d_flag.alloc(8));
    BATCH_HIP(f, hipMemcpyAsync(d_rec, rec_off.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
    BATCH_HIP(f, hipMemsetAsync(d_flag, 0xFF, 8, st));
    const RbHeadArgs H{bytes, total, d_rec, R, n_samples, head_most, d_hl, d_flag};
    hipLaunchKernelGGL(k_rb_head_len, dim3(grid_for((R + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, H);
    BATCH_HIP(f, hipGetLastError());
    hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(1), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)d_hl, (int64_t*)d_hoff, (int32_t)R);
    BATCH_HIP(f, hipGetLastError());
    int64_t head_bytes = 0; unsigned long long flag = rb::FLAG_NONE;
    BATCH_HIP(f, hipMemcpyAsync(&head_bytes, d_hoff + R, 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(&flag, d_flag, 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipStreamSynchronize(st));
    if (flag != rb::FLAG_NONE) { out->why = (int)(flag & 0xFF); out->ordinal = (int64_t)(flag >> 8); f->st.t_heads = now() - t0; return 0; }
    if (head_bytes < R * rb::RB_REC_LEAST || head_bytes > total) return f->refuse("the head stream is longer than the file");
    BATCH_HIP(f, d_heads.alloc((size_t)head_bytes));
    const RbCopyArgs C{bytes, total, d_rec, d_hoff, R, n_samples, head_most, d_heads, head_bytes};
    hipLaunchKernelGGL(k_rb_head_copy, dim3(grid_for((R + RF_NT / 64 - 1) / (RF_NT / 64))), dim3(RF_NT), 0, st, C);
    BATCH_HIP(f, hipGetLastError());
    out->heads.resize((size_t)head_bytes); out->hoff.resize((size_t)R + 1);
    BATCH_HIP(f, hipMemcpyAsync(out->heads.data(), d_heads, (size_t)head_bytes, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipMemcpyAsync(out->hoff.data(), d_hoff, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(f, hipStreamSynchronize(st));
    f->st.head_bytes = head_bytes; f->st.down += head_bytes + (R + 1) * 8; f->st.t_heads = now() - t0;
    return 0;
}
