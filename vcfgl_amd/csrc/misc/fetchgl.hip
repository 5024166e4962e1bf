// fetchgl.hip -- the kernels of fetchgl_hip and their launch code (a translation unit of the program: the library gets no entry point).
// A batch is the sample-column text of up to max_recs records that get a CSV line (or, for BCF, their GL vector blocks) and one
// fgl::Rec per record; the per-column rules are fgl_core.h.
//   k_fgl_parse   one workgroup of 256 lanes per record.  The region is walked as k_gtd_parse walks a line (column_walk.hip.h): chunks of
//                 256 x 16 bytes on 16-byte address boundaries, a lane whose 16 bytes lie inside the region loads them at once, the lanes at
//                 the two ends read their bytes one by one -- no byte outside the region is read.  A scan of the tab counts numbers the columns; the
//                 lane that owns the tab before column s reads that column (fgl::sample_value, bounded by the region's end): it skips k
//                 colons, counts the field's values, finds value g and parses it into float bits (END for a count <= g), stored in the
//                 [record][sample] uint32 plane.  The workgroup then reduces the largest count to n_gls and lane 0 stores the status:
//                 OK, HOST (a picked token outside the device grammar) or RANGE (g >= n_gls, or a column count other than N).  No atomics.
//   k_fgl_pick    BCF: a workgroup per record, a lane per sample: value g of the sample's vector into the same plane (<false>: from the
//                 staging, on 4-byte addresses; <true>: from a resident file, at any byte)
//   k_fgl_plan    a workgroup per record: the byte count of its line, "POS," included (0 for a record that is not OK)
//   k_offsets_scan (wg_scan.hip.h) one workgroup: the exclusive prefix sums of the counts over the batch's records
//   k_fgl_write   a workgroup per record, a lane per value: the values' lengths are scanned across the workgroup, chunk by chunk, and
//                 every lane formats its value at its offset, never past the text's capacity
// The plane never leaves the device: the status, the offsets and the CSV text come back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/vcfgl_hip.h"
#include "fgl_dev.h"
#include "rb_core.h"
#include "column_walk.hip.h"
#include "batch_dev.hip.h"

namespace {

using colwalk::NT;                       // lanes per workgroup of the parser, the planner and the writer (column_walk.hip.h)
using colwalk::LB;                       // bytes per lane and chunk
using colwalk::scan_columns;

struct ParseArgs {
    const uint8_t* text; int64_t text_bytes;
    const fgl::Rec* recs; int32_t n_recs, N;
    uint32_t* plane; int32_t* status;
};

__global__ void __launch_bounds__(NT) k_fgl_parse(const ParseArgs A) {
    __shared__ int32_t s_tot[2][NT / 64];
    __shared__ int32_t s_bad[NT / 64];
    __shared__ int32_t s_max[NT / 64];
    const int rec = blockIdx.x;
    if (rec >= A.n_recs) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const fgl::Rec r = A.recs[rec];
    const int32_t N = A.N;
    const int64_t lb = r.off, le = r.off + (int64_t)r.len;
    if (r.off < 0 || r.len < 0 || le > A.text_bytes || r.k < 0 || r.g < 0) {   // (the host sends no such record; never read outside the text)
        if (t == 0) A.status[rec] = fgl::ST_HOST;
        return;
    }
    const uint8_t* __restrict__ text = A.text;
    uint32_t* __restrict__ plane = A.plane + (size_t)rec * (size_t)N;
    int bad = 0; int32_t most = 0;
    const int32_t cols = scan_columns(text, lb, le, s_tot, [&](const int32_t col, const int64_t q) {
        if (col >= N) return;
        uint32_t b; int32_t c;
        if (!fgl::sample_value(text, q, le, r.k, r.g, b, c)) { bad = 1; return; }
        plane[col] = b;
        if (c > most) most = c;
    });
    bad = __any(bad) ? 1 : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const int32_t y = __shfl_down(most, d, 64); if (y > most) most = y; }
    if (lane == 0) { s_bad[wave] = bad; s_max[wave] = most; }
    __syncthreads();
    if (t == 0) {
        int B = 0; int32_t n_gls = 0;
        for (int k = 0; k < NT / 64; k++) { B |= s_bad[k]; if (s_max[k] > n_gls) n_gls = s_max[k]; }
        A.status[rec] = fgl::record_status(B != 0, cols, N, n_gls, r.g);
    }
}

// BCF: text holds the records' GL vector blocks, N vectors of r.len floats from byte r.off.  ANY = false: the slot's staging, where
// r.off is a multiple of 4.  ANY = true: a resident file (resident_file.h), where a block begins at any byte: a float is read from
// the aligned words around it (rb::load_u32_any), never from a word that reaches past text_bytes
template <bool ANY>
__global__ void __launch_bounds__(NT) k_fgl_pick(const ParseArgs A) {
    const int rec = blockIdx.x, t = threadIdx.x;
    if (rec >= A.n_recs) return;
    const fgl::Rec r = A.recs[rec];
    const int64_t n = r.len, N = A.N;
    const bool fits = r.off >= 0 && (ANY || (r.off & 3) == 0) && n >= 1 && r.off + N * n * 4 <= A.text_bytes;
    if (!fits || r.g < 0 || r.g >= n) {
        if (t == 0) A.status[rec] = fits ? fgl::ST_RANGE : fgl::ST_HOST;
        return;
    }
    uint32_t* __restrict__ plane = A.plane + (size_t)rec * (size_t)N;
    if (ANY) {
        const uint8_t* __restrict__ text = A.text;
        for (int64_t s = t; s < N; s += NT) plane[s] = rb::load_u32_any(text, r.off + (s * n + r.g) * 4, A.text_bytes);
    } else {
        const uint32_t* __restrict__ v = reinterpret_cast<const uint32_t*>(A.text + r.off);
        for (int64_t s = t; s < N; s += NT) plane[s] = v[s * n + r.g];
    }
    if (t == 0) A.status[rec] = fgl::ST_OK;
}

struct LineArgs {
    int32_t N, n_recs;
    const fgl::Rec* recs; const uint32_t* plane; const int32_t* status;
    int64_t* len;                        // [n_recs]
    int64_t* off;                        // [n_recs + 1]
    uint8_t* csv; int64_t cap;
};

__global__ void __launch_bounds__(NT) k_fgl_plan(const LineArgs A) {
    __shared__ unsigned long long s_sum[NT / 64];
    const int rec = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rec >= A.n_recs) return;
    unsigned long long n = 0;
    if (A.status[rec] == fgl::ST_OK) {
        const uint32_t* __restrict__ row = A.plane + (size_t)rec * (size_t)A.N;
        for (int32_t s = t; s < A.N; s += NT) n += fgl::value_len(row[s]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
    if (lane == 0) s_sum[wave] = n;
    __syncthreads();
    if (t == 0) {
        unsigned long long x = 0;
        for (int k = 0; k < NT / 64; k++) x += s_sum[k];
        if (A.status[rec] == fgl::ST_OK) x += fgl::pos_len(A.recs[rec].pos);
        A.len[rec] = (int64_t)x;
    }
}

__global__ void __launch_bounds__(NT) k_fgl_write(const LineArgs A) {
    __shared__ uint32_t s_tot[2][NT / 64];
    const int rec = blockIdx.x, t = threadIdx.x;
    if (rec >= A.n_recs || A.status[rec] != fgl::ST_OK) return;        // (uniform over the workgroup)
    const uint32_t* __restrict__ row = A.plane + (size_t)rec * (size_t)A.N;
    const int64_t pos = A.recs[rec].pos;
    int64_t at0 = A.off[rec];
    if (t == 0 && at0 >= 0 && at0 < A.cap) {
        const int64_t room = A.cap - at0;
        vgl_fetchgl::Emit<true> e{A.csv + at0, 0u, (uint32_t)(room < fgl::MAX_POS_LEN + 1 ? room : fgl::MAX_POS_LEN + 1)};
        fgl::put_pos(e, (uint64_t)pos);
    }
    at0 += fgl::pos_len(pos);
    const int n_chunks = (A.N + NT - 1) / NT;
    for (int c = 0; c < n_chunks; c++) {
        const int32_t s = c * NT + t;
        uint32_t bits = 0, l = 0;
        if (s < A.N) { bits = row[s]; l = fgl::value_len(bits); }
        const wgscan::Sums<uint32_t> sc = wgscan::step<NT>(l, s_tot, c & 1);
        if (l) {
            const int64_t at = at0 + sc.before + sc.inc - l;
            if (at >= 0 && at < A.cap) {
                const int64_t room = A.cap - at;
                vgl_fetchgl::Emit<true> e{A.csv + at, 0u, (uint32_t)(room < fgl::VALUE_BOUND ? room : fgl::VALUE_BOUND)};
                fgl::put_value(e, bits, s == A.N - 1);
            }
        }
        at0 += sc.total;
    }
}

}  // namespace

// ---- the handle (batch_dev.hip.h) ------------------------------------------------------------------------------------------------
struct FglDev : batchdev::BatchDev {
    int32_t N = 0, max_recs = 0; int64_t max_text = 0, cap = 0;
    struct Slot {
        batchdev::PinMem<uint8_t> h_text; batchdev::PinMem<fgl::Rec> h_recs;
        batchdev::PinMem<int32_t> h_status; batchdev::PinMem<int64_t> h_off; batchdev::PinMem<uint8_t> h_csv;
        batchdev::DevMem<uint8_t> d_text; batchdev::DevMem<fgl::Rec> d_recs;
        batchdev::DevMem<uint32_t> d_plane; batchdev::DevMem<int32_t> d_status; batchdev::DevMem<int64_t> d_len, d_off; batchdev::DevMem<uint8_t> d_csv;
    } slot[2];
};

const char* fgl_dev_error(FglDev* d) { return d->err; }
int64_t fgl_dev_line_bound(int32_t n_samples) { return (int64_t)fgl::MAX_POS_LEN + 1 + (int64_t)n_samples * fgl::VALUE_BOUND; }

FglDev* fgl_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, char* err, size_t err_len) {
    if (n_samples <= 0 || max_recs <= 0 || max_text < 0) { snprintf(err, err_len, "bad batch shape"); return nullptr; }
    return batchdev::create<FglDev>(device, err, err_len, [&](FglDev* d) {
        d->N = n_samples; d->max_recs = max_recs; d->max_text = max_text;
        d->cap = (int64_t)max_recs * fgl_dev_line_bound(n_samples);
        const size_t R = (size_t)d->max_recs, N = (size_t)d->N;
        for (FglDev::Slot& s : d->slot) {
            bool ok = s.h_text.alloc(d->device, (size_t)d->max_text); ok &= s.h_recs.alloc(d->device, R * sizeof(fgl::Rec));
            ok &= s.h_status.alloc(d->device, R * 4); ok &= s.h_off.alloc(d->device, (R + 1) * 8); ok &= s.h_csv.alloc(d->device, (size_t)d->cap);
            if (!ok) return d->no_pinned();
            BATCH_HIP(d, s.d_text.alloc((size_t)d->max_text + LB));
            BATCH_HIP(d, s.d_recs.alloc(R * sizeof(fgl::Rec)));
            BATCH_HIP(d, s.d_plane.alloc(R * N * 4));
            BATCH_HIP(d, s.d_status.alloc(R * 4));
            BATCH_HIP(d, s.d_len.alloc(R * 8));
            BATCH_HIP(d, s.d_off.alloc((R + 1) * 8));
            BATCH_HIP(d, s.d_csv.alloc((size_t)d->cap + 1));
        }
        return 0;
    });
}

uint8_t* fgl_dev_text(FglDev* d, int slot) { return d->slot[slot & 1].h_text; }
fgl::Rec* fgl_dev_recs(FglDev* d, int slot) { return d->slot[slot & 1].h_recs; }

// the copies of a batch up and its launch sequence; text [text_bytes] is what the parser reads (the slot's staging, or a resident file)
static int submit_on(FglDev* d, int slot, int32_t n_recs, const uint8_t* staged, const uint8_t* text, int64_t text_bytes, int bcf) {
    FglDev::Slot& s = d->slot[slot & 1];
    if (n_recs == 0) return 0;
    hipStream_t st = d->stream;
    const size_t R = (size_t)n_recs;
    if (staged && text_bytes > 0) BATCH_HIP(d, hipMemcpyAsync(s.d_text, staged, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemcpyAsync(s.d_recs, s.h_recs, R * sizeof(fgl::Rec), hipMemcpyHostToDevice, st));
    const ParseArgs P{text, text_bytes, s.d_recs, n_recs, d->N, s.d_plane, s.d_status};
    if (bcf && !staged) hipLaunchKernelGGL(k_fgl_pick<true>, dim3((unsigned)n_recs), dim3(NT), 0, st, P);
    else if (bcf) hipLaunchKernelGGL(k_fgl_pick<false>, dim3((unsigned)n_recs), dim3(NT), 0, st, P);
    else hipLaunchKernelGGL(k_fgl_parse, dim3((unsigned)n_recs), dim3(NT), 0, st, P);
    BATCH_HIP(d, hipGetLastError());
    const LineArgs L{d->N, n_recs, s.d_recs, s.d_plane, s.d_status, s.d_len, s.d_off, s.d_csv, d->cap};
    hipLaunchKernelGGL(k_fgl_plan, dim3((unsigned)n_recs), dim3(NT), 0, st, L);
    BATCH_HIP(d, hipGetLastError());
    hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(1), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)s.d_len, (int64_t*)s.d_off, n_recs);
    BATCH_HIP(d, hipGetLastError());
    hipLaunchKernelGGL(k_fgl_write, dim3((unsigned)n_recs), dim3(NT), 0, st, L);
    BATCH_HIP(d, hipGetLastError());
    BATCH_HIP(d, hipMemcpyAsync(s.h_off, s.d_off, (R + 1) * 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(d, hipMemcpyAsync(s.h_status, s.d_status, R * 4, hipMemcpyDeviceToHost, st));
    return d->end_submit(slot);
}

int fgl_dev_submit(FglDev* d, int slot, int32_t n_recs, int64_t text_bytes, int bcf) {
    FglDev::Slot& s = d->slot[slot & 1];
    if (d->begin_submit(slot, n_recs, n_recs >= 0 && n_recs <= d->max_recs && text_bytes >= 0 && text_bytes <= d->max_text) != 0) return -1;
    return submit_on(d, slot, n_recs, s.h_text, s.d_text, text_bytes, bcf);
}

int fgl_dev_submit_resident(FglDev* d, int slot, int32_t n_recs, const uint8_t* d_text, int64_t text_bytes, int bcf) {
    if (d->begin_submit(slot, n_recs, n_recs >= 0 && n_recs <= d->max_recs && d_text && text_bytes >= 0) != 0) return -1;
    return submit_on(d, slot, n_recs, nullptr, d_text, text_bytes, bcf);
}

int fgl_dev_wait(FglDev* d, int slot, FglBatchOut* out) {
    FglDev::Slot& s = d->slot[slot & 1];
    if (d->begin_wait(slot) != 0) return -1;
    const size_t R = (size_t)d->head[slot & 1].n_recs;
    if (R == 0) s.h_off[0] = 0;
    const int64_t n_csv = s.h_off[R];
    if (n_csv < 0 || n_csv > d->cap) return d->refuse("a batch's CSV text is longer than its bound");
    if (n_csv > 0) {
        BATCH_HIP(d, hipMemcpyAsync(s.h_csv, s.d_csv, (size_t)n_csv, hipMemcpyDeviceToHost, d->stream));
        BATCH_HIP(d, hipStreamSynchronize(d->stream));
    }
    out->status = s.h_status; out->off = s.h_off; out->csv = s.h_csv;
    return 0;
}

void fgl_dev_quiesce(FglDev* d) { if (d) d->quiesce(); }
void fgl_dev_destroy(FglDev* d) { batchdev::destroy(d); }
