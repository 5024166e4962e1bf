// setalres.hip -- setalleles_hip --resident 1: the kernels that assemble a batch's output records on the device, and the handle that
// runs a batch (a translation unit of the program: the library gets no entry point).  The per-record rules are salres_core.h.
//   k_sal_bcf_apply<true>  (sal_apply.hip.h) the relabelling kernel over the resident file: a vector block begins at any byte
//   k_salres_plan          a lane per record: the statuses of the relabelling folded into one (an `over` word makes ST_RANGE), the
//                          descriptor checked, the record's length with PL at the width the device chose; a record that is not
//                          ST_OK has length 0
//   k_offsets_scan         (wg_scan.hip.h) the lengths -> where every record begins in the batch's output
//   k_salres_write         a workgroup per record, its pieces in turn (salres::write_record): destination-aligned 16-byte stores
//                          for the body of a piece, the source realigned from aligned loads, heads and tails by bytes.  A record
//                          whose descriptor or planned length does not hold raises ST_HOST and writes nothing
//   k_salres_guards        the 64 bytes in front of and behind the slot's plane, output and member buffers, gathered behind the
//                          status words so that they come down with them
// No kernel reads outside the file, the batch's shared bytes or its planes, and none stores outside a record's [off[i], off[i + 1]).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/vcfgl_hip.h"
#include "salres_dev.h"
#include "batch_dev.hip.h"
#include "sal_apply.hip.h"
#include "wg_scan.hip.h"

namespace {

using salapply::NT;
using salres::GUARD;

constexpr uint8_t GUARD_BYTE = 0xA5;
constexpr int N_GUARDS = 6;              // planes, output, members: in front and behind

struct PArgs {
    const sal::BRec* recs; const salres::Desc* descs; int32_t n_recs, N;
    salres::Sources S;
    int32_t* status; const int32_t* over; const int32_t* width;
    int64_t* len;
};

__global__ void __launch_bounds__(NT) k_salres_plan(const PArgs A) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= A.n_recs) return;
    int st = A.status[i];
    if (st == sal::ST_OK && A.over[i]) st = sal::ST_RANGE;
    int64_t len = 0;
    if (st == sal::ST_OK) {
        const salres::Desc d = A.descs[i]; const sal::BRec r = A.recs[i];
        const int w = A.width[i];
        len = salres::check(d, r, A.N, w, A.S) ? salres::record_len(d, r, A.N, w) : -1;
        if (len < 0) { st = sal::ST_HOST; len = 0; }
    }
    A.status[i] = st; A.len[i] = len;
}

struct WArgs {
    const sal::BRec* recs; const salres::Desc* descs; int32_t n_recs, N;
    salres::Sources S;
    int32_t* status; const int32_t* width;
    const int64_t* off; uint8_t* out; int64_t out_cap;
};

__global__ void __launch_bounds__(NT) k_salres_write(const WArgs A) {
    const int rec = blockIdx.x;
    if (rec >= A.n_recs) return;
    const int64_t o0 = A.off[rec], o1 = A.off[rec + 1];               // (uniform over the workgroup, as everything below but the lane)
    bool ok = o0 >= 0 && o1 >= o0 && o1 <= A.out_cap;
    if (ok) {
        const salres::Desc d = A.descs[rec]; const sal::BRec r = A.recs[rec];
        ok = salres::write_record(A.out, o0, o1, d, r, A.N, A.width[rec], A.S, (int)threadIdx.x, NT);
    }
    if (!ok && threadIdx.x == 0) A.status[rec] = sal::ST_HOST;
}

struct GArgs { const uint8_t* at[N_GUARDS]; uint8_t* dst; };
__global__ void __launch_bounds__(GUARD) k_salres_guards(const GArgs A) {
    const int g = blockIdx.x;
    if (g < N_GUARDS) A.dst[g * GUARD + threadIdx.x] = A.at[g][threadIdx.x];
}

// behind the 3 n status words of a batch
struct Tail { int64_t total, members; uint8_t guards[N_GUARDS * GUARD]; };
size_t tail_at(size_t R) { return (3 * R * 4 + 7) & ~(size_t)7; }

// a device buffer with GUARD bytes in front and behind
struct Guarded {
    batchdev::DevMem<uint8_t> m; size_t n = 0;
    hipError_t alloc(size_t bytes) {
        n = (bytes + 15) & ~(size_t)15;
        const hipError_t e = m.alloc(n + 2 * GUARD);
        if (e != hipSuccess) return e;
        return hipMemset(m.p, GUARD_BYTE, n + 2 * GUARD);
    }
    uint8_t* body() const { return m.p + GUARD; }
    const uint8_t* front() const { return m.p; }
    const uint8_t* back() const { return m.p + GUARD + n; }
    static int64_t bytes_for(int64_t bytes) { return ((bytes + 15) & ~15ll) + 2 * GUARD; }
};

}  // namespace

struct SalRes : batchdev::BatchDev {
    SalResShape sh;
    int64_t mem_cap = 0, ws_bytes = 0;
    batchdev::Stream cp;                                               // the members (or the records) of a retired batch come down here
    batchdev::DevMem<uint8_t> d_ws;                                    // the compressor's workspace: one stream, one workspace
    struct Slot {
        batchdev::PinMem<sal::BRec> h_recs; batchdev::PinMem<salres::Desc> h_descs; batchdev::PinMem<uint8_t> h_shared, h_status, h_bytes;
        batchdev::DevMem<sal::BRec> d_recs; batchdev::DevMem<salres::Desc> d_descs; batchdev::DevMem<uint8_t> d_shared, d_status;
        batchdev::DevMem<uint32_t> d_work; batchdev::DevMem<int64_t> d_len, d_off;
        Guarded planes, out, mem;
        batchdev::Event ev[6], cp0, cp1;                               // timing: start, relabelled, planned, write begins, written, compressed; the copy down
        bool assembled = false;
    } slot[2];
};

int64_t salres_device_bytes(const SalResShape& s) {
    const int64_t R = s.max_recs, V = s.max_vals > 0 ? s.max_vals : 1;
    const int64_t mem = s.compress ? vgl_bgzf_bound(s.max_out) : 0, ws = s.compress ? vgl_bgzf_workspace_bytes(s.max_out) : 0;
    const int64_t a_slot = R * (int64_t)(sizeof(sal::BRec) + sizeof(salres::Desc)) + s.max_shared + (int64_t)tail_at((size_t)R) + (int64_t)sizeof(Tail) + V * 4 + (2 * R + 1) * 8 +
                           Guarded::bytes_for(V * 4) + Guarded::bytes_for(s.max_out) + Guarded::bytes_for(mem);
    return 2 * a_slot + ws;
}

const char* salres_error(SalRes* d) { return d->err; }

SalRes* salres_create(int device, const SalResShape& shape, char* err, size_t err_len) {
    if (shape.n_samples < 0 || shape.max_recs <= 0 || shape.max_vals < 0 || shape.max_shared < 0 || shape.max_out < 0) { snprintf(err, err_len, "bad batch shape"); return nullptr; }
    return batchdev::create<SalRes>(device, err, err_len, [&](SalRes* d) {
        d->sh = shape;
        const size_t R = (size_t)shape.max_recs, V = (size_t)(shape.max_vals > 0 ? shape.max_vals : 1);
        d->mem_cap = shape.compress ? vgl_bgzf_bound(shape.max_out) : 0;
        d->ws_bytes = shape.compress ? vgl_bgzf_workspace_bytes(shape.max_out) : 0;
        BATCH_HIP(d, hipStreamCreateWithFlags(&d->cp.h, hipStreamNonBlocking));
        BATCH_HIP(d, d->d_ws.alloc((size_t)(d->ws_bytes > 0 ? d->ws_bytes : 1)));
        const size_t st_bytes = tail_at(R) + sizeof(Tail);
        for (SalRes::Slot& s : d->slot) {
            bool ok = s.h_recs.alloc(d->device, R * sizeof(sal::BRec)); ok &= s.h_descs.alloc(d->device, R * sizeof(salres::Desc));
            ok &= s.h_shared.alloc(d->device, (size_t)shape.max_shared); ok &= s.h_status.alloc(d->device, st_bytes);
            ok &= s.h_bytes.alloc(d->device, (size_t)(shape.compress ? d->mem_cap : shape.max_out));
            if (!ok) return d->no_pinned();
            BATCH_HIP(d, s.d_recs.alloc(R * sizeof(sal::BRec))); BATCH_HIP(d, s.d_descs.alloc(R * sizeof(salres::Desc)));
            BATCH_HIP(d, s.d_shared.alloc((size_t)shape.max_shared + 16)); BATCH_HIP(d, s.d_status.alloc(st_bytes));
            BATCH_HIP(d, s.d_work.alloc(V * 4)); BATCH_HIP(d, s.d_len.alloc(R * 8)); BATCH_HIP(d, s.d_off.alloc((R + 1) * 8));
            BATCH_HIP(d, s.planes.alloc(V * 4)); BATCH_HIP(d, s.out.alloc((size_t)(shape.max_out > 0 ? shape.max_out : 1)));
            BATCH_HIP(d, s.mem.alloc((size_t)(d->mem_cap > 0 ? d->mem_cap : 1)));
            for (batchdev::Event& e : s.ev) BATCH_HIP(d, hipEventCreate(&e.h));
            BATCH_HIP(d, hipEventCreate(&s.cp0.h)); BATCH_HIP(d, hipEventCreate(&s.cp1.h));
        }
        BATCH_HIP(d, hipDeviceSynchronize());                              // (the guards are filled)
        return 0;
    });
}

sal::BRec* salres_brecs(SalRes* d, int slot) { return d->slot[slot & 1].h_recs; }
salres::Desc* salres_descs(SalRes* d, int slot) { return d->slot[slot & 1].h_descs; }
uint8_t* salres_shared(SalRes* d, int slot) { return d->slot[slot & 1].h_shared; }

int salres_submit(SalRes* d, int slot, int32_t n_recs, int64_t vals, int64_t shared_bytes, const uint8_t* file, int64_t file_total) {
    SalRes::Slot& s = d->slot[slot & 1];
    const SalResShape& sh = d->sh;
    if (d->begin_submit(slot, n_recs, n_recs >= 0 && n_recs <= sh.max_recs && vals >= 0 && vals <= (sh.max_vals > 0 ? sh.max_vals : 1) && shared_bytes >= 0 &&
                                          shared_bytes <= sh.max_shared && file && file_total >= 0) != 0) return -1;
    s.assembled = false;
    if (n_recs == 0) return 0;
    hipStream_t st = d->stream;
    const size_t R = (size_t)n_recs, t_at = tail_at(R);
    int32_t* const status = (int32_t*)s.d_status.p;
    Tail* const tail = (Tail*)(s.d_status.p + t_at);
    BATCH_HIP(d, hipMemcpyAsync(s.d_recs, s.h_recs, R * sizeof(sal::BRec), hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemcpyAsync(s.d_descs, s.h_descs, R * sizeof(salres::Desc), hipMemcpyHostToDevice, st));
    if (shared_bytes > 0) BATCH_HIP(d, hipMemcpyAsync(s.d_shared, s.h_shared, (size_t)shared_bytes, hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemsetAsync(s.d_status, 0, t_at + sizeof(Tail), st));
    BATCH_HIP(d, hipEventRecord(s.ev[0], st));
    // the vectors are relabelled where the inflater wrote them
    const salapply::BArgs B{file, file_total, s.d_recs, n_recs, sh.n_samples, (uint32_t*)s.planes.body(), s.d_work, vals, status, status + R, status + 2 * R};
    hipLaunchKernelGGL(salapply::k_sal_bcf_apply<true>, dim3((unsigned)n_recs, sal::NF), dim3(NT), 0, st, B);
    BATCH_HIP(d, hipGetLastError());
    BATCH_HIP(d, hipEventRecord(s.ev[1], st));
    const salres::Sources S{file, file_total, s.d_shared, shared_bytes, s.planes.body(), vals};
    const PArgs P{s.d_recs, s.d_descs, n_recs, sh.n_samples, S, status, status + R, status + 2 * R, s.d_len};
    hipLaunchKernelGGL(k_salres_plan, dim3((unsigned)((n_recs + NT - 1) / NT)), dim3(NT), 0, st, P);
    BATCH_HIP(d, hipGetLastError());
    hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(1), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)s.d_len, (int64_t*)s.d_off, n_recs);
    BATCH_HIP(d, hipGetLastError());
    BATCH_HIP(d, hipEventRecord(s.ev[2], st));
    // the batch's length and statuses decide what is enqueued next: the host waits for them here (the other slot's batch runs on)
    BATCH_HIP(d, hipMemcpyAsync(&tail->total, s.d_off + R, 8, hipMemcpyDeviceToDevice, st));
    BATCH_HIP(d, hipMemcpyAsync(s.h_status, s.d_status, t_at + 8, hipMemcpyDeviceToHost, st));
    BATCH_HIP(d, hipStreamSynchronize(st));
    const int32_t* h_st = (const int32_t*)s.h_status.p;
    const int64_t total = ((const Tail*)(s.h_status.p + t_at))->total;
    bool all_ok = true;
    for (size_t i = 0; i < R; i++) all_ok = all_ok && h_st[i] == sal::ST_OK;
    if (all_ok && (total < 0 || total > sh.max_out)) return d->refuse("a batch's assembled records are longer than the bound they were planned with");
    if (all_ok) {
        const WArgs W{s.d_recs, s.d_descs, n_recs, sh.n_samples, S, status, status + 2 * R, s.d_off, s.out.body(), sh.max_out};
        BATCH_HIP(d, hipEventRecord(s.ev[3], st));
        hipLaunchKernelGGL(k_salres_write, dim3((unsigned)n_recs), dim3(NT), 0, st, W);
        BATCH_HIP(d, hipGetLastError());
        BATCH_HIP(d, hipEventRecord(s.ev[4], st));
        if (sh.compress && total > 0 &&
            vgl_bgzf_compress_device(d->device, s.out.body(), total, s.mem.body(), d->mem_cap, &tail->members, d->d_ws, d->ws_bytes, (void*)st) != VGL_OK)
            return d->refuse(vgl_last_error());
        BATCH_HIP(d, hipEventRecord(s.ev[5], st));
        s.assembled = true;
    }
    const GArgs G{{s.planes.front(), s.planes.back(), s.out.front(), s.out.back(), s.mem.front(), s.mem.back()}, tail->guards};
    hipLaunchKernelGGL(k_salres_guards, dim3(N_GUARDS), dim3(GUARD), 0, st, G);
    BATCH_HIP(d, hipGetLastError());
    BATCH_HIP(d, hipMemcpyAsync(s.h_status, s.d_status, t_at + sizeof(Tail), hipMemcpyDeviceToHost, st));
    return d->end_submit(slot);
}

int salres_wait(SalRes* d, int slot, SalResOut* out) {
    SalRes::Slot& s = d->slot[slot & 1];
    *out = SalResOut();
    if (d->begin_wait(slot) != 0) return -1;
    const int32_t n = d->head[slot & 1].n_recs;
    out->status = (const int32_t*)s.h_status.p; out->guards_ok = true;
    if (n == 0) return 0;
    const Tail* tail = (const Tail*)(s.h_status.p + tail_at((size_t)n));
    for (int i = 0; i < N_GUARDS * GUARD; i++) if (tail->guards[i] != GUARD_BYTE) out->guards_ok = false;
    bool all_ok = s.assembled;
    for (int32_t i = 0; i < n; i++) all_ok = all_ok && out->status[i] == sal::ST_OK;      // (k_salres_write may have refused a record)
    out->handed_back = !all_ok;
    float ms = 0;
    BATCH_HIP(d, hipEventElapsedTime(&ms, s.ev[0], s.ev[1])); out->t_relabel = ms * 1e-3;
    if (!s.assembled) return 0;
    BATCH_HIP(d, hipEventElapsedTime(&ms, s.ev[1], s.ev[2])); out->t_assemble = ms * 1e-3;       // (the host's look at the statuses lies between ev[2] and ev[3])
    BATCH_HIP(d, hipEventElapsedTime(&ms, s.ev[3], s.ev[4])); out->t_write = ms * 1e-3; out->t_assemble += out->t_write;
    BATCH_HIP(d, hipEventElapsedTime(&ms, s.ev[4], s.ev[5])); out->t_compress = ms * 1e-3;
    if (!all_ok || !out->guards_ok) return 0;
    out->raw_n = tail->total;
    const int64_t m = d->sh.compress ? tail->members : tail->total;
    if (m < 0 || m > (d->sh.compress ? d->mem_cap : d->sh.max_out) || (d->sh.compress && tail->total > 0 && m == 0)) return d->refuse("a batch's member bytes are outside their bound");
    if (m > 0) {
        BATCH_HIP(d, hipEventRecord(s.cp0, d->cp));
        BATCH_HIP(d, hipMemcpyAsync(s.h_bytes, d->sh.compress ? s.mem.body() : s.out.body(), (size_t)m, hipMemcpyDeviceToHost, d->cp));
        BATCH_HIP(d, hipEventRecord(s.cp1, d->cp));
        BATCH_HIP(d, hipStreamSynchronize(d->cp));
        BATCH_HIP(d, hipEventElapsedTime(&ms, s.cp0, s.cp1)); out->t_down = ms * 1e-3;
    }
    out->bytes = s.h_bytes; out->n = m;
    return 0;
}

void salres_quiesce(SalRes* d) { if (d) { d->quiesce(); if (d->cp.h) (void)hipStreamSynchronize(d->cp); } }
void salres_destroy(SalRes* d) { salres_quiesce(d); batchdev::destroy(d); }
