// setalfile.hip -- the kernel of setalleles_hip and its launch code (a translation unit of the program: the library gets no entry
// point).  A batch is the GL / PL / GP vector blocks of up to max_recs BCF records and one sal::BRec per record; the per-sample rules
// are sal_core.h.  k_sal_bcf_apply is described where it stands.  The new vectors, the status, the over words and the PL widths come
// back; the host splices the vectors between the copied fields.  (VCF text is worked on the host: setal_main.cpp.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/vcfgl_hip.h"
#include "sal_dev.h"
#include "batch_dev.hip.h"

namespace {

constexpr int NT = 256;                  // lanes per workgroup

struct BArgs {
    const uint8_t* in; int64_t in_bytes;
    const sal::BRec* recs; int32_t n_recs, N;
    uint32_t* planes; uint32_t* work; int64_t vals;
    int32_t* status; int32_t* over; int32_t* width;
};

// BCF.  grid: (records, 3 fields), a workgroup per record and field, its lanes on consecutive samples.  A lane reads its sample's old
// vector at its width (PL: int8 / 16 / 32 with the sentinels widened), gathers the new order out of a register pair, normalises and
// writes nG_new floats.  PL goes to the int32 workspace first; the workgroup reduces the record's minimum and maximum (missing and
// end-of-vector left out, as bcf_enc_vint does), takes the narrowest width that holds them and every lane narrows its own samples
// into the plane.  A PL sample whose cast would overflow raises the record's `over` word.
__global__ void __launch_bounds__(NT) k_sal_bcf_apply(const BArgs A) {
    __shared__ int32_t s_mn[NT / 64], s_mx[NT / 64];
    const int rec = blockIdx.x, f = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rec >= A.n_recs) return;
    const sal::BRec r = A.recs[rec];
    const int nv = f == 0 ? r.nv[0] : f == 1 ? r.nv[1] : r.nv[2];
    const int ty = f == 0 ? r.ty[0] : f == 1 ? r.ty[1] : r.ty[2];
    const int64_t in_off = f == 0 ? r.in_off[0] : f == 1 ? r.in_off[1] : r.in_off[2];
    if (nv <= 0) return;                                               // (uniform over the workgroup)
    const int64_t N = A.N;
    const int w_in = sal::type_width(ty), nG = r.n_new_g;
    const bool fits = sal::brec_sane(r) && in_off >= 0 && (in_off & 3) == 0 && in_off + N * nv * w_in <= A.in_bytes &&
                      r.plane_off >= 0 && r.plane_off + sal::b_plane_vals(r, N) <= A.vals;
    if (!fits) {                                                       // (the host sends no such record; never read or write outside)
        if (t == 0) A.status[rec] = sal::ST_HOST;
        return;
    }
    const uint8_t* __restrict__ in = A.in + in_off;
    const int64_t base = r.plane_off + (int64_t)sal::b_slot(r, f) * nG * N;
    uint32_t v[sal::MAX_G];
    if (f != sal::F_PL) {
        for (int64_t s = t; s < N; s += NT) {
            sal::bcf_sample(in + s * nv * w_in, ty, nv, r.n2o, nG, f, v);
#pragma unroll
            for (int h = 0; h < sal::MAX_G; ++h) if (h < nG) A.planes[base + s * nG + h] = v[h];
        }
        return;
    }
    int32_t mn = INT32_MAX, mx = INT32_MIN + 1;
    int over = 0;
    for (int64_t s = t; s < N; s += NT) {
        if (sal::bcf_sample(in + s * nv * w_in, ty, nv, r.n2o, nG, f, v)) over = 1;
#pragma unroll
        for (int h = 0; h < sal::MAX_G; ++h)
            if (h < nG) {
                A.work[base + s * nG + h] = v[h];
                const int32_t x = (int32_t)v[h];
                if (v[h] != sal::I_MISSING && v[h] != sal::I_END) { if (x < mn) mn = x; if (x > mx) mx = x; }
            }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const int32_t a = __shfl_down(mn, d, 64), b = __shfl_down(mx, d, 64); if (a < mn) mn = a; if (b > mx) mx = b; }
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    over = __syncthreads_or(over);
    for (int k = 0; k < NT / 64; k++) { if (s_mn[k] < mn) mn = s_mn[k]; if (s_mx[k] > mx) mx = s_mx[k]; }
    const int w = sal::int_width(mn, mx);                              // (every lane now holds the record's minimum and maximum)
    if (t == 0) { A.width[rec] = w; if (over) A.over[rec] = 1; }
    if (over) return;
    uint8_t* out = reinterpret_cast<uint8_t*>(A.planes + base);
    for (int64_t s = t; s < N; s += NT)
#pragma unroll
        for (int h = 0; h < sal::MAX_G; ++h)
            if (h < nG) sal::store_narrow(out, w, s * nG + h, A.work[base + s * nG + h]);
}

}  // namespace

// ---- the handle (batch_dev.hip.h) ------------------------------------------------------------------------------------------------
struct SalDev : batchdev::BatchDev {
    int32_t N = 0, max_recs = 0; int64_t max_text = 0, max_vals = 0;
    struct Slot {
        batchdev::PinMem<uint8_t> h_text; batchdev::PinMem<sal::BRec> h_recs;
        batchdev::PinMem<int32_t> h_status; batchdev::PinMem<uint32_t> h_planes;      // h_status: n status words, n over words, n PL widths
        batchdev::DevMem<uint8_t> d_text; batchdev::DevMem<sal::BRec> d_recs;
        batchdev::DevMem<uint32_t> d_planes, d_work; batchdev::DevMem<int32_t> d_status;
    } slot[2];
};

const char* sal_dev_error(SalDev* d) { return d->err; }

SalDev* sal_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, int64_t max_vals, char* err, size_t err_len) {
    if (n_samples < 0 || max_recs <= 0 || max_text < 0 || max_vals < 0) { snprintf(err, err_len, "bad batch shape"); return nullptr; }
    return batchdev::create<SalDev>(device, err, err_len, [&](SalDev* d) {
        d->N = n_samples; d->max_recs = max_recs; d->max_text = max_text; d->max_vals = max_vals;
        const size_t R = (size_t)d->max_recs, V = (size_t)d->max_vals;
        for (SalDev::Slot& s : d->slot) {
            bool ok = s.h_text.alloc(d->device, (size_t)d->max_text); ok &= s.h_recs.alloc(d->device, R * sizeof(sal::BRec));
            ok &= s.h_status.alloc(d->device, 3 * R * 4); ok &= s.h_planes.alloc(d->device, V * 4);
            if (!ok) return d->no_pinned();
            BATCH_HIP(d, s.d_text.alloc((size_t)d->max_text + 16));
            BATCH_HIP(d, s.d_recs.alloc(R * sizeof(sal::BRec)));
            BATCH_HIP(d, s.d_planes.alloc((V ? V : 1) * 4));
            BATCH_HIP(d, s.d_work.alloc((V ? V : 1) * 4));
            BATCH_HIP(d, s.d_status.alloc(3 * R * 4));
        }
        return 0;
    });
}

uint8_t* sal_dev_text(SalDev* d, int slot) { return d->slot[slot & 1].h_text; }
sal::BRec* sal_dev_brecs(SalDev* d, int slot) { return d->slot[slot & 1].h_recs; }

int sal_dev_submit(SalDev* d, int slot, int32_t n_recs, int64_t text_bytes, int64_t vals) {
    SalDev::Slot& s = d->slot[slot & 1];
    if (d->begin_submit(slot, n_recs, n_recs >= 0 && n_recs <= d->max_recs && text_bytes >= 0 && text_bytes <= d->max_text && vals >= 0 && vals <= d->max_vals) != 0) return -1;
    if (n_recs == 0) return 0;
    hipStream_t st = d->stream;
    const size_t R = (size_t)n_recs;
    if (text_bytes > 0) BATCH_HIP(d, hipMemcpyAsync(s.d_text, s.h_text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemcpyAsync(s.d_recs, s.h_recs, R * sizeof(sal::BRec), hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemsetAsync(s.d_status, 0, 3 * R * 4, st));
    const BArgs B{s.d_text, text_bytes, s.d_recs, n_recs, d->N, s.d_planes, s.d_work, vals, s.d_status, s.d_status.p + R, s.d_status.p + 2 * R};
    hipLaunchKernelGGL(k_sal_bcf_apply, dim3((unsigned)n_recs, sal::NF), dim3(NT), 0, st, B);
    BATCH_HIP(d, hipGetLastError());
    BATCH_HIP(d, hipMemcpyAsync(s.h_status, s.d_status, 3 * R * 4, hipMemcpyDeviceToHost, st));
    if (vals > 0) BATCH_HIP(d, hipMemcpyAsync(s.h_planes, s.d_planes, (size_t)vals * 4, hipMemcpyDeviceToHost, st));
    return d->end_submit(slot);
}

int sal_dev_wait(SalDev* d, int slot, SalBatchOut* out) {
    SalDev::Slot& s = d->slot[slot & 1];
    if (d->begin_wait(slot) != 0) return -1;
    const int32_t n = d->head[slot & 1].n_recs;
    for (int32_t i = 0; i < n; i++)                                    // a sample whose PL cast would overflow: the record is the host's
        if (s.h_status[i] == sal::ST_OK && s.h_status[n + i]) s.h_status[i] = sal::ST_RANGE;
    out->status = s.h_status; out->planes = s.h_planes; out->width = s.h_status.p + 2 * (size_t)n;
    return 0;
}

void sal_dev_quiesce(SalDev* d) { if (d) d->quiesce(); }
void sal_dev_destroy(SalDev* d) { batchdev::destroy(d); }
