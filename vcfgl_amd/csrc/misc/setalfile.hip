// setalfile.hip -- the kernel of setalleles_hip and its launch code (a translation unit of the program: the library gets no entry
// point).  A batch is the GL / PL / GP vector blocks of up to max_recs BCF records and one sal::BRec per record; the per-sample rules
// are sal_core.h.  k_sal_bcf_apply is described where it stands (sal_apply.hip.h; here its ANY = false form).  The new vectors, the
// status, the over words and the PL widths come back; the host splices the vectors between the copied fields.  (VCF text is worked on
// the host: setal_main.cpp.  --resident 1 is setalres.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/vcfgl_hip.h"
#include "sal_dev.h"
#include "batch_dev.hip.h"
#include "sal_apply.hip.h"

using salapply::NT;
using salapply::BArgs;

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
    hipLaunchKernelGGL(salapply::k_sal_bcf_apply<false>, dim3((unsigned)n_recs, sal::NF), dim3(NT), 0, st, B);
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
