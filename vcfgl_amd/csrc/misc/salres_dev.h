// salres_dev.h -- what setal_main.cpp sees of setalres.hip (--resident 1): a handle that holds two batches of records (slots 0 and 1)
// on one stream.  A batch is one sal::BRec and one salres::Desc per record and the records' new shared blocks; the file itself is
// resident (resident_file.h).  The device relabels the vectors where the inflater wrote them, assembles the batch's records
// (salres_core.h) and, for -O b, compresses them: BGZF members come back, or for -O u the records as they are.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "salres_core.h"

struct SalRes;

struct SalResShape {
    int32_t n_samples = 0, max_recs = 1;
    int64_t max_vals = 1;              // plane words of a batch
    int64_t max_shared = 1;            // bytes of a batch's new shared blocks
    int64_t max_out = 1;               // bytes of a batch's assembled records (PL taken at 4 bytes: an upper bound)
    int compress = 0;                  // 1: -O b
};

// what a retired batch gives back; the pointers are page-locked host memory of the slot, valid until the slot is submitted again
struct SalResOut {
    const int32_t* status;             // [n_recs] sal::ST_OK / ST_HOST / ST_RANGE
    bool handed_back;                  // a record is not ST_OK: nothing was assembled, the batch is the host's
    bool guards_ok;                    // the 64 bytes in front of and behind the slot's plane, output and member buffers are as they were filled
    const uint8_t* bytes; int64_t n;   // the BGZF members (compress) or the assembled records
    int64_t raw_n;                     // the assembled records' bytes
    double t_relabel, t_assemble, t_write, t_compress, t_down;      // hipEvent pairs, seconds; t_write: k_salres_write alone, a part of t_assemble
};

// device memory both slots take beside the file, by the arithmetic salres_create allocates with
int64_t salres_device_bytes(const SalResShape& s);
SalRes* salres_create(int device, const SalResShape& s, char* err, size_t err_len);
sal::BRec* salres_brecs(SalRes* d, int slot);                  // the slot's staging: max_recs descriptors of either kind, max_shared bytes
salres::Desc* salres_descs(SalRes* d, int slot);
uint8_t* salres_shared(SalRes* d, int slot);
// file: rf_device_text / rf_total of the resident file.  Relabels, plans, waits for the batch's length and statuses, and -- when every
// record is ST_OK -- enqueues assembly, compression and the small copies down before it returns.
int salres_submit(SalRes* d, int slot, int32_t n_recs, int64_t vals, int64_t shared_bytes, const uint8_t* file, int64_t file_total);
int salres_wait(SalRes* d, int slot, SalResOut* out);
void salres_quiesce(SalRes* d);
void salres_destroy(SalRes* d);
const char* salres_error(SalRes* d);
