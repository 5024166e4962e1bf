// sal_dev.h -- what setal_main.cpp sees of setalfile.hip: a handle that holds two batches of records (slots 0 and 1) on one stream
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sal_core.h"

struct SalDev;

// what a retired batch gives back; the pointers are page-locked host memory of the slot, valid until the slot is submitted again
struct SalBatchOut {
    const int32_t* status;             // [n_recs] sal::ST_OK / ST_HOST / ST_RANGE
    const uint32_t* planes;            // the normalised planes, each record's at its Rec::plane_off (a record that is not ST_OK: unspecified)
    const int32_t* width;              // BCF: [n_recs] the bytes of a new PL value, 1 / 2 / 4 (htslib's narrowing over the record's values)
};

// n_samples, the most records, staged bytes and plane values of a batch, nullptr with the reason in err
SalDev* sal_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, int64_t max_vals, char* err, size_t err_len);
uint8_t* sal_dev_text(SalDev* d, int slot);                    // the slot's staging: max_text bytes, max_recs descriptors
sal::BRec* sal_dev_brecs(SalDev* d, int slot);
// the staging holds the records' GL / PL / GP vector blocks (k_sal_bcf_apply)
int sal_dev_submit(SalDev* d, int slot, int32_t n_recs, int64_t text_bytes, int64_t vals);
int sal_dev_wait(SalDev* d, int slot, SalBatchOut* out);
void sal_dev_quiesce(SalDev* d);                               // waits for whatever is in flight (before the process leaves on an error)
void sal_dev_destroy(SalDev* d);
const char* sal_dev_error(SalDev* d);
