// fgl_dev.h -- what fetchgl_main.cpp sees of fetchgl.hip: a handle that holds two batches of records (slots 0 and 1) on one stream
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fgl_core.h"

struct FglDev;

// what a retired batch gives back; the pointers are page-locked host memory of the slot, valid until the slot is submitted again
struct FglBatchOut {
    const int32_t* status;             // [n_recs] fgl::ST_OK / ST_HOST / ST_RANGE
    const int64_t* off;                // [n_recs + 1] offsets of the records' CSV lines in csv (a record that is not ST_OK: empty)
    const uint8_t* csv;
};

// n_samples, the most records and staging bytes of a batch.  nullptr with the reason in err
FglDev* fgl_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, char* err, size_t err_len);
uint8_t* fgl_dev_text(FglDev* d, int slot);                    // the slot's staging: max_text bytes, max_recs descriptors
fgl::Rec* fgl_dev_recs(FglDev* d, int slot);
// bcf 0: the staging holds sample-column text (k_fgl_parse); 1: GL vector blocks of floats (k_fgl_pick)
int fgl_dev_submit(FglDev* d, int slot, int32_t n_recs, int64_t text_bytes, int bcf);
// the records' sample columns lie in device memory of the handle's device already (resident_file.h): the descriptors' offsets are into
// d_text [text_bytes], k_fgl_parse reads them there, and nothing of the slot's staging is copied.  bcf 1: the file is BCF, a descriptor's
// offset is where the record's GL vectors begin (any byte), and k_fgl_pick<true> reads them there
int fgl_dev_submit_resident(FglDev* d, int slot, int32_t n_recs, const uint8_t* d_text, int64_t text_bytes, int bcf);
int fgl_dev_wait(FglDev* d, int slot, FglBatchOut* out);
void fgl_dev_quiesce(FglDev* d);                               // waits for whatever is in flight (before the process leaves on an error)
void fgl_dev_destroy(FglDev* d);
const char* fgl_dev_error(FglDev* d);
int64_t fgl_dev_line_bound(int32_t n_samples);                 // the most bytes one CSV line takes
