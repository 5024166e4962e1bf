// gtdisc_dev.h -- what gtdisc_main.cpp sees of gtdisc.hip: a handle that holds two batches of records (slots 0 and 1) on one stream
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gtdisc_core.h"
#include "gtdbcf_core.h"

struct GtdDev;

// what a retired batch gives back; the pointers are page-locked host memory of the slot, valid until the slot is submitted again
struct GtdBatchOut {
    const int32_t* status;             // [n_recs] gtd::ST_OK / gtd::ST_HOST
    const int64_t* list_off;           // [n_recs + 1] offsets of the records' -doGQ 1 / 2 lines in list_text (a ST_HOST record: empty)
    const int64_t* site_off;           // [n_recs + 1] likewise for -perSite 1
    const uint8_t* list_text;
    const uint8_t* site_text;
};

// n_samples, the most records and text bytes of a batch, the listing (gtd::LIST_*) and -perSite.  nullptr with the reason in err.
// bcf 1 (--bcf-direct 1 with a BCF file in the pair): a batch also carries two gtd::BSide per record (truth, call), its bytes hold the
// typed vectors of the BCF sides beside the text of the others, k_gtd_bcf_decode fills the planes in k_gtd_parse's place, and the
// batches are timed by hipEvent pairs.  timed 1 (--resident 1): the batches are timed whichever kernel fills the planes
GtdDev* gtd_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, int list, int per_site, int bcf, int timed, char* err, size_t err_len);
gtd::BSide* gtd_dev_sides(GtdDev* d, int slot);                // bcf 1: the slot's 2 * max_recs side descriptors
void gtd_dev_times(GtdDev* d, double* stage_ms, double* decode_ms);   // bcf 1 or timed 1: the retired batches' device time (copies up to the last kernel), and the share of k_gtd_bcf_decode (bcf 1) or k_gtd_parse
uint8_t* gtd_dev_text(GtdDev* d, int slot);                    // the slot's staging: max_text bytes, max_recs descriptors
gtd::Rec* gtd_dev_recs(GtdDev* d, int slot);
int gtd_dev_submit(GtdDev* d, int slot, int32_t n_recs, int64_t text_bytes);
// --resident 1: a side whose file lies in device memory (resident_file.h) is read there -- t_file / c_file: the file's first byte and
// its byte count, and the side's offsets in gtd::Rec / gtd::BSide count from it; nullptr: the side is staged as for gtd_dev_submit.
// A batch stages the descriptors and the text_bytes of whichever side is not resident.  The file must outlive the batch.
int gtd_dev_submit_resident(GtdDev* d, int slot, int32_t n_recs, int64_t text_bytes, const uint8_t* t_file, int64_t t_bytes, const uint8_t* c_file, int64_t c_bytes);
int gtd_dev_wait(GtdDev* d, int slot, GtdBatchOut* out);
int gtd_dev_table(GtdDev* d, int64_t* table);                  // the cells and call-missing counts of every batch so far (vgl_disc_table_len(n_samples) elements)
void gtd_dev_quiesce(GtdDev* d);                               // waits for whatever is in flight (before the process leaves on an error)
void gtd_dev_destroy(GtdDev* d);
const char* gtd_dev_error(GtdDev* d);
