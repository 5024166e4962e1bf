// resident_file.h -- what a main sees of resident_file.hip: a BGZF file of VCF text that is sent up compressed, inflated into one
// device buffer (vgl_inflate_members_device) and left there; the device finds the lines and hands back their heads (rf_core.h) and,
// per line, where the sample columns lie in the buffer.  fetchgl_hip --resident 1 parses the columns where the inflater wrote them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "rf_core.h"
#include "rb_core.h"

struct RfFile;

// why the file is not resident (rf_load's second result)
enum RfWhy {
    RF_RESIDENT = 0,
    RF_NOT_BGZF,                       // not a clean series of BGZF members: zlib reads the file
    RF_MEMBER_HOST,                    // a member came back VGL_INFLATE_HOST: zlib reads the file
    RF_TOO_LARGE,                      // the inflated and the compressed bytes together exceed max_bytes
};

struct RfStats {
    int64_t members = 0, compressed_up = 0, total = 0, lines = 0, head_bytes = 0, down = 0;
    double t_upload = 0, t_inflate = 0, t_split = 0;
    int64_t records = 0, chain_launches = 0;           // a BCF file (rf_bcf_split)
    double t_chain = 0, t_heads = 0;
};

// Opens `device`; nullptr with the reason in err (no device, no memory for the handle).
RfFile* rf_create(int device, char* err, size_t err_len);
void rf_destroy(RfFile* f);
const char* rf_error(RfFile* f);
// the device's free memory less 1 GiB (0 when there is less): the default of max_bytes
int64_t rf_default_max_bytes(RfFile* f);
// The file goes up in pieces through page-locked staging, a piece copied while the next is read, and is inflated into one buffer.
// 0 with *why = RF_RESIDENT or the reason it is not; -1: a device error or a file that cannot be read (rf_error).
int rf_load(RfFile* f, const char* path, int64_t max_bytes, RfWhy* why);
int64_t rf_total(const RfFile* f);
const uint8_t* rf_device_text(const RfFile* f);                       // device memory: rf_total bytes
// n bytes from byte off of the resident text into host memory
int rf_fetch(RfFile* f, int64_t off, int64_t n, uint8_t* dst);
// The split: lines, heads and sample-column spans.  out.over: a line's ninth tab was not within head_most bytes.  more_lines: the
// file has more than INT32_MAX - 1024 lines, the most the offsets scan takes (out is then empty).
int rf_split(RfFile* f, int64_t head_most, rf::Split* out, bool* more_lines);
const RfStats* rf_stats(const RfFile* f);

// ---- a resident BCF file (rb_core.h): what rf_split is for text ------------------------------------------------------------------
struct RbSplit {
    int64_t records = 0;
    int why = rb::OK; int64_t ordinal = -1;            // the flag: why the file is handed back (rb::Why), and at which record (0-based)
    bool more_records = false;                         // more than INT32_MAX - 1024 records, the most the offsets scan takes
    std::vector<int64_t> rec_off;                      // [records] where every record begins in the file
    std::vector<int64_t> hoff;                         // [records + 1] where record i's head begins in `heads`
    std::vector<uint8_t> heads;                        // per record: the 8 length bytes, the shared block, every FORMAT field's key and descriptor
};
// The file's header: 9 bytes, then l_text more.  fits = false (hdr empty): not BCF2, or a header that does not fit the file.
int rf_bcf_header(RfFile* f, std::vector<uint8_t>* hdr, bool* fits);
// The records from byte `start` (behind the header), n_samples samples: the chain in launches of at most hops_most records, the head
// lengths, the heads.  0 with out->why / more_records set when the file is to be handed back; -1: a device error (rf_error).
int rf_bcf_split(RfFile* f, int64_t start, int64_t n_samples, int64_t hops_most, int64_t head_most, RbSplit* out);
