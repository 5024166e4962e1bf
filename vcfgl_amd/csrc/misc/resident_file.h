// resident_file.h -- what a main sees of resident_file.hip: a BGZF file of VCF text that is sent up compressed, inflated into one
// device buffer (vgl_inflate_members_device) and left there; the device finds the lines and hands back their heads (rf_core.h) and,
// per line, where the sample columns lie in the buffer.  fetchgl_hip --resident 1 parses the columns where the inflater wrote them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "rf_core.h"

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
