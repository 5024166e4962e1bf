// salres_core.h -- the rules by which setalleles_hip --resident 1 assembles the records of its output on the device (setalres.hip), as
// code that compiles for the host and for the device: the kernels k_salres_plan and k_salres_write, the program's piece tables
// (table_begin, table_field) and a host program under the sanitizers (tests/salres_core_main.cpp) all run these routines.
//
// A record of the output is its two lengths, the new shared block the host built, and its FORMAT fields in file order:
//   untouched   a field that is not the record's GL, PL or GP is its bytes, copied from the resident file.  Untouched fields that
//               follow each other are one copy run, so a record has at most MAX_RUNS = 4 runs around at most MAX_TOUCHED = 3 fields
//   touched     the key's bytes from the file, the descriptor put_typed_len(n_new_g, type) -- type 5 for GL and GP, 1 / 2 / 3 for
//               PL by the record's width (1 / 2 / 4 bytes: k_sal_bcf_apply's width[rec]) -- and the field's plane, N n_new_g values
//               of that width, where k_sal_bcf_apply left it (sal::BRec::plane_off, sal::b_slot)
// Desc is the fixed-size piece table of a record; pieces() names the pieces in output order, and both the planned length and the
// writer go through it.  check() is what the device asks of a descriptor before it trusts it: every piece inside its source.
//   copy_run    n bytes from byte s of a source [0, s_total) to dst + d, by `n_lanes` lanes of which the caller is `lane`: the bytes up
//               to the first 16-byte address of the destination and the bytes behind the last one singly, the body as aligned 16-byte
//               stores.  A body piece's source comes from load16_any: one aligned 16-byte load, or the two aligned pieces around it
//               put together; where the second would reach outside [0, s_total) its bytes are read one by one.
// No routine reads outside the source it is given, and write_record stores to [o0, o1) of the output alone.
#ifndef SALRES_CORE_H
#define SALRES_CORE_H
#include <stdint.h>
#include <string.h>

#include "sal_core.h"

namespace salres {

enum { MAX_TOUCHED = 3, MAX_RUNS = 4, GUARD = 64, KEY_MOST = 64 };

struct Desc {
    int64_t shared_off;                // the record's new shared block in the batch's shared bytes
    int64_t run_off[MAX_RUNS];         // run k: the untouched fields in front of touched field k (k = n_touched: behind the last), in the file
    int64_t run_len[MAX_RUNS];
    int64_t key_off[MAX_TOUCHED];      // touched field k: its key in the file
    int32_t key_len[MAX_TOUCHED];
    int32_t shared_len;
    int8_t f[MAX_TOUCHED];             // touched field k is the record's GL, PL or GP (sal::F_*)
    int8_t n_touched;
    int32_t pad;
};

// where the pieces of a batch come from
struct Sources {
    const uint8_t* file; int64_t file_total;          // the resident file
    const uint8_t* shared; int64_t shared_total;      // the batch's new shared blocks
    const uint8_t* planes; int64_t plane_vals;        // the batch's planes, 32-bit words
};

// The piece table from a record's fields in file order: table_begin with where the first field lies (a record without fields: where
// the record ends), then table_field for every field -- [at, end) in the file, its key up to key_end, f = sal::F_* for the record's
// GL, PL or GP and -1 for an untouched field, which lengthens the run it lies in.  False: a fourth touched field.
VGL_HD void table_begin(Desc& d, const int64_t first_at) { memset(&d, 0, sizeof d); d.run_off[0] = first_at; }
VGL_HD bool table_field(Desc& d, const int64_t at, const int64_t key_end, const int64_t end, const int f) {
    const int k = d.n_touched;
    if (f < 0) { d.run_len[k] += end - at; return true; }
    if (k >= MAX_TOUCHED) return false;
    d.key_off[k] = at; d.key_len[k] = (int32_t)(key_end - at); d.f[k] = (int8_t)f;
    d.n_touched = (int8_t)(k + 1);
    d.run_off[k + 1] = end;
    return true;
}

VGL_HD int pl_type(const int width) { return width == 1 ? 1 : width == 2 ? 2 : 3; }
// htslib's bcf_enc_size for a count of at most 127: the descriptor's bytes into o, their number back
VGL_HD int put_typed_len(uint8_t* o, const int n, const int ty) {
    if (n < 15) { o[0] = (uint8_t)((n << 4) | ty); return 1; }
    o[0] = (uint8_t)(0xF0 | ty); o[1] = 0x11; o[2] = (uint8_t)n;
    return 3;
}
VGL_HD int value_width(const int f, const int pl_width) { return f == sal::F_PL ? pl_width : 4; }

enum { P_GEN = 0, P_SHARED, P_FILE, P_PLANE };
// the pieces of a record behind its 8 length bytes, in output order: put(kind, where, len, k) -- P_SHARED / P_FILE / P_PLANE: len bytes
// from byte `where` of that source; P_GEN: the descriptor of touched field k (put_typed_len)
template <class F>
VGL_HD void pieces(const Desc& d, const sal::BRec& r, const int64_t N, const int pl_width, F put) {
    put((int)P_SHARED, d.shared_off, (int64_t)d.shared_len, -1);
    VGL_SA_UNROLL
    for (int k = 0; k < MAX_RUNS; k++) {                               // (a fixed count, unrolled: the table stays in registers)
        if (k > d.n_touched) break;
        put((int)P_FILE, d.run_off[k], d.run_len[k], -1);
        if (k == d.n_touched || k == MAX_TOUCHED) break;
        const int f = d.f[k];
        put((int)P_FILE, d.key_off[k], (int64_t)d.key_len[k], -1);
        put((int)P_GEN, (int64_t)0, (int64_t)(r.n_new_g < 15 ? 1 : 3), k);
        put((int)P_PLANE, (r.plane_off + (int64_t)sal::b_slot(r, f) * r.n_new_g * N) * 4, N * r.n_new_g * value_width(f, pl_width), -1);
    }
}

// Every piece inside its source, the counts inside the rules.  pl_width is looked at only when PL is touched.
VGL_HD bool check(const Desc& d, const sal::BRec& r, const int64_t N, const int pl_width, const Sources& S) {
    if (N < 0 || d.n_touched < 0 || d.n_touched > MAX_TOUCHED || d.shared_len < 24) return false;
    if (d.shared_off < 0 || d.shared_off > S.shared_total - d.shared_len) return false;
    bool ok = true;
    VGL_SA_UNROLL
    for (int k = 0; k < MAX_RUNS; k++)
        if (k <= d.n_touched && (d.run_off[k] < 0 || d.run_len[k] < 0 || d.run_len[k] > S.file_total || d.run_off[k] > S.file_total - d.run_len[k])) ok = false;
    if (!ok) return false;
    if (d.n_touched == 0) return true;
    if (!sal::brec_sane(r) || d.n_touched != sal::b_fields(r)) return false;
    if (r.plane_off < 0 || r.plane_off > S.plane_vals || sal::b_plane_vals(r, N) > S.plane_vals - r.plane_off) return false;
    int seen = 0;
    VGL_SA_UNROLL
    for (int k = 0; k < MAX_TOUCHED; k++) {
        if (k >= d.n_touched) break;
        const int f = d.f[k];
        const int nv = f == 0 ? r.nv[0] : f == 1 ? r.nv[1] : f == 2 ? r.nv[2] : 0;
        if (f < 0 || f >= sal::NF || ((seen >> f) & 1) || nv <= 0) ok = false;
        seen |= 1 << (f & 3);
        if (f == sal::F_PL && !(pl_width == 1 || pl_width == 2 || pl_width == 4)) ok = false;
        if (d.key_len[k] < 2 || d.key_len[k] > KEY_MOST || d.key_off[k] < 0 || d.key_off[k] > S.file_total - d.key_len[k]) ok = false;
    }
    return ok;
}

// l_indiv of the record (a checked descriptor: every term is small against 2^63)
VGL_HD int64_t indiv_len(const Desc& d, const sal::BRec& r, const int64_t N, const int pl_width) {
    int64_t n = 0;
    pieces(d, r, N, pl_width, [&](int kind, int64_t, int64_t len, int) { if (kind != P_SHARED) n += len; });
    return n;
}
// the record's bytes in the output; -1: a length that does not fit the 32 bits of its length word
VGL_HD int64_t record_len(const Desc& d, const sal::BRec& r, const int64_t N, const int pl_width) {
    const int64_t li = indiv_len(d, r, N, pl_width);
    return li > (int64_t)0xFFFFFFFFll ? -1 : 8 + (int64_t)d.shared_len + li;
}

// the 16 bytes at byte a of src (a + 16 <= total) as four words, little end first
VGL_HD void load16_any(const uint8_t* src, const int64_t a, const int64_t total, uint32_t w[4]) {
    const unsigned k = (unsigned)(((uintptr_t)(src + a)) & 15u);
    if (k == 0) { __builtin_memcpy(w, __builtin_assume_aligned(src + a, 16), 16); return; }
    const int64_t lo = a - (int64_t)k;
    if (lo < 0 || lo + 32 > total) {
        w[0] = w[1] = w[2] = w[3] = 0;
        for (int i = 0; i < 16; i++) w[i >> 2] |= (uint32_t)src[a + i] << (8 * (i & 3));
        return;
    }
    uint32_t x[8];
    __builtin_memcpy(x, __builtin_assume_aligned(src + lo, 16), 16);
    __builtin_memcpy(x + 4, __builtin_assume_aligned(src + lo + 16, 16), 16);
    const unsigned ws = k >> 2, bs = 8 * (k & 3u);
    uint32_t y[5];
    for (int i = 0; i < 5; i++) y[i] = ws == 0 ? x[i] : ws == 1 ? x[i + 1] : ws == 2 ? x[i + 2] : x[i + 3];      // (selects, not an indexed array: registers)
    for (int i = 0; i < 4; i++) w[i] = bs == 0 ? y[i] : (y[i] >> bs) | (y[i + 1] << (32 - bs));
}

VGL_HD void copy_run(uint8_t* dst, const int64_t d, const uint8_t* src, const int64_t s, const int64_t s_total, const int64_t n, const int lane, const int n_lanes) {
    if (n <= 0) return;
    int64_t head = (int64_t)((16u - (unsigned)(((uintptr_t)(dst + d)) & 15u)) & 15u);
    if (head > n) head = n;
    const int64_t body = (n - head) >> 4, tail = head + (body << 4);
    for (int64_t j = lane; j < head; j += n_lanes) dst[d + j] = src[s + j];
    for (int64_t j = tail + lane; j < n; j += n_lanes) dst[d + j] = src[s + j];
    for (int64_t c = lane; c < body; c += n_lanes) {
        uint32_t w[4];
        load16_any(src, s + head + 16 * c, s_total, w);
        __builtin_memcpy(__builtin_assume_aligned(dst + d + head + 16 * c, 16), w, 16);
    }
}

// The record into out[o0, o1): false, and nothing written, when the descriptor does not pass check() or its length is not o1 - o0.
// Every lane of the caller's n_lanes makes the same call with its own `lane`; lane 0 writes the lengths and the descriptors.
VGL_HD bool write_record(uint8_t* out, const int64_t o0, const int64_t o1, const Desc& d, const sal::BRec& r, const int64_t N, const int pl_width, const Sources& S,
                         const int lane, const int n_lanes) {
    if (o0 < 0 || o1 < o0 || !check(d, r, N, pl_width, S) || record_len(d, r, N, pl_width) != o1 - o0) return false;
    const uint32_t li = (uint32_t)indiv_len(d, r, N, pl_width);
    if (lane == 0)
        for (int i = 0; i < 4; i++) { out[o0 + i] = (uint8_t)((uint32_t)d.shared_len >> (8 * i)); out[o0 + 4 + i] = (uint8_t)(li >> (8 * i)); }
    int64_t p = o0 + 8;
    pieces(d, r, N, pl_width, [&](int kind, int64_t where, int64_t len, int k) {
        if (kind == P_GEN) {
            uint8_t b[3];
            const int nb = put_typed_len(b, r.n_new_g, d.f[k] == sal::F_PL ? pl_type(pl_width) : 5);
            if (lane == 0) for (int i = 0; i < nb; i++) out[p + i] = b[i];
        }
        else if (kind == P_SHARED) copy_run(out, p, S.shared, where, S.shared_total, len, lane, n_lanes);
        else if (kind == P_FILE) copy_run(out, p, S.file, where, S.file_total, len, lane, n_lanes);
        else copy_run(out, p, S.planes, where, S.plane_vals * 4, len, lane, n_lanes);
        p += len;
    });
    return true;
}

}  // namespace salres
#endif
