// gtdbcf_core.h -- gtdiscordance_hip --bcf-direct 1: the rules of gtdisc_core.h on the typed GT / GQ / PL vectors of a BCF record,
// as code that compiles for the host and for the device (the host path, k_gtd_bcf_decode of gtdisc.hip and tests/gtdbcf_core_main.cpp
// run these routines).  The specification is the text route: bcf_lines() of gtdisc_main.cpp writes a record's vectors as the sample
// columns "GT[:GQ][:PL]" and gtd::sample_true / gtd::sample_call judge that text.  Every routine here returns, for one sample, what
// those two return on that text -- nothing is guessed: a sample outside the rules below makes the record ST_HOST, its line is then
// written after all and the permissive reader of the program takes it.
//   widening    as BcfIn::ints: int8 -128 / int16 -32768 -> missing (INT32_MIN), -127 / -32767 -> end-of-vector (INT32_MIN + 1);
//               int32 holds the two as they are
//   alleles     the values before the first end-of-vector, allele index = (x >> 1) - 1, a negative index is written '.'
//   plain GT    exactly two alleles, each '.' or an index 0 .. 99 (the text grammar takes one or two digits); one allele ("0"), none
//               ("."), three ("0/1/2") and an index of three digits are not plain
//   true GT     both alleles present, below min(allele count, 16), both mapping to a base -- gtd::sample_true's order
//   called GT   gtd::sample_call's order: under GQ_PL with more than one allele the PL rule first, for every sample; then a missing
//               allele makes the call CALL_MISSING (before the allele-count limit: "./17" of 4 alleles is a missing call); then the
//               limit, the base map, and GQ under GQ_TAG
//   GQ_TAG      the first GQ value, plain for 1 .. 127; missing, end-of-vector, an empty vector, 0, negative and 128 and above are not
//   GQ_PL       exactly nG values before the end-of-vector, each missing or 0 .. 9999 (the text grammar takes four digits), walked by
//               gtd::PlWalk as it is; a zero found and GQ >= 1
// A descriptor (BSide) says where the record's vectors lie in the bytes a batch carries; vec_fits() is checked before a vector is read
// and no routine reads outside the N vectors it describes.
#ifndef GTDBCF_CORE_H
#define GTDBCF_CORE_H
#include "gtdisc_core.h"

namespace gtd {

enum { B_GT = 1, B_GQ = 2, B_PL = 4 };                   // BSide::have: the FORMAT fields of the record that hold integers
enum : int32_t { BCF_MISSING = INT32_MIN, BCF_EOV = INT32_MIN + 1 };

// one side (truth or call) of a matched pair of records.  have == 0: the side is text (Rec::t_off / c_off say where)
struct BSide {
    int64_t gt_off, gq_off, pl_off;    // where the N vectors of each field start in the batch's bytes (unused where absent)
    int32_t gt_type, gq_type, pl_type; // BCF types 1 / 2 / 3: int8 / int16 / int32
    int32_t gt_n, gq_n, pl_n;          // values per sample
    int32_t nal;                       // allele count
    uint32_t have;                     // B_GT | B_GQ | B_PL
    uint64_t map;                      // allele -> base, a nibble per allele
};

VGL_HD int bcf_width(const int type) { return type == 1 ? 1 : type == 2 ? 2 : type == 3 ? 4 : 0; }

// N vectors of n values of `type` from byte `off` lie inside `bytes` bytes
VGL_HD bool vec_fits(const int64_t off, const int type, const int32_t n, const int64_t N, const int64_t bytes) {
    const int w = bcf_width(type);
    if (!w || off < 0 || n < 0 || N < 1 || off > bytes) return false;
    const int64_t per = (int64_t)w * n;
    return per == 0 || per <= (bytes - off) / N;
}

// value k of the vector at p, widened (read a byte at a time: no alignment is asked of p)
VGL_HD int32_t bcf_value(const uint8_t* p, const int type, const int64_t k) {
    if (type == 1) { const int8_t x = (int8_t)p[k]; return x == -128 ? BCF_MISSING : x == -127 ? BCF_EOV : (int32_t)x; }
    if (type == 2) {
        const int16_t x = (int16_t)(uint16_t)((uint32_t)p[2 * k] | (uint32_t)p[2 * k + 1] << 8);
        return x == -32768 ? BCF_MISSING : x == -32767 ? BCF_EOV : (int32_t)x;
    }
    return (int32_t)((uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24);
}

// two widened GT values that are both alleles -> a0 / a1 (-1 for '.'); false: an index of three digits or more
VGL_HD bool gt_pair(const int32_t x0, const int32_t x1, int& a0, int& a1) {
    const int32_t i0 = (x0 >> 1) - 1, i1 = (x1 >> 1) - 1;
    a0 = i0 < 0 ? -1 : (int)i0; a1 = i1 < 0 ? -1 : (int)i1;
    return i0 <= 99 && i1 <= 99;
}

// the GT vector of sample s: plain -> its two alleles
VGL_HD bool bcf_gt(const uint8_t* bytes, const BSide& b, const int64_t s, int& a0, int& a1) {
    if (b.gt_n < 2) return false;                                      // "0" or ".": no separator
    const uint8_t* p = bytes + b.gt_off + s * (int64_t)b.gt_n * bcf_width(b.gt_type);
    const int32_t x0 = bcf_value(p, b.gt_type, 0), x1 = bcf_value(p, b.gt_type, 1);
    if (x0 == BCF_EOV || x1 == BCF_EOV) return false;
    if (b.gt_n > 2 && bcf_value(p, b.gt_type, 2) != BCF_EOV) return false;   // a third allele
    return gt_pair(x0, x1, a0, a1);
}

// gtd::sample_true behind its gt_token
VGL_HD bool true_of(const BSide& b, const int a0, const int a1, uint32_t& tb) {
    if (a0 < 0 || a1 < 0) return false;
    const int lim = b.nal < 16 ? b.nal : 16;
    if (a0 >= lim || a1 >= lim) return false;
    const uint32_t b0 = map_nibble(b.map, a0), b1 = map_nibble(b.map, a1);
    tb = b0 | b1 << 4;
    return b0 < 4u && b1 < 4u;
}

// gtd::pl_gq on the PL vector of sample s
VGL_HD bool bcf_pl_gq(const uint8_t* bytes, const BSide& b, const int64_t s, const int nG, int& gq) {
    if (!(b.have & B_PL) || nG < 1 || b.pl_n < nG) return false;
    const uint8_t* p = bytes + b.pl_off + s * (int64_t)b.pl_n * bcf_width(b.pl_type);
    PlWalk w;
    for (int g = 0; g < nG; g++) {
        const int32_t x = bcf_value(p, b.pl_type, g);
        if (x == BCF_EOV) return false;                                // too few values
        if (x == BCF_MISSING) { w.add(-1); continue; }
        if (x < 0 || x > 9999) return false;
        w.add((int)x);
    }
    if (b.pl_n > nG && bcf_value(p, b.pl_type, nG) != BCF_EOV) return false;      // too many
    if (!w.zero) return false;
    gq = w.gq();
    return gq >= 1;
}

// gtd::sample_call behind its gt_token: the call's byte and GQ from its two alleles
VGL_HD bool call_of(const uint8_t* bytes, const BSide& b, const int64_t s, const int gq_mode, const int nG, const int a0, const int a1, uint32_t& cb, uint32_t& gq) {
    int g = 0;
    cb = CALL_MISSING; gq = 0;
    if (gq_mode == GQ_PL && b.nal > 1) { if (!bcf_pl_gq(bytes, b, s, nG, g)) return false; }     // (every sample, before GT is looked at)
    else if (gq_mode == GQ_PL || gq_mode == GQ_MAX) g = MAX_GQ;
    if (a0 < 0 || a1 < 0) return true;
    const int lim = b.nal < 16 ? b.nal : 16;
    if (a0 >= lim || a1 >= lim) return false;
    const uint32_t b0 = map_nibble(b.map, a0), b1 = map_nibble(b.map, a1);
    if (b0 > 3u || b1 > 3u) return false;
    if (gq_mode == GQ_TAG) {
        if (!(b.have & B_GQ) || b.gq_n < 1) return false;              // the column's GQ is '.'
        const int32_t x = bcf_value(bytes + b.gq_off + s * (int64_t)b.gq_n * bcf_width(b.gq_type), b.gq_type, 0);
        if (x < 1 || x > MAX_GQ) return false;                         // (missing and end-of-vector are negative)
        g = (int)x;
    }
    cb = b0 | b1 << 4; gq = (uint32_t)g;
    return true;
}

VGL_HD bool bcf_sample_true(const uint8_t* bytes, const BSide& b, const int64_t s, uint32_t& tb) {
    int a0, a1;
    return bcf_gt(bytes, b, s, a0, a1) && true_of(b, a0, a1, tb);
}
VGL_HD bool bcf_sample_call(const uint8_t* bytes, const BSide& b, const int64_t s, const int gq_mode, const int nG, uint32_t& cb, uint32_t& gq) {
    int a0, a1;
    cb = CALL_MISSING; gq = 0;
    return bcf_gt(bytes, b, s, a0, a1) && call_of(bytes, b, s, gq_mode, nG, a0, a1, cb, gq);
}

// the descriptor of a BCF side can be judged at all: every vector the mode reads lies inside `bytes` (truth: GT; call: GT, GQ under
// GQ_TAG, PL under GQ_PL with more than one allele)
VGL_HD bool side_fits(const BSide& b, const bool call, const int gq_mode, const int nG, const int64_t N, const int64_t bytes) {
    if (!(b.have & B_GT) || b.nal < 1 || !vec_fits(b.gt_off, b.gt_type, b.gt_n, N, bytes)) return false;
    if (!call) return true;
    if (gq_mode == GQ_TAG && (!(b.have & B_GQ) || !vec_fits(b.gq_off, b.gq_type, b.gq_n, N, bytes))) return false;
    if (gq_mode == GQ_PL && b.nal > 1 && (!(b.have & B_PL) || b.nal > 5 || nG != n_genotypes(b.nal) || !vec_fits(b.pl_off, b.pl_type, b.pl_n, N, bytes))) return false;
    return true;
}

// One side of a record from its vectors, a sample at a time: what k_gtd_bcf_decode does with its lanes.  tb (truth) or cb / gq (call):
// N bytes each.  Returns ST_OK, or ST_HOST (the planes are then unspecified).
inline int bcf_side_plain(const uint8_t* bytes, const int64_t n_bytes, const BSide& b, const bool call, const int gq_mode, const int nG, const int64_t N,
                          uint8_t* tb, uint8_t* cb, uint8_t* gq) {
    if (!side_fits(b, call, gq_mode, nG, N, n_bytes)) return ST_HOST;
    for (int64_t s = 0; s < N; s++) {
        uint32_t x, g;
        if (!call) { if (!bcf_sample_true(bytes, b, s, x)) return ST_HOST; tb[s] = (uint8_t)x; }
        else { if (!bcf_sample_call(bytes, b, s, gq_mode, nG, x, g)) return ST_HOST; cb[s] = (uint8_t)x; gq[s] = (uint8_t)g; }
    }
    return ST_OK;
}

}  // namespace gtd
#endif
