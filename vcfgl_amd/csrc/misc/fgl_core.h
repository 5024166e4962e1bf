// fgl_core.h -- the rules of fetchgl_hip (misc/fetchGl of the reference: one genotype's FORMAT/GL of every sample of a record file, as
// CSV) as code that compiles for the host and for the device: the host path (--on-device 0), the kernels of fetchgl.hip and a host
// program under the sanitizers (tests/fgl_core_main.cpp) all run these routines, so they cannot drift apart.
//
// A record of VCF text is one region, its sample columns, and a descriptor (Rec) from the first nine columns: the index k of GL in
// FORMAT, the genotype's index g, POS.
//   column      the text between two tabs; its GL field is found by skipping k ':'.  A column that ends before the field, and a field
//               '.', are one missing value (count 1).  Otherwise the field's count c is its commas + 1
//   value       g < c: token g of the field.  '.' is MISSING; any other token is the float htslib reads, the nearest double of the text
//               and then the nearest float of that double.  g >= c: END -- as long as g < n_gls, the largest count of the record
//   RANGE       g >= n_gls (the tool reads outside its buffer there), or a column count other than the header's sample count
//   HOST        the picked token is outside the DEVICE GRAMMAR: the host redoes the record with strtod (and owns every message)
// The device grammar of a token: an optional sign, digits with at most one point (one digit at least), an optional exponent
// ('e' / 'E', an optional sign, one to three digits); at most 15 significant digits m (counted from the first digit that is not 0)
// and a decimal scale k, the exponent less the digits behind the point, with |k| <= 22.  m < 2^53 and 10^|k| are exact doubles, so
// the nearest double of the text is ONE correctly rounded multiplication or division, and one conversion gives the float (no
// translation unit that includes this header may be built with fast-math).  Besides that exactly ".", "inf", "-inf" and "nan".
// A BCF record is its GL vector block: N vectors of n floats; the value is the stored float g of sample s, n_gls = n.
// A line is "POS,v0,...,vN-1\n", every value printed by vgl_fetchgl::fmt_value in MODE_FLOAT (the bits are the file's float already).
// No routine reads a byte at or past the `le` it is given.
#ifndef FGL_CORE_H
#define FGL_CORE_H
#include <stdint.h>
#include <string.h>

#include "../vgl_fetchgl_core.h"

namespace fgl {

enum { ST_OK = 0, ST_HOST = 1, ST_RANGE = 2 };
enum { MAX_DIGITS = 15, MAX_SCALE = 22, MAX_POS_LEN = 20 };
enum : uint32_t { MISSING_BITS = vgl_fetchgl::MISSING_BITS, END_BITS = vgl_fetchgl::END_BITS };
// a value's text and the ',' or '\n' behind it
enum { VALUE_BOUND = vgl_fetchgl::MAX_VALUE_LEN + 1 };

// what the first nine columns of a record say (VCF text), or where its GL vectors lie (BCF: len = the vector length n, k unused)
struct Rec {
    int64_t off;                       // the region in the batch's text (BCF: a multiple of 4)
    int64_t pos;                       // POS as written (1-based)
    int32_t len;
    int32_t k;                         // GL's index in FORMAT
    int32_t g;                         // the genotype's index
    int32_t pad;
};

// g of two allele indices
VGL_HD int genotype_of(const int a, const int b) { const int hi = a > b ? a : b, lo = a > b ? b : a; return hi * (hi + 1) / 2 + lo; }

VGL_HD bool is_digit(const int c) { return c >= '0' && c <= '9'; }

// the token [b, e) of `t` -> the bits of the float htslib reads; false: outside the device grammar
VGL_HD bool parse_token(const uint8_t* t, int64_t b, const int64_t e, uint32_t& bits) {
    const int64_t n = e - b;
    if (n <= 0) return false;
    if (n == 1 && t[b] == '.') { bits = MISSING_BITS; return true; }
    if (n == 3 && t[b] == 'i' && t[b + 1] == 'n' && t[b + 2] == 'f') { bits = 0x7F800000u; return true; }
    if (n == 4 && t[b] == '-' && t[b + 1] == 'i' && t[b + 2] == 'n' && t[b + 3] == 'f') { bits = 0xFF800000u; return true; }
    if (n == 3 && t[b] == 'n' && t[b + 1] == 'a' && t[b + 2] == 'n') { bits = 0x7FC00000u; return true; }
    bool neg = false;
    if (t[b] == '-' || t[b] == '+') { neg = t[b] == '-'; b++; }
    uint64_t m = 0;
    int sig = 0, digits = 0, behind = 0;
    bool point = false;
    for (; b < e; b++) {
        const int c = t[b];
        if (c == '.') { if (point) return false; point = true; continue; }
        if (!is_digit(c)) break;
        digits++;
        if (point) behind++;
        if (sig > 0 || c != '0') { if (++sig > MAX_DIGITS) return false; m = m * 10u + (uint64_t)(c - '0'); }
    }
    if (digits == 0) return false;
    int ex = 0;
    if (b < e) {
        if (t[b] != 'e' && t[b] != 'E') return false;
        b++;
        bool eneg = false;
        if (b < e && (t[b] == '-' || t[b] == '+')) { eneg = t[b] == '-'; b++; }
        int nd = 0;
        for (; b < e && is_digit(t[b]); b++) { if (++nd > 3) return false; ex = ex * 10 + (t[b] - '0'); }
        if (nd == 0 || b < e) return false;
        if (eneg) ex = -ex;
    }
    const int k = ex - behind;
    if (k > MAX_SCALE || k < -MAX_SCALE) return false;
    double d = (double)m;                                              // exact: m < 10^15
    if (k > 0) d = d * vgl_fetchgl::fg_pow10(k);                       // one IEEE operation each
    else if (k < 0) d = d / vgl_fetchgl::fg_pow10(-k);
    const float f = (float)d;                                          // (at most 1e37: it fits)
    uint32_t fb; memcpy(&fb, &f, 4);
    bits = fb | (neg ? 0x80000000u : 0u);
    return true;
}

// The column that starts at q of the region that ends at le: its GL field's value count and the bits of value g (END_BITS for
// count <= g).  false: the picked token is outside the device grammar (bits and count are then unspecified).
VGL_HD bool sample_value(const uint8_t* t, int64_t q, const int64_t le, const int k, const int g, uint32_t& bits, int32_t& count) {
    for (int f = 0; f < k; f++) {
        for (;;) {
            if (q >= le || t[q] == '\t') { count = 1; bits = g == 0 ? MISSING_BITS : END_BITS; return true; }
            if (t[q++] == ':') break;
        }
    }
    int32_t c = 1;
    int64_t tb = q, te = -1;                                           // token g: [tb, te)
    for (; q < le && t[q] != '\t' && t[q] != ':'; q++) {
        if (t[q] != ',') continue;
        if (c - 1 == g) te = q;
        c++;
        if (c - 1 == g) tb = q + 1;
    }
    count = c;
    if (g >= c) { bits = END_BITS; return true; }
    if (te < 0) te = q;
    return parse_token(t, tb, te, bits);
}

// what a record's counts say once every column is read: cols against the header's N, g against the largest count
VGL_HD int record_status(const bool bad, const int64_t cols, const int64_t N, const int32_t n_gls, const int32_t g) {
    if (bad) return ST_HOST;
    return (cols != N || g >= n_gls) ? ST_RANGE : ST_OK;
}

// One record of VCF text by the rules above, a column at a time: what k_fgl_parse does with a lane per column.  plane: N values.
// Returns ST_OK, or ST_HOST / ST_RANGE (the plane is then unspecified).
inline int record_plain(const uint8_t* text, const Rec& r, const int64_t N, uint32_t* plane, int32_t* n_gls_out) {
    const int64_t le = r.off + r.len;
    int64_t col = 0, q = r.off;
    int32_t n_gls = 0; bool bad = false;
    for (;;) {
        if (col < N) {
            uint32_t b = 0; int32_t c = 0;
            if (!sample_value(text, q, le, r.k, r.g, b, c)) bad = true; else { plane[col] = b; if (c > n_gls) n_gls = c; }
        }
        col++;
        while (q < le && text[q] != '\t') q++;
        if (q >= le) break;
        q++;
    }
    if (n_gls_out) *n_gls_out = n_gls;
    return record_status(bad, col, N, n_gls, r.g);
}

// ---- the line ------------------------------------------------------------------------------------------------------------------
template <bool W>
VGL_HD void put_pos(vgl_fetchgl::Emit<W>& e, uint64_t v) {
    char d[MAX_POS_LEN]; int k = 0;
    do { d[k++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
    while (k) e.put(d[--k]);
    e.put(',');
}
VGL_HD uint32_t pos_len(const int64_t pos) { vgl_fetchgl::Emit<false> e{nullptr, 0u, 0u}; put_pos(e, (uint64_t)pos); return e.n; }
// a value and the separator behind it: ',' or, for the last sample, '\n'
template <bool W>
VGL_HD void put_value(vgl_fetchgl::Emit<W>& e, const uint32_t bits, const bool last) {
    vgl_fetchgl::fmt_value(e, bits, vgl_fetchgl::MODE_FLOAT);
    e.put(last ? '\n' : ',');
}
VGL_HD uint32_t value_len(const uint32_t bits) { vgl_fetchgl::Emit<false> e{nullptr, 0u, 0u}; put_value(e, bits, false); return e.n; }

}  // namespace fgl
#endif
