// sal_core.h -- the rules of setalleles_hip (misc/setAlleles of the reference: a record file gets a new REF/ALT list per record, its
// FORMAT GL / PL / GP are put in the new genotype order and renormalised) as code that compiles for the host and for the device: the
// host path (--on-device 0), the kernel of setalfile.hip (the BCF rules) and a host program under the sanitizers (tests/sal_core_main.cpp) all run
// these routines.  The maps and the three normalisations are vgl_setal_core.h's; the float token grammar is fgl_core.h's.
//
// A record of VCF text is one region, its sample columns, and a descriptor (Rec) from the first nine columns: the places k[] of GL, PL
// and GP in FORMAT (-1: the record does not have the field), the old and the new genotype count, and oldgt2newgt as 15 nibbles.
//   column      the text between two tabs, fields between ':'.  A column that ends before a field, and a field ".", are one missing
//               value (count 1).  Otherwise the field's count is its commas + 1
//   old vector  the field's tokens, then end-of-vector up to n_old_g.  More tokens than n_old_g: RANGE
//   token       GL, GP: fgl::parse_token (the float htslib reads).  PL: "." (INT32_MIN), or an optional sign and 1 .. 10 digits inside
//               int32.  A token outside these grammars: HOST -- the record is redone with strtod / strtol by the program, which owns every message
//   scatter     plane[field][new genotype h][sample] = old value g for h = oldgt2newgt[g] >= 0, in ascending g (the tool's loop)
//   normalise   per sample and field, see norm_flt / norm_pl below
// A plane of a record and field is n_new_g rows of N values.  The planes of a record's fields follow each other from Rec::plane_off in the order
// GL, PL, GP, absent fields left out.
// No routine reads a byte at or past the `le` it is given.  No translation unit that includes this header may be built with fast-math.
#ifndef SAL_CORE_H
#define SAL_CORE_H
#include <stdint.h>
#include <string.h>

#include "../vgl_setal_core.h"
#include "fgl_core.h"

namespace sal {

enum { ST_OK = 0, ST_HOST = 1, ST_RANGE = 2 };
enum { F_GL = 0, F_PL = 1, F_GP = 2, NF = 3 };
enum { FL_BAD = 1, FL_MANY = 2 };                                  // a token outside the grammar; a field with more values than n_old_g
enum { MAX_A = vgl_setal::MAX_A, MAX_G = vgl_setal::MAX_G };
enum : uint32_t { F_MISSING = 0x7F800001u, F_END = 0x7F800002u, I_MISSING = 0x80000000u, I_END = 0x80000001u, QNAN = 0x7FC00000u };

struct Rec {
    int64_t off;                       // the region in the batch's text
    int64_t plane_off;                 // the record's first plane, in values
    uint64_t o2n;                      // nibble g: oldgt2newgt[g] + 1 (0: the old genotype is dropped)
    int32_t len;
    int16_t k[NF];                     // the field's index in FORMAT, -1: absent
    int8_t n_old_g, n_new_g;
};

VGL_HD int n_fields(const Rec& r) { return (r.k[0] >= 0) + (r.k[1] >= 0) + (r.k[2] >= 0); }
// the place of field f's plane behind plane_off, in planes
VGL_HD int field_slot(const Rec& r, const int f) { return (f > 0 && r.k[0] >= 0) + (f > 1 && r.k[1] >= 0); }
VGL_HD int64_t plane_vals(const Rec& r, const int64_t N) { return (int64_t)n_fields(r) * r.n_new_g * N; }
VGL_HD uint64_t pack_o2n(const int8_t* oldgt2newgt) {
    uint64_t m = 0;
    for (int g = 0; g < MAX_G; g++) m |= (uint64_t)(oldgt2newgt[g] + 1) << (4 * g);
    return m;
}
// what the device checks before it trusts a descriptor: counts inside the maps, every nibble a genotype of the new list
VGL_HD bool rec_sane(const Rec& r) {
    if (r.n_old_g < 1 || r.n_old_g > MAX_G || r.n_new_g < 1 || r.n_new_g > MAX_G || (r.o2n >> 60)) return false;
    bool ok = true;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; g++) if ((int)((r.o2n >> (4 * g)) & 15u) > r.n_new_g) ok = false;
    return ok;
}

// PL: the token [b, e) -> its int32 bits; false: outside the device grammar
VGL_HD bool parse_pl_token(const uint8_t* t, int64_t b, const int64_t e, uint32_t& bits) {
    if (e - b == 1 && t[b] == '.') { bits = I_MISSING; return true; }
    bool neg = false;
    if (b < e && (t[b] == '-' || t[b] == '+')) { neg = t[b] == '-'; b++; }
    const int64_t n = e - b;
    if (n < 1 || n > 10) return false;
    uint64_t v = 0;
    for (; b < e; b++) { if (!fgl::is_digit(t[b])) return false; v = v * 10u + (uint64_t)(t[b] - '0'); }
    if (v > (neg ? 2147483648ull : 2147483647ull)) return false;
    bits = neg ? (uint32_t)(0u - (uint32_t)v) : (uint32_t)v;
    return true;
}

// the device grammar's reader of a token; the host's strtod / strtol reader (setal_main.cpp) has the same shape
struct GrammarReader {
    VGL_HD bool flt(const uint8_t* t, int64_t b, int64_t e, int64_t, int, uint32_t& bits) const { return fgl::parse_token(t, b, e, bits); }
    VGL_HD bool pl(const uint8_t* t, int64_t b, int64_t e, int64_t, uint32_t& bits) const { return parse_pl_token(t, b, e, bits); }
};

// The column `col` that starts at q of the region that ends at le: the values of its GL / PL / GP fields, scattered into the record's
// planes.  Returns FL_ flags.
template <class R>
VGL_HD int column_values(const uint8_t* t, int64_t q, const int64_t le, const Rec& r, const int64_t N, const int64_t col, R& rd, uint32_t* planes) {
    int flags = 0, seen = 0;
    const int nog = r.n_old_g;
    auto put = [&](const int f, const int g, const uint32_t bits) {
        const int h = (int)((r.o2n >> (4 * g)) & 15u) - 1;
        if (h >= 0) planes[r.plane_off + ((int64_t)field_slot(r, f) * r.n_new_g + h) * N + col] = bits;
    };
    for (int fi = 0;; fi++) {
        const int f = fi == r.k[F_GL] ? F_GL : fi == r.k[F_PL] ? F_PL : fi == r.k[F_GP] ? F_GP : -1;
        if (f < 0) {
            while (q < le && t[q] != '\t' && t[q] != ':') q++;
        } else {
            seen |= 1 << f;
            int c = 0;
            for (;;) {
                const int64_t tb = q;
                while (q < le && t[q] != '\t' && t[q] != ':' && t[q] != ',') q++;
                if (c < nog) {
                    uint32_t bits = 0;
                    const bool ok = f == F_PL ? rd.pl(t, tb, q, col, bits) : rd.flt(t, tb, q, col, f, bits);
                    if (ok) put(f, c, bits); else flags |= FL_BAD;
                } else flags |= FL_MANY;
                c++;
                if (q < le && t[q] == ',') { q++; continue; }
                break;
            }
            for (; c < nog; c++) put(f, c, f == F_PL ? (uint32_t)I_END : (uint32_t)F_END);
        }
        if (q >= le || t[q] == '\t') break;
        q++;                                                           // the ':'
    }
    for (int f = 0; f < NF; f++) {
        if (r.k[f] < 0 || ((seen >> f) & 1)) continue;                 // the column ended before the field: one missing value
        put(f, 0, f == F_PL ? (uint32_t)I_MISSING : (uint32_t)F_MISSING);
        for (int c = 1; c < nog; c++) put(f, c, f == F_PL ? (uint32_t)I_END : (uint32_t)F_END);
    }
    return flags;
}

VGL_HD int record_status(const int flags, const int64_t cols, const int64_t N) {
    if (flags & FL_BAD) return ST_HOST;
    return (cols != N || (flags & FL_MANY)) ? ST_RANGE : ST_OK;
}

// One record of VCF text by the rules above, a column at a time
template <class R>
inline int record_plain(const uint8_t* text, const Rec& r, const int64_t N, R& rd, uint32_t* planes, int64_t* cols_out) {
    const int64_t le = r.off + r.len;
    int64_t col = 0, q = r.off;
    int flags = 0;
    for (;;) {
        if (col < N) flags |= column_values(text, q, le, r, N, col, rd, planes);
        col++;
        while (q < le && text[q] != '\t') q++;
        if (q >= le) break;
        q++;
    }
    if (cols_out) *cols_out = col;
    return record_status(flags, col, N);
}

// ---- the normalisations: v[0 .. n) in the new genotype order, as bits -----------------------------------------------------------------
// GL (gp false) and GP: any NaN among the new values -- the missing pattern, end-of-vector or a real one -- makes the sample missing:
// the FIRST NaN becomes the missing pattern and nothing else changes.  Otherwise vgl_setal's norm_gl / norm_gp, and a NaN the
// arithmetic makes (-inf - -inf, 0 / 0) is the canonical quiet NaN whatever the machine's own choice of sign.
VGL_HD void norm_flt(uint32_t* v, const int n, const bool gp) {
    int first = -1;
    VGL_SA_UNROLL
    for (int g = MAX_G - 1; g >= 0; --g)
        if (g < n && vgl_setal::sa_isnan(v[g])) first = g;
    if (first >= 0) {
        VGL_SA_UNROLL
        for (int g = 0; g < MAX_G; ++g)
            if (g == first) v[g] = F_MISSING;
        return;
    }
    if (gp) vgl_setal::norm_gp(v, n); else vgl_setal::norm_gl(v, n);
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n && vgl_setal::sa_isnan(v[g])) v[g] = QNAN;
}

// PL: INT32_MIN among the new values leaves the sample as gathered.  Otherwise (int32)((float)pl - (float)min), end-of-vector an
// ordinary value: a sample of nothing but end-of-vector becomes zeros.  True: the cast would overflow (end-of-vector beside ordinary
// values, or a difference of 2^31 and more) -- undefined in the tool, the run stops there.
VGL_HD bool norm_pl(uint32_t* v, const int n) {
    bool miss = false, any_end = false, all_end = true;
    float mn = vgl_setal::sa_float(0x7F800000u);
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) {
            miss = miss || v[g] == I_MISSING; any_end = any_end || v[g] == I_END; all_end = all_end && v[g] == I_END;
            const float x = (float)(int32_t)v[g];
            if (x < mn) mn = x;
        }
    if (miss) return false;
    if (any_end && !all_end) return true;
    bool over = false;
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) {
            const float d = (float)(int32_t)v[g] - mn;
            if (!(d < 2147483648.0f)) over = true; else v[g] = (uint32_t)(int32_t)d;
        }
    return over;
}

// sample s of one plane (n rows of N values): loaded, normalised, stored back.  True: norm_pl's overflow
VGL_HD bool norm_sample(uint32_t* plane, const int64_t N, const int64_t s, const int n, const int f) {
    uint32_t v[MAX_G];
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g) v[g] = g < n ? plane[(int64_t)g * N + s] : 0u;
    bool over = false;
    if (f == F_PL) over = norm_pl(v, n); else norm_flt(v, n, f == F_GP);
    VGL_SA_UNROLL
    for (int g = 0; g < MAX_G; ++g)
        if (g < n) plane[(int64_t)g * N + s] = v[g];
    return over;
}

// ---- BCF: a record is its GL / PL / GP vector blocks, N vectors of nv values each ------------------------------------------------------
// The old vector of a sample is the stored nv values and then end-of-vector up to n_old_g; the new one is gathered, new[h] =
// old[newgt2oldgt[h]] (with distinct names on either side the same assignment as the scatter), and normalised as above.
struct BRec {
    int64_t in_off[NF];                // the field's vectors in the batch's bytes, a multiple of 4
    int64_t plane_off;                 // the record's first plane, in 32-bit words: n_new_g N words per field it has, GL, PL, GP
    uint64_t n2o;                      // nibble h: newgt2oldgt[h] + 1
    int32_t nv[NF];                    // values per old vector; 0: the record does not have the field
    int8_t ty[NF];                     // the BCF type of the old vectors: 5 for GL and GP, 1 / 2 / 3 for PL
    int8_t n_old_g, n_new_g;
    int8_t pad[3];
};
VGL_HD int b_fields(const BRec& r) { return (r.nv[0] > 0) + (r.nv[1] > 0) + (r.nv[2] > 0); }
VGL_HD int b_slot(const BRec& r, const int f) { return (f > 0 && r.nv[0] > 0) + (f > 1 && r.nv[1] > 0); }
VGL_HD int64_t b_plane_vals(const BRec& r, const int64_t N) { return (int64_t)b_fields(r) * r.n_new_g * N; }
VGL_HD int type_width(const int ty) { return ty == 1 ? 1 : ty == 2 ? 2 : (ty == 3 || ty == 5) ? 4 : 0; }
VGL_HD bool brec_sane(const BRec& r) {
    if (r.n_old_g < 1 || r.n_old_g > MAX_G || r.n_new_g < 1 || r.n_new_g > MAX_G || (r.n2o >> 60)) return false;
    bool ok = true;
    VGL_SA_UNROLL
    for (int h = 0; h < MAX_G; h++) {
        const int g = (int)((r.n2o >> (4 * h)) & 15u);
        if (h < r.n_new_g ? (g < 1 || g > r.n_old_g) : g != 0) ok = false;
    }
    VGL_SA_UNROLL
    for (int f = 0; f < NF; f++) {
        if (r.nv[f] < 0 || r.nv[f] > r.n_old_g) ok = false;
        if (r.nv[f] > 0 && (f == F_PL ? (r.ty[f] < 1 || r.ty[f] > 3) : r.ty[f] != 5)) ok = false;
    }
    return ok;
}
// value i of a vector of BCF type ty as 32 bits, the narrow sentinels widened
VGL_HD uint32_t widen8(const uint8_t b) { const int8_t x = (int8_t)b; return x == -128 ? (uint32_t)I_MISSING : x == -127 ? (uint32_t)I_END : (uint32_t)(int32_t)x; }
VGL_HD uint32_t widen16(const uint16_t b) { const int16_t x = (int16_t)b; return x == -32768 ? (uint32_t)I_MISSING : x == -32767 ? (uint32_t)I_END : (uint32_t)(int32_t)x; }
VGL_HD uint32_t bcf_load(const uint8_t* p, const int ty, const int i) {
    if (ty == 1) return widen8(p[i]);
    if (ty == 2) { uint16_t x; memcpy(&x, p + 2 * i, 2); return widen16(x); }
    uint32_t b; memcpy(&b, p + 4 * i, 4);
    return b;
}
// one sample: load(g) = value g of its old vector, widened -> v[0 .. n_new_g) gathered and normalised.  True: norm_pl's overflow
template <class L>
VGL_HD bool bcf_sample_from(const L load, const int nv, const uint64_t n2o, const int n_new, const int f, uint32_t* v) {
    VGL_SA_UNROLL
    for (int h = 0; h < MAX_G; ++h) {
        const int g = (int)((n2o >> (4 * h)) & 15u) - 1;
        v[h] = (h < n_new && g >= 0 && g < nv) ? load(g) : (f == F_PL ? (uint32_t)I_END : (uint32_t)F_END);
    }
    if (f == F_PL) return norm_pl(v, n_new);
    norm_flt(v, n_new, f == F_GP);
    return false;
}
// ... its old vector at vec
struct VecLoad { const uint8_t* vec; int ty; VGL_HD uint32_t operator()(const int g) const { return bcf_load(vec, ty, g); } };
VGL_HD bool bcf_sample(const uint8_t* vec, const int ty, const int nv, const uint64_t n2o, const int n_new, const int f, uint32_t* v) {
    return bcf_sample_from(VecLoad{vec, ty}, nv, n2o, n_new, f, v);
}
// an int32 of the new PL at the record's width w (1, 2, 4 bytes), missing and end-of-vector as that width's sentinels
VGL_HD void store_narrow(uint8_t* p, const int w, const int64_t i, const uint32_t x) {
    if (w == 1) p[i] = x == I_MISSING ? 0x80u : x == I_END ? 0x81u : (uint8_t)x;
    else if (w == 2) { const uint16_t y = x == I_MISSING ? 0x8000u : x == I_END ? 0x8001u : (uint16_t)x; memcpy(p + 2 * i, &y, 2); }
    else memcpy(p + 4 * i, &x, 4);
}

// htslib's bcf_enc_vint: the narrowest of int8 / int16 / int32 that holds every value of [mn, mx] beside its sentinels (1, 2, 4 bytes)
VGL_HD int int_width(const int32_t mn, const int32_t mx) {
    if (mx <= 127 && mn >= -120) return 1;
    if (mx <= 32767 && mn >= -32760) return 2;
    return 4;
}

}  // namespace sal
#endif
