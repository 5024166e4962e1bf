// gtdisc_core.h -- the per-record and per-sample rules of gtdiscordance_hip (misc/gtDiscordance of the reference: a call file against
// -printTruth's file) as code that compiles for the host and for the device: the host path (--on-device 0), the kernels of gtdisc.hip
// and a host program under the sanitizers (tests/gtdisc_core_main.cpp) all run these routines, so they cannot drift apart.
//
// A record is two regions of text, the sample columns of the truth line and of the call line, and a descriptor (Rec) from the first nine
// columns.  The PLAIN grammar is what the routines here accept; anything else gives the record the status HOST and the program's
// permissive host reader takes the whole record (it also owns every message: nothing is guessed here).
//   column      the text between two tabs; its ':'-separated fields are found by index (GT, GQ, PL of the record's FORMAT)
//   GT          A S A, A = '.' or one or two decimal digits, S = '/' or '|'; an index must be below 16 and below the record's allele count
//   true GT     both alleles present, both mapping to a base (allele map nibble 0 .. 3)
//   called GT   either allele '.': the call is missing (plane byte 0xFF), nothing else of the column is judged -- but see PL
//   allele map  a nibble per allele: the base of its first character, A a 0 -> 0, C c 1 -> 1, G g 2 -> 2, T t 3 -> 3 (the tool's refToInt),
//               0xF for any other character
//   GQ          GQ_NONE (-doGQ 0): 0.  GQ_TAG: the GQ field, one to three digits, 1 .. 127.  GQ_MAX (a record without the tag under
//               -doGQ 7 / 8): 127.  GQ_PL (-doGQ 8, a header without GQ): one allele 127; otherwise exactly nG values, each '.' or one to
//               four digits, walked as the tool walks them: a missing value counts as a zero found and puts the second best back to 255,
//               a 0 is a zero found, any other value below the second best replaces it; GQ = min(second best, 127), and a sample
//               without a zero found is not plain -- for EVERY sample, compared or not (the tool asserts it before it looks at GT)
//   cell        true bases against called bases as unordered pairs: 0 hom->hom concordant, 1 hom->hom discordant, 2 het->het concordant,
//               3 het->het discordant, 4 hom->het, 5 het->hom (VGL_DISC_* of the library's table)
//   lines       -doGQ 1: nSites1 \t i \t dcType \t GQ;  -doGQ 2: nSites1 \t i \t dcType \t refToCallType \t GQ;
//               -perSite 1: POS \t i \t dcType \t refToCallType.  At most LINE_BOUND bytes each.
// No routine reads a byte at or past the `le` it is given.
#ifndef GTDISC_CORE_H
#define GTDISC_CORE_H
#include <stdint.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif

namespace gtd {

enum { ST_OK = 0, ST_HOST = 1 };
enum { GQ_NONE = 0, GQ_TAG = 1, GQ_MAX = 2, GQ_PL = 3 };
enum { LIST_NONE = 0, LIST_GQ = 1, LIST_GQ_TYPE = 2 };
enum { CALL_MISSING = 0xFF, MAX_GQ = 127, MAX_PL = 255, LINE_BOUND = 40, N_CELLS = 6, N_GQ = 128 };

// what the first nine columns of a matched pair of lines say
struct Rec {
    int64_t t_off, c_off;              // the two regions in the batch's text
    int32_t t_len, c_len;
    uint64_t t_map, c_map;             // allele -> base, a nibble per allele (16 alleles)
    int64_t pos;                       // POS as written (1-based)
    int32_t nsites1;                   // truth records read when this one was compared (1-based)
    int32_t t_nal, c_nal;              // allele counts
    int32_t t_gti, c_gti, c_gqi, c_pli;   // FORMAT indices; GQ / PL -1 where absent
    int32_t gq_mode, nG;
};

VGL_HD uint32_t base_of(const int c) {
    switch (c) {
        case 'A': case 'a': case '0': return 0u;
        case 'C': case 'c': case '1': return 1u;
        case 'G': case 'g': case '2': return 2u;
        case 'T': case 't': case '3': return 3u;
        default: return 15u;
    }
}
VGL_HD uint32_t map_nibble(const uint64_t map, const int a) { return (uint32_t)(map >> (4 * a)) & 15u; }
VGL_HD int n_genotypes(const int n_alleles) { return n_alleles * (n_alleles + 1) / 2; }

VGL_HD bool col_end(const uint8_t* t, const int64_t q, const int64_t le) { return q >= le || t[q] == '\t'; }
VGL_HD bool field_end(const uint8_t* t, const int64_t q, const int64_t le) { return q >= le || t[q] == '\t' || t[q] == ':'; }

// q to the start of the k-th field of the column that q stands in; false: the column has fewer fields
VGL_HD bool skip_fields(const uint8_t* t, int64_t& q, const int64_t le, const int k) {
    for (int f = 0; f < k; f++) {
        for (;;) {
            if (col_end(t, q, le)) return false;
            if (t[q++] == ':') break;
        }
    }
    return true;
}

// one allele at q: '.' -> -1, one or two digits -> the index, anything else -> -2
VGL_HD int allele(const uint8_t* t, int64_t& q, const int64_t le) {
    if (q >= le) return -2;
    const int c = t[q];
    if (c == '.') { q++; return -1; }
    if (c < '0' || c > '9') return -2;
    int v = c - '0'; q++;
    if (q < le && t[q] >= '0' && t[q] <= '9') { v = v * 10 + (t[q] - '0'); q++; }
    return v;
}

// the GT field of the column at q: exactly two alleles
VGL_HD bool gt_token(const uint8_t* t, int64_t q, const int64_t le, const int gti, int& a0, int& a1) {
    if (!skip_fields(t, q, le, gti)) return false;
    a0 = allele(t, q, le);
    if (a0 == -2 || q >= le || (t[q] != '/' && t[q] != '|')) return false;
    q++;
    a1 = allele(t, q, le);
    return a1 != -2 && field_end(t, q, le);
}

// an unsigned number of at most `max_digits` digits at q; -1: not one
VGL_HD int small_uint(const uint8_t* t, int64_t& q, const int64_t le, const int max_digits) {
    int v = 0, n = 0;
    while (q < le && t[q] >= '0' && t[q] <= '9') { if (++n > max_digits) return -1; v = v * 10 + (t[q++] - '0'); }
    return n ? v : -1;
}

// the tool's walk over the PL values of one sample, a value at a time: v < 0 is a missing value
struct PlWalk {
    int second = MAX_PL; bool zero = false;
    VGL_HD void add(const int v) {
        if (v < 0) { zero = true; second = MAX_PL; }
        else if (v == 0) zero = true;
        else if (v < second) second = v;
    }
    VGL_HD int gq() const { return second > MAX_GQ ? MAX_GQ : second; }
};

// GQ of the column at q by the PL rule; false: not plain (a value count other than nG, another token, no zero found)
VGL_HD bool pl_gq(const uint8_t* t, int64_t q, const int64_t le, const int pli, const int nG, int& gq) {
    if (!skip_fields(t, q, le, pli)) return false;
    PlWalk w;
    for (int g = 0; g < nG; g++) {
        if (g) { if (q >= le || t[q] != ',') return false; q++; }
        if (q < le && t[q] == '.') { q++; w.add(-1); continue; }
        const int v = small_uint(t, q, le, 4);
        if (v < 0) return false;
        w.add(v);
    }
    if (!field_end(t, q, le) || !w.zero) return false;
    gq = w.gq();
    return gq >= 1;
}

// the truth column at q -> the byte b0 | b1 << 4 of its bases; false: not plain
VGL_HD bool sample_true(const uint8_t* t, const int64_t q, const int64_t le, const Rec& r, uint32_t& tb) {
    int a0, a1;
    if (!gt_token(t, q, le, r.t_gti, a0, a1) || a0 < 0 || a1 < 0) return false;
    const int lim = r.t_nal < 16 ? r.t_nal : 16;
    if (a0 >= lim || a1 >= lim) return false;
    const uint32_t b0 = map_nibble(r.t_map, a0), b1 = map_nibble(r.t_map, a1);
    tb = b0 | b1 << 4;
    return b0 < 4u && b1 < 4u;
}

// the call column at q -> the byte of its bases (CALL_MISSING for a missing call) and its GQ; false: not plain
VGL_HD bool sample_call(const uint8_t* t, const int64_t q, const int64_t le, const Rec& r, uint32_t& cb, uint32_t& gq) {
    int a0, a1, g = 0;
    cb = CALL_MISSING; gq = 0;
    if (!gt_token(t, q, le, r.c_gti, a0, a1)) return false;
    if (r.gq_mode == GQ_PL && r.c_nal > 1) { if (!pl_gq(t, q, le, r.c_pli, r.nG, g)) return false; }      // (every sample: see above)
    else if (r.gq_mode == GQ_PL || r.gq_mode == GQ_MAX) g = MAX_GQ;
    if (a0 < 0 || a1 < 0) return true;
    const int lim = r.c_nal < 16 ? r.c_nal : 16;
    if (a0 >= lim || a1 >= lim) return false;
    const uint32_t b0 = map_nibble(r.c_map, a0), b1 = map_nibble(r.c_map, a1);
    if (b0 > 3u || b1 > 3u) return false;
    if (r.gq_mode == GQ_TAG) {
        int64_t p = q;
        if (!skip_fields(t, p, le, r.c_gqi)) return false;
        g = small_uint(t, p, le, 3);
        if (g < 1 || g > MAX_GQ || !field_end(t, p, le)) return false;
    }
    cb = b0 | b1 << 4; gq = (uint32_t)g;
    return true;
}

VGL_HD uint32_t classify(const uint32_t tb, const uint32_t cb) {
    const uint32_t t0 = tb & 15u, t1 = tb >> 4, c0 = cb & 15u, c1 = cb >> 4;
    const bool thom = t0 == t1, chom = c0 == c1;
    if (thom && chom) return t0 == c0 ? 0u : 1u;
    if (!thom && !chom) return ((t0 == c0 && t1 == c1) || (t0 == c1 && t1 == c0)) ? 2u : 3u;
    return thom ? 4u : 5u;
}
VGL_HD uint32_t dc_type(const uint32_t cell) { return (cell == 0u || cell == 2u) ? 0u : 1u; }                   // T_CONCORDANT 0, T_DISCORDANT 1
VGL_HD uint32_t call_type(const uint32_t cell) { return cell < 2u ? 1u : cell < 4u ? 2u : cell == 4u ? 3u : 4u; }   // HOM_TO_HOM .. HET_TO_HOM

// byte sink of one line: W = false counts only; W = true stores, never at or past `lim`
template <bool W>
struct Emit {
    uint8_t* p;
    uint32_t n, lim;
    VGL_HD void put(const char c) { if (W && n < lim) p[n] = (uint8_t)c; n++; }
    VGL_HD void num(uint64_t v) {
        char d[20]; int k = 0;
        do { d[k++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (k) put(d[--k]);
    }
};

// the listing line of one compared call (-doGQ 1 / 2)
template <bool W>
VGL_HD void list_line(Emit<W>& e, const int list, const int32_t nsites1, const uint32_t i, const uint32_t cell, const uint32_t gq) {
    e.num((uint64_t)(uint32_t)nsites1); e.put('\t'); e.num(i); e.put('\t'); e.put((char)('0' + dc_type(cell))); e.put('\t');
    if (list == LIST_GQ_TYPE) { e.put((char)('0' + call_type(cell))); e.put('\t'); }
    e.num(gq); e.put('\n');
}
// the -perSite 1 line of one compared call
template <bool W>
VGL_HD void site_line(Emit<W>& e, const int64_t pos, const uint32_t i, const uint32_t cell) {
    e.num((uint64_t)pos); e.put('\t'); e.num(i); e.put('\t'); e.put((char)('0' + dc_type(cell))); e.put('\t');
    e.put((char)('0' + call_type(cell))); e.put('\n');
}
VGL_HD uint32_t list_len(const int list, const int32_t nsites1, const uint32_t i, const uint32_t cell, const uint32_t gq) {
    Emit<false> e{nullptr, 0u, 0u}; list_line(e, list, nsites1, i, cell, gq); return e.n;
}
VGL_HD uint32_t site_len(const int64_t pos, const uint32_t i, const uint32_t cell) {
    Emit<false> e{nullptr, 0u, 0u}; site_line(e, pos, i, cell); return e.n;
}

// One record by the plain grammar, a column at a time: what k_gtd_parse does with a lane per column.  tb / cb / gq: N bytes each;
// t_text / c_text: what Rec::t_off and Rec::c_off count from (the device has both regions in one text).
// Returns ST_OK, or ST_HOST (the planes are then unspecified).
// side_plain: one of its two regions (side 0 the truth's into tb, side 1 the call's into cb / gq).
inline int side_plain(const uint8_t* text, const int side, const Rec& r, const int64_t N, uint8_t* tb, uint8_t* cb, uint8_t* gq) {
    const int64_t lb = side ? r.c_off : r.t_off, le = lb + (side ? r.c_len : r.t_len);
    int64_t col = 0, q = lb;
    for (;;) {
        if (col < N) {
            uint32_t b, g;
            if (side == 0) { if (!sample_true(text, q, le, r, b)) return ST_HOST; tb[col] = (uint8_t)b; }
            else { if (!sample_call(text, q, le, r, b, g)) return ST_HOST; cb[col] = (uint8_t)b; gq[col] = (uint8_t)g; }
        }
        col++;
        while (q < le && text[q] != '\t') q++;
        if (q >= le) break;
        q++;
    }
    return col == N ? ST_OK : ST_HOST;
}
inline int record_plain(const uint8_t* t_text, const uint8_t* c_text, const Rec& r, const int64_t N, uint8_t* tb, uint8_t* cb, uint8_t* gq) {
    if (side_plain(t_text, 0, r, N, tb, cb, gq) != ST_OK) return ST_HOST;
    return side_plain(c_text, 1, r, N, tb, cb, gq);
}

}  // namespace gtd
#endif
