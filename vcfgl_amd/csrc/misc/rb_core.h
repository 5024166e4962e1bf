// rb_core.h -- the rules of the resident BCF file (resident_file.hip: a BGZF file of BCF inflated into device memory and left there)
// as code that compiles for the host and for the device: the kernels, the host model below (walk_model) and a host program under the
// sanitizers (tests/rb_core_main.cpp) all run these routines.  Every routine takes (bytes, total) and reads nothing outside [0, total).
//   record     from offset o: l_shared and l_indiv (8 bytes inside the file), l_shared >= 24, rec_end = o + 8 + l_shared + l_indiv <=
//              total in 64 bits -- the rule of bcf_scan_record, and 24 because the six fixed words of the shared block are read
//              unasked.  The chain of records ends cleanly only at o == total.  Every record is at least RB_REC_LEAST bytes.
//   typed      a descriptor byte: type = low four bits, n = high four; n == 15 is followed by ONE typed integer scalar (a byte with
//              n = 1 and type 1 .. 3, then the value, which must be >= 0) -- the rule of BcfIn::typed for what htslib writes (fifteen
//              GLs are 0xF5 0x11 0x0F); any other continuation is not known here
//   shared     the shared block must read to exactly its length by the walk bcf_shared makes (ID and alleles: strings; FILTER: nothing
//              or integers; INFO: an integer key and a value of type 0, 1 .. 3, 5 or 7), so that bcf_shared, given the block alone,
//              reads no byte behind it
//   FORMAT     n_fmt and n_sample from the last fixed word; n_sample must be N; per field a key (a typed integer vector of type 1 .. 3,
//              n >= 1), a descriptor, and bcf_type_width(type) * n * N bytes (64 bits) of data that end at or before rec_end
//   head       of a record: its 8 length bytes, its shared block, and the key and descriptor bytes of every field, back to back
// What the walk is not sure of -- a width of 0, a descriptor it does not know, a field past rec_end, another n_sample, a shared block
// longer than head_most or one that does not read to its length -- has a reason (Why) and makes the caller hand the whole file back to
// the host reader.  Stricter than the host is safe; laxer is not.
#ifndef RB_CORE_H
#define RB_CORE_H
#include <stdint.h>
#include <string.h>
#include "rf_core.h"

namespace rb {

constexpr int RB_WIN_LANES = 64;                                 // the chain's wavefront: a lane loads RF_LANE bytes of the window
constexpr int64_t RB_WINDOW = (int64_t)RB_WIN_LANES * rf::RF_LANE;
constexpr int64_t RB_WINDOW_LEAST = 2 * rf::RF_LANE;             // (8 length bytes at any place of a 16-byte piece)
constexpr int64_t RB_HOPS_MOST = 1 << 20;                        // records a chain launch takes
constexpr int64_t RB_REC_LEAST = 32;

enum Why : int32_t {
    OK = 0,
    W_LENGTHS,                         // the two lengths do not lie inside the file
    W_SHARED_SHORT,                    // l_shared < 24
    W_PAST_END,                        // the record ends behind the file
    W_HEAD_MOST,                       // the shared block is longer than head_most
    W_N_SAMPLE,                        // n_sample is not the header's sample count
    W_SHARED,                          // the shared block does not read to its length
    W_DESCRIPTOR,                      // a descriptor the walk does not know (or one cut off by rec_end)
    W_KEY,                             // a FORMAT key that is not an integer vector of at least one value
    W_WIDTH,                           // a FORMAT type without a width
    W_FIELD_PAST,                      // a field's key or data run past rec_end
    W_COUNT
};
inline const char* why_text(const int w) {
    static const char* const T[W_COUNT] = {"nothing", "a record's lengths lie outside the file", "a shared block shorter than 24 bytes", "a record that ends behind the file",
                                           "a shared block longer than the head bound", "a sample count other than the header's", "a shared block that does not read to its length",
                                           "a typed descriptor outside the walk's rules", "a FORMAT key that is not an integer vector", "a FORMAT type without a width",
                                           "a FORMAT field that runs past its record"};
    return w >= 0 && w < W_COUNT ? T[w] : "an unknown reason";
}

VGL_HD uint32_t rd_u32(const uint8_t* b, const int64_t o) {
    return (uint32_t)b[o] | (uint32_t)b[o + 1] << 8 | (uint32_t)b[o + 2] << 16 | (uint32_t)b[o + 3] << 24;
}
// bytes of one value (bcf_type_width of record_file.h)
VGL_HD int type_width(const int ty) { return ty == 1 ? 1 : ty == 2 ? 2 : (ty == 3 || ty == 5) ? 4 : ty == 7 ? 1 : 0; }
VGL_HD int int_width(const int ty) { return ty == 1 ? 1 : ty == 2 ? 2 : ty == 3 ? 4 : 0; }
// the integer of width w at o, sign-extended (the bytes lie inside the file: the caller has compared)
VGL_HD int32_t rd_int(const uint8_t* b, const int64_t o, const int w) {
    if (w == 1) return (int32_t)(int8_t)b[o];
    if (w == 2) return (int32_t)(int16_t)((uint32_t)b[o] | (uint32_t)b[o + 1] << 8);
    return (int32_t)rd_u32(b, o);
}

// the rule of a record step on lengths already read
VGL_HD int step_rule(const int64_t o, const int64_t total, const uint32_t l_shared, const uint32_t l_indiv, int64_t& rec_end) {
    rec_end = o;
    if (l_shared < 24u) return W_SHARED_SHORT;
    const int64_t e = o + 8 + (int64_t)l_shared + (int64_t)l_indiv;
    if (e > total) return W_PAST_END;
    rec_end = e;
    return OK;
}
// a record step from offset o of the file (0 <= o < total)
VGL_HD int record_step(const uint8_t* bytes, const int64_t total, const int64_t o, uint32_t& l_shared, int64_t& rec_end) {
    rec_end = o; l_shared = 0;
    if (o < 0 || o + 8 > total) return W_LENGTHS;
    l_shared = rd_u32(bytes, o);
    return step_rule(o, total, l_shared, rd_u32(bytes, o + 4), rec_end);
}

struct Typed { int32_t type; int64_t n; int32_t len; bool ok; };       // len: the descriptor's own bytes (1, or 2 + the scalar's width)
// the typed descriptor at o, read inside [.., hi) (hi <= total)
VGL_HD Typed typed_at(const uint8_t* bytes, const int64_t o, const int64_t hi) {
    Typed t; t.type = 0; t.n = 0; t.len = 0; t.ok = false;
    if (o < 0 || o >= hi) return t;
    const uint8_t b = bytes[o];
    t.type = b & 15; t.n = b >> 4; t.len = 1;
    if (t.n < 15) { t.ok = true; return t; }
    if (o + 1 >= hi) return t;
    const uint8_t b2 = bytes[o + 1];
    const int w = int_width(b2 & 15);
    if ((b2 >> 4) != 1 || w == 0 || o + 2 + w > hi) return t;
    const int32_t v = rd_int(bytes, o + 2, w);
    if (v < 0) return t;
    t.n = v; t.len = 2 + w; t.ok = true;
    return t;
}

// the shared block [sb, se) behind its six fixed words reads to exactly se by the walk of bcf_shared
VGL_HD bool shared_reads_whole(const uint8_t* bytes, const int64_t sb, const int64_t se, const uint32_t n_allele, const uint32_t n_info) {
    int64_t p = sb + 24;
    // ID and the alleles: strings
    for (uint32_t i = 0; i <= n_allele; i++) {
        const Typed t = typed_at(bytes, p, se);
        if (!t.ok || t.type != 7 || t.n > se - (p + t.len)) return false;
        p += t.len + t.n;
    }
    {   // FILTER: nothing, or integers
        const Typed t = typed_at(bytes, p, se);
        if (!t.ok) return false;
        p += t.len;
        if (!(t.type == 0 || t.n == 0)) {
            const int w = int_width(t.type);
            if (w == 0 || t.n > (se - p) / w) return false;
            p += t.n * w;
        }
    }
    for (uint32_t i = 0; i < n_info; i++) {
        const Typed k = typed_at(bytes, p, se);
        const int kw = int_width(k.type);
        if (!k.ok || kw == 0 || k.n < 1 || k.n > (se - (p + k.len)) / kw) return false;
        p += k.len + k.n * kw;
        const Typed v = typed_at(bytes, p, se);
        if (!v.ok) return false;
        p += v.len;
        if (v.type == 0 || v.n == 0) continue;
        const int w = v.type == 7 ? 1 : v.type == 5 ? 4 : int_width(v.type);
        if (w == 0 || v.n > (se - p) / w) return false;
        p += v.n * w;
    }
    return p == se;
}

// The fields alone: n_fmt fields from byte p of a record that ends at rec_end.  f(k, hdr_at, hdr_len, key, type, n, data_off) for field
// k, whose key and descriptor are the hdr_len bytes from hdr_at and whose N vectors of n values lie from data_off; hdr = the header
// bytes of all fields.  Returns a Why; f has then been called for the fields before the one that failed.
template <class F>
VGL_HD int fields_walk(const uint8_t* bytes, int64_t p, const int64_t rec_end, const int n_fmt, const int64_t N, int64_t& hdr, F f) {
    hdr = 0;
    for (int k = 0; k < n_fmt; k++) {
        const Typed key = typed_at(bytes, p, rec_end);
        if (!key.ok) return W_DESCRIPTOR;
        const int kw = int_width(key.type);
        if (kw == 0 || key.n < 1) return W_KEY;
        if (key.n > (rec_end - (p + key.len)) / kw) return W_FIELD_PAST;
        const int32_t kv = rd_int(bytes, p + key.len, kw);
        const int64_t q = p + key.len + key.n * kw;
        const Typed d = typed_at(bytes, q, rec_end);
        if (!d.ok) return W_DESCRIPTOR;
        const int w = type_width(d.type);
        if (w == 0) return W_WIDTH;
        const int64_t data = q + d.len;
        const int64_t len = (int64_t)w * d.n * N;                       // < 2^2 2^31 2^24
        if (len > rec_end - data) return W_FIELD_PAST;
        f(k, p, data - p, kv, d.type, d.n, data);
        hdr += data - p;
        p = data + len;
    }
    return OK;
}

// what a record's fixed part says of its fields, by the checks of format_walk up to the shared block's own walk
struct Lead { int64_t rec_end, se; uint32_t l_shared, nai; int n_fmt; };
VGL_HD int record_lead(const uint8_t* bytes, const int64_t total, const int64_t o, const int64_t N, const int64_t head_most, Lead& L) {
    const int st = record_step(bytes, total, o, L.l_shared, L.rec_end);
    if (st != OK) return st;
    if ((int64_t)L.l_shared > head_most) return W_HEAD_MOST;
    const int64_t sb = o + 8;
    L.se = sb + (int64_t)L.l_shared;
    L.nai = rd_u32(bytes, sb + 16);
    const uint32_t nfs = rd_u32(bytes, sb + 20);
    L.n_fmt = (int)(nfs >> 24);                                        // <= 255
    if ((int64_t)(nfs & 0xFFFFFFu) != N) return W_N_SAMPLE;
    return OK;
}

// The FORMAT walk of the record at o: every check above, then the fields.  head_len = 8 + l_shared + the fields' header bytes.
template <class F>
VGL_HD int format_walk(const uint8_t* bytes, const int64_t total, const int64_t o, const int64_t N, const int64_t head_most, int64_t& head_len, F f) {
    head_len = 0;
    Lead L;
    int st = record_lead(bytes, total, o, N, head_most, L);
    if (st != OK) return st;
    if (!shared_reads_whole(bytes, o + 8, L.se, L.nai >> 16, L.nai & 0xFFFFu)) return W_SHARED;
    int64_t hdr;
    st = fields_walk(bytes, L.se, L.rec_end, L.n_fmt, N, hdr, f);
    if (st != OK) return st;
    head_len = 8 + (int64_t)L.l_shared + hdr;
    return OK;
}

// the four bytes at byte a of the file as one word, little end first, for any a with 0 <= a and a + 4 <= total: one aligned load, or
// the two aligned words around a put together; where the second word would reach past total (or the buffer is not word-aligned) the
// bytes are read one by one.  No word that reaches past total is touched.
VGL_HD uint32_t load_u32_any(const uint8_t* bytes, const int64_t a, const int64_t total) {
    const unsigned k = (unsigned)(((uintptr_t)(bytes + a)) & 3u);
    if (k == 0) { uint32_t v; __builtin_memcpy(&v, __builtin_assume_aligned(bytes + a, 4), 4); return v; }
    const int64_t lo = a - k;
    if (lo < 0 || lo + 8 > total) return rd_u32(bytes, a);
    uint32_t w[2];
    __builtin_memcpy(w, __builtin_assume_aligned(bytes + lo, 4), 8);
    return (w[0] >> (8 * k)) | (w[1] << (32 - 8 * k));
}

// the two lengths of the record at byte `rel` of a window held as words (little end first): three aligned words put together.
// rel + 8 <= the window's bytes, so the third word is read only where it lies inside
VGL_HD void win_lengths(const uint32_t* win, const int64_t rel, uint32_t& l_shared, uint32_t& l_indiv) {
    const int64_t i = rel >> 2; const unsigned k = (unsigned)(rel & 3);
    const uint32_t w0 = win[i], w1 = win[i + 1];
    if (k == 0) { l_shared = w0; l_indiv = w1; return; }
    const uint32_t w2 = win[i + 2];
    l_shared = (w0 >> (8 * k)) | (w1 << (32 - 8 * k));
    l_indiv = (w1 >> (8 * k)) | (w2 << (32 - 8 * k));
}

// a flag of a pass: the lowest ordinal that raised it wins, whatever order the lanes come in
VGL_HD unsigned long long flag_word(const int64_t ordinal, const int why) { return ((unsigned long long)ordinal << 8) | (unsigned long long)(why & 0xFF); }
constexpr unsigned long long FLAG_NONE = ~0ull;

}  // namespace rb

// ---- the host model of the passes (chain launches, head lengths, head copy) -------------------------------------------------------
#include <vector>

namespace rb {

struct Field { int32_t key, type; int64_t n, data_off; };

struct Walk {
    int64_t records = 0, launches = 0;
    int why = OK; int64_t ordinal = -1;           // flagged: why != OK, at record `ordinal` (0-based)
    std::vector<int64_t> rec_off;                 // [records] where every record begins in the file
    std::vector<int64_t> hoff;                    // [records + 1] where record i's head begins in `heads`
    std::vector<uint8_t> heads;
    std::vector<int64_t> field_first;             // [records + 1] record i's fields are fields[field_first[i] .. field_first[i + 1])
    std::vector<Field> fields;
    bool flagged() const { return why != OK; }
};

struct ChainEnd { int64_t next = 0, taken = 0; int32_t done = 0, why = OK; };

// one launch of the chain as the kernel makes it: at most hops_most records from o0, the lengths read from a window of `window`
// bytes that begins on a 16-byte offset and is loaded again only when the next record's lengths lie outside it
inline ChainEnd chain_launch_model(const uint8_t* bytes, const int64_t total, const int64_t o0, const int64_t hops_most, const int64_t window, std::vector<int64_t>& offs) {
    ChainEnd e;
    std::vector<uint32_t> win((size_t)window / 4);
    int64_t o = o0, wb = -1;
    while (e.taken < hops_most) {
        if (o == total) { e.done = 1; break; }
        if (o + 8 > total) { e.why = W_LENGTHS; break; }
        if (wb < 0 || o < wb || o + 8 > wb + window) {
            wb = o & ~(int64_t)(rf::RF_LANE - 1);
            for (int64_t j = 0; j < window; j += rf::RF_LANE) { uint32_t w[4]; rf::load_piece(bytes, wb + j, total, w); memcpy(win.data() + j / 4, w, rf::RF_LANE); }
        }
        int64_t rec_end; uint32_t l_shared, l_indiv;
        win_lengths(win.data(), o - wb, l_shared, l_indiv);
        e.why = step_rule(o, total, l_shared, l_indiv, rec_end);
        if (e.why != OK) break;
        offs.push_back(o); e.taken++;
        o = rec_end;
    }
    e.next = o;
    return e;
}

// the passes from the first record's offset `start` (behind the header), N samples
inline void walk_model(const uint8_t* bytes, const int64_t total, const int64_t start, const int64_t N, const int64_t hops_most, const int64_t window,
                       const int64_t head_most, Walk& out) {
    out = Walk();
    // the chain, launch by launch
    for (int64_t o = start;;) {
        const ChainEnd e = chain_launch_model(bytes, total, o, hops_most, window, out.rec_off);
        out.launches++;
        if (e.why != OK) { out.why = e.why; out.ordinal = (int64_t)out.rec_off.size(); out.records = out.ordinal; return; }
        if (e.done) break;
        o = e.next;
    }
    const size_t R = out.rec_off.size();
    out.records = (int64_t)R;
    // the head lengths, a record at a time; the lowest ordinal that hands back is the flag
    std::vector<int64_t> hl(R);
    unsigned long long flag = FLAG_NONE;
    for (size_t i = 0; i < R; i++) {
        const int st = format_walk(bytes, total, out.rec_off[i], N, head_most, hl[i], [](int, int64_t, int64_t, int32_t, int32_t, int64_t, int64_t) {});
        if (st != OK) { const unsigned long long w = flag_word((int64_t)i, st); if (w < flag) flag = w; hl[i] = 0; }
    }
    if (flag != FLAG_NONE) { out.why = (int)(flag & 0xFF); out.ordinal = (int64_t)(flag >> 8); return; }
    out.hoff.assign(R + 1, 0);
    for (size_t i = 0; i < R; i++) out.hoff[i + 1] = out.hoff[i] + hl[i];
    // the heads: the lengths and the shared block, then the fields' headers by walking again
    out.heads.assign((size_t)out.hoff[R], 0);
    out.field_first.assign(R + 1, 0);
    for (size_t i = 0; i < R; i++) {
        const int64_t o = out.rec_off[i], lead = 8 + (int64_t)rd_u32(bytes, o);
        uint8_t* const h = out.heads.data() + out.hoff[i];
        memcpy(h, bytes + o, (size_t)lead);
        int64_t at = lead, hdr;
        Lead L;
        if (record_lead(bytes, total, o, N, head_most, L) != OK) continue;          // (pass 3 took the record: never so)
        fields_walk(bytes, L.se, L.rec_end, L.n_fmt, N, hdr, [&](int, int64_t hdr_at, int64_t hdr_len, int32_t key, int32_t type, int64_t n, int64_t data_off) {
            memcpy(h + at, bytes + hdr_at, (size_t)hdr_len); at += hdr_len;
            out.fields.push_back(Field{key, type, n, data_off});
        });
        out.field_first[i + 1] = (int64_t)out.fields.size();
    }
}

}  // namespace rb
#endif
