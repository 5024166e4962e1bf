// rf_core.h -- the rules of the resident record file (resident_file.hip: a BGZF file of VCF text inflated into device memory and left
// there) as code that compiles for the host and for the device: the kernels, the host model below (split_model) and a host program
// under the sanitizers (tests/rf_core_main.cpp) all run these routines.
//
// The text is taken in chunks of RF_CHUNK bytes, chunk k = bytes [k RF_CHUNK, (k + 1) RF_CHUNK), a lane's piece = RF_LANE of them.
//   line      line i is [begin, end): begin = 0 for i = 0, else one past the '\n' that ends line i - 1; end = the place of its '\n', or
//             `total` for a last line without one.  A text that ends in '\n' has no line behind it.
//   head      of an empty line: nothing.  Of a line that begins with '#': the line.  Of any other line: [begin, one past the ninth tab),
//             or the line when it has fewer than nine tabs.  What lies behind the head are the line's sample columns.
//   over      the walk for the ninth tab reads at most head_most bytes of a line; a longer line whose ninth tab was not among them
//             cannot be classified (`over`: the whole file is then read the other way)
//   stream    the heads back to back in line order, a '\n' behind each
// No routine reads a byte outside [0, total).
#ifndef RF_CORE_H
#define RF_CORE_H
#include <stdint.h>
#include <string.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif

namespace rf {

constexpr int RF_LANE = 16;                       // bytes a lane takes of a chunk
constexpr int RF_NT = 256;                        // lanes of a workgroup of the chunk kernels
constexpr int64_t RF_CHUNK = (int64_t)RF_NT * RF_LANE;
constexpr int64_t RF_HEAD_MOST = 1 << 20;

// the bytes [o, o + RF_LANE) that lie inside [0, hi) as four words, little end first; a byte outside is 0.  Sixteen bytes inside on
// a 16-byte address are one load.
VGL_HD void load_piece(const uint8_t* text, const int64_t o, const int64_t hi, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (o >= 0 && o + RF_LANE <= hi && (((uintptr_t)(text + o)) & (uintptr_t)(RF_LANE - 1)) == 0) {
        __builtin_memcpy(w, __builtin_assume_aligned(text + o, RF_LANE), RF_LANE);
        return;
    }
    for (int i = 0; i < RF_LANE; i++) { const int64_t at = o + i; if (at >= 0 && at < hi) w[i >> 2] |= (uint32_t)text[at] << (8 * (i & 3)); }
}

// bit i: byte i of the piece is '\n'
VGL_HD uint32_t newline_mask(const uint32_t w[4]) {
    uint32_t m = 0;
    for (int i = 0; i < RF_LANE; i++) m |= (((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == (uint32_t)'\n' ? 1u : 0u) << i;
    return m;
}

VGL_HD int popcount16(uint32_t m) { int n = 0; for (; m; m &= m - 1) n++; return n; }

// where line i begins, from the ends of the lines before it
VGL_HD int64_t line_begin(const int64_t* ends, const int64_t i) { return i == 0 ? 0 : ends[i - 1] + 1; }

struct Head { int64_t head_len, s_off, s_len; bool over; };

// the head of the line [begin, end) and the span of its sample columns
VGL_HD Head classify(const uint8_t* text, const int64_t begin, const int64_t end, const int64_t head_most) {
    Head h; h.head_len = end - begin; h.s_off = end; h.s_len = 0; h.over = false;
    if (end <= begin || text[begin] == (uint8_t)'#') return h;
    const int64_t stop = end - begin > head_most ? begin + head_most : end;
    int tabs = 0;
    for (int64_t q = begin; q < stop; q++)
        if (text[q] == (uint8_t)'\t' && ++tabs == 9) { h.head_len = q + 1 - begin; h.s_off = q + 1; h.s_len = end - (q + 1); return h; }
    h.over = stop < end;
    return h;
}

}  // namespace rf

// ---- the host model of the four passes (count, ends, head lengths, head copy) ---------------------------------------------------
#include <vector>

namespace rf {

struct Split {
    int64_t lines = 0;
    bool over = false;
    std::vector<int64_t> ends;                    // [lines]
    std::vector<int64_t> hoff;                    // [lines + 1] where line i's head begins in `heads`
    std::vector<int64_t> s_off, s_len;            // [lines] the sample columns of line i
    std::vector<uint8_t> heads;
};

// the passes as the kernels make them, at any chunk size (the kernels': RF_CHUNK)
inline void split_model(const uint8_t* text, const int64_t total, const int64_t chunk, const int64_t head_most, Split& out) {
    out = Split();
    const int64_t n_chunks = (total + chunk - 1) / chunk;
    // pass 1: '\n' per chunk, piece by piece; then the first line ordinal of every chunk
    std::vector<int64_t> first((size_t)n_chunks + 1, 0);
    auto pieces = [&](int64_t c, auto f) {
        const int64_t c0 = c * chunk, c1 = c0 + chunk < total ? c0 + chunk : total;
        for (int64_t o = c0; o < c1; o += RF_LANE) { uint32_t w[4]; load_piece(text, o, c1, w); f(o, newline_mask(w)); }
    };
    for (int64_t c = 0; c < n_chunks; c++) { int64_t n = 0; pieces(c, [&](int64_t, uint32_t m) { n += popcount16(m); }); first[(size_t)c + 1] = first[(size_t)c] + n; }
    const int64_t n_nl = first[(size_t)n_chunks];
    // pass 2: the place of every '\n' in order; a last line without one ends at total
    out.ends.assign((size_t)n_nl + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        int64_t at = first[(size_t)c];
        pieces(c, [&](int64_t o, uint32_t m) { for (int i = 0; i < RF_LANE; i++) if (m >> i & 1) out.ends[(size_t)at++] = o + i; });
    }
    out.ends[(size_t)n_nl] = total;
    out.lines = n_nl + ((total > 0 && text[total - 1] != (uint8_t)'\n') ? 1 : 0);
    out.ends.resize((size_t)out.lines);
    // pass 3: a line at a time
    const size_t L = (size_t)out.lines;
    out.hoff.assign(L + 1, 0); out.s_off.assign(L, 0); out.s_len.assign(L, 0);
    std::vector<int64_t> hl(L);
    for (size_t i = 0; i < L; i++) {
        const Head h = classify(text, line_begin(out.ends.data(), (int64_t)i), out.ends[i], head_most);
        hl[i] = h.head_len; out.s_off[i] = h.s_off; out.s_len[i] = h.s_len; out.over |= h.over;
    }
    for (size_t i = 0; i < L; i++) out.hoff[i + 1] = out.hoff[i] + hl[i] + 1;
    // pass 4: the heads, a '\n' behind each
    out.heads.assign((size_t)out.hoff[L], (uint8_t)'\n');
    for (size_t i = 0; i < L; i++) if (hl[i] > 0) memcpy(out.heads.data() + out.hoff[i], text + line_begin(out.ends.data(), (int64_t)i), (size_t)hl[i]);
}

}  // namespace rf
#endif
