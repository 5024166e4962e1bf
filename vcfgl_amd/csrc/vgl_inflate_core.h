// vgl_inflate_core.h -- the decoder of vgl_inflate.hip (k_inflate_member) and the member walk of vgl_bgzf_index, as code that
// compiles for the host and for the device: the bit reader, the table build, the symbol loop and every bound check.  The kernel adds
// staging, the write-out and the CRC32; a host program around this header (tests/test_inflate_core_cpu.py) runs the same decoder
// under the host sanitizers.  zlib's inflate is the specification of what is accepted:
//   * any number of blocks until BFINAL; BTYPE 00 (LEN / NLEN checked, LEN 0 allowed), 01, 10; BTYPE 11 is refused
//   * HLIT <= 286 and HDIST <= 30; the code-length code must be complete; repeats 16 / 17 / 18, 16 needs a previous length, a run
//     may not cross the end of the lengths; the literal/length code needs an end-of-block code
//   * a literal/length or distance code may be incomplete only when its longest code has one bit (zlib's inflate_table: the block
//     without any distance code, and the single distance code of one bit); an oversubscribed code is refused; an unused bit
//     pattern met in the data is refused
//   * literal/length symbols 286 / 287 and distance symbols 30 / 31 are refused where they occur
//   * a distance beyond the bytes produced, output beyond `isize`, input running out: refused at the first violation
//   * at BFINAL's end the output must be exactly `isize` bytes and the data must end in the input's last byte
// Bounds: no byte outside in[0, in_len) is read and no byte outside win[0, isize) is written, whatever the input holds.
// Lanes: every lane of the caller's group (one wavefront on the device, the single host thread) runs the whole decode on the same
// values, so that control flow is uniform; stores of literals are lane 0's, and the bytes of a match or of a stored block are dealt
// to the lanes.  Byte i of a match of distance d at position p is win[p - d + i % d]: every source lies before p, so the lanes copy
// independently, overlapping matches (d < length) included.  VGL_INFLATE_SYNC() makes earlier stores of the group visible to it.
#ifndef VGL_INFLATE_CORE_H
#define VGL_INFLATE_CORE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define VGL_INFLATE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define VGL_INFLATE_SYNC() do { } while (0)
#endif

enum { VGL_INF_FAST_LL = 10, VGL_INF_FAST_D = 9 };     // bits of the direct tables; longer codes are walked canonically

// decode tables of one block (4 KiB: in LDS on the device)
struct vgl_inflate_tabs {
    uint16_t fast_ll[1 << VGL_INF_FAST_LL];             // symbol << 4 | length over the next bits; 0: a longer code, or none
    uint16_t fast_d[1 << VGL_INF_FAST_D];               // (first the code-length code's table, then the distance code's)
    uint16_t cnt_ll[16], cnt_d[16];                     // codes per length
    uint16_t sym_ll[288], sym_d[32];                    // symbols in canonical order
    uint8_t lens[320];                                  // code lengths read from a dynamic block's header
};

struct vgl_inflate_bits {
    const uint8_t* in; int32_t in_len, pos; uint64_t acc; int32_t n;
};

// at least 33 bits in the accumulator while the input lasts (never a byte at or beyond in_len)
VGL_HD void vgl_inf_refill(vgl_inflate_bits& b) {
    if (b.n > 32) return;
    if (b.pos + 4 <= b.in_len) {
        uint32_t v; memcpy(&v, b.in + b.pos, 4);        // (little endian hosts and devices only)
        b.acc |= (uint64_t)v << b.n; b.n += 32; b.pos += 4;
    } else {
        while (b.pos < b.in_len && b.n <= 56) { b.acc |= (uint64_t)b.in[b.pos++] << b.n; b.n += 8; }
    }
}
// k <= 16 bits; false when the input has run out
VGL_HD bool vgl_inf_get(vgl_inflate_bits& b, const int k, uint32_t& v) {
    vgl_inf_refill(b);
    if (b.n < k) return false;
    v = (uint32_t)(b.acc & ((1u << k) - 1u)); b.acc >>= k; b.n -= k;
    return true;
}

// canonical code of lens[0, n): counts, symbols in order and the direct table of fast_bits bits.  strict: the code must be complete
// (the code-length code); otherwise an incomplete code passes when its longest code has at most one bit.  false: refused.
VGL_HD bool vgl_inf_build(const uint8_t* lens, const int n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, const int fast_bits, const bool strict) {
    uint16_t offs[16];
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int s = 0; s < n; s++) cnt[lens[s] & 15]++;
    int left = 1, maxl = 0;
    for (int l = 1; l < 16; l++) {
        left <<= 1; left -= cnt[l];
        if (left < 0) return false;                     // oversubscribed
        if (cnt[l]) maxl = l;
    }
    if (left > 0 && (strict || maxl > 1)) return false; // incomplete
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int s = 0; s < n; s++) { const int l = lens[s] & 15; if (l) sym[offs[l]++] = (uint16_t)s; }
    for (int i = 0; i < (1 << fast_bits); i++) fast[i] = 0;
    // the codes of length <= fast_bits, in canonical order, bit-reversed into the table
    uint32_t code = 0; int idx = 0;
    for (int l = 1; l <= fast_bits && l < 16; l++) {
        for (int k = 0; k < cnt[l]; k++, idx++, code++) {
            uint32_t r = 0;
            for (int j = 0; j < l; j++) r |= ((code >> j) & 1u) << (l - 1 - j);
            const uint16_t e = (uint16_t)(sym[idx] << 4 | l);
            for (uint32_t j = r; j < (1u << fast_bits); j += 1u << l) fast[j] = e;
        }
        code <<= 1;
    }
    cnt[0] = 0;
    return true;
}

// one symbol; -1: an unused bit pattern or the input ran out
VGL_HD int vgl_inf_sym(vgl_inflate_bits& b, const uint16_t* cnt, const uint16_t* sym, const uint16_t* fast, const int fast_bits) {
    const uint32_t e = fast[(uint32_t)b.acc & ((1u << fast_bits) - 1u)];
    if (e) {
        const int l = (int)(e & 15u);
        if (l > b.n) return -1;
        b.acc >>= l; b.n -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    uint64_t a = b.acc;
    for (int l = 1; l < 16; l++) {
        code |= (int)(a & 1u); a >>= 1;
        const int c = cnt[l];
        if (code - c < first) {
            if (l > b.n) return -1;
            b.acc >>= l; b.n -= l;
            return sym[index + (code - first)];
        }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// RFC 1951 3.2.5 / 3.2.7
#if defined(__HIP_DEVICE_COMPILE__)
#define VGL_INF_TABLE static __constant__
#else
#define VGL_INF_TABLE static const
#endif
VGL_INF_TABLE uint16_t vgl_inf_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
VGL_INF_TABLE uint8_t vgl_inf_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
VGL_INF_TABLE uint16_t vgl_inf_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                                6145, 8193, 12289, 16385, 24577};
VGL_INF_TABLE uint8_t vgl_inf_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Inflate in[0, in_len) (raw deflate data) into win[0, isize).  0: every block decoded, exactly isize bytes produced and the data
// ends in the input's last byte.  Nonzero: refused (the number names the check, for the test program's messages).
VGL_HD int vgl_inflate_core(const uint8_t* in, const int32_t in_len, uint8_t* win, const int32_t isize, vgl_inflate_tabs* T, const int lane, const int nlanes) {
    if (in_len < 0 || isize < 0 || isize > 65536) return 1;
    vgl_inflate_bits b{in, in_len, 0, 0, 0};
    int32_t outp = 0;
    for (;;) {
        uint32_t final_, btype;
        if (!vgl_inf_get(b, 1, final_) || !vgl_inf_get(b, 2, btype)) return 2;
        if (btype == 3) return 3;
        if (btype == 0) {
            b.acc >>= b.n & 7; b.n -= b.n & 7;
            uint32_t len, nlen;
            if (!vgl_inf_get(b, 16, len) || !vgl_inf_get(b, 16, nlen)) return 2;
            if ((len ^ nlen) != 0xffffu) return 4;
            b.pos -= b.n >> 3; b.acc = 0; b.n = 0;       // the whole bytes read ahead are the block's first
            if ((int32_t)len > in_len - b.pos) return 2;
            if ((int32_t)len > isize - outp) return 5;
            for (int32_t i = lane; i < (int32_t)len; i += nlanes) win[outp + i] = in[b.pos + i];
            b.pos += (int32_t)len; outp += (int32_t)len;
        } else {
            if (btype == 1) {
                for (int s = 0; s < 288; s++) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (int s = 0; s < 32; s++) T->lens[288 + s] = 5;
                VGL_INFLATE_SYNC();
                if (!vgl_inf_build(T->lens, 288, T->cnt_ll, T->sym_ll, T->fast_ll, VGL_INF_FAST_LL, false)) return 6;
                if (!vgl_inf_build(T->lens + 288, 32, T->cnt_d, T->sym_d, T->fast_d, VGL_INF_FAST_D, false)) return 6;
            } else {
                uint32_t hlit, hdist, hclen, v;
                if (!vgl_inf_get(b, 5, hlit) || !vgl_inf_get(b, 5, hdist) || !vgl_inf_get(b, 4, hclen)) return 2;
                hlit += 257; hdist += 1; hclen += 4;
                if (hlit > 286 || hdist > 30) return 7;
                for (int i = 0; i < 19; i++) T->lens[i] = 0;
                VGL_INFLATE_SYNC();
                for (uint32_t i = 0; i < hclen; i++) { if (!vgl_inf_get(b, 3, v)) return 2; T->lens[vgl_inf_cl_order[i]] = (uint8_t)v; }
                VGL_INFLATE_SYNC();
                if (!vgl_inf_build(T->lens, 19, T->cnt_d, T->sym_d, T->fast_d, 7, true)) return 8;
                VGL_INFLATE_SYNC();
                const int total = (int)(hlit + hdist);
                int i = 0, prev = 0;
                while (i < total) {
                    vgl_inf_refill(b);
                    const int s = vgl_inf_sym(b, T->cnt_d, T->sym_d, T->fast_d, 7);
                    if (s < 0) return 9;
                    if (s < 16) { T->lens[i++] = (uint8_t)s; prev = s; continue; }
                    int rep, val = 0;
                    if (s == 16) { if (i == 0) return 10; if (!vgl_inf_get(b, 2, v)) return 2; rep = 3 + (int)v; val = prev; }
                    else if (s == 17) { if (!vgl_inf_get(b, 3, v)) return 2; rep = 3 + (int)v; }
                    else { if (!vgl_inf_get(b, 7, v)) return 2; rep = 11 + (int)v; }
                    if (i + rep > total) return 11;
                    while (rep-- > 0) T->lens[i++] = (uint8_t)val;
                    prev = val;
                }
                VGL_INFLATE_SYNC();
                if (T->lens[256] == 0) return 12;
                if (!vgl_inf_build(T->lens, (int)hlit, T->cnt_ll, T->sym_ll, T->fast_ll, VGL_INF_FAST_LL, false)) return 13;
                if (!vgl_inf_build(T->lens + hlit, (int)hdist, T->cnt_d, T->sym_d, T->fast_d, VGL_INF_FAST_D, false)) return 14;
            }
            VGL_INFLATE_SYNC();
            for (;;) {
                vgl_inf_refill(b);
                const int s = vgl_inf_sym(b, T->cnt_ll, T->sym_ll, T->fast_ll, VGL_INF_FAST_LL);
                if (s < 0) return 15;
                if (s < 256) {
                    if (outp >= isize) return 5;
                    if (lane == 0) win[outp] = (uint8_t)s;
                    outp++;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return 16;
                uint32_t v = 0;
                const int le = vgl_inf_len_extra[s - 257];
                if (le && !vgl_inf_get(b, le, v)) return 2;
                const int32_t len = (int32_t)vgl_inf_len_base[s - 257] + (int32_t)v;
                vgl_inf_refill(b);
                const int ds = vgl_inf_sym(b, T->cnt_d, T->sym_d, T->fast_d, VGL_INF_FAST_D);
                if (ds < 0) return 17;
                if (ds > 29) return 18;
                const int de = ds < 4 ? 0 : (ds >> 1) - 1;
                v = 0;
                if (de && !vgl_inf_get(b, de, v)) return 2;
                const int32_t dist = (int32_t)vgl_inf_dist_base[ds] + (int32_t)v;
                if (dist > outp) return 19;
                if (len > isize - outp) return 5;
                VGL_INFLATE_SYNC();
                const uint8_t* from = win + (outp - dist);
                if (dist >= len) { for (int32_t i = lane; i < len; i += nlanes) win[outp + i] = from[i]; }
                else { for (int32_t i = lane; i < len; i += nlanes) win[outp + i] = from[i % dist]; }
                outp += len;
            }
        }
        if (final_) break;
    }
    VGL_INFLATE_SYNC();
    if (outp != isize) return 20;
    if (b.pos - (b.n >> 3) != in_len) return 21;
    return 0;
}

// A BGZF member at raw[off, n): its size (BSIZE + 1), where its deflate data begins and its trailer's CRC32 and ISIZE.  false: the
// bytes are not a whole BGZF member (magic 1f 8b 08, FLG 4, a 'BC' subfield of length 2 among the XLEN bytes of extra subfields,
// room for deflate data and the trailer inside BSIZE + 1 <= n - off).  Reads no byte outside raw[off, n).
VGL_HD bool vgl_bgzf_member_at(const uint8_t* raw, const int64_t off, const int64_t n, int32_t& size, int32_t& deflate_at, uint32_t& crc, uint32_t& isize) {
    if (off < 0 || n - off < 12 + 6 + 2 + 8) return false;
    const uint8_t* p = raw + off;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return false;
    const int32_t xlen = p[10] | p[11] << 8;
    if (12 + (int64_t)xlen > n - off) return false;
    int32_t bsize = -1;
    for (int32_t q = 12; q + 4 <= 12 + xlen;) {
        const int32_t sl = p[q + 2] | p[q + 3] << 8;
        if (q + 4 + sl > 12 + xlen) return false;
        if (p[q] == 'B' && p[q + 1] == 'C') { if (sl != 2) return false; bsize = p[q + 4] | p[q + 5] << 8; }
        q += 4 + sl;
    }
    if (bsize < 0) return false;
    size = bsize + 1; deflate_at = 12 + xlen;
    if (size > n - off || size < deflate_at + 2 + 8) return false;
    crc = (uint32_t)p[size - 8] | (uint32_t)p[size - 7] << 8 | (uint32_t)p[size - 6] << 16 | (uint32_t)p[size - 5] << 24;
    isize = (uint32_t)p[size - 4] | (uint32_t)p[size - 3] << 8 | (uint32_t)p[size - 2] << 16 | (uint32_t)p[size - 1] << 24;
    return true;
}

// the members of raw[0, n): 0 and *n_members when the buffer is a clean series of BGZF members with ISIZE <= 65536 (written to the
// arrays while they last: max_members), -1 when it is not
VGL_HD int vgl_bgzf_index_core(const uint8_t* raw, const int64_t n, const int64_t max_members, int64_t* begin, int32_t* csize, int32_t* isize, int64_t* n_members) {
    int64_t off = 0, m = 0;
    if (n <= 0) return -1;
    while (off < n) {
        int32_t size, at; uint32_t crc, is;
        if (!vgl_bgzf_member_at(raw, off, n, size, at, crc, is) || is > 65536u) return -1;
        if (m < max_members) { begin[m] = off; csize[m] = size; isize[m] = (int32_t)is; }
        m++; off += size;
    }
    *n_members = m;
    return 0;
}
#endif /* VGL_INFLATE_CORE_H */
