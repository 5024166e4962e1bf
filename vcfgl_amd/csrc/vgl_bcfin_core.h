// vgl_bcfin_core.h -- the per-sample rule of vgl_bcfin.hip (k_bcfin_decode) as code that compiles for the host and for the device; the
// host program's --dump-gt FILE SOURCE 3 and a host program around this header (tests/test_bcfin_core_cpu.py, under the host
// sanitizers) run it on the CPU.  The host program's read_bcf + make_site are the specification.
//   value        a BCF2 typed integer of w = 1, 2 or 4 bytes, little endian, sign-extended; the int8 / int16 sentinels become the int32
//                ones (missing INT32_MIN, end-of-vector INT32_MIN + 1), as BcfIn::ints does.  Assembled from single bytes: a record's
//                FORMAT block starts at any address
//   per sample   v0, v1 = its first two of n values (v1 = end-of-vector when n == 1); later values do not matter.
//                a0 = -1 if v0 is end-of-vector, else (v0 >> 1) - 1;  a1 = -1 if v0 is end-of-vector, a0 if v1 is, else (v1 >> 1) - 1
//                byte = (b1 << 4) | b0, b = allele_map[a] & 0xF, 0xF for a == -1;  sum = the non-negative a added up
//   plain        v0 -- and v1 where it is used: n >= 2 and v0 is not end-of-vector -- is end-of-vector or an ordinary value >= 0 whose
//                allele index is below n_alleles.  Anything else (the missing sentinel, another negative value, an index >= n_alleles
//                -- which covers every value whose (int8_t) wrap the host relies on) makes the RECORD the caller's: VGL_BCFIN_HOST
//   record       plain needs an integer GT type (1, 2, 3), n >= 1 and n_alleles in 1 .. 5 (allele_map has five entries)
// The five map entries travel as one word of six nibbles, indexed by a + 1.  Plain C++ only.
#ifndef VGL_BCFIN_CORE_H
#define VGL_BCFIN_CORE_H
#include <stdint.h>
#include <string.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif

namespace vgl_bcfin {

enum { ST_OK = 0, ST_HOST = 1 };                                     // VGL_BCFIN_OK, VGL_BCFIN_HOST
enum : int32_t { V_MISSING = INT32_MIN, V_END = INT32_MIN + 1 };
enum { OCT = 8 };                                                    // samples of one step of the int8 diploid path: 16 bytes in, 8 out

// bytes of a value of BCF type `type`; 0: not an integer type
VGL_HD int width(const int type) { return type == 1 ? 1 : type == 2 ? 2 : type == 3 ? 4 : 0; }

VGL_HD int32_t value8(const uint32_t b) { const int32_t x = (int32_t)(b & 0xFFu) - (int32_t)((b & 0x80u) << 1); return x == -128 ? V_MISSING : x == -127 ? V_END : x; }

VGL_HD int32_t value(const uint8_t* p, const int w) {
    if (w == 1) return value8(p[0]);
    if (w == 2) {
        const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
        const int32_t x = (int32_t)u - (int32_t)((u & 0x8000u) << 1);
        return x == -32768 ? V_MISSING : x == -32767 ? V_END : x;
    }
    const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    int32_t x; memcpy(&x, &u, 4);
    return x;
}

// nibble a + 1 of the word: 0xF for a == -1, allele_map[a] & 0xF for a = 0 .. 4
VGL_HD uint32_t map_word(const int8_t* allele_map) {
    uint32_t m = 0xFu;
    for (int a = 0; a < 5; a++) m |= ((uint32_t)allele_map[a] & 0xFu) << (4 * (a + 1));
    return m;
}

// does the slice of a record with an integer type and n >= 1 lie inside the bytes?  (w = 0 or n < 1: nothing is read, nothing to check)
VGL_HD bool slice_ok(const int64_t begin, const int w, const int32_t n, const int64_t N, const int64_t gt_bytes) {
    if (w == 0 || n < 1) return true;
    if (begin < 0 || begin > gt_bytes) return false;
    return (gt_bytes - begin) / (N * w) >= (int64_t)n;                 // (N * w <= 2^33: no overflow, whatever n is)
}

// can a record of this GT type, n values per sample and n_alleles be plain at all?
VGL_HD bool describable(const int type, const int n, const int n_alleles) { return width(type) != 0 && n >= 1 && n_alleles >= 1 && n_alleles <= 5; }

// one sample from its first two values; false = not plain (byte and sum are then 0xFF and 0)
VGL_HD bool pair(const int32_t v0, const int32_t v1, const int n_alleles, const uint32_t map, uint32_t& byte, int& sum) {
    int a0 = -1, a1 = -1;
    bool plain = true;
    if (v0 != V_END) {
        if (v0 < 0) plain = false;
        else {
            a0 = (v0 >> 1) - 1;
            if (v1 == V_END) a1 = a0;
            else if (v1 < 0) plain = false;
            else a1 = (v1 >> 1) - 1;
        }
    }
    if (a0 >= n_alleles || a1 >= n_alleles) plain = false;
    if (!plain) { byte = 0xFFu; sum = 0; return false; }
    byte = ((map >> (4 * (a0 + 1))) & 0xFu) | (((map >> (4 * (a1 + 1))) & 0xFu) << 4);
    sum = (a0 > 0 ? a0 : 0) + (a1 > 0 ? a1 : 0);
    return true;
}

// one sample at p: n values of w bytes
VGL_HD bool sample(const uint8_t* p, const int w, const int n, const int n_alleles, const uint32_t map, uint32_t& byte, int& sum) {
    const int32_t v0 = value(p, w);
    const int32_t v1 = n >= 2 ? value(p + w, w) : (int32_t)V_END;
    return pair(v0, v1, n_alleles, map, byte, sum);
}

// eight int8 diploid samples: their 16 bytes as four little-endian words in, their 8 packed bytes as two words out; the sum is
// added to, false = one of them is not plain
VGL_HD bool oct8(const uint32_t in[4], const int n_alleles, const uint32_t map, uint32_t out[2], int& sum) {
    bool plain = true;
    out[0] = out[1] = 0;
    for (int k = 0; k < OCT; k++) {
        const uint32_t h = in[k >> 1] >> (16 * (k & 1));
        uint32_t b; int s;
        plain &= pair(value8(h), value8(h >> 8), n_alleles, map, b, s);
        out[k >> 2] |= b << (8 * (k & 3));
        sum += s;
    }
    return plain;
}

// A whole record on one thread, in the steps the kernel takes: slice = n_samples * n * width(type) bytes, row = n_samples bytes.
// Reads and writes exactly those.  Returns the status; row and *allelesum are unspecified for ST_HOST
VGL_HD int record(const uint8_t* slice, const int type, const int n, const int n_alleles, const int8_t* allele_map, const int64_t n_samples,
                  uint8_t* row, int32_t* allelesum) {
    *allelesum = 0;
    if (!describable(type, n, n_alleles)) return ST_HOST;
    const int w = width(type);
    const uint32_t map = map_word(allele_map);
    int sum = 0; bool plain = true;
    int64_t s = 0;
    if (w == 1 && n == 2)
        for (; s + OCT <= n_samples; s += OCT) {
            uint32_t in[4], out[2];
            memcpy(in, slice + 2 * s, 16);
            plain &= oct8(in, n_alleles, map, out, sum);
            memcpy(row + s, out, 8);
        }
    const int64_t stride = (int64_t)n * w;
    for (; s < n_samples; s++) {
        uint32_t b; int t;
        plain &= sample(slice + s * stride, w, n, n_alleles, map, b, t);
        row[s] = (uint8_t)b; sum += t;
    }
    *allelesum = sum;
    return plain ? ST_OK : ST_HOST;
}

}  // namespace vgl_bcfin
#endif
