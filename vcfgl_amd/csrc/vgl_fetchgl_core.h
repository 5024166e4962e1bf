// vgl_fetchgl_core.h -- the per-value formatter of vgl_fetchgl.hip (k_fetchgl_plan, k_fetchgl_write) as code that compiles for the
// host and for the device; a host program around this header (tests/test_fetchgl_core_cpu.py) runs it under the host sanitizers.
// What misc/fetchGl prints for one FORMAT/GL value:
//   bits 0x7F800001 -> "MISSING", bits 0x7F800002 -> "END", otherwise glibc's %f: the exact binary value correctly rounded to six
//   decimals, ties to even, the sign first ("-0.000000" for a negative value that rounds to zero), "inf" / "-inf".
// Two value modes, because the tool prints the float of the file it reads:
//   VGL_FETCHGL_FLOAT (0)  the float as simulated (a BCF holds it); another NaN prints "nan" / "-nan" by its sign
//   VGL_FETCHGL_TEXT  (1)  the float a VCF text file gives back: first the text the writers give it (vgl_text.hip fmt_float: "." for the
//                          missing pattern, "nan" for every other NaN -- the END pattern included --, kputd's 6 digits in
//                          [1e-4, 999999], %g's outside), then htslib's way back: the nearest double of that text, then the nearest float.
//                          "." prints "MISSING" and NaN "nan".  The text is q 10^k with q < 10^6: the nearest double is one correctly
//                          rounded multiplication or division of q by 10^|k| (exact in a double up to 10^22).  Below 10^-17 only
//                          the sign survives %f; from 1e21 on the simulated float is printed as VGL_FETCHGL_FLOAT does.
// %f in integers: a float is m 2^e with m < 2^24.  For e < 0 the integer part is m >> -e and the fraction's six decimals are
// (f 10^6) >> -e with f < 2^24 (64 bits hold the product; from -e = 64 on the decimals are 0), rounded by the remainder against half;
// a fraction that rounds up to 1000000 carries into the integer part.  For e >= 0 the value is an integer: 32 bits while it fits, the
// multi-word path (fg_big, up to 39 digits) beyond.
// The 6-digit routines (fg_kputd_digits, fg_g_digits, fg_scaled, fg_big) are those of vgl_text.hip's fmt_float, host and device.
#ifndef VGL_FETCHGL_CORE_H
#define VGL_FETCHGL_CORE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif
#if defined(__clang__)
#define VGL_FG_UNROLL _Pragma("unroll")
#else
#define VGL_FG_UNROLL
#endif

namespace vgl_fetchgl {

enum { MODE_FLOAT = 0, MODE_TEXT = 1 };
enum : uint32_t { MISSING_BITS = 0x7F800001u, END_BITS = 0x7F800002u };
enum { MAX_VALUE_LEN = 47 };                                    // "-" + the 39 digits of FLT_MAX + ".000000"

// byte sink of one value: W = false counts only; W = true stores, never at or past `lim`
template <bool W>
struct Emit {
    uint8_t* p;
    uint32_t n, lim;
    VGL_HD void put(char c) { if (W && n < lim) p[n] = (uint8_t)c; n++; }
    VGL_HD void put_at(uint32_t at, char c) { if (W && at < lim) p[at] = (uint8_t)c; }
};

VGL_HD int fg_ndig32(uint32_t u) {
    int n = 1;
    if (u >= 10u) n = 2;
    if (u >= 100u) n = 3;
    if (u >= 1000u) n = 4;
    if (u >= 10000u) n = 5;
    if (u >= 100000u) n = 6;
    if (u >= 1000000u) n = 7;
    if (u >= 10000000u) n = 8;
    if (u >= 100000000u) n = 9;
    if (u >= 1000000000u) n = 10;
    return n;
}

// ---- exact 256-bit unsigned integers (8 x 32-bit limbs, little endian; every index a constant after unrolling) ------------------
struct fg_big { uint32_t w[8]; };

VGL_HD void fg_mul_small(fg_big& a, uint32_t c) {
    uint64_t carry = 0;
VGL_FG_UNROLL
    for (int j = 0; j < 8; ++j) { const uint64_t t = (uint64_t)a.w[j] * c + carry; a.w[j] = (uint32_t)t; carry = t >> 32; }
}
VGL_HD void fg_mul_pow10(fg_big& a, int p) {
    for (; p >= 9; p -= 9) fg_mul_small(a, 1000000000u);
    uint32_t m = 1; for (int r = 0; r < p; ++r) m *= 10u;
    fg_mul_small(a, m);
}
VGL_HD void fg_mul_pow5(fg_big& a, int p) {
    for (; p >= 13; p -= 13) fg_mul_small(a, 1220703125u);
    uint32_t m = 1; for (int r = 0; r < p; ++r) m *= 5u;
    fg_mul_small(a, m);
}
VGL_HD uint32_t fg_div10(fg_big& a) {                         // a /= 10, returns the remainder
    uint64_t rem = 0;
VGL_FG_UNROLL
    for (int j = 7; j >= 0; --j) { const uint64_t cur = (rem << 32) | a.w[j]; a.w[j] = (uint32_t)(cur / 10u); rem = cur % 10u; }
    return (uint32_t)rem;
}
VGL_HD void fg_shl(fg_big& a, int s) {
    for (; s >= 32; s -= 32) {
VGL_FG_UNROLL
        for (int j = 7; j > 0; --j) a.w[j] = a.w[j - 1];
        a.w[0] = 0;
    }
    if (s > 0) {
VGL_FG_UNROLL
        for (int j = 7; j > 0; --j) a.w[j] = (a.w[j] << s) | (a.w[j - 1] >> (32 - s));
        a.w[0] <<= s;
    }
}
// a >>= s; returns whether a nonzero bit was shifted out
VGL_HD bool fg_shr_sticky(fg_big& a, int s) {
    bool sticky = false;
    for (; s >= 32; s -= 32) {
        sticky |= a.w[0] != 0;
VGL_FG_UNROLL
        for (int j = 0; j < 7; ++j) a.w[j] = a.w[j + 1];
        a.w[7] = 0;
    }
    if (s > 0) {
        sticky |= (a.w[0] & ((1u << s) - 1u)) != 0;
VGL_FG_UNROLL
        for (int j = 0; j < 7; ++j) a.w[j] = (a.w[j] >> s) | (a.w[j + 1] << (32 - s));
        a.w[7] >>= s;
    }
    return sticky;
}
VGL_HD uint32_t fg_low_or_huge(const fg_big& a) {             // the value when it fits 32 bits, else 0xffffffff
    uint32_t hi = 0;
VGL_FG_UNROLL
    for (int j = 1; j < 8; ++j) hi |= a.w[j];
    return hi ? 0xffffffffu : a.w[0];
}
VGL_HD bool fg_is_zero(const fg_big& a) {
    uint32_t any = 0;
VGL_FG_UNROLL
    for (int j = 0; j < 8; ++j) any |= a.w[j];
    return any == 0;
}

enum { FG_BELOW = 0, FG_HALF = 1, FG_ABOVE = 2 };

// floor(m 2^e / 10^k) (0xffffffff when it does not fit 32 bits) and where the remainder lies against half a unit
VGL_HD void fg_scaled(uint32_t m, int e, int k, uint32_t& fl, int& cls) {
    fg_big a;
VGL_FG_UNROLL
    for (int j = 0; j < 8; ++j) a.w[j] = 0;
    a.w[0] = m;
    if (k < 0) {                                            // m 10^-k / 2^-e
        fg_mul_pow10(a, -k);
        int sh = -e;
        if (sh <= 0) { fg_shl(a, -sh); fl = fg_low_or_huge(a); cls = FG_BELOW; return; }
        const bool sticky = fg_shr_sticky(a, sh - 1);       // one bit more than the quotient: the half bit
        const uint32_t half = a.w[0] & 1u;
        fg_shr_sticky(a, 1);
        fl = fg_low_or_huge(a);
        cls = half ? (sticky ? FG_ABOVE : FG_HALF) : FG_BELOW;
        return;
    }
    int t = k;                                               // m 2^e = a / 10^t with a an integer
    if (e >= 0) fg_shl(a, e);
    else { fg_mul_pow5(a, -e); t = k - e; }
    bool sticky = false;
    uint32_t last = 0;
    for (int r = 0; r < t; ++r) { if (r) sticky |= last != 0; last = fg_div10(a); }
    fl = fg_low_or_huge(a);
    cls = (last > 5u || (last == 5u && sticky)) ? FG_ABOVE : (last == 5u ? FG_HALF : FG_BELOW);
}

// the 6 significant digits q (100000 .. 999999) and decimal exponent X (value ~ q 10^(X - 5)) of %g for a finite positive float
VGL_HD void fg_g_digits(uint32_t a, double d, uint32_t& q, int& X) {
    const uint32_t ef = a >> 23, fr = a & 0x7fffffu;
    const uint32_t m = ef ? (fr | 0x800000u) : fr;
    const int e = ef ? (int)ef - 150 : -149;
    int E = (int)floor(log10(d));
    uint32_t fl = 0; int cls = FG_BELOW;
    for (int it = 0; it < 6; ++it) {                        // the estimate is off by at most one near powers of ten
        fg_scaled(m, e, E - 5, fl, cls);
        if (fl >= 1000000u) { E++; continue; }
        if (fl < 100000u) { E--; continue; }
        break;
    }
    q = fl + ((cls == FG_ABOVE || (cls == FG_HALF && (fl & 1u))) ? 1u : 0u);
    if (q == 1000000u) { q = 100000u; E++; }
    X = E;
}

// kputd: (uint64_t)(d * 1e10) plus half a unit of the 6th significant digit (one double multiply: nothing to contract)
VGL_HD void fg_kputd_digits(double d, uint32_t& q, int& X) {
    uint64_t i = (uint64_t)(d * 10000000000.0);
    if (d < 0.001) i += 5; else if (d < 0.01) i += 50; else if (d < 0.1) i += 500;
    else if (d < 1) i += 5000; else if (d < 10) i += 50000; else if (d < 100) i += 500000; else if (d < 1000) i += 5000000;
    else if (d < 10000) i += 50000000; else if (d < 100000) i += 500000000; else i += 5000000000ULL;
    int n = 1;
    for (uint64_t p = 10; n < 20 && i >= p; p *= 10) n++;   // decimal digits of i (7 .. 16 here)
    for (int j = n; j > 6; --j) i /= 10u;
    q = (uint32_t)i;
    X = n - 11;
}

VGL_HD double fg_pow10(int k) {                              // exact for k <= 22
    double p = 1.0;
    for (int j = 0; j < k; ++j) p *= 10.0;
    return p;
}

// VGL_FETCHGL_TEXT: the bits of the float that the 6-digit text of a finite, nonzero value reads back as
VGL_HD uint32_t fg_text_roundtrip(uint32_t bits) {
    const uint32_t a = bits & 0x7fffffffu;
    float af; memcpy(&af, &a, 4);
    const double d = (double)af;
    if (d >= 1e21) return bits;
    uint32_t q; int X;
    if (d >= 0.0001 && d <= 999999) fg_kputd_digits(d, q, X);
    else fg_g_digits(a, d, q, X);
    const int k = X - 5;                                     // the text's value is q 10^k
    double r;
    if (k >= 0) r = (double)q * fg_pow10(k);                 // (k <= 16 below 1e21)
    else if (k >= -22) r = (double)q / fg_pow10(-k);         // IEEE division: this translation unit is never built with fast-math
    else r = 0.0;
    const float f = (float)r;
    uint32_t fb; memcpy(&fb, &f, 4);
    return (bits & 0x80000000u) | fb;
}

// an integer m 2^e of more than 32 bits (e <= 104: at most 39 digits) and ".000000"
template <bool W>
VGL_HD void fg_fmt_huge(Emit<W>& e, uint32_t m, int ex) {
    fg_big a;
VGL_FG_UNROLL
    for (int j = 0; j < 8; ++j) a.w[j] = 0;
    a.w[0] = m;
    fg_shl(a, ex);
    fg_big c = a;
    uint32_t L = 0;
    while (!fg_is_zero(c)) { fg_div10(c); L++; }
    if (W) for (uint32_t j = 0; j < L; ++j) e.put_at(e.n + L - 1u - j, (char)('0' + fg_div10(a)));
    e.n += L;
    e.put('.');
    for (int j = 0; j < 6; ++j) e.put('0');
}

// glibc's %f of a float that is not a NaN
template <bool W>
VGL_HD void fg_fmt_f(Emit<W>& e, uint32_t bits) {
    if (bits >> 31) e.put('-');
    const uint32_t a = bits & 0x7fffffffu;
    if (a == 0x7f800000u) { e.put('i'); e.put('n'); e.put('f'); return; }
    const uint32_t ef = a >> 23, fr = a & 0x7fffffu;
    const uint32_t m = ef ? (fr | 0x800000u) : fr;
    const int ex = ef ? (int)ef - 150 : -149;
    uint32_t ip, q = 0;
    if (ex > 8) { fg_fmt_huge(e, m, ex); return; }           // 2^32 and beyond
    if (ex >= 0) ip = m << ex;
    else {
        const int s = -ex;
        ip = s < 24 ? m >> s : 0u;
        if (s < 64) {
            const uint64_t f = s < 24 ? (uint64_t)(m & ((1u << s) - 1u)) : (uint64_t)m;
            const uint64_t p = f * 1000000ull, half = 1ull << (s - 1), rem = p & ((1ull << s) - 1ull);
            q = (uint32_t)(p >> s);
            if (rem > half || (rem == half && (q & 1u))) q++;
            if (q == 1000000u) { q = 0; ip++; }
        }
    }
    const uint32_t L = (uint32_t)fg_ndig32(ip);
    if (W) { uint32_t x = ip; for (uint32_t j = 0; j < L; ++j) { e.put_at(e.n + L - 1u - j, (char)('0' + x % 10u)); x /= 10u; } }
    e.n += L;
    e.put('.');
    if (W) { uint32_t x = q; for (uint32_t j = 0; j < 6u; ++j) { e.put_at(e.n + 5u - j, (char)('0' + x % 10u)); x /= 10u; } }
    e.n += 6u;
}

template <bool W>
VGL_HD void fg_word(Emit<W>& e, const char* s) { for (; *s; ++s) e.put(*s); }

// one FORMAT/GL value as misc/fetchGl prints it
template <bool W>
VGL_HD void fmt_value(Emit<W>& e, uint32_t bits, int mode) {
    if (bits == MISSING_BITS) { fg_word(e, "MISSING"); return; }
    const uint32_t a = bits & 0x7fffffffu;
    if (mode == MODE_FLOAT) {
        if (bits == END_BITS) { fg_word(e, "END"); return; }
        if (a > 0x7f800000u) { if (bits >> 31) e.put('-'); fg_word(e, "nan"); return; }
    } else {
        if (a > 0x7f800000u) { fg_word(e, "nan"); return; }
        if (a != 0u && a != 0x7f800000u) bits = fg_text_roundtrip(bits);
    }
    fg_fmt_f(e, bits);
}

// the genotype's index at a site, or -1: a2b = the site's alleles2acgt (0 .. 4 = A, C, G, T, unobserved), nA its allele count; the
// last allele that matches wins, as in the tool's loop
VGL_HD int genotype_index(const int8_t* a2b, int nA, int a, int b) {
    int j0 = -1, j1 = -1;
    nA = nA < 0 ? 0 : (nA > 5 ? 5 : nA);
    for (int j = 0; j < nA; ++j) { if (a2b[j] == a) j0 = j; if (a2b[j] == b) j1 = j; }
    if (j0 < 0 || j1 < 0) return -1;
    const int hi = j0 > j1 ? j0 : j1, lo = j0 > j1 ? j1 : j0;
    return hi * (hi + 1) / 2 + lo;
}

}  // namespace vgl_fetchgl
#endif
