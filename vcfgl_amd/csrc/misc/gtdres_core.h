// gtdres_core.h -- gtdiscordance_hip --resident 1: sixteen bytes from any address of a side's buffer, as code that compiles for the
// host and for the device (k_gtd_bcf_decode of gtdisc.hip and tests/gtdres_core_main.cpp run this routine).  A resident file holds a
// record's GT vector where the inflater wrote it, at any byte; a lane that takes eight int8 GT pairs at once loads the two aligned
// 16-byte pieces around them and joins the pieces by a byte shift.  A piece is loaded only when all of it lies inside [0, n_bytes) of
// the side: no byte outside the buffer is read, and a lane whose pieces do not lie inside reads its samples a value at a time.
#ifndef GTDRES_CORE_H
#define GTDRES_CORE_H
#include <stdint.h>

#ifndef VGL_HD
#if defined(__HIPCC__)
#define VGL_HD __host__ __device__ inline
#else
#define VGL_HD inline
#endif
#endif

namespace gtd {

// w = the bytes [o, o + 16) of `bytes` as four words, little end first.  mis = how far bytes + o lies behind a 16-byte address: 0 is
// one load; otherwise the pieces [o - mis, + 16) and [o - mis + 16, + 16) are loaded and joined.  false (w untouched): a piece the
// join needs does not lie whole inside [0, n_bytes).
VGL_HD bool load16_any(const uint8_t* bytes, const int64_t o, const int64_t n_bytes, uint32_t w[4]) {
    const int mis = (int)((uintptr_t)(bytes + o) & 15u);
    const int64_t lo = o - mis;
    if (lo < 0 || lo + 16 > n_bytes) return false;
    uint64_t a[2];
    __builtin_memcpy(a, __builtin_assume_aligned(bytes + lo, 16), 16);
    if (mis == 0) { w[0] = (uint32_t)a[0]; w[1] = (uint32_t)(a[0] >> 32); w[2] = (uint32_t)a[1]; w[3] = (uint32_t)(a[1] >> 32); return true; }
    if (lo + 32 > n_bytes) return false;
    uint64_t b[2];
    __builtin_memcpy(b, __builtin_assume_aligned(bytes + lo + 16, 16), 16);
    // the three 64-bit words that hold the bytes (selects: no register is indexed), then a shift of 0 .. 56 bits
    const bool up = mis >= 8;
    const uint64_t q0 = up ? a[1] : a[0], q1 = up ? b[0] : a[1], q2 = up ? b[1] : b[0];
    const int sh = 8 * (mis & 7);
    const uint64_t lo64 = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0, hi64 = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
    w[0] = (uint32_t)lo64; w[1] = (uint32_t)(lo64 >> 32); w[2] = (uint32_t)hi64; w[3] = (uint32_t)(hi64 >> 32);
    return true;
}

}  // namespace gtd
#endif
