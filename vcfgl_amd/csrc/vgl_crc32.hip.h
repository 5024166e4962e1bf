// vgl_crc32.hip.h -- CRC32 (reflected, polynomial 0xEDB88320) in slices: what the BGZF compressor (vgl_bgzf.hip) and the inflater
// (vgl_inflate.hip) share.  A buffer is cut into slices aligned to its END (the slice that holds byte 0 starts from 0xffffffff, the
// others from 0), every slice's register is computed on its own, and neighbours are combined pairwise: crc(A B) = F^|B|(crc(A)) ^
// crc(B), F^n = the GF(2) operator of n zero bytes shifted through the register.  The operators F^(64 * 2^k bytes), k = 0..9, are
// computed at compile time; every translation unit that uses them defines its own __constant__ copy:
//     __constant__ CrcShifts c_crc_shift = make_crc_shifts();
#pragma once
#include <stdint.h>

namespace {

struct Gf2 { uint32_t m[32]; };
constexpr uint32_t gf2_apply(const Gf2& a, uint32_t v) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) if ((v >> i) & 1u) r ^= a.m[i];
    return r;
}
constexpr Gf2 gf2_square(const Gf2& a) {
    Gf2 r{};
    for (int i = 0; i < 32; ++i) r.m[i] = gf2_apply(a, a.m[i]);
    return r;
}
struct CrcShifts { Gf2 s[10]; };
constexpr CrcShifts make_crc_shifts() {
    Gf2 a{};
    a.m[0] = 0xEDB88320u;                                         // one zero bit shifted through the register
    for (int i = 1; i < 32; ++i) a.m[i] = 1u << (i - 1);
    for (int k = 0; k < 9; ++k) a = gf2_square(a);                // 2^9 bits = 64 bytes
    CrcShifts r{};
    for (int k = 0; k < 10; ++k) { r.s[k] = a; a = gf2_square(a); }
    return r;
}
// one step of the register over 4 bytes (little endian word) or 1 byte
__device__ __forceinline__ uint32_t crc32_word(uint32_t r, const uint32_t w) {
    r ^= w;
    for (int k = 0; k < 32; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
    return r;
}
__device__ __forceinline__ uint32_t crc32_byte(uint32_t r, const uint32_t b) {
    r ^= b;
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
    return r;
}

}  // namespace
