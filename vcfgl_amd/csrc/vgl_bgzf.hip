// vgl_bgzf.hip -- BGZF compression on the device (ABI 7: vgl_bgzf_bound, vgl_bgzf_workspace_bytes, vgl_bgzf_compress_device).
// BGZF (SAMv1 section 4.1) is a series of independent gzip members of at most 64 KiB, each carrying its size in a 'BC' extra field.
// The input is cut into members of exactly 0xff00 bytes (the last one shorter) -- the boundaries the host writer's zlib path uses --
// and every member is compressed by one workgroup with the member staged in LDS:
//   * LZ77 (RFC 1951): a 4096-entry hash table of 3-byte prefixes in LDS, filled 1024 positions per step; a position's candidates are
//     the nearest earlier position of its wavefront with the same hash and the table's entry (the latest earlier position outside
//     the wavefront: the wavefronts of a step read and fill the table in turn), distances <= 32768.  The member is parsed in segments
//     of 512 positions, one lane per segment (a match ends at its segment's end; one-byte lazy evaluation as in zlib): the lanes
//     parse independently, so the parse does not depend on timing.
//   * Huffman: literal/length and distance histograms (LDS atomics: counts do not depend on order), a minimum-redundancy code
//     (Moffat-Katajainen, in place on the sorted frequencies) limited to 15 bits (7 for the code-length code), canonical codes.
//     The member is written as whichever of dynamic (BTYPE 10), fixed (01) and stored (00) is smallest; the stored form bounds
//     every member by 0xff00 + 31 bytes.
//   * bit packing: every segment's bit count, a prefix sum over the segments, then every lane writes its tokens at its offset.
//   * CRC32: 1024 slices of 64 bytes (aligned to the member's end), combined by a tree of GF(2) shift operators.
// The members go to 64 KiB slots of the workspace; a scan of their sizes and a compaction pass make one contiguous stream.
// Output bytes depend on the input bytes only (no floating point, no order-dependent atomics): not on the device, the grid, or
// how a caller splits its input at member boundaries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_crc32.hip.h"

namespace {

constexpr int MEMBER = 0xff00;                  // input bytes per BGZF member
constexpr int SLOT = 65536;                     // workspace bytes per member slot
constexpr int SLOT_DEFLATE = 20;                // deflate data starts at this byte of a slot (word aligned); the gzip header is [2, 20)
constexpr int NT = 1024;                        // threads per member workgroup
constexpr int HASH_BITS = 12;
constexpr int SEG = 512;                        // parse segment per lane
constexpr int MAX_SEGS = (MEMBER + SEG - 1) / SEG;
constexpr int GRID_MAX = 512;                   // resident member workgroups (per-workgroup match scratch in the workspace)
constexpr int64_t MEMBER_OVERHEAD = 18 + 5 + 8; // header + stored block header + trailer

// CRC32: shift operators F^(64 * 2^k bytes), k = 0..9 (vgl_crc32.hip.h)
__constant__ CrcShifts c_crc_shift = make_crc_shifts();
// RFC 1951 3.2.7: order of the code-length code's lengths; the first 16 bytes of every BGZF member (SAMv1 4.1)
__constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__constant__ uint8_t c_gz_header[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};

// ---- deflate symbol helpers --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void len_sym(const int len, int& sym, int& nextra, int& extra) {
    if (len <= 10) { sym = 254 + len; nextra = 0; extra = 0; return; }
    if (len == 258) { sym = 285; nextra = 0; extra = 0; return; }
    const int v = len - 3, hb = 31 - __clz(v), e = hb - 2, idx = (v >> e) & 3;
    sym = 261 + 4 * e + idx; nextra = e; extra = v - ((4 + idx) << e);
}
__device__ __forceinline__ void dist_sym(const int d, int& sym, int& nextra, int& extra) {
    if (d <= 4) { sym = d - 1; nextra = 0; extra = 0; return; }
    const int v = d - 1, hb = 31 - __clz(v);
    sym = 2 * hb + ((v >> (hb - 1)) & 1); nextra = hb - 1; extra = v - ((2 + (sym & 1)) << (hb - 1));
}
__device__ __forceinline__ int len_extra_bits(const int s) { return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0; }
__device__ __forceinline__ int dist_extra_bits(const int s) { return s >= 4 ? (s >> 1) - 1 : 0; }

// ---- LDS layout ----------------------------------------------------------------------------------------------------------------
// region A: the member's bytes (+ 16 zero bytes, so that unaligned 4-byte reads near the end stay inside)
// region B: the hash table while matching; afterwards histograms, codes, CRC slices, segment bit counts and the Huffman scratch
struct Post {
    uint32_t hist_ll[288], hist_d[32];
    uint32_t crc[NT];
    uint32_t seg_bits[MAX_SEGS];
    uint16_t code_ll[288], code_d[32];
    uint8_t  len_ll[288], len_d[32];
    int32_t  huf_sym[288], huf_w[288];               // build_lengths scratch
    uint16_t rle[288 + 32];                          // code-length sequence: symbol | extra << 5
    uint32_t cl_hist[19];
    uint8_t  len_cl[19];
    uint16_t code_cl[19];
    int32_t  n_rle, hlit, hdist, hclen, mode, hdr_bits;
    uint32_t total_bits;
    int32_t  cnt[48];                                // build_lengths / canonical: counts per code length
};
static_assert(sizeof(Post) <= (4u << HASH_BITS), "region B");
struct Smem {
    uint32_t in[(MEMBER + 16) / 4];
    union { int32_t tab[1 << HASH_BITS]; Post p; } b;
};
static_assert(sizeof(Smem) <= 81920, "two member workgroups per CU");

__device__ __forceinline__ uint32_t byte_at(const uint32_t* w, const int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }
__device__ __forceinline__ uint32_t load4(const uint32_t* w, const int i) {           // bytes [i, i + 4), little endian
    const int q = i >> 2, r = i & 3;
    return r ? __builtin_amdgcn_alignbyte(w[q + 1], w[q], r) : w[q];          // (the shift operand counts bytes)
}
__device__ __forceinline__ uint32_t hash3(const uint32_t* w, const int i) {
    return ((load4(w, i) & 0xffffffu) * 2654435761u) >> (32 - HASH_BITS);
}
// length of the common prefix of [p, ...) and [c, ...), c < p, at most lim bytes
__device__ __forceinline__ int match_len(const uint32_t* w, const int c, const int p, const int lim) {
    int k = 0;
    while (k < lim) {
        const uint32_t x = load4(w, c + k) ^ load4(w, p + k);
        if (x) { k += __builtin_ctz(x) >> 3; break; }
        k += 4;
    }
    return k < lim ? k : lim;
}

// code lengths of a minimum-redundancy code for freq[0..n), at most maxbits bits; at least two symbols get a code (a used symbol
// count of 0 or 1 is completed with the first unused symbols: every code is complete, as inflaters expect).  One wavefront.
__device__ __noinline__ void build_lengths(const uint32_t* freq, const int n, const int maxbits, uint8_t* len, int32_t* sym, int32_t* w, int32_t* cnt, const int lane) {
    int used = 0;
    for (int s = 0; s < n; ++s) used += freq[s] != 0;
    int forced0 = -1, forced1 = -1;
    if (used < 2) {
        for (int s = 0; s < n && used + (forced0 >= 0) + (forced1 >= 0) < 2; ++s)
            if (!freq[s]) { if (forced0 < 0) forced0 = s; else forced1 = s; }
    }
    auto wt = [&](const int s) -> uint32_t { return (s == forced0 || s == forced1) ? 1u : freq[s]; };
    // rank sort: ascending weight, ties by symbol
    for (int s = lane; s < n; s += 64) {
        len[s] = 0;
        const uint32_t ws = wt(s);
        if (!ws) continue;
        int r = 0;
        for (int t = 0; t < n; ++t) { const uint32_t wt_ = wt(t); r += wt_ && (wt_ < ws || (wt_ == ws && t < s)); }
        sym[r] = s; w[r] = (int32_t)ws;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane == 0) {
        const int m = used + (forced0 >= 0) + (forced1 >= 0);
        int* A = w;
        // in-place minimum-redundancy code lengths (Moffat & Katajainen 1995) of the ascending weights A[0..m)
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < m - 1; ++next) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, usedn = 0, dpth = 0; root = m - 2; int next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && A[root] == dpth) { usedn++; root--; }
            while (avbl > usedn) { A[next--] = dpth; avbl--; }
            avbl = 2 * usedn; dpth++; usedn = 0;
        }
        // limit to maxbits: count per length (longer ones clamped), then shorten the Kraft sum to exactly 1
        for (int i = 0; i <= maxbits; ++i) cnt[i] = 0;
        for (int i = 0; i < m; ++i) cnt[A[i] > maxbits ? maxbits : A[i]]++;
        uint32_t total = 0;
        for (int i = maxbits; i > 0; --i) total += (uint32_t)cnt[i] << (maxbits - i);
        while (total != (1u << maxbits)) {
            cnt[maxbits]--;
            for (int i = maxbits - 1; i > 0; --i) if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
            total--;
        }
        // longest codes to the rarest symbols
        int j = 0;
        for (int i = maxbits; i > 0; --i) for (int k = cnt[i]; k > 0; --k) len[sym[j++]] = (uint8_t)i;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first output.  One lane.
__device__ __noinline__ void canonical(const uint8_t* len, const int n, uint16_t* code, int32_t* bl) {
    int32_t* next = bl + 16;
    for (int b = 0; b < 16; ++b) bl[b] = 0;
    for (int s = 0; s < n; ++s) bl[len[s]]++;
    bl[0] = 0;
    int c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        if (!l) { code[s] = 0; continue; }
        code[s] = (uint16_t)(__builtin_bitreverse32((uint32_t)next[l]++) >> (32 - l));
    }
}

// LSB-first bit writer into zeroed 32-bit words; every word goes in by atomicOr (neighbouring lanes share their boundary words)
struct BitWriter {
    uint32_t* out; uint64_t acc; int nacc; uint32_t word;
    __device__ BitWriter(uint32_t* o, const uint32_t bit0) : out(o), acc(0), nacc((int)(bit0 & 31)), word(bit0 >> 5) {}
    __device__ __forceinline__ void put(const uint32_t v, const int n) {
        acc |= (uint64_t)v << nacc; nacc += n;
        if (nacc >= 32) { if ((uint32_t)acc) atomicOr(out + word, (uint32_t)acc); word++; acc >>= 32; nacc -= 32; }
    }
    __device__ __forceinline__ void finish() { if (nacc > 0 && (uint32_t)acc) atomicOr(out + word, (uint32_t)acc); }
};

// walk a segment's tokens: fn(p, len, dist) with len = 0 for a literal
template <class F>
__device__ __forceinline__ void walk(const uint32_t* info, const int s0, const int s1, F fn) {
    for (int p = s0; p < s1;) {
        const uint32_t t = info[p];
        const int l = (int)(t & 511u);
        if (l >= 3) { fn(p, l, (int)(t >> 9)); p += l; }
        else { fn(p, 0, 0); p += 1; }
    }
}

__global__ __launch_bounds__(NT) void k_bgzf_member(const uint8_t* __restrict__ src, const int64_t n, const int64_t n_members,
                                                     uint32_t* __restrict__ scratch, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes) {
    __shared__ Smem sm;
    const int t = threadIdx.x, lane = t & 63;
    uint32_t* info = scratch + (size_t)blockIdx.x * MEMBER;           // per position: dist << 9 | len (len set at token starts by the parse)
    Post& P = sm.b.p;
    for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        const int64_t off = m * MEMBER;
        const int len = (int)((n - off) < MEMBER ? (n - off) : MEMBER);
        const uint8_t* in = src + off;
        uint8_t* slot = slots + (size_t)m * SLOT;
        // ---- stage the member in LDS (word loads when the source is 4-byte aligned: off is a multiple of 4)
        const int nw = (len + 3) >> 2;
        if ((((uintptr_t)in) & 3) == 0) {
            for (int i = t; i < nw; i += NT) {
                uint32_t v;
                if (4 * i + 4 <= len) v = *(const uint32_t*)(in + 4 * i);
                else { v = 0; for (int k = 0; 4 * i + k < len; ++k) v |= (uint32_t)in[4 * i + k] << (8 * k); }
                sm.in[i] = v;
            }
        } else {
            for (int i = t; i < nw; i += NT) {
                uint32_t v = 0;
                for (int k = 0; k < 4 && 4 * i + k < len; ++k) v |= (uint32_t)in[4 * i + k] << (8 * k);
                sm.in[i] = v;
            }
        }
        for (int i = nw + t; i < nw + 4; i += NT) sm.in[i] = 0;
        for (int i = t; i < (1 << HASH_BITS); i += NT) sm.b.tab[i] = -1;
        __syncthreads();

        // ---- LZ77 candidates, 1024 positions per step
        for (int base = 0; base < len; base += NT) {
            const int p = base + t;
            const bool hv = p + 2 < len;
            const uint32_t h = hv ? hash3(sm.in, p) : 0xffffffffu - (uint32_t)lane;      // (no position without a hash matches another)
            int wc = -1;                                                                  // nearest earlier lane of this wavefront, same hash
            for (int d = 1; d < 64; ++d) {
                const uint32_t ho = __shfl_up(h, d, 64);
                if (wc < 0 && lane >= d && ho == h) wc = p - d;
                if (__all(wc >= 0 || lane < d || !hv)) break;
            }
            // the table in wavefront order: wavefront w reads the latest position before its own 64, then enters its own (the
            // largest of equal hashes wins: atomicMax), so every position sees the latest earlier one outside its wavefront
            int tc = -1;
            for (int w = 0; w < NT / 64; ++w) {
                if ((t >> 6) == w && hv) { tc = sm.b.tab[h]; atomicMax(&sm.b.tab[h], p); }
                __syncthreads();
            }
            uint32_t best = 0;
            if (hv) {
                const int lim = (len - p) < 32 ? (len - p) : 32;                          // choose on the first 32 bytes, full length in the parse
                const int lw = wc >= 0 ? match_len(sm.in, wc, p, lim) : 0;
                const int lt = (tc >= 0 && p - tc <= 32768) ? match_len(sm.in, tc, p, lim) : 0;
                if (lw >= 3 && lw >= lt) best = (uint32_t)(p - wc) << 9;
                else if (lt >= 3) best = (uint32_t)(p - tc) << 9;
            }
            if (p < len) info[p] = best;
            __syncthreads();
        }

        // ---- parse pass 1 (token lengths into info, histograms) and the CRC slices
        const int nseg = (len + SEG - 1) / SEG;
        for (int i = t; i < 288; i += NT) P.hist_ll[i] = 0;
        if (t < 32) P.hist_d[t] = 0;
        __syncthreads();
        {
            // slice t covers [len - 64 (NT - t), len - 64 (NT - 1 - t)) clipped to the member; the one holding byte 0 starts from 0xffffffff
            int b0 = len - 64 * (NT - t), b1 = len - 64 * (NT - 1 - t);
            uint32_t r = 0;
            if (b1 > 0) {
                if (b0 <= 0) { b0 = 0; r = 0xffffffffu; }
                int i = b0;
                for (; i + 4 <= b1; i += 4) {
                    r ^= load4(sm.in, i);
                    for (int k = 0; k < 32; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
                }
                for (; i < b1; ++i) {
                    r ^= byte_at(sm.in, i);
                    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
                }
            }
            P.crc[t] = r;
        }
        if (t < nseg) {
            const int s0 = t * SEG, s1 = (s0 + SEG) < len ? s0 + SEG : len;
            auto len_at = [&](const int q, const uint32_t d) -> int {
                if (!d) return 0;
                const int lim = (s1 - q) < 258 ? (s1 - q) : 258;
                return match_len(sm.in, q - (int)d, q, lim);
            };
            for (int p = s0; p < s1;) {
                const uint32_t d = info[p] >> 9;
                int l = len_at(p, d);
                if (l >= 3 && l < 32 && p + 1 < s1 && len_at(p + 1, info[p + 1] >> 9) > l) l = 0;     // lazy: a longer match one byte on
                if (l >= 3) {
                    info[p] = d << 9 | (uint32_t)l;
                    int s, ne, ex;
                    len_sym(l, s, ne, ex); atomicAdd(&P.hist_ll[s], 1u);
                    dist_sym((int)d, s, ne, ex); atomicAdd(&P.hist_d[s], 1u);
                    p += l;
                } else {
                    info[p] = 0;
                    atomicAdd(&P.hist_ll[byte_at(sm.in, p)], 1u);
                    p += 1;
                }
            }
        }
        for (int k = 0; k < 10; ++k) {                                  // CRC tree: right operands are whole blocks of 64 * 2^k bytes
            __syncthreads();
            if ((t & ((2 << k) - 1)) == 0) P.crc[t] = gf2_apply(c_crc_shift.s[k], P.crc[t]) ^ P.crc[t + (1 << k)];
        }
        __syncthreads();

        // ---- codes (wavefront 0): dynamic, fixed or stored, whichever is smallest
        if (t < 64) {
            if (t == 0) P.hist_ll[256] = 1;                              // end of block
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            build_lengths(P.hist_ll, 286, 15, P.len_ll, P.huf_sym, P.huf_w, P.cnt, lane);
            build_lengths(P.hist_d, 30, 15, P.len_d, P.huf_sym, P.huf_w, P.cnt, lane);
            if (t == 0) {
                P.len_ll[286] = P.len_ll[287] = 0; P.len_d[30] = P.len_d[31] = 0;
                int hlit = 286; while (hlit > 257 && !P.len_ll[hlit - 1]) hlit--;
                int hdist = 30; while (hdist > 1 && !P.len_d[hdist - 1]) hdist--;
                // run-length code of the code lengths (RFC 1951 3.2.7), one sequence over both alphabets
                const int tot = hlit + hdist;
                auto L = [&](const int i) -> int { return i < hlit ? P.len_ll[i] : P.len_d[i - hlit]; };
                for (int i = 0; i < 19; ++i) P.cl_hist[i] = 0;
                int nr = 0;
                for (int i = 0; i < tot;) {
                    const int v = L(i);
                    int run = 1; while (i + run < tot && L(i + run) == v) run++;
                    if (v == 0) {
                        while (run >= 11) { const int r = run < 138 ? run : 138; P.rle[nr++] = (uint16_t)(18 | (r - 11) << 5); P.cl_hist[18]++; run -= r; i += r; }
                        if (run >= 3) { P.rle[nr++] = (uint16_t)(17 | (run - 3) << 5); P.cl_hist[17]++; i += run; run = 0; }
                        for (; run > 0; --run, ++i) { P.rle[nr++] = 0; P.cl_hist[0]++; }
                    } else {
                        P.rle[nr++] = (uint16_t)v; P.cl_hist[v]++; i++; run--;
                        while (run >= 3) { const int r = run < 6 ? run : 6; P.rle[nr++] = (uint16_t)(16 | (r - 3) << 5); P.cl_hist[16]++; run -= r; i += r; }
                        for (; run > 0; --run, ++i) { P.rle[nr++] = (uint16_t)v; P.cl_hist[v]++; }
                    }
                }
                P.n_rle = nr; P.hlit = hlit; P.hdist = hdist;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            build_lengths(P.cl_hist, 19, 7, P.len_cl, P.huf_sym, P.huf_w, P.cnt, lane);
            if (t == 0) {
                int hclen = 19; while (hclen > 4 && !P.len_cl[c_cl_order[hclen - 1]]) hclen--;
                P.hclen = hclen;
                uint64_t hdr = 3 + 5 + 5 + 4 + 3 * hclen, data = 0, fix = 3, data_extra = 0;
                for (int i = 0; i < P.n_rle; ++i) { const int s = P.rle[i] & 31; hdr += P.len_cl[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0); }
                for (int s = 0; s < 286; ++s) {
                    const uint32_t f = P.hist_ll[s];
                    if (!f) continue;
                    data += (uint64_t)f * P.len_ll[s];
                    fix += (uint64_t)f * (s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                    data_extra += (uint64_t)f * len_extra_bits(s);
                }
                for (int s = 0; s < 30; ++s) {
                    const uint32_t f = P.hist_d[s];
                    data += (uint64_t)f * P.len_d[s]; fix += (uint64_t)f * 5; data_extra += (uint64_t)f * dist_extra_bits(s);
                }
                const uint64_t dyn = hdr + data + data_extra;
                fix += data_extra;
                const uint64_t stored = 8 * (uint64_t)(5 + len);
                int mode = 2; uint64_t bits = dyn;
                if (fix < bits) { mode = 1; bits = fix; }
                if (stored < ((bits + 7) & ~7ull)) mode = 0;
                P.mode = mode;
                P.hdr_bits = mode == 2 ? (int)hdr : 3;
                if (mode == 1) {                                        // fixed codes are the canonical code of these lengths
                    for (int s = 0; s < 288; ++s) P.len_ll[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                    for (int s = 0; s < 32; ++s) P.len_d[s] = 5;
                }
                if (mode) {
                    canonical(P.len_ll, 288, P.code_ll, P.cnt);
                    canonical(P.len_d, 32, P.code_d, P.cnt);
                    canonical(P.len_cl, 19, P.code_cl, P.cnt);
                }
            }
        }
        __syncthreads();
        int mode = P.mode;
        if (mode) {
            // ---- parse pass 2: bits per segment, offsets
            if (t < nseg) {
                const int s0 = t * SEG, s1 = (s0 + SEG) < len ? s0 + SEG : len;
                uint32_t b = 0;
                walk(info, s0, s1, [&](const int p, const int l, const int d) {
                    if (l) { int s, ne, ex; len_sym(l, s, ne, ex); b += P.len_ll[s] + ne; dist_sym(d, s, ne, ex); b += P.len_d[s] + ne; }
                    else b += P.len_ll[byte_at(sm.in, p)];
                });
                P.seg_bits[t] = b;
            }
            __syncthreads();
            if (t == 0) {
                uint32_t run = (uint32_t)P.hdr_bits;
                for (int s = 0; s < nseg; ++s) { const uint32_t b = P.seg_bits[s]; P.seg_bits[s] = run; run += b; }
                P.total_bits = run + P.len_ll[256];
                if (((P.total_bits + 7) >> 3) > (uint32_t)(5 + len)) P.mode = 0;    // (never expected: the choice above counted the same bits)
            }
            __syncthreads();
            mode = P.mode;
        }
        uint32_t dbytes;
        if (mode == 0) {
            // stored: 01, LEN, NLEN, the bytes
            uint8_t* d = slot + SLOT_DEFLATE;
            if (t == 0) { d[0] = 1; d[1] = (uint8_t)len; d[2] = (uint8_t)(len >> 8); d[3] = (uint8_t)~len; d[4] = (uint8_t)(~len >> 8); }
            for (int i = t; i < len; i += NT) d[5 + i] = (uint8_t)byte_at(sm.in, i);
            dbytes = 5 + len;
        } else {
            const uint32_t total = P.total_bits;
            dbytes = (total + 7) >> 3;
            uint32_t* ow = (uint32_t*)(slot + SLOT_DEFLATE);
            for (uint32_t i = t; i < (dbytes + 3) / 4; i += NT) ow[i] = 0;
            __threadfence();
            __syncthreads();
            // ---- header (lane 0), then parse pass 3: the tokens
            if (t == 0) {
                BitWriter bw(ow, 0);
                if (mode == 1) bw.put(1 | 1 << 1, 3);
                else {
                    bw.put(1 | 2 << 1, 3); bw.put(P.hlit - 257, 5); bw.put(P.hdist - 1, 5); bw.put(P.hclen - 4, 4);
                    for (int i = 0; i < P.hclen; ++i) bw.put(P.len_cl[c_cl_order[i]], 3);
                    for (int i = 0; i < P.n_rle; ++i) {
                        const int s = P.rle[i] & 31, x = P.rle[i] >> 5;
                        bw.put(P.code_cl[s], P.len_cl[s]);
                        if (s == 16) bw.put(x, 2); else if (s == 17) bw.put(x, 3); else if (s == 18) bw.put(x, 7);
                    }
                }
                bw.finish();
            }
            if (t < nseg) {
                const int s0 = t * SEG, s1 = (s0 + SEG) < len ? s0 + SEG : len;
                BitWriter bw(ow, P.seg_bits[t]);
                walk(info, s0, s1, [&](const int p, const int l, const int d) {
                    if (l) {
                        int s, ne, ex;
                        len_sym(l, s, ne, ex); bw.put(P.code_ll[s], P.len_ll[s]); if (ne) bw.put(ex, ne);
                        dist_sym(d, s, ne, ex); bw.put(P.code_d[s], P.len_d[s]); if (ne) bw.put(ex, ne);
                    } else {
                        const int c = byte_at(sm.in, p);
                        bw.put(P.code_ll[c], P.len_ll[c]);
                    }
                });
                if (t == nseg - 1) bw.put(P.code_ll[256], P.len_ll[256]);
                bw.finish();
            }
        }
        __threadfence();
        __syncthreads();
        if (t == 0) {
            uint8_t* g = slot + SLOT_DEFLATE - 18;
            for (int i = 0; i < 16; ++i) g[i] = c_gz_header[i];
            const uint32_t size = 18 + dbytes + 8, bsize = size - 1;
            g[16] = (uint8_t)bsize; g[17] = (uint8_t)(bsize >> 8);
            const uint32_t crc = P.crc[0] ^ 0xffffffffu;
            uint8_t* tr = slot + SLOT_DEFLATE + dbytes;
            for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(crc >> (8 * i)); tr[4 + i] = (uint8_t)((uint32_t)len >> (8 * i)); }
            sizes[m] = size;
        }
        __syncthreads();                                                // LDS and the scratch are reused by the next member
    }
}

// exclusive prefix sums of the member sizes (one workgroup, chunks of 1024); off[n_members] = the stream's length
__global__ __launch_bounds__(1024) void k_bgzf_scan(const int64_t n_members, const uint32_t* __restrict__ sizes, int64_t* __restrict__ off,
                                                   int64_t* __restrict__ out_n) {
    __shared__ int64_t s_w[16];
    __shared__ int64_t s_carry;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_members; base += 1024) {
        const int64_t i = base + t;
        const int64_t v = i < n_members ? (int64_t)sizes[i] : 0;
        int64_t x = v;
        for (int d = 1; d < 64; d <<= 1) { const int64_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        if (t == 0) { int64_t run = s_carry; for (int k = 0; k < 16; ++k) { const int64_t y = s_w[k]; s_w[k] = run; run += y; } s_carry = run; }
        __syncthreads();
        if (i < n_members) off[i] = s_w[w] + x - v;
        __syncthreads();
    }
    if (t == 0) { off[n_members] = s_carry; if (out_n) *out_n = s_carry; }
}

// the members, slot by slot, into one contiguous stream
__global__ __launch_bounds__(256) void k_bgzf_compact(const int64_t n_members, const uint8_t* __restrict__ slots, const int64_t* __restrict__ off,
                                                      const uint32_t* __restrict__ sizes, uint8_t* __restrict__ dst) {
    for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        const uint8_t* s = slots + (size_t)m * SLOT + SLOT_DEFLATE - 18;
        uint8_t* d = dst + off[m];
        const int size = (int)sizes[m];
        for (int i = threadIdx.x; i < size; i += 256) d[i] = s[i];
    }
}

// workspace: offsets int64 [n_members + 1] | sizes uint32 [n_members] | slots [n_members][64 KiB] | match scratch [grid][0xff00] uint32
struct Layout { int64_t members, grid, off, sizes, slots, scratch, total; };
Layout layout_of(const int64_t n) {
    Layout L;
    auto al = [](const int64_t x) { return (x + 255) & ~(int64_t)255; };
    L.members = (n + MEMBER - 1) / MEMBER;
    L.grid = L.members < GRID_MAX ? L.members : GRID_MAX;
    L.off = 0;
    L.sizes = al(L.off + 8 * (L.members + 1));
    L.slots = al(L.sizes + 4 * L.members);
    L.scratch = L.slots + (int64_t)SLOT * L.members;
    L.total = L.scratch + 4 * (int64_t)MEMBER * L.grid;
    return L;
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_bgzf_bound(int64_t n) {
    if (n < 0) return -1;
    return n + MEMBER_OVERHEAD * ((n + MEMBER - 1) / MEMBER);
}

extern "C" int64_t vgl_bgzf_workspace_bytes(int64_t n) {
    if (n < 0) return -1;
    return n == 0 ? 0 : layout_of(n).total;
}

extern "C" int vgl_bgzf_compress_device(int32_t device, const uint8_t* src, int64_t n, uint8_t* dst, int64_t dst_cap, int64_t* out_n,
                                        void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (n < 0 || (n > 0 && (!src || !dst))) return vgl_pack_set_error(VGL_E_ARG, "vgl_bgzf_compress_device: bad argument");
    if (dst_cap < vgl_bgzf_bound(n)) return vgl_pack_set_error(VGL_E_ARG, "vgl_bgzf_compress_device: dst_cap is below vgl_bgzf_bound(n)");
    const Layout L = layout_of(n);
    if (n > 0 && (!workspace || workspace_bytes < L.total)) return vgl_pack_set_error(VGL_E_ARG, "vgl_bgzf_compress_device: workspace smaller than vgl_bgzf_workspace_bytes(n)");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bgzf_compress_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n == 0) {
        if (out_n && hipMemsetAsync(out_n, 0, sizeof(int64_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bgzf_compress_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    uint8_t* ws = (uint8_t*)workspace;
    int64_t* off = (int64_t*)(ws + L.off);
    uint32_t* sizes = (uint32_t*)(ws + L.sizes);
    uint8_t* slots = ws + L.slots;
    uint32_t* scratch = (uint32_t*)(ws + L.scratch);
    hipLaunchKernelGGL(k_bgzf_member, dim3((unsigned)L.grid), dim3(NT), 0, st, src, n, L.members, scratch, slots, sizes);
    hipLaunchKernelGGL(k_bgzf_scan, dim3(1), dim3(1024), 0, st, L.members, sizes, off, out_n);
    const int64_t cg = L.members < 4096 ? L.members : 4096;
    hipLaunchKernelGGL(k_bgzf_compact, dim3((unsigned)cg), dim3(256), 0, st, L.members, slots, off, sizes, dst);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bgzf_compress_device: a launch failed");
    return VGL_OK;
}
