// gtdisc.hip -- the kernels of gtdiscordance_hip and their launch code (a translation unit of the program: the library gets no entry point).
// A batch is the text of the sample columns of up to max_recs matched truth / call lines and one gtd::Rec per record; the per-sample
// rules are gtdisc_core.h.
//   k_gtd_parse       one workgroup of 256 lanes per record, the truth region and then the call region.  A region is walked in chunks of
//                     256 x 16 bytes on 16-byte address boundaries as k_vcfin_parse walks a line (column_walk.hip.h, shared with fetchgl.hip): a lane whose 16 bytes lie inside the
//                     region loads them at once, the lanes at the two ends read their bytes one by one -- no byte outside the region is
//                     read.  A scan of the tab counts numbers the columns; the lane that owns the tab before column s parses that column
//                     (gtd::sample_true / gtd::sample_call, bounded by the region's end) and stores one byte per plane: true bases,
//                     called bases (0xFF missing), GQ.  The status (an OR over the columns, and the column count against n_samples) is
//                     stored by lane 0.  No atomics.
//   k_gtd_bcf_decode  --bcf-direct 1, in k_gtd_parse's place: the same planes and status from the typed GT / GQ / PL vectors of a BCF
//                     side (gtdbcf_core.h), 16 bytes a lane where GT is int8 pairs; a text side of a mixed pair is walked as above
//   k_gtd_tally       k_disc_tally's shape: a workgroup of 16 wavefronts owns 64 consecutive samples over a run of records, a wavefront
//                     takes a record (ST_OK ones only), its lanes the samples; counts go to an LDS histogram [cell][GQ][sample] of 16-bit
//                     counters -- a counter belongs to one sample and a run has at most 32768 records, so none can wrap -- and once per
//                     workgroup the non-zero counters are added to the int64 table (layout of vgl_disc_table_len) with 64-bit atomics.
//   k_gtd_list_plan   a workgroup per record: the byte counts of its -doGQ 1 / 2 lines and of its -perSite lines (0 for a ST_HOST record)
//   k_offsets_scan    (wg_scan.hip.h) a workgroup per count: the exclusive prefix sums of both counts over the batch's records
//   k_gtd_list_write  a workgroup per record, a lane per line: the lines' lengths are scanned across the workgroup, chunk by chunk, and
//                     every lane formats its line at its offset, never past the text's capacity
// The planes never leave the device; the table is read once, the listing text per batch.
// Two bases: the truth side and the call side of a record are read from a base pointer and a byte count of their own.  A batch that
// is staged whole passes its staging twice; under --resident 1 a side whose file lies in device memory (resident_file.h) passes that
// file, and Rec::t_off / c_off and the BSide offsets of the side count from the file's first byte.  Every bound is the side's own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/vcfgl_hip.h"
#include "gtdisc_dev.h"
#include "gtdres_core.h"
#include "column_walk.hip.h"
#include "batch_dev.hip.h"

namespace {

using colwalk::NT;                       // lanes per workgroup of the parser and the listing kernels (column_walk.hip.h)
using colwalk::LB;                       // bytes per lane and chunk
using colwalk::scan_columns;
constexpr int TNT = 1024;                // lanes per workgroup of the tally
constexpr int SG = 64;                   // samples per tally workgroup
constexpr int NCELL = gtd::N_CELLS, NGQ = gtd::N_GQ;
constexpr int HIST = NCELL * NGQ * SG;   // 16-bit counters
constexpr int MAX_RUN = 32768;           // records per tally workgroup: below 2^16
constexpr size_t TALLY_LDS = (size_t)HIST * 2 + SG * sizeof(uint32_t);

struct ParseArgs {
    const uint8_t* t_text; int64_t t_bytes;                            // the truth side's base and byte count
    const uint8_t* c_text; int64_t c_bytes;                            // the call side's
    const gtd::Rec* recs; int32_t n_recs, N;
    uint8_t* tb; uint8_t* cb; uint8_t* gq; int32_t* status;
};

__global__ void __launch_bounds__(NT) k_gtd_parse(const ParseArgs A) {
    __shared__ int32_t s_tot[2][NT / 64];
    __shared__ int32_t s_bad[NT / 64];
    const int rec = blockIdx.x;
    if (rec >= A.n_recs) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const gtd::Rec r = A.recs[rec];
    const int32_t N = A.N;
    const int64_t tl = r.t_off, te = r.t_off + r.t_len, cl = r.c_off, ce = r.c_off + r.c_len;
    const bool fits = r.t_off >= 0 && r.t_len >= 0 && te <= A.t_bytes && r.c_off >= 0 && r.c_len >= 0 && ce <= A.c_bytes;
    const bool known = r.t_gti >= 0 && r.c_gti >= 0 && r.t_nal >= 1 && r.c_nal >= 1 && (r.gq_mode != gtd::GQ_TAG || r.c_gqi >= 0) &&
                       (r.gq_mode != gtd::GQ_PL || r.c_nal == 1 || (r.c_pli >= 0 && r.c_nal <= 5 && r.nG == gtd::n_genotypes(r.c_nal)));
    if (!fits || !known) {                                             // (the host sends no such record; never read outside the text)
        if (t == 0) A.status[rec] = gtd::ST_HOST;
        return;
    }
    const uint8_t* __restrict__ t_text = A.t_text;
    const uint8_t* __restrict__ c_text = A.c_text;
    uint8_t* __restrict__ tb = A.tb + (size_t)rec * (size_t)N;
    uint8_t* __restrict__ cb = A.cb + (size_t)rec * (size_t)N;
    uint8_t* __restrict__ gq = A.gq + (size_t)rec * (size_t)N;
    int bad = 0;
    const int32_t cols_t = scan_columns(t_text, tl, te, s_tot, [&](const int32_t col, const int64_t q) {
        if (col >= N) return;
        uint32_t b;
        if (!gtd::sample_true(t_text, q, te, r, b)) bad = 1; else tb[col] = (uint8_t)b;
    });
    __syncthreads();                                                   // (s_tot is used again)
    const int32_t cols_c = scan_columns(c_text, cl, ce, s_tot, [&](const int32_t col, const int64_t q) {
        if (col >= N) return;
        uint32_t b, g;
        if (!gtd::sample_call(c_text, q, ce, r, b, g)) bad = 1; else { cb[col] = (uint8_t)b; gq[col] = (uint8_t)g; }
    });
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (t == 0) {
        int B = 0;
        for (int k = 0; k < NT / 64; k++) B |= s_bad[k];
        if (cols_t != N || cols_c != N) B = 1;
        A.status[rec] = B ? gtd::ST_HOST : gtd::ST_OK;
    }
}

// ---- --bcf-direct 1: the planes from typed vectors ---------------------------------------------------------------------------------
struct DecodeArgs {
    const uint8_t* t_bytes; int64_t t_n;                               // the truth side's base and byte count: the batch's staging (vectors of
    const uint8_t* c_bytes; int64_t c_n;                               // a BCF side, text of another), or a resident file; the call side's
    const gtd::Rec* recs; const gtd::BSide* sides;                     // [n_recs], [2 * n_recs] (truth, call)
    int32_t n_recs, N;
    uint8_t* tb; uint8_t* cb; uint8_t* gq; int32_t* status;
};

constexpr int WS = 8;                    // samples a lane takes at once in the wide form: 16 bytes of int8 GT pairs

__device__ __forceinline__ void store8(uint8_t* __restrict__ p, const uint64_t v) {
    if (((uintptr_t)p & 7u) == 0) { *reinterpret_cast<uint64_t*>(p) = v; return; }
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
__device__ __forceinline__ int32_t widen8(const uint32_t byte) {
    const int8_t x = (int8_t)byte;
    return x == -128 ? gtd::BCF_MISSING : x == -127 ? gtd::BCF_EOV : (int32_t)x;
}

// one BCF side of a record: the samples' bytes into `plane` (true or called bases) and, for a call, `gqp`.  Returns 1 when a sample
// is not plain.  The common shape -- int8 GT, two values a sample -- is read 16 bytes a lane, so that a wavefront takes 1 KiB of
// consecutive bytes and stores its 8 bytes a plane at once: one load where the vector starts on a 16-byte address (the staging puts it
// there), the two aligned pieces around the lane's bytes joined by a byte shift where it does not (a resident file: gtd::load16_any,
// which loads a piece only when all of it lies inside [0, n_bytes) of the side).  Everything else, the last samples of such a vector
// and a lane whose pieces do not lie inside go a sample a lane through the per-value routines of gtdbcf_core.h (consecutive lanes
// still read consecutive vectors).  The caller has checked the descriptor against the side's byte count (gtd::side_fits).
template <bool CALL>
__device__ __forceinline__ int decode_side(const uint8_t* __restrict__ bytes, const int64_t n_bytes, const gtd::BSide& b, const gtd::Rec& r, const int32_t N,
                                           uint8_t* __restrict__ plane, uint8_t* __restrict__ gqp) {
    const int t = threadIdx.x;
    int bad = 0;
    auto one = [&](const int64_t s) {
        uint32_t x = 0, g = 0;
        if (CALL) { if (!gtd::bcf_sample_call(bytes, b, s, r.gq_mode, r.nG, x, g)) bad = 1; plane[s] = (uint8_t)x; gqp[s] = (uint8_t)g; }
        else { if (!gtd::bcf_sample_true(bytes, b, s, x)) bad = 1; plane[s] = (uint8_t)x; }
    };
#ifdef GTD_NO_WIDE_ANY                                                 // (the measurement of DESIGN.md 4.32: an unaligned vector a sample a lane)
    const bool wide = b.gt_type == 1 && b.gt_n == 2 && ((uintptr_t)(bytes + b.gt_off) & 15u) == 0;
#else
    const bool wide = b.gt_type == 1 && b.gt_n == 2;
#endif
    if (wide) {
        for (int64_t s0 = (int64_t)t * WS; s0 < N; s0 += (int64_t)NT * WS) {
            uint32_t w[4];
            // [gt_off + 2 s0, + 16) lies inside the N pairs; the pieces around it need not
            if (s0 + WS > N || !gtd::load16_any(bytes, b.gt_off + 2 * s0, n_bytes, w)) { for (int64_t s = s0; s < N && s < s0 + WS; s++) one(s); continue; }
            uint64_t o0 = 0, o1 = 0;
#pragma unroll
            for (int i = 0; i < WS; i++) {
                const uint32_t h = w[i >> 1] >> (16 * (i & 1));
                const int32_t x0 = widen8(h & 0xFFu), x1 = widen8((h >> 8) & 0xFFu);
                int a0 = 0, a1 = 0; uint32_t x = 0, g = 0;
                bool ok = x0 != gtd::BCF_EOV && x1 != gtd::BCF_EOV && gtd::gt_pair(x0, x1, a0, a1);
                if (ok) ok = CALL ? gtd::call_of(bytes, b, s0 + i, r.gq_mode, r.nG, a0, a1, x, g) : gtd::true_of(b, a0, a1, x);
                if (!ok) bad = 1;
                o0 |= (uint64_t)(x & 0xFFu) << (8 * i); o1 |= (uint64_t)(g & 0xFFu) << (8 * i);
            }
            store8(plane + s0, o0);
            if (CALL) store8(gqp + s0, o1);
        }
    } else {
        for (int64_t s = t; s < N; s += NT) one(s);
    }
    return bad;
}

// One workgroup of 256 lanes per record, the truth side and then the call side.  A BCF side (BSide::have) is decoded from its vectors,
// a text side is walked as k_gtd_parse walks it; the status is the OR of both.  Every descriptor is checked against the byte count
// of its own side before a byte is read; a record that fails the check is ST_HOST.  No atomics.
__global__ void __launch_bounds__(NT) k_gtd_bcf_decode(const DecodeArgs A) {
    __shared__ int32_t s_tot[2][NT / 64];
    __shared__ int32_t s_bad[NT / 64];
    const int rec = blockIdx.x;
    if (rec >= A.n_recs) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const gtd::Rec r = A.recs[rec];
    const gtd::BSide T = A.sides[2 * (size_t)rec], C = A.sides[2 * (size_t)rec + 1];
    const int32_t N = A.N;
    const int64_t tl = r.t_off, te = r.t_off + r.t_len, cl = r.c_off, ce = r.c_off + r.c_len;
    bool ok = r.t_nal >= 1 && r.c_nal >= 1;
    if (T.have) ok = ok && T.nal == r.t_nal && gtd::side_fits(T, false, r.gq_mode, r.nG, N, A.t_n);
    else ok = ok && r.t_off >= 0 && r.t_len >= 0 && te <= A.t_n && r.t_gti >= 0;
    if (C.have) ok = ok && C.nal == r.c_nal && gtd::side_fits(C, true, r.gq_mode, r.nG, N, A.c_n);
    else ok = ok && r.c_off >= 0 && r.c_len >= 0 && ce <= A.c_n && r.c_gti >= 0 && (r.gq_mode != gtd::GQ_TAG || r.c_gqi >= 0) &&
              (r.gq_mode != gtd::GQ_PL || r.c_nal == 1 || (r.c_pli >= 0 && r.c_nal <= 5 && r.nG == gtd::n_genotypes(r.c_nal)));
    if (!ok) {                                                         // (the host sends no such record; never read outside the bytes)
        if (t == 0) A.status[rec] = gtd::ST_HOST;
        return;
    }
    const uint8_t* __restrict__ t_bytes = A.t_bytes;
    const uint8_t* __restrict__ c_bytes = A.c_bytes;
    uint8_t* __restrict__ tb = A.tb + (size_t)rec * (size_t)N;
    uint8_t* __restrict__ cb = A.cb + (size_t)rec * (size_t)N;
    uint8_t* __restrict__ gq = A.gq + (size_t)rec * (size_t)N;
    int bad = 0;
    int32_t cols_t = N, cols_c = N;
    if (T.have) bad |= decode_side<false>(t_bytes, A.t_n, T, r, N, tb, nullptr);
    else cols_t = scan_columns(t_bytes, tl, te, s_tot, [&](const int32_t col, const int64_t q) {
        if (col >= N) return;
        uint32_t b;
        if (!gtd::sample_true(t_bytes, q, te, r, b)) bad = 1; else tb[col] = (uint8_t)b;
    });
    __syncthreads();                                                   // (s_tot is used again)
    if (C.have) bad |= decode_side<true>(c_bytes, A.c_n, C, r, N, cb, gq);
    else cols_c = scan_columns(c_bytes, cl, ce, s_tot, [&](const int32_t col, const int64_t q) {
        if (col >= N) return;
        uint32_t b, g;
        if (!gtd::sample_call(c_bytes, q, ce, r, b, g)) bad = 1; else { cb[col] = (uint8_t)b; gq[col] = (uint8_t)g; }
    });
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (t == 0) {
        int B = 0;
        for (int k = 0; k < NT / 64; k++) B |= s_bad[k];
        if (cols_t != N || cols_c != N) B = 1;
        A.status[rec] = B ? gtd::ST_HOST : gtd::ST_OK;
    }
}

struct TallyArgs {
    int32_t N, n_recs, run;
    const uint8_t* tb; const uint8_t* cb; const uint8_t* gq; const int32_t* status;
    unsigned long long* table;
};

__global__ __launch_bounds__(TNT) void k_gtd_tally(const TallyArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];       // [HIST / 2] counters, [SG] call-missing
    uint32_t* const s_mis = s_h + HIST / 2;
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < HIST / 2 + SG; k += TNT) s_h[k] = 0u;
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const int N = A.N;
    const int s = (int)blockIdx.x * SG + lane;
    const int i0 = (int)blockIdx.y * A.run;
    const int i1 = (A.n_recs - i0 < A.run) ? A.n_recs : i0 + A.run;
    uint32_t mis = 0;
    const int wv0 = __builtin_amdgcn_readfirstlane(wv);
    for (int i = i0 + wv0; i < i1; i += TNT / 64) {
        if (A.status[i] != gtd::ST_OK || s >= N) continue;
        const size_t at = (size_t)i * (size_t)N + (size_t)s;
        const uint32_t c = A.cb[at];
        if (c == (uint32_t)gtd::CALL_MISSING) { ++mis; continue; }
        const uint32_t cell = gtd::classify(A.tb[at], c);
        const uint32_t g = A.gq[at] & (uint32_t)(NGQ - 1);
        const uint32_t idx = (cell * NGQ + g) * SG + (uint32_t)lane;
        atomicAdd(&s_h[idx >> 1], 1u << (16u * (idx & 1u)));
    }
    if (mis) atomicAdd(&s_mis[lane], mis);
    __syncthreads();
    for (int w = tid; w < HIST / 2; w += TNT) {
        const uint32_t word = s_h[w];
        if (!word) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t n = word >> (16 * h) & 0xffffu;
            const int idx = 2 * w + h, ls = idx & (SG - 1), cg = idx >> 6;   // cg = cell * 128 + GQ
            const int sm = (int)blockIdx.x * SG + ls;
            if (n && sm < N) atomicAdd(&A.table[(size_t)sm * (NCELL * NGQ) + cg], (unsigned long long)n);
        }
    }
    if (tid < SG) {
        const int sm = (int)blockIdx.x * SG + tid;
        if (s_mis[tid] && sm < N) atomicAdd(&A.table[(size_t)N * (NCELL * NGQ) + sm], (unsigned long long)s_mis[tid]);
    }
}

struct ListArgs {
    int32_t N, n_recs, list, per_site;
    const gtd::Rec* recs;
    const uint8_t* tb; const uint8_t* cb; const uint8_t* gq; const int32_t* status;
    int64_t* len;                        // [2][n_recs]: listing, per-site
    int64_t* off;                        // [2][n_recs + 1]
    uint8_t* list_text; uint8_t* site_text; int64_t list_cap, site_cap;
};

// the lengths of sample s's two lines (0 where it has none)
__device__ __forceinline__ void line_lens(const ListArgs& A, const gtd::Rec& r, const size_t row, const int32_t s, uint32_t& l0, uint32_t& l1, uint32_t& cell, uint32_t& g) {
    l0 = l1 = 0; cell = 0; g = 0;
    const uint32_t c = A.cb[row + s];
    if (c == (uint32_t)gtd::CALL_MISSING) return;
    cell = gtd::classify(A.tb[row + s], c); g = A.gq[row + s];
    if (A.list) l0 = gtd::list_len(A.list, r.nsites1, (uint32_t)s, cell, g);
    if (A.per_site) l1 = gtd::site_len(r.pos, (uint32_t)s, cell);
}

__global__ void __launch_bounds__(NT) k_gtd_list_plan(const ListArgs A) {
    __shared__ unsigned long long s_sum[2][NT / 64];
    const int rec = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rec >= A.n_recs) return;
    unsigned long long n0 = 0, n1 = 0;
    if (A.status[rec] == gtd::ST_OK) {
        const gtd::Rec r = A.recs[rec];
        const size_t row = (size_t)rec * (size_t)A.N;
        for (int32_t s = t; s < A.N; s += NT) { uint32_t l0, l1, cell, g; line_lens(A, r, row, s, l0, l1, cell, g); n0 += l0; n1 += l1; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { n0 += __shfl_down(n0, d, 64); n1 += __shfl_down(n1, d, 64); }
    if (lane == 0) { s_sum[0][wave] = n0; s_sum[1][wave] = n1; }
    __syncthreads();
    if (t < 2) {
        unsigned long long x = 0;
        for (int k = 0; k < NT / 64; k++) x += s_sum[t][k];
        A.len[(size_t)t * A.n_recs + rec] = (int64_t)x;
    }
}

// (two values a lane go through one step here, with one __syncthreads a chunk: the step is written out, not wgscan::step twice)
__global__ void __launch_bounds__(NT) k_gtd_list_write(const ListArgs A) {
    __shared__ uint32_t s_tot[2][2][NT / 64];
    const int rec = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rec >= A.n_recs || A.status[rec] != gtd::ST_OK) return;       // (uniform over the workgroup)
    const gtd::Rec r = A.recs[rec];
    const size_t row = (size_t)rec * (size_t)A.N;
    int64_t at0 = A.off[rec], at1 = A.off[(size_t)A.n_recs + 1 + rec];
    const int n_chunks = (A.N + NT - 1) / NT;
    for (int c = 0; c < n_chunks; c++) {
        const int32_t s = c * NT + t;
        uint32_t l0 = 0, l1 = 0, cell = 0, g = 0;
        if (s < A.N) line_lens(A, r, row, s, l0, l1, cell, g);
        uint32_t i0 = l0, i1 = l1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y0 = __shfl_up(i0, d, 64), y1 = __shfl_up(i1, d, 64); if (lane >= d) { i0 += y0; i1 += y1; } }
        if (lane == 63) { s_tot[c & 1][0][wave] = i0; s_tot[c & 1][1][wave] = i1; }
        __syncthreads();
        uint32_t b0 = 0, b1 = 0, t0 = 0, t1 = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; k++) {
            const uint32_t x0 = s_tot[c & 1][0][k], x1 = s_tot[c & 1][1][k];
            if (k < wave) { b0 += x0; b1 += x1; }
            t0 += x0; t1 += x1;
        }
        if (l0) {
            const int64_t at = at0 + b0 + i0 - l0;
            if (at >= 0 && at < A.list_cap) {
                const int64_t room = A.list_cap - at;
                gtd::Emit<true> e{A.list_text + at, 0u, (uint32_t)(room < gtd::LINE_BOUND ? room : gtd::LINE_BOUND)};
                gtd::list_line(e, A.list, r.nsites1, (uint32_t)s, cell, g);
            }
        }
        if (l1) {
            const int64_t at = at1 + b1 + i1 - l1;
            if (at >= 0 && at < A.site_cap) {
                const int64_t room = A.site_cap - at;
                gtd::Emit<true> e{A.site_text + at, 0u, (uint32_t)(room < gtd::LINE_BOUND ? room : gtd::LINE_BOUND)};
                gtd::site_line(e, r.pos, (uint32_t)s, cell);
            }
        }
        at0 += t0; at1 += t1;
    }
}

}  // namespace

// ---- the handle (batch_dev.hip.h) ------------------------------------------------------------------------------------------------
struct GtdDev : batchdev::BatchDev {
    int32_t N = 0, max_recs = 0; int64_t max_text = 0; int list = 0, per_site = 0;
    int64_t list_cap = 0, site_cap = 0;
    batchdev::DevMem<unsigned long long> d_table; int64_t table_len = 0;
    int bcf = 0, timed = 0; double ms_stage = 0, ms_decode = 0;        // --bcf-direct 1 / --resident 1: the retired batches' device time
    struct Slot {
        batchdev::PinMem<gtd::BSide> h_sides; batchdev::DevMem<gtd::BSide> d_sides;
        batchdev::Event t0, k0, k1, t1;                                // (timing events: the batch's first copy, around the decode, its last kernel)
        batchdev::PinMem<uint8_t> h_text; batchdev::PinMem<gtd::Rec> h_recs;
        batchdev::PinMem<int32_t> h_status; batchdev::PinMem<int64_t> h_off; batchdev::PinMem<uint8_t> h_list, h_site;
        batchdev::DevMem<uint8_t> d_text; batchdev::DevMem<gtd::Rec> d_recs;
        batchdev::DevMem<uint8_t> d_planes; batchdev::DevMem<int32_t> d_status; batchdev::DevMem<int64_t> d_len, d_off;
        batchdev::DevMem<uint8_t> d_list, d_site;
    } slot[2];
};

const char* gtd_dev_error(GtdDev* d) { return d->err; }

GtdDev* gtd_dev_create(int device, int32_t n_samples, int32_t max_recs, int64_t max_text, int list, int per_site, int bcf, int timed, char* err, size_t err_len) {
    if (n_samples <= 0 || max_recs <= 0 || max_text < 0) { snprintf(err, err_len, "bad batch shape"); return nullptr; }
    return batchdev::create<GtdDev>(device, err, err_len, [&](GtdDev* d) {
        d->N = n_samples; d->max_recs = max_recs; d->max_text = max_text; d->list = list; d->per_site = per_site; d->bcf = bcf; d->timed = (bcf || timed) ? 1 : 0;
        d->list_cap = list ? (int64_t)max_recs * n_samples * gtd::LINE_BOUND : 0;
        d->site_cap = per_site ? (int64_t)max_recs * n_samples * gtd::LINE_BOUND : 0;
        d->table_len = vgl_disc_table_len(d->N);
        BATCH_HIP(d, d->d_table.alloc((size_t)d->table_len * 8));
        BATCH_HIP(d, hipMemsetAsync(d->d_table, 0, (size_t)d->table_len * 8, d->stream));
        const size_t R = (size_t)d->max_recs, N = (size_t)d->N;
        for (GtdDev::Slot& s : d->slot) {
            bool ok = s.h_text.alloc(d->device, (size_t)d->max_text); ok &= s.h_recs.alloc(d->device, R * sizeof(gtd::Rec));
            ok &= s.h_status.alloc(d->device, R * 4); ok &= s.h_off.alloc(d->device, 2 * (R + 1) * 8);
            ok &= s.h_list.alloc(d->device, (size_t)d->list_cap); ok &= s.h_site.alloc(d->device, (size_t)d->site_cap);
            if (!ok) return d->no_pinned();
            BATCH_HIP(d, s.d_text.alloc((size_t)d->max_text + LB));
            BATCH_HIP(d, s.d_recs.alloc(R * sizeof(gtd::Rec)));
            if (d->bcf) {
                if (!s.h_sides.alloc(d->device, 2 * R * sizeof(gtd::BSide))) return d->no_pinned();
                BATCH_HIP(d, s.d_sides.alloc(2 * R * sizeof(gtd::BSide)));
            }
            if (d->timed) for (batchdev::Event* e : {&s.t0, &s.k0, &s.k1, &s.t1}) BATCH_HIP(d, hipEventCreate(&e->h));
            BATCH_HIP(d, s.d_planes.alloc(3 * R * N));
            BATCH_HIP(d, s.d_status.alloc(R * 4));
            BATCH_HIP(d, s.d_len.alloc(2 * R * 8));
            BATCH_HIP(d, s.d_off.alloc(2 * (R + 1) * 8));
            BATCH_HIP(d, s.d_list.alloc((size_t)d->list_cap + 1));
            BATCH_HIP(d, s.d_site.alloc((size_t)d->site_cap + 1));
        }
        return 0;
    });
}

uint8_t* gtd_dev_text(GtdDev* d, int slot) { return d->slot[slot & 1].h_text; }
gtd::Rec* gtd_dev_recs(GtdDev* d, int slot) { return d->slot[slot & 1].h_recs; }
gtd::BSide* gtd_dev_sides(GtdDev* d, int slot) { return d->slot[slot & 1].h_sides; }
void gtd_dev_times(GtdDev* d, double* stage_ms, double* decode_ms) { *stage_ms = d->ms_stage; *decode_ms = d->ms_decode; }

// the copies of a batch up and its launch sequence; a side's base is the resident file it was given, or the slot's staging
static int submit_on(GtdDev* d, int slot, int32_t n_recs, int64_t text_bytes, const uint8_t* t_base, int64_t t_bytes, const uint8_t* c_base, int64_t c_bytes) {
    GtdDev::Slot& s = d->slot[slot & 1];
    if (n_recs == 0) return 0;
    hipStream_t st = d->stream;
    const size_t R = (size_t)n_recs, N = (size_t)d->N;
    if (!t_base) { t_base = s.d_text; t_bytes = text_bytes; }
    if (!c_base) { c_base = s.d_text; c_bytes = text_bytes; }
    if (d->timed) BATCH_HIP(d, hipEventRecord(s.t0, st));
    if (text_bytes > 0) BATCH_HIP(d, hipMemcpyAsync(s.d_text, s.h_text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    BATCH_HIP(d, hipMemcpyAsync(s.d_recs, s.h_recs, R * sizeof(gtd::Rec), hipMemcpyHostToDevice, st));
    uint8_t* tb = s.d_planes; uint8_t* cb = tb + (size_t)d->max_recs * N; uint8_t* gq = cb + (size_t)d->max_recs * N;
    if (d->bcf) BATCH_HIP(d, hipMemcpyAsync(s.d_sides, s.h_sides, 2 * R * sizeof(gtd::BSide), hipMemcpyHostToDevice, st));
    if (d->timed) BATCH_HIP(d, hipEventRecord(s.k0, st));
    if (d->bcf) {
        const DecodeArgs P{t_base, t_bytes, c_base, c_bytes, s.d_recs, s.d_sides, n_recs, d->N, tb, cb, gq, s.d_status};
        hipLaunchKernelGGL(k_gtd_bcf_decode, dim3((unsigned)n_recs), dim3(NT), 0, st, P);
    } else {
        const ParseArgs P{t_base, t_bytes, c_base, c_bytes, s.d_recs, n_recs, d->N, tb, cb, gq, s.d_status};
        hipLaunchKernelGGL(k_gtd_parse, dim3((unsigned)n_recs), dim3(NT), 0, st, P);
    }
    BATCH_HIP(d, hipGetLastError());
    if (d->timed) BATCH_HIP(d, hipEventRecord(s.k1, st));
    // the tally: about two workgroups per CU where the batch has them, runs of at least 16 records, never more than MAX_RUN
    const int groups = (d->N + SG - 1) / SG;
    int runs = 512 / groups;
    const int most = (n_recs + 15) / 16;
    if (runs > most) runs = most;
    if (runs < 1) runs = 1;
    int run = (n_recs + runs - 1) / runs;
    if (run > MAX_RUN) run = MAX_RUN;
    runs = (n_recs + run - 1) / run;
    const TallyArgs T{d->N, n_recs, run, tb, cb, gq, s.d_status, d->d_table};
    if (runs > 65535) return d->refuse("too many records for one batch");
    hipLaunchKernelGGL(k_gtd_tally, dim3((unsigned)groups, (unsigned)runs), dim3(TNT), TALLY_LDS, st, T);
    BATCH_HIP(d, hipGetLastError());
    if (d->list || d->per_site) {
        const ListArgs L{d->N, n_recs, d->list, d->per_site, s.d_recs, tb, cb, gq, s.d_status, s.d_len, s.d_off, s.d_list, s.d_site, d->list_cap, d->site_cap};
        hipLaunchKernelGGL(k_gtd_list_plan, dim3((unsigned)n_recs), dim3(NT), 0, st, L);
        BATCH_HIP(d, hipGetLastError());
        hipLaunchKernelGGL(wgscan::k_offsets_scan, dim3(2), dim3(wgscan::SCAN_NT), 0, st, (const int64_t*)s.d_len, (int64_t*)s.d_off, n_recs);
        BATCH_HIP(d, hipGetLastError());
        hipLaunchKernelGGL(k_gtd_list_write, dim3((unsigned)n_recs), dim3(NT), 0, st, L);
        BATCH_HIP(d, hipGetLastError());
        BATCH_HIP(d, hipMemcpyAsync(s.h_off, s.d_off, 2 * (R + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    if (d->timed) BATCH_HIP(d, hipEventRecord(s.t1, st));
    BATCH_HIP(d, hipMemcpyAsync(s.h_status, s.d_status, R * 4, hipMemcpyDeviceToHost, st));
    return d->end_submit(slot);
}

int gtd_dev_submit(GtdDev* d, int slot, int32_t n_recs, int64_t text_bytes) {
    if (d->begin_submit(slot, n_recs, n_recs >= 0 && n_recs <= d->max_recs && text_bytes >= 0 && text_bytes <= d->max_text) != 0) return -1;
    return submit_on(d, slot, n_recs, text_bytes, nullptr, 0, nullptr, 0);
}

int gtd_dev_submit_resident(GtdDev* d, int slot, int32_t n_recs, int64_t text_bytes, const uint8_t* t_file, int64_t t_bytes, const uint8_t* c_file, int64_t c_bytes) {
    const bool ok = n_recs >= 0 && n_recs <= d->max_recs && text_bytes >= 0 && text_bytes <= d->max_text && (!t_file || t_bytes >= 0) && (!c_file || c_bytes >= 0);
    if (d->begin_submit(slot, n_recs, ok) != 0) return -1;
    return submit_on(d, slot, n_recs, text_bytes, t_file, t_bytes, c_file, c_bytes);
}

int gtd_dev_wait(GtdDev* d, int slot, GtdBatchOut* out) {
    GtdDev::Slot& s = d->slot[slot & 1];
    if (d->begin_wait(slot) != 0) return -1;
    const size_t R = (size_t)d->head[slot & 1].n_recs;
    if (d->timed && R > 0) {
        float a = 0, b = 0;
        BATCH_HIP(d, hipEventElapsedTime(&a, s.t0, s.t1)); BATCH_HIP(d, hipEventElapsedTime(&b, s.k0, s.k1));
        d->ms_stage += a; d->ms_decode += b;
    }
    if (!(d->list || d->per_site) || R == 0) for (size_t i = 0; i < 2 * (R + 1); i++) s.h_off[i] = 0;
    const int64_t n_list = s.h_off[R], n_site = s.h_off[2 * R + 1];
    if (n_list < 0 || n_list > d->list_cap || n_site < 0 || n_site > d->site_cap) return d->refuse("a batch's listing is longer than its bound");
    if (n_list > 0) BATCH_HIP(d, hipMemcpyAsync(s.h_list, s.d_list, (size_t)n_list, hipMemcpyDeviceToHost, d->stream));
    if (n_site > 0) BATCH_HIP(d, hipMemcpyAsync(s.h_site, s.d_site, (size_t)n_site, hipMemcpyDeviceToHost, d->stream));
    if (n_list > 0 || n_site > 0) BATCH_HIP(d, hipStreamSynchronize(d->stream));
    out->status = s.h_status; out->list_off = s.h_off; out->site_off = s.h_off + R + 1; out->list_text = s.h_list; out->site_text = s.h_site;
    return 0;
}

int gtd_dev_table(GtdDev* d, int64_t* table) {
    BATCH_HIP(d, hipMemcpyAsync(table, d->d_table, (size_t)d->table_len * 8, hipMemcpyDeviceToHost, d->stream));
    BATCH_HIP(d, hipStreamSynchronize(d->stream));
    return 0;
}

void gtd_dev_quiesce(GtdDev* d) { if (d) d->quiesce(); }
void gtd_dev_destroy(GtdDev* d) { batchdev::destroy(d); }
