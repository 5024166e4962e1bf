// sal_apply.hip.h -- k_sal_bcf_apply, the relabelling kernel of setalleles_hip, for its two translation units: setalfile.hip launches
// it over a batch's staged vector blocks (ANY = false: every block begins on a multiple of 4 of the staging), setalres.hip over the
// resident file (ANY = true: a block begins at whatever byte the inflater wrote it to).  The per-sample rules are sal_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sal_core.h"
#include "rb_core.h"

namespace salapply {

constexpr int NT = 256;                  // lanes per workgroup

struct BArgs {
    const uint8_t* in; int64_t in_bytes;
    const sal::BRec* recs; int32_t n_recs, N;
    uint32_t* planes; uint32_t* work; int64_t vals;
    int32_t* status; int32_t* over; int32_t* width;
};

// value i of the vector at byte `at` of the resident file, widened as sal::bcf_load widens it: a byte, two bytes, or the four bytes
// through rb::load_u32_any -- never a word that reaches past `total`
struct AnyLoad {
    const uint8_t* bytes; int64_t at, total; int ty;
    VGL_HD uint32_t operator()(const int i) const {
        if (ty == 1) return sal::widen8(bytes[at + i]);
        if (ty == 2) return sal::widen16((uint16_t)((uint32_t)bytes[at + 2 * i] | (uint32_t)bytes[at + 2 * i + 1] << 8));
        return rb::load_u32_any(bytes, at + 4 * (int64_t)i, total);
    }
};

// BCF.  grid: (records, 3 fields), a workgroup per record and field, its lanes on consecutive samples.  A lane reads its sample's old
// vector at its width (PL: int8 / 16 / 32 with the sentinels widened), gathers the new order out of a register pair, normalises and
// writes nG_new floats.  PL goes to the int32 workspace first; the workgroup reduces the record's minimum and maximum (missing and
// end-of-vector left out, as bcf_enc_vint does), takes the narrowest width that holds them and every lane narrows its own samples
// into the plane.  A PL sample whose cast would overflow raises the record's `over` word.
template <bool ANY>
__global__ void __launch_bounds__(NT) k_sal_bcf_apply(const BArgs A) {
    __shared__ int32_t s_mn[NT / 64], s_mx[NT / 64];
    const int rec = blockIdx.x, f = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rec >= A.n_recs) return;
    const sal::BRec r = A.recs[rec];
    const int nv = f == 0 ? r.nv[0] : f == 1 ? r.nv[1] : r.nv[2];
    const int ty = f == 0 ? r.ty[0] : f == 1 ? r.ty[1] : r.ty[2];
    const int64_t in_off = f == 0 ? r.in_off[0] : f == 1 ? r.in_off[1] : r.in_off[2];
    if (nv <= 0) return;                                               // (uniform over the workgroup)
    const int64_t N = A.N;
    const int w_in = sal::type_width(ty), nG = r.n_new_g;
    const bool fits = sal::brec_sane(r) && in_off >= 0 && (ANY || (in_off & 3) == 0) && in_off + N * nv * w_in <= A.in_bytes &&
                      r.plane_off >= 0 && r.plane_off + sal::b_plane_vals(r, N) <= A.vals;
    if (!fits) {                                                       // (the host sends no such record; never read or write outside)
        if (t == 0) A.status[rec] = sal::ST_HOST;
        return;
    }
    const uint8_t* __restrict__ in = A.in + in_off;
    const int64_t base = r.plane_off + (int64_t)sal::b_slot(r, f) * nG * N;
    uint32_t v[sal::MAX_G];
    auto sample = [&](const int64_t s) {
        if (ANY) return sal::bcf_sample_from(AnyLoad{A.in, in_off + s * nv * w_in, A.in_bytes, ty}, nv, r.n2o, nG, f, v);
        return sal::bcf_sample(in + s * nv * w_in, ty, nv, r.n2o, nG, f, v);
    };
    if (f != sal::F_PL) {
        for (int64_t s = t; s < N; s += NT) {
            sample(s);
#pragma unroll
            for (int h = 0; h < sal::MAX_G; ++h) if (h < nG) A.planes[base + s * nG + h] = v[h];
        }
        return;
    }
    int32_t mn = INT32_MAX, mx = INT32_MIN + 1;
    int over = 0;
    for (int64_t s = t; s < N; s += NT) {
        if (sample(s)) over = 1;
#pragma unroll
        for (int h = 0; h < sal::MAX_G; ++h)
            if (h < nG) {
                A.work[base + s * nG + h] = v[h];
                const int32_t x = (int32_t)v[h];
                if (v[h] != sal::I_MISSING && v[h] != sal::I_END) { if (x < mn) mn = x; if (x > mx) mx = x; }
            }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const int32_t a = __shfl_down(mn, d, 64), b = __shfl_down(mx, d, 64); if (a < mn) mn = a; if (b > mx) mx = b; }
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    over = __syncthreads_or(over);
    for (int k = 0; k < NT / 64; k++) { if (s_mn[k] < mn) mn = s_mn[k]; if (s_mx[k] > mx) mx = s_mx[k]; }
    const int w = sal::int_width(mn, mx);                              // (every lane now holds the record's minimum and maximum)
    if (t == 0) { A.width[rec] = w; if (over) A.over[rec] = 1; }
    if (over) return;
    uint8_t* out = reinterpret_cast<uint8_t*>(A.planes + base);
    for (int64_t s = t; s < N; s += NT)
#pragma unroll
        for (int h = 0; h < sal::MAX_G; ++h)
            if (h < nG) sal::store_narrow(out, w, s * nG + h, A.work[base + s * nG + h]);
}

}  // namespace salapply
