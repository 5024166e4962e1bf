// The pure layer of the host batches (vcfgl_amd/csrc/hostlib/batch.h) on the CPU with -DVGL_MEM_TEST: the staging layouts of the
// three input families against the formulas vgl_*_host_create / _submit used before the layouts had one function each (written out
// here a second time, on purpose), the two-slot ring, the stream handle's tickets, and an allocation failure at every index of every
// family's buffers.  Built with -fsanitize=address,undefined by tests/test_hostbatch_cpu.py: a leak, a double free or a use after
// free is the sanitizer's report.  Prints `checks <n>` at the end.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "../include/vcfgl_hip.h"
#include "hostlib/err.h"
#include "hostlib/mem.h"
#include "hostlib/batch.h"

static int n_checks = 0;
#define CHECK(x) do { ++n_checks; if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)
static void fail_at(long k) { vgl_mem_calls = 0; vgl_mem_fail_at = k; }
static bool said(const char* text) { return strstr(g_err, text) != nullptr; }
static int64_t up(int64_t x) { return (x + 255) & ~(int64_t)255; }

static const int64_t COUNTS[] = {0, 1, 3, 77, 256, 2000};                 // 3 and 77: L * 4, L * 5 and L * 8 are no multiples of 256
static const int64_t BYTES[] = {0, 1, 255, 256, 257, 70001, 1 << 20};
static const int64_t SAMPLES[] = {1, 8, 1000};
constexpr int64_t MAX_COUNT = 2000, MAX_BYTES = 1 << 20;

static int layouts() {
    for (const int64_t N : SAMPLES) {
        const VcfinLayout vcap = vcfin_layout(MAX_BYTES, MAX_COUNT, N);
        const BcfinLayout bcap = bcfin_layout(MAX_BYTES, MAX_COUNT, N);
        {   // the capacities: never above what create allocated, below it by the last section's round-up at the most
            const int64_t L = MAX_COUNT;
            const int64_t vin = up(MAX_BYTES) + 2 * up(L * 8) + 2 * up(L * 4) + up(L * 5), out = up(L * N) + 2 * up(L * 4);
            const int64_t bin = up(MAX_BYTES) + up(L * 8) + 3 * up(L * 4) + up(L * 5);
            CHECK(vcap.in_used <= vin && vin - vcap.in_used == up(L * 5) - L * 5 && vcap.out_used <= out && out - vcap.out_used == up(L * 4) - L * 4);
            CHECK(bcap.in_used <= bin && bin - bcap.in_used == up(L * 5) - L * 5 && bcap.out_used <= out && out - bcap.out_used == up(L * 4) - L * 4);
        }
        for (const int64_t L : COUNTS) for (const int64_t T : BYTES) {
            {   // vgl_vcfin_host_submit
                const int64_t o_lb = up(T), o_le = o_lb + up(L * 8), o_gti = o_le + up(L * 8), o_nal = o_gti + up(L * 4), o_map = o_nal + up(L * 4);
                const int64_t in_used = o_map + L * 5, off_sum = up(L * N), off_status = off_sum + up(L * 4), out_used = off_status + L * 4;
                const VcfinLayout y = vcfin_layout(T, L, N);
                CHECK(y.text_bytes == T && y.lb == o_lb && y.le == o_le && y.gti == o_gti && y.nal == o_nal && y.map == o_map && y.in_used == in_used);
                CHECK(y.sum == off_sum && y.status == off_status && y.out_used == out_used);
                CHECK(y.in_used <= vcap.in_used && y.out_used <= vcap.out_used);
            }
            {   // vgl_bcfin_host_submit
                const int64_t o_beg = up(T), o_type = o_beg + up(L * 8), o_n = o_type + up(L * 4), o_nal = o_n + up(L * 4), o_map = o_nal + up(L * 4);
                const int64_t in_used = o_map + L * 5, off_sum = up(L * N), off_status = off_sum + up(L * 4), out_used = off_status + L * 4;
                const BcfinLayout y = bcfin_layout(T, L, N);
                CHECK(y.gt_bytes == T && y.beg == o_beg && y.type == o_type && y.n == o_n && y.nal == o_nal && y.map == o_map && y.in_used == in_used);
                CHECK(y.sum == off_sum && y.status == off_status && y.out_used == out_used);
                CHECK(y.in_used <= bcap.in_used && y.out_used <= bcap.out_used);
            }
        }
    }
    // vgl_inflate_host_*: a member is at most 65536 bytes either way, so a handle of M members takes inflate_layout(M * 65536, M * 65536, M)
    for (const int64_t M : {(int64_t)1, (int64_t)64, (int64_t)1 << 20}) {
        const InflateLayout cap = inflate_layout(M * 65536, M * 65536, M);
        const int64_t cin = up(M * 65536) + 2 * up(M * 8) + 2 * up(M * 4), cout = up(M * 65536) + up(M * 4);
        CHECK(cap.in_used <= cin && cin - cap.in_used == up(M * 4) - M * 4 && cap.out_used <= cout && cout - cap.out_used == up(M * 4) - M * 4);
        for (const int64_t L : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)63, M}) {
            if (L > M) continue;
            for (const int64_t in_sum : {(int64_t)0, (int64_t)28, L * 65536 - (L > 0), L * 65536}) for (const int64_t out_sum : {(int64_t)0, (int64_t)1, L * 65536}) {
                if (in_sum < 0) continue;
                const int64_t o_b = up(in_sum), o_o = o_b + up(L * 8), o_c = o_o + up(L * 8), o_i = o_c + up(L * 4);
                const int64_t in_used = o_i + L * 4, off_status = up(out_sum), out_used = off_status + L * 4;
                const InflateLayout y = inflate_layout(in_sum, out_sum, L);
                CHECK(y.in_sum == in_sum && y.begin == o_b && y.out_off == o_o && y.csize == o_c && y.isize == o_i && y.in_used == in_used);
                CHECK(y.out_bytes == out_sum && y.status == off_status && y.out_used == out_used);
                CHECK(y.in_used <= cap.in_used && y.out_used <= cap.out_used);
            }
        }
    }
    return 0;
}

template <typename R> static int ring(R& r) {
    CHECK(!r.ticket_ok(0) && !r.ticket_ok(1) && !r.release(0));                       // nothing is in flight
    CHECK(r.acquire("vgl_x_host") == VGL_OK && &r.cur() == &r.s[0] && r.commit() == 0);
    CHECK(r.acquire("vgl_x_host") == VGL_OK && &r.cur() == &r.s[1] && r.commit() == 1);
    CHECK(r.acquire("vgl_x_host") == VGL_E_ARG && said("vgl_x_host_submit: two batches are in flight (vgl_x_host_wait the older one first)"));
    CHECK(r.ticket_ok(0) && r.ticket_ok(1) && !r.ticket_ok(-1) && !r.ticket_ok(2) && !r.release(-1) && !r.release(2));
    CHECK(r.release(0) && !r.ticket_ok(0) && !r.release(0) && r.ticket_ok(1));       // a ticket is waited for once
    CHECK(r.acquire("vgl_x_host") == VGL_OK && r.commit() == 0);                      // tickets alternate: 0, 1, 0, ...
    CHECK(r.acquire("vgl_x_host") == VGL_E_ARG && r.release(1) && r.acquire("vgl_x_host") == VGL_OK && r.commit() == 1);
    CHECK(r.release(0) && r.release(1) && !r.release(1));
    return 0;
}

static int stream_tickets() {
    StreamSlots s;
    CHECK(s.reserve(3, 8, 100, 1000, 64, 2000) == VGL_OK && s.nb == 3 && vgl_mem_live == 2 + 3 * 8);
    CHECK(s.in_range(0) && s.in_range(2) && !s.in_range(3) && !s.in_range(-1));
    CHECK(s.ticket_ok(0) == VGL_E_ARG && said("vgl_stream_host_wait: bad ticket"));
    s.commit(2, 10); s.commit(0, 20);                                                 // submit order: buffer 2, then buffer 0
    CHECK(s.ticket_ok(0) == VGL_E_ARG && said("vgl_stream_host_wait: tickets are waited for in submit order"));
    CHECK(s.ticket_ok(1) == VGL_E_ARG && said("bad ticket") && s.ticket_ok(3) == VGL_E_ARG && s.ticket_ok(-1) == VGL_E_ARG);
    CHECK(s.ticket_ok(2) == VGL_OK && s.b[2].raw == 10);
    s.release(2);
    CHECK(s.ticket_ok(2) == VGL_E_ARG && said("bad ticket"));                         // waited for twice
    s.commit(2, 30);                                                                  // the buffer is free again: behind buffer 0 now
    CHECK(s.ticket_ok(2) == VGL_E_ARG && said("submit order") && s.ticket_ok(0) == VGL_OK);
    s.release(0);
    CHECK(s.ticket_ok(2) == VGL_OK && s.b[2].raw == 30);
    // the growth rule of the members' page-locked buffer
    CHECK(stream_members_room(1, 64 << 20) == 1 << 20 && stream_members_room(8 << 20, 64 << 20) == 10 << 20 && stream_members_room(60 << 20, 64 << 20) == 64 << 20);
    CHECK(stream_members_room(100, 4000) == 4000);
    return 0;
}

// an allocation failure at every index 0 .. n_allocs (the last: none fails): the code of the allocator, and nothing left behind
template <typename Set, typename Reserve> static int failures(long n_allocs, Reserve reserve) {
    for (long k = 0; k <= n_allocs; k++) {
        {
            Set set;
            fail_at(k);
            const int rc = reserve(set);
            CHECK(rc == (k < n_allocs ? VGL_E_NOMEM : VGL_OK) && vgl_mem_live == k && vgl_mem_calls == std::min(k + 1, n_allocs));
        }
        CHECK(vgl_mem_live == 0);
    }
    fail_at(-1);
    return 0;
}

int main() {
    if (layouts()) return 1;
    {
        StagedRing<VcfinLayout> a; BgzfRing b;
        CHECK(a.reserve(1000, 500) == VGL_OK && vgl_mem_live == 8 && a.s[1].h_in.cap == 1000 && a.s[1].d_in.cap == 1000 && a.s[0].h_out.cap == 500 && a.s[0].d_out.cap == 500);
        memset(a.s[1].h_in, 1, 1000); memset(a.s[0].h_out, 1, 500);
        CHECK(b.reserve(100, 120, 64) == VGL_OK && vgl_mem_live == 8 + 9 && b.ws.cap == 64 && b.d_n.cap == 2 && b.h_n.cap == 2 && b.s[1].d_in.cap == 100 && b.s[1].h_out.cap == 120);
        if (ring(a) || ring(b)) return 1;
    }
    CHECK(vgl_mem_live == 0);
    if (stream_tickets()) return 1;
    CHECK(vgl_mem_live == 0);
    if (failures<StagedRing<VcfinLayout>>(8, [](auto& s) { return s.reserve(1000, 500); })) return 1;
    if (failures<StagedRing<BcfinLayout>>(8, [](auto& s) { return s.reserve(1000, 500); })) return 1;
    if (failures<StagedRing<InflateLayout>>(8, [](auto& s) { return s.reserve(1000, 500); })) return 1;
    if (failures<BgzfRing>(9, [](auto& s) { return s.reserve(100, 120, 64); })) return 1;
    if (failures<StreamSlots>(2 + 8 * 8, [](auto& s) { return s.reserve(8, 8, 100, 1000, 64, 2000); })) return 1;
    if (failures<StreamSlots>(2 + 8, [](auto& s) { return s.reserve(1, 1, 1, 1, 0, 1); })) return 1;
    printf("checks %d\n", n_checks);
    return 0;
}
