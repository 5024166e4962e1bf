// The owners of the host library's memory (vcfgl_amd/csrc/hostlib/mem.h) on the CPU with -DVGL_MEM_TEST: the allocator is
// malloc / free with a "fail the k-th allocation" counter.  Built with -fsanitize=address,undefined by tests/test_hostmem_cpu.py:
// a leak, a double free or a use after free is the sanitizer's report; the program itself checks capacities, the byte account
// and the count of live blocks.  Prints `checks <n>` at the end.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <utility>

#include "../include/vcfgl_hip.h"
#include "hostlib/mem.h"

static int n_checks = 0;
#define CHECK(x) do { ++n_checks; if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)
static void fail_at(long k) { vgl_mem_calls = 0; vgl_mem_fail_at = k; }

int main() {
    size_t acct = 0;
    {   // growth, no-op reserve, reserve(0), release
        DevBuf<int32_t> b(&acct);
        CHECK(!b && b.cap == 0 && acct == 0);
        CHECK(b.reserve(10) == VGL_OK && b.cap == 10 && acct == 40 && vgl_mem_live == 1);
        int32_t* const first = b;
        for (int i = 0; i < 10; i++) b.p[i] = i;
        CHECK(b.reserve(10) == VGL_OK && b.reserve(3) == VGL_OK && b.reserve(0) == VGL_OK && b.p == first && b.cap == 10 && acct == 40);
        CHECK(b.reserve(11) == VGL_OK && b.cap == 11 && acct == 44 && vgl_mem_live == 1);          // freed, then allocated
        b.p[10] = 7;
        b.release();
        CHECK(!b && b.cap == 0 && acct == 0 && vgl_mem_live == 0);
        CHECK(b.reserve(0) == VGL_OK && b.cap == 1 && acct == 4);                                  // one element, as dmalloc did
        b.p[0] = 1;
        DevBuf<uint8_t> bytes;                                                                     // no account
        CHECK(bytes.reserve(5) == VGL_OK && bytes.bytes() == 5 && acct == 4 && bytes.as<char>() == (char*)bytes.p);
        PinBuf<int64_t> pin(&acct);
        CHECK(pin.reserve(2) == VGL_OK && acct == 20 && vgl_mem_live == 3);
    }
    CHECK(acct == 0 && vgl_mem_live == 0);
    {   // a failure at each allocation index: the buffer is left empty, the account exact
        DevBuf<double> b(&acct);
        fail_at(0);
        CHECK(b.reserve(4) == VGL_E_NOMEM && !b && b.cap == 0 && acct == 0 && vgl_mem_live == 0);
        fail_at(1);
        CHECK(b.reserve(4) == VGL_OK && acct == 32);
        CHECK(b.reserve(8) == VGL_E_NOMEM && !b && b.cap == 0 && acct == 0 && vgl_mem_live == 0);  // the old block is gone too
        fail_at(-1);
        CHECK(b.reserve(8) == VGL_OK && b.cap == 8 && acct == 64);
    }
    CHECK(acct == 0 && vgl_mem_live == 0);
    {   // move: one owner at any time
        DevBuf<int32_t> a(&acct);
        CHECK(a.reserve(6) == VGL_OK);
        int32_t* const p = a;
        DevBuf<int32_t> b(std::move(a));
        CHECK(!a && a.cap == 0 && b.p == p && b.cap == 6 && acct == 24 && vgl_mem_live == 1);
        DevBuf<int32_t> c(&acct);
        CHECK(c.reserve(2) == VGL_OK && acct == 32);
        c = std::move(b);                                                                           // c's own block is freed
        CHECK(!b && c.p == p && c.cap == 6 && acct == 24 && vgl_mem_live == 1);
    }
    CHECK(acct == 0 && vgl_mem_live == 0);
    {   // the non-owning state is never freed, never counted, and ends with the next reserve
        DevBuf<int64_t> parent(&acct);
        CHECK(parent.reserve(3) == VGL_OK && acct == 24);
        size_t acct2 = 0;
        {
            DevBuf<int64_t> sibling(&acct2);
            sibling.borrow(parent);
            CHECK(sibling.p == parent.p && !sibling.owned && acct2 == 0);
            sibling.release();
            CHECK(!sibling && vgl_mem_live == 1);
            sibling.borrow(parent);
            DevBuf<int64_t> moved(std::move(sibling));
            CHECK(moved.p == parent.p && !moved.owned && sibling.owned && !sibling);
            CHECK(moved.reserve(2) == VGL_OK && moved.owned && moved.p != parent.p && acct2 == 16 && vgl_mem_live == 2);
            moved.borrow(parent);                                                                   // its own block is freed first
            CHECK(acct2 == 0 && vgl_mem_live == 1);
        }
        CHECK(vgl_mem_live == 1 && acct == 24);
        parent.p[2] = 5;                                                                            // still the parent's
    }
    CHECK(acct == 0 && vgl_mem_live == 0);
    {   // TextOut: workspace, offsets, text -- a failure on the second and on the third leaves what was reserved to the destructor
        for (long k = 0; k < 3; k++) {
            TextOut t;
            fail_at(k);
            CHECK(t.reserve(100, 8, 64) == VGL_E_NOMEM);
            CHECK((k > 0) == (bool)t.ws && (k > 1) == (bool)t.off && !t.text && vgl_mem_live == k);
            fail_at(-1);
            CHECK(t.reserve(100, 8, 64) == VGL_OK && t.ws.cap == 64 && t.off.cap == 9 && t.text.cap == 100 && t.ws_bytes == 64 && vgl_mem_live == 3);
            const long calls = vgl_mem_calls;
            CHECK(calls == 3 - k && t.reserve(50, 8, 64) == VGL_OK && vgl_mem_calls == calls);     // nothing grows: no allocation
        }
        TextOut shared;                                                                             // no text, no workspace of its own
        CHECK(shared.reserve(-1, 4, -1) == VGL_OK && !shared.text && !shared.ws && shared.off.cap == 5 && vgl_mem_live == 1);
    }
    CHECK(vgl_mem_live == 0);
    {   // release_all
        DevBuf<int32_t> a(&acct); DevBuf<uint8_t> b(&acct);
        CHECK(a.reserve(1) == VGL_OK && b.reserve(1) == VGL_OK && acct == 5);
        release_all(a, b);
        CHECK(!a && !b);
    }
    CHECK(acct == 0 && vgl_mem_live == 0);
    printf("checks %d\n", n_checks);
    return 0;
}
