// hostlib/mem.h -- owners of the host library's device and pinned-host memory, streams and events.
//
// DevBuf<T>: a device pointer and its capacity in elements; move-only, freed by its destructor.  reserve(n) is grow-only: a buffer
// that holds n elements stays, a smaller one is freed and allocated again (never copied: every user refills it).  PinBuf<T> is the
// same for page-locked host memory.  A buffer built with an `account` adds its bytes there while it holds them: the context's
// workspace_bytes (vgl_ctx_info).  borrow() puts a buffer into the non-owning state: the pointer of another buffer, never freed here
// (the two tables the sibling context of a deep tile takes from its parent).
//
// The header reaches the allocator through vgl_mem_alloc / vgl_mem_free alone.  With -DVGL_MEM_TEST those are malloc / free with a
// "fail the k-th allocation" counter and a count of the live blocks, so that the owners run on the CPU under a sanitizer
// (tests/hostmem_main.cpp); nothing of HIP is needed then.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef VGL_MEM_TEST
#include <stdlib.h>
static long vgl_mem_calls = 0, vgl_mem_fail_at = -1, vgl_mem_live = 0;       // allocation k (from 0) fails when k == vgl_mem_fail_at
static inline int vgl_mem_alloc(void** p, size_t bytes, bool /*pinned*/) {
    *p = (vgl_mem_calls++ == vgl_mem_fail_at) ? nullptr : malloc(bytes);
    if (!*p) return VGL_E_NOMEM;
    ++vgl_mem_live;
    return VGL_OK;
}
static inline void vgl_mem_free(void* p, bool /*pinned*/) { --vgl_mem_live; free(p); }
#else
static inline int vgl_mem_alloc(void** p, size_t bytes, bool pinned) {
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e == hipSuccess) return VGL_OK;
    *p = nullptr;
    return fail(hip_code(e), "%s of %zu bytes: %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
}
static inline void vgl_mem_free(void* p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
#endif

template <typename T, bool PINNED = false> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                    // elements
    size_t* account = nullptr;
    bool owned = true;

    DevBuf() = default;
    explicit DevBuf(size_t* acct) : account(acct) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), account(o.account), owned(o.owned) { o.p = nullptr; o.cap = 0; o.owned = true; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; account = o.account; owned = o.owned; o.p = nullptr; o.cap = 0; o.owned = true; }
        return *this;
    }
    ~DevBuf() { release(); }

    // the raw pointer, two ways: the implicit conversion (kernels and launchers take raw pointers), and as() where the language does
    // not convert by itself (an arm of ?:, pointer arithmetic on bytes) or the bytes are read as another type, as<const int32_t>()
    operator T*() const { return p; }
    template <typename U = T> U* as() const { return (U*)p; }
    size_t bytes() const { return cap * sizeof(T); }

    void release() {
        if (p && owned) { vgl_mem_free((void*)p, PINNED); if (account) *account -= bytes(); }
        p = nullptr; cap = 0; owned = true;
    }
    // room for n elements (n = 0: one).  VGL_E_NOMEM / VGL_E_NODEVICE from the allocator, with the buffer left empty
    int reserve(size_t n) {
        if (n == 0) n = 1;
        if (p && owned && cap >= n) return VGL_OK;
        release();
        const int rc = vgl_mem_alloc((void**)&p, n * sizeof(T), PINNED);
        if (rc != VGL_OK) { p = nullptr; return rc; }
        cap = n;
        if (account) *account += bytes();
        return VGL_OK;
    }
    void borrow(T* q) { release(); p = q; owned = false; }
};
template <typename T> using PinBuf = DevBuf<T, true>;
template <typename... B> static inline void release_all(B&... b) { (b.release(), ...); }       // (free a group before any of it is allocated again)

// One text side output of a tile (record text, gVCF block text, pileup, fetch-GL): the text, the n_sites + 1 offsets of its sites and
// the formatter's workspace.  text_cap < 0 / ws_bytes < 0: that part lives elsewhere (a device destination written in place; the block
// formatter shares the record formatter's workspace).
struct TextOut {
    DevBuf<uint8_t> text; DevBuf<int64_t> off; DevBuf<uint8_t> ws;
    int64_t ws_bytes = 0;              // what the formatter was promised (<= ws.cap)
    int reserve(int64_t text_cap, size_t max_sites, int64_t ws_need) {
        int rc = VGL_OK;
        if (ws_need >= 0 && (rc = ws.reserve((size_t)ws_need)) != VGL_OK) return rc;
        if (ws_need >= 0) ws_bytes = ws_need;
        if ((rc = off.reserve(max_sites + 1)) != VGL_OK) return rc;
        if (text_cap >= 0 && (rc = text.reserve((size_t)text_cap)) != VGL_OK) return rc;
        return VGL_OK;
    }
};

#ifndef VGL_MEM_TEST
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    int create() { if (!s) HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return VGL_OK; }
};
struct Event {                         // (no timing: the order of two streams)
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create() { if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return VGL_OK; }
};
#endif
