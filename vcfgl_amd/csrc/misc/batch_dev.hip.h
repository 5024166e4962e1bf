// batch_dev.hip.h -- what the device handles of the misc programs share (GtdDev of gtdisc.hip, FglDev of fetchgl.hip, SalDev of
// setalfile.hip): the owners of their memory, stream and events, and a base that holds two batches in flight on one stream.
//
// DevMem<T> / PinMem<T> / Stream / Event are move-only and freed by their destructors, in the manner of hostlib/mem.h.  That header is
// not used here: it belongs to the library's one translation unit, and page-locked memory comes from the library's vgl_host_alloc_on
// here, not from hipHostMalloc.  Every hipMalloc, hipFree, vgl_host_free, hipEventDestroy and hipStreamDestroy of misc/ is in this file:
// a buffer a handle gains is a member, and a member cannot be forgotten when the handle goes.
//
// BatchDev: the device, the stream, the handle's message and the two slots' heads (the event behind a batch's last copy, its record
// count, whether it is in flight).  A handle derives from it, adds its buffers per slot and its own launch sequence; X_dev_destroy is
// quiesce and delete.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/vcfgl_hip.h"

namespace batchdev {

// device memory (PINNED false: alloc(bytes)) or page-locked staging on the device's NUMA node (true: alloc(device, bytes), through
// vgl_host_alloc_on; 0 bytes: one)
template <typename T, bool PINNED> struct Mem {
    T* p = nullptr;
    Mem() = default;
    Mem(const Mem&) = delete;
    Mem& operator=(const Mem&) = delete;
    Mem(Mem&& o) noexcept : p(o.p) { o.p = nullptr; }
    Mem& operator=(Mem&& o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~Mem() { release(); }
    operator T*() const { return p; }
    void release() { if (p) { if (PINNED) vgl_host_free(p); else (void)hipFree(p); } p = nullptr; }
    hipError_t alloc(size_t bytes) { static_assert(!PINNED, "device memory"); release(); return hipMalloc((void**)&p, bytes); }
    bool alloc(int device, size_t bytes) { static_assert(PINNED, "page-locked memory"); release(); p = (T*)vgl_host_alloc_on(device, bytes ? bytes : 1); return p != nullptr; }
};
template <typename T> using DevMem = Mem<T, false>;
template <typename T> using PinMem = Mem<T, true>;

// a stream or an event (no timing: a batch's last copy has landed)
template <typename H, hipError_t (*DESTROY)(H)> struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    ~Owned() { if (h) (void)DESTROY(h); }
    operator H() const { return h; }
};
typedef Owned<hipStream_t, hipStreamDestroy> Stream;
typedef Owned<hipEvent_t, hipEventDestroy> Event;

// "<call>: <what HIP says>" into the handle's message, and -1 out of the function
#define BATCH_HIP(d, call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return (d)->fail(#call, e_); } while (0)

struct SlotHead { Event done; int32_t n_recs = 0; bool busy = false; };

struct BatchDev {
    int device = 0;
    Stream stream;
    char err[256] = {0};
    SlotHead head[2];

    // (a handle's buffers are members of the derived struct and go before the stream does: X_dev_destroy waits first)
    ~BatchDev() { quiesce(); }

    int refuse(const char* why) { snprintf(err, sizeof err, "%s", why); return -1; }
    int fail(const char* what, hipError_t e) { snprintf(err, sizeof err, "%s: %s", what, hipGetErrorString(e)); return -1; }
    int no_pinned() { snprintf(err, sizeof err, "page-locked host memory could not be allocated: %s", vgl_last_error()); return -1; }
    // the device, the stream and the slots' events
    int open(int dev) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return refuse("no HIP device is available");
        if (dev < 0 || dev >= nd) return refuse("no such device");
        device = dev;
        BATCH_HIP(this, hipSetDevice(device));
        BATCH_HIP(this, hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking));
        for (SlotHead& h : head) BATCH_HIP(this, hipEventCreateWithFlags(&h.done.h, hipEventDisableTiming));
        return 0;
    }
    // a slot takes a batch of n_recs records: refused while its last one is in flight, or when the handle was not made for its shape
    int begin_submit(int slot, int32_t n_recs, bool ok_shape) {
        SlotHead& h = head[slot & 1];
        if (h.busy || !ok_shape) return refuse("a batch outside the shape the handle was made for, or a slot still in flight");
        h.n_recs = n_recs; h.busy = true;
        return 0;
    }
    int end_submit(int slot) { BATCH_HIP(this, hipEventRecord(head[slot & 1].done, stream)); return 0; }
    // the slot's batch has landed (a batch of no records was never sent)
    int begin_wait(int slot) {
        SlotHead& h = head[slot & 1];
        if (!h.busy) return refuse("nothing in flight in this slot");
        h.busy = false;
        if (h.n_recs > 0) BATCH_HIP(this, hipEventSynchronize(h.done));
        return 0;
    }
    void quiesce() { if (stream.h) (void)hipStreamSynchronize(stream); }
};

// X_dev_create behind its shape check: the handle opened on the device and set up by setup(d), or nullptr with the reason in why
template <typename D, typename Setup> D* create(int device, char* why, size_t why_len, Setup setup) {
    D* d = new D();
    if (d->open(device) == 0 && setup(d) == 0) return d;
    snprintf(why, why_len, "%s", d->err);
    d->quiesce();
    delete d;
    return nullptr;
}
template <typename D> void destroy(D* d) { if (!d) return; d->quiesce(); delete d; }

}  // namespace batchdev
