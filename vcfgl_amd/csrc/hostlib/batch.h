// hostlib/batch.h -- the five host-batch families (vgl_bgzf_host_*, vgl_stream_host_*, vgl_vcfin_host_*, vgl_inflate_host_*,
// vgl_bcfin_host_*): what a program without HIP of its own (the host program) uses.  Part of the one translation unit vgl_host.cpp.
//
// Two layers.  The upper one is pure: where a batch's sections lie in its staging (one layout function per input family, called with
// the batch's counts by submit and with the maxima by create, so the capacity formula exists once), the buffers of every family as
// owners of mem.h, and the two ticket disciplines -- the ring of two slots (ticket = slot index, slots taken in turn) and the stream
// handle's n_buffers slots that are waited for in submit order.  It needs fail() and mem.h only, and with -DVGL_MEM_TEST it runs on
// the CPU under a sanitizer (tests/hostbatch_main.cpp).  The lower one is HIP: one device check for the five creates, the staged
// submit (copy up, launch, copy down, event) and wait of the three input families, and the entry points.  A handle's destroy waits
// for its streams and deletes the handle; the owners free what it held.
#pragma once

// ---- pure layer -----------------------------------------------------------------------------------------------------------------
static inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }
// sections back to back, each starting on a multiple of 256 bytes; end = the bytes used (the last section is not rounded up)
struct Sections {
    int64_t end = 0;
    int64_t add(int64_t bytes) { const int64_t o = up256(end); end = o + bytes; return o; }
};

// in: text | line_begin, line_end (int64) | gti, n_alleles (int32) | allele_map [5] (int8).  out: rows [L][N] | sums | statuses (int32)
struct VcfinLayout { int64_t text_bytes, lb, le, gti, nal, map, in_used, sum, status, out_used; };
static inline VcfinLayout vcfin_layout(int64_t text_bytes, int64_t n_lines, int64_t n_samples) {
    VcfinLayout y; Sections in, out; const int64_t L = n_lines;
    in.add(y.text_bytes = text_bytes); y.lb = in.add(L * 8); y.le = in.add(L * 8); y.gti = in.add(L * 4); y.nal = in.add(L * 4); y.map = in.add(L * 5);
    out.add(L * n_samples); y.sum = out.add(L * 4); y.status = out.add(L * 4);
    y.in_used = in.end; y.out_used = out.end;
    return y;
}
// in: the GT slices | their starts (int64) | gt_type, gt_n, n_alleles (int32) | allele_map [5] (int8).  out: as vcfin
struct BcfinLayout { int64_t gt_bytes, beg, type, n, nal, map, in_used, sum, status, out_used; };
static inline BcfinLayout bcfin_layout(int64_t gt_bytes, int64_t n_records, int64_t n_samples) {
    BcfinLayout y; Sections in, out; const int64_t L = n_records;
    in.add(y.gt_bytes = gt_bytes); y.beg = in.add(L * 8); y.type = in.add(L * 4); y.n = in.add(L * 4); y.nal = in.add(L * 4); y.map = in.add(L * 5);
    out.add(L * n_samples); y.sum = out.add(L * 4); y.status = out.add(L * 4);
    y.in_used = in.end; y.out_used = out.end;
    return y;
}
// in: the members | begin, out_off (int64) | csize, isize (int32).  out: the inflated bytes | statuses (int32)
struct InflateLayout { int64_t in_sum, begin, out_off, csize, isize, in_used, out_bytes, status, out_used; };
static inline InflateLayout inflate_layout(int64_t in_sum, int64_t out_sum, int64_t n_members) {
    InflateLayout y; Sections in, out; const int64_t L = n_members;
    in.add(y.in_sum = in_sum); y.begin = in.add(L * 8); y.out_off = in.add(L * 8); y.csize = in.add(L * 4); y.isize = in.add(L * 4);
    out.add(y.out_bytes = out_sum); y.status = out.add(L * 4);
    y.in_used = in.end; y.out_used = out.end;
    return y;
}

// Two slots taken in turn: a batch is enqueued into s[next] and its ticket is that index; a slot is free again when its ticket was
// waited for.  `who` is the family's name, "vgl_vcfin_host"
template <typename Slot> struct Ring {
    Slot s[2];
    int next = 0;
    int acquire(const char* who) const {                                                    // is cur() free for the next batch?
        return s[next].busy ? fail(VGL_E_ARG, "%s_submit: two batches are in flight (%s_wait the older one first)", who, who) : VGL_OK;
    }
    Slot& cur() { return s[next]; }
    int commit() { const int k = next; s[k].busy = true; next = k ^ 1; return k; }          // cur() is in flight: its ticket
    bool ticket_ok(int ticket) const { return ticket >= 0 && ticket <= 1 && s[ticket].busy; }
    bool release(int ticket) { if (!ticket_ok(ticket)) return false; s[ticket].busy = false; return true; }
};

// a slot of the three input families: page-locked staging and its device twin, one copy up and one copy down; lay = where the
// batch in flight has its sections
template <typename Lay> struct StagedSlot {
    PinBuf<uint8_t> h_in, h_out; DevBuf<uint8_t> d_in, d_out;
    Lay lay{}; bool busy = false;
};
template <typename Lay> struct StagedRing : Ring<StagedSlot<Lay>> {
    int reserve(int64_t in_bytes, int64_t out_bytes) {
        for (auto& S : this->s) {
            VGLCHK(S.d_in.reserve((size_t)in_bytes)); VGLCHK(S.d_out.reserve((size_t)out_bytes));
            VGLCHK(S.h_in.reserve((size_t)in_bytes)); VGLCHK(S.h_out.reserve((size_t)out_bytes));
        }
        return VGL_OK;
    }
};

struct BgzfSlot { DevBuf<uint8_t> d_in, d_out; PinBuf<uint8_t> h_out; int64_t n = 0; bool busy = false; };
struct BgzfRing : Ring<BgzfSlot> {
    DevBuf<uint8_t> ws; DevBuf<int64_t> d_n; PinBuf<int64_t> h_n;          // the compressor's workspace; the compressed length of each slot
    int reserve(int64_t max_batch, int64_t out_cap, int64_t ws_bytes) {
        VGLCHK(ws.reserve((size_t)ws_bytes)); VGLCHK(d_n.reserve(2)); VGLCHK(h_n.reserve(2));
        for (auto& S : s) { VGLCHK(S.d_in.reserve((size_t)max_batch)); VGLCHK(S.d_out.reserve((size_t)out_cap)); VGLCHK(S.h_out.reserve((size_t)out_cap)); }
        return VGL_OK;
    }
};

// The stream handle: the caller names the buffer, so a ticket is the buffer's index; the assembled stream and the BGZF workspace are
// shared by the buffers (one HIP stream orders their work), hence tickets are waited for in submit order
constexpr int STREAM_MAX_BUFFERS = 8;
struct StreamBuf {
    DevBuf<uint8_t> d_body, d_heads, d_mem; DevBuf<int64_t> d_off, d_n;    // d_off: head offsets, then body offsets; d_n: {assembled total, compressed length}
    PinBuf<uint8_t> h_heads, h_mem; PinBuf<int64_t> h_off, h_n;            // h_mem grows to what the members take (page-locking is not free)
    int64_t raw = 0, seq = 0; bool busy = false;
};
struct StreamSlots {
    int nb = 0;
    StreamBuf b[STREAM_MAX_BUFFERS];
    DevBuf<uint8_t> d_stream, ws;
    int64_t next_seq = 0, wait_seq = 0;
    int reserve(int n_buffers, int64_t max_sites, int64_t max_head, int64_t max_body, int64_t ws_bytes, int64_t out_cap) {
        nb = n_buffers;
        VGLCHK(d_stream.reserve((size_t)(max_head + max_body))); VGLCHK(ws.reserve((size_t)ws_bytes));
        const size_t offs = 2 * ((size_t)max_sites + 1);
        for (int k = 0; k < nb; k++) {
            StreamBuf& B = b[k];
            VGLCHK(B.d_body.reserve((size_t)max_body)); VGLCHK(B.d_heads.reserve((size_t)max_head)); VGLCHK(B.d_off.reserve(offs));
            VGLCHK(B.h_heads.reserve((size_t)max_head)); VGLCHK(B.h_off.reserve(offs)); VGLCHK(B.d_mem.reserve((size_t)out_cap));
            VGLCHK(B.d_n.reserve(2)); VGLCHK(B.h_n.reserve(2));
        }
        return VGL_OK;
    }
    bool in_range(int k) const { return k >= 0 && k < nb; }
    void commit(int k, int64_t raw) { b[k].raw = raw; b[k].seq = next_seq++; b[k].busy = true; }
    int ticket_ok(int ticket) const {
        if (!in_range(ticket) || !b[ticket].busy) return fail(VGL_E_ARG, "vgl_stream_host_wait: bad ticket");
        if (b[ticket].seq != wait_seq) return fail(VGL_E_ARG, "vgl_stream_host_wait: tickets are waited for in submit order");
        return VGL_OK;
    }
    void release(int ticket) { b[ticket].busy = false; wait_seq++; }
};
// page-locked room for m bytes of members: a quarter more than asked for, a MiB at least, never above what a batch can take
static inline int64_t stream_members_room(int64_t m, int64_t out_cap) { return std::min(out_cap, std::max<int64_t>(m + m / 4, 1 << 20)); }


#ifndef VGL_MEM_TEST
// ---- HIP layer ------------------------------------------------------------------------------------------------------------------
static int pick_device(const char* who, int device) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return fail(VGL_E_NODEVICE, "%s: no HIP device is available", who);
    if (device < 0 || device >= nd) return fail(VGL_E_NODEVICE, "%s: no such device", who);
    if (hipSetDevice(device) != hipSuccess) return fail(VGL_E_NODEVICE, "%s: hipSetDevice failed", who);
    return VGL_OK;
}
// a failure whose text an owner or HIPCHK wrote ("... of N bytes: ..."): the entry point's name in front of it
static int named(const char* who, int rc) {
    if (rc == VGL_OK) return rc;
    const std::string text = g_err;
    return fail(rc, "%s: %s", who, text.c_str());
}

// What every handle has.  st: the batches' work; cp (bgzf, stream): copies of finished batches back to the host.  A handle is
// created into a unique_ptr and destroyed by batch_destroy: the owners free what it holds
struct BatchHost {
    int device = 0;
    Stream st, cp;
    Event done[STREAM_MAX_BUFFERS];                      // one per slot
    int open(int dev, int n_slots, bool copy_stream) {
        device = dev;
        VGLCHK(st.create());
        if (copy_stream) VGLCHK(cp.create());
        for (int k = 0; k < n_slots; k++) VGLCHK(done[k].create());
        return VGL_OK;
    }
    // once something is enqueued a failure waits for the stream: the slot stays free, so whatever already runs must be over before
    // the caller can submit again and overwrite the page-locked staging.  The message stands
    int failed(int rc) const { (void)hipStreamSynchronize(st); return rc; }
};
template <typename H> static int batch_destroy(H* h) {
    if (!h) return VGL_OK;
    (void)hipSetDevice(h->device);
    if (h->st.s) (void)hipStreamSynchronize(h->st);
    if (h->cp.s) (void)hipStreamSynchronize(h->cp);
    delete h;
    return VGL_OK;
}

// The three input families.  H has `name` and `ring`, a StagedRing.  create: the handle, its limits set, gets its device objects
template <typename H> static int staged_create(std::unique_ptr<H> h, int device, int64_t in_cap, int64_t out_cap, H** out) {
    const std::string who = std::string(H::name) + "_create";
    VGLCHK(named(who.c_str(), h->open(device, 2, false)));
    VGLCHK(named(who.c_str(), h->ring.reserve(in_cap, out_cap)));
    *out = h.release();
    return VGL_OK;
}
// submit, first half: ring.cur() is free and the device is set; a refused batch has left the staging as it was
template <typename H> static int staged_acquire(H* h) {
    VGLCHK(h->ring.acquire(H::name));
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "%s_submit: hipSetDevice failed", H::name);
    return VGL_OK;
}
// submit, second half: the caller has filled ring.cur()'s staging as cur().lay says.  One copy up, launch(slot), one copy down; an
// empty batch records its event without a launch
template <typename H, typename Launch> static int staged_enqueue(H* h, int64_t n, int32_t* ticket, Launch launch) {
    auto& S = h->ring.cur();
    const char* what = nullptr;
    if (n > 0) {
        if (hipMemcpyAsync(S.d_in, S.h_in, (size_t)S.lay.in_used, hipMemcpyHostToDevice, h->st) != hipSuccess) what = "copy to the device failed";
        else if (launch(S) != 0) what = "the launch failed";
        else if (hipMemcpyAsync(S.h_out, S.d_out, (size_t)S.lay.out_used, hipMemcpyDeviceToHost, h->st) != hipSuccess) what = "copy back failed";
    }
    if (!what && hipEventRecord(h->done[h->ring.next], h->st) != hipSuccess) what = "enqueue failed";
    if (what) return h->failed(fail(VGL_E_NODEVICE, "%s_submit: %s", H::name, what));
    *ticket = h->ring.commit();
    return VGL_OK;
}
// wait: the ticket's slot, finished and free again; `what`: "the parse failed"
template <typename H> static int staged_wait(H* h, int32_t ticket, bool args_ok, const char* what) {
    if (!h || !args_ok || !h->ring.ticket_ok(ticket)) return fail(VGL_E_ARG, "%s_wait: bad ticket", H::name);
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "%s_wait: hipSetDevice failed", H::name);
    if (hipEventSynchronize(h->done[ticket]) != hipSuccess) return fail(VGL_E_NODEVICE, "%s_wait: %s", H::name, what);
    h->ring.release(ticket);
    return VGL_OK;
}

// ---- vgl_vcfin_host_* -----------------------------------------------------------------------------------------------------------
struct vgl_vcfin_host : BatchHost {
    static constexpr const char* name = "vgl_vcfin_host";
    int32_t N = 0, max_lines = 0; int64_t max_text = 0;
    StagedRing<VcfinLayout> ring;
};

extern "C" int vgl_vcfin_host_create(int32_t device, int32_t n_samples, int32_t max_lines, int64_t max_text_bytes, vgl_vcfin_host** out) {
    if (!out || n_samples <= 0 || max_lines <= 0 || max_text_bytes <= 0) return fail(VGL_E_ARG, "vgl_vcfin_host_create: bad argument");
    *out = nullptr;
    VGLCHK(pick_device("vgl_vcfin_host_create", device));
    std::unique_ptr<vgl_vcfin_host> h(new vgl_vcfin_host);
    h->N = n_samples; h->max_lines = max_lines; h->max_text = max_text_bytes;
    const VcfinLayout cap = vcfin_layout(max_text_bytes, max_lines, n_samples);
    return staged_create(std::move(h), device, cap.in_used, cap.out_used, out);
}

extern "C" int vgl_vcfin_host_submit(vgl_vcfin_host* h, const uint8_t* text, int64_t text_bytes, int32_t n_lines, const int64_t* line_begin,
                                     const int64_t* line_end, const int32_t* gti, const int32_t* n_alleles, const int8_t* allele_map, int32_t* ticket) {
    if (!h || !ticket || n_lines < 0 || n_lines > h->max_lines || text_bytes < 0 || text_bytes > h->max_text ||
        (n_lines > 0 && (!text || !line_begin || !line_end || !gti || !n_alleles || !allele_map)))
        return fail(VGL_E_ARG, "vgl_vcfin_host_submit: bad argument");
    for (int32_t i = 0; i < n_lines; i++)
        if (line_begin[i] < 0 || line_begin[i] > line_end[i] || line_end[i] > text_bytes)
            return fail(VGL_E_ARG, "vgl_vcfin_host_submit: a line range lies outside the text (0 <= line_begin <= line_end <= text_bytes)");
    VGLCHK(staged_acquire(h));
    if (n_lines > 0) {                                   // the batch's text and arrays lie back to back in the staging, sized by n_lines
        auto& S = h->ring.cur();
        const VcfinLayout& y = S.lay = vcfin_layout(text_bytes, n_lines, h->N);
        const size_t L = (size_t)n_lines;
        memcpy(S.h_in, text, (size_t)text_bytes);
        memcpy(S.h_in + y.lb, line_begin, L * 8); memcpy(S.h_in + y.le, line_end, L * 8);
        memcpy(S.h_in + y.gti, gti, L * 4); memcpy(S.h_in + y.nal, n_alleles, L * 4);
        memcpy(S.h_in + y.map, allele_map, L * 5);
    }
    return staged_enqueue(h, n_lines, ticket, [&](const StagedSlot<VcfinLayout>& S) {
        const uint8_t* in = S.d_in; uint8_t* o = S.d_out; const VcfinLayout& y = S.lay;
        const VglVcfinArgs A{in, text_bytes, n_lines, h->N, (const int64_t*)(in + y.lb), (const int64_t*)(in + y.le), (const int32_t*)(in + y.gti),
                             (const int32_t*)(in + y.nal), (const int8_t*)(in + y.map), o, (int32_t*)(o + y.sum), (int32_t*)(o + y.status)};
        return vgl_launch_vcfin_parse(&A, h->st);
    });
}

extern "C" int vgl_vcfin_host_wait(vgl_vcfin_host* h, int32_t ticket, const uint8_t** gt, const int32_t** allelesum, const int32_t** status) {
    VGLCHK(staged_wait(h, ticket, gt && allelesum && status, "the parse failed"));
    const auto& S = h->ring.s[ticket];
    *gt = S.h_out; *allelesum = (const int32_t*)(S.h_out + S.lay.sum); *status = (const int32_t*)(S.h_out + S.lay.status);
    return VGL_OK;
}
extern "C" int vgl_vcfin_host_destroy(vgl_vcfin_host* h) { return batch_destroy(h); }

// ---- vgl_bcfin_host_*: vgl_vcfin_host_* for BCF records; submit takes the buffer that holds the records -------------------------
struct vgl_bcfin_host : BatchHost {
    static constexpr const char* name = "vgl_bcfin_host";
    int32_t N = 0, max_records = 0; int64_t max_gt = 0;
    StagedRing<BcfinLayout> ring;
};

extern "C" int vgl_bcfin_host_create(int32_t device, int32_t n_samples, int32_t max_records, int64_t max_gt_bytes, vgl_bcfin_host** out) {
    if (!out || n_samples <= 0 || max_records <= 0 || max_gt_bytes <= 0) return fail(VGL_E_ARG, "vgl_bcfin_host_create: bad argument");
    *out = nullptr;
    VGLCHK(pick_device("vgl_bcfin_host_create", device));
    std::unique_ptr<vgl_bcfin_host> h(new vgl_bcfin_host);
    h->N = n_samples; h->max_records = max_records; h->max_gt = max_gt_bytes;
    const BcfinLayout cap = bcfin_layout(max_gt_bytes, max_records, n_samples);
    return staged_create(std::move(h), device, cap.in_used, cap.out_used, out);
}

extern "C" int vgl_bcfin_host_submit(vgl_bcfin_host* h, const uint8_t* src, int64_t src_bytes, int32_t n_records, const int64_t* gt_begin,
                                     const int32_t* gt_type, const int32_t* gt_n, const int32_t* n_alleles, const int8_t* allele_map, int32_t* ticket) {
    if (!h || !ticket || n_records < 0 || n_records > h->max_records || src_bytes < 0 ||
        (n_records > 0 && (!src || !gt_begin || !gt_type || !gt_n || !n_alleles || !allele_map)))
        return fail(VGL_E_ARG, "vgl_bcfin_host_submit: bad argument");
    // only the GT slices go into the staging, back to back: what lies between them in src (the other FORMAT fields, the shared blocks)
    // never crosses the link.  First their ranges and their total, so that a refused batch leaves the staging as it was
    auto slice_len = [&](int32_t i) { const int w = vgl_bcfin::width(gt_type[i]); return (w != 0 && gt_n[i] >= 1) ? (int64_t)h->N * gt_n[i] * w : 0; };
    int64_t total = 0;
    for (int32_t i = 0; i < n_records; i++) {
        if (!vgl_bcfin::slice_ok(gt_begin[i], vgl_bcfin::width(gt_type[i]), gt_n[i], h->N, src_bytes))
            return fail(VGL_E_ARG, "vgl_bcfin_host_submit: a GT slice lies outside the bytes (0 <= gt_begin, gt_begin + n_samples * n * width <= src_bytes)");
        total += slice_len(i);
        if (total > h->max_gt) return fail(VGL_E_ARG, "vgl_bcfin_host_submit: the batch's GT slices exceed max_gt_bytes");
    }
    VGLCHK(staged_acquire(h));
    if (n_records > 0) {
        auto& S = h->ring.cur();
        const BcfinLayout& y = S.lay = bcfin_layout(total, n_records, h->N);
        const size_t L = (size_t)n_records;
        int64_t* packed = (int64_t*)(S.h_in + y.beg);
        int64_t at = 0;
        for (int32_t i = 0; i < n_records; i++) {
            const int64_t len = slice_len(i);
            packed[i] = at;
            if (len > 0) memcpy(S.h_in + at, src + gt_begin[i], (size_t)len);
            at += len;
        }
        memcpy(S.h_in + y.type, gt_type, L * 4); memcpy(S.h_in + y.n, gt_n, L * 4);
        memcpy(S.h_in + y.nal, n_alleles, L * 4); memcpy(S.h_in + y.map, allele_map, L * 5);
    }
    return staged_enqueue(h, n_records, ticket, [&](const StagedSlot<BcfinLayout>& S) {
        const uint8_t* in = S.d_in; uint8_t* o = S.d_out; const BcfinLayout& y = S.lay;
        const VglBcfinArgs A{in, total, n_records, h->N, (const int64_t*)(in + y.beg), (const int32_t*)(in + y.type), (const int32_t*)(in + y.n),
                             (const int32_t*)(in + y.nal), (const int8_t*)(in + y.map), o, (int32_t*)(o + y.sum), (int32_t*)(o + y.status)};
        return vgl_launch_bcfin_decode(&A, h->st);
    });
}

extern "C" int vgl_bcfin_host_wait(vgl_bcfin_host* h, int32_t ticket, const uint8_t** gt, const int32_t** allelesum, const int32_t** status) {
    VGLCHK(staged_wait(h, ticket, gt && allelesum && status, "the decode failed"));
    const auto& S = h->ring.s[ticket];
    *gt = S.h_out; *allelesum = (const int32_t*)(S.h_out + S.lay.sum); *status = (const int32_t*)(S.h_out + S.lay.status);
    return VGL_OK;
}
extern "C" int vgl_bcfin_host_destroy(vgl_bcfin_host* h) { return batch_destroy(h); }

// ---- vgl_inflate_host_* ---------------------------------------------------------------------------------------------------------
struct vgl_inflate_host : BatchHost {
    static constexpr const char* name = "vgl_inflate_host";
    int32_t max_members = 0;
    StagedRing<InflateLayout> ring;
};

extern "C" int vgl_inflate_host_create(int32_t device, int32_t max_members, vgl_inflate_host** out) {
    if (!out || max_members <= 0 || max_members > (1 << 20)) return fail(VGL_E_ARG, "vgl_inflate_host_create: bad argument");
    *out = nullptr;
    VGLCHK(pick_device("vgl_inflate_host_create", device));
    std::unique_ptr<vgl_inflate_host> h(new vgl_inflate_host);
    h->max_members = max_members;
    const int64_t M = max_members;
    const InflateLayout cap = inflate_layout(M * 65536, M * 65536, M);          // (a member is at most 65536 bytes either way)
    return staged_create(std::move(h), device, cap.in_used, cap.out_used, out);
}

extern "C" int vgl_inflate_host_submit(vgl_inflate_host* h, const uint8_t* src, int64_t src_bytes, int32_t n_members, const int64_t* begin,
                                       const int32_t* csize, const int32_t* isize, int32_t* ticket) {
    if (!h || !ticket || n_members < 0 || n_members > h->max_members || src_bytes < 0 || (n_members > 0 && (!src || !begin || !csize || !isize)))
        return fail(VGL_E_ARG, "vgl_inflate_host_submit: bad argument");
    int64_t in_sum = 0, out_sum = 0;
    for (int32_t i = 0; i < n_members; i++) {
        if (begin[i] < 0 || csize[i] < 0 || csize[i] > 65536 || begin[i] > src_bytes || csize[i] > src_bytes - begin[i] || isize[i] < 0 || isize[i] > 65536)
            return fail(VGL_E_ARG, "vgl_inflate_host_submit: a member's range lies outside src, or its csize or isize is not in 0 .. 65536");
        in_sum += csize[i]; out_sum += isize[i];
    }
    VGLCHK(staged_acquire(h));
    auto& S = h->ring.cur();
    const InflateLayout& y = S.lay = inflate_layout(in_sum, out_sum, n_members);
    if (n_members > 0) {                                 // the members are packed back to back into the staging, their arrays behind them
        const size_t L = (size_t)n_members;
        int64_t* sb = (int64_t*)(S.h_in + y.begin); int64_t* so = (int64_t*)(S.h_in + y.out_off);
        int64_t at = 0, oat = 0;
        for (int32_t i = 0; i < n_members; i++) {
            memcpy(S.h_in + at, src + begin[i], (size_t)csize[i]);
            sb[i] = at; so[i] = oat; at += csize[i]; oat += isize[i];
        }
        memcpy(S.h_in + y.csize, csize, L * 4); memcpy(S.h_in + y.isize, isize, L * 4);
    }
    return staged_enqueue(h, n_members, ticket, [&](const StagedSlot<InflateLayout>& S) {
        const uint8_t* in = S.d_in; uint8_t* o = S.d_out;
        const VglInflateArgs A{in, in_sum, n_members, (const int64_t*)(in + y.begin), (const int32_t*)(in + y.csize), (const int64_t*)(in + y.out_off),
                               (const int32_t*)(in + y.isize), o, out_sum, (int32_t*)(o + y.status)};
        return vgl_launch_inflate_members(&A, h->st);
    });
}

extern "C" int vgl_inflate_host_wait(vgl_inflate_host* h, int32_t ticket, const uint8_t** out, int64_t* out_bytes, const int32_t** status) {
    VGLCHK(staged_wait(h, ticket, out && out_bytes && status, "the batch failed"));
    const auto& S = h->ring.s[ticket];
    *out = S.h_out; *out_bytes = S.lay.out_bytes; *status = (const int32_t*)(S.h_out + S.lay.status);
    return VGL_OK;
}
extern "C" int vgl_inflate_host_destroy(vgl_inflate_host* h) { return batch_destroy(h); }

// ---- vgl_bgzf_host_* ------------------------------------------------------------------------------------------------------------
struct vgl_bgzf_host : BatchHost {
    int64_t cap = 0, ws_bytes = 0;
    BgzfRing ring;
};

extern "C" int vgl_bgzf_host_create(int32_t device, int64_t max_batch, vgl_bgzf_host** out) {
    if (!out || max_batch <= 0) return fail(VGL_E_ARG, "vgl_bgzf_host_create: bad argument");
    *out = nullptr;
    VGLCHK(pick_device("vgl_bgzf_host_create", device));
    std::unique_ptr<vgl_bgzf_host> h(new vgl_bgzf_host);
    h->cap = max_batch; h->ws_bytes = vgl_bgzf_workspace_bytes(max_batch);
    VGLCHK(named("vgl_bgzf_host_create", h->open(device, 2, true)));
    VGLCHK(named("vgl_bgzf_host_create", h->ring.reserve(max_batch, vgl_bgzf_bound(max_batch), h->ws_bytes)));
    *out = h.release();
    return VGL_OK;
}

extern "C" int vgl_bgzf_host_submit(vgl_bgzf_host* h, const uint8_t* src, int64_t n, int32_t* ticket) {
    if (!h || !ticket || n < 0 || n > h->cap || (n > 0 && !src)) return fail(VGL_E_ARG, "vgl_bgzf_host_submit: bad argument");
    VGLCHK(h->ring.acquire("vgl_bgzf_host"));
    const int k = h->ring.next;
    auto& S = h->ring.cur();
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_bgzf_host_submit: hipSetDevice failed");
    if (n > 0 && hipMemcpyAsync(S.d_in, src, (size_t)n, hipMemcpyHostToDevice, h->st) != hipSuccess)
        return h->failed(fail(VGL_E_NODEVICE, "vgl_bgzf_host_submit: copy to the device failed"));
    const int rc = vgl_bgzf_compress_device(h->device, S.d_in, n, S.d_out, vgl_bgzf_bound(h->cap), h->ring.d_n + k, h->ring.ws, h->ws_bytes, h->st);
    if (rc != VGL_OK) return h->failed(rc);
    if (hipMemcpyAsync(h->ring.h_n + k, h->ring.d_n + k, sizeof(int64_t), hipMemcpyDeviceToHost, h->st) != hipSuccess || hipEventRecord(h->done[k], h->st) != hipSuccess)
        return h->failed(fail(VGL_E_NODEVICE, "vgl_bgzf_host_submit: enqueue failed"));
    S.n = n;
    *ticket = h->ring.commit();
    return VGL_OK;
}

extern "C" int vgl_bgzf_host_wait(vgl_bgzf_host* h, int32_t ticket, const uint8_t** out, int64_t* out_n) {
    if (!h || !out || !out_n || !h->ring.ticket_ok(ticket)) return fail(VGL_E_ARG, "vgl_bgzf_host_wait: bad ticket");
    auto& S = h->ring.s[ticket];
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_bgzf_host_wait: hipSetDevice failed");
    if (hipEventSynchronize(h->done[ticket]) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_bgzf_host_wait: the compression failed");   // (not the stream: the next batch may run behind it)
    const int64_t m = h->ring.h_n[ticket];
    if (m < 0 || m > vgl_bgzf_bound(S.n)) return fail(VGL_E_NODEVICE, "vgl_bgzf_host_wait: compressed size out of range");
    if (m > 0 && (hipMemcpyAsync(S.h_out, S.d_out, (size_t)m, hipMemcpyDeviceToHost, h->cp) != hipSuccess || hipStreamSynchronize(h->cp) != hipSuccess))
        return fail(VGL_E_NODEVICE, "vgl_bgzf_host_wait: copy back failed");
    h->ring.release(ticket);
    *out = S.h_out; *out_n = m;
    return VGL_OK;
}
extern "C" int vgl_bgzf_host_destroy(vgl_bgzf_host* h) { return batch_destroy(h); }

// ---- vgl_stream_host_*: what the host program's writer thread uses --------------------------------------------------------------
struct vgl_stream_host : BatchHost {
    int32_t max_sites = 0;
    int64_t max_head = 0, max_body = 0, ws_bytes = 0, out_cap = 0;
    StreamSlots slots;
};

extern "C" int vgl_stream_host_create(int32_t device, int32_t n_buffers, int32_t max_sites, int64_t max_head_bytes, int64_t max_body_bytes,
                                      vgl_stream_host** out) {
    if (!out) return fail(VGL_E_ARG, "vgl_stream_host_create: null out");
    *out = nullptr;
    if (n_buffers < 1 || n_buffers > STREAM_MAX_BUFFERS) return fail(VGL_E_ARG, "vgl_stream_host_create: n_buffers outside [1, 8]");
    if (max_sites < 1) return fail(VGL_E_ARG, "vgl_stream_host_create: max_sites below 1");
    if (max_head_bytes < 1) return fail(VGL_E_ARG, "vgl_stream_host_create: max_head_bytes below 1");
    if (max_body_bytes < 1) return fail(VGL_E_ARG, "vgl_stream_host_create: max_body_bytes below 1");
    VGLCHK(pick_device("vgl_stream_host_create", device));
    std::unique_ptr<vgl_stream_host> h(new vgl_stream_host);
    h->max_sites = max_sites; h->max_head = max_head_bytes; h->max_body = max_body_bytes;
    const int64_t cap = max_head_bytes + max_body_bytes;
    h->ws_bytes = vgl_bgzf_workspace_bytes(cap); h->out_cap = vgl_bgzf_bound(cap);
    VGLCHK(named("vgl_stream_host_create", h->open(device, n_buffers, true)));
    VGLCHK(named("vgl_stream_host_create", h->slots.reserve(n_buffers, max_sites, max_head_bytes, max_body_bytes, h->ws_bytes, h->out_cap)));
    *out = h.release();
    return VGL_OK;
}

extern "C" uint8_t* vgl_stream_host_body(vgl_stream_host* h, int32_t k) {
    if (!h || !h->slots.in_range(k)) { fail(VGL_E_ARG, "vgl_stream_host_body: k is out of range"); return nullptr; }
    return h->slots.b[k].d_body;
}

extern "C" int vgl_stream_host_submit(vgl_stream_host* h, int32_t k, int32_t n_sites, const uint8_t* heads, const int64_t* head_offsets,
                                      const int64_t* body_offsets, int32_t* ticket) {
    if (!h || !ticket) return fail(VGL_E_ARG, "vgl_stream_host_submit: null handle or ticket");
    if (!h->slots.in_range(k)) return fail(VGL_E_ARG, "vgl_stream_host_submit: k is out of range");
    StreamBuf& B = h->slots.b[k];
    if (B.busy) return fail(VGL_E_ARG, "vgl_stream_host_submit: buffer k is still in flight (vgl_stream_host_wait its ticket first)");
    if (n_sites < 0 || n_sites > h->max_sites) return fail(VGL_E_ARG, "vgl_stream_host_submit: n_sites outside [0, max_sites]");
    int64_t hb = 0, bb = 0;
    if (n_sites > 0) {
        if (!head_offsets) return fail(VGL_E_ARG, "vgl_stream_host_submit: null head_offsets");
        if (!body_offsets) return fail(VGL_E_ARG, "vgl_stream_host_submit: null body_offsets");
        for (int32_t i = 0; i < n_sites; i++) {
            if (head_offsets[i + 1] < head_offsets[i]) return fail(VGL_E_ARG, "vgl_stream_host_submit: head_offsets is not monotone");
            if (body_offsets[i + 1] < body_offsets[i]) return fail(VGL_E_ARG, "vgl_stream_host_submit: body_offsets is not monotone");
        }
        hb = head_offsets[n_sites] - head_offsets[0]; bb = body_offsets[n_sites] - body_offsets[0];
        if (hb > h->max_head) return fail(VGL_E_ARG, "vgl_stream_host_submit: head_offsets spans more than max_head_bytes");
        if (body_offsets[0] < 0 || body_offsets[n_sites] > h->max_body) return fail(VGL_E_ARG, "vgl_stream_host_submit: body_offsets leaves the body buffer (max_body_bytes)");
        if (hb > 0 && !heads) return fail(VGL_E_ARG, "vgl_stream_host_submit: null heads");
    }
    const int64_t raw = hb + bb;
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_stream_host_submit: hipSetDevice failed");
    B.h_n[0] = 0; B.h_n[1] = 0;
    if (raw > 0) {
        // the caller's arrays are free again when this returns: page-locked copies go up the link
        const size_t no = (size_t)n_sites + 1;
        memcpy(B.h_off, head_offsets, no * sizeof(int64_t));
        memcpy(B.h_off + no, body_offsets, no * sizeof(int64_t));
        if (hb > 0) memcpy(B.h_heads, heads + head_offsets[0], (size_t)hb);
        bool ok = hipMemcpyAsync(B.d_off, B.h_off, 2 * no * sizeof(int64_t), hipMemcpyHostToDevice, h->st) == hipSuccess;
        if (hb > 0) ok = ok && hipMemcpyAsync(B.d_heads, B.h_heads, (size_t)hb, hipMemcpyHostToDevice, h->st) == hipSuccess;
        if (!ok) return h->failed(fail(VGL_E_NODEVICE, "vgl_stream_host_submit: copy to the device failed"));
        int rc = vgl_stream_assemble_device(h->device, n_sites, B.d_heads, B.d_off, B.d_body + body_offsets[0], B.d_off + no, h->slots.d_stream, raw, B.d_n, h->st);
        if (rc == VGL_OK) rc = vgl_bgzf_compress_device(h->device, h->slots.d_stream, raw, B.d_mem, h->out_cap, B.d_n + 1, h->slots.ws, h->ws_bytes, h->st);
        if (rc != VGL_OK) return h->failed(rc);
        if (hipMemcpyAsync(B.h_n, B.d_n, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->st) != hipSuccess)
            return h->failed(fail(VGL_E_NODEVICE, "vgl_stream_host_submit: enqueue failed"));
    }
    if (hipEventRecord(h->done[k], h->st) != hipSuccess) return h->failed(fail(VGL_E_NODEVICE, "vgl_stream_host_submit: enqueue failed"));
    h->slots.commit(k, raw);
    *ticket = k;
    return VGL_OK;
}

extern "C" int vgl_stream_host_wait(vgl_stream_host* h, int32_t ticket, const uint8_t** members, int64_t* members_n, int64_t* raw_n) {
    if (!h || !members || !members_n) return fail(VGL_E_ARG, "vgl_stream_host_wait: null argument");
    VGLCHK(h->slots.ticket_ok(ticket));
    StreamBuf& B = h->slots.b[ticket];
    if (hipSetDevice(h->device) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_stream_host_wait: hipSetDevice failed");
    if (hipEventSynchronize(h->done[ticket]) != hipSuccess) return fail(VGL_E_NODEVICE, "vgl_stream_host_wait: the assembly or compression failed");
    h->slots.release(ticket);
    int64_t m = 0;
    if (B.raw > 0) {
        m = B.h_n[1];
        if (B.h_n[0] != B.raw) return fail(VGL_E_NODEVICE, "vgl_stream_host_wait: the assembled length differs from the offsets' total");
        if (m <= 0 || m > vgl_bgzf_bound(B.raw)) return fail(VGL_E_NODEVICE, "vgl_stream_host_wait: compressed size out of range");
        if ((size_t)m > B.h_mem.cap) VGLCHK(named("vgl_stream_host_wait", B.h_mem.reserve((size_t)stream_members_room(m, h->out_cap))));
        if (hipMemcpyAsync(B.h_mem, B.d_mem, (size_t)m, hipMemcpyDeviceToHost, h->cp) != hipSuccess || hipStreamSynchronize(h->cp) != hipSuccess)
            return fail(VGL_E_NODEVICE, "vgl_stream_host_wait: copy back failed");
    }
    *members = B.h_mem; *members_n = m;
    if (raw_n) *raw_n = B.raw;
    return VGL_OK;
}
extern "C" int vgl_stream_host_destroy(vgl_stream_host* h) { return batch_destroy(h); }
#endif
