// hostlib/slot.h -- the host entry points: a tile submitted from host buffers (vgl_simulate_tile / _async / _text_async /
// _gvcf_async), its copies back, the rerun of a tile with a deeper draw on the sibling context, vgl_tile_wait.
// Part of the one translation unit vgl_host.cpp.
#pragma once

// the device planes a tile needs: those the caller wants back and those its side outputs are formatted from (bit f: FIELDS[f])
static uint32_t wanted_fields(const vgl_ctx* c, const HostSlot& S, vgl_tile_out* o) {
    // text: the planes of the formatted tags are computed on the device whether or not the caller also wants them back
    uint32_t mask = 0;
    if (S.text || S.gvcf) {
        vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
        const int nf = text_fields(c, tf, fid);
        for (int k = 0; k < nf; k++) mask |= 1u << fid[k];
        if (S.gvcf) mask |= 1u << 10 | 1u << 12;                       // (the blocker reads FORMAT/DP and PL)
    }
    if (S.pile) mask |= 1u << 10;                                      // (the pileup formatter reads FORMAT/DP)
    if (S.fetch) mask |= 1u << 11;                                     // (the fetch-GL formatter reads FORMAT/GL)
    if (S.setal && (o->pl_u8 || (mask >> 17 & 1u))) mask |= 1u << 10;  // (the one-byte PL is relabelled by FORMAT/DP == 0)
    if (S.setal) mask |= 1u << 0 | 1u << 1 | 1u << 3;
    if (S.inf) mask |= 1u << 0 | 1u << 1 | 1u << 2 | 1u << 3;          // (the fill writes all four per-site arrays)
    for (int f = 0; f < N_FIELDS; f++) if (field_ptr(o, f)) mask |= 1u << f;
    return mask;
}

// room on the device for everything the tile in S writes there; `d`: the arrays its kernels get
static int reserve_host_tile(vgl_ctx* c, HostSlot& S, int32_t n_sites, vgl_tile_out* o, vgl_tile_out& d) {
    const size_t N = c->dp.n_samples, M = (size_t)c->max_sites;
    S.dev_fields = wanted_fields(c, S, o);
    for (int f = 0; f < N_FIELDS; f++) {
        if (!(S.dev_fields >> f & 1u)) continue;
        const size_t need = field_bytes(c, f, M);
        if (S.d_out[f].cap < need) {
            VGLCHK(S.d_out[f].reserve(need));
            // VGL_LAYOUT_SAMPLE_MAJOR: the kernels write n_samples x nK(site) values of a slab, the copy below takes the slab whole --
            // what lies behind a record's array is then zeros from here, not another job's memory (once per buffer, not per tile)
            HIPCHK(hipMemsetAsync(S.d_out[f], 0, need, c->s_compute));
        }
    }
    d = slot_planes(c, S, S.dev_fields);
    // a pileup: the read dump (and, for --adjust-qs 4 with --error-qs 2, the error probabilities) on the device whether or not the
    // caller also wants them back -- at the caller's capacity when it asks for a dump, else at the context's staging capacity
    const bool pile_errp = S.pile && (c->p.adjust_qs & 4) && c->p.error_qs == 2;
    const int32_t dump_cap = ((o->reads || o->read_errp) && o->read_capacity > 0) ? o->read_capacity : (S.pile ? c->dp.read_cap : 0);
    if ((o->reads || S.pile) && dump_cap > 0) {
        VGLCHK(S.d_reads_out.reserve((size_t)dump_cap * M * N));
        d.reads = S.d_reads_out; d.read_capacity = dump_cap;
    }
    if ((o->read_errp || pile_errp) && dump_cap > 0) {
        VGLCHK(S.d_errp_out.reserve((size_t)dump_cap * M * N));
        d.read_errp = S.d_errp_out; d.read_capacity = dump_cap;
    }
    if (o->site_pick_err) {
        VGLCHK(S.d_pick_out.reserve(M));
        HIPCHK(hipMemsetAsync(S.d_pick_out, 0xFF, (size_t)n_sites * sizeof(double), c->s_compute));
        d.site_pick_err = S.d_pick_out;
    }
    if (S.text || S.gvcf)
        VGLCHK(S.rec.reserve(S.text_dev ? -1 : S.text_cap, M, std::max(vgl_text_workspace_bytes((int32_t)N, c->max_sites), vgl_bcf_workspace_bytes((int32_t)N, c->max_sites))));
    if (S.pile) VGLCHK(S.pil.reserve(S.pile->text_cap, M, vgl_pileup_workspace_bytes((int32_t)N, c->max_sites)));
    if (S.fetch) VGLCHK(S.fet.reserve(S.fetch->text_cap, M, vgl_fetchgl_workspace_bytes((int32_t)N, c->max_sites)));
    return VGL_OK;
}

// Host buffers in, host buffers out, asynchronously: the tile's kernels are enqueued on the context's compute stream, the copies of
// its tags back to the host on its copy stream behind them; with two tiles in flight the copies of tile t overlap the kernels of
// tile t + 1.  Destination buffers from vgl_host_alloc() (pinned) are written by DMA directly; pageable ones work, more slowly.
// the fallible part of vgl_simulate_tile_async, from the first enqueue on (its caller cleans up after a failure)
static int enqueue_host_tile(vgl_ctx* c, HostSlot& S, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o,
                             const int32_t* contig, const int64_t* pos0) {
    const size_t N = c->dp.n_samples;
    memcpy(S.h_gt, gt, (size_t)n_sites * N);
    HIPCHK(hipMemcpyAsync(S.d_gt, S.h_gt, (size_t)n_sites * N, hipMemcpyHostToDevice, c->s_compute));
    vgl_tile_out d;
    int rc = reserve_host_tile(c, S, n_sites, o, d);
    if (rc != VGL_OK) return rc;
    if (S.gvcf && (rc = stage_gvcf(c, S, n_sites, contig, pos0)) != VGL_OK) return rc;
    if ((rc = vgl_simulate_tile_device(c, site0, n_sites, S.d_gt, &d, c->s_compute))) return rc;
    if (S.inf && (rc = enqueue_true_values_rc(c, S)) != VGL_OK) return rc;
    if (S.setal && (rc = enqueue_setal(c, S, site0, n_sites, d, c->s_compute)) != VGL_OK) return rc;
    if (S.pile && (rc = enqueue_pileup(c, S, n_sites, d)) != VGL_OK) return rc;
    if (S.fetch && (rc = enqueue_fetchgl(c, S, n_sites)) != VGL_OK) return rc;
    // this tile's device error flags, then a clean word for the next tile
    HIPCHK(hipMemcpyAsync(S.h_flag, c->d_errflag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute));
    HIPCHK(hipMemsetAsync(c->d_errflag, 0, sizeof(uint32_t), c->s_compute));
    if (S.text && (rc = enqueue_text(c, S, n_sites)) != VGL_OK) return rc;
    if (S.gvcf && (rc = enqueue_gvcf(c, S, n_sites)) != VGL_OK) return rc;
    HIPCHK(hipEventRecord(S.ev_kernels, c->s_compute));
    HIPCHK(hipStreamWaitEvent(c->s_copy, S.ev_kernels, 0));
    for (int f = 0; f < N_FIELDS; f++)
        if (void* host = field_ptr(o, f)) HIPCHK(hipMemcpyAsync(host, S.d_out[f], field_bytes(c, f, (size_t)n_sites), hipMemcpyDeviceToHost, c->s_copy));
    if (d.reads && o->reads && o->read_capacity > 0) HIPCHK(hipMemcpyAsync(o->reads, d.reads, (size_t)o->read_capacity * n_sites * N, hipMemcpyDeviceToHost, c->s_copy));
    if (d.read_errp && o->read_errp && o->read_capacity > 0 && c->dp.error_qs == 2) HIPCHK(hipMemcpyAsync(o->read_errp, d.read_errp, (size_t)o->read_capacity * n_sites * N * sizeof(double), hipMemcpyDeviceToHost, c->s_copy));
    if (d.site_pick_err) HIPCHK(hipMemcpyAsync(o->site_pick_err, d.site_pick_err, (size_t)n_sites * sizeof(double), hipMemcpyDeviceToHost, c->s_copy));
    if (S.text) HIPCHK(hipMemcpyAsync(S.h_toff, S.rec.off, sizeof(int64_t) * ((size_t)n_sites + 1), hipMemcpyDeviceToHost, c->s_copy));
    if (S.gvcf && (rc = copy_gvcf_small(c, S, n_sites, c->s_copy)) != VGL_OK) return rc;
    if (S.pile) HIPCHK(hipMemcpyAsync(S.pile->offsets, S.pil.off, sizeof(int64_t) * ((size_t)n_sites + 1), hipMemcpyDeviceToHost, c->s_copy));
    if (S.fetch) HIPCHK(hipMemcpyAsync(S.fetch->offsets, S.fet.off, sizeof(int64_t) * ((size_t)n_sites + 1), hipMemcpyDeviceToHost, c->s_copy));
    HIPCHK(hipEventRecord(S.ev_copied, c->s_copy));
    return VGL_OK;
}

// The ticket and the slot are committed only when everything is enqueued: after a failure part-way the streams are drained, the
// sticky device error word is cleared and the slot is free again -- no later tile inherits this one's flags or shares its buffers
// with work still in flight.
struct GvcfReq { const int32_t* contig; const int64_t* pos0; const int32_t* dps; int32_t n_dps; vgl_gvcf_tile* g; };
static int tile_async(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o, int32_t* ticket,
                      uint8_t* text, int64_t text_cap, int64_t* toff, bool want_text, const GvcfReq* gq = nullptr) {
    if (!c || !o || !ticket) return fail(VGL_E_ARG, "null argument");
    vgl_pileup_tile* const pile = c->pile_next;                     // (taken by this call, whether it succeeds or not)
    c->pile_next = nullptr;
    vgl_fetchgl_tile* const fetch = c->fetch_next;                  // (likewise)
    c->fetch_next = nullptr;
    if (gq) {
        const vgl_gvcf_tile* g = gq->g;
        if (!g || !g->items || !g->record_offsets || !g->block_offsets || g->text_cap < 0 || (g->text_cap > 0 && !g->text) || gq->n_dps < 0 ||
            (gq->n_dps > 0 && !gq->dps) || (n_sites > 0 && (!gq->contig || !gq->pos0)))
            return fail(VGL_E_ARG, "vgl_simulate_tile_gvcf_async: null or bad argument");
        if (c->p.out_layout != VGL_LAYOUT_SAMPLE_MAJOR || !c->p.add_fmt_dp || !c->p.add_pl)
            return fail(VGL_E_ARG, "vgl_simulate_tile_gvcf_async: the context needs out_layout = VGL_LAYOUT_SAMPLE_MAJOR, add_fmt_dp and add_pl");
        text = g->text; text_cap = g->text_cap;
    }
    if (want_text && (!toff || text_cap < 0 || (text_cap > 0 && !text))) return fail(VGL_E_ARG, "vgl_simulate_tile_text_async: null text or offsets");
    if (want_text && c->p.out_layout != VGL_LAYOUT_SAMPLE_MAJOR) return fail(VGL_E_ARG, "vgl_simulate_tile_text_async: the context needs out_layout = VGL_LAYOUT_SAMPLE_MAJOR");
    if (n_sites < 0 || n_sites > c->max_sites) return fail(VGL_E_ARG, "n_sites %d exceeds max_sites_per_tile %d", n_sites, c->max_sites);
    if (n_sites > 0 && !gt) return fail(VGL_E_ARG, "null gt");
    if (c->true_values) {
        if (gq) return fail(VGL_E_ARG, "vgl_simulate_tile_gvcf_async: not supported while vgl_ctx_true_values is on (the reference writes no gVCF from true values)");
        if (pile) return fail(VGL_E_ARG, "vgl_ctx_pileup_next: not supported while vgl_ctx_true_values is on (no read is drawn: there is no pileup)");
        if (fetch) return fail(VGL_E_ARG, "vgl_ctx_fetchgl_next: not supported while vgl_ctx_true_values is on");
        VGLCHK(true_values_ctx_ok(c, "vgl_ctx_true_values is on"));
        VGLCHK(true_values_outputs_ok(o));
    }
    if (c->d_setal && gq) return fail(VGL_E_ARG, "vgl_simulate_tile_gvcf_async: not supported while vgl_ctx_set_alleles is set");
    if (c->d_setal && n_sites > 0 && (site0 < c->setal_first || site0 + n_sites > c->setal_first + c->setal_n))
        return fail(VGL_E_ARG, "the tile's sites %lld .. %lld are not all inside vgl_ctx_set_alleles' table (%lld .. %lld)", (long long)site0, (long long)(site0 + n_sites - 1),
                    (long long)c->setal_first, (long long)(c->setal_first + c->setal_n - 1));
    HIPCHK(hipSetDevice(c->device));
    const int k = c->next_slot;
    HostSlot& S = c->slot[k];
    if (S.busy) return fail(VGL_E_ARG, "two tiles are already in flight: vgl_tile_wait() the older one first");
    VGLCHK(c->s_compute.create()); VGLCHK(c->s_copy.create());
    VGLCHK(S.ev_kernels.create()); VGLCHK(S.ev_copied.create());
    const size_t N = c->dp.n_samples;
    VGLCHK(S.d_gt.reserve((size_t)c->max_sites * N)); VGLCHK(S.h_gt.reserve((size_t)c->max_sites * N)); VGLCHK(S.h_flag.reserve(1));
    S.rc = VGL_OK; *S.h_flag = 0;
    S.site0 = site0; S.n_sites = n_sites; S.o = *o;
    S.text = want_text; S.h_text = text; S.text_cap = text_cap; S.h_toff = toff;
    S.text_dev = want_text && c->text_dev;
    S.gvcf = gq != nullptr; S.h_gv = gq ? gq->g : nullptr;
    S.pile = pile;
    S.fetch = fetch;
    S.setal = c->d_setal && n_sites > 0;
    S.inf = c->true_values && n_sites > 0;
    if (S.inf) { VGLCHK(S.h_ibad.reserve(1)); *S.h_ibad = VGL_INF_NO_BAD_SITE; }
    if (pile) { const int rc = pileup_qual_char(c, &S.pile_qc); if (rc != VGL_OK) { S.pile = nullptr; S.fetch = nullptr; return rc; } }
    if (gq) S.dps.assign(gq->dps, gq->dps + gq->n_dps);
    if (want_text || gq || pile || fetch) VGLCHK(c->s_text.create());
    if (n_sites == 0) {
        if (want_text) toff[0] = 0;
        if (gq) { gq->g->record_offsets[0] = 0; gq->g->block_offsets[0] = 0; }
        if (pile) pile->offsets[0] = 0;
        if (fetch) fetch->offsets[0] = 0;
        HIPCHK(hipEventRecord(S.ev_copied, c->s_copy));
    } else {
        const int rc = enqueue_host_tile(c, S, site0, n_sites, gt, o, gq ? gq->contig : nullptr, gq ? gq->pos0 : nullptr);
        if (rc != VGL_OK) {
            char keep[sizeof g_err];
            memcpy(keep, g_err, sizeof keep);                        // the first error is the one to report
            (void)hipStreamSynchronize(c->s_compute);
            (void)hipStreamSynchronize(c->s_copy);
            (void)hipMemset(c->d_errflag, 0, sizeof(uint32_t));
            memcpy(g_err, keep, sizeof keep);
            return rc;
        }
    }
    *ticket = k; c->next_slot = k ^ 1;
    S.busy = true;
    return VGL_OK;
}

extern "C" int vgl_simulate_tile_async(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o, int32_t* ticket) {
    return tile_async(c, site0, n_sites, gt, o, ticket, nullptr, 0, nullptr, false);
}

extern "C" int vgl_simulate_tile_text_async(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o,
                                            uint8_t* text, int64_t text_cap, int64_t* offsets, int32_t* ticket) {
    return tile_async(c, site0, n_sites, gt, o, ticket, text, text_cap, offsets, true);
}

extern "C" int vgl_simulate_tile_gvcf_async(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, const int32_t* contig, const int64_t* pos0,
                                            const int32_t* dps, int32_t n_dps, vgl_tile_out* o, vgl_gvcf_tile* g, int32_t* ticket) {
    const GvcfReq q{contig, pos0, dps, n_dps, g};
    return tile_async(c, site0, n_sites, gt, o, ticket, nullptr, 0, nullptr, false, &q);
}

// A tile whose device flags report a draw deeper than the staging capacity, run again through the sibling context (host buffers: the slot's own copy of
// the genotypes, the caller's output arrays), VGL_DEEP_TILE_SITES sites at a time -- every tag array of a tile is site-major, so a sub-tile is a slice of
// it.  Returns VGL_E_CAPACITY (quietly) where that cannot be done: serial mode (the streams have moved on), a per-read dump (read-major planes of the
// caller's own capacity) or a pileup (formatted from such planes), a capacity already at the layout's maximum, or no memory for the sibling.
static int deep_ctx(vgl_ctx* c, HostSlot& S) {
    const VglDevParams& D = c->dp;
    if (D.serial || D.read_cap >= VGL_READ_CAP_MAX || (S.o.read_capacity > 0 && (S.o.reads || S.o.read_errp)) || S.pile) return VGL_E_CAPACITY;
    if (!c->deep) {
        vgl_params p = c->p;
        std::vector<double> depths; std::vector<int32_t> bins;
        if (c->depths_copy.size()) { depths = c->depths_copy; p.depths = depths.data(); }
        if (c->bins_copy.size()) { bins = c->bins_copy; p.qs_bins = bins.data(); }
        char keep[sizeof g_err];
        memcpy(keep, g_err, sizeof keep);
        const int rc = ctx_create_cap(&p, c->device, c->max_sites < VGL_DEEP_TILE_SITES ? c->max_sites : VGL_DEEP_TILE_SITES, &c->deep, VGL_READ_CAP_MAX);
        if (rc != VGL_OK) { c->deep = nullptr; memcpy(g_err, keep, sizeof keep); return VGL_E_CAPACITY; }
    }
    deep_share(c);
    return VGL_OK;
}
static int deep_rerun(vgl_ctx* c, HostSlot& S) {
    if (deep_ctx(c, S) != VGL_OK) return VGL_E_CAPACITY;
    const size_t N = (size_t)c->dp.n_samples;
    for (int32_t k = 0; k < S.n_sites; k += c->deep->max_sites) {
        const int32_t n = (S.n_sites - k < c->deep->max_sites) ? (S.n_sites - k) : c->deep->max_sites;
        vgl_tile_out o = S.o;
        for (int f = 0; f < N_FIELDS; f++)
            if (char* host = (char*)field_ptr(&S.o, f)) field_ptr(&o, f) = host + field_bytes(c, f, (size_t)k);
        if (o.site_pick_err) o.site_pick_err += k;
        const int rc = vgl_simulate_tile(c->deep, S.site0 + k, n, S.h_gt + (size_t)k * N, &o);
        if (rc != VGL_OK) return rc;                                 // (a draw beyond VGL_READ_CAP_MAX reads: VGL_E_CAPACITY after all)
    }
    c->deep_runs++;
    return VGL_OK;
}
// The same for a text tile: the sibling runs the sub-tiles into the slot's own device planes (the genotypes are still in S.d_gt), then
// the whole tile is formatted again and its per-site arrays and offsets copied again (compute stream, synchronously: a rare path).
static int deep_rerun_text(vgl_ctx* c, HostSlot& S) {
    if (deep_ctx(c, S) != VGL_OK) return VGL_E_CAPACITY;
    const size_t N = (size_t)c->dp.n_samples;
    for (int32_t k = 0; k < S.n_sites; k += c->deep->max_sites) {
        const int32_t n = (S.n_sites - k < c->deep->max_sites) ? (S.n_sites - k) : c->deep->max_sites;
        vgl_tile_out d = slot_planes(c, S, S.dev_fields, (size_t)k);
        if (S.o.site_pick_err && S.d_pick_out) d.site_pick_err = S.d_pick_out + k;
        int rc = vgl_simulate_tile_device(c->deep, S.site0 + k, n, S.d_gt + (size_t)k * N, &d, c->s_compute);
        if (rc == VGL_OK) rc = vgl_ctx_check(c->deep, c->s_compute);
        if (rc != VGL_OK) return rc;                                 // (a draw beyond VGL_READ_CAP_MAX reads: VGL_E_CAPACITY after all)
    }
    // relabelled again from the rerun's values
    if (S.setal) VGLCHK(enqueue_setal(c, S, S.site0, S.n_sites, slot_planes(c, S, S.dev_fields), c->s_compute));
    const int rc = S.gvcf ? enqueue_gvcf(c, S, S.n_sites) : S.text ? enqueue_text(c, S, S.n_sites) : VGL_OK;
    if (rc != VGL_OK) return rc;
    if (S.fetch) {                                                   // fetched again from the rerun's values: the first run's text is never delivered
        VGLCHK(enqueue_fetchgl(c, S, S.n_sites));
        HIPCHK(hipMemcpyAsync(S.fetch->offsets, S.fet.off, sizeof(int64_t) * ((size_t)S.n_sites + 1), hipMemcpyDeviceToHost, c->s_compute));
    }
    for (int f = 0; f < N_FIELDS; f++)
        if (void* host = field_ptr(&S.o, f)) HIPCHK(hipMemcpyAsync(host, S.d_out[f], field_bytes(c, f, (size_t)S.n_sites), hipMemcpyDeviceToHost, c->s_compute));
    if (S.o.site_pick_err && S.d_pick_out) HIPCHK(hipMemcpyAsync(S.o.site_pick_err, S.d_pick_out, (size_t)S.n_sites * sizeof(double), hipMemcpyDeviceToHost, c->s_compute));
    if (S.text) HIPCHK(hipMemcpyAsync(S.h_toff, S.rec.off, sizeof(int64_t) * ((size_t)S.n_sites + 1), hipMemcpyDeviceToHost, c->s_compute));
    if (S.gvcf) VGLCHK(copy_gvcf_small(c, S, S.n_sites, c->s_compute));
    HIPCHK(hipStreamSynchronize(c->s_compute));
    c->deep_runs++;
    return setal_rc(S);
}

extern "C" int vgl_tile_wait(vgl_ctx* c, int32_t ticket) {
    if (!c || ticket < 0 || ticket > 1) return fail(VGL_E_ARG, "bad ticket");
    HostSlot& S = c->slot[ticket];
    if (!S.busy) return fail(VGL_E_ARG, "no tile in flight under this ticket");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(S.ev_copied));
    S.busy = false;
    if (S.pile && S.n_sites == 0) S.pile->text_needed = 0;
    if ((*S.h_flag & VGL_DEVERR_CAPACITY) && S.n_sites > 0) {
        const bool dev_text = S.text || S.gvcf || S.fetch;               // (formatted from the slot's device planes: the rerun fills those)
        const int rc = dev_text ? deep_rerun_text(c, S) : deep_rerun(c, S);
        if (rc != VGL_E_CAPACITY && (rc != VGL_OK || !dev_text)) return rc;      // done (or failed for another reason, reported as such)
        if (rc == VGL_E_CAPACITY) return flags_to_rc(c, *S.h_flag);
    } else {
        VGLCHK(flags_to_rc(c, *S.h_flag));
        if (S.inf) VGLCHK(true_values_rc(*S.h_ibad));
        VGLCHK(setal_rc(S));
        if (S.pile) VGLCHK(finish_pileup(c, S));
    }
    if (S.fetch) VGLCHK(finish_fetchgl(c, S));
    if (S.gvcf) return finish_gvcf(c, S);
    if (!S.text) return VGL_OK;
    return deliver_text(c, {"text", "offsets[n_sites]", "vgl_ctx_text_bound"}, S.text_cap, S.h_text, S.text_dev ? nullptr : S.rec.text.as(), S.h_toff[S.n_sites]);
}

extern "C" int vgl_simulate_tile(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o) {
    if (c) for (int k = 0; k < 2; k++) if (c->slot[k].busy) return fail(VGL_E_ARG, "vgl_simulate_tile with a tile in flight: vgl_tile_wait() it first");
    int32_t t = 0;
    int rc = vgl_simulate_tile_async(c, site0, n_sites, gt, o, &t);
    if (rc) return rc;
    return vgl_tile_wait(c, t);
}
