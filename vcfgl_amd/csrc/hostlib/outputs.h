// hostlib/outputs.h -- what a tile of the host entry points can deliver beside its tag arrays, each with its entry points and the
// enqueue_* that runs it on the slot's device planes: record text / BCF vectors, gVCF blocks, pileup, fetch-GL, set-alleles,
// the discordance tally.  Part of the one translation unit vgl_host.cpp.
#pragma once

// field table of vgl_tile_out in declaration order: element size and per-tile element count
struct FieldDesc { size_t off; size_t esz; int kind; };
enum { K_SITE, K_SITE5, K_SITEA, K_SITE16, K_EVAL, K_PLANEG, K_PLANEA };
enum { N_FIELDS = 18 };
static const FieldDesc FIELDS[N_FIELDS] = {
    {offsetof(vgl_tile_out, site_status), 4, K_SITE}, {offsetof(vgl_tile_out, n_alleles), 4, K_SITE},
    {offsetof(vgl_tile_out, n_alleles_obs), 4, K_SITE}, {offsetof(vgl_tile_out, alleles2acgt), 1, K_SITE5},
    {offsetof(vgl_tile_out, info_dp), 4, K_SITE}, {offsetof(vgl_tile_out, info_ad), 4, K_SITEA},
    {offsetof(vgl_tile_out, info_adf), 4, K_SITEA}, {offsetof(vgl_tile_out, info_adr), 4, K_SITEA},
    {offsetof(vgl_tile_out, qs), 4, K_SITEA}, {offsetof(vgl_tile_out, i16), 4, K_SITE16},
    {offsetof(vgl_tile_out, fmt_dp), 4, K_EVAL}, {offsetof(vgl_tile_out, gl), 4, K_PLANEG},
    {offsetof(vgl_tile_out, pl), 4, K_PLANEG}, {offsetof(vgl_tile_out, gp), 4, K_PLANEG},
    {offsetof(vgl_tile_out, fmt_ad), 4, K_PLANEA}, {offsetof(vgl_tile_out, fmt_adf), 4, K_PLANEA},
    {offsetof(vgl_tile_out, fmt_adr), 4, K_PLANEA}, {offsetof(vgl_tile_out, pl_u8), 1, K_PLANEG},
};
static size_t field_count(const vgl_ctx* c, int kind, size_t n_sites) {
    const size_t N = c->dp.n_samples, A = c->dp.A, G = c->dp.G;
    switch (kind) {
        case K_SITE: return n_sites; case K_SITE5: return n_sites * 5; case K_SITEA: return n_sites * A;
        case K_SITE16: return n_sites * 16; case K_EVAL: return n_sites * N; case K_PLANEG: return n_sites * G * N;
        default: return n_sites * A * N;
    }
}
static size_t field_bytes(const vgl_ctx* c, int f, size_t n_sites) { return field_count(c, FIELDS[f].kind, n_sites) * FIELDS[f].esz; }
static void*& field_ptr(vgl_tile_out* o, int f) { return *(void**)((char*)o + FIELDS[f].off); }
// the slot's device planes of the fields in `mask`, from site k on, as a vgl_tile_out
static vgl_tile_out slot_planes(const vgl_ctx* c, const HostSlot& S, uint32_t mask, size_t k = 0) {
    vgl_tile_out d;
    memset(&d, 0, sizeof d);
    for (int f = 0; f < N_FIELDS; f++) if (mask >> f & 1u) field_ptr(&d, f) = S.d_out[f].as() + field_bytes(c, f, k);
    return d;
}

// One text side output crosses the link (only the bytes produced), in one or two parts; `what` names it in the refusal
struct TextNames { const char* noun; const char* holder; const char* bound; };
static int deliver_text(vgl_ctx* c, const TextNames& what, int64_t cap, uint8_t* dst, const uint8_t* src, int64_t n,
                        const uint8_t* src2 = nullptr, int64_t n2 = 0) {
    if (n < 0 || n2 < 0 || n + n2 > cap)
        return fail(VGL_E_CAPACITY, "the tile's %s needs %lld bytes, text_cap is %lld (%s holds the size; %s bounds it)", what.noun, (long long)(n + n2), (long long)cap,
                    what.holder, what.bound);
    const bool first = n > 0 && src, second = n2 > 0;                  // (src null: a device destination, written in place)
    if (first) HIPCHK(hipMemcpyAsync(dst, src, (size_t)n, hipMemcpyDeviceToHost, c->s_text));
    if (second) HIPCHK(hipMemcpyAsync(dst + n, src2, (size_t)n2, hipMemcpyDeviceToHost, c->s_text));
    if (first || second) HIPCHK(hipStreamSynchronize(c->s_text));
    return VGL_OK;
}

// ---- record text / BCF typed vectors (vgl_text.hip, vgl_bcf.hip) --------------------------------------------------------------------
// The FORMAT tags vgl_simulate_tile_text_async formats, in add_tags()'s order (bcf_utils.cpp:426-507): DP, GL, PL, GP, AD, ADF, ADR.
// vgl_ctx_true_values: GL, GP, PL, the order simulate_record_true_values adds them in (vcfgl.cpp:1243-1259).
// Returns their count; fid[k] = index into FIELDS.
static int text_fields(const vgl_ctx* c, vgl_text_field* tf, int* fid) {
    struct T { int on; const char* key; int is_float; int count; int f; };
    const T all[] = {{c->p.add_fmt_dp, "DP", 0, VGL_TEXT_ONE, 10}, {c->p.add_gl, "GL", 1, VGL_TEXT_PER_G, 11}, {c->p.add_pl, "PL", 0, VGL_TEXT_PER_G, 12},
                     {c->p.add_gp, "GP", 1, VGL_TEXT_PER_G, 13}, {c->p.add_fmt_ad, "AD", 0, VGL_TEXT_PER_A, 14},
                     {c->p.add_fmt_adf, "ADF", 0, VGL_TEXT_PER_A, 15}, {c->p.add_fmt_adr, "ADR", 0, VGL_TEXT_PER_A, 16}};
    static const int ORDER[2][7] = {{0, 1, 2, 3, 4, 5, 6}, {0, 1, 3, 2, 4, 5, 6}};
    int n = 0;
    for (const int k : ORDER[c->true_values ? 1 : 0]) {
        const T& t = all[k];
        if (!t.on) continue;
        tf[n].key = t.key; tf[n].is_float = t.is_float; tf[n].count = t.count; tf[n].base = nullptr;
        tf[n].site_stride = (int64_t)field_count(c, FIELDS[t.f].kind, 1);
        fid[n++] = t.f;
    }
    return n;
}

// the same fields as BCF descriptors (vgl_ctx_bcf_keys: FIELDS[10 .. 16] = DP, GL, PL, GP, AD, ADF, ADR)
static void bcf_fields(const vgl_ctx* c, const vgl_text_field* tf, const int* fid, int nf, vgl_bcf_field* bf) {
    for (int k = 0; k < nf; k++) {
        bf[k].key_id = c->bcf_keys[fid[k] - 10]; bf[k].is_float = tf[k].is_float; bf[k].count = tf[k].count; bf[k].base = tf[k].base;
        bf[k].site_stride = tf[k].site_stride;
    }
}

extern "C" int vgl_ctx_bcf_keys(vgl_ctx* c, const int32_t* key_ids, int32_t n) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_bcf_keys: null context");
    if (!key_ids) { c->bcf = false; return VGL_OK; }
    if (n != 7) return fail(VGL_E_ARG, "vgl_ctx_bcf_keys: 7 dictionary ids are expected (DP, GL, PL, GP, AD, ADF, ADR), %d given", (int)n);
    vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
    const int nf = text_fields(c, tf, fid);
    for (int k = 0; k < nf; k++)
        if (key_ids[fid[k] - 10] < 0) return fail(VGL_E_ARG, "vgl_ctx_bcf_keys: negative dictionary id of FORMAT/%s", tf[k].key);
    memcpy(c->bcf_keys, key_ids, sizeof c->bcf_keys);
    c->bcf = true;
    return VGL_OK;
}

extern "C" int vgl_ctx_text_device(vgl_ctx* c, int32_t on) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_text_device: null context");
    for (int k = 0; k < 2; k++) if (c->slot[k].busy) return fail(VGL_E_ARG, "vgl_ctx_text_device: a tile is in flight (vgl_tile_wait it first)");
    c->text_dev = on != 0;
    return VGL_OK;
}

extern "C" int64_t vgl_ctx_text_bound(const vgl_ctx* c, int32_t n_sites) {
    if (!c || n_sites < 0) return -1;
    vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
    const int nf = text_fields(c, tf, fid);
    if (c->bcf) {
        vgl_bcf_field bf[VGL_TEXT_MAX_FIELDS];
        bcf_fields(c, tf, fid, nf, bf);
        return vgl_bcf_bound(c->dp.n_samples, n_sites, bf, nf, (int32_t)c->dp.A);
    }
    return vgl_text_bound(c->dp.n_samples, n_sites, tf, nf, (int32_t)c->dp.A);
}

// one formatter pass over `n_sites` sites of the slot's planes (compute stream): text or BCF vectors of the fields tf[0 .. nf) into
// `out` (or `dst`, a destination of the caller's), with the record formatter's workspace
static int format_fields(vgl_ctx* c, HostSlot& S, int32_t n_sites, const vgl_text_field* tf, const int* fid, int nf, const int32_t* status,
                         const int32_t* n_alleles, TextOut& out, uint8_t* dst = nullptr) {
    if (!dst) dst = out.text;
    if (c->bcf) {
        vgl_bcf_field bf[VGL_TEXT_MAX_FIELDS];
        bcf_fields(c, tf, fid, nf, bf);
        return vgl_bcf_encode_device(c->device, bf, nf, c->dp.n_samples, n_sites, status, n_alleles, dst, S.text_cap, out.off, S.rec.ws, S.rec.ws_bytes, c->s_compute);
    }
    return vgl_text_format_device(c->device, tf, nf, c->dp.n_samples, n_sites, status, n_alleles, dst, S.text_cap, out.off, S.rec.ws, S.rec.ws_bytes, c->s_compute);
}

// the formatter on the slot's device planes (compute stream): text into rec.text, site offsets into rec.off
static int enqueue_text(vgl_ctx* c, HostSlot& S, int32_t n_sites) {
    vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
    const int nf = text_fields(c, tf, fid);
    for (int k = 0; k < nf; k++) tf[k].base = S.d_out[fid[k]];
    // (a device destination is written in place: no copy in vgl_tile_wait)
    return format_fields(c, S, n_sites, tf, fid, nf, S.d_out[0].as<const int32_t>(), S.d_out[1].as<const int32_t>(), S.rec, S.text_dev ? S.h_text : nullptr);
}

// ---- gVCF blocks (vgl_gvcf.hip) ------------------------------------------------------------------------------------------------------
extern "C" int vgl_gvcf_edges_device(int32_t n_samples, int32_t n_sites, const vgl_gvcf_in* in, const vgl_gvcf_out* out, void* workspace,
                                     int32_t* edge, void* hip_stream);            // vgl_gvcf.hip (not exported)

// the block columns: PL (the founder's nG values per sample) and DP of each block's aggregates
static const int GVCF_BLOCK_FID[2] = {12, 10};                          // PL, DP
static int gvcf_block_fields(const vgl_ctx* c, const HostSlot* S, vgl_text_field* bf) {
    bf[0].key = "PL"; bf[0].is_float = 0; bf[0].count = VGL_TEXT_PER_G; bf[0].base = S ? S->d_bpl.as() : nullptr; bf[0].site_stride = (int64_t)field_count(c, K_PLANEG, 1);
    bf[1].key = "DP"; bf[1].is_float = 0; bf[1].count = VGL_TEXT_ONE; bf[1].base = S ? S->d_bdp.as() : nullptr; bf[1].site_stride = c->dp.n_samples;
    return 2;
}

extern "C" int64_t vgl_ctx_gvcf_text_bound(const vgl_ctx* c, int32_t n_sites) {
    if (!c || n_sites < 0) return -1;
    vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
    const int nf = text_fields(c, tf, fid);
    vgl_text_field bf[2];
    gvcf_block_fields(c, nullptr, bf);
    // a site is a record or a member of at most one block: the larger of the two texts per site
    int64_t rec, blk;
    if (c->bcf) {
        vgl_bcf_field rb[VGL_TEXT_MAX_FIELDS], bb[2];
        bcf_fields(c, tf, fid, nf, rb);
        bcf_fields(c, bf, GVCF_BLOCK_FID, 2, bb);
        rec = vgl_bcf_bound(c->dp.n_samples, 1, rb, nf, (int32_t)c->dp.A); blk = vgl_bcf_bound(c->dp.n_samples, 1, bb, 2, (int32_t)c->dp.A);
    } else {
        rec = vgl_text_bound(c->dp.n_samples, 1, tf, nf, (int32_t)c->dp.A); blk = vgl_text_bound(c->dp.n_samples, 1, bf, 2, (int32_t)c->dp.A);
    }
    if (rec < 0 || blk < 0) return -1;
    return (int64_t)n_sites * (rec > blk ? rec : blk);
}

// the blocker, the edges and both formatters on the slot's device planes (compute stream)
static int enqueue_gvcf(vgl_ctx* c, HostSlot& S, int32_t n_sites) {
    const int32_t N = c->dp.n_samples;
    vgl_gvcf_in in; memset(&in, 0, sizeof in);
    in.site_status = S.d_out[0].as<const int32_t>(); in.n_alleles = S.d_out[1].as<const int32_t>(); in.n_alleles_obs = S.d_out[2].as<const int32_t>();
    in.contig = S.d_contig; in.pos0 = S.d_pos0;
    in.dp = S.d_out[10].as<const int32_t>(); in.dp_site_stride = N; in.pl = S.d_out[12].as<const int32_t>(); in.pl_site_stride = (int64_t)field_count(c, K_PLANEG, 1);
    in.dps = S.d_dps; in.n_dps = (int32_t)S.dps.size();
    vgl_gvcf_out out; memset(&out, 0, sizeof out);
    out.items = S.d_items; out.counts = S.d_counts; out.block_dp = S.d_bdp; out.block_pl = S.d_bpl; out.block_n_alleles = S.d_bna;
    out.block_status = S.d_bst; out.record_status = S.d_rst;
    int rc = vgl_gvcf_blocks_device(c->device, N, n_sites, &in, &out, S.d_gws, S.gws_bytes, c->s_compute);
    if (rc == VGL_OK) rc = vgl_gvcf_edges_device(N, n_sites, &in, &out, S.d_gws, S.d_edge, c->s_compute);
    if (rc != VGL_OK) return rc;
    vgl_text_field tf[VGL_TEXT_MAX_FIELDS]; int fid[VGL_TEXT_MAX_FIELDS];
    const int nf = text_fields(c, tf, fid);
    for (int k = 0; k < nf; k++) tf[k].base = S.d_out[fid[k]];
    vgl_text_field bf[2];
    gvcf_block_fields(c, &S, bf);
    rc = format_fields(c, S, n_sites, tf, fid, nf, S.d_rst, in.n_alleles, S.rec);
    if (rc != VGL_OK) return rc;
    return format_fields(c, S, n_sites, bf, GVCF_BLOCK_FID, 2, S.d_bst, S.d_bna, S.blk);
}

// the bounded gVCF outputs of a tile: items, counts, offsets, the first / last block's aggregates
static int copy_gvcf_small(vgl_ctx* c, HostSlot& S, int32_t n_sites, hipStream_t st) {
    vgl_gvcf_tile* g = S.h_gv;
    const size_t N = c->dp.n_samples, GN = field_count(c, K_PLANEG, 1);
    HIPCHK(hipMemcpyAsync(g->items, S.d_items, sizeof(vgl_gvcf_item) * (size_t)n_sites, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(S.h_counts, S.d_counts, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(g->record_offsets, S.rec.off, sizeof(int64_t) * ((size_t)n_sites + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(g->block_offsets, S.blk.off, sizeof(int64_t) * ((size_t)n_sites + 1), hipMemcpyDeviceToHost, st));
    if (g->first_dp) HIPCHK(hipMemcpyAsync(g->first_dp, S.d_edge, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    if (g->last_dp) HIPCHK(hipMemcpyAsync(g->last_dp, S.d_edge + N, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    if (g->first_pl) HIPCHK(hipMemcpyAsync(g->first_pl, S.d_edge + 2 * N, sizeof(int32_t) * GN, hipMemcpyDeviceToHost, st));
    if (g->last_pl) HIPCHK(hipMemcpyAsync(g->last_pl, S.d_edge + 2 * N + GN, sizeof(int32_t) * GN, hipMemcpyDeviceToHost, st));
    return VGL_OK;
}

// device buffers of a gVCF tile (sized for max_sites) and its contig / pos0 / thresholds (compute stream)
static int stage_gvcf(vgl_ctx* c, HostSlot& S, int32_t n_sites, const int32_t* contig, const int64_t* pos0) {
    const size_t M = (size_t)c->max_sites, N = c->dp.n_samples, GN = field_count(c, K_PLANEG, 1);
    VGLCHK(S.d_contig.reserve(M)); VGLCHK(S.d_pos0.reserve(M));
    VGLCHK(S.h_contig.reserve(M)); VGLCHK(S.h_pos0.reserve(M));
    VGLCHK(S.h_counts.reserve(4)); VGLCHK(S.d_counts.reserve(4));
    VGLCHK(S.d_bdp.reserve(M * N)); VGLCHK(S.d_bpl.reserve(M * GN));
    VGLCHK(S.d_bna.reserve(M)); VGLCHK(S.d_bst.reserve(M));
    VGLCHK(S.d_rst.reserve(M)); VGLCHK(S.d_edge.reserve(2 * (N + GN)));
    S.gws_bytes = vgl_gvcf_workspace_bytes((int32_t)N, (int32_t)M);
    VGLCHK(S.d_gws.reserve((size_t)S.gws_bytes));
    VGLCHK(S.d_items.reserve(M));
    VGLCHK(S.blk.reserve(S.text_cap, M, -1));                          // (the block formatter runs in the record formatter's workspace)
    if (!S.dps.empty()) VGLCHK(S.d_dps.reserve(S.dps.size()));
    memcpy(S.h_contig, contig, sizeof(int32_t) * (size_t)n_sites);
    memcpy(S.h_pos0, pos0, sizeof(int64_t) * (size_t)n_sites);
    HIPCHK(hipMemcpyAsync(S.d_contig, S.h_contig, sizeof(int32_t) * (size_t)n_sites, hipMemcpyHostToDevice, c->s_compute));
    HIPCHK(hipMemcpyAsync(S.d_pos0, S.h_pos0, sizeof(int64_t) * (size_t)n_sites, hipMemcpyHostToDevice, c->s_compute));
    // (S.dps lives in the slot until its next tile, which waits for this one)
    if (!S.dps.empty()) HIPCHK(hipMemcpyAsync(S.d_dps, S.dps.data(), sizeof(int32_t) * S.dps.size(), hipMemcpyHostToDevice, c->s_compute));
    return VGL_OK;
}

// gVCF tile: counts into the caller's struct; the record text, then the block text behind it, cross the link
static int finish_gvcf(vgl_ctx* c, HostSlot& S) {
    vgl_gvcf_tile* g = S.h_gv;
    const int32_t n = S.n_sites;
    if (n == 0) { g->n_items = 0; g->n_blocks = 0; g->error_site = -1; g->text_needed = 0; return VGL_OK; }
    g->n_items = S.h_counts[0]; g->n_blocks = S.h_counts[1]; g->error_site = S.h_counts[2];
    const int64_t rt = g->record_offsets[n], bt = g->block_offsets[n];
    g->text_needed = rt + bt;
    VGLCHK(deliver_text(c, {"gVCF text", "text_needed", "vgl_ctx_gvcf_text_bound"}, g->text_cap, g->text, S.rec.text, rt, S.blk.text, bt));
    for (int32_t i = 0; i <= n; i++) g->block_offsets[i] += rt;
    return VGL_OK;
}

// ---- pileup (vgl_pileup.hip) ---------------------------------------------------------------------------------------------------------
extern "C" int vgl_pileup_format_impl(int32_t device, int32_t n_samples, int32_t n_sites, const int32_t* site_status, const int32_t* fmt_dp,
                                      const uint8_t* reads, int32_t read_capacity, int32_t qual_char, const double* errp, const VglDevParams* P,
                                      uint32_t* errflag, uint8_t* dst, int64_t dst_cap, int64_t* offsets, void* workspace, int64_t workspace_bytes,
                                      void* hip_stream);          // vgl_pileup.hip (not exported)

extern "C" int64_t vgl_ctx_pileup_bound(const vgl_ctx* c, int32_t n_sites) {
    if (!c || n_sites < 0) return -1;
    return vgl_pileup_bound(c->dp.n_samples, n_sites, c->dp.read_cap);
}

extern "C" int vgl_ctx_pileup_next(vgl_ctx* c, vgl_pileup_tile* p) {
    if (!c) return fail(VGL_E_ARG, "null ctx");
    if (p && (!p->offsets || p->text_cap < 0 || (p->text_cap > 0 && !p->text))) return fail(VGL_E_ARG, "vgl_ctx_pileup_next: null text or offsets");
    c->pile_next = p;
    return VGL_OK;
}

// the score byte of every read of a pileup: -1 = each read's own (or, --adjust-qs 4 with --error-qs 2, from its error probability);
// --adjust-qs 4 with --error-qs 0 / 1: the adjusted score of error_rate (PROGRAM_WILL_ADJUST_QS_FOR_PILEUP, vcfgl.cpp:1664-1693)
static int pileup_qual_char(const vgl_ctx* c, int32_t* qc) {
    *qc = -1;
    if (!(c->p.adjust_qs & 4) || c->p.error_qs == 2) return VGL_OK;
    vgl_params p = c->p;
    if (!c->bins_copy.empty()) p.qs_bins = c->bins_copy.data();
    int q = -1, aq = -1;
    char msg[VGL_PLAN_ERR];
    const int rc = errprob_to_qs_fixed(&p, p.error_rate, &q, &aq, msg);
    if (rc != VGL_OK) return fail(rc, "%s", msg);
    if (aq + 33 < 0 || aq + 33 > 255) return fail(VGL_E_ADJQ, "--adjust-qs 4: the adjusted score %d of the error rate is not a pileup byte", aq);
    *qc = aq + 33;
    return VGL_OK;
}

// the pileup formatter on the slot's device read dump and DP plane (compute stream): text into pil.text, site offsets into pil.off;
// a --qs-bins miss of a score lands in the tile's device flags (this runs before they are copied)
static int enqueue_pileup(vgl_ctx* c, HostSlot& S, int32_t n_sites, const vgl_tile_out& d) {
    const int32_t cap = d.read_capacity < c->dp.read_cap ? d.read_capacity : c->dp.read_cap;
    const bool from_errp = (c->p.adjust_qs & 4) && c->p.error_qs == 2;
    return vgl_pileup_format_impl(c->device, c->dp.n_samples, n_sites, S.d_out[0].as<const int32_t>(), S.d_out[10].as<const int32_t>(), d.reads, cap, S.pile_qc,
                                  from_errp ? d.read_errp : nullptr, from_errp ? &c->dp : nullptr, from_errp ? c->d_errflag.as() : nullptr,
                                  S.pil.text, S.pile->text_cap, S.pil.off, S.pil.ws, S.pil.ws_bytes, c->s_compute);
}

// pileup: offsets[n_sites] = -1: a dp beyond the dump's capacity
static int finish_pileup(vgl_ctx* c, HostSlot& S) {
    vgl_pileup_tile* p = S.pile;
    const int64_t total = p->offsets[S.n_sites];
    p->text_needed = total;
    if (total < 0)
        return fail(VGL_E_CAPACITY, "a simulated read depth exceeded the capacity of the tile's read dump (%d reads per sample): no pileup", c->dp.read_cap);
    return deliver_text(c, {"pileup", "text_needed", "vgl_ctx_pileup_bound"}, p->text_cap, p->text, S.pil.text, total);
}

// ---- one genotype's GL of a context's tiles as CSV text (vgl_fetchgl.hip) ----------------------------------------------------------
extern "C" int vgl_ctx_fetchgl(vgl_ctx* c, int32_t a, int32_t b, int32_t value_mode) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_fetchgl: null context");
    for (const auto& S : c->slot) if (S.busy) return fail(VGL_E_ARG, "vgl_ctx_fetchgl: a tile of the context is in flight");
    if (a < 0) { c->fetch_a = c->fetch_b = -1; c->fetch_next = nullptr; return VGL_OK; }
    if (a > 4 || b < 0 || b > 4) return fail(VGL_E_ARG, "vgl_ctx_fetchgl: alleles are 0 .. 4 (A, C, G, T, unobserved)");
    if (value_mode != VGL_FETCHGL_FLOAT && value_mode != VGL_FETCHGL_TEXT) return fail(VGL_E_ARG, "vgl_ctx_fetchgl: value_mode must be VGL_FETCHGL_FLOAT or VGL_FETCHGL_TEXT");
    if (!c->p.add_gl) return fail(VGL_E_ARG, "vgl_ctx_fetchgl: the context computes no GL (add_gl = 0)");
    c->fetch_a = a; c->fetch_b = b; c->fetch_mode = value_mode;
    return VGL_OK;
}

extern "C" int64_t vgl_ctx_fetchgl_bound(const vgl_ctx* c, int32_t n_sites) {
    if (!c || n_sites < 0) return -1;
    return vgl_fetchgl_bound(c->dp.n_samples, n_sites);
}

extern "C" int vgl_ctx_fetchgl_next(vgl_ctx* c, vgl_fetchgl_tile* p) {
    if (!c) return fail(VGL_E_ARG, "null ctx");
    if (p && c->fetch_a < 0) return fail(VGL_E_ARG, "vgl_ctx_fetchgl_next: no genotype is set (vgl_ctx_fetchgl)");
    if (p && (!p->offsets || p->text_cap < 0 || (p->text_cap > 0 && !p->text))) return fail(VGL_E_ARG, "vgl_ctx_fetchgl_next: null text or offsets");
    c->fetch_next = p;
    return VGL_OK;
}

// the formatter on the slot's device planes (compute stream): text into fet.text, site offsets into fet.off
static int enqueue_fetchgl(vgl_ctx* c, HostSlot& S, int32_t n_sites) {
    return vgl_fetchgl_format_device(c->device, c->dp.n_samples, n_sites, c->dp.G, c->dp.out_layout, S.d_out[0].as<const int32_t>(), S.d_out[1].as<const int32_t>(),
                                     S.d_out[3].as<const int8_t>(), S.d_out[11].as<const float>(), c->fetch_a, c->fetch_b, c->fetch_mode, S.fet.text,
                                     S.fetch->text_cap, S.fet.off, S.fet.ws, S.fet.ws_bytes, c->s_compute);
}

static int finish_fetchgl(vgl_ctx* c, HostSlot& S) {
    vgl_fetchgl_tile* p = S.fetch;
    if (S.n_sites == 0) { p->text_needed = 0; return VGL_OK; }
    p->text_needed = p->offsets[S.n_sites];
    return deliver_text(c, {"fetch-GL text", "text_needed", "vgl_ctx_fetchgl_bound"}, p->text_cap, p->text, S.fet.text, p->text_needed);
}

// ---- discordance tally of a context's tiles (vgl_disc.hip) ------------------------------------------------------------------------
extern "C" int vgl_ctx_discordance(vgl_ctx* c, int32_t on) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_discordance: null context");
    for (const auto& S : c->slot) if (S.busy) return fail(VGL_E_ARG, "vgl_ctx_discordance: a tile of the context is in flight");
    if (on && !c->d_disc_table) {
        HIPCHK(hipSetDevice(c->device));
        const size_t n = (size_t)vgl_disc_table_len(c->dp.n_samples);
        if (c->d_disc_table.reserve(n)) return fail(VGL_E_NOMEM, "out of device memory (discordance table)");
        HIPCHK(hipMemset(c->d_disc_table, 0, n * sizeof(int64_t)));
        HIPCHK(hipDeviceSynchronize());
    }
    c->disc = on != 0;
    return VGL_OK;
}

extern "C" int vgl_ctx_discordance_read(vgl_ctx* c, int64_t* host_table, int32_t reset) {
    if (!c || !host_table) return fail(VGL_E_ARG, "vgl_ctx_discordance_read: null argument");
    if (!c->d_disc_table) return fail(VGL_E_ARG, "vgl_ctx_discordance_read: the context has no table (vgl_ctx_discordance was never switched on)");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t bytes = (size_t)vgl_disc_table_len(c->dp.n_samples) * sizeof(int64_t);
    HIPCHK(hipMemcpy(host_table, c->d_disc_table, bytes, hipMemcpyDeviceToHost));
    if (reset) { HIPCHK(hipMemset(c->d_disc_table, 0, bytes)); HIPCHK(hipDeviceSynchronize()); }
    return VGL_OK;
}

// the sibling context of a deep tile counts into its parent's table and relabels from its parent's target table (vgl_ctx_set_alleles)
static void deep_share(vgl_ctx* c) {
    c->deep->disc = c->disc; c->deep->d_disc_table.borrow(c->d_disc_table);
    c->deep->d_setal.borrow(c->d_setal); c->deep->setal_first = c->setal_first; c->deep->setal_n = c->setal_n;
}

// ---- a prescribed REF/ALT list for the records of a context's tiles (vgl_setal.hip) -------------------------------------------------
extern "C" int vgl_ctx_set_alleles(vgl_ctx* c, const int8_t* table, int64_t first_site, int64_t n_sites) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: null context");
    for (const auto& S : c->slot) if (S.busy) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: a tile of the context is in flight");
    HIPCHK(hipSetDevice(c->device));
    if (!table) {
        c->d_setal.release(); c->setal_first = c->setal_n = 0;
        if (c->deep) { c->deep->d_setal.release(); c->deep->setal_n = 0; }
        return VGL_OK;
    }
    const vgl_params& p = c->p;
    if (p.add_fmt_ad || p.add_info_ad || p.add_fmt_adf || p.add_info_adf || p.add_fmt_adr || p.add_info_adr)
        return fail(VGL_E_ARG, "vgl_ctx_set_alleles: the context writes AD / ADF / ADR tags, which keep the old alleles (misc/setAlleles leaves them stale)");
    if (p.do_gvcf) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: not supported with do_gvcf (block records)");
    if (first_site < 0 || n_sites < 0) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: negative first_site or n_sites");
    for (int64_t i = 0; i < n_sites; i++) {
        const int8_t* e = table + i * 8;
        if (e[0] < 2 || e[0] > 5) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: site %lld has %d alleles (2 .. 5)", (long long)(first_site + i), (int)e[0]);
        for (int j = 0; j < e[0]; j++) {
            if (e[1 + j] < 0 || e[1 + j] > 4) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: site %lld: allele %d is not 0 .. 4", (long long)(first_site + i), (int)e[1 + j]);
            for (int k = 0; k < j; k++) if (e[1 + k] == e[1 + j]) return fail(VGL_E_ARG, "vgl_ctx_set_alleles: site %lld names an allele twice", (long long)(first_site + i));
        }
    }
    c->d_setal.release(); c->setal_n = 0;                               // (a new table is a new buffer: the sibling may still hold the old pointer)
    VGLCHK(c->d_setal.reserve((size_t)(n_sites ? n_sites * 8 : 8)));
    if (n_sites) HIPCHK(hipMemcpy(c->d_setal, table, (size_t)n_sites * 8, hipMemcpyHostToDevice));
    c->setal_first = first_site; c->setal_n = n_sites;
    if (c->deep) deep_share(c);
    return VGL_OK;
}

// the relabelling of a tile's device arrays `d` (compute stream); the first refused site of the tile into S.h_sbad
static int enqueue_setal(vgl_ctx* c, HostSlot& S, int64_t site0, int32_t n_sites, const vgl_tile_out& d, hipStream_t st) {
    const int32_t N = c->dp.n_samples;
    S.sws_bytes = vgl_setal_workspace_bytes(N, c->max_sites, c->dp.G);
    VGLCHK(S.d_sws.reserve((size_t)S.sws_bytes)); VGLCHK(S.d_sbad.reserve(1)); VGLCHK(S.h_sbad.reserve(1));
    HIPCHK(hipMemsetAsync(S.d_sbad, 0x7F, sizeof(int32_t), st));
    const int rc = vgl_setal_apply_device(c->device, N, n_sites, c->dp.G, c->dp.A, c->dp.out_layout, c->d_setal + (site0 - c->setal_first) * 8, d.site_status, d.n_alleles,
                                          d.alleles2acgt, d.qs, d.fmt_dp, d.gl, d.pl, d.gp, d.pl_u8, S.d_sbad, S.d_sws, S.sws_bytes, st);
    if (rc != VGL_OK) return rc;
    HIPCHK(hipMemcpyAsync(S.h_sbad, S.d_sbad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return VGL_OK;
}
// ---- tiles filled from their true genotypes instead of simulated (vgl_inf.hip; the tile itself: true_values_tile, tile_device.h) -----
extern "C" int vgl_ctx_true_values(vgl_ctx* c, int32_t on) {
    if (!c) return fail(VGL_E_ARG, "vgl_ctx_true_values: null context");
    for (const auto& S : c->slot) if (S.busy) return fail(VGL_E_ARG, "vgl_ctx_true_values: a tile of the context is in flight");
    if (!on) { c->true_values = false; return VGL_OK; }
    const vgl_params& p = c->p;
    if (p.add_fmt_dp || p.add_info_dp || p.add_fmt_ad || p.add_info_ad || p.add_fmt_adf || p.add_info_adf || p.add_fmt_adr || p.add_info_adr || p.add_qs || p.add_i16)
        return fail(VGL_E_ARG, "vgl_ctx_true_values: the context writes DP, AD, ADF, ADR, QS or I16 tags, which true values do not define (no read is drawn)");
    VGLCHK(true_values_ctx_ok(c, "vgl_ctx_true_values"));
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_inf_abs) {
        VGLCHK(c->d_inf_ws.reserve((size_t)vgl_inf_workspace_bytes(c->dp.n_samples, c->max_sites)));
        VGLCHK(c->d_inf_bad.reserve(1)); VGLCHK(c->d_inf_abs.reserve(1));
        HIPCHK(hipMemset(c->d_inf_abs, 0xFF, sizeof(unsigned long long)));
        HIPCHK(hipDeviceSynchronize());
    }
    c->true_values = true;
    return VGL_OK;
}
// the tile's smallest bad site into S.h_ibad, and a clean word for the next tile (compute stream)
static int enqueue_true_values_rc(vgl_ctx* c, HostSlot& S) {
    HIPCHK(hipMemcpyAsync(S.h_ibad, c->d_inf_abs, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute));
    HIPCHK(hipMemsetAsync(c->d_inf_abs, 0xFF, sizeof(unsigned long long), c->s_compute));
    return VGL_OK;
}

static int setal_rc(HostSlot& S) {
    if (!S.setal || !S.h_sbad || *S.h_sbad < 0 || *S.h_sbad >= S.n_sites) return VGL_OK;
    return fail(VGL_E_SETAL, "site %lld: the target allele list names an allele the record does not have (misc/setAlleles is undefined there)",
                (long long)(S.site0 + *S.h_sbad));
}
