// hostlib/ctx.h -- the context: what it owns, vgl_ctx_create / _destroy / _info, kernel timing, and the entry points that need no
// context (RNG window arithmetic, the BGZF member walk, pinned host memory).  Part of the one translation unit vgl_host.cpp.
#pragma once

extern "C" int vgl_default_rng_layout(const vgl_params* p, vgl_rng_layout* out) {
    if (!p || !out) return fail(VGL_E_ARG, "null argument");
    *out = plan_default_layout(p);
    return VGL_OK;
}

// Sites [0, max) a VGL_RNG_TILE job of this shape may address: evaluation (site, sample) owns draws [e block, (e + 1) block),
// e = H(site) * n_samples + sample, and H (vgl_site_hash, vgl_device.h) permutes [0, 2^W) with 2^W * n_samples * block <= 2^48.
extern "C" int vgl_rng_tile_max_sites(const vgl_params* p, int64_t* max_sites) {
    if (!p || !max_sites || p->n_samples <= 0) return fail(VGL_E_ARG, "null argument");
    const int W = site_hash_bits(p);
    if (W < 0) return fail(VGL_E_ARG, VGL_MSG_PERIOD);
    *max_sites = (int64_t)1 << W;
    return VGL_OK;
}

extern "C" int vgl_rng_tile_site_hash(const vgl_params* p, int64_t site, int64_t* hashed) {
    if (!p || !hashed || p->n_samples <= 0) return fail(VGL_E_ARG, "null argument");
    const int W = site_hash_bits(p);
    if (W < 0) return fail(VGL_E_ARG, VGL_MSG_PERIOD);
    if (site < 0 || site >= ((int64_t)1 << W)) return fail(VGL_E_ARG, "site %lld outside [0, 2^%d)", (long long)site, W);
    *hashed = (int64_t)vgl_site_hash((uint64_t)site, W);
    return VGL_OK;
}

// ---- the members of a BGZF stream (pure host arithmetic: vgl_inflate_core.h holds the walk) -----------------------------------------
extern "C" int vgl_bgzf_index(const uint8_t* raw, int64_t n, int64_t max_members, int64_t* begin, int32_t* csize, int32_t* isize, int64_t* n_members) {
    if (!raw || n < 0 || max_members < 0 || !n_members || (max_members > 0 && (!begin || !csize || !isize))) return fail(VGL_E_ARG, "vgl_bgzf_index: bad argument");
    *n_members = 0;
    if (vgl_bgzf_index_core(raw, n, max_members, begin, csize, isize, n_members) != 0)
        return fail(VGL_E_UNSUPPORTED, "vgl_bgzf_index: the bytes are not a series of whole BGZF members (gzip members with FLG 4, a 'BC' subfield and ISIZE <= 65536)");
    if (*n_members > max_members) return fail(VGL_E_CAPACITY, "vgl_bgzf_index: %lld members, room for %lld", (long long)*n_members, (long long)max_members);
    return VGL_OK;
}

extern "C" void* vgl_host_alloc(size_t bytes) {
    void* p = nullptr;
    // default flags: page-locked, placed on the host NUMA node nearest to the calling thread's current device (measured: 53 GB/s
    // of DMA into it against 35 GB/s into hipHostMallocPortable memory on the two-socket box); every device of the process can
    // still write it.  VGL_HOST_ALLOC_FLAGS overrides (diagnostic).
    const unsigned flags = hook_env("VGL_HOST_ALLOC_FLAGS") ? (unsigned)strtoul(hook_env("VGL_HOST_ALLOC_FLAGS"), nullptr, 0) : hipHostMallocDefault;
    if (hipHostMalloc(&p, bytes ? bytes : 1, flags) != hipSuccess) { fail(VGL_E_NOMEM, "hipHostMalloc of %zu bytes failed", bytes); return nullptr; }
    return p;
}
extern "C" void* vgl_host_alloc_on(int32_t device, size_t bytes) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || hipSetDevice(device) != hipSuccess) { fail(VGL_E_NODEVICE, "device %d is not available", device); return nullptr; }
    void* p = vgl_host_alloc(bytes);
    (void)hipSetDevice(cur);
    return p;
}
extern "C" void vgl_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- context ---------------------------------------------------------------------------
// One tile in flight through the host entry points (vgl_simulate_tile / _async): two slots of device mirrors, so that the copies of
// one tile's tags back to the host (copy stream) run beside the kernels of the next tile (compute stream) -- SURVEY H8
struct HostSlot {
    Event ev_kernels, ev_copied;
    DevBuf<uint8_t> d_gt; PinBuf<uint8_t> h_gt;                 // h_gt: pinned staging of the packed genotypes
    DevBuf<uint8_t> d_out[18];                                  // the tag planes, FIELDS order (counted in workspace_bytes)
    DevBuf<uint8_t> d_reads_out; DevBuf<double> d_errp_out, d_pick_out;
    PinBuf<uint32_t> h_flag;                                    // pinned: the tile's device error flags
    bool busy = false; int rc = VGL_OK;
    int64_t site0 = 0; int32_t n_sites = 0; vgl_tile_out o{};    // the tile in flight (vgl_tile_wait may run it again through `deep`)
    // vgl_simulate_tile_text_async: the FORMAT tags formatted on the device (vgl_text.hip); the text is copied back by vgl_tile_wait,
    // which knows its size
    bool text = false; uint8_t* h_text = nullptr; int64_t text_cap = 0; int64_t* h_toff = nullptr;
    bool text_dev = false;                                      // vgl_ctx_text_device: h_text is device memory, written in place
    uint32_t dev_fields = 0;                                    // fields of d_out the tile's kernels wrote (bit f: FIELDS[f])
    TextOut rec;
    // vgl_simulate_tile_gvcf_async: the tile blocked on the device (vgl_gvcf.hip), its record and block columns formatted there
    // (record text in rec, block text in blk); vgl_tile_wait copies the text back, which knows its size
    bool gvcf = false; vgl_gvcf_tile* h_gv = nullptr;
    PinBuf<int32_t> h_counts, h_contig; PinBuf<int64_t> h_pos0;
    DevBuf<int32_t> d_contig; DevBuf<int64_t> d_pos0;
    std::vector<int32_t> dps; DevBuf<int32_t> d_dps;
    DevBuf<vgl_gvcf_item> d_items;
    DevBuf<int32_t> d_counts, d_bdp, d_bpl, d_bna, d_bst, d_rst, d_edge;
    DevBuf<uint8_t> d_gws; int64_t gws_bytes = 0;
    TextOut blk;
    // vgl_ctx_pileup_next: the tile's pileup formatted on the device (vgl_pileup.hip) from its read dump and DP plane; vgl_tile_wait
    // copies the text back, which knows its size
    vgl_pileup_tile* pile = nullptr; int32_t pile_qc = -1;
    TextOut pil;
    // vgl_ctx_fetchgl_next: one genotype's GL of the tile as CSV text, formatted on the device (vgl_fetchgl.hip) from its GL planes --
    // kept on the device whether or not the caller asks for them; vgl_tile_wait copies the text back, which knows its size
    vgl_fetchgl_tile* fetch = nullptr;
    TextOut fet;
    // vgl_ctx_set_alleles: the tile's arrays are relabelled on the device (vgl_setal.hip) behind its likelihood kernels; d_sbad / h_sbad
    // (pinned) hold the first refused site of the tile, counted from its first site (>= n_sites: none)
    bool setal = false; DevBuf<int32_t> d_sbad; PinBuf<int32_t> h_sbad; DevBuf<uint8_t> d_sws; int64_t sws_bytes = 0;
    // vgl_ctx_true_values: the tile was filled from its genotypes (vgl_inf.hip); h_ibad (pinned) holds the smallest bad absolute site of
    // the tile (VGL_INF_NO_BAD_SITE: none)
    bool inf = false; PinBuf<unsigned long long> h_ibad;
};
#define VGL_INF_NO_BAD_SITE (~0ULL)

#define VGL_NEV (VGL_N_TIMING_BUCKETS + 1)
struct vgl_ctx {
    vgl_params p{};                                                 // (depths / qs_bins: the copies below)
    std::vector<double> depths_copy; std::vector<int32_t> bins_copy;
    int device = 0;
    int max_sites = 0;
    VglDevParams dp{};
    size_t ws_bytes = 0;            // device memory owned (vgl_ctx_info): the buffers built with W below and the slots' tag planes
    size_t* const W = &ws_bytes;   // (a pointer into this object, as are the accounts of its buffers: a context is never copied or moved)
    Stream s_compute, s_copy;
    Stream s_text;                                                  // text copies of vgl_tile_wait (never behind the next tile's copies)
    // device tables
    DevBuf<VglAffine> d_depth_tab{W}, d_samp_tab{W}, d_qs_read_tab{W}, d_step_tab{W};
    DevBuf<int32_t> d_dp_pre{W}; DevBuf<uint64_t> d_site_base{W}, d_site_hash{W}; DevBuf<VglPois> d_pois{W};
    DevBuf<float> d_gl2_run{W}, d_pois_zt{W}; DevBuf<unsigned long long> d_fslot{W};
    DevBuf<double> d_q2gl{W}, d_gamma_ln{W}, d_gl1_beta{W}, d_gl1_bsum{W}, d_gl1_lhet{W};
    // workspace
    DevBuf<uint8_t> d_reads{W}; DevBuf<double> d_errp{W}; DevBuf<uint64_t> d_ad4{W}, d_adf4{W};
    DevBuf<uint32_t> d_qsum{W}, d_qsumsq{W}; DevBuf<int32_t> d_acc{W}; DevBuf<VglSiteInfo> d_sinfo{W}; DevBuf<uint64_t> d_rowmap{W}, d_rowmap8{W};
    DevBuf<uint32_t> d_gl2_redo{W}, d_gl2_list{W}, d_gl2_count{W}; size_t gl2_redo_words = 0;
    DevBuf<uint32_t> d_errflag{W};
    DevBuf<unsigned long long> d_redo_list{W}; DevBuf<uint32_t> d_redo_count{W}; uint32_t redo_cap = 0; DevBuf<uint32_t> d_redo_bits{W};   // k_sample<2, deferred> -> k_redo
    DevBuf<uint32_t> d_seg_list{W};                                      // k_sample_seg<., 1> -> k_sample_seg<., 2>
    // beta chain of VGL_RNG_SERIAL with --error-qs 2 and the std beta sampler (vgl_betachain.hip); grow-only buffers
    DevBuf<long long> d_roff{W}, d_rtotal{W}; DevBuf<double> d_errp_lin{W};
    DevBuf<uint32_t> d_cw{W}; DevBuf<uint8_t> d_ccons{W}, d_cexit{W}, d_centry{W}; DevBuf<int32_t> d_ccnt{W};
    DevBuf<long long> d_cbase{W}, d_csnapw{W}; DevBuf<uint32_t> d_cpos{W}, d_csnap{W}; DevBuf<VglChainCtl> d_cctl{W};
    long long chain_words_cap = 0;
    DevBuf<unsigned long long> d_dbg{W};
    // VGL_RNG_SERIAL
    DevBuf<long long> d_hts_off{W}; DevBuf<uint64_t> d_hts_base{W};
    DevBuf<VglSerialState> d_serial{W}; DevBuf<uint64_t> d_sst{W}, d_site_thresh{W}; DevBuf<int32_t> d_scout_dp{W}, d_sdp{W}; DevBuf<VglSiteTail> d_site_tail{W};
    DevBuf<uint64_t> d_tail_base{W};   // VGL_RNG_TILE with -addI16 (k_tail)
    int64_t serial_next_site = 0;   // VGL_DEBUG_STAMPS=1 diagnostic counters
    HostSlot slot[2];
    vgl_pileup_tile* pile_next = nullptr;                           // vgl_ctx_pileup_next: taken by the next tile call
    // vgl_ctx_fetchgl: the requested alleles (0 .. 4; fetch_a < 0: off) and value mode; vgl_ctx_fetchgl_next: taken by the next tile call
    int32_t fetch_a = -1, fetch_b = -1, fetch_mode = 0;
    vgl_fetchgl_tile* fetch_next = nullptr;
    // vgl_ctx_set_alleles: the target entries (8 bytes each) of the absolute sites setal_first .. setal_first + setal_n - 1 on the device;
    // the sibling context `deep` borrows its parent's
    DevBuf<int8_t> d_setal; int64_t setal_first = 0, setal_n = 0;
    // vgl_ctx_true_values: tiles are filled from their genotypes (vgl_inf.hip) instead of simulated.  d_inf_ws: the kernels' workspace;
    // d_inf_bad: the stateless call's tile-relative word; d_inf_abs: the smallest bad absolute site since it was last read
    // (VGL_INF_NO_BAD_SITE: none); d_inf_nobs: n_alleles_obs of a device tile whose caller does not ask for it
    bool true_values = false;
    DevBuf<uint8_t> d_inf_ws{W}; DevBuf<int32_t> d_inf_bad{W}, d_inf_nobs{W}; DevBuf<unsigned long long> d_inf_abs{W};
    // vgl_ctx_bcf_keys: the text / gVCF tile calls deliver BCF typed vectors (vgl_bcf.hip) instead of text; dictionary ids of
    // DP, GL, PL, GP, AD, ADF, ADR
    bool bcf = false; int32_t bcf_keys[7] = {0, 0, 0, 0, 0, 0, 0};
    bool text_dev = false;                                          // vgl_ctx_text_device: the text tile call's `text` is device memory
    // a draw deeper than the staging capacity (vcfgl grows its read buffers, bcf_utils.cpp:618-648): the host entry points run such a tile again on
    // this sibling context, created on first need with the staging layout's largest capacity (VGL_READ_CAP_MAX reads) and tiles of at most
    // VGL_DEEP_TILE_SITES sites.  VGL_RNG_TILE only (a value depends on (seed, site, sample) alone, so the second run is the same tile)
    vgl_ctx* deep = nullptr;
    int32_t deep_runs = 0;
    // vgl_ctx_discordance: every tile is tallied behind its likelihood kernel (vgl_disc.hip).  The sibling context `deep` borrows its
    // parent's table; d_disc_dp / d_disc_pl hold FORMAT/DP and the one-byte PL of a tile whose caller asks for neither (one set: the
    // tally runs on the tile's own stream, ahead of the next tile's kernels)
    bool disc = false;
    DevBuf<int64_t> d_disc_table{W}; DevBuf<int32_t> d_disc_dp{W}; DevBuf<uint8_t> d_disc_pl{W};
    int next_slot = 0;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;     // groups of VGL_N_TIMING_BUCKETS + 1
    double ms[VGL_N_TIMING_BUCKETS] = {0}; int64_t launches[VGL_N_TIMING_BUCKETS] = {0};    // VGL_T_*

    vgl_ctx() { for (HostSlot& S : slot) for (auto& b : S.d_out) b.account = W; }
    vgl_ctx(const vgl_ctx&) = delete;
    vgl_ctx& operator=(const vgl_ctx&) = delete;
    ~vgl_ctx() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

extern "C" int vgl_ctx_destroy(vgl_ctx* c) {
    if (!c) return VGL_OK;
    if (c->deep) { (void)vgl_ctx_destroy(c->deep); c->deep = nullptr; }
    (void)hipSetDevice(c->device);
    for (HostSlot& S : c->slot) if (S.busy && S.ev_copied) (void)hipEventSynchronize(S.ev_copied);
    delete c;                                                       // (every buffer, stream and event is a member that frees itself)
    return VGL_OK;
}
struct CtxDeleter { void operator()(vgl_ctx* c) const { (void)vgl_ctx_destroy(c); } };

#define VGL_DEEP_TILE_SITES 2048       // tiles of the sibling context that takes over a tile with a deeper draw

// a table: room for it on the device and its upload
template <typename T> static int upload(DevBuf<T>& d, const std::vector<T>& h) {
    const int rc = d.reserve(h.size());
    if (rc != VGL_OK) return rc;
    HIPCHK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return VGL_OK;
}
// words that start as zero
template <typename T> static int zeroed(DevBuf<T>& d, size_t n) {
    const int rc = d.reserve(n);
    if (rc != VGL_OK) return rc;
    HIPCHK(hipMemset(d, 0, sizeof(T) * n));
    return VGL_OK;
}

// the constant tables of tables.h on the device, and their pointers in the kernels' parameters
static int ctx_upload_tables(vgl_ctx* c, const VglPlanExtra& X) {
    const vgl_params* p = &c->p;
    VglDevParams& D = c->dp;
    const int N = D.n_samples;
    const std::vector<VglAffine> samp = aff_table(aff_pow(X.lay.block), (size_t)N);       // J^(block * s): one evaluation block per sample
    if (!D.serial) {                                               // k_depth: J^(off0 + block*s)
        std::vector<VglAffine> dt(N);
        for (int s = 0; s < N; s++) dt[s] = aff_compose(D.off[0], samp[s]);
        VGLCHK(upload(c->d_depth_tab, dt));
        D.depth_tab = c->d_depth_tab;
    }
    VGLCHK(upload(c->d_samp_tab, samp));
    D.samp_tab = c->d_samp_tab;
    if (p->error_qs == 2) { VGLCHK(upload(c->d_qs_read_tab, qs_read_table(X.lay.qs_read_stride, D.read_cap))); D.qs_read_tab = c->d_qs_read_tab; }
    if (!c->depths_copy.empty()) {
        std::vector<VglPois> pv(N);
        for (int s = 0; s < N; s++) pois_init(&pv[s], c->depths_copy[s]);
        VGLCHK(upload(c->d_pois, pv));
        D.pois = c->d_pois;
    }
    const int n = 2048;
    const std::vector<double> gl = gamma_ln_table(n);
    VGLCHK(upload(c->d_gamma_ln, gl));
    D.gamma_ln_tab = c->d_gamma_ln; D.gamma_ln_n = n;
    if (X.pois_zt) {
        std::vector<float> zt(n);
        vgl_pois_zt_host(&D.pois0, gl.data(), n, zt.data());
        VGLCHK(upload(c->d_pois_zt, zt));
        D.pois_zt = c->d_pois_zt;
    }
    VGLCHK(upload(c->d_q2gl, X.q2gl));
    D.q2gl = c->d_q2gl;
    if (X.gl2_run) { VGLCHK(upload(c->d_gl2_run, build_gl2_run(D.read_cap, D.pre_homT, D.pre_het, D.pre_homF))); D.gl2_run = c->d_gl2_run; }
    if (p->gl_model == 1) {
        std::vector<double> bsum, lhet, fkv, betav;
        if (p->error_qs == 2) {                                    // gl_methods.cpp:233-302: per-read qScores
            build_gl1_tables(1.0 - p->gl1_theta, -1, bsum, lhet, &fkv, &betav);
            VGLCHK(upload(c->d_gl1_beta, build_gl1_fkbeta(fkv, betav, D.gl1_nc)));
            D.gl1_fkbeta = c->d_gl1_beta;
        } else
            build_gl1_tables(1.0 - p->gl1_theta, (p->adjust_qs & 1) ? D.pre_adjq : D.pre_q, bsum, lhet);   // io.cpp:1276, gl_methods.cpp:318
        VGLCHK(upload(c->d_gl1_bsum, bsum)); VGLCHK(upload(c->d_gl1_lhet, lhet));
        D.gl1_bsum = c->d_gl1_bsum; D.gl1_lhet = c->d_gl1_lhet;
    }
    if (D.serial) {
        VGLCHK(upload(c->d_step_tab, aff_table(aff_pow(1), 192)));
        D.step_tab = c->d_step_tab;
        VGLCHK(upload(c->d_serial, std::vector<VglSerialState>(1, serial_start_state(p->seed, D.x0))));
    }
    return VGL_OK;
}

// the workspace of a tile of max_sites sites
static int ctx_alloc_workspace(vgl_ctx* c) {
    const vgl_params* p = &c->p;
    const VglDevParams& D = c->dp;
    const size_t M = (size_t)c->max_sites, E = M * D.n_samples;
    if (!D.serial) {                                               // k_sitebase's outputs
        VGLCHK(c->d_site_base.reserve(M)); VGLCHK(c->d_site_hash.reserve(M));
        if (p->add_i16) { VGLCHK(c->d_tail_base.reserve(M)); VGLCHK(c->d_site_tail.reserve(M)); }     // INFO/I16 fields 13-16 (k_tail, vgl_gl.hip)
        VGLCHK(c->d_dp_pre.reserve(E));
    }
    VGLCHK(c->d_reads.reserve(E * D.read_cap));
    if ((p->precise_gl || (D.serial && !D.beta_chain)) && p->error_qs == 2) VGLCHK(c->d_errp.reserve(E * D.read_cap));
    if (D.beta_chain) { VGLCHK(c->d_roff.reserve(E)); VGLCHK(c->d_rtotal.reserve(1)); VGLCHK(c->d_cctl.reserve(1)); }
    if (D.serial) {
        VGLCHK(c->d_sst.reserve(E * 2)); VGLCHK(c->d_site_thresh.reserve(M)); VGLCHK(c->d_scout_dp.reserve((size_t)D.n_samples)); VGLCHK(c->d_sdp.reserve(E));
        if (p->add_i16) VGLCHK(c->d_site_tail.reserve(M));
        if (D.gl1_deep) { VGLCHK(c->d_hts_off.reserve(E)); VGLCHK(c->d_hts_base.reserve(1)); }
    }
    VGLCHK(c->d_ad4.reserve(E));
    if (D.need_adf) VGLCHK(c->d_adf4.reserve(E));
    if (D.need_qsum) VGLCHK(c->d_qsum.reserve(E * 4));
    if (D.need_qsumsq) VGLCHK(c->d_qsumsq.reserve(E * 4));
    VGLCHK(c->d_acc.reserve(M * VGL_ACC_STRIDE));
    VGLCHK(c->d_sinfo.reserve(M));
    if (p->gl_model == 2) VGLCHK(c->d_rowmap.reserve(M * 16));
    if (D.gl2x) {
        VGLCHK(c->d_rowmap8.reserve(M * 32));
        VGLCHK(zeroed(c->d_gl2_redo, c->gl2_redo_words));
        VGLCHK(c->d_gl2_list.reserve(c->gl2_redo_words * 32));
        VGLCHK(c->d_gl2_count.reserve(1));
    }
    if (D.fused && D.fused_split > 1) VGLCHK(c->d_fslot.reserve(M * D.fused_split * 2));
    if (D.defer_ok) {                                              // k_redo's list, and the bitmap over the staged reads for what does not fit
        VGLCHK(zeroed(c->d_redo_bits, (E * (size_t)D.read_cap + 31) / 32));
        VGLCHK(c->d_redo_list.reserve(std::max<size_t>(1, (size_t)c->redo_cap * VGL_REDO_PARTS)));
        VGLCHK(zeroed(c->d_redo_count, (size_t)VGL_REDO_PARTS * VGL_REDO_STRIDE));
        if (D.seg_split) VGLCHK(c->d_seg_list.reserve(M * D.chunks));
    }
    VGLCHK(zeroed(c->d_errflag, 1));
    return VGL_OK;
}

static int ctx_create_cap(const vgl_params* p, int32_t device, int32_t max_sites, vgl_ctx** out, const int cap_override) {
    if (!p || !out) return fail(VGL_E_ARG, "null argument");
    *out = nullptr;
    char msg[VGL_PLAN_ERR];
    int rc = vgl_plan_validate(p, max_sites, msg);
    if (rc != VGL_OK) return fail(rc, "%s", msg);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VGL_E_NODEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VGL_E_NODEVICE, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));

    std::unique_ptr<vgl_ctx, CtxDeleter> c(new vgl_ctx());
    c->p = *p; c->p.depths = nullptr; c->p.qs_bins = nullptr;
    if (p->depths) c->depths_copy.assign(p->depths, p->depths + p->n_samples);
    if (p->n_qs_bins > 0 && p->qs_bins) c->bins_copy.assign(p->qs_bins, p->qs_bins + 3 * (size_t)p->n_qs_bins);
    c->device = device; c->max_sites = max_sites;
    VglPlanExtra X;
    if ((rc = vgl_plan_derive(p, max_sites, cap_override, hook_env, &c->dp, &X, msg)) != VGL_OK) return fail(rc, "%s", msg);
    c->p.layout = X.lay;
    c->redo_cap = X.redo_cap; c->gl2_redo_words = X.gl2_redo_words;
    VGLCHK(ctx_upload_tables(c.get(), X));
    VGLCHK(ctx_alloc_workspace(c.get()));
    if (X.dbg_words) VGLCHK(zeroed(c->d_dbg, 16));
    HIPCHK(hipDeviceSynchronize());          // tables and cleared words are in place before any (non-blocking) stream uses them
    *out = c.release();
    return VGL_OK;
}
extern "C" int vgl_ctx_create(const vgl_params* p, int32_t device, int32_t max_sites, vgl_ctx** out) { return ctx_create_cap(p, device, max_sites, out, 0); }

static int resolve_timing(vgl_ctx* c) {
    for (size_t i = 0; i + VGL_NEV - 1 < c->ev.size(); i += VGL_NEV) {
        HIPCHK(hipEventSynchronize(c->ev[i + VGL_NEV - 1]));
        for (int k = 0; k < VGL_N_TIMING_BUCKETS; k++) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->ev[i + k], c->ev[i + k + 1]));
            c->ms[k] += ms; c->launches[k] += 1;
        }
    }
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    c->ev.clear();
    return VGL_OK;
}

extern "C" int vgl_ctx_timing(vgl_ctx* c, int32_t enable) {
    if (!c) return fail(VGL_E_ARG, "null ctx");
    c->timing = enable != 0;
    return VGL_OK;
}

extern "C" int vgl_ctx_kernel_ms(vgl_ctx* c, double* ms, int64_t* launches, int32_t n_buckets, int32_t reset) {
    if (!c || !ms || !launches || n_buckets < 0) return fail(VGL_E_ARG, "null ctx / arrays");
    HIPCHK(hipSetDevice(c->device));
    int rc = resolve_timing(c);
    if (rc) return rc;
    for (int k = 0; k < n_buckets; k++) { ms[k] = k < VGL_N_TIMING_BUCKETS ? c->ms[k] : 0.0; launches[k] = k < VGL_N_TIMING_BUCKETS ? c->launches[k] : 0; }
    if (reset) for (int k = 0; k < VGL_N_TIMING_BUCKETS; k++) { c->ms[k] = 0; c->launches[k] = 0; }
    return VGL_OK;
}

// what this context launches (include/vcfgl_hip.h: vgl_ctx_info_t)
extern "C" int vgl_ctx_info(const vgl_ctx* c, vgl_ctx_info_t* out) {
    if (!c || !out) return fail(VGL_E_ARG, "null argument");
    if (out->size < (int32_t)sizeof(int32_t) * 2) return fail(VGL_E_ARG, "vgl_ctx_info_t.size must be set by the caller");
    vgl_ctx_info_t r;
    memset(&r, 0, sizeof r);
    r.size = out->size < (int32_t)sizeof r ? out->size : (int32_t)sizeof r;
    vgl_plan_info(c->dp, c->p.rng_mode, c->max_sites, &r);
    r.device = c->device;
#ifdef VGL_TEST_HOOKS
    r.test_hooks = 1;
#endif
    r.workspace_bytes = (int64_t)c->ws_bytes;
    memcpy(out, &r, (size_t)r.size);
    return VGL_OK;
}
