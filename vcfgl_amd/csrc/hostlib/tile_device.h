// hostlib/tile_device.h -- vgl_simulate_tile_device: one tile's kernels on the caller's stream and device arrays; the beta chain of
// the serial mode; the vgl_dbg_* diagnostics of the hooks build.  Part of the one translation unit vgl_host.cpp.
#pragma once

extern "C" int vgl_disc_tally_impl(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout, const int32_t* site_status,
                                   const int32_t* n_alleles, const int8_t* alleles2acgt, const int32_t* fmt_dp, const uint8_t* pl_u8, const int32_t* pl,
                                   const uint8_t* gt, int64_t* table, const uint32_t* errflag, void* hip_stream);      // vgl_disc.hip (not exported)

// VGL_RNG_SERIAL, --error-qs 2, std beta sampler: the beta deviates of the tile's reads in draw order
// (vgl_betachain.hip).  Synchronises the stream: the number of reads and each chunk's progress come back to the host.
static int run_beta_chain(vgl_ctx* c, const VglDevParams& D, int n_sites, hipStream_t st) {
    const long long E = (long long)n_sites * D.n_samples;
    if (vgl_chain_read_offsets(c->d_sdp, E, c->d_roff, c->d_rtotal, st)) return fail(VGL_E_NODEVICE, "k_read_offsets launch failed");
    long long R = 0;
    HIPCHK(hipMemcpyAsync(&R, c->d_rtotal, sizeof R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (R == 0) return VGL_OK;
    if ((size_t)R > c->d_errp_lin.cap && c->d_errp_lin.reserve((size_t)R + (size_t)R / 8 + 1024)) return VGL_E_NOMEM;
    const long long margin = vgl_chain_margin_words(), seg = vgl_chain_seg();
    long long done = 0;
    while (done < R) {
        const long long remaining = R - done;
        // a deviate takes ~15-19 words on average; the chunk is sized for the rest of the tile, at most 2^28 words
        long long n_words = remaining * 24 + 4096 + margin;
        long long cap_words = 1LL << 28;
        if (hook_env("VGL_CHAIN_MAX_WORDS")) cap_words = atoll(hook_env("VGL_CHAIN_MAX_WORDS"));      // test hook: many small chunks
        if (n_words > cap_words) n_words = cap_words;
        n_words &= ~1LL;
        if (n_words > c->chain_words_cap) {
            release_all(c->d_cw, c->d_ccons, c->d_cexit, c->d_ccnt, c->d_centry, c->d_cbase, c->d_cpos, c->d_csnap, c->d_csnapw);
            c->chain_words_cap = 0;
            const size_t npos = (size_t)n_words / 2, nseg = npos / (size_t)seg + 2, nsnap = (size_t)vgl_chain_snapshots_needed(n_words);
            if (c->d_cw.reserve((size_t)n_words) || c->d_ccons.reserve(npos) || c->d_cexit.reserve(nseg * 64) || c->d_ccnt.reserve(nseg * 64) ||
                c->d_centry.reserve(nseg) || c->d_cbase.reserve(nseg) || c->d_cpos.reserve(npos / 4 + 1024) ||
                c->d_csnap.reserve(nsnap * 624) || c->d_csnapw.reserve(nsnap + 1)) return VGL_E_NOMEM;
            c->chain_words_cap = n_words;
        }
        VglChainCtl h; memset(&h, 0, sizeof h);
        h.remaining = remaining; h.n_pos = (n_words - margin) / 2; h.n_seg = (int)((h.n_pos + seg - 1) / seg);
        HIPCHK(hipMemcpyAsync(c->d_cctl, &h, sizeof h, hipMemcpyHostToDevice, st));
        if (vgl_chain_chunk(&D, c->d_serial, c->d_cctl, c->d_cw, n_words, c->d_ccons, c->d_cexit, c->d_ccnt, c->d_centry, c->d_cbase, c->d_cpos,
                            c->d_csnap, c->d_csnapw, st)) return fail(VGL_E_NODEVICE, "beta chain launch failed: %s", hipGetErrorString(hipGetLastError()));
        HIPCHK(hipMemcpyAsync(&h, c->d_cctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h.err) return fail(VGL_E_UNSUPPORTED, "a beta deviate consumed more generator words than the chain scheme allows");
        if (h.n_chunk <= 0 || h.endw <= 0) return fail(VGL_E_NODEVICE, "beta chain made no progress");
        if (vgl_chain_emit(&D, c->d_serial, c->d_cctl, c->d_cw, c->d_cpos, h.n_chunk, c->d_errp_lin + done, c->d_csnap, c->d_csnapw,
                           vgl_chain_snapshots_needed(n_words), st)) return fail(VGL_E_NODEVICE, "beta chain launch failed");
        done += h.n_chunk;
    }
    return VGL_OK;
}

// the context's scratch and the caller's output arrays as the kernels take them
static void fill_tile_ptrs(const vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, const vgl_tile_out* o, VglTilePtrs& T) {
    const VglDevParams& D = c->dp;
    memset(&T, 0, sizeof T);
    T.site0 = site0; T.n_sites = n_sites; T.gt = gt;
    T.reads = c->d_reads; T.errp = c->d_errp; T.ad4 = c->d_ad4; T.adf4 = c->d_adf4; T.qsum = c->d_qsum; T.qsumsq = c->d_qsumsq;
    T.acc = c->d_acc; T.sinfo = c->d_sinfo; T.rowmap = c->d_rowmap; T.rowmap8 = c->d_rowmap8; T.gl2_redo = c->d_gl2_redo; T.gl2_redo_list = c->d_gl2_list; T.gl2_redo_count = c->d_gl2_count; T.errflag = c->d_errflag; T.dbg = c->d_dbg; T.dp_pre = c->d_dp_pre;
    T.site_base = c->d_site_base; T.site_hash = c->d_site_hash; T.fslot = c->d_fslot;
    T.redo_list = c->d_redo_list; T.redo_count = c->d_redo_count; T.redo_cap = c->redo_cap; T.redo_bits = c->d_redo_bits;
    T.seg_list = c->d_seg_list;
    if (!D.serial && o->i16 && c->d_tail_base) { T.tail_base = c->d_tail_base; T.site_tail = c->d_site_tail; }   // (k_sitebase, k_tail; a tile without an I16 output skips both)
    if (D.serial) {
        const size_t E = (size_t)c->max_sites * D.n_samples;
        T.sst_hap = c->d_sst; T.sst_base = c->d_sst + E; T.sdp = c->d_sdp;
        T.site_thresh = c->d_site_thresh; T.scout_off = c->d_scout_dp; T.site_tail = c->d_site_tail;
    }
    T.site_status = o->site_status; T.n_alleles = o->n_alleles; T.n_alleles_obs = o->n_alleles_obs; T.alleles2acgt = o->alleles2acgt;
    T.info_dp = o->info_dp; T.info_ad = o->info_ad; T.info_adf = o->info_adf; T.info_adr = o->info_adr;
    T.qs = o->qs; T.i16 = o->i16; T.fmt_dp = o->fmt_dp; T.gl = o->gl; T.pl = o->pl; T.gp = o->gp;
    T.fmt_ad = o->fmt_ad; T.fmt_adf = o->fmt_adf; T.fmt_adr = o->fmt_adr; T.pl_u8 = o->pl_u8;
    T.reads_out = o->read_capacity > 0 ? o->reads : nullptr;
    T.reads_out_cap = o->read_capacity > 0 ? (o->read_capacity < D.read_cap ? o->read_capacity : D.read_cap) : 0;
}

// ---- vgl_ctx_true_values: a tile filled from its genotypes (vgl_inf.hip) instead of simulated ----------------------------------------
extern "C" int vgl_inf_fill_impl(int32_t device, int32_t n_samples, int32_t n_sites, int32_t do_unobserved, int32_t max_genotypes, int32_t max_alleles,
                                 int32_t layout, const uint8_t* gt, int32_t* site_status, int32_t* n_alleles, int32_t* n_alleles_obs, int8_t* alleles2acgt,
                                 float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site, void* workspace, int64_t workspace_bytes,
                                 int64_t site0, unsigned long long* bad_abs, void* hip_stream);       // vgl_inf.hip (not exported)

// the outputs a true-value tile does not define
static int true_values_outputs_ok(const vgl_tile_out* o) {
    if (o->info_dp || o->info_ad || o->info_adf || o->info_adr || o->qs || o->i16 || o->fmt_dp || o->fmt_ad || o->fmt_adf || o->fmt_adr || o->reads ||
        o->read_errp || o->site_pick_err)
        return fail(VGL_E_ARG, "vgl_ctx_true_values is on: no read is drawn, so DP, AD, ADF, ADR, QS, I16, the read dumps and site_pick_err are not defined (their vgl_tile_out pointers must be NULL)");
    return VGL_OK;
}
// what else a context in that mode does not compose with (`who`: the entry point that reports it)
static int true_values_ctx_ok(const vgl_ctx* c, const char* who) {
    if (c->disc) return fail(VGL_E_ARG, "%s: not supported together with vgl_ctx_discordance (every call would be the truth)", who);
    if (c->fetch_a >= 0) return fail(VGL_E_ARG, "%s: not supported together with vgl_ctx_fetchgl", who);
    if (c->d_setal) return fail(VGL_E_ARG, "%s: not supported together with vgl_ctx_set_alleles", who);
    return VGL_OK;
}

static int true_values_tile(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* o, hipStream_t st) {
    VGLCHK(true_values_outputs_ok(o));
    VGLCHK(true_values_ctx_ok(c, "vgl_ctx_true_values is on"));
    HIPCHK(hipSetDevice(c->device));
    int32_t* nobs = o->n_alleles_obs;
    if (!nobs) { VGLCHK(c->d_inf_nobs.reserve((size_t)c->max_sites)); nobs = c->d_inf_nobs; }
    HIPCHK(hipMemsetAsync(c->d_inf_bad, 0x7F, sizeof(int32_t), st));
    return vgl_inf_fill_impl(c->device, c->dp.n_samples, n_sites, c->p.do_unobserved, c->dp.G, c->dp.A, c->dp.out_layout, gt, o->site_status, o->n_alleles, nobs,
                             o->alleles2acgt, o->gl, o->pl, o->gp, o->pl_u8, c->d_inf_bad, c->d_inf_ws, (int64_t)c->d_inf_ws.bytes(), site0, c->d_inf_abs, st);
}
static int true_values_rc(unsigned long long bad) {
    if (bad == VGL_INF_NO_BAD_SITE) return VGL_OK;
    return fail(VGL_E_ARG, "site %llu: a true genotype is not a pair of A, C, G, T (true values need complete genotypes)", bad);
}

extern "C" int vgl_simulate_tile_device(vgl_ctx* c, int64_t site0, int32_t n_sites, const uint8_t* gt,
                                        vgl_tile_out* o, void* stream) {
    if (!c || !o) return fail(VGL_E_ARG, "null argument");
    if (n_sites < 0 || n_sites > c->max_sites) return fail(VGL_E_ARG, "n_sites %d exceeds max_sites_per_tile %d", n_sites, c->max_sites);
    if (n_sites == 0) return VGL_OK;
    if (!gt || !o->site_status || !o->n_alleles || !o->alleles2acgt) return fail(VGL_E_ARG, "gt, site_status, n_alleles and alleles2acgt are required");
    if (site0 < 0) return fail(VGL_E_ARG, "site0 must be >= 0");
    if (c->true_values) return true_values_tile(c, site0, n_sites, gt, o, (hipStream_t)stream);
    if (!c->dp.serial) {
        // VGL_RNG_TILE windows are slices of ONE rand48 sequence of period 2^48: evaluation (site, sample) owns draws
        // [e block, (e + 1) block), e = H(site) n_samples + sample, H a permutation of [0, 2^W).  Past 2^W sites the windows would
        // silently repeat earlier ones.
        if ((uint64_t)site0 + (uint64_t)n_sites > (1ULL << c->dp.site_hash_bits))
            return fail(VGL_E_ARG, "VGL_RNG_TILE: sites [%lld, %lld) x %d samples x %llu draws per evaluation run past the 2^48 period of rand48 "
                        "(at most %llu sites with this layout); split the job over seeds or use a smaller layout.block",
                        (long long)site0, (long long)site0 + n_sites, c->dp.n_samples, (unsigned long long)c->p.layout.block,
                        (unsigned long long)(1ULL << c->dp.site_hash_bits));
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const VglDevParams& D = c->dp;
    VglTilePtrs T;
    fill_tile_ptrs(c, site0, n_sites, gt, o, T);
    if (D.serial && site0 != c->serial_next_site)
        return fail(VGL_E_ARG, "VGL_RNG_SERIAL consumes the streams in call order: expected site0 %lld, got %lld", (long long)c->serial_next_site, (long long)site0);
    if (o->read_capacity > D.read_cap && o->reads)
        HIPCHK(hipMemsetAsync(o->reads + (size_t)D.read_cap * n_sites * D.n_samples, 0xFF,
                              (size_t)(o->read_capacity - D.read_cap) * n_sites * D.n_samples, st));
    if ((o->qs && !D.need_qsum) || (o->i16 && !D.need_qsumsq))
        return fail(VGL_E_ARG, "qs / i16 outputs need -addQS / -addI16 in the context parameters");
    // dumps of the deviates (ABI 2): the per-read error probabilities go through the --precise-gl staging planes
    const bool dump_errp = o->read_errp && o->read_capacity > 0 && D.error_qs == 2;
    if (dump_errp && c->d_errp.reserve((size_t)c->max_sites * D.n_samples * D.read_cap))
        return fail(VGL_E_NOMEM, "out of device memory (read_errp staging)");
    const bool errp_always = (c->p.precise_gl || (D.serial && !D.beta_chain)) && D.error_qs == 2;    // as sized by vgl_ctx_create
    T.errp = (errp_always || dump_errp) ? c->d_errp.as() : nullptr;
    T.site_pick_err = (D.error_qs == 1) ? o->site_pick_err : nullptr;
    if (c->disc) {                                                // the tally reads FORMAT/DP and PL: kept on the device when the caller asks for neither
        if (!T.fmt_dp) {
            if (c->d_disc_dp.reserve((size_t)c->max_sites * D.n_samples)) return fail(VGL_E_NOMEM, "out of device memory (discordance: FORMAT/DP)");
            T.fmt_dp = c->d_disc_dp;
        }
        if (!T.pl && !T.pl_u8) {
            if (c->d_disc_pl.reserve((size_t)c->max_sites * D.G * D.n_samples)) return fail(VGL_E_NOMEM, "out of device memory (discordance: PL)");
            T.pl_u8 = c->d_disc_pl;
        }
    }

    // the timing events belong to this call until the last one is recorded: any early return below destroys them (a failed call
    // leaks nothing), the successful end hands them to the context
    struct EvGuard { hipEvent_t e[VGL_NEV]; bool armed = true;
                     EvGuard() { for (int k = 0; k < VGL_NEV; k++) e[k] = nullptr; }
                     ~EvGuard() { if (armed) for (int k = 0; k < VGL_NEV; k++) if (e[k]) (void)hipEventDestroy(e[k]); } } evg;
    hipEvent_t* const e = evg.e;
    if (c->timing) for (int k = 0; k < VGL_NEV; k++) HIPCHK(hipEventCreate(&e[k]));
    HIPCHK(hipMemsetAsync(c->d_acc, 0, sizeof(int32_t) * VGL_ACC_STRIDE * (size_t)n_sites, st));
    if (c->d_redo_count) HIPCHK(hipMemsetAsync(c->d_redo_count, 0, sizeof(uint32_t) * VGL_REDO_PARTS * VGL_REDO_STRIDE, st));
    if (c->d_fslot) HIPCHK(hipMemsetAsync(c->d_fslot, 0, sizeof(unsigned long long) * 2 * (size_t)D.fused_split * (size_t)n_sites, st));
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_DEPTH], st));        // depth draws ahead of k_sample (k_sitebase + k_depth; the scouts in serial mode)
    if (D.serial) {
        if (vgl_launch_scout(&D, &T, c->d_serial, st)) return fail(VGL_E_NODEVICE, "k_scout launch failed");
        c->serial_next_site = site0 + n_sites;
        if (D.beta_chain) {
            const int rc = run_beta_chain(c, D, n_sites, st);
            if (rc != VGL_OK) return rc;
            T.roff = c->d_roff; T.errp_lin = c->d_errp_lin;
        }
    } else {
        if (vgl_launch_sitebase(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_sitebase launch failed");
        if (D.depth_pre == 1 && vgl_launch_depth(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_depth launch failed");
    }
    const bool fused = D.fused && !T.reads_out && !o->qs && !o->i16 && !dump_errp;
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_SAMPLE], st));
    if (!fused && vgl_launch_sample(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_sample launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_REDO], st));
    if (!fused && vgl_launch_redo(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_redo launch failed");
    // INFO/I16 tail distances in tile mode (k_tail wants the LAST read's base): with the other site aggregates, behind k_gl -- unless k_gl's GL model 1
    // path may shuffle a deep evaluation's staged reads in place (gl1_deep), then ahead of it
    if (T.tail_base && D.gl1_deep && vgl_launch_tail(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_tail launch failed");
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_SITE], st));
    if (!fused && vgl_launch_site(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_site launch failed");
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_GL], st));
    if (D.serial && D.gl1_deep) {                            // where each deep evaluation's shuffle starts in htslib's stream
        if (vgl_launch_hts_offsets(&D, &T, c->d_serial, c->d_hts_off, c->d_hts_base, st)) return fail(VGL_E_NODEVICE, "k_hts_offsets launch failed");
        T.hts_off = c->d_hts_off; T.hts_base = c->d_hts_base;
    }
    if (fused) { if (vgl_launch_fused(&D, &T, st)) return fail(VGL_E_NODEVICE, "fused k_gl launch failed"); }
    else if (vgl_launch_gl(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_gl launch failed");
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_T_SITEAGG], st));
    if (T.tail_base && !D.gl1_deep && vgl_launch_tail(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_tail launch failed");
    if (o->qs || o->i16) if (vgl_launch_siteagg(&D, &T, st)) return fail(VGL_E_NODEVICE, "k_siteagg launch failed");
    if (dump_errp) {
        const size_t row = (size_t)n_sites * D.n_samples;
        const size_t rows = (size_t)(o->read_capacity < D.read_cap ? o->read_capacity : D.read_cap);
        if (vgl_launch_errp_dump(&D, c->d_errp, o->read_errp, row, (int)rows, st)) return fail(VGL_E_NODEVICE, "k_errp_dump launch failed");
        if ((size_t)o->read_capacity > rows)
            HIPCHK(hipMemsetAsync(o->read_errp + rows * row, 0xFF, ((size_t)o->read_capacity - rows) * row * sizeof(double), st));
    }
    if (c->disc && vgl_disc_tally_impl(c->device, D.n_samples, n_sites, D.G, D.out_layout, T.site_status, T.n_alleles, T.alleles2acgt, T.fmt_dp,
                                       T.pl_u8, T.pl_u8 ? nullptr : T.pl, gt, c->d_disc_table, c->d_errflag, st)) return VGL_E_NODEVICE;
    if (c->timing) HIPCHK(hipEventRecord(e[VGL_NEV - 1], st));
    if (c->timing) for (int k = 0; k < VGL_NEV; k++) c->ev.push_back(e[k]);
    evg.armed = false;
    return VGL_OK;
}

// the device error flags of a tile as a return code and text (vgl_ctx_check, vgl_tile_wait)
static int flags_to_rc(const vgl_ctx* c, uint32_t flag) {
    if (flag & VGL_DEVERR_CAPACITY) return fail(VGL_E_CAPACITY, "a simulated read depth exceeded the staging capacity of %d reads per sample", c->dp.read_cap);
    if (flag & VGL_DEVERR_QSBIN) return fail(VGL_E_QSBIN, "Could not find a range for a simulated qs value in --qs-bins");
    if (flag & VGL_DEVERR_ADJQ) return fail(VGL_E_ADJQ, "--adjust-qs %d: a read has no valid adjusted quality score (error probability exactly 0 or 1, or a negative adjusted score)", c->dp.adjust_qs);
    if (flag & VGL_DEVERR_INTERNAL) return fail(VGL_E_NODEVICE, "internal: a kernel's LDS layout assumption does not hold on this build (k_sample<2>)");
    return VGL_OK;
}

extern "C" int vgl_ctx_check(vgl_ctx* c, void* stream) {
    if (!c) return fail(VGL_E_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    uint32_t flag = 0;
    unsigned long long bad = VGL_INF_NO_BAD_SITE;                   // vgl_ctx_true_values: the smallest bad site of the tiles since the last check
    HIPCHK(hipMemcpyAsync(&flag, c->d_errflag, sizeof flag, hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (c->d_inf_abs) HIPCHK(hipMemcpyAsync(&bad, c->d_inf_abs, sizeof bad, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (flag) HIPCHK(hipMemsetAsync(c->d_errflag, 0, sizeof flag, (hipStream_t)stream));
    if (bad != VGL_INF_NO_BAD_SITE) HIPCHK(hipMemsetAsync(c->d_inf_abs, 0xFF, sizeof bad, (hipStream_t)stream));
    VGLCHK(flags_to_rc(c, flag));
    return true_values_rc(bad);
}

#ifdef VGL_TEST_HOOKS
// diagnostic (not in the public header): the beta deviates of the last serial tile in draw order
extern "C" __attribute__((visibility("default"))) long long vgl_dbg_chain(vgl_ctx* c, double* out, long long n) {
    if (!c || !c->d_errp_lin) return -1;
    long long R = 0;
    if (hipMemcpy(&R, c->d_rtotal, sizeof R, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n > R) n = R;
    if (hipMemcpy(out, c->d_errp_lin, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return R;
}

// diagnostic (not in the public header): the generator states in front of the windows of the last tile's sites (k_sitebase)
extern "C" __attribute__((visibility("default"))) int vgl_dbg_site_base(vgl_ctx* c, uint64_t* out, int n) {
    if (!c || !c->d_site_base || n > c->max_sites) return VGL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->d_site_base, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
    return VGL_OK;
}

// diagnostic (not in the public header): read and clear the VGL_DEBUG_STAMPS counters
extern "C" __attribute__((visibility("default"))) int vgl_dbg_stamps(vgl_ctx* c, unsigned long long out[16]) {
    if (!c || !c->d_dbg) return fail(VGL_E_ARG, "context was not created with VGL_DEBUG_STAMPS=1");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->d_dbg, 128, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(c->d_dbg, 0, 128));
    return VGL_OK;
}

// diagnostic (not part of the C ABI): entries of the last tile's redo list (k_sample<2, deferred> -> k_redo)
extern "C" __attribute__((visibility("default"))) int vgl_dbg_redo_count(vgl_ctx* c, unsigned* n) {
    if (!c || !n) return VGL_E_ARG;
    *n = 0;
    if (!c->d_redo_count) return VGL_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[VGL_REDO_PARTS * VGL_REDO_STRIDE];                         // one counter per partition of the list
    HIPCHK(hipMemcpy(h, c->d_redo_count, sizeof h, hipMemcpyDeviceToHost));
    for (int p = 0; p < VGL_REDO_PARTS; ++p) *n += h[p * VGL_REDO_STRIDE];
    return VGL_OK;
}
#endif
