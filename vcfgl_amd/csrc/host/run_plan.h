// run_plan.h -- what a device run does, decided once from the arguments (RunPlan), and the buffers of one tile in flight (TileBufs):
// allocation, the device workers and the writer all read the same plan
#pragma once

#include "sites.h"

// the three tile calls of the library: vgl_simulate_tile_async (the FORMAT arrays come back), ..._text_async (the sample columns as VCF
// text or, with bcf, as BCF typed vectors) and ..._gvcf_async (the gVCF items with their sample columns)
enum TilePath { ARRAYS, TEXT, GVCF };

struct RunPlan {
    int N = 0, A = 0, G = 0;                  // samples; the most alleles / genotypes a site can have
    int TS = 0, D = 0, R = 0, pile_cap = 0;   // sites per tile, devices, ring entries, rows of the per-read dumps
    char mode = 'b'; std::string ext; const char* nonref = nullptr; int enc_threads = 1;
    std::vector<int> devices; int bgzf_dev = -1;          // --device-bgzf 1: the run's first device compresses every BGZF stream
    TilePath path = ARRAYS;
    bool bcf = false;                         // --device-bcf 1: the FORMAT part of BCF records comes from the device
    bool stream = false;                      // --device-stream 1: records assembled and compressed where the tile was simulated
    bool device_pileup = false;               // --device-pileup 1: the pileup's sample columns come from the device
    bool rec0 = false;                        // --records 0: no record file, no FORMAT array back; the tiles are simulated and tallied
    bool fetch = false;                       // --fetch-gl XY: one genotype's GL of every tile comes back as CSV text
    bool setal = false;                       // --set-alleles FILE: every context relabels its tiles from the file's table
    bool inf = false;                         // --device-inf 1: the contexts fill their tiles from the true genotypes (--depth inf), nothing is simulated
    bool want_dp = false, want_errp = false, dump_reads = false, dump_pick = false;
    bool host_pileup = false;                 // -printPileup 1 without it: the lines are formatted on the host from the read dump
};

static vgl_params make_params(const Args& a, int N) {
    vgl_params p; memset(&p, 0, sizeof p);
    p.abi_version = VGL_ABI_VERSION; p.out_layout = VGL_LAYOUT_SAMPLE_MAJOR; p.seed = a.seed; p.n_samples = N; p.rng_mode = a.rng_mode; p.beta_sampler = a.beta_sampler;
    p.depth = a.depth; p.depths = a.depths.empty() ? nullptr : a.depths.data();
    p.error_rate = a.error_rate; p.error_qs = a.error_qs; p.beta_variance = a.beta_variance; p.gl_model = a.gl_model;
    p.gl1_theta = a.gl1_theta; p.precise_gl = a.precise_gl; p.adjust_qs = a.adjust_qs; p.adjust_by = a.adjust_by;
    p.n_qs_bins = (int)a.qs_bins.size() / 3; p.qs_bins = a.qs_bins.empty() ? nullptr : a.qs_bins.data(); p.i16_mapq = a.i16_mapq;
    p.do_unobserved = a.do_unobserved; p.rm_invar_sites = a.rm_invar; p.rm_empty_sites = a.rm_empty; p.do_gvcf = a.do_gvcf;
    p.add_gl = a.add_gl; p.add_gp = a.add_gp; p.add_pl = a.add_pl; p.add_i16 = a.add_i16; p.add_qs = a.add_qs;
    p.add_fmt_dp = a.add_fmt_dp; p.add_info_dp = a.add_info_dp; p.add_fmt_ad = a.add_fmt_ad; p.add_info_ad = a.add_info_ad;
    p.add_fmt_adf = a.add_fmt_adf; p.add_info_adf = a.add_info_adf; p.add_fmt_adr = a.add_fmt_adr; p.add_info_adr = a.add_info_adr;
    return p;
}

// --device-inf 1: the arguments of the device run.  What run_depth_inf ignores -- the depth, the error and likelihood models, the
// quality-score adjustments, the DP / AD tags, the per-read listings, the RNG mode, the device's own site filters -- is neutral here,
// so that the contexts are created without any of it and the plan asks no tile for it.  (The site stream keeps the run's own
// arguments: --rm-invar-sites 1|2|3 and -explode act there, as on the host path.)
static Args true_values_args(const Args& a) {
    Args r = a;
    r.depth = 1.0; r.depths.clear(); r.depths_fn.clear();
    r.error_rate = 0.01; r.error_qs = 0; r.beta_variance = -1.0; r.qs_bins.clear(); r.qs_bins_fn.clear();
    r.gl_model = 2; r.precise_gl = 0; r.adjust_qs = 0; r.i16_mapq = 20;
    r.rm_invar = 0; r.rm_empty = 0;
    r.add_fmt_dp = r.add_info_dp = r.add_fmt_ad = r.add_info_ad = r.add_fmt_adf = r.add_info_adf = r.add_fmt_adr = r.add_info_adr = r.add_qs = r.add_i16 = 0;
    r.print_bpe = r.print_qs_err = r.print_gl_err = r.print_qscores = 0;
    r.rng_mode = VGL_RNG_TILE; r.beta_sampler = VGL_BETA_RAND48;
    return r;
}

static RunPlan make_plan(const Args& a, const vgl_params& p, int N, int enc_threads) {
    RunPlan P;
    P.N = N; P.mode = a.output_mode[0]; P.ext = output_ext(a);
    P.nonref = nonref_name(a); P.enc_threads = enc_threads; P.bgzf_dev = bgzf_device(a);
    P.TS = a.tile_sites > 0 ? a.tile_sites : 4096;
    P.device_pileup = a.device_pileup != 0; P.bcf = a.device_bcf != 0; P.host_pileup = a.print_pileup && !P.device_pileup;
    // per-read dump rows: the library's own staging capacity (vgl_host.cpp: depth + 8 sqrt(depth) + 16)
    double dmax = a.depth; for (double d : a.depths) dmax = std::max(dmax, d); if (!(dmax >= 0)) dmax = 0;
    P.pile_cap = (((int)ceil(dmax + 8.0 * sqrt(dmax) + 16.0)) + 3) & ~3;
    if (P.host_pileup || a.print_qs_err || a.print_gl_err || a.print_qscores)      // per-read dumps: bounded host / device staging
        P.TS = std::max(1, std::min(P.TS, (int)((64u << 20) / ((size_t)1024 * (size_t)std::max(N, 1)) + 1)));
    else if (P.device_pileup) {                                  // the pileup text of a tile: at most 256 MiB per ring entry (two per device)
        const int64_t per_site = vgl_pileup_bound(N, 1, P.pile_cap);
        P.TS = std::max(1, (int)std::min<int64_t>(P.TS, (int64_t)(256u << 20) / std::max<int64_t>(per_site, 1)));
    }
    P.fetch = a.fetch; P.setal = !a.set_alleles_fn.empty(); P.inf = a.device_inf != 0;
    if (P.fetch) {                                               // the fetched text of a tile: at most 256 MiB per ring entry, as the pileup's
        const int64_t per_site = vgl_fetchgl_bound(N, 1);
        P.TS = std::max(1, (int)std::min<int64_t>(P.TS, (int64_t)(256u << 20) / std::max<int64_t>(per_site, 1)));
    }
    // ---- devices: one context and one host thread per GPU; tiles are dealt to them round robin and come back to the writer
    //      (the main thread) in site order.  Every value depends only on the absolute site index (VGL_RNG_TILE), so the file does
    //      not depend on the number of devices.  VGL_RNG_SERIAL consumes its streams in call order: one device.
    P.devices = a.devices.empty() ? std::vector<int>{a.device} : a.devices;
    if (P.devices.size() > 1 && a.rng_mode == VGL_RNG_SERIAL) die("--devices: --rng-mode 1 (the reference's serial draw order) does not shard; use one device");
    P.D = (int)P.devices.size();
    P.A = vgl_max_alleles(&p); P.G = vgl_max_genotypes(&p);
    P.rec0 = a.records == 0;
    P.dump_reads = a.error_qs == 2 && (a.print_qs_err || a.print_gl_err || a.print_qscores);
    P.want_errp = P.dump_reads || (a.error_qs == 2 && P.host_pileup && (a.adjust_qs & 4));
    P.dump_pick = a.error_qs == 1 && a.print_bpe;
    // ---- what comes back from the device: only what this run prints is requested
    // TEXT, --device-text 1: the FORMAT arrays stay on the device (formatted there), DP comes back only for the pileup / per-read listings;
    //       --device-bcf 1: the same path for -O u / -O b -- the tile's FORMAT part comes back as BCF typed vectors (vgl_ctx_bcf_keys)
    // GVCF, --device-gvcf 1: the same for -doGVCF 1 (text, or typed vectors with --device-bcf 1); the blocks are built on the device
    P.path = (a.device_text || (P.bcf && !a.do_gvcf)) ? TEXT : a.device_gvcf ? GVCF : ARRAYS;
    // --device-pileup 1: the read dump and DP stay on the device (the pileup's sample columns come back as text)
    P.want_dp = !P.rec0 && ((a.add_fmt_dp && P.path == ARRAYS) || (a.do_gvcf && P.path != GVCF) || P.host_pileup || P.dump_reads);
    P.stream = a.device_stream != 0;
    // tiles in flight: two per device.  --device-stream 1: three -- an entry stays busy until its members are written, one tile behind
    // the writer, and with two the device would wait for the writer before every other tile
    P.R = (P.stream ? 3 : 2) * P.D;
    return P;
}

// page-locked host array (vgl_host_alloc): grows, never shrinks
template <class T> struct PBuf {
    T* p = nullptr; size_t n = 0;
    void resize(size_t m, int device) {            // device >= 0: place the memory for DMA from that device (vgl_host_alloc_on)
        if (m <= n) return;
        if (p) vgl_host_free(p);
        p = (T*)(device >= 0 ? vgl_host_alloc_on(device, m * sizeof(T)) : vgl_host_alloc(m * sizeof(T)));
        if (!p) die("%s", vgl_last_error());
        n = m;
    }
    T* data() { return p; }
    const T* data() const { return p; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
    PBuf() = default; PBuf(const PBuf&) = delete; PBuf& operator=(const PBuf&) = delete;
    ~PBuf() { if (p) vgl_host_free(p); }
};

// ---- tile buffers (host side of vgl_tile_out): the union of what the modes need; allocate() makes what the plan asks for
struct TileBufs {
    int ns = 0; int64_t t0 = 0; int dev = 0;
    long bad_pos = -1;                        // --device-inf 1: the position of the tile's first site without complete A/C/G/T genotypes
    std::vector<SiteMeta> meta; std::vector<uint8_t> gt;
    // outputs live in page-locked memory (vgl_host_alloc): the device writes them by DMA while the next tile is computed
    PBuf<uint8_t> reads;
    PBuf<int32_t> st, na, nobs, idp, iad, iadf, iadr, dp, pl, ad, adf, adr;
    PBuf<int8_t> a2b; PBuf<float> qs, i16, gl, gp; PBuf<double> errp, pick;
    PBuf<uint8_t> text; PBuf<int64_t> toff; int64_t text_cap = 0;      // --device-text 1: the tile's sample columns and site offsets
    // --device-stream 1: the sample columns stay in body buffer `sbuf` of the device's stream handle; the heads of the tile's records
    // back to back and their offsets go up; sticket: the handle's ticket while the tile's members are on their way
    int sbuf = 0; int32_t sticket = -1; std::string heads; std::vector<int64_t> hoff;
    // --device-gvcf 1: contig id and position per site (in), the items, block offsets and the first / last block's aggregates (out)
    std::vector<int32_t> contig; std::vector<int64_t> pos0;
    PBuf<int32_t> gitems, fdp, fpl, ldp, lpl; PBuf<int64_t> boff; vgl_gvcf_tile g;
    PBuf<uint8_t> ptext; PBuf<int64_t> poff; vgl_pileup_tile pt;      // --device-pileup 1: the tile's pileup columns and site offsets
    PBuf<uint8_t> ftext; PBuf<int64_t> foff; vgl_fetchgl_tile ft;     // --fetch-gl XY: the tile's CSV columns and site offsets
    vgl_tile_out o;
    std::mutex m; std::condition_variable cv; bool done = false;

    // Every buffer of the entry and every pointer of o, g and pt that the run needs -- the non-null pointers of o are what the library
    // copies back.  The entry only ever serves `ctx` on `device` (tiles are dealt round robin): its page-locked buffers are placed next
    // to that device.  sbuf: the entry's body buffer in the device's stream handle.
    void allocate(const Args& a, const RunPlan& P, vgl_ctx* ctx, const int device, const int sbuf_) {
        const size_t TS = (size_t)P.TS, N = (size_t)P.N, A = (size_t)P.A, G = (size_t)P.G, E = TS * N;
        meta.resize(TS); gt.resize(E);
        st.resize(TS, device); na.resize(TS, device); nobs.resize(TS, device); a2b.resize(TS * 5, device);
        memset(&o, 0, sizeof o); memset(&pt, 0, sizeof pt); memset(&g, 0, sizeof g); memset(&ft, 0, sizeof ft);
        o.site_status = st.data(); o.n_alleles = na.data(); o.n_alleles_obs = nobs.data(); o.alleles2acgt = a2b.data();
        if (P.fetch) {
            const int64_t cap = vgl_ctx_fetchgl_bound(ctx, P.TS);
            if (cap < 0) die("--fetch-gl: %s", vgl_last_error());
            ftext.resize((size_t)std::max<int64_t>(cap, 1), device); foff.resize(TS + 1, device);
            ft.text = ftext.data(); ft.text_cap = cap; ft.offsets = foff.data();
        }
        if (P.rec0) return;                                      // (the per-site status and alleles above: a few bytes per site, for the run's summary)
        if (!P.inf) { idp.resize(TS, device); o.info_dp = idp.data(); }         // also tells which sites reach the read loop (TSV dumps)
        if (a.add_info_ad) { iad.resize(TS * A, device); o.info_ad = iad.data(); }
        if (a.add_info_adf) { iadf.resize(TS * A, device); o.info_adf = iadf.data(); }
        if (a.add_info_adr) { iadr.resize(TS * A, device); o.info_adr = iadr.data(); }
        if (a.add_qs) { qs.resize(TS * A, device); o.qs = qs.data(); }
        if (a.add_i16) { i16.resize(TS * 16, device); o.i16 = i16.data(); }
        if (P.want_dp) { dp.resize(E, device); o.fmt_dp = dp.data(); }
        if (P.device_pileup) {
            const int64_t cap = vgl_ctx_pileup_bound(ctx, P.TS);
            if (cap < 0) die("--device-pileup 1: %s", vgl_last_error());
            ptext.resize((size_t)std::max<int64_t>(cap, 1), device); poff.resize(TS + 1, device);
            pt.text = ptext.data(); pt.text_cap = cap; pt.offsets = poff.data();
        }
        switch (P.path) {
        case TEXT:
            text_cap = vgl_ctx_text_bound(ctx, P.TS);
            if (text_cap < 0) die("%s 1: %s", P.bcf ? "--device-bcf" : "--device-text", vgl_last_error());
            toff.resize(TS + 1, device);
            if (P.stream) { sbuf = sbuf_; hoff.resize(TS + 1); }     // (text is not allocated: the bodies stay on the device)
            else text.resize((size_t)std::max<int64_t>(text_cap, 1), device);
            break;
        case GVCF:
            text_cap = vgl_ctx_gvcf_text_bound(ctx, P.TS);
            if (text_cap < 0) die("--device-gvcf 1: %s", vgl_last_error());
            text.resize((size_t)std::max<int64_t>(text_cap, 1), device); toff.resize(TS + 1, device); boff.resize(TS + 1, device);
            gitems.resize(TS * (sizeof(vgl_gvcf_item) / sizeof(int32_t)), device);
            fdp.resize(N, device); ldp.resize(N, device); fpl.resize(G * N, device); lpl.resize(G * N, device);
            contig.resize(TS); pos0.resize(TS);
            g.items = (vgl_gvcf_item*)gitems.data(); g.text = text.data(); g.text_cap = text_cap;
            g.record_offsets = toff.data(); g.block_offsets = boff.data();
            g.first_dp = fdp.data(); g.first_pl = fpl.data(); g.last_dp = ldp.data(); g.last_pl = lpl.data();
            break;
        case ARRAYS:
            if (a.add_gl) { gl.resize(E * G, device); o.gl = gl.data(); }
            if (a.add_pl) { pl.resize(E * G, device); o.pl = pl.data(); }
            if (a.add_gp) { gp.resize(E * G, device); o.gp = gp.data(); }
            if (a.add_fmt_ad) { ad.resize(E * A, device); o.fmt_ad = ad.data(); }
            if (a.add_fmt_adf) { adf.resize(E * A, device); o.fmt_adf = adf.data(); }
            if (a.add_fmt_adr) { adr.resize(E * A, device); o.fmt_adr = adr.data(); }
            break;
        }
        // the per-read dumps: the library stages at most pile_cap reads per sample and site
        if (P.host_pileup) { reads.resize((size_t)P.pile_cap * E, device); o.reads = reads.data(); o.read_capacity = P.pile_cap; }
        if (P.want_errp) { errp.resize((size_t)P.pile_cap * E, device); o.read_errp = errp.data(); o.read_capacity = P.pile_cap; }
        if (P.dump_pick) { pick.resize(TS, device); o.site_pick_err = pick.data(); }
    }
};
