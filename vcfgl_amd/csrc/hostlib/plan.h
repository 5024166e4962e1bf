// hostlib/plan.h -- what a context will launch, as a pure function of its parameters: argument validation, the staging and pool
// capacities, and which build of every kernel serves the run (VglDevParams) -- the project's measured tuning decisions.
// No HIP call, no global: a refusal's text goes into the caller's buffer, the hooks build's environment comes in as a function
// (tests/plan_core_main.cpp runs this header on the CPU).  Needs hostlib/tables.h.
#pragma once
#include <stdarg.h>

#define VGL_READ_CAP_MAX 1020          // the staging layout's largest capacity (four reads per word, below 1024)
#define VGL_PLAN_ERR 512               // bytes of a refusal's text

typedef const char* (*vgl_env_fn)(const char*);
static inline const char* vgl_no_env(const char*) { return nullptr; }

// what vgl_ctx_create needs beside VglDevParams
struct VglPlanExtra {
    vgl_rng_layout lay;                // the caller's windows, or the default ones
    std::vector<double> q2gl;          // [3][257] (the fixed-score terms of VglDevParams come from it)
    uint32_t redo_cap = 0;             // entries per partition of k_redo's list
    size_t gl2_redo_words = 0;         // bitmap words over the workgroups of k_gl2
    bool pois_zt = false, gl2_run = false, dbg_words = false;      // tables / words to allocate
};

static inline int plan_fail(char* err, int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(err, VGL_PLAN_ERR, fmt, ap); va_end(ap);
    return code;
}

// PROGRAM_WILL_ADD_UNOBSERVED (shared.h:151-152): <*> / <NON_REF> appended => 5 alleles
extern "C" int32_t vgl_max_alleles(const vgl_params* p) {
    const int d = p->do_unobserved;
    return (d == 1 || d == 2 || d == 4 || d == 5) ? 5 : 4;
}
extern "C" int32_t vgl_max_genotypes(const vgl_params* p) { return vgl_max_alleles(p) == 5 ? 15 : 10; }

static inline double max_depth(const vgl_params* p) {
    double dmax = p->depth;
    if (p->depths) { dmax = 0; for (int i = 0; i < p->n_samples; i++) if (p->depths[i] > dmax) dmax = p->depths[i]; }
    if (!(dmax >= 0)) dmax = 0;
    return dmax;
}

static inline vgl_rng_layout plan_default_layout(const vgl_params* p) {
    vgl_rng_layout out;
    const uint64_t d = (uint64_t)ceil(max_depth(p));
    const uint64_t s0 = 64;                                   // depth draws (Poisson)
    const uint64_t s1 = 4 * d + 64;                           // one haplotype draw per read
    const uint64_t s2 = 3 * s1;                               // error test + wrong base + strand
    const uint64_t qstride = 32;                              // draws reserved per beta deviate
    const uint64_t s3 = (p->error_qs == 2) ? qstride * s1 : 64;
    out.qs_read_stride = qstride;
    out.off[0] = 0; out.off[1] = s0; out.off[2] = s0 + s1; out.off[3] = s0 + s1 + s2;
    out.block = (s0 + s1 + s2 + s3) | 1;
    return out;
}

// W of vgl_site_hash(): the largest W with 2^W * n_samples * block <= 2^48, the period of rand48
// (-1: not even one site's windows fit the period -- block * n_samples > 2^48)
static inline int site_hash_bits(const vgl_params* p) {
    const vgl_rng_layout lay = p->layout.block ? p->layout : plan_default_layout(p);
    const uint64_t raw = (uint64_t)((((unsigned __int128)1 << 48) / lay.block) / (uint64_t)p->n_samples);
    if (raw < 1) return -1;
    int W = 0;
    while (W < 40 && (2ULL << W) <= raw) ++W;
    return W;
}
#define VGL_MSG_PERIOD "VGL_RNG_TILE: layout.block x n_samples exceeds the 2^48 period of rand48: not even one site is addressable"

static inline int errprob_to_qs_fixed(const vgl_params* p, double ep, int* qs, int* adjqs, char* err) {
    // vcfgl.cpp:1668-1694
    const int adj = p->adjust_qs != 0;
    int q = -1, aq = -1;
    if (0.0 == ep) { q = 63; aq = 63; }
    else if (1.0 == ep) { q = 0; aq = 0; }
    else if (0.0 < ep && ep < 1.0) {
        const double tmp = -10.0 * log10(ep);
        q = (int)tmp;
        if (adj) aq = (int)(tmp + p->adjust_by);
    } else return plan_fail(err, VGL_E_ARG, "Bad error probability value: %f", ep);
    auto bins = [&](int in, int* out) -> int {
        for (int i = 0; i < p->n_qs_bins; ++i)
            if (in >= p->qs_bins[3 * i] && in <= p->qs_bins[3 * i + 1]) { *out = p->qs_bins[3 * i + 2]; return 0; }
        return plan_fail(err, VGL_E_QSBIN, "Could not find a range for qs value %d", in);
    };
    if (p->n_qs_bins != 0) {
        int r = bins(q, &q); if (r) return r;
        if (adj) { r = bins(aq, &aq); if (r) return r; }
    } else {
        q = q > 63 ? 63 : q;
        if (adj) aq = aq > 63 ? 63 : aq;
    }
    if (!adj) aq = -1;
    *qs = q; *adjqs = aq;
    return VGL_OK;
}

// the arguments alone (what vgl_ctx_create refuses before it looks for a device)
static inline int vgl_plan_validate(const vgl_params* p, int max_sites, char* err) {
    if (p->abi_version != VGL_ABI_VERSION) return plan_fail(err, VGL_E_ARG, "abi version mismatch");
    if (p->n_samples <= 0) return plan_fail(err, VGL_E_ARG, "n_samples must be positive");
    if (max_sites <= 0) return plan_fail(err, VGL_E_ARG, "max_sites_per_tile must be positive");
    if (p->gl_model != 1 && p->gl_model != 2) return plan_fail(err, VGL_E_ARG, "[Bad argument value: '--gl-model %d'] Allowed range is [1,2]", p->gl_model);
    if (p->error_qs < 0 || p->error_qs > 2) return plan_fail(err, VGL_E_ARG, "[Bad argument value: '--error-qs %d'] Allowed range is [0,2]", p->error_qs);
    if (p->do_unobserved < 0 || p->do_unobserved > 5) return plan_fail(err, VGL_E_ARG, "[Bad argument value: '-doUnobserved %d'] Allowed range is [0,5]", p->do_unobserved);
    if (!(p->error_rate >= 0.0 && p->error_rate < 1.0)) return plan_fail(err, VGL_E_ARG, "[Bad argument value: '--error-rate %f'] Allowed range is [0,1)", p->error_rate);
    if (p->n_qs_bins < 0 || p->n_qs_bins > VGL_MAX_QS_BINS) return plan_fail(err, VGL_E_ARG, "at most %d qs bins are supported", VGL_MAX_QS_BINS);
    // a staged read is one byte, score << 2 | base, and the two-byte items / LDS sum words of k_sample<2> give a score six bits too: a binned score above
    // 63 (the reference takes --qs-bins values up to 255, io.cpp:161-163; its own default scores stop at CAP_BASEQ = 63) would be cut, so such a run is refused
    if (p->n_qs_bins > 0 && !p->qs_bins) return plan_fail(err, VGL_E_ARG, "n_qs_bins > 0 without qs_bins");
    for (int i = 0; i < p->n_qs_bins; ++i)
        if (p->qs_bins[3 * i + 2] < 0 || p->qs_bins[3 * i + 2] > 63)
            return plan_fail(err, VGL_E_UNSUPPORTED, "--qs-bins: bin %d maps to quality score %d; the device path stages quality scores in six bits (0 ... 63)", i, p->qs_bins[3 * i + 2]);
    if (p->gl_model == 1 && p->precise_gl) return plan_fail(err, VGL_E_ARG, "Precise genotype likelihood error (--precise-gl 1) is not supported with genotype likelihood model 1 (--gl-model 1).");
    if (p->rng_mode != VGL_RNG_TILE && p->rng_mode != VGL_RNG_SERIAL) return plan_fail(err, VGL_E_ARG, "rng_mode must be VGL_RNG_TILE or VGL_RNG_SERIAL");
    if (p->out_layout != VGL_LAYOUT_PLANES && p->out_layout != VGL_LAYOUT_SAMPLE_MAJOR) return plan_fail(err, VGL_E_ARG, "out_layout must be VGL_LAYOUT_PLANES or VGL_LAYOUT_SAMPLE_MAJOR");
    if (p->rng_mode == VGL_RNG_TILE && p->error_qs != 0 && p->beta_sampler != VGL_BETA_RAND48)
        return plan_fail(err, VGL_E_UNSUPPORTED, "the mt19937 beta sampler is one global serial stream: use VGL_RNG_SERIAL, or VGL_BETA_RAND48 with VGL_RNG_TILE");
    if (p->depths) { for (int i = 0; i < p->n_samples; i++) if (!(p->depths[i] >= 0.0)) return plan_fail(err, VGL_E_ARG, "depths must be >= 0"); }
    else if (!(p->depth >= 0.0)) return plan_fail(err, VGL_E_ARG, "[Bad argument value: '--depth %f'] Allowed range is [0,500]", p->depth);
    return VGL_OK;
}

// the quality-score pool of k_sample<2> (error_qs 2) and the choice between its builds
static inline void plan_pool(const vgl_params* p, vgl_env_fn env, VglDevParams& D) {
    auto env_int = [&](const char* name, int dflt) { const char* v = env(name); return v ? atoi(v) : dflt; };
    const int N = p->n_samples;
    int pool_want = 0; double pool_lmax = 0.0;
    {   // quality-score pool of one wavefront: the summed depth of its (up to) 64 samples
        double lmax = 0.0;
        for (int c0 = 0; c0 < N; c0 += 64) {
            double l = 0.0;
            for (int s = c0; s < N && s < c0 + 64; s++) l += p->depths ? p->depths[s] : p->depth;
            if (l > lmax) lmax = l;
        }
        int pc = (int)ceil(lmax + 8.0 * sqrt(lmax) + 64.0);
        pc = (pc + 63) & ~63;
        pool_want = pc; pool_lmax = lmax;              // (the two-byte-item builds below take their own limit from these)
        if (pc > 1920) pc = 1920;                      // 520 + 5 x 1920 B per wavefront: 16 wavefronts (the 4 per SIMD the kernel is
                                                       // built for) fit a CU's 160 KB LDS; larger pools run in several segments
        D.pool_cap = pc;
        D.pool_lds_bytes = (576 + 4 * (pc + 2) + pc + 7) & ~7;         // stream bases | gamma constants by stage | item slots (+ zero slot, counter) | bases
    }
    // The deferred builds of k_sample<2> (5 wavefronts per SIMD, no double-precision fallback code in the kernel: the reads a float32
    // bound cannot settle go to k_redo) serve every tag surface -- LEAN 2 the default one, LEAN 3 (round 4) -addQS / -addI16, strand tags
    // and --adjust-qs, with or without --precise-gl 1 (k_redo then also rewrites the read's staged error probability).  The build with
    // the fallbacks inline (LEAN 0 / 1) remains for a per-read dump and for a beta shape parameter below 8 (the gamma sampler's bounded
    // test then leaves its series' range |a2 x| <= 1/3 too often).
    D.dbg_redo_every = env_int("VGL_DEBUG_REDO_EVERY", 0);
    // the tag surface needs none of the owners' optional per-read state (quality sums, strand draws, --adjust-qs): the LEAN builds of k_sample
    bool bins_below_255 = true;
    for (int i = 0; i < p->n_qs_bins; ++i) if (p->qs_bins[3 * i] > 254 || p->qs_bins[3 * i + 1] > 254) bins_below_255 = false;
    D.lean_ok = (!D.need_qsum && !D.sample_strand && !D.need_adf && p->adjust_qs == 0 && !env("VGL_NO_LEAN")) ? 1 : 0;
    D.defer_ok = (!D.serial && p->error_qs == 2 &&
                  !D.gx.changed && !D.gy.changed && D.gx.alpha0 >= 8.0 && D.gy.alpha0 >= 8.0 && !env("VGL_NO_DEFER") && !env("VGL_DEBUG_QS_EXACT") && !env("VGL_NO_LEAN") &&
#ifdef VGL_PREC_F64
                  !(!p->precise_gl && (D.read_cap > 256 || !bins_below_255))) ? 1 : 0;   // (the two-byte items of the float32 builds hold a read index of 8 bits
#else
                  !(D.read_cap > 256 || !bins_below_255)) ? 1 : 0;                       // (the two-byte items of the float32 builds hold a read index of 8 bits
#endif
                                                                             // and look binned scores up in a 256-entry table: other runs take the inline build)
    D.qsum_lds = (D.defer_ok && !D.lean_ok && ((p->adjust_qs & 3) == 0 || (p->adjust_qs & 3) == 3) && D.read_cap <= 130) ? 1 : 0;    // 130 x 63 = 8190 < 2^13, 130 x 63^2 = 515970 < 2^19
    if (!D.defer_ok) return;
    // pools of the deferred builds.  Without --precise-gl 1 (float32 loop, round 5) an item is TWO bytes: 576 B + 2 x (items + 2) (+ 1 KB of
    // quality-sum words with qsum_lds, + 256 B of binned scores with --qs-bins) -- 2240 items (depth 30 in one segment) leave LDS for the eight
    // wavefronts per SIMD k_sample<2, LEAN 2> is built for (32 x 5.1 KB in a CU's 160 KB).  With --precise-gl 1 (float64 loop): five bytes, 1472
    // items = 5 wavefronts per SIMD (1416 with the 512 B of sum words)
#if !defined(VGL_POOL_F64) && !defined(VGL_PREC_F64)
    const bool p16 = true;                                   // (round 6: --precise-gl 1 runs the float32 loop too, + 32 bytes of double constants)
#elif !defined(VGL_POOL_F64)
    const bool p16 = !p->precise_gl;
#else
    const bool p16 = false;
#endif
    const int extra16 = (D.qsum_lds ? 1024 : 0) + (p->n_qs_bins ? 256 : 0) + (p->precise_gl ? 32 : 0);
    const int cap_defer = p16 ? ((5120 - 576 - 8 - (D.lean_ok ? (p->n_qs_bins ? 256 : 0) : 0)) / 2 / 64 * 64) : (D.qsum_lds ? 1416 : 1472);
    // the float32 build of the default tag surface as two kernels (k_sample_seg, vgl_sample.hip) when a wavefront's reads fit one pool up to 8 sigma
    // (a pool that holds the summed depth + 4 sigma: 3e-5 of the wavefronts go through the list -- depth 30 with --qs-bins: 2112 items for 1920 + 4 x 43.8)
    D.seg_split = (p16 && (double)cap_defer >= pool_lmax + 4.0 * sqrt(pool_lmax) && !env("VGL_NO_SEG_SPLIT")) ? 1 : 0;
    // round 6: the two-byte-item builds take min(summed depth + 8 sigma, what eight wavefronts per SIMD leave) -- the five-byte limit of 1920 above
    // was still applied first, so that depth 30 (mean 1920 reads per wavefront) ran half of its wavefronts in two segments
    if (p16) D.pool_cap = pool_want;
    if (D.pool_cap > cap_defer) D.pool_cap = cap_defer;
    if (env("VGL_DEBUG_POOL_CAP")) { D.pool_cap = std::max(64, std::min(D.pool_cap, atoi(env("VGL_DEBUG_POOL_CAP")) / 64 * 64)); if (env_int("VGL_SEG_SPLIT", 0)) D.seg_split = p16 ? 1 : 0; }   // test hooks: small pools, the split forced on
    D.seg_limit = env_int("VGL_DEBUG_SEG_LIMIT", D.pool_cap);
    if (D.seg_limit > D.pool_cap) D.seg_limit = D.pool_cap;
    D.pool_lds_bytes = p16 ? (((576 + 2 * (D.pool_cap + 2) + 7) & ~7) + extra16)
                           : (((576 + 4 * (D.pool_cap + 2) + D.pool_cap + 7) & ~7) + (D.qsum_lds ? 512 : 0));   // (vgl_launch_sample sizes the LDS of the build it launches)
}

// the fixed-score terms (--error-qs 0 / 1) and the beta shapes (--error-qs 1 / 2)
static inline int plan_scores(const vgl_params* p, const std::vector<double>& q2gl, VglDevParams& D, char* err) {
    int rc = VGL_OK;
    D.pre_q = D.pre_adjq = -1;
    if (p->error_qs == 0 || p->error_qs == 1) {                  // preCalc, vcfgl.cpp:1661-1743
        if ((rc = errprob_to_qs_fixed(p, p->error_rate, &D.pre_q, &D.pre_adjq, err))) return rc;
        if ((p->adjust_qs & 3) && D.pre_adjq < 0) return plan_fail(err, VGL_E_ADJQ, "--adjust-qs %d --adjust-by %g: the adjusted quality score is negative", p->adjust_qs, p->adjust_by);
        if (p->gl_model == 2) {
            if (!p->precise_gl) {
                const int q = (p->adjust_qs & 1) ? D.pre_adjq : D.pre_q;
                D.pre_homT = q2gl[q]; D.pre_het = q2gl[257 + q]; D.pre_homF = q2gl[514 + q];
            } else {
                const double e = p->error_rate;
                if (0.0 == e) { D.pre_homT = 0; D.pre_het = -0.3010299956639812; D.pre_homF = -INFINITY; }
                else { D.pre_homT = log10(1.0 - e); D.pre_het = log10((1.0 - e) / 2.0 + e / 6.0); D.pre_homF = log10(e) - 0.47712125471966244; }
            }
        }
    }
    if (p->error_qs != 0) {                                       // rng.h:455-477
        const double mean = p->error_rate, var = p->beta_variance;
        if (!(mean > 0.0 && mean < 1.0 && var > 0.0)) return plan_fail(err, VGL_E_ARG, "--error-qs 1 or 2 requires 0 < --error-rate < 1 and --beta-variance > 0");
        const double oom = 1.0 / mean;
        const double a = (((1.0 - mean) / var) - oom) * pow(mean, 2), b = a * (oom - 1);
        if (a <= 0.0 || b <= 0.0) return plan_fail(err, VGL_E_ARG, "Beta shape parameters must be positive (alpha=%f beta=%f); use different --error-rate / --beta-variance", a, b);
        gamma1_init(&D.gx, a); gamma1_init(&D.gy, b);
        // k_sample<2>'s sure-accept bound: far above the rounding of the reference's own right-hand side
        // 0.5 x^2 + a1 (1 - v + log v), which is about 4e-16 a1 + 1e-16 x^2
        D.sure_margin = 1e-9 + 1e-14 * std::max(D.gx.a1, D.gy.a1);
        D.beta_a = a; D.beta_b = b;
    }
    return VGL_OK;
}

// which likelihood kernels: the fused one, k_gl2 or k_gl; and k_redo's list
static inline void plan_gl(const vgl_params* p, int max_sites, vgl_env_fn env, VglDevParams& D, VglPlanExtra& X) {
    auto env_int = [&](const char* name, int dflt) { const char* v = env(name); return v ? atoi(v) : dflt; };
    const int N = p->n_samples;
    // one workgroup per site does everything (k_gl<.., FUSED>, vgl_gl.hip): sampling with one fixed score, the site's allele order and the
    // likelihoods, with nothing staged in HBM between them
    // (round 4: sites of more than 512 samples split over up to four consecutive workgroups, up to 128 staged reads.  The kernel also takes its
    // depths from k_depth where the rejection method draws them, but at depth 20 the three kernels measure faster, so that stays behind the
    // hooks build's VGL_FUSE_DEEP; VGL_FUSE_MAX_SPLIT: tuning hook)
    D.fused_split = N <= 512 ? 1 : (N + 511) / 512;
    D.fused = (!D.serial && p->error_qs == 0 && p->gl_model == 2 && !p->precise_gl && (D.depth_pre == 2 || D.depth_pre == 1) && !D.need_qsum && !D.sample_strand &&
               (D.depth_pre == 2 || env_int("VGL_FUSE_DEEP", 0)) &&      // measured (tools/fuse_ab.sh): at depth 20 the three kernels are faster (1.50e10 against 1.40e10 at N = 500, 1.55e10 against 1.36e10 at N = 1000)
               !D.need_adf && p->adjust_qs == 0 && N > 128 && D.fused_split <= env_int("VGL_FUSE_MAX_SPLIT", 4) && D.read_cap <= 128 &&
               !env("VGL_NO_FUSE") && !env("VGL_NO_LEAN")) ? 1 : 0;
    if (!D.fused) D.fused_split = 0;
    {
        // GL model 2, three-kernel path: k_gl2 (two evaluations per thread: vgl_gl.hip) where it measured faster than k_gl (tools/gl2x_sweep.py,
        // k_gl's time per tile with k_gl2 / with k_gl): one fixed score 0.77 - 0.85 at depths 12 ... 60, per-read scores 0.99 at depth 16, 0.95 at
        // 20, 0.91 at 30, 0.87 at 40.  Its pool holds the upper accumulator rows of 256 three- / four-base evaluations of a workgroup's 1024:
        // beyond ~0.8 expected base-call errors per evaluation workgroups start to overflow into k_gl_redo, and k_gl is the better choice.
        // Planes layout, sort on, no --precise-gl 1
        double dsum = 0.0;
        for (int i = 0; i < N; i++) dsum += p->depths ? p->depths[i] : p->depth;
        const bool can = p->gl_model == 2 && !p->precise_gl && D.gl_sort != 0 && D.gl_wpb == 8 && p->out_layout == VGL_LAYOUT_PLANES && !D.fused;
        const double dmean = dsum / (double)N, errs = dmean * p->error_rate;      // expected base-call errors per evaluation: what makes three- and four-base evaluations
        // (at the bench's full tile size per-read scores at depth 20 measured equal with the first version, 2.40-2.43 ms either way, depth 30 -6.5 %; and with
        //  GP or the AD-type FORMAT tags k_gl2's two epilogues per thread cost more than they hide -- all tags: 4.9 -> 5.7 ms: vgl_launch_gl looks at the tile)
        // (... and without the GP / AD epilogue in the shipped k_gl2, depth 20 measures 2.355-2.388 against 2.397-2.413 ms: from depth 18)
        const bool want = dmean >= (p->error_qs != 2 ? 12.0 : 18.0) && errs <= 0.8;
        D.gl2x = can ? env_int("VGL_GL2X", want ? 1 : 0) : 0;                    // (VGL_GL2X=2: also for tiles with GP / FORMAT/AD*)
        D.dbg_gl2_ovc = env_int("VGL_DEBUG_GL2_OVC", 0);
    }
    if (D.gl2x) X.gl2_redo_words = ((size_t)max_sites * D.chunks / 16 + 1 + 31) / 32;
    if (D.defer_ok) {
        // about 6 reads in 10^4 take this path at C3 / C4 (tools/redo_rate.py); the list has room for 1 in 64 of the staging capacity
        // (VGL_DEBUG_REDO_CAP: test hook), what does not fit is marked in a bitmap over the staged reads (all zero between tiles)
        const size_t reads = (size_t)max_sites * N * (size_t)D.read_cap;
        X.redo_cap = (uint32_t)std::min<size_t>(0xFFFFFFF0u, env("VGL_DEBUG_REDO_CAP") ? (size_t)atol(env("VGL_DEBUG_REDO_CAP")) : std::max<size_t>(65536, reads / 64));
        X.redo_cap /= VGL_REDO_PARTS;                                     // entries per partition (0 with a tiny VGL_DEBUG_REDO_CAP: every entry goes to the bitmap)
    }
}

// everything vgl_ctx_create decides from validated arguments.  cap_override: the staging capacity of the sibling context of a tile
// with a deeper draw (0: from the depth)
static inline int vgl_plan_derive(const vgl_params* p, int max_sites, int cap_override, vgl_env_fn env, VglDevParams* Dp, VglPlanExtra* Xp, char* err) {
    auto env_int = [&](const char* name, int dflt) { const char* v = env(name); return v ? atoi(v) : dflt; };
    VglDevParams& D = *Dp; VglPlanExtra& X = *Xp;
    memset(&D, 0, sizeof D);
    const double dmax = max_depth(p);
    const int N = p->n_samples;
    D.n_samples = N; D.chunks = (N + 63) / 64;
    D.A = vgl_max_alleles(p); D.G = vgl_max_genotypes(p);
    int cap = (int)ceil(dmax + 8.0 * sqrt(dmax) + 16.0);
    D.read_cap = (cap + 3) & ~3;
    if (env("VGL_DEBUG_READ_CAP")) D.read_cap = (atoi(env("VGL_DEBUG_READ_CAP")) + 3) & ~3;   // test hook: force the overflow path (a multiple of 4: staged reads are packed four per word)
    if (cap_override) D.read_cap = cap_override;                  // the sibling context of a tile with a deeper draw (vgl_tile_wait)
    if (D.read_cap > 1023) return plan_fail(err, VGL_E_ARG, "mean depth too large for the staging layout");
    D.error_qs = p->error_qs; D.gl_model = p->gl_model; D.precise_gl = p->precise_gl; D.adjust_qs = p->adjust_qs;
    D.n_qs_bins = p->n_qs_bins; D.do_unobserved = p->do_unobserved; D.rm_invar_sites = p->rm_invar_sites;
    D.rm_empty_sites = p->rm_empty_sites;
    D.sample_strand = (p->add_i16 || p->add_fmt_adf || p->add_fmt_adr || p->add_info_adf || p->add_info_adr) ? 1 : 0;  // shared.h:160-161
    D.per_sample_depth = p->depths ? 1 : 0;
    D.need_qsum = (p->add_qs || p->add_i16) ? 1 : 0; D.need_qsumsq = p->add_i16 ? 1 : 0; D.need_adf = D.sample_strand;
    D.i16_mapq = p->i16_mapq; D.add_i16 = p->add_i16;
    D.out_layout = p->out_layout;
    D.adjust_by = p->adjust_by;
    D.serial = (p->rng_mode == VGL_RNG_SERIAL) ? 1 : 0;
    D.gl1_deep = (p->gl_model == 1 && D.read_cap > 255) ? 1 : 0;
    if (p->gl_model == 1 && p->error_qs == 2) D.gl1_nc = std::min(255, D.read_cap) + 1;    // per-read qScores: the compact fk x beta table (tables.h)
    D.stage_fixed = (p->gl_model != 1 || D.gl1_deep || (p->add_i16 && !D.serial)) ? 1 : 0;
    D.scout_lds_bytes = ((size_t)p->n_samples * 9 <= 144 * 1024) ? (int32_t)(((size_t)p->n_samples * 9 + 15) & ~(size_t)15) : 0;
    D.beta_std = (p->beta_sampler == VGL_BETA_STD) ? 1 : 0;
    D.beta_chain = (D.serial && D.beta_std && p->error_qs == 2 && !env("VGL_NO_BETA_CHAIN")) ? 1 : 0;
    {   // depth mode: k_depth pays for the rejection sampler (lambda >= 12, rng.h:300); the product method's short loop
        // stays inside k_sample, which is specialised for "all product" (2) and "mixed" (0)
        double dmin = p->depth, dmx = p->depth;
        if (p->depths) { dmin = dmx = p->depths[0]; for (int i = 1; i < N; i++) { dmin = std::min(dmin, p->depths[i]); dmx = std::max(dmx, p->depths[i]); } }
        D.depth_pre = D.serial ? 0 : (dmin >= 12.0 ? 1 : (dmx < 12.0 ? 2 : 0));
    }
    // k_gl lane order: 0 natural, 1 depth-sorted lanes storing their own evaluations (4-byte pieces), 2 depth-sorted lanes and
    // natural-order stores through LDS -- the last is at least as fast as the others from depth 5 (config C5) to depth 30
    D.gl_sort = env_int("VGL_GL_SORT", dmax >= 1.0 ? 2 : 0);
    D.gl_flip2 = env_int("VGL_GL_FLIP2", 1);
    D.gl_wpb = env_int("VGL_GL_WPB", D.gl_sort ? 8 : 4);
    D.slow_period = env_int("VGL_SLOW_PERIOD", 4);
    if (D.slow_period < 1) D.slow_period = 1;
    D.slow_period_n = env_int("VGL_SLOW_PERIOD_N", 4);
    if (D.slow_period_n < 1) D.slow_period_n = 1;
    D.xcd_map = env_int("VGL_XCD_MAP", 1);
    D.dbg_phase = env_int("VGL_DEBUG_PHASE", 0);
    D.dbg_stamps = env_int("VGL_DEBUG_STAMPS", 0);
    D.dbg_fuse_alone = env_int("VGL_DEBUG_FUSE_ALONE", 0);
    D.dbg_depth_chunk = env_int("VGL_DEPTH_CHUNK", 0);
    D.dbg_qs_exact = env_int("VGL_DEBUG_QS_EXACT", 0);
    for (int i = 0; i < p->n_qs_bins * 3; i++) D.qs_bins[i] = p->qs_bins[i];
    D.err_thresh = (uint64_t)ceil(ldexp(p->error_rate, 48));

    X.q2gl = build_q2gl();
    const int rc = plan_scores(p, X.q2gl, D, err);
    if (rc != VGL_OK) return rc;
    plan_pool(p, env, D);
    pois_init(&D.pois0, p->depths ? 0.0 : p->depth);

    // rand48 addressing
    X.lay = p->layout.block ? p->layout : plan_default_layout(p);
    D.x0 = ((((uint64_t)(uint32_t)p->seed) << 16) | 0x330EULL) & VGL_MASK48;   // io.cpp:1054-1061
    for (int k = 0; k < 4; k++) D.off[k] = aff_pow(X.lay.off[k]);
    VglAffine js = aff_pow_of(aff_pow(X.lay.block), (uint64_t)N);  // one site = N evaluation blocks
    for (int b = 0; b < 40; b++) { D.site_pow[b] = js; js = aff_compose(js, js); }
    if (!D.serial) {
        D.site_hash_bits = site_hash_bits(p);
        if (D.site_hash_bits < 0) return plan_fail(err, VGL_E_ARG, VGL_MSG_PERIOD);
        D.depth_magic = (uint32_t)((1ULL << 32) / (uint64_t)N + 1ULL);
        // INFO/I16 fields 13-16 (k_tail, vgl_gl.hip): the same windows of a second rand48 sequence; the staging capacity fits a window
        if (p->add_i16 && (uint64_t)D.read_cap > X.lay.block)
            return plan_fail(err, VGL_E_ARG, "-addI16: layout.block (%llu) is smaller than the staging capacity of %d reads", (unsigned long long)X.lay.block, D.read_cap);
    }
    if (p->error_qs == 2 && X.lay.qs_read_stride == 0) return plan_fail(err, VGL_E_ARG, "layout.qs_read_stride must be > 0 with --error-qs 2");
    plan_gl(p, max_sites, env, D, X);
    X.pois_zt = !p->depths && !D.pois0.st12 && !env("VGL_NO_POIS_ZT");
    X.gl2_run = p->gl_model == 2 && p->error_qs != 2 && !env("VGL_NO_GL2_RUN");
    X.dbg_words = env("VGL_DEBUG_STAMPS") || env("VGL_DEBUG_PHASE");
    return VGL_OK;
}

static inline int vgl_plan(const vgl_params* p, int max_sites, int cap_override, vgl_env_fn env, VglDevParams* D, VglPlanExtra* X, char* err) {
    const int rc = vgl_plan_validate(p, max_sites, err);
    return rc != VGL_OK ? rc : vgl_plan_derive(p, max_sites, cap_override, env, D, X, err);
}

// the part of vgl_ctx_info the plan decides (every field but device, workspace_bytes and test_hooks)
static inline void vgl_plan_info(const VglDevParams& D, int rng_mode, int max_sites, vgl_ctx_info_t* r) {
    r->abi_version = VGL_ABI_VERSION;
    r->n_samples = D.n_samples; r->max_sites_per_tile = max_sites; r->max_alleles = D.A; r->max_genotypes = D.G;
    r->rng_mode = rng_mode;
    r->depth_mode = D.serial ? VGL_DEPTH_SERIAL_SCOUT : D.depth_pre;
    r->fused = D.fused; r->fused_split = D.fused ? (D.fused_split > 0 ? D.fused_split : 1) : 0;
    r->sample_lean = D.serial ? 0 : (D.lean_ok ? ((D.error_qs == 2 && D.defer_ok) ? 2 : 1) : ((D.error_qs == 2 && D.defer_ok) ? 3 : 0));
    r->gl_sort = D.gl_sort; r->gl_wpb = D.gl2x ? 16 : ((D.gl_model == 2 && D.gl_wpb == 8) ? 8 : 4);   // 16: k_gl2 (sixteen natural wavefronts, two evaluations per thread)
    r->read_cap = D.read_cap; r->pool_cap = D.error_qs == 2 ? D.pool_cap : 0; r->pool_lds_bytes = D.error_qs == 2 ? D.pool_lds_bytes : 0;
    r->rng_tile_max_sites = D.serial ? 0 : ((int64_t)1 << D.site_hash_bits);
}
