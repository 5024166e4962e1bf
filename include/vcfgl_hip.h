/*
 * vcfgl_hip.h -- C ABI of the MI355X (gfx950) implementation of vcfgl's per-site
 * genotype-likelihood simulation hot path.
 *
 * The reference (isinaltinkaya/vcfgl) has no plugin / FFI surface.  Its de-facto
 * boundary for this path is
 *
 *     static int simulate_record_values(simRecord* sim)       vcfgl.cpp:327
 *     void (*calculate_gls)(simRecord* sim)                   vcfgl.cpp:222, sole call :788
 *
 * whose inputs are the parsed flags (`argStruct* args`, io.h:40-148), the decoded true
 * genotypes (`true_gts_acgt_int`, vcfgl.cpp:66, filled :132-147) and the RNG states, and
 * whose outputs are the simRecord arrays consumed by simRecord::add_tags()
 * (bcf_utils.cpp:426-507).  The entry points below are what a record loop calls IN PLACE
 * of `simulate_record_values` (vcfgl.cpp:1522,1552,1611): it batches records into a tile,
 * calls vgl_simulate_tile*, and feeds every site of the returned tile to add_tags().
 *
 * Everything is plain C: pointers, sizes, int error codes.  The library never calls
 * exit(); the reference's ERROR()/ASSERT() exits (shared.h:292-327) become VGL_E_* codes
 * plus a message retrievable with vgl_last_error().
 *
 * Tile layout (structure of arrays, sample index fastest so that one wavefront = 64
 * consecutive samples of one site reads and writes contiguous 256-byte segments):
 *
 *     per (site, sample) scalar      x[site * n_samples + sample]
 *     per (site, k, sample) plane    x[(site * K + k) * n_samples + sample]      (VGL_LAYOUT_PLANES, the default)
 *     per site vector                x[site * K + k]
 *
 * With vgl_params.out_layout = VGL_LAYOUT_SAMPLE_MAJOR (ABI 4) the multi-valued FORMAT arrays come back as the reference
 * itself keeps them (simRecord::gl_arr etc., bcf_utils.h:193-196), one slab per site: see VGL_LAYOUT_* below.
 */
#ifndef VCFGL_HIP_H
#define VCFGL_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGL_ABI_VERSION 7
/* the library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table */
#define VGL_API __attribute__((visibility("default")))

/* ---- error codes (returned by every entry point; 0 = success) ----------------------- */
#define VGL_OK              0
#define VGL_E_ARG          (-1)  /* bad parameter value (reference: io.cpp:757-1000 range checks) */
#define VGL_E_NODEVICE     (-2)  /* no HIP device / HIP runtime error                            */
#define VGL_E_NOMEM        (-3)  /* allocation failure                                           */
#define VGL_E_CAPACITY     (-4)  /* a per-sample read depth exceeded the staging capacity (mean + 8 sigma + 16 reads) where the tile could not be run
                                    again: the host-buffer entry points (vgl_simulate_tile, vgl_tile_wait) run such a tile once more on an internal
                                    context with the layout's largest capacity, 1020 reads (the reference grows its buffers, bcf_utils.cpp:618-648), so
                                    this code is left to vgl_ctx_check() (device buffers), VGL_RNG_SERIAL, per-read dumps, pileups formatted on the
                                    device (vgl_ctx_pileup_next) and draws beyond 1020 reads */
#define VGL_E_UNSUPPORTED  (-5)  /* flag combination not implemented on the device path (the mt19937 beta sampler in VGL_RNG_TILE) */
#define VGL_E_QSBIN        (-6)  /* "Could not find a range for qs value" (vcfgl.cpp:63)         */
#define VGL_E_ADJQ         (-7)  /* --adjust-qs 1|2 met a read without a valid adjusted quality score: error probability
                                    exactly 0 or 1, or a negative adjusted score (the reference exits on
                                    ASSERT(adjqScore_i != -1), vcfgl.cpp:558, and ASSERT(qs >= 0 ...), gl_methods.cpp:101) */
#define VGL_E_SETAL        (-8)  /* vgl_ctx_set_alleles: a site's target list names an allele its record does not have (misc/setAlleles
                                    reads uninitialised memory there); vgl_last_error() names the absolute site */

/* ---- per-site status (reference: return value of simulate_record_values) ------------- */
#define VGL_SITE_OK            0
#define VGL_SITE_SKIP_INVAR  (-3) /* one simulated allele + --rm-invar-sites&4 (vcfgl.cpp:675-681) */
#define VGL_SITE_SKIP_EMPTY  (-4) /* INFO/DP==0 + --rm-empty-sites 1           (vcfgl.cpp:400-402) */
#define VGL_SITE_NO_READS      1  /* INFO/DP==0, site kept: simulate_site_with_no_reads (:228-315) */

/* ---- missing / special values (htslib encodings that add_tags() expects) ------------- */
#define VGL_FLOAT_MISSING_BITS 0x7F800001u  /* bcf_float_missing */
#define VGL_INT32_MISSING      ((int32_t)0x80000000) /* bcf_int32_missing = INT32_MIN */
#define VGL_GT_MISSING         0xF          /* allele nibble: missing true genotype */

/* ---- RNG addressing modes ------------------------------------------------------------ */
/* All uniform streams are the reference's own generator: glibc rand48,
 * X <- (0x5DEECE66D * X + 0xB) mod 2^48, u = X * 2^-48, X0 = (seed << 16) | 0x330E
 * (io.cpp:1054-1061, shared.h:17-22).  They differ in WHICH draw index a consumer uses. */
#define VGL_RNG_TILE    0  /* counter addressed: each (site,sample) owns a private window      */
#define VGL_RNG_SERIAL  1  /* the reference's serial consumption order: reproduces the reference
                              program bit for bit.  On the device scout kernels resolve the serial
                              stream chains (64 stream positions at a time; the std::mt19937 beta
                              stream as a parallel chain over the generator output) and record the
                              stream states per (site,sample); everything else runs in parallel.
                              Tiles must be submitted in site order (site0 = sites done so far). */

/* quality-score error sampler (rng.h:353-500) */
#define VGL_BETA_RAND48 0  /* rng.h:426-446, reference built with -D__USE_STD_BETA__=0, rng2   */
#define VGL_BETA_STD    1  /* rng.h:353-421, std::mt19937 + std::gamma_distribution (default
                              reference build; one global stream => VGL_RNG_SERIAL only)       */

/* Window layout of VGL_RNG_TILE.  Evaluation e = H(site_abs) * n_samples + sample owns draws
 * [e*block, (e+1)*block) of the rand48 sequence; stream k of that evaluation starts at
 * e*block + off[k].  A consumer that needs more draws than its sub-window simply keeps
 * stepping the generator (deterministic, only statistically overlapping).
 * H is a fixed permutation of the site indices [0, 2^W), 2^W = vgl_rng_tile_max_sites() (ABI version 4; H(0) = 0):
 *     sh = (W + 1) / 2;  x ^= x >> sh;  x = x * 0xBF58476D1CE4E5B9 mod 2^W;  x ^= x >> sh;
 *                        x = x * 0x94D049BB133111EB mod 2^W;  x ^= x >> sh            (identity for W <= 1)
 * (vgl_rng_tile_site_hash() evaluates it).  It breaks the regular spacing of the sites' windows: rand48 is a linear
 * congruential generator mod 2^48, and at offsets that are multiples of a high power of two its states are linearly
 * related (sites s, s + 2^k, s + 2^(k+1) at equal spacing would give u(s) - 2 u(s + 2^k) + u(s + 2^(k+1)) = const for
 * large k).  Results still depend only on (seed, absolute site index, sample): tiling and sharding never change a value.
 *   k=0 depth        rng1, Poisson draws                  (vcfgl.cpp:364-368, rng.h:284-351)
 *   k=1 haplotype    rng1, one draw per read              (vcfgl.cpp:473)
 *   k=2 base/strand  rng0, error test, wrong base, strand (vcfgl.cpp:486-488,582)
 *   k=3 qscore       rng2, beta deviates                  (vcfgl.cpp:428,495; rng.h:433-444)
 * Stream 3 is further divided per read: the beta deviate of read r starts at
 * e*block + off[3] + r*qs_read_stride, so the quality scores of one wavefront's reads are
 * independent work items that the device balances across lanes.  With --error-qs 1 the single
 * per-site beta deviate uses stream 3 of sample 0, read 0.
 * I16 tail distances (-addI16; vcfgl.cpp:647-663): the reference draws one per read from libc rand(), never seeded -- one serial
 * stream, which VGL_RNG_SERIAL follows.  VGL_RNG_TILE takes them from a SECOND rand48 sequence, X0 = 0x7A11D157A11D (no --seed
 * produces that state), addressed like the first: evaluation e owns draws [e*block, (e+1)*block) of it and read r uses draw r
 * as a 31-bit integer x (the state's top 31 bits, as lrand48()): tail = min(1 + x / (RAND_MAX / 50 + 1), 25)  (rng.h:12,
 * CAP_TAIL_DIST), credited -- as in the reference -- to the base of the site's last simulated read, float32 sums in (sample,
 * read) order.  (ABI 6, round 6: until then fields 13-16 of INFO/I16 were 0 in VGL_RNG_TILE.) */
typedef struct vgl_rng_layout {
    uint64_t block;
    uint64_t off[4];
    uint64_t qs_read_stride;
} vgl_rng_layout;

/* ---- layout of the per-(site, sample) FORMAT arrays with several values per sample (GL, PL, GP, AD, ADF, ADR, pl_u8) -- ABI 4
 * VGL_LAYOUT_PLANES (default): x[(site * K + k) * n_samples + sample], K = G or A of the context; entries k >= the site's own
 *   count hold the missing value.  Best for consumers on the device (one contiguous plane per genotype).
 * VGL_LAYOUT_SAMPLE_MAJOR: the slab of site i starts at x + i * K * n_samples (same allocation) and holds the record's array
 *   exactly as simRecord keeps it for bcf_update_format_*() (bcf_utils.h:193-196: gl_arr[sample * nGenotypes + g], nGenotypes
 *   variable per record): x[i * K * n_samples + sample * nK(i) + k], nK(i) = nGenotypes(site i) (GL, PL, GP, pl_u8) or
 *   n_alleles[i] (AD, ADF, ADR); what lies behind the record's array in a slab is unspecified (the kernels do not write it).  A record loop hands slab pointers to add_tags()
 *   unchanged: no per-record transposition on the host.  Skipped sites (site_status < 0) write nothing. */
#define VGL_LAYOUT_PLANES        0
#define VGL_LAYOUT_SAMPLE_MAJOR  1

/* ---- parameters = the subset of argStruct (io.h:40-148) the hot path reads ----------- */
typedef struct vgl_params {
    int32_t  abi_version;        /* VGL_ABI_VERSION */
    int32_t  seed;               /* --seed                                   io.cpp:1047-1061 */
    int32_t  n_samples;          /* bcf_hdr_nsamples                                         */
    int32_t  rng_mode;           /* VGL_RNG_*                                                */
    int32_t  beta_sampler;       /* VGL_BETA_*                                               */

    double   depth;              /* --depth (mean)   ; ignored if depths != NULL             */
    const double* depths;        /* --depths-file    ; [n_samples] per-sample means or NULL  */
    double   error_rate;         /* --error-rate                                             */
    int32_t  error_qs;           /* --error-qs 0|1|2                         io.h / README   */
    double   beta_variance;      /* --beta-variance (error_qs != 0)                          */
    int32_t  gl_model;           /* --gl-model 1|2                                           */
    double   gl1_theta;          /* --gl1-theta (default 0.83)               io.cpp:455      */
    int32_t  precise_gl;         /* --precise-gl 0|1 (usePreciseGlError)                     */
    int32_t  adjust_qs;          /* --adjust-qs bitmask                      shared.h:103-117 */
    double   adjust_by;          /* --adjust-by (default 0.499)                              */
    int32_t  n_qs_bins;          /* --qs-bins: number of [start,end,value] triples           */
    const int32_t* qs_bins;      /* [n_qs_bins][3]                           vcfgl.cpp:57-64 */
    int32_t  i16_mapq;           /* --i16-mapq (default 20)                                  */

    int32_t  do_unobserved;      /* -doUnobserved 0..5                       shared.h:70-89  */
    int32_t  rm_invar_sites;     /* --rm-invar-sites bitmask (only bit 4 acts here)          */
    int32_t  rm_empty_sites;     /* --rm-empty-sites                                         */
    int32_t  do_gvcf;            /* -doGVCF (only affects the no-reads site, vcfgl.cpp:242)  */

    int32_t  add_gl, add_gp, add_pl, add_i16, add_qs;              /* -addGL ... -addQS      */
    int32_t  add_fmt_dp, add_info_dp;                              /* -addFormatDP/-addInfoDP */
    int32_t  add_fmt_ad, add_info_ad;
    int32_t  add_fmt_adf, add_info_adf;
    int32_t  add_fmt_adr, add_info_adr;

    vgl_rng_layout layout;       /* VGL_RNG_TILE window layout; block==0 => library default  */
    int32_t  out_layout;         /* VGL_LAYOUT_* of the multi-valued FORMAT arrays (ABI 4)   */
} vgl_params;

/* ---- one tile of outputs = the simRecord arrays add_tags() reads (bcf_utils.h:157-211) -
 * Any pointer may be NULL (that output is not produced / not copied back), except
 * site_status, n_alleles and alleles2acgt which are always written.
 * G = vgl_max_genotypes(params) (10 or 15), A = vgl_max_alleles(params) (4 or 5).        */
typedef struct vgl_tile_out {
    /* per site */
    int32_t* site_status;    /* [n_sites]      VGL_SITE_*                                      */
    int32_t* n_alleles;      /* [n_sites]      sim->nAlleles (incl. <*> / <NON_REF>)           */
    int32_t* n_alleles_obs;  /* [n_sites]      sim->nAllelesObserved                           */
    int8_t*  alleles2acgt;   /* [n_sites][5]   sim->alleles2acgt; 4 = unobserved allele, -1 = none */
    int32_t* info_dp;        /* [n_sites]      INFO/DP                                         */
    int32_t* info_ad;        /* [n_sites][A]   INFO/AD  (allele order)                         */
    int32_t* info_adf;       /* [n_sites][A]                                                   */
    int32_t* info_adr;       /* [n_sites][A]                                                   */
    float*   qs;             /* [n_sites][A]   INFO/QS                                         */
    float*   i16;            /* [n_sites][16]  INFO/I16; fields 12-15 (tail distance): the reference's own
                                               libc rand() draws in VGL_RNG_SERIAL, a counter-addressed rand48
                                               sequence in VGL_RNG_TILE (see vgl_rng_layout)                */
    /* per (site, sample) */
    int32_t* fmt_dp;         /* [n_sites][n_samples]          FORMAT/DP                        */
    float*   gl;             /* [n_sites][G][n_samples]       FORMAT/GL, VCF genotype order;
                                entries g >= nGenotypes(site) hold VGL_FLOAT_MISSING_BITS       */
    int32_t* pl;             /* [n_sites][G][n_samples]       FORMAT/PL                        */
    float*   gp;             /* [n_sites][G][n_samples]       FORMAT/GP                        */
    int32_t* fmt_ad;         /* [n_sites][A][n_samples]       FORMAT/AD (allele order)         */
    int32_t* fmt_adf;        /* [n_sites][A][n_samples]                                        */
    int32_t* fmt_adr;        /* [n_sites][A][n_samples]                                        */
    /* optional per-read staging dump (reference: -printPileup, vcfgl.cpp:616-634)            */
    uint8_t* reads;          /* [read_capacity][n_sites][n_samples]  (qs << 2) | base           */
    int32_t  read_capacity;  /* rows available in `reads` / `read_errp` (0 = not requested)    */
    /* optional dumps behind -printQsError / -printGlError / -printQScores / -printBasePickError and
     * --adjust-qs 4|8|16 (vcfgl.cpp:430-435, 533-554): the deviates themselves, from which the caller derives
     * qScore and adjusted qScore exactly as vcfgl.cpp:500-523 does.  (ABI version 2.)                    */
    double*  read_errp;      /* [read_capacity][n_sites][n_samples]  error_prob_forQs_i of every read
                                (error_qs 2 only; rows >= the library's staging capacity hold NaN)         */
    double*  site_pick_err;  /* [n_sites]  base_pick_error_prob of the site (error_qs 1 only; written for
                                sites that reach the read loop, i.e. INFO/DP > 0)                          */
    /* ABI 4: FORMAT/PL in one byte per value (PL is capped at 255, shared.h:208; htslib narrows the int32 array the
     * reference hands it when it writes the record, vcfgl.cpp:907-939): a quarter of `pl`'s bytes over HBM and PCIe.
     * Same layout as `pl` (G planes, or sample-major); a missing PL (sample without reads, g >= nGenotypes(site)) is 255
     * here -- tell it from a capped value by fmt_dp == 0 / n_alleles.  Independent of `pl`: either, both or neither. */
    uint8_t* pl_u8;          /* [n_sites][G][n_samples]                                        */
} vgl_tile_out;

typedef struct vgl_ctx vgl_ctx;

/* Layout helpers (pure host arithmetic, usable without a GPU). */
VGL_API int32_t vgl_max_alleles(const vgl_params* p);      /* 4 or 5:  shared.h:148-152              */
VGL_API int32_t vgl_max_genotypes(const vgl_params* p);    /* 10 or 15: lut_nAlleles_to_nGenotypes    */
VGL_API int     vgl_default_rng_layout(const vgl_params* p, vgl_rng_layout* out);
/* VGL_RNG_TILE addresses one rand48 sequence of period 2^48: a job may use sites [0, *max_sites) before its windows
 * would repeat; *max_sites = 2^W, the largest power of two with 2^W * n_samples * block <= 2^48 (BASELINE config C4, 1e7
 * sites x 2000 samples at depth 30: 2^24 = 1.68e7).  vgl_simulate_tile* return VGL_E_ARG beyond that.  The reference's
 * serial streams have no such limit (rng.h:8-10) -- VGL_RNG_SERIAL neither. */
VGL_API int     vgl_rng_tile_max_sites(const vgl_params* p, int64_t* max_sites);
/* H(site) of the window layout above (pure host arithmetic; VGL_E_ARG outside [0, max_sites)). */
VGL_API int     vgl_rng_tile_site_hash(const vgl_params* p, int64_t site, int64_t* hashed);
VGL_API int     vgl_abi_version(void);
VGL_API const char* vgl_last_error(void);

/* Replaces args_get()'s sampler/LUT construction (io.cpp:1036-1074,1276) and main()'s
 * preCalc block (vcfgl.cpp:1661-1767): validates flags, builds the Poisson constants,
 * beta shape parameters, fixed-qscore terms, GL1 error-model tables and rand48 jump
 * tables, uploads them, and sizes the staging workspace for `max_sites_per_tile`.
 * `device` is the HIP device ordinal.  Fails with VGL_E_NODEVICE when no GPU is present. */
VGL_API int vgl_ctx_create(const vgl_params* p, int32_t device, int32_t max_sites_per_tile, vgl_ctx** out);
VGL_API int vgl_ctx_destroy(vgl_ctx* ctx);

/* Replaces the call of simulate_record_values() (vcfgl.cpp:1522,1552,1611) for `n_sites`
 * consecutive records whose absolute indices (in simulation order) start at `site0`.
 *   gt : [n_sites][n_samples] one byte per sample, (allele1 << 4) | allele0, alleles in ACGT
 *        space 0..3 exactly as check_rec_alleles() leaves them in true_gts_acgt_int
 *        (vcfgl.cpp:132-147); VGL_GT_MISSING (0xF) in either nibble = missing genotype.
 * Host variant: `gt` and every pointer in `out` are host memory; the call is synchronous. */
VGL_API int vgl_simulate_tile(vgl_ctx* ctx, int64_t site0, int32_t n_sites,
                      const uint8_t* gt, vgl_tile_out* out);

/* Asynchronous host variant (the tags of a tile are 65 B per evaluation and must stream over PCIe while the next
 * tile is computed).  vgl_simulate_tile_async() enqueues the tile -- its kernels on the context's compute stream, the copies of
 * its outputs into the caller's host buffers on a second stream behind them -- and returns a ticket; vgl_tile_wait(ticket)
 * returns once the outputs are complete (and reports the tile's device-side errors, like the synchronous call).  At most two
 * tiles may be in flight per context, submitted in site order; the buffers of an in-flight tile must not be touched.
 * Buffers obtained from vgl_host_alloc() are page-locked and are written by DMA at the link's rate; ordinary (pageable)
 * buffers work too, more slowly.  vgl_simulate_tile() is the two calls back to back. */
VGL_API int   vgl_simulate_tile_async(vgl_ctx* ctx, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* out, int32_t* ticket);
VGL_API int   vgl_tile_wait(vgl_ctx* ctx, int32_t ticket);
VGL_API void* vgl_host_alloc(size_t bytes);            /* page-locked host memory (NULL on failure); needs a HIP device */
/* the same, placed for DMA from `device` (on a two-socket host page-locked memory lands on the NUMA node next to the device
 * that is current when it is allocated: 53 against 35 GB/s of copy-back measured): buffers of a multi-device record loop (ABI 4) */
VGL_API void* vgl_host_alloc_on(int32_t device, size_t bytes);
VGL_API void  vgl_host_free(void* p);

/* Device variant: `gt` and every pointer in `out` are device memory owned by the caller
 * (hipMalloc / a torch tensor's data_ptr); work is enqueued on `hip_stream` (a hipStream_t
 * cast to void*, NULL = default stream) and the call returns without synchronising.  A context owns
 * one staging workspace: tiles of one context must be enqueued on one stream (or otherwise ordered);
 * use one context per stream / per GPU for concurrent tiles.
 * (VGL_RNG_SERIAL with error_qs 2 and VGL_BETA_STD synchronises the stream inside the call: the number of
 * reads of the tile and the progress of the beta chain come back to the host.) */
VGL_API int vgl_simulate_tile_device(vgl_ctx* ctx, int64_t site0, int32_t n_sites,
                             const uint8_t* gt, vgl_tile_out* out, void* hip_stream);

/* Sticky device-side error flags of the last tiles (capacity overflow, qs-bin miss):
 * synchronises the stream, returns VGL_OK or the first VGL_E_* raised, and clears them. */
VGL_API int vgl_ctx_check(vgl_ctx* ctx, void* hip_stream);

/* Kernel timing hook for bench.py: brackets the device work of every following
 * vgl_simulate_tile_device call with hipEvents on its stream.  vgl_ctx_kernel_ms returns
 * accumulated milliseconds and launch counts since the last reset, one entry per bucket (ABI 5: six buckets,
 * the caller passes the length of its arrays; entries beyond VGL_N_TIMING_BUCKETS are zeroed):
 *   [VGL_T_DEPTH]   what runs ahead of the sampling kernel: k_sitebase + k_depth (the stream scouts in VGL_RNG_SERIAL)
 *   [VGL_T_SAMPLE]  k_sample
 *   [VGL_T_REDO]    k_redo (the reads the deferred build of k_sample<2> leaves to a double-precision second look)
 *   [VGL_T_SITE]    k_site
 *   [VGL_T_GL]      k_gl (the fused kernel, when it runs, is all of the tile and is counted here)
 *   [VGL_T_SITEAGG] what runs behind k_gl: k_siteagg (INFO/QS, INFO/I16) and the device copies of the per-read dumps
 * (ABI 3 had four buckets and left k_siteagg untimed; k_redo was part of k_sample's.) */
#define VGL_N_TIMING_BUCKETS 6
#define VGL_T_DEPTH   0
#define VGL_T_SAMPLE  1
#define VGL_T_REDO    2
#define VGL_T_SITE    3
#define VGL_T_GL      4
#define VGL_T_SITEAGG 5
VGL_API int vgl_ctx_timing(vgl_ctx* ctx, int32_t enable);
VGL_API int vgl_ctx_kernel_ms(vgl_ctx* ctx, double* ms, int64_t* launches, int32_t n_buckets, int32_t reset);

/* ---- what a context will launch (ABI 5) ------------------------------------------------------------------------------
 * The library picks one of several builds of its kernels from the flags (vgl_ctx_create); a record loop sizes its tiles
 * and a test asserts "the fused kernel runs here" from this record instead of inferring either from timings.
 * `size` is set by the caller to sizeof(vgl_ctx_info_t) (fields beyond it are not written; new fields are appended). */
#define VGL_DEPTH_INPLACE_MIXED   0  /* mixed per-sample means: rng.h:284-351's general sampler inside k_sample          */
#define VGL_DEPTH_KDEPTH          1  /* every mean >= 12: k_depth (rejection method, rng.h:300-312) ahead of k_sample    */
#define VGL_DEPTH_INPLACE_PRODUCT 2  /* every mean < 12: the product method's loop (rng.h:289-299) inside k_sample        */
#define VGL_DEPTH_SERIAL_SCOUT    3  /* VGL_RNG_SERIAL: the scout kernels walk the reference's stream                     */
typedef struct vgl_ctx_info_t {
    int32_t size;                /* in: sizeof(vgl_ctx_info_t) of the caller                                              */
    int32_t abi_version;
    int32_t device;
    int32_t n_samples, max_sites_per_tile;
    int32_t max_alleles, max_genotypes;
    int32_t rng_mode;            /* VGL_RNG_*                                                                             */
    int32_t depth_mode;          /* VGL_DEPTH_*                                                                           */
    int32_t fused;               /* 1: a tile that asks for no QS / I16 / per-read dump runs as ONE kernel (k_gl<.., FUSED>) */
    int32_t fused_split;         /* workgroups per site of that kernel (1, or several with the site sums exchanged in HBM)   */
    int32_t sample_lean;         /* build of k_sample a tile without per-read dump gets: 0 every option's state carried, double-precision
                                    fallbacks inline; 1 default tag surface; 2 = 1 with the fallbacks deferred to k_redo; 3 = 0 with the
                                    fallbacks deferred (optional tags: -addQS / -addI16 / strand tags / --adjust-qs; a tile with the strand
                                    tags and the quality sums and no --adjust-qs gets that build with its options fixed, "LEAN 4").
                                    ABI 6: the float32 builds (2, 3) run as two kernels, k_sample_seg<., 1> + <., 2>, when a wavefront's reads
                                    fit one pool (see pool_cap)                                                                     */
    int32_t gl_sort;             /* k_gl re-deals a workgroup's evaluations in (distinct bases, depth) order                */
    int32_t gl_wpb;              /* natural wavefronts per k_gl workgroup (4 or 8); 16 = the context is ELIGIBLE for k_gl2 (two evaluations per thread):
                                    a tile that asks for GP or FORMAT/AD* still runs k_gl with 8 -- the choice is per tile (vgl_launch_gl)              */
    int32_t read_cap;            /* staged reads per (site, sample); a deeper draw: see VGL_E_CAPACITY                       */
    int32_t pool_cap;            /* quality-score work items per wavefront and LDS segment (--error-qs 2)                   */
    int32_t pool_lds_bytes;      /* LDS bytes per wavefront of k_sample<2>                                                  */
    int32_t test_hooks;          /* 1: this library was built with -DVGL_TEST_HOOKS (environment overrides, vgl_dbg_*)      */
    int64_t workspace_bytes;     /* device memory the context owns for max_sites_per_tile (tables + staging)                */
    int64_t rng_tile_max_sites;  /* VGL_RNG_TILE: sites [0, this) are addressable (vgl_rng_tile_max_sites); 0 in serial mode */
} vgl_ctx_info_t;
VGL_API int vgl_ctx_info(const vgl_ctx* ctx, vgl_ctx_info_t* out);

/* ---- record packing on the device (ABI 6) ---------------------------------------------------------------------------------
 * The reference writes one record at a time with bcf_write (vcfgl.cpp:167-206) from the arrays simRecord::add_tags() filled
 * (bcf_utils.cpp:426-507: of every FORMAT tag only the record's nGenotypes / nAlleles values per sample).  With the sites of a job
 * sharded over the GPUs of a node, each rank hands the writer its kept sites in that form -- skipped sites (site_status < 0) dropped,
 * nG(site) = nA (nA + 1) / 2 planes of GL / PL / GP and nA(site) planes of AD / ADF / ADR -- and these two calls are the producer side
 * of that gather: an exclusive prefix sum over the tile's sites, then coalesced row copies (every byte read once, written once).
 * Every pointer but `totals` is device memory of `device`; work is enqueued on `hip_stream`.
 *
 *   vgl_pack_plan_device     offsets: int32 [3][n_sites + 1] -- row c = exclusive prefix sums of the rows a site contributes to a field of
 *                            kind c (VGL_PACK_ROW: 1 per kept site; _ROWS_G: nG(site); _ROWS_A: nA(site)), entry [n_sites] = the total.
 *                            The three totals also come back to the host (the caller sizes the packed arrays from them): synchronises the stream.
 *   vgl_pack_records_device  index_out: int32 [n_kept][3] = (site index in the tile, site_status, n_alleles) of the kept sites (may be NULL);
 *                            field f: the rows of src -- [n_sites][planes] rows of row_bytes bytes -- that belong to records, in site order,
 *                            into dst (sized from the plan: total rows of its kind x row_bytes).  Asynchronous. */
#define VGL_PACK_ROW    0   /* one row per site: per-site vectors and FORMAT tags with one value per sample (planes = 1) */
#define VGL_PACK_ROWS_G 1   /* a [site][planes][N] array of which a record keeps its nGenotypes(site) first planes        */
#define VGL_PACK_ROWS_A 2   /* ... its nAlleles(site) first planes                                                       */
typedef struct vgl_pack_field {
    const void* src;
    void*       dst;
    int32_t     kind;        /* VGL_PACK_*                                   */
    int32_t     planes;      /* rows per site in src                         */
    int64_t     row_bytes;   /* bytes of one row (N x element size, or the per-site vector) */
} vgl_pack_field;
typedef struct vgl_pack_plan { int64_t n_kept, rows_g, rows_a; } vgl_pack_plan;
VGL_API int vgl_pack_plan_device(int32_t device, int32_t n_sites, const int32_t* site_status, const int32_t* n_alleles, int32_t* offsets,
                                 vgl_pack_plan* totals, void* hip_stream);
VGL_API int vgl_pack_records_device(int32_t device, int32_t n_sites, const int32_t* site_status, const int32_t* n_alleles, const int32_t* offsets,
                                    int32_t* index_out, const vgl_pack_field* fields, int32_t n_fields, void* hip_stream);

/* ---- BGZF compression on the device (ABI 7) ------------------------------------------------------------------------------
 * BGZF (SAMv1 section 4.1): independent gzip members of at most 64 KiB with their size in a 'BC' extra field -- what the reference
 * writes through htslib for -O b / -O z (vcfgl.cpp:1790-1803) and its pileup.  The input is cut into members of exactly 0xff00 bytes
 * (the last one shorter), the boundaries of the host program's zlib path, so the member count is ceil(n / 0xff00) and each member's
 * ISIZE is the same as there; the compressed bytes differ from zlib's, what they decompress to does not.  Each member is LZ77 +
 * Huffman coded by one workgroup and written as the smallest of a dynamic, a fixed and a stored deflate block (stored bounds every
 * member by 0xff00 + 31 bytes).  The output depends on the input bytes only: not on the device, and not on how a caller splits its
 * input at member boundaries (compressing a + b equals compressing a, then b, when a's length is a multiple of 0xff00).
 *   vgl_bgzf_bound(n)            largest output for n input bytes: n + 31 * ceil(n / 0xff00) (-1 for n < 0).  Pure host arithmetic.
 *   vgl_bgzf_workspace_bytes(n)  device workspace a call on n bytes needs (0 for n = 0, -1 for n < 0).  Pure host arithmetic.
 *   vgl_bgzf_compress_device     src [n], dst [dst_cap >= vgl_bgzf_bound(n)], out_n (int64, may be NULL) and the workspace are device
 *                                memory of `device`; work is enqueued on `hip_stream` and the call returns without synchronising.  dst
 *                                receives the members back to back WITHOUT the 28-byte end-of-file member (a file ends with it once:
 *                                1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00), *out_n their
 *                                length.  Calls on one workspace must be ordered (one stream).  n = 0 writes *out_n = 0 and nothing else. */
VGL_API int64_t vgl_bgzf_bound(int64_t n);
VGL_API int64_t vgl_bgzf_workspace_bytes(int64_t n);
VGL_API int vgl_bgzf_compress_device(int32_t device, const uint8_t* src, int64_t n, uint8_t* dst, int64_t dst_cap, int64_t* out_n,
                                     void* workspace, int64_t workspace_bytes, void* hip_stream);
/* Host batches, for a program that writes BGZF from host memory (the host program's --device-bgzf 1): a handle owns the device
 * buffers, workspace and streams for batches of up to max_batch bytes, two of which may be in flight.
 *   vgl_bgzf_host_submit  enqueues the copy of src [n <= max_batch] to the device and its compression; returns at once with a ticket.
 *                         src must stay unchanged until the ticket is waited for (page-locked memory from vgl_host_alloc_on copies
 *                         at the link's rate).  A third submit before a wait fails with VGL_E_ARG.
 *   vgl_bgzf_host_wait    blocks until the ticket's members are back in host memory: *out (owned by the handle, valid until the
 *                         ticket's slot is submitted again) holds *out_n bytes of members, without the EOF member.
 * Tickets are waited for in submit order to keep a file's members in order.  No HIP device: VGL_E_NODEVICE from create. */
typedef struct vgl_bgzf_host vgl_bgzf_host;
VGL_API int vgl_bgzf_host_create(int32_t device, int64_t max_batch, vgl_bgzf_host** out);
VGL_API int vgl_bgzf_host_submit(vgl_bgzf_host* h, const uint8_t* src, int64_t n, int32_t* ticket);
VGL_API int vgl_bgzf_host_wait(vgl_bgzf_host* h, int32_t ticket, const uint8_t** out, int64_t* out_n);
VGL_API int vgl_bgzf_host_destroy(vgl_bgzf_host* h);

/* ---- VCF text of the sample columns on the device (ABI 7, additive) --------------------------------------------------------
 * The N-wide part of a VCF text record -- what the host writer appends behind the eight fixed columns -- formatted from the tile's
 * FORMAT arrays where they are computed.  For every site i with site_status[i] >= 0 the text is
 *     "\t" KEYS ( "\t" sample_0 ) ... ( "\t" sample_{N-1} ) "\n"
 * KEYS = the fields' keys joined by ':' ("." without fields); a sample column = its fields joined by ':', a field's values by ','.
 * A skipped site (site_status < 0) has no text.  Numbers are written as the host program writes them (htslib's kputd): int32 %d with
 * VGL_INT32_MISSING as "."; float32 VGL_FLOAT_MISSING_BITS as ".", other NaN "nan", [1e-4, 999999] in kputd's 6-digit integer
 * form, everything else (infinity included) as glibc's %g, correctly rounded.  The bytes are identical to the host writer's.
 *   vgl_text_field            one FORMAT field: value k of sample s of site i at ((T*)base)[i * site_stride + s * n(i) + k] -- the
 *                             VGL_LAYOUT_SAMPLE_MAJOR slabs -- with n(i) = 1 (VGL_TEXT_ONE), nA (nA + 1) / 2 (VGL_TEXT_PER_G) or nA
 *                             (VGL_TEXT_PER_A), nA = n_alleles[i].  Fields are written in the order given.
 *   vgl_text_bound            largest text of n_sites sites with at most max_alleles alleles (pure host arithmetic; -1 on bad input).
 *   vgl_text_workspace_bytes  device workspace of a call (pure host arithmetic).
 *   vgl_text_format_device    site_status, n_alleles, the fields' values, dst [dst_cap], offsets (int64 [n_sites + 1]) and the workspace
 *                             are device memory of `device`; work is enqueued on `hip_stream` without synchronising.  offsets[i] = where
 *                             site i's text starts in dst, offsets[n_sites] = the total.  When the total exceeds dst_cap NOTHING is
 *                             written to dst; offsets still receives the sizes, so the caller reads offsets[n_sites] to learn what
 *                             the text needs.
 *   vgl_ctx_text_bound        vgl_text_bound of the fields vgl_simulate_tile_text_async formats for this context.
 *   vgl_simulate_tile_text_async
 *                             vgl_simulate_tile_async whose FORMAT tags come back as text (a context with out_layout =
 *                             VGL_LAYOUT_SAMPLE_MAJOR; VGL_E_ARG otherwise): the tags the context's add_* flags enable
 *                             (DP, GL, PL, GP, AD, ADF, ADR: add_tags()'s order) are formatted on the device and the tile's text is
 *                             copied to `text` [text_cap] (host memory; page-locked copies at the link's rate), its site offsets to
 *                             `offsets` (host, int64 [n_sites + 1]).  The per-site arrays of `out` are copied as by
 *                             vgl_simulate_tile_async; its per-sample FORMAT pointers may be NULL (those planes are then not copied back:
 *                             the text replaces them).  Completed by vgl_tile_wait: a tile that drew deeper than the staging capacity is
 *                             run again and formatted again; a text larger than text_cap gives VGL_E_CAPACITY, offsets[n_sites] = the
 *                             size it needs, and nothing is written to `text`.  Only the bytes the tile produced cross the link. */
#define VGL_TEXT_ONE        0
#define VGL_TEXT_PER_G      1
#define VGL_TEXT_PER_A      2
#define VGL_TEXT_MAX_FIELDS 8
typedef struct vgl_text_field {
    const char* key;          /* FORMAT key (host string)                          */
    int32_t     is_float;     /* 1: float32 values, 0: int32                       */
    int32_t     count;        /* VGL_TEXT_*                                        */
    const void* base;         /* device memory                                     */
    int64_t     site_stride;  /* elements from one site's slab to the next         */
} vgl_text_field;
VGL_API int64_t vgl_text_bound(int32_t n_samples, int32_t n_sites, const vgl_text_field* fields, int32_t n_fields, int32_t max_alleles);
VGL_API int64_t vgl_text_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_text_format_device(int32_t device, const vgl_text_field* fields, int32_t n_fields, int32_t n_samples, int32_t n_sites,
                                   const int32_t* site_status, const int32_t* n_alleles, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                   void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int64_t vgl_ctx_text_bound(const vgl_ctx* ctx, int32_t n_sites);
VGL_API int vgl_simulate_tile_text_async(vgl_ctx* ctx, int64_t site0, int32_t n_sites, const uint8_t* gt, vgl_tile_out* out,
                                         uint8_t* text, int64_t text_cap, int64_t* offsets, int32_t* ticket);

/* ---- gVCF blocks on the device (ABI 7, additive) ------------------------------------------------------------------------------
 * The block machine of the host writer (prepare_gvcf_block) over one tile, as rules on neighbouring kept sites (site_status >= 0;
 * skipped sites are passed over).  r(i) = the index of the first --gvcf-dps threshold above the site's smallest per-sample DP (the
 * number of thresholds when none is).  A kept site is BLOCKABLE when n_alleles_obs == 1 and r > 0; it CONTINUES the block of the
 * previous kept site when that site is blockable, on the same contig, pos0 <= its pos0 + 1, with the same r; a blockable site that
 * does not continue FOUNDS a block; any other kept site is a RECORD.  A block's aggregates: per sample the minimum DP and the
 * lexicographically smallest (PL[1], PL[2]) compared as signed int32; PL[0] (and, for the caller, alleles and QS) of the founder;
 * MIN_DP = the smallest DP of all members.  A site that joins a block while it or the founder has n_alleles != 2 is the host's fatal
 * "Unexpected number of PL values": the first such site is reported.  A one-site block whose founder has n_alleles != 2 keeps the
 * founder's nG PL values per sample.
 *   vgl_gvcf_item             one item of the tile's ordered output: a record (first = last = founder = the site, block = -1) or a
 *                             block (first / last member, founder = first, dpr = r, min_dp = MIN_DP, block = index of its aggregates)
 *   vgl_gvcf_workspace_bytes  device workspace of a call (pure host arithmetic).
 *   vgl_gvcf_blocks_device    `in` and `out` arrays and the workspace are device memory of `device`; work is enqueued on `hip_stream`
 *                             without synchronising.  dp[i * dp_site_stride + s], pl[i * pl_site_stride + s * nG(i) + g]: the
 *                             VGL_LAYOUT_SAMPLE_MAJOR slabs (pl_site_stride >= n_samples * nG of every founder).  Out: items[0 ..
 *                             n_items), counts = {n_items, n_blocks, first error site or -1, 0}; block b's DP slab at block_dp[b *
 *                             n_samples], its PL slab at block_pl[b * pl_site_stride] (founder's nG values per sample), its founder's
 *                             n_alleles in block_n_alleles[b]; block_status[b] = 0 for b < n_blocks, -1 up to n_sites;
 *                             record_status[i] = site_status[i] for records, -1 for block members and skipped sites.  With the
 *                             fields {"PL", VGL_TEXT_PER_G, block_pl, pl_site_stride}, {"DP", VGL_TEXT_ONE, block_dp, n_samples},
 *                             block_status and block_n_alleles, vgl_text_format_device writes each block's sample columns
 *                             ("\tPL:DP" ("\t" PL ":" DP)* "\n"); with record_status, the records' columns.
 *   vgl_ctx_gvcf_text_bound   the text_cap that always suffices for vgl_simulate_tile_gvcf_async on n_sites sites (host arithmetic).
 *   vgl_simulate_tile_gvcf_async
 *                             vgl_simulate_tile_async of a -doGVCF 1 record loop (a context with out_layout = VGL_LAYOUT_SAMPLE_MAJOR,
 *                             add_fmt_dp and add_pl; VGL_E_ARG otherwise): contig (int32) and pos0 (int64) per site and the thresholds
 *                             dps[n_dps] are host arrays; the tile is blocked and its record and block columns formatted on the device.
 *                             The per-site arrays of `out` are copied as by vgl_simulate_tile_async (its per-sample FORMAT pointers
 *                             may be NULL: PL and GL then stay on the device).  vgl_tile_wait completes it, filling `g`: n_items,
 *                             n_blocks, error_site (tile index or -1), items [n_items]; record site i's text at text[record_offsets[i]
 *                             .. record_offsets[i + 1]) (empty for members and skipped sites), block b's at text[block_offsets[b] ..
 *                             block_offsets[b + 1]) (behind the record text, block_offsets[0] = record_offsets[n_sites]); first_dp [N],
 *                             first_pl [n_samples * max genotypes] and last_dp / last_pl: the aggregates of block 0 and block
 *                             n_blocks - 1 (to stitch blocks across tiles).  A tile that drew deeper than the staging capacity is run,
 *                             blocked and formatted again; a text larger than text_cap gives VGL_E_CAPACITY and text_needed = its
 *                             size, nothing is written to `text`.  `g` and its arrays must live until vgl_tile_wait returns. */
#define VGL_GVCF_RECORD 0
#define VGL_GVCF_BLOCK  1
typedef struct vgl_gvcf_item {
    int32_t kind;             /* VGL_GVCF_RECORD / VGL_GVCF_BLOCK                */
    int32_t first, last;      /* tile indices of the first and last member       */
    int32_t founder;          /* tile index of the founding site (= first)       */
    int32_t dpr;              /* the block's r (0 for a record)                  */
    int32_t min_dp;           /* MIN_DP (a record: its smallest per-sample DP)   */
    int32_t block;            /* index of the block's aggregates, -1: a record   */
    int32_t reserved;
} vgl_gvcf_item;
typedef struct vgl_gvcf_in {
    const int32_t* site_status;
    const int32_t* n_alleles_obs;
    const int32_t* n_alleles;
    const int32_t* contig;        /* any int32 id, equal for sites of one contig    */
    const int64_t* pos0;
    const int32_t* dp;   int64_t dp_site_stride;
    const int32_t* pl;   int64_t pl_site_stride;
    const int32_t* dps;  int32_t n_dps;   /* the --gvcf-dps thresholds (device memory) */
    int32_t reserved;
} vgl_gvcf_in;
typedef struct vgl_gvcf_out {
    vgl_gvcf_item* items;         /* [n_sites]                                        */
    int32_t* counts;              /* [4]                                              */
    int32_t* block_dp;            /* [n_sites * n_samples]                            */
    int32_t* block_pl;            /* [n_sites * pl_site_stride]                       */
    int32_t* block_n_alleles;     /* [n_sites]                                        */
    int32_t* block_status;        /* [n_sites]                                        */
    int32_t* record_status;       /* [n_sites]                                        */
} vgl_gvcf_out;
typedef struct vgl_gvcf_tile {     /* host memory */
    vgl_gvcf_item* items;         /* [n_sites]                                        */
    uint8_t* text; int64_t text_cap;
    int64_t* record_offsets;      /* [n_sites + 1]                                    */
    int64_t* block_offsets;       /* [n_sites + 1]                                    */
    int32_t* first_dp; int32_t* first_pl; int32_t* last_dp; int32_t* last_pl;
    int32_t n_items, n_blocks, error_site, reserved;    /* written by vgl_tile_wait   */
    int64_t text_needed;                                /* written by vgl_tile_wait   */
} vgl_gvcf_tile;
VGL_API int64_t vgl_gvcf_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_gvcf_blocks_device(int32_t device, int32_t n_samples, int32_t n_sites, const vgl_gvcf_in* in, const vgl_gvcf_out* out,
                                   void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int64_t vgl_ctx_gvcf_text_bound(const vgl_ctx* ctx, int32_t n_sites);
VGL_API int vgl_simulate_tile_gvcf_async(vgl_ctx* ctx, int64_t site0, int32_t n_sites, const uint8_t* gt, const int32_t* contig,
                                         const int64_t* pos0, const int32_t* dps, int32_t n_dps, vgl_tile_out* out, vgl_gvcf_tile* g,
                                         int32_t* ticket);

/* ---- pileup lines on the device (ABI 7, additive) -----------------------------------------------------------------------------
 * The N-wide part of a -printPileup 1 line -- what the host writer appends behind the prefix chrom "\t" pos "\t" ref -- formatted from
 * the tile's DP plane and read dump where they are computed.  For every site i with site_status[i] != VGL_SITE_SKIP_EMPTY the text is
 *     ( "\t" COL(i, s) ) for s = 0 .. N-1, then "\n"
 *     COL = "0\t*\t*" when dp(i, s) == 0, else dp "\t" B_0 .. B_{dp-1} "\t" Q_0 .. Q_{dp-1}
 *     B_r = "ACGT"[reads[r][i][s] & 3]; Q_r = (reads[r][i][s] >> 2) + 33, or qual_char for every read when qual_char >= 0
 * An empty site (VGL_SITE_SKIP_EMPTY) has no text; every other status has its line (VGL_SITE_SKIP_INVAR and VGL_SITE_NO_READS included).
 *   vgl_pileup_bound          largest text of n_sites sites whose depths are at most read_capacity (pure host arithmetic; -1 on bad
 *                             input): n_sites (1 + n_samples max(6, 3 + digits(read_capacity) + 2 read_capacity)).
 *   vgl_pileup_workspace_bytes  device workspace of a call (pure host arithmetic).
 *   vgl_pileup_format_device  site_status (int32 [n_sites]), fmt_dp (int32 [n_sites][n_samples]), reads (uint8 [read_capacity][n_sites]
 *                             [n_samples], vgl_tile_out.reads' layout), dst [dst_cap], offsets (int64 [n_sites + 1]) and the workspace are
 *                             device memory of `device`; work is enqueued on `hip_stream` without synchronising.  No dump row at or
 *                             beyond read_capacity is read.  offsets[i] = where site i's text starts in dst, offsets[n_sites] = the
 *                             total.  When the total exceeds dst_cap NOTHING is written to dst and offsets[n_sites] is the size the text
 *                             needs.  A dp below 0 or above read_capacity is an error reported through the same word: NOTHING is
 *                             written and offsets[n_sites] = -1 (the call itself returns VGL_OK: it does not synchronise).
 *   vgl_ctx_pileup_bound      vgl_pileup_bound at the context's staging capacity (vgl_ctx_info_t.read_cap): the text_cap that always
 *                             suffices for a tile of n_sites sites of this context.
 *   vgl_ctx_pileup_next       asks for the pileup of the NEXT tile submitted on ctx by vgl_simulate_tile_async, _text_async or
 *                             _gvcf_async (NULL withdraws a pending request; the next tile call consumes it, whether it succeeds or
 *                             not).  That tile's read dump and DP plane feed the formatter on the device: they cross the link only if
 *                             `out` also asks for them (reads / read_capacity, fmt_dp).  --adjust-qs 4 (adjust_qs & 4) is applied from
 *                             the context's parameters: with error_qs 0 / 1 every read gets the adjusted score of error_rate, with
 *                             error_qs 2 each read the adjusted score of its staged error probability (the sampler's rule: double
 *                             log10, adjust_by, the bins or the cap of 63; an error probability of exactly 0 or 1 has no adjusted score
 *                             and gives the byte 32, as the host writer's).  vgl_tile_wait copies the text into p->text (host memory)
 *                             and the site offsets into p->offsets (host, int64 [n_sites + 1]), sets p->text_needed, and copies only the
 *                             bytes produced.  A text larger than text_cap gives VGL_E_CAPACITY (text_needed = its size, nothing is
 *                             written to text).  A tile that drew deeper than the staging capacity is not run again when it carries a
 *                             pileup: VGL_E_CAPACITY, as for a per-read dump.  `p` and its arrays must live until vgl_tile_wait returns. */
typedef struct vgl_pileup_tile {   /* host memory */
    uint8_t* text; int64_t text_cap;
    int64_t* offsets;             /* [n_sites + 1]                                    */
    int64_t text_needed;          /* written by vgl_tile_wait                         */
} vgl_pileup_tile;
VGL_API int64_t vgl_pileup_bound(int32_t n_samples, int32_t n_sites, int32_t read_capacity);
VGL_API int64_t vgl_pileup_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_pileup_format_device(int32_t device, int32_t n_samples, int32_t n_sites, const int32_t* site_status, const int32_t* fmt_dp,
                                     const uint8_t* reads, int32_t read_capacity, int32_t qual_char, uint8_t* dst, int64_t dst_cap,
                                     int64_t* offsets, void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int64_t vgl_ctx_pileup_bound(const vgl_ctx* ctx, int32_t n_sites);
VGL_API int vgl_ctx_pileup_next(vgl_ctx* ctx, vgl_pileup_tile* p);

/* ---- the FORMAT part of BCF records on the device (ABI 7, additive) -------------------------------------------------------------
 * The N-wide part of a BCF record -- the `indiv` block the host writer (BCF 2.2 section 6.3.3) puts behind the shared block -- encoded
 * from the tile's FORMAT arrays where they are computed.  For every site i with site_status[i] >= 0 and every field, in the order given:
 *     the typed key           0x11 id (id <= 127), 0x12 id16 (<= 32767), 0x13 id32
 *     the size/type byte      (n << 4 | bt) for n < 15; (0xF0 | bt) followed by the typed integer n for n >= 15; bt alone for n = 0
 *     n(i) * n_samples values int32 fields in the narrowest of int8 (max <= 127, min >= -120), int16 (max <= 32767, min >= -32760) and
 *                             int32 that holds the record's range -- VGL_INT32_MISSING and the vector end INT32_MIN + 1 are left out of
 *                             the range and become 0x80 / 0x8000 and 0x81 / 0x8001; a vector without an ordinary value is int8 --
 *                             float32 fields as their bit patterns, untouched; little endian
 * A skipped site (site_status < 0) has no bytes.  The bytes are identical to the host writer's (htslib's choices).
 *   vgl_bcf_field             one FORMAT field: value k of sample s of site i at ((T*)base)[i * site_stride + s * n(i) + k] -- the
 *                             VGL_LAYOUT_SAMPLE_MAJOR slabs -- with n(i) by `count`, as in vgl_text_field: VGL_TEXT_ONE / _PER_G / _PER_A;
 *                             key_id = the key's index in the output header's string dictionary.
 *   vgl_bcf_bound             largest encoding of n_sites sites with at most max_alleles alleles (pure host arithmetic; -1 on bad input).
 *   vgl_bcf_workspace_bytes   device workspace of a call (pure host arithmetic; -1 on bad input).
 *   vgl_bcf_encode_device     the contract of vgl_text_format_device: every pointer is device memory of `device`, work is enqueued on
 *                             `hip_stream` without synchronising; offsets[i] = where site i's bytes start in dst, offsets[n_sites] = the
 *                             total.  When the total exceeds dst_cap NOTHING is written to dst and offsets[n_sites] says what is needed.
 *   vgl_ctx_bcf_keys          key_ids[7] = the output header's dictionary ids of DP, GL, PL, GP, AD, ADF, ADR (entries of tags the
 *                             context does not write are ignored; n must be 7).  From then on vgl_simulate_tile_text_async and
 *                             vgl_simulate_tile_gvcf_async of this context deliver the sample data as these typed vectors instead of
 *                             text, in the same buffers and through the same offsets arrays (gVCF blocks: the fields PL then DP), and
 *                             vgl_ctx_text_bound / vgl_ctx_gvcf_text_bound bound this encoding.  NULL switches back to text.  Call it
 *                             while no tile of the context is in flight. */
typedef struct vgl_bcf_field {
    int32_t     key_id;       /* index of the FORMAT key in the header's dictionary */
    int32_t     is_float;     /* 1: float32 values, 0: int32                       */
    int32_t     count;        /* VGL_TEXT_*                                        */
    const void* base;         /* device memory                                     */
    int64_t     site_stride;  /* elements from one site's slab to the next         */
} vgl_bcf_field;
VGL_API int64_t vgl_bcf_bound(int32_t n_samples, int32_t n_sites, const vgl_bcf_field* fields, int32_t n_fields, int32_t max_alleles);
VGL_API int64_t vgl_bcf_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_bcf_encode_device(int32_t device, const vgl_bcf_field* fields, int32_t n_fields, int32_t n_samples, int32_t n_sites,
                                  const int32_t* site_status, const int32_t* n_alleles, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                  void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int vgl_ctx_bcf_keys(vgl_ctx* ctx, const int32_t* key_ids, int32_t n);

/* ---- a tile's record stream assembled and compressed on the device (ABI 7, additive) -------------------------------------------------
 * A record of the output is a HEAD the host builds from the tile's per-site arrays (the eight fixed columns of a VCF line; l_shared,
 * l_indiv and the shared block of a BCF record) followed by the BODY the device built (vgl_simulate_tile_text_async: the sample columns,
 * or the indiv block after vgl_ctx_bcf_keys).  These calls keep the bodies on the device, take the heads up the link, interleave the
 * two there and compress the stream with vgl_bgzf_compress_device: only heads go up, only BGZF members come down.
 *   vgl_stream_assemble_device  heads, head_offsets (int64 [n_sites + 1]), bodies, body_offsets (int64 [n_sites + 1]), dst [dst_cap] and
 *                             total (int64) are device memory of `device`; work is enqueued on `hip_stream` without synchronising.
 *                             Both offset arrays are non-decreasing prefix sums that may start at any value: `heads` and `bodies`
 *                             point at the first byte of site 0, so head i is heads[head_offsets[i] - head_offsets[0] ..
 *                             head_offsets[i + 1] - head_offsets[0]), body i likewise.  Record i = head i then body i, written at
 *                             dst + (head_offsets[i] - head_offsets[0]) + (body_offsets[i] - body_offsets[0]); a site whose head and
 *                             body are empty contributes nothing.  *total = the stream's length.  When it exceeds dst_cap NOTHING is
 *                             written to dst and *total still says what is needed.  heads, bodies and dst may start at any byte; all
 *                             offsets and counts are 64-bit (a tile's text can exceed 2 GiB).  n_sites = 0 writes *total = 0 only.
 *   vgl_ctx_text_device       on != 0: from then on the `text` argument of vgl_simulate_tile_text_async is memory of the context's
 *                             DEVICE: the formatter (or the BCF encoder) writes the tile's bodies there and vgl_tile_wait copies no
 *                             text; `offsets` stays host memory and receives the site offsets as before (offsets[n_sites] = the total;
 *                             beyond text_cap: VGL_E_CAPACITY and nothing written).  A tile that is run again after a deep draw is
 *                             delivered to the same place.  vgl_simulate_tile_gvcf_async and the pileup are unaffected.  Call it while
 *                             no tile of the context is in flight.
 * Host handle, for a program that writes BGZF from host memory (the host program's --device-stream 1).  It is independent of any
 * vgl_ctx: one thread may drive the context while another drives the handle.  It owns n_buffers (1 .. 8) device body buffers of
 * max_body_bytes, the device stream and member buffers, the BGZF workspace, its HIP streams and page-locked member buffers.
 *   vgl_stream_host_body      body buffer k (device memory; NULL for a k out of range): the `text` of a tile call on a context with
 *                             vgl_ctx_text_device, text_cap = max_body_bytes.
 *   vgl_stream_host_submit    n_sites <= max_sites sites whose bodies lie in buffer k at [body_offsets[i], body_offsets[i + 1]) -- the
 *                             offsets the tile call returned, complete once vgl_tile_wait has returned -- and whose heads are the host
 *                             bytes heads[head_offsets[i] .. head_offsets[i + 1]).  Both arrays index ABSOLUTELY here -- the offsets
 *                             of the tile call address the body buffer as they are, and `heads` is indexed the same way -- whereas
 *                             vgl_stream_assemble_device takes pointers to site 0's first byte.  Copies heads and offsets (the caller's arrays are
 *                             free again on return), enqueues upload, assembly and compression, and returns at once with a ticket.
 *                             VGL_E_ARG, before any device call, with a message naming the argument: k out of range, buffer k still in
 *                             flight, n_sites out of range, offsets that decrease, head bytes beyond max_head_bytes, body offsets
 *                             outside the buffer.
 *   vgl_stream_host_wait      blocks until the ticket's members are in host memory: *members (owned by the handle, valid until buffer k
 *                             is submitted again) holds *members_n bytes of BGZF members WITHOUT the EOF member, *raw_n (may be NULL)
 *                             the length of the stream they decompress to.  The members are those vgl_bgzf_compress_device gives for the
 *                             stream: cut every 0xff00 bytes from the tile's first byte, the last one shorter.  n_sites = 0 or an empty
 *                             stream gives *members_n = 0.  Tickets are waited for in submit order (VGL_E_ARG otherwise).
 * No HIP device: VGL_E_NODEVICE from create. */
typedef struct vgl_stream_host vgl_stream_host;
VGL_API int vgl_stream_assemble_device(int32_t device, int32_t n_sites, const uint8_t* heads, const int64_t* head_offsets, const uint8_t* bodies,
                                       const int64_t* body_offsets, uint8_t* dst, int64_t dst_cap, int64_t* total, void* hip_stream);
VGL_API int vgl_ctx_text_device(vgl_ctx* ctx, int32_t on);
VGL_API int vgl_stream_host_create(int32_t device, int32_t n_buffers, int32_t max_sites, int64_t max_head_bytes, int64_t max_body_bytes,
                                   vgl_stream_host** out);
VGL_API uint8_t* vgl_stream_host_body(vgl_stream_host* h, int32_t k);
VGL_API int vgl_stream_host_submit(vgl_stream_host* h, int32_t k, int32_t n_sites, const uint8_t* heads, const int64_t* head_offsets,
                                   const int64_t* body_offsets, int32_t* ticket);
VGL_API int vgl_stream_host_wait(vgl_stream_host* h, int32_t ticket, const uint8_t** members, int64_t* members_n, int64_t* raw_n);
VGL_API int vgl_stream_host_destroy(vgl_stream_host* h);

/* ---- genotype calls and their discordance against the truth, tallied on the device (ABI 7, additive) -----------------------------
 * What the reference's misc/gtDiscordance computes from a call file and -printTruth's file, from a tile's arrays where they are
 * computed.  Per kept site (site_status >= 0) and sample:
 *   call missing  fmt_dp == 0 (a missing true genotype is simulated with depth 0), a true allele nibble outside 0 .. 3, or a site without a
 *                 genotype of two A/C/G/T alleles: callmis[sample] goes up and nothing else is counted
 *   call          the lowest g < nG(site) with the smallest PL among the genotypes whose two alleles both map to A/C/G/T through
 *                 alleles2acgt -- a genotype with the unobserved allele is never called; g = b (b + 1) / 2 + a, a <= b (htslib's order)
 *   GQ            gtDiscordance -doGQ 8: the smallest PL over ALL g < nG(site) that is not 0, capped at 127; 127 when there is none
 *                 (a one-allele site, every PL 0): 1 .. 127
 *   PL            pl_u8 or pl.  An int32 value outside [0, 255] (VGL_INT32_MISSING included) counts as 255, the byte pl_u8 holds for it:
 *                 both forms give the same table
 *   cell          true bases (the nibbles of gt) against called bases as unordered pairs: VGL_DISC_*
 * A skipped site (site_status < 0) is a site of the truth file that the call file lacks.
 * The table is int64: cell[sample][VGL_DISC_CELLS][128] indexed by GQ (index 0 unused), then callmis[sample], then sites[2] = kept,
 * skipped.  Totals over samples are left to the reader.  Every count is an integer sum: the table depends neither on the tiling nor on
 * the order of the additions.
 *   vgl_disc_table_len     elements of the table: n_samples * (6 * 128 + 1) + 2 (-1 for n_samples < 0).  Pure host arithmetic.
 *   vgl_disc_tally_device  ADDS one tile to `table`.  Every pointer is device memory of `device`; exactly one of pl_u8 / pl is non-NULL,
 *                          in `layout` (VGL_LAYOUT_*) with max_genotypes planes per site (vgl_max_genotypes; 1 .. 15); gt as for
 *                          vgl_simulate_tile.  Work is enqueued on `hip_stream`; the call returns without synchronising.
 *   vgl_ctx_discordance    on != 0: every following tile of the context is tallied behind its likelihood kernel into a table the context
 *                          owns (zeroed when it is first switched on), whichever entry point enqueues it: vgl_simulate_tile, _async,
 *                          _device, _text_async, _gvcf_async, with or without vgl_ctx_bcf_keys / vgl_ctx_pileup_next.  The caller need
 *                          not ask for PL or DP: the context keeps what the tally reads on the device, and the caller's own outputs are
 *                          unchanged.  A tile whose draw exceeded the staging capacity is not counted; the host entry points count the
 *                          run that replaces it, once (vgl_simulate_tile_device: nothing is counted from such a tile until
 *                          vgl_ctx_check has cleared the error).  Call it while no tile of the context is in flight.
 *   vgl_ctx_discordance_read  waits for the device, copies the table to host_table [vgl_disc_table_len(n_samples)] and, with reset != 0,
 *                          zeroes the context's table. */
#define VGL_DISC_CELLS          6
#define VGL_DISC_HOM_HOM_CONC   0
#define VGL_DISC_HOM_HOM_DISC   1
#define VGL_DISC_HET_HET_CONC   2
#define VGL_DISC_HET_HET_DISC   3
#define VGL_DISC_HOM_HET        4   /* always discordant */
#define VGL_DISC_HET_HOM        5   /* always discordant */
VGL_API int64_t vgl_disc_table_len(int32_t n_samples);
VGL_API int vgl_disc_tally_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout,
                                  const int32_t* site_status, const int32_t* n_alleles, const int8_t* alleles2acgt, const int32_t* fmt_dp,
                                  const uint8_t* pl_u8, const int32_t* pl, const uint8_t* gt, int64_t* table, void* hip_stream);
VGL_API int vgl_ctx_discordance(vgl_ctx* ctx, int32_t on);
VGL_API int vgl_ctx_discordance_read(vgl_ctx* ctx, int64_t* host_table, int32_t reset);

/* ---- the sample columns of VCF text parsed on the device (ABI 7, additive: the version stays 7) ------------------------------------
 * The host program's own record parser is the specification.  A line is the bytes up to its '\n'; its sample region is what follows
 * the ninth tab; sample column s lies between the tabs of that region.  The token of a column is its gti-th ':'-separated subfield
 * (gti = the index of GT in the line's FORMAT); a column with fewer subfields has no token and both alleles are missing.
 *   plain line    every token is absent or A or A S A: A = '.' or one or two decimal digits, S = the first '|' or '/'; a token
 *                 without S gives a1 = a0.  The line gets status VGL_VCFIN_OK, gt_out[line][s] = (b1 << 4) | b0 with
 *                 b = allele_map[line][a] & 0xF (0xF for a missing allele: allele_map holds what the caller maps allele a to,
 *                 -1 for none), and allelesum_out[line] = the sum of the non-missing allele indices.
 *   any other     an empty allele, a byte outside that grammar ('\r' included), three or more alleles, more than two digits, an
 *                 allele index >= n_alleles[line], a number of sample columns that is not n_samples, or a line whose gti is
 *                 negative or whose n_alleles is outside 1 .. 5 (allele_map has five entries): status VGL_VCFIN_HOST,
 *                 the line's row and sum are unspecified and the caller parses the line itself.
 * The kernel reads no byte outside [line_begin, line_end) and writes no byte outside the line's row, whatever the text holds.
 *   vgl_vcfin_workspace_bytes  bytes of device workspace vgl_vcfin_parse_device needs (-1 for bad arguments).  Pure host arithmetic.
 *   vgl_vcfin_parse_device     every pointer is device memory of `device`.  line_begin[i] is the offset in `text` of line i's first
 *                              sample column, line_end[i] that of its '\n' (text_bytes for a last line without one); gti and
 *                              n_alleles are int32 per line, allele_map int8 [n_lines][5].  The line ranges are compared with
 *                              text_bytes by a small kernel whose one word the call waits for: a range outside the text
 *                              (line_begin < 0, line_begin > line_end, line_end > text_bytes) returns VGL_E_ARG before the parser
 *                              is launched.  The parse itself is enqueued on `hip_stream` and not waited for.
 *   vgl_vcfin_host_create      for a program without HIP of its own: batches of lines from host memory, parsed on `device`, with
 *                              page-locked staging and device buffers owned by the handle for two batches of at most max_lines
 *                              lines and max_text_bytes bytes of text each.
 *   vgl_vcfin_host_submit      copies the text and the per-line arrays (host memory; offsets relative to `text`) into the handle's
 *                              staging, enqueues copy, parse and copy back, and returns at once with a ticket: one batch is on the
 *                              device while the caller prepares the next.  A third submit before a wait fails with VGL_E_ARG, and
 *                              so does a line range outside the text (nothing is enqueued).
 *   vgl_vcfin_host_wait        blocks until the ticket's results are in host memory: gt [n_lines][n_samples], allelesum [n_lines],
 *                              status [n_lines], owned by the handle and valid until the second submit after this one.
 * No HIP device: VGL_E_NODEVICE from vgl_vcfin_parse_device and vgl_vcfin_host_create. */
#define VGL_VCFIN_OK    0
#define VGL_VCFIN_HOST  1
typedef struct vgl_vcfin_host vgl_vcfin_host;
VGL_API int64_t vgl_vcfin_workspace_bytes(int32_t n_samples, int32_t n_lines);
VGL_API int vgl_vcfin_parse_device(int32_t device, const uint8_t* text, int64_t text_bytes, int32_t n_lines, const int64_t* line_begin,
                                   const int64_t* line_end, const int32_t* gti, const int32_t* n_alleles, const int8_t* allele_map,
                                   int32_t n_samples, uint8_t* gt_out, int32_t* allelesum_out, int32_t* status_out, void* workspace,
                                   void* hip_stream);
VGL_API int vgl_vcfin_host_create(int32_t device, int32_t n_samples, int32_t max_lines, int64_t max_text_bytes, vgl_vcfin_host** out);
VGL_API int vgl_vcfin_host_submit(vgl_vcfin_host* h, const uint8_t* text, int64_t text_bytes, int32_t n_lines, const int64_t* line_begin,
                                  const int64_t* line_end, const int32_t* gti, const int32_t* n_alleles, const int8_t* allele_map,
                                  int32_t* ticket);
VGL_API int vgl_vcfin_host_wait(vgl_vcfin_host* h, int32_t ticket, const uint8_t** gt, const int32_t** allelesum, const int32_t** status);
VGL_API int vgl_vcfin_host_destroy(vgl_vcfin_host* h);

/* ---- the FORMAT/GT vectors of BCF records decoded on the device (ABI 7, additive: the version stays 7) ------------------------------
 * The counterpart of vgl_vcfin_* for the binary format; the host program's BCF reader is the specification.  A record's GT field is
 * n_samples vectors of n values of one BCF integer type (1 = int8, 2 = int16, 3 = int32; little endian), back to back: its slice of
 * n_samples * n * width bytes starts at gt_begin, at any alignment.  Values are sign-extended; E is the type's end-of-vector value
 * (0x81, 0x8001, 0x80000001), M its missing value (0x80, 0x8000, 0x80000000).  Per sample, from its first two values v0, v1 (later
 * values do not matter):
 *      a0 = -1 if v0 == E, else (v0 >> 1) - 1;    a1 = a0 if n == 1 or v1 == E;  a1 = -1 if v0 == E;  else a1 = (v1 >> 1) - 1
 *   plain record  the type is 1, 2 or 3, n >= 1, n_alleles is in 1 .. 5 (allele_map has five entries), and every used value -- v0,
 *                 and v1 when n >= 2 and v0 != E -- is E or a value >= 0 whose allele index is below n_alleles.  The record gets status
 *                 VGL_BCFIN_OK, gt_out[record][s] = (b1 << 4) | b0 with b = allele_map[record][a] & 0xF (0xF for a == -1), and
 *                 allelesum_out[record] = the sum of the non-negative a.
 *   any other     M, another negative value, an allele index >= n_alleles, a type that is no integer type, n < 1, n_alleles outside
 *                 1 .. 5: status VGL_BCFIN_HOST, the record's row and sum are unspecified and the caller decodes the record itself.
 * The kernel reads no byte outside a record's slice and writes no byte outside its row, whatever the bytes hold.
 *   vgl_bcfin_workspace_bytes  bytes of device workspace vgl_bcfin_decode_device needs (-1 for bad arguments).  Pure host arithmetic.
 *   vgl_bcfin_decode_device    every pointer is device memory of `device`: gt [gt_bytes], gt_begin (int64), gt_type, gt_n and n_alleles
 *                              (int32) per record, allele_map int8 [n_records][5].  The slices of the records with an integer type and
 *                              n >= 1 are compared with gt_bytes by a small kernel whose one word the call waits for: gt_begin < 0 or
 *                              gt_begin + n_samples * n * width > gt_bytes returns VGL_E_ARG before the decoder is launched (which
 *                              clamps all the same).  The decode itself is enqueued on `hip_stream` and not waited for.
 *   vgl_bcfin_host_create      for a program without HIP of its own: batches of records from host memory, decoded on `device`, with
 *                              page-locked staging and device buffers owned by the handle for two batches of at most max_records
 *                              records and max_gt_bytes bytes of GT slices each, on one stream.
 *   vgl_bcfin_host_submit      src [src_bytes] is host memory that holds the records (a whole file, say) and gt_begin the offsets of
 *                              their GT slices in it; ONLY the slices are copied into the handle's staging, back to back -- what lies
 *                              between them is not sent up.  Enqueues copy, decode and copy back and returns at once with a ticket:
 *                              one batch is on the device while the caller prepares the next.  A third submit before a wait fails with
 *                              VGL_E_ARG, and so does a slice outside src or slices of more than max_gt_bytes (nothing is enqueued).
 *   vgl_bcfin_host_wait        blocks until the ticket's results are in host memory: gt [n_records][n_samples], allelesum [n_records],
 *                              status [n_records], owned by the handle and valid until the second submit after this one.  A ticket is
 *                              waited for once (VGL_E_ARG otherwise).
 * No HIP device: VGL_E_NODEVICE from vgl_bcfin_decode_device and vgl_bcfin_host_create. */
#define VGL_BCFIN_OK    0
#define VGL_BCFIN_HOST  1
typedef struct vgl_bcfin_host vgl_bcfin_host;
VGL_API int64_t vgl_bcfin_workspace_bytes(int32_t n_samples, int32_t n_records);
VGL_API int vgl_bcfin_decode_device(int32_t device, const uint8_t* gt, int64_t gt_bytes, int32_t n_records, const int64_t* gt_begin,
                                    const int32_t* gt_type, const int32_t* gt_n, const int32_t* n_alleles, const int8_t* allele_map,
                                    int32_t n_samples, uint8_t* gt_out, int32_t* allelesum_out, int32_t* status_out, void* workspace,
                                    void* hip_stream);
VGL_API int vgl_bcfin_host_create(int32_t device, int32_t n_samples, int32_t max_records, int64_t max_gt_bytes, vgl_bcfin_host** out);
VGL_API int vgl_bcfin_host_submit(vgl_bcfin_host* h, const uint8_t* src, int64_t src_bytes, int32_t n_records, const int64_t* gt_begin,
                                  const int32_t* gt_type, const int32_t* gt_n, const int32_t* n_alleles, const int8_t* allele_map,
                                  int32_t* ticket);
VGL_API int vgl_bcfin_host_wait(vgl_bcfin_host* h, int32_t ticket, const uint8_t** gt, const int32_t** allelesum, const int32_t** status);
VGL_API int vgl_bcfin_host_destroy(vgl_bcfin_host* h);

/* ---- BGZF input inflated on the device (ABI 7, additive: the version stays 7) -------------------------------------------------------
 * The counterpart of vgl_bgzf_compress_device: a BGZF stream (SAMv1 4.1: independent gzip members of at most 64 KiB, each with its
 * size in a 'BC' extra subfield) is inflated one member per workgroup, RFC 1951 complete (stored, fixed and dynamic blocks, any
 * number of them per member).  zlib's inflate is the specification: a member gets
 *   VGL_INFLATE_OK    its output has exactly ISIZE bytes, their CRC32 is the trailer's, and the deflate data ends where the trailer
 *                     begins;
 *   VGL_INFLATE_HOST  anything else (a header that is not a BGZF member's, BTYPE 11, LEN / NLEN mismatch, an oversubscribed or
 *                     incomplete code -- other than the two incomplete codes zlib accepts: no distance code, or one code of one bit
 *                     --, literal/length symbol 286 / 287, distance symbol 30 / 31, a distance beyond the bytes produced, output
 *                     past ISIZE or short of it, input running out or left over, a trailer ISIZE that is not isize[m], CRC mismatch):
 *                     the member's output bytes are unspecified and the caller inflates it (or the file) itself.
 * Whatever the bytes hold, the kernel reads no byte outside [begin, begin + csize) and writes no byte outside
 * [out_off, out_off + isize) of a member.
 *   vgl_bgzf_index              pure host arithmetic, no GPU: walks the members of raw [n] by their gzip headers (magic 1f 8b 08, FLG 4,
 *                               the 'BC' subfield of length 2 anywhere among the extra subfields of XLEN bytes; BSIZE from it, ISIZE
 *                               from the trailer, ISIZE <= 65536) and writes begin / csize / isize of at most max_members members and
 *                               their number (the 28-byte EOF member counts like any other, ISIZE 0).  The arrays may be NULL with
 *                               max_members = 0 to count.  VGL_E_UNSUPPORTED for anything that is not a clean series of such members
 *                               up to byte n (plain gzip, plain text, an empty buffer, a truncated last member, trailing bytes);
 *                               VGL_E_CAPACITY (and *n_members = the count) when there are more than max_members.
 *   vgl_inflate_workspace_bytes device workspace of a call on n_members members (-1 for n_members < 0).  Pure host arithmetic.
 *   vgl_inflate_members_device  every pointer is device memory of `device`: src [src_bytes], begin (int64), csize, isize (int32) and
 *                               out_off (int64) per member, dst [dst_cap], status (int32 per member).  A small kernel compares the
 *                               ranges with the buffers and the call waits for its one word: begin < 0, csize < 0, begin + csize >
 *                               src_bytes, isize < 0 or > 65536, out_off < 0 or out_off + isize > dst_cap return VGL_E_ARG before the
 *                               decoder is launched (which clamps all the same).  The decode itself is enqueued on `hip_stream` and
 *                               not waited for.  Output ranges of different members must not overlap.
 *   vgl_inflate_host_create     for a program without HIP of its own: batches of at most max_members members from host memory,
 *                               inflated on `device`, with page-locked staging and device buffers for two batches on one stream.
 *   vgl_inflate_host_submit     src [src_bytes] holds the batch's members at begin[m] (offsets relative to src), csize[m] bytes each,
 *                               isize[m] bytes of output each; outputs lie back to back in member order.  Enqueues copy, decode and
 *                               copy back and returns at once with a ticket; a submit of batch b is allowed before the wait for
 *                               b - 1.  A third submit before a wait fails with VGL_E_ARG, and so does a range outside src or an
 *                               isize > 65536 (nothing is enqueued).
 *   vgl_inflate_host_wait       blocks until the ticket's bytes are in host memory: out [*out_bytes = the sum of isize], status
 *                               [n_members], owned by the handle and valid until the second submit after this one.
 * No HIP device: VGL_E_NODEVICE from vgl_inflate_members_device and vgl_inflate_host_create. */
#define VGL_INFLATE_OK    0
#define VGL_INFLATE_HOST  1
typedef struct vgl_inflate_host vgl_inflate_host;
VGL_API int vgl_bgzf_index(const uint8_t* raw, int64_t n, int64_t max_members, int64_t* begin, int32_t* csize, int32_t* isize, int64_t* n_members);
VGL_API int64_t vgl_inflate_workspace_bytes(int64_t n_members);
VGL_API int vgl_inflate_members_device(int32_t device, const uint8_t* src, int64_t src_bytes, int64_t n_members, const int64_t* begin,
                                       const int32_t* csize, const int64_t* out_off, const int32_t* isize, uint8_t* dst, int64_t dst_cap,
                                       int32_t* status, void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int vgl_inflate_host_create(int32_t device, int32_t max_members, vgl_inflate_host** out);
VGL_API int vgl_inflate_host_submit(vgl_inflate_host* h, const uint8_t* src, int64_t src_bytes, int32_t n_members, const int64_t* begin,
                                    const int32_t* csize, const int32_t* isize, int32_t* ticket);
VGL_API int vgl_inflate_host_wait(vgl_inflate_host* h, int32_t ticket, const uint8_t** out, int64_t* out_bytes, const int32_t** status);
VGL_API int vgl_inflate_host_destroy(vgl_inflate_host* h);

/* ---- one genotype's FORMAT/GL as CSV text on the device (ABI 7, additive: the version stays 7) --------------------------------------
 * What the reference's misc/fetchGl prints behind "POS," for a record: the GL of one requested genotype for every sample.  Alleles
 * are given as 0 .. 4 (A, C, G, T, the unobserved allele <*> / <NON_REF>), the values of alleles2acgt.  A site has a line when
 * site_status >= 0 and both alleles occur among its n_alleles entries of alleles2acgt, at indices j0 and j1; the genotype is
 * g = max (max + 1) / 2 + min and the line is value(0) "," ... "," value(n_samples - 1) "\n".  Every other site (and a site whose
 * genotype count exceeds max_genotypes) has no bytes.
 * A value: bits 0x7F800001 -> "MISSING"; otherwise glibc's %f (the exact binary value correctly rounded to six decimals, ties to even,
 * "-0.000000" for a negative value that rounds to zero, "inf" / "-inf").  The tool prints the float of the file it reads:
 *   VGL_FETCHGL_FLOAT   the simulated float (what a BCF holds): bits 0x7F800002 -> "END", another NaN -> "nan" / "-nan" by its sign
 *   VGL_FETCHGL_TEXT    the float a VCF text file gives back: the writers' 6 significant digits (vgl_text_format_device) read as the
 *                       nearest double, then the nearest float; every NaN but the missing pattern -> "nan"; from 1e21 on as _FLOAT
 *   vgl_fetchgl_bound            n_sites * n_samples * 48: the longest %f of a float has 47 characters, plus its separator or newline
 *                                (-1 for a negative argument).  Pure host arithmetic.
 *   vgl_fetchgl_workspace_bytes  device workspace of a call (-1 for a negative argument).  Pure host arithmetic.
 *   vgl_fetchgl_format_device    every pointer is device memory of `device`: gl in `layout` (VGL_LAYOUT_*) with max_genotypes
 *                                (1 .. 15) planes per site.  The contract of vgl_text_format_device: offsets [n_sites + 1] (int64),
 *                                offsets[i] = where site i's text starts in dst, offsets[n_sites] = the total; a site without a line
 *                                has length 0.  When the total exceeds dst_cap nothing is written and offsets[n_sites] is the size
 *                                needed.  Work is enqueued on `hip_stream`; the call returns without synchronising.  VGL_E_ARG for a
 *                                bad a, b, value_mode, layout, max_genotypes or n_samples < 1.
 *   vgl_ctx_fetchgl              sets the genotype (a, b in 0 .. 4) and the value mode of a context; a < 0 switches it off.  VGL_E_ARG
 *                                when the context has add_gl == 0.  Call it while no tile of the context is in flight.
 *   vgl_ctx_fetchgl_bound        vgl_fetchgl_bound for the context's samples.
 *   vgl_ctx_fetchgl_next         the side channel of vgl_ctx_pileup_next: the NEXT tile submitted on ctx by vgl_simulate_tile_async,
 *                                _text_async or _gvcf_async (vgl_simulate_tile included) is also fetched -- whether or not the caller
 *                                asks for gl: the context keeps the tile's GL on the device, the caller's own outputs are unchanged.
 *                                text and offsets [n_sites + 1] are host memory that stays valid until vgl_tile_wait, which copies only
 *                                the bytes produced.  A text larger than text_cap: VGL_E_CAPACITY from vgl_tile_wait with text_needed
 *                                set.  A tile that is run again on the sibling context after a deep draw is fetched again from the
 *                                rerun's values; the first run's text is never delivered.  NULL withdraws the request.
 *                                vgl_simulate_tile_device has no side channel: its caller holds the tile's device arrays and calls
 *                                vgl_fetchgl_format_device on them. */
typedef struct vgl_fetchgl_tile {
    uint8_t* text;          /* host, text_cap bytes */
    int64_t  text_cap;
    int64_t* offsets;       /* host, n_sites + 1 */
    int64_t  text_needed;   /* out (vgl_tile_wait): the size of the tile's text */
} vgl_fetchgl_tile;
#define VGL_FETCHGL_FLOAT 0
#define VGL_FETCHGL_TEXT  1
VGL_API int64_t vgl_fetchgl_bound(int32_t n_samples, int32_t n_sites);
VGL_API int64_t vgl_fetchgl_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_fetchgl_format_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t layout,
                                      const int32_t* site_status, const int32_t* n_alleles, const int8_t* alleles2acgt, const float* gl,
                                      int32_t a, int32_t b, int32_t value_mode, uint8_t* dst, int64_t dst_cap, int64_t* offsets,
                                      void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int vgl_ctx_fetchgl(vgl_ctx* ctx, int32_t a, int32_t b, int32_t value_mode);
VGL_API int64_t vgl_ctx_fetchgl_bound(const vgl_ctx* ctx, int32_t n_sites);
VGL_API int vgl_ctx_fetchgl_next(vgl_ctx* ctx, vgl_fetchgl_tile* p);

/* ---- a prescribed REF/ALT list for every record, on the device (ABI 7, additive: the version stays 7) ------------------------------
 * What the reference's misc/setAlleles does to a record file, done to the arrays of a tile before any writer reads them.  For a site
 * with site_status >= 0 and its target entry -- 8 bytes: [n_alleles_new (2 .. 5), a0 .. a4 as 0 .. 4 (A, C, G, T, the unobserved
 * allele <*> / <NON_REF>; -1 behind the count), 2 pad bytes] --
 *   old2new[a]      the index of old allele a (alleles2acgt) in the new list, or -1;
 *   oldgt2newgt[g]  bcf_alleles2gt(old2new[a1], old2new[a2]) for g = a2 (a2 + 1) / 2 + a1 when both are >= 0
 *   qs              new[old2new[a]] = old[a]; entries behind the new count keep what they held
 *   gl, pl, gp      per sample new[oldgt2newgt[g]] = old[g], then: GL -- a NaN among the new values: the sample is missing and stays as
 *                   it is; otherwise the float maximum is subtracted.  PL -- VGL_INT32_MISSING among them: missing; otherwise
 *                   (int32)((float)pl - (float)min).  GP -- a NaN: missing; otherwise each value is divided by the float sum taken in
 *                   ascending genotype order (IEEE division, no fused operation)
 *   pl_u8           the same selection; a sample is missing iff fmt_dp == 0 (255 is also a capped value), otherwise v - min
 *   n_alleles, alleles2acgt   the target's, written last
 * VGL_LAYOUT_PLANES: planes g >= nGenotypes_new(site) get the missing value (0x7F800001, VGL_INT32_MISSING, 255).
 * VGL_LAYOUT_SAMPLE_MAJOR: the record's array shrinks to n_samples * nGenotypes_new(site) values at the head of its slab; what lies
 * behind it is unspecified.  Nothing else is touched: DP, I16, n_alleles_obs and the AD tags keep the old alleles (the tool leaves AD,
 * ADF and ADR with the old count -- a malformed record; vgl_ctx_set_alleles refuses a context that writes them).
 * A target that is not a list of 2 .. 5 distinct alleles all of which the record has is REFUSED (the tool reads uninitialised memory
 * for an absent allele): the site's arrays are left as they are and the smallest such site index is stored into *bad_site.
 *   vgl_setal_workspace_bytes  device workspace of a call (-1 for a negative argument).  Pure host arithmetic.
 *   vgl_setal_apply_device     every pointer is device memory of `device`.  targets [n_sites][8] (int8), site_status [n_sites],
 *                              n_alleles [n_sites] and alleles2acgt [n_sites][5] (read and written), qs [n_sites][max_alleles] or NULL,
 *                              fmt_dp [n_sites][n_samples] (needed with pl_u8), gl / pl / gp / pl_u8 in `layout` with max_genotypes
 *                              (1 .. 15) planes per site, each may be NULL.  bad_site: one int32 the CALLER sets to INT32_MAX (or any
 *                              value >= n_sites) beforehand; the call lowers it (atomic minimum) to the first refused site of the
 *                              tile, counted from 0.  Work is enqueued on `hip_stream`; the call returns without synchronising.
 *                              VGL_E_ARG for a bad count, layout, a NULL among the required pointers, pl_u8 without fmt_dp or a
 *                              workspace smaller than vgl_setal_workspace_bytes.
 *   vgl_ctx_set_alleles        `table` is host memory, n_sites entries for the absolute sites first_site .. first_site + n_sites - 1; it
 *                              is validated (VGL_E_ARG for a count outside 2 .. 5, an allele outside 0 .. 4 or a duplicate) and copied
 *                              to the device.  NULL switches the feature off.  Call it while no tile of the context is in flight.
 *                              Every tile then submitted by vgl_simulate_tile, vgl_simulate_tile_async or _text_async (text, BCF
 *                              vectors and the record streams built from them alike) is relabelled behind its likelihood kernels
 *                              and before any copy-back, formatter or encoder; a tile with a site outside the table returns
 *                              VGL_E_ARG at submit.  A tile that is run again on the sibling context after a deep draw is relabelled
 *                              from the rerun's values.  A refused site: VGL_E_SETAL from vgl_tile_wait, vgl_last_error() names the
 *                              absolute site.  VGL_E_ARG when the context has add_fmt_ad, add_info_ad, an ADF / ADR flag or do_gvcf
 *                              set; vgl_simulate_tile_gvcf_async returns VGL_E_ARG while a table is set.
 *                              vgl_simulate_tile_device has no hook: its caller holds the tile's device arrays and calls
 *                              vgl_setal_apply_device on them.  The discordance tally and the fetch-GL side channel of a context see
 *                              the tile as simulated / as relabelled respectively; composing them is not specified. */
VGL_API int64_t vgl_setal_workspace_bytes(int32_t n_samples, int32_t n_sites, int32_t max_genotypes);
VGL_API int vgl_setal_apply_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t max_genotypes, int32_t max_alleles, int32_t layout,
                                   const int8_t* targets, const int32_t* site_status, int32_t* n_alleles, int8_t* alleles2acgt, float* qs,
                                   const int32_t* fmt_dp, float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site,
                                   void* workspace, int64_t workspace_bytes, void* hip_stream);
VGL_API int vgl_ctx_set_alleles(vgl_ctx* ctx, const int8_t* table, int64_t first_site, int64_t n_sites);

/* ---- the records of --depth inf, on the device (ABI 7, additive: the version stays 7) ----------------------------------------------
 * simulate_record_true_values (vcfgl.cpp:1089-1262): no read is drawn.  From a tile's packed true genotypes `gt` (one byte per site
 * and sample, the two bases 0 .. 3 = A, C, G, T in its nibbles, as for vgl_simulate_tile_device):
 *   the allele list   the four bases by descending allele count over the site's samples, ties in the order A < C < G < T (the
 *                     reference's insertion sort swaps on strictly greater only); do_unobserved 0 / 1 / 2: the bases that occur,
 *                     3 / 4 / 5: all four; 1, 2, 4 and 5 append the unobserved allele (4)
 *   site_status       VGL_SITE_OK;  n_alleles: the length of the list;  n_alleles_obs: the number of bases that occur
 *   alleles2acgt      the list, -1 behind n_alleles
 *   gl, gp, pl, pl_u8 per sample and genotype g < nG(site) = n_alleles (n_alleles + 1) / 2: at the sample's true genotype
 *                     bcf_alleles2gt(index of base 0, index of base 1) GL 0 (bits 0x00000000), GP 1, PL 0; at every other one GL -inf
 *                     (bits 0xFF800000), GP 0, PL 255.  Each array may be NULL.
 * VGL_LAYOUT_PLANES: planes g >= nG(site) get the missing value (0x7F800001, VGL_INT32_MISSING, 255).
 * VGL_LAYOUT_SAMPLE_MAJOR: the record's array is the n_samples * nG(site) values at the head of its slab; nothing behind it is written.
 * A nibble outside 0 .. 3 makes the site BAD: the smallest such site index is stored into *bad_site; the per-site arrays of a bad
 * site are written from the nibbles that are valid, its gl / gp / pl / pl_u8 are unspecified.
 *   vgl_inf_workspace_bytes  device workspace of a call (-1 for a negative argument).  Pure host arithmetic.
 *   vgl_inf_fill_device      every pointer is device memory of `device`.  gt [n_sites][n_samples]; site_status, n_alleles and
 *                            n_alleles_obs [n_sites], alleles2acgt [n_sites][5] (all four required); gl / pl / gp / pl_u8 in `layout`
 *                            with max_genotypes planes per site.  bad_site: one int32 the CALLER sets to INT32_MAX (or any value >=
 *                            n_sites) beforehand; the call lowers it (atomic minimum) to the first bad site of the tile, counted
 *                            from 0.  Work is enqueued on `hip_stream`; the call returns without synchronising.  VGL_E_ARG for a bad
 *                            count, do_unobserved outside 0 .. 5, a max_genotypes / max_alleles pair that do_unobserved does not
 *                            give (10 / 4 for 0 and 3, else 15 / 5: vgl_max_genotypes, vgl_max_alleles), a bad layout, a NULL among
 *                            gt, the four per-site arrays and bad_site, or a workspace smaller than vgl_inf_workspace_bytes.
 *   vgl_ctx_true_values      on != 0: every tile the context is then given through vgl_simulate_tile, _async, _text_async or
 *                            vgl_simulate_tile_device is filled from its gt as above instead of simulated (do_unobserved, the
 *                            layout and add_gl / add_gp / add_pl are the context's; no random draw is consumed).  The text formatter,
 *                            vgl_ctx_bcf_keys, vgl_ctx_text_device and the stream handles work as for a simulated tile, with the
 *                            FORMAT fields in the reference's order for such records: GL, GP, PL (vcfgl.cpp:1243-1259), for text
 *                            and BCF vectors alike.  on = 0: the context simulates again, exactly as before.  Call it while no
 *                            tile of the context is in flight.  VGL_E_ARG when the context's parameters ask for what true values
 *                            do not define (add_fmt_dp, add_info_dp, an AD / ADF / ADR flag, add_qs, add_i16), or while a
 *                            discordance tally, a fetch-GL genotype or a set-alleles table is set.  While it is on, VGL_E_ARG from
 *                            a tile call whose vgl_tile_out has a non-NULL info_dp, info_ad, info_adf, info_adr, qs, i16, fmt_dp,
 *                            fmt_ad, fmt_adf, fmt_adr, reads, read_errp or site_pick_err, from a tile call with a pileup or
 *                            fetch-GL tile pending, a tally or a table set, and from vgl_simulate_tile_gvcf_async.  A bad site:
 *                            VGL_E_ARG from vgl_tile_wait / vgl_ctx_check, vgl_last_error() names the absolute site (the smallest
 *                            one of the tiles checked).  The sampler's tables and staging the context allocated at creation stay. */
VGL_API int64_t vgl_inf_workspace_bytes(int32_t n_samples, int32_t n_sites);
VGL_API int vgl_inf_fill_device(int32_t device, int32_t n_samples, int32_t n_sites, int32_t do_unobserved, int32_t max_genotypes, int32_t max_alleles,
                                int32_t layout, const uint8_t* gt, int32_t* site_status, int32_t* n_alleles, int32_t* n_alleles_obs, int8_t* alleles2acgt,
                                float* gl, int32_t* pl, float* gp, uint8_t* pl_u8, int32_t* bad_site, void* workspace, int64_t workspace_bytes,
                                void* hip_stream);
VGL_API int vgl_ctx_true_values(vgl_ctx* ctx, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* VCFGL_HIP_H */
