// hostlib/tables.h -- the constant tables a run needs, built on the host: rand48 jump tables, the qScore -> GL terms, the GL-model-1
// error-model tables, Poisson and gamma sampler constants, the one-base rows of GL model 2 and the serial mode's start state.
// Pure functions of their arguments (no HIP call, no global): vgl_ctx_create uploads what they return.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

// ---- rand48 affine powers ---------------------------------------------------------------
static inline VglAffine aff_compose(VglAffine f, VglAffine g) {      // f after g
    VglAffine r; r.a = (f.a * g.a) & VGL_MASK48; r.c = (f.a * g.c + f.c) & VGL_MASK48; return r;
}
static inline VglAffine aff_pow_of(VglAffine base, uint64_t n) {
    VglAffine r = {1, 0};
    while (n) { if (n & 1) r = aff_compose(base, r); base = aff_compose(base, base); n >>= 1; }
    return r;
}
static inline VglAffine aff_pow(uint64_t n) { return aff_pow_of(VglAffine{VGL_LCG_A, VGL_LCG_C}, n); }      // J^n, J = one rand48 step
// [n] base^k, k < n
static inline std::vector<VglAffine> aff_table(VglAffine base, size_t n) {
    std::vector<VglAffine> t(n);
    VglAffine cur = {1, 0};
    for (size_t k = 0; k < n; k++) { t[k] = cur; cur = aff_compose(base, cur); }
    return t;
}
// [max(256, read_cap)] J^(qs_read_stride * r) with the constants scaled by 16: the pool loop's states are (aff52).
// At least 256 entries (zeros behind the reads'): the two-byte-item pool loop prefetches the table entry of a lane's NEXT item from the item's 8-bit
// read index without asking whether there is a next item -- a lane past the end of its items reads an arbitrary slot and never uses what comes back
static inline std::vector<VglAffine> qs_read_table(uint64_t qs_read_stride, int read_cap) {
    std::vector<VglAffine> rt = aff_table(aff_pow(qs_read_stride), (size_t)read_cap);
    for (VglAffine& e : rt) e.c <<= 4;
    rt.resize(std::max<size_t>(256, (size_t)read_cap), VglAffine{0, 0});
    return rt;
}

// ---- qScore -> log10 GL terms: shared.cpp:110-114 lists them with 7 significant digits
// (generator: shared.h:512-527); the same doubles are obtained by rounding the formula.
static inline double round7(double v) {
    if (isinf(v) || v == 0.0) return v;
    char buf[64]; snprintf(buf, sizeof buf, "%.7g", v);
    return strtod(buf, NULL);
}
static inline std::vector<double> build_q2gl() {                     // [3][257]
    std::vector<double> t(3 * 257);
    for (int q = 0; q <= 256; q++) {
        const double p = pow(10.0, -q / 10.0);
        t[q] = round7(log10(1.0 - p));
        t[257 + q] = round7(log10((1.0 - p) / 2.0 + p / 6.0));
        t[514 + q] = round7(log10(p) - log10(3.0));
    }
    return t;
}

// ---- GL model 1 tables (htslib errmod.c cal_coef(), restated from the published model) --
// For one fixed qScore q the per-base sums of errmod_cal() depend only on (n, count):
//   bsum[n][c] = sum_{i<c} fk[i] * beta[q][n][i],   lhet[n][k] = lC[n][k] - n ln 2
// With per-read qScores (q < 0) the full fk[256] and beta[64][256][256] tables are returned instead.
static inline void build_gl1_tables(double depcorr, int q, std::vector<double>& bsum, std::vector<double>& lhet,
                             std::vector<double>* fk_out = nullptr, std::vector<double>* beta_out = nullptr) {
    const double eta = 0.03;
    double fk[256];
    fk[0] = 1.0;
    for (int n = 1; n != 256; ++n) fk[n] = pow(1. - depcorr, n) * (1.0 - eta) + eta;
    std::vector<double> lC(256 * 256, 0.0), beta(256, 0.0);
    for (int n = 1; n <= 255; ++n)
        for (int k = 1; k <= n; ++k)
            lC[n << 8 | k] = lgamma(n + 1) - lgamma(k + 1) - lgamma(n - k + 1);
    bsum.assign(256 * 256, 0.0);
    lhet.assign(256 * 256, 0.0);
    for (int n = 0; n < 256; ++n)
        for (int k = 0; k < 256; ++k) lhet[n << 8 | k] = lC[n << 8 | k] - M_LN2 * n;
    if (fk_out && beta_out) {
        fk_out->assign(fk, fk + 256);
        beta_out->assign((size_t)64 * 256 * 256, 0.0);
        for (int qv = 1; qv < 64; ++qv) {
            const double e = pow(10.0, -qv / 10.0), le = log(e), le1 = log(1.0 - e);
            for (int n = 1; n <= 255; ++n) {
                double* b = beta_out->data() + ((size_t)qv << 16 | (size_t)n << 8);
                double sum, sum1 = lC[n << 8 | n] + n * le;
                b[n] = HUGE_VAL;
                for (int k = n - 1; k >= 0; --k, sum1 = sum) {
                    sum = sum1 + log1p(exp(lC[n << 8 | k] + k * le + (n - k) * le1 - sum1));
                    b[k] = -10. / M_LN10 * (sum1 - sum);
                }
            }
        }
        return;
    }
    int qq = q < 4 ? 4 : q; if (qq > 63) qq = 63;              // errmod_cal clamps qual to [4,63]
    const double e = pow(10.0, -qq / 10.0), le = log(e), le1 = log(1.0 - e);
    for (int n = 1; n <= 255; ++n) {
        double sum, sum1 = lC[n << 8 | n] + n * le;
        beta[n] = HUGE_VAL;
        for (int k = n - 1; k >= 0; --k, sum1 = sum) {
            sum = sum1 + log1p(exp(lC[n << 8 | k] + k * le + (n - k) * le1 - sum1));
            beta[k] = -10. / M_LN10 * (sum1 - sum);
        }
        double acc = 0.0;
        bsum[n * 256 + 0] = 0.0;
        for (int c = 1; c <= n; ++c) { acc += fk[c - 1] * beta[c - 1]; bsum[n * 256 + c] = acc; }
    }
}
// errmod_cal()'s per-read term fk[w] * beta[q << 16 | n << 8 | c] (one double product, the same bits wherever it is
// formed), q in [4, 63], n <= min(255, staging capacity), c < n: compact in n and c -- [60][nc][nc]  (gl_methods.cpp:233-302: per-read qScores)
static inline std::vector<double> build_gl1_fkbeta(const std::vector<double>& fkv, const std::vector<double>& betav, int nc) {
    std::vector<double> fb((size_t)60 * nc * nc, 0.0);
    for (int q = 4; q < 64; ++q)
        for (int n = 1; n < nc; ++n)
            for (int i = 0; i < n; ++i)
                fb[((size_t)(q - 4) * nc + n) * nc + i] = fkv[i] * betav[(size_t)q << 16 | (size_t)n << 8 | (size_t)i];
    return fb;
}

// ---- samplers ---------------------------------------------------------------------------
static inline double gamma_ln_host(double xx) {                      // gamma_ln, rng.h:38-43,60-64
    static const double cof[6] = {76.18009172947146, -86.50532032941677, 24.01409824083091,
                                  -1.231739572450155, 0.1208650973866179e-2, -0.5395239384953e-5};
    double x = xx, y = xx, tmp = x + 5.5;
    tmp -= (x + 0.5) * log(tmp);
    double ser = 1.000000000190015;
    for (int j = 0; j <= 5; j++) ser += cof[j] / ++y;
    return -tmp + log(2.5066282746310005 * ser / x);
}
static inline std::vector<double> gamma_ln_table(int n) {            // [n] gamma_ln(k), k >= 1 (entry 0 unused)
    std::vector<double> gl(n, 0.0);
    for (int k = 1; k < n; k++) gl[k] = gamma_ln_host((double)k);
    return gl;
}

static inline void pois_init(VglPois* o, double lambda) {            // PoissonSampler_init, rng.h:259-280
    o->lm = lambda; o->sq = -1.0; o->alxm = -1.0; o->g = -1.0; o->st12 = 1; o->sqf = -1.0f; o->lmf = (float)lambda; o->e_hi = INFINITY;
    if (lambda < 12.0) o->g = exp(-lambda);
    else {
        o->st12 = 0; o->sq = sqrt(2.0 * lambda); o->alxm = log(lambda);
        // gamma_ln (rng.h:60-64)
        static const double cof[6] = {76.18009172947146, -86.50532032941677, 24.01409824083091,
                                      -1.231739572450155, 0.1208650973866179e-2, -0.5395239384953e-5};
        double x = lambda + 1.0, y = x, tmp = x + 5.5;
        tmp -= (x + 0.5) * log(tmp);
        double ser = 1.000000000190015;
        for (int j = 0; j <= 5; j++) ser += cof[j] / ++y;
        o->g = lambda * o->alxm - (-tmp + log(2.5066282746310005 * ser / x));
        // poisson_fast (vgl_common.hip.h): the float32 parameters, and e_hi = the smallest integer E with
        //     B(em) = 0.9 (1 + ((em + 1 - lm) / sq + 1e-6)^2) exp(em alxm - lgamma(em + 1) - g) < 2^-60   for every em >= E.
        // B(em) bounds the acceptance threshold t of every attempt whose floor is em (y < (em + 1 - lm) / sq), and B decreases from
        // em + 1 - lm = k0 >= 2 sqrt(lm) + 8 on: B(em + 1) / B(em) <= (1 + 2.2 / k) / (1 + k / lm) < 1 for k^2 > 2.2 lm -- so E is found by
        // bisection above k0.  (lgamma against the reference's six-term gamma_ln: 2e-10 relative, against a margin of 2^28.)
        o->sqf = (float)o->sq;
        const double lim = -60.0 * 0.6931471805599453;
        auto logB = [&](double em) {
            const double yb = (em + 1.0 - lambda) / o->sq + 1e-6;
            return log(0.9) + log1p(yb * yb) + em * o->alxm - lgamma(em + 1.0) - o->g;
        };
        double lo = ceil(lambda + 2.0 * sqrt(lambda) + 8.0);                // B decreases from here on
        if (logB(lo) >= lim) {
            double hi = 2.0 * lo + 64.0;
            while (logB(hi) >= lim && hi < 1e12) hi *= 2.0;
            while (hi - lo > 1.0) { const double mid = floor(0.5 * (lo + hi)); if (logB(mid) >= lim) lo = mid; else hi = mid; }
            lo = hi;
        }
        o->e_hi = (lo < 8.0e6) ? (float)lo : INFINITY;                      // (integers below 2^23 are float32 values)
    }
}

extern "C" void vgl_pois_init(VglPois* o, double lambda) { pois_init(o, lambda); }
extern "C" double vgl_gamma_ln_host(double x) { return gamma_ln_host(x); }
// VglDevParams::pois_zt: zt[k] = (float)((k alxm - gamma_ln(k + 1) - g) log2 e), k < n - 1 (the float64 operations of poisson_fast's other branch)
extern "C" void vgl_pois_zt_host(const VglPois* p, const double* gl, int n, float* zt) {
    for (int k = 0; k + 1 < n; k++) zt[k] = (float)((((double)k * p->alxm - gl[k + 1]) - p->g) * 1.4426950408889634);
    zt[n - 1] = 0.0f;
}

static inline void gamma1_init(VglGamma1* g, double shape) {         // Gamma1Sampler_init, rng.h:155-173
    double alpha = shape;
    g->alpha0 = shape; g->changed = 0; g->pad = 0;
    if (alpha < 1.0) { alpha += 1.0; g->changed = 1; }
    g->a1 = alpha - 1.0 / 3.0;
    g->a2 = 1.0 / sqrt(9. * g->a1);
}

// ---- GL model 2 with one fixed score ----------------------------------------------------
// An evaluation whose n reads all show one base ends in accumulators that depend on n alone.
// The reference's loop (gl_methods.cpp:22-59: per read one double add rounded to float per genotype, float maximum over the
// genotypes that exist, float subtraction) is run here once per n and variant; k_gl looks the three values up instead of
// running the loop for every such evaluation (most of them: all reads of a homozygous sample without a base-call error).
// Same operations in the same order and precision as k_gl's read loop (-ffp-contract=off; float / double are IEEE on this host).
// [2][read_cap + 1][3]
static inline std::vector<float> build_gl2_run(int read_cap, double pre_homT, double pre_het, double pre_homF) {
    const int rows = read_cap + 1;
    std::vector<float> run((size_t)2 * rows * 3);
    const double term[3] = {pre_homT, pre_het, pre_homF};
    for (int variant = 0; variant < 2; ++variant) {
        volatile float tr[3] = {-0.0f, -0.0f, -0.0f};                   // bcf_utils.h:310 (volatile: every step rounds to float32 in memory)
        for (int i = 0; i < 3; ++i) run[((size_t)variant * rows) * 3 + i] = tr[i];
        for (int n = 1; n < rows; ++n) {
            float mx = -INFINITY;
            for (int i = 0; i < 3; ++i) {
                const float v = (float)((double)tr[i] + term[i]);
                tr[i] = v;
                if (variant == 0 || i == 0) mx = (v > mx) ? v : mx;
            }
            for (int i = 0; i < 3; ++i) { const float d = tr[i] - mx; tr[i] = d; }
            for (int i = 0; i < 3; ++i) run[((size_t)variant * rows + n) * 3 + i] = tr[i];
        }
    }
    return run;
}

// ---- VGL_RNG_SERIAL: the generator states a run of the reference starts from --------------
static inline VglSerialState serial_start_state(int32_t seed, uint64_t x0) {
    VglSerialState hs; memset(&hs, 0, sizeof hs);
    hs.st0 = hs.st1 = hs.st2 = x0;                           // io.cpp:1054-1061: all three streams start equal
    hs.mt[0] = (uint32_t)seed;                               // io.cpp:1039, rng.h:400
    for (int i = 1; i < 624; i++) hs.mt[i] = 1812433253u * (hs.mt[i - 1] ^ (hs.mt[i - 1] >> 30)) + (uint32_t)i;
    hs.mt_idx = 624;
    hs.st_hts = VGL_HTS_RAND48_X0;                           // htslib never seeds hts_drand48
    {   // glibc srandom_r(1) + the 310 discarded outputs: the state a process that never calls srand() starts from
        int32_t word = 1; hs.rand_state[0] = 1;
        for (int i = 1; i < 31; i++) { const long hi = word / 127773, lo = word % 127773; long w = 16807 * lo - 2836 * hi; if (w < 0) w += 2147483647; word = (int32_t)w; hs.rand_state[i] = (uint32_t)word; }
        hs.rand_f = 3; hs.rand_r = 0;
        for (int k = 0; k < 310; k++) {
            hs.rand_state[hs.rand_f] += hs.rand_state[hs.rand_r];
            if (++hs.rand_f >= 31) { hs.rand_f = 0; ++hs.rand_r; } else if (++hs.rand_r >= 31) hs.rand_r = 0;
        }
    }
    return hs;
}
