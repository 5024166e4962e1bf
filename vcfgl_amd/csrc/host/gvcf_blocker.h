// gvcf_blocker.h -- the host's gVCF block builder
#pragma once
#include "host_util.h"

// ---------------------------------------------------------------------------------------
// gVCF blocks: prepare_gvcf_block(), bcf_utils.cpp:662-942.  Invariant records (one observed
// allele) whose minimum per-sample depth falls in the same --gvcf-dps range are merged into one
// record with END / MIN_DP, per-sample minimum DP and the smallest (REF,ALT),(ALT,ALT) PLs.
struct SiteView {
    const std::string* chrom; long pos0; int n_obs, n_alleles, N, G;
    const int32_t* dp;        // [N]
    const int32_t* pl;        // [G][N] planes of this site
    const float* qs;          // [n_alleles] or null
    std::string alleles;      // "A,<NON_REF>"
};
struct GvcfBlocker {
    enum { NO_WRITE = 0, FLUSH_BLOCK = 1, WRITE_SIMREC = 2 };
    std::vector<int> block_dps;
    int current_dpr = 0;
    std::vector<int32_t> dp, pl;
    std::vector<float> qsum;
    std::string chrom, alleles;
    long start_pos = -1, end_pos = -1;
    int32_t min_dp = 0;

    int prepare(const SiteView* sv) {
        if (!sv) return current_dpr == 0 ? NO_WRITE : FLUSH_BLOCK;
        if (current_dpr == 0) { if (sv->n_obs != 1) return WRITE_SIMREC; }
        else {
            if (sv->n_obs != 1) return FLUSH_BLOCK;                       // broken by a variant site
            if (*sv->chrom != chrom) return FLUSH_BLOCK;                  // other contig
            if (sv->pos0 > end_pos + 1) return FLUSH_BLOCK;               // gap
        }
        int32_t mdp = sv->dp[0];
        for (int s = 1; s < sv->N; ++s) if (mdp > sv->dp[s]) mdp = sv->dp[s];
        int r = 0;
        for (r = 0; r < (int)block_dps.size(); ++r) if (mdp < block_dps[r]) break;
        const int dp_range = r;
        if (!dp_range) return current_dpr == 0 ? WRITE_SIMREC : FLUSH_BLOCK;
        if (current_dpr != 0 && current_dpr != dp_range) return FLUSH_BLOCK;
        if (current_dpr == 0) {                                           // founder of a new block
            const int nG = sv->n_alleles * (sv->n_alleles + 1) / 2;
            open(*sv->chrom, sv->pos0, sv->pos0, sv->alleles, dp_range, mdp, sv->dp, sv->pl, sv->N, nG, sv->qs, sv->n_alleles);   // (pl sample-major, like the block's own array)
        } else {
            if (sv->n_alleles != 2 || pl.size() != (size_t)sv->N * 3) die("Unexpected number of PL values: %d", sv->N * sv->n_alleles * (sv->n_alleles + 1) / 2);
            merge(mdp, sv->dp, sv->pl, sv->N, sv->pos0);
        }
        return NO_WRITE;
    }

    // A new open block from its founder's values (a site here; --device-gvcf 1: the last block of a tile, which stays open on the
    // host until a later tile decides).  qs null: no QS sum.
    void open(const std::string& chrom_, long start, long end, const std::string& alleles_, int dpr, int32_t mdp, const int32_t* dp_, const int32_t* pl_,
              int N, int nG, const float* qs, int n_qs) {
        dp.assign(dp_, dp_ + N); pl.assign(pl_, pl_ + (size_t)N * nG);
        qsum.clear(); if (qs) qsum.assign(qs, qs + n_qs);
        chrom = chrom_; start_pos = start; end_pos = end; alleles = alleles_; min_dp = mdp; current_dpr = dpr;
    }
    // --device-gvcf 1: does a tile's first block (its founder's contig and position, its range) continue the open block?
    bool continues(const std::string& chrom_, long pos0, int dpr) const { return current_dpr != 0 && chrom_ == chrom && pos0 <= end_pos + 1 && dpr == current_dpr; }
    // The open block takes in a site, or (--device-gvcf 1) the aggregates of the device block that continues it: minimum depths, and per
    // sample the lexicographic minimum of ((REF,ALT), (ALT,ALT)) PLs; the founder stays the one from the left.  Two alleles on both sides.
    void merge(int32_t mdp, const int32_t* dp_, const int32_t* pl_, int N, long end) {
        if (min_dp > mdp) min_dp = mdp;
        for (int s = 0; s < N; ++s) {
            if (dp[s] > dp_[s]) dp[s] = dp_[s];
            const int32_t p1 = pl_[(size_t)3 * s + 1], p2 = pl_[(size_t)3 * s + 2];
            if (pl[3 * s + 1] > p1) { pl[3 * s + 1] = p1; pl[3 * s + 2] = p2; }
            else if (pl[3 * s + 1] == p1 && pl[3 * s + 2] > p2) pl[3 * s + 2] = p2;
        }
        end_pos = end;
    }

    // the eight fixed columns of a block record (also --device-gvcf 1, whose blocks carry their sample columns from the device)
    static void fixed_columns(std::string& line, const vsink::Sink& out, const std::string& chrom, long start_pos, long end_pos,
                              const std::string& alleles, int32_t min_dp, const float* qs, size_t n_qs) {
        const long end1 = end_pos + 1;                                    // 0-based -> 1-based
        line += chrom;
        char hb[64]; snprintf(hb, sizeof hb, "\t%ld\t.\t", start_pos + 1); line += hb;
        const size_t c = alleles.find(',');
        line += alleles.substr(0, c); line += '\t'; line += (c == std::string::npos) ? "." : alleles.substr(c + 1);
        line += "\t.\t.\t";
        if (end1 - start_pos >= 2) { snprintf(hb, sizeof hb, "END=%ld;", end1); line += hb; }
        snprintf(hb, sizeof hb, "MIN_DP=%d", min_dp); line += hb;
        if (n_qs) { line += ";QS="; for (size_t k = 0; k < n_qs; k++) { if (k) line += ','; out.put_float(line, qs[k]); } }
    }

    void emit(vsink::Sink& out, int N) {
        std::string line;
        fixed_columns(line, out, chrom, start_pos, end_pos, alleles, min_dp, qsum.data(), qsum.size());
        line += "\tPL:DP";
        const size_t nG = pl.size() / (size_t)N;
        for (int s = 0; s < N; ++s) {
            line += '\t';
            for (size_t g = 0; g < nG; ++g) { if (g) line += ','; put_int(line, pl[(size_t)s * nG + g]); }
            line += ':'; put_int(line, dp[s]);
        }
        out.write_line(line);
        current_dpr = 0; chrom.clear();
    }
};
