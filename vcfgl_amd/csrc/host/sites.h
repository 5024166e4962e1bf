// sites.h -- the sites of a run in simulation order (the record loop incl. -explode and the input filters), and the qScore
// arithmetic of the per-read listings
#pragma once
#include "vcf_input.h"

// ---------------------------------------------------------------------------------------
// qScores on the host, for the TSV lines of -printQsError / -printGlError / -printQScores and the adjusted
// pileup (--adjust-qs 4): the library hands over the deviates, this is vcfgl.cpp:494-523 / :1664-1693 on them.
static void host_errprob_to_qs(const Args& a, double ep, int& q, int& aq) {
    q = -1; aq = -1;
    if (0.0 == ep) { q = 63; if (a.error_qs != 2) aq = 63; }                   // CAP_BASEQ; the preCalc block also sets adjqs (:1668-1673)
    else if (1.0 == ep) { q = 0; if (a.error_qs != 2) aq = 0; }
    else if (0.0 < ep && ep < 1.0) {
        const double tmp = -10.0 * log10(ep);
        q = (int)tmp;
        if (a.adjust_qs) aq = (int)(tmp + a.adjust_by);
    } else die("Bad error probability value: %f", ep);
    auto bins = [&](int v) {                                                    // apply_qs_bins, vcfgl.cpp:57-64
        for (size_t i = 0; i + 2 < a.qs_bins.size(); i += 3) if (v >= a.qs_bins[i] && v <= a.qs_bins[i + 1]) return (int)a.qs_bins[i + 2];
        die("Could not find a range for the simulated qs value: %d", v);
        return 0;
    };
    if (!a.qs_bins.empty()) { q = bins(q); if (a.adjust_qs) aq = bins(aq); }
    else { q = q > 63 ? 63 : q; if (a.adjust_qs) aq = aq > 63 ? 63 : aq; }
}
// QS_TO_ERRPROB (shared.h:493): the table shared.cpp:31 holds 10^(-q/10) at 7 significant digits (checked for
// every entry by tests/test_cli_format_cpu.py against the reference's own table)
static double host_qs_to_errprob(int q) {
    if (q == 0) return 1.0;
    if (q >= 63) return 0.0000005011872;
    char b[40]; snprintf(b, sizeof b, "%.7g", pow(10.0, -(double)q / 10.0));
    return strtod(b, nullptr);
}

// One site in simulation order.  Its contig is rec->chrom: a record that -explode 1 synthesises keeps the contig of the
// template record it was copied from (reference quirk, bcf_copy at vcfgl.cpp:1490, visible in test/reference/test18).
struct SiteMeta { const Rec* rec; long pos0; char ref_char; };

// check_rec_alleles (vcfgl.cpp:75-163) + the n_allele==1 filter (vcfgl.cpp:335-338); false = skipped.
// gt_row[N] receives the packed true genotypes; truth_line (when given) the record as -printTruth writes it.
static bool make_site(const Args& a, const Rec& rec, long pos0, bool blank, int N, uint8_t* gt_row, SiteMeta& out, std::string* truth_line) {
    // (the n_allele == 1 filter below belongs to simulate_record_values and is not applied with --depth inf)
    const int n_alleles = (int)rec.alleles.size();
    if (n_alleles > 5) die("Multiallelic sites with more than 4 alleles are not supported.");
    int ra[5] = {-1, -1, -1, -1, -1};
    for (int i = 0; i < n_alleles; i++) {
        if (a.source == 1) { ra[i] = allele_to_int(rec.alleles[i]); if (ra[i] == -1) die("Allele '%s' at position %ld is not a valid base.", rec.alleles[i].c_str(), pos0 + 1); }
        else {
            const int x = rec.alleles[i][0] - '0';
            if (x != 0 && x != 1) die("[--source %d] Found allele '%s' at position %ld. Only 0 and 1 are allowed when using binary GT source.", a.source, rec.alleles[i].c_str(), pos0 + 1);
            ra[i] = x;
        }
    }
    if (a.source == 0 && n_alleles > 2) die("Multiallelic sites are not supported when using binary GT source.");
    long allelesum = 0;
    if (rec.dev_row && !blank) { memcpy(gt_row, rec.dev_row, (size_t)N); allelesum = rec.dev_sum; }      // --device-input 1: parsed, mapped through ra[] and summed on the device
    else for (int s = 0; s < N; s++) {
        int g0 = blank ? 0 : rec.gt[2 * s], g1 = blank ? 0 : rec.gt[2 * s + 1];
        int b0 = 0xF, b1 = 0xF;
        if (g0 >= 0) { if (g0 >= n_alleles) die("GT allele index out of range at position %ld", pos0 + 1); allelesum += g0; b0 = ra[g0] & 0xF; }
        if (g1 >= 0) { if (g1 >= n_alleles) die("GT allele index out of range at position %ld", pos0 + 1); allelesum += g1; b1 = ra[g1] & 0xF; }
        gt_row[s] = (uint8_t)(b0 | (b1 << 4));
    }
    if ((a.rm_invar & 1) && allelesum == 0) return false;
    if (a.rm_invar & 2) for (int k = 1; k < n_alleles; k++) if ((long)k * N * 2 == allelesum) return false;
    if (truth_line) {                                  // bcf_write(out_truth_fp, ...) at vcfgl.cpp:1518,1548,1607
        std::string& l = *truth_line;
        l = rec.chrom; char hb[48]; snprintf(hb, sizeof hb, "\t%ld\t", pos0 + 1); l += hb; l += rec.id; l += '\t';
        if (a.source == 0) l += "A\tC";                // binary source: alleles become A,C (vcfgl.cpp:127)
        else { l += rec.alleles[0]; l += '\t'; if (n_alleles == 1) l += '.'; else for (int k = 1; k < n_alleles; k++) { if (k > 1) l += ','; l += rec.alleles[k]; } }
        l += '\t'; l += rec.qual; l += '\t'; l += rec.filt; l += '\t'; l += rec.info; l += "\tGT";
        for (int s = 0; s < N; s++) { l += '\t'; l += blank ? std::string("0|0") : rec.gt_str[s]; }
    }
    if (!a.depth_inf && (a.rm_invar & 3) && n_alleles == 1) return false;
    out.rec = &rec; out.pos0 = pos0; out.ref_char = (a.source == 0) ? 'A' : rec.ref_char;
    return true;
}

// main_simulate_record_values (vcfgl.cpp:1456-1639): the sites in simulation order, produced one at a time -- the sites that
// -explode 1 adds are never materialised (BASELINE config C5: 50M exploded sites x 500 samples), the truth file is written
// as the sites go by.
struct SiteStream {
    const Args& a; const Vcf& v; const int N;
    vsink::Sink* truth = nullptr;
    size_t ri = 0; const Rec* tpl = nullptr; std::string last; long n_in = 0, tail_size = -1; bool tail = false, done = false;
    std::string tl;
    SiteStream(const Args& a_, const Vcf& v_, int N_) : a(a_), v(v_), N(N_) {}
    bool emit(const Rec& r, long pos0, bool blank, uint8_t* gt_row, SiteMeta& m) {
        tl.clear();
        const bool ok = make_site(a, r, pos0, blank, N, gt_row, m, truth ? &tl : nullptr);
        if (truth && !tl.empty()) truth->write_line(tl);
        return ok;
    }
    bool next(uint8_t* gt_row, SiteMeta& m) {
        while (!done) {
            if (!tail) {
                if (ri == v.recs.size()) {
                    if (a.explode == 1 && !v.recs.empty()) {           // to the end of the last contig (vcfgl.cpp:1565-1625)
                        auto it = v.contig_len.find(v.recs.back().chrom);
                        tail_size = (it == v.contig_len.end()) ? -1 : it->second;
                        tail = true;
                        continue;
                    }
                    done = true; break;
                }
                const Rec& r = v.recs[ri];
                if (r.chrom != last) { n_in = 0; last = r.chrom; }
                if (a.explode == 1 && n_in != r.pos0) {
                    // the reference's `while (n_in != pos)` (vcfgl.cpp:1481) never ends on such input
                    if (r.pos0 < n_in) die("[-explode 1] Record %s:%ld is not after the previous record of its contig (duplicate or unsorted positions cannot be exploded).", r.chrom.c_str(), r.pos0 + 1);
                    if (!tpl) tpl = &r;                                // bcf_copy(explode_rec, in_rec): keeps its contig (reference quirk)
                    const long p0 = n_in++;
                    if (emit(*tpl, p0, true, gt_row, m)) return true;
                    continue;
                }
                ri++; n_in++;
                if (emit(r, r.pos0, false, gt_row, m)) return true;
            } else {
                if (!(tail_size >= 0 && n_in < tail_size)) { done = true; break; }
                if (!tpl) tpl = &v.recs.back();
                const long p0 = n_in++;
                if (emit(*tpl, p0, true, gt_row, m)) return true;
            }
        }
        return false;
    }
};

// the unobserved allele's name (-doUnobserved 1 / 4: <*>, 2 / 5: <NON_REF>), and an allele of a simulated record by its
// base index (0..3 = A/C/G/T, 4 = the unobserved allele, negative = none)
static const char* nonref_name(const Args& a) { return (a.do_unobserved == 1 || a.do_unobserved == 4) ? "<*>" : "<NON_REF>"; }
static std::string allele_name(int b, const char* nonref) { return b == 4 ? std::string(nonref) : b >= 0 ? std::string(1, "ACGT"[b]) : std::string("."); }
