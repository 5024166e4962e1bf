// out_header.h -- the '##' lines of the files a run writes
#pragma once
#include "sites.h"

// binary output needs every contig / FILTER / INFO key of the records defined in the header (exploded sites carry the
// contig of an input record)
static void complete_header(const char mode, const Vcf& vcf, std::vector<std::string>& hdr) {
    if (mode != 'u' && mode != 'b') return;
    std::vector<std::string> contigs, filters, keys, tmp;
    auto add = [](std::vector<std::string>& v, const std::string& x) { if (!x.empty() && std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x); };
    for (const Rec& r : vcf.recs) {
        add(contigs, r.chrom);
        split(r.filt, ';', tmp); for (auto& f : tmp) add(filters, f);
        if (r.info != ".") { split(r.info, ';', tmp); for (auto& kv : tmp) add(keys, kv.substr(0, kv.find('='))); }
    }
    vsink::Sink::define_missing(hdr, contigs, filters, keys);
}

// ---- output header (set_hdr, bcf_utils.cpp:511-615): input header minus FORMAT/GT, plus our tags.
// truth_values: the header of --depth inf (no device, no library: GL / GP / PL alone, in its own order)
static std::vector<std::string> output_header(const Args& a, const Vcf& vcf, const bool truth_values) {
    std::vector<std::string> hdr;
    char hb[128];
    for (const std::string& h : vcf.header) if (h.find("##FORMAT=<ID=GT,") == std::string::npos) hdr.push_back(h);
    snprintf(hb, sizeof hb, "##source=vcfgl_hip (libvcfgl_hip ABI %d, gfx950)", vgl_abi_version());
    hdr.push_back(truth_values ? "##source=vcfgl_hip" : hb);
    hdr.push_back("##source=" + a.command);
    const char* const GL = "##FORMAT=<ID=GL,Number=G,Type=Float,Description=\"log10 genotype likelihoods, best = 0\">";
    const char* const PL = "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">";
    const char* const GP = "##FORMAT=<ID=GP,Number=G,Type=Float,Description=\"Genotype probabilities\">";
    if (truth_values) {
        if (a.add_gl) hdr.push_back(GL);
        if (a.add_gp) hdr.push_back(GP);
        if (a.add_pl) hdr.push_back(PL);
    } else {
        if (a.do_unobserved == 1 || a.do_unobserved == 4) hdr.push_back("##ALT=<ID=*,Description=\"Any other alternative allele (unobserved)\">");
        if (a.do_unobserved == 2 || a.do_unobserved == 5) hdr.push_back("##ALT=<ID=NON_REF,Description=\"Any other alternative allele (unobserved)\">");
        if (a.do_gvcf) { hdr.push_back("##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of the non-variant block\">");
                         hdr.push_back("##INFO=<ID=MIN_DP,Number=1,Type=Integer,Description=\"Smallest per-sample depth within the block\">"); }
        if (a.add_fmt_dp) hdr.push_back("##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Simulated read depth of the sample\">");
        if (a.add_info_dp) hdr.push_back("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Read depth summed over samples\">");
        if (a.add_gl) hdr.push_back(GL);
        if (a.add_pl) hdr.push_back(PL);
        if (a.add_gp) hdr.push_back(GP);
        if (a.add_qs) hdr.push_back("##INFO=<ID=QS,Number=R,Type=Float,Description=\"Normalised per-allele base quality sum\">");
        if (a.add_i16) hdr.push_back("##INFO=<ID=I16,Number=16,Type=Float,Description=\"bcftools call auxiliary tag\">");
        if (a.add_fmt_ad) hdr.push_back("##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic depths\">");
        if (a.add_fmt_adf) hdr.push_back("##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"Allelic depths, forward strand\">");
        if (a.add_fmt_adr) hdr.push_back("##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"Allelic depths, reverse strand\">");
        if (a.add_info_ad) hdr.push_back("##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Total allelic depths\">");
        if (a.add_info_adf) hdr.push_back("##INFO=<ID=ADF,Number=R,Type=Integer,Description=\"Total allelic depths, forward strand\">");
        if (a.add_info_adr) hdr.push_back("##INFO=<ID=ADR,Number=R,Type=Integer,Description=\"Total allelic depths, reverse strand\">");
    }
    complete_header(a.output_mode[0], vcf, hdr);
    return hdr;
}

// -printTruth 1: the input's own header (FORMAT/GT included) for <prefix>.truth.*
static std::vector<std::string> truth_header(const Args& a, const Vcf& vcf) {
    std::vector<std::string> hdr = vcf.header;
    hdr.push_back("##source=vcfgl_hip"); hdr.push_back("##source=" + a.command);
    complete_header(a.output_mode[0], vcf, hdr);
    return hdr;
}
