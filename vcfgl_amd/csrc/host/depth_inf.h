// depth_inf.h -- --depth inf: no sampling, no device
#pragma once
#include "out_header.h"
#include "run_report.h"

// simulate_record_true_values, vcfgl.cpp:1089-1262: the true genotype gets GL 0 / GP 1 / PL 0 and every other genotype -inf / 0 / 255
static void run_depth_inf(const Args& a, const Vcf& vcf, SiteStream& stream, vsink::Sink& truth_sink, RunLog& runlog) {
    const int N = (int)vcf.samples.size();
    const std::string ext = output_ext(a);
    size_t n_sites_total = 0;
    vsink::Sink out; out.text_float = put_float;
    out.open(a.out_prefix + ext, a.output_mode[0], output_header(a, vcf, true), vcf.samples, 1, bgzf_device(a));
    const bool explode_acgt = a.do_unobserved >= 3;
    const bool add_unobs = (a.do_unobserved == 1 || a.do_unobserved == 2 || a.do_unobserved == 4 || a.do_unobserved == 5);
    std::string line;
    std::vector<uint8_t> gtrow(N);
    SiteMeta S;
    while (stream.next(gtrow.data(), S)) {
        n_sites_total++;
        int ac[4] = {0, 0, 0, 0};
        for (int s = 0; s < N; s++) {
            const int b0 = gtrow[s] & 0xF, b1 = (gtrow[s] >> 4) & 0xF;
            if (b0 > 3 || b1 > 3) die("--depth inf needs complete A/C/G/T genotypes (position %ld)", S.pos0 + 1);
            ac[b0]++; ac[b1]++;
        }
        int order[4] = {0, 1, 2, 3}, n_obs = 0;
        for (int i = 0; i < 4; ++i) {
            if (ac[i] > 0) n_obs++;
            for (int j = i; j > 0 && ac[order[j]] > ac[order[j - 1]]; j--) std::swap(order[j], order[j - 1]);
        }
        std::vector<std::string> al;
        int idx_of[5] = {-1, -1, -1, -1, -1};
        const int n_acgt = explode_acgt ? 4 : n_obs;
        for (int i = 0; i < n_acgt; i++) { idx_of[order[i]] = (int)al.size(); al.push_back(allele_name(order[i], nullptr)); }
        if (add_unobs) al.push_back(nonref_name(a));
        const int nA = (int)al.size(), nG = nA * (nA + 1) / 2;
        line = S.rec->chrom; char hb[64]; snprintf(hb, sizeof hb, "\t%ld\t", S.pos0 + 1); line += hb;
        line += S.rec->id; line += '\t'; line += al[0]; line += '\t';
        if (nA == 1) line += '.'; else for (int k = 1; k < nA; k++) { if (k > 1) line += ','; line += al[k]; }
        line += '\t'; line += S.rec->qual; line += '\t'; line += S.rec->filt; line += '\t'; line += S.rec->info; line += '\t';
        std::string fmt;
        if (a.add_gl) fmt += "GL"; if (a.add_gp) { if (!fmt.empty()) fmt += ':'; fmt += "GP"; } if (a.add_pl) { if (!fmt.empty()) fmt += ':'; fmt += "PL"; }
        line += fmt.empty() ? "." : fmt;
        for (int s = 0; s < N; s++) {
            const int i0 = idx_of[gtrow[s] & 0xF], i1 = idx_of[(gtrow[s] >> 4) & 0xF];
            const int tg = i0 > i1 ? i0 * (i0 + 1) / 2 + i1 : i1 * (i1 + 1) / 2 + i0;
            line += '\t';
            bool first = true;
            auto sep = [&]() { if (!first) line += ':'; first = false; };
            if (a.add_gl) { sep(); for (int g = 0; g < nG; g++) { if (g) line += ','; line += (g == tg) ? "0" : "-inf"; } }
            if (a.add_gp) { sep(); for (int g = 0; g < nG; g++) { if (g) line += ','; line += (g == tg) ? "1" : "0"; } }
            if (a.add_pl) { sep(); for (int g = 0; g < nG; g++) { if (g) line += ','; line += (g == tg) ? "0" : "255"; } }
            if (first) line += '.';
        }
        out.write_line(line);
    }
    out.close();
    if (a.print_truth) truth_sink.close();
    char sb[512]; snprintf(sb, sizeof sb, "\n\n-> Simulation finished successfully.\n\nSummary:\n\tNumber of samples: %d\n\tTotal number of sites simulated: %zu\n", N, n_sites_total);
    fputs(sb, stderr);
    std::vector<std::string> files = {"-> Simulation output file: " + a.out_prefix + ext};
    if (a.print_truth) files.push_back("-> True genotypes output file: " + a.out_prefix + ".truth" + ext);
    runlog.finish(sb, files);
}
