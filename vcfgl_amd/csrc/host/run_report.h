// run_report.h -- what a run says about itself: the <prefix>.arg log, the stage timer and --verbose 1 report, the discordance table, the summary
#pragma once
#include "tile_writer.h"

// <prefix>.arg: the run log the reference writes beside its outputs (io.cpp:1031,1109; vcfgl.cpp:1657-1871)
struct RunLog {
    FILE* fp = nullptr; std::string prefix; time_t t0 = 0; clock_t c0 = 0;
    void open(const Args& a) {
        prefix = a.out_prefix; t0 = time(NULL); c0 = clock();
        fp = fopen((prefix + ".arg").c_str(), "w");
        if (!fp) die("Could not open file: %s.arg", prefix.c_str());
        char when[64]; struct tm tmv; localtime_r(&t0, &tmv); strftime(when, sizeof when, "%a %b %d %H:%M:%S %Y", &tmv);
        fprintf(fp, "vcfgl_hip (libvcfgl_hip ABI %d, gfx950)\n\n%s\n\n\n[Program start] %s\n", vgl_abi_version(), a.command.c_str(), when);
    }
    void finish(const std::string& summary, const std::vector<std::string>& files) {
        if (!fp) return;
        fputs(summary.c_str(), fp);
        fprintf(fp, "\n\tElapsed time (CPU): %f seconds\n\tElapsed time (Real): %f seconds\n", (double)(clock() - c0) / CLOCKS_PER_SEC, difftime(time(NULL), t0));
        fprintf(fp, "\n-> Log file: %s.arg\n", prefix.c_str());
        for (const std::string& f : files) fprintf(fp, "%s\n", f.c_str());
        fclose(fp); fp = nullptr;
    }
};

// <prefix>.discordance.tsv: the table of --gt-discordance 1 (include/vcfgl_hip.h: cell[sample][6][128] by GQ, callmis[sample], sites[2]) in
// the layout misc/gtDiscordance prints for -doGQ `mode` (gtDiscordance.cpp:629-833: columns, order, %d / %f; rows k = 1 .. 129)
static std::string format_discordance(const std::vector<int64_t>& t, const std::vector<std::string>& names, int mode) {
    const size_t n = names.size();
    const int64_t* cell = t.data(); const int64_t* mis = cell + n * VGL_DISC_CELLS * 128; const int64_t* sites = mis + n;
    auto at = [&](size_t i, int c, int k) -> long long { return k < 128 ? (long long)cell[(i * VGL_DISC_CELLS + c) * 128 + k] : 0; };
    auto rate = [](double num, double den) { char b[64]; if (den == 0) return std::string("-nan"); snprintf(b, sizeof b, "%f", num / den); return std::string(b); };
    std::string o; char b[512];
    if (mode == 0) {
        const long long kept = sites[0], skipped = sites[1], total = kept + skipped;
        for (size_t i = 0; i < n; i++) {
            long long c[VGL_DISC_CELLS];
            for (int j = 0; j < VGL_DISC_CELLS; j++) { c[j] = 0; for (int k = 0; k < 128; k++) c[j] += at(i, j, k); }
            const long long compared = c[0] + c[1] + c[2] + c[3] + c[4] + c[5], disc = c[1] + c[3] + c[4] + c[5];
            char m[64]; snprintf(m, sizeof m, "%f", total ? 1.0 - (double)compared / (double)total : 0.0);
            o += names[i];
            snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t", total, kept, compared, (long long)mis[i], disc, skipped, compared - disc); o += b;
            o += total ? std::string(m) : std::string("-nan"); o += '\t'; o += rate((double)disc, (double)compared); o += '\t'; o += rate((double)(compared - disc), (double)compared);
            snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld", c[VGL_DISC_HOM_HOM_CONC], c[VGL_DISC_HET_HET_CONC], c[VGL_DISC_HOM_HOM_DISC], c[VGL_DISC_HOM_HET],
                     c[VGL_DISC_HET_HOM], c[VGL_DISC_HET_HET_DISC]); o += b;
            const int ord[6] = {VGL_DISC_HOM_HOM_CONC, VGL_DISC_HET_HET_CONC, VGL_DISC_HOM_HOM_DISC, VGL_DISC_HOM_HET, VGL_DISC_HET_HOM, VGL_DISC_HET_HET_DISC};
            for (int j : ord) { o += '\t'; o += rate((double)c[j], (double)compared); }
            o += '\n';
        }
        return o;
    }
    // a -doGQ 4 row: discordant (all, hom->hom, hom->het, het->hom, het->het), concordant (all, hom->hom, het->het)
    auto row = [&](size_t i0, size_t i1, int k, long long r[8]) {
        for (int j = 0; j < 8; j++) r[j] = 0;
        for (size_t i = i0; i < i1; i++) {
            r[1] += at(i, VGL_DISC_HOM_HOM_DISC, k); r[2] += at(i, VGL_DISC_HOM_HET, k); r[3] += at(i, VGL_DISC_HET_HOM, k); r[4] += at(i, VGL_DISC_HET_HET_DISC, k);
            r[6] += at(i, VGL_DISC_HOM_HOM_CONC, k); r[7] += at(i, VGL_DISC_HET_HET_CONC, k);
        }
        r[0] = r[1] + r[2] + r[3] + r[4]; r[5] = r[6] + r[7];
    };
    long long r[8];
    if (mode == 3 || mode == 4) {
        for (int k = 1; k < 130; k++) {
            row(0, n, k, r);
            if (mode == 3) snprintf(b, sizeof b, "%d\t%lld\t%lld\n", k, r[0], r[5]);
            else snprintf(b, sizeof b, "%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", k, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
            o += b;
        }
        return o;
    }
    for (size_t i = 0; i < n; i++) {
        long long compared = 0;
        for (int j = 0; j < VGL_DISC_CELLS; j++) for (int k = 0; k < 128; k++) compared += at(i, j, k);
        for (int k = 1; k < 130; k++) {
            row(i, i + 1, k, r);
            if (mode == 5) snprintf(b, sizeof b, "%zu\t%d\t%lld\t%lld\t%lld\n", i, k, r[0], r[5], compared);
            else snprintf(b, sizeof b, "%zu\t%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", i, k, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], compared);
            o += b;
        }
    }
    return o;
}

// --gt-discordance 1: every context's table, summed: integer counts, the same for any device count
static void write_discordance(const Args& a, const Vcf& vcf, const std::vector<vgl_ctx*>& ctxs) {
    const int64_t len = vgl_disc_table_len((int)vcf.samples.size());
    std::vector<int64_t> table((size_t)len, 0), part((size_t)len);
    for (vgl_ctx* ctx : ctxs) {
        if (vgl_ctx_discordance_read(ctx, part.data(), 0) != VGL_OK) die("--gt-discordance 1: %s", vgl_last_error());
        for (int64_t k = 0; k < len; k++) table[(size_t)k] += part[(size_t)k];
    }
    const std::string tsv_text = format_discordance(table, vcf.samples, a.disc_gq);
    FILE* fp = fopen((a.out_prefix + ".discordance.tsv").c_str(), "w");
    if (!fp) die("Could not open file: %s.discordance.tsv", a.out_prefix.c_str());
    if (fwrite(tsv_text.data(), 1, tsv_text.size(), fp) != tsv_text.size() || fclose(fp) != 0) die("Could not write file: %s.discordance.tsv", a.out_prefix.c_str());
}

// --verbose 1: the [device N], [timing] and [input] lines on stderr
static void verbose_report(const Args& a, const RunPlan& P, const std::vector<vgl_ctx*>& ctxs, const std::vector<std::unique_ptr<DeviceWorker>>& workers,
                           const TileWriter& w, const InputStats& in_stats) {
    const int N = P.N, A = P.A, G = P.G;
    // bytes a finished tile brings back over the link, per site (the FORMAT arrays dominate: sample-major slabs, copied whole)
    // (--device-text 1 / --device-gvcf 1 / --device-bcf 1: the text or the encoded vectors instead of the FORMAT arrays, counted as they come back)
    const double bytes_per_site = P.rec0 ? 64.0 : (double)N * ((P.want_dp ? 4.0 : 0.0) + (P.path != ARRAYS ? 0.0 : 4.0 * G * ((a.add_gl ? 1 : 0) + (a.add_pl ? 1 : 0) + (a.add_gp ? 1 : 0)) +
                                               4.0 * A * ((a.add_fmt_ad ? 1 : 0) + (a.add_fmt_adf ? 1 : 0) + (a.add_fmt_adr ? 1 : 0)))) + 64.0;
    // per device: tiles, sites, bytes of tags copied back and the rate over the device's own busy interval (first submit to last
    // completed wait) -- a multi-GPU run shows an idle or slow device (or link) here at once
    for (int d = 0; d < P.D; d++) {
        const DeviceWorker& W = *workers[d];
        vgl_ctx_info_t ci; memset(&ci, 0, sizeof ci); ci.size = (int32_t)sizeof ci;
        (void)vgl_ctx_info(ctxs[d], &ci);
        const double dt = W.t_last - W.t_first, gb = (bytes_per_site * (double)W.sites + W.text_bytes + w.stream_down[d]) / 1e9;
        if (P.stream) fprintf(stderr, "[device %d] --device-stream 1: %.6f GB of heads and offsets sent up, %.6f GB of BGZF members copied back\n", P.devices[d], w.stream_up[d] / 1e9, w.stream_down[d] / 1e9);
        fprintf(stderr, "[device %d] %ld tiles, %ld sites, %.3f GB of tags copied back in %.3f s = %.1f GB/s, %.3g evaluations/s; context: %.2f GB workspace, k_sample build %d, fused %d (split %d)\n",
                P.devices[d], W.tiles, W.sites, gb, dt > 0 ? dt : 0.0, dt > 0 ? gb / dt : 0.0, dt > 0 ? (double)W.sites * N / dt : 0.0,
                (double)ci.workspace_bytes / 1e9, ci.sample_lean, ci.fused, ci.fused_split);
    }
    if (P.fetch) fprintf(stderr, "[fetch-gl] --fetch-gl %s (%s values): %ld lines written, %ld sites without the genotype\n", a.fetch_gl.c_str(),
                         a.fetch_mode == VGL_FETCHGL_TEXT ? "VCF text" : "simulated float", w.n_fetch_lines, w.n_fetch_absent);
    const double* t = w.timer.t;
    fprintf(stderr, "\n[timing] read input %.3f s, decode sites %.3f s, device context(s) %.3f s, waiting for the device(s) (simulation incl. PCIe, overlapped with the writer) %.3f s, encode %.3f s, write/compress %.3f s, tile buffers %.3f s, teardown %.3f s, pileup %.3f s\n",
            t[StageTimer::READ], t[StageTimer::SITES], t[StageTimer::CONTEXT], t[StageTimer::DEVICE_WAIT], t[StageTimer::ENCODE], t[StageTimer::WRITE], t[StageTimer::TILE_BUFFERS],
            t[StageTimer::TEARDOWN], t[StageTimer::PILEUP]);
    // the parts of "read input" (the HIP runtime's start-up, which the reading overlaps with, is what remains of it)
    fprintf(stderr, "[input] --device-input %d: %ld lines parsed on the device, %ld of them again on the host, %.3f GB of text sent up; file read %.3f s, line scan %.3f s, fixed columns %.3f s, device parse and wait %.3f s, host %s %.3f s\n",
            a.device_input, in_stats.lines_dev, a.device_input ? in_stats.lines_host : 0L, in_stats.text_up / 1e9, in_stats.t_read, in_stats.t_scan, in_stats.t_fixed,
            in_stats.t_dev, a.device_input ? "re-parse" : "parse", in_stats.t_host);
    if (a.device_bcf_input)
        fprintf(stderr, "[input] --device-bcf-input 1: %ld records decoded on the device, %ld of them again on the host, %.3f GB of genotype bytes sent up; %s%s; header and record chain %.3f s, shared blocks %.3f s, device decode and wait %.3f s, host GT loop %.3f s\n",
                in_stats.bcf_dev, in_stats.bcf_host, in_stats.gt_up / 1e9, in_stats.bcf_fallback ? "the host read the file: " : "no fallback",
                in_stats.bcf_fallback ? in_stats.bcf_fallback : "", in_stats.bt_scan, in_stats.bt_shared, in_stats.bt_dev, in_stats.bt_host);
    if (!a.device_inflate) fprintf(stderr, "[input] --device-inflate 0: the host read the file (zlib)\n");
    else fprintf(stderr, "[input] --device-inflate 1: %ld members inflated on the device, %lld compressed bytes sent up, %lld inflated bytes received, %s%s; inflate stage %.3f s of file read %.3f s\n",
                 in_stats.members_dev, (long long)in_stats.inflate_up, (long long)in_stats.inflate_down, in_stats.fallback ? "the host read the file (zlib): " : "no fallback",
                 in_stats.fallback ? in_stats.fallback : "", in_stats.t_inflate, in_stats.t_read);
}

// the summary on stderr and, with the list of the files written, at the end of the run log
static void finish_run(const Args& a, const RunPlan& P, RunLog& runlog, const size_t n_sites_total, const TileWriter& w) {
    char sb[512];
    if (P.inf) snprintf(sb, sizeof sb, "\n\n-> Simulation finished successfully.\n\nSummary:\n\tNumber of samples: %d\n\tTotal number of sites simulated: %zu\n", P.N, n_sites_total);   // (run_depth_inf's block)
    else
    snprintf(sb, sizeof sb, "\n\n-> Simulation finished successfully.\n\nSummary:\n\tNumber of samples: %d\n\tTotal number of sites simulated: %zu\n"
                            "\tNumber of sites included in simulation output file: %ld\n\tNumber of sites skipped: %ld\n", P.N, n_sites_total, w.n_out, w.n_skipped);
    fputs(sb, stderr);
    std::vector<std::string> files;
    if (!P.rec0) files.push_back("-> Simulation output file: " + a.out_prefix + P.ext);
    if (a.gt_disc) files.push_back("-> Genotype discordance file: " + a.out_prefix + ".discordance.tsv");
    if (a.fetch) files.push_back("-> Fetched genotype likelihoods file: " + a.out_prefix + ".fetchgl.csv");
    if (a.print_pileup) files.push_back("-> Pileup output file: " + a.out_prefix + ".pileup.gz");
    if (a.print_truth) files.push_back("-> True genotypes output file: " + a.out_prefix + ".truth" + P.ext);
    if (a.print_bpe) files.push_back("-> Base pick error output: stdout");
    if (a.print_qs_err) files.push_back("-> QS error output: stdout");
    if (a.print_gl_err) files.push_back("-> GL error output: stdout");
    if (a.print_qscores) files.push_back("-> Qscores output: stdout");
    fflush(stdout);
    runlog.finish(sb, files);
}
