// vcfgl_hip -- command-line front end with vcfgl's flag surface (io.cpp:538-752) over the C ABI
// of libvcfgl_hip.so.  It restates, on the host, what surrounds the hot path in the reference:
//   * the flag parser / defaults / range checks          io.cpp:428-526, 538-752, 757-1000
//   * the record loop incl. -explode and input filters   vcfgl.cpp:75-163, 1456-1639
//   * tag formatting of add_tags()                       bcf_utils.cpp:426-507
//   * VCF text in; VCF text / bgzip'd VCF / BCF out (vcf_sink.h; neither box has htslib): float
//     printing follows htslib's kputd() (6 significant digits, %g outside [1e-4, 999999]), so
//     `diff -I '^##'` against the reference's golden VCFs is empty in --rng-mode 1 (serial) runs.
// Records are batched into tiles and simulated on the GPU by vgl_simulate_tile(); there is no
//   * the gVCF block builder prepare_gvcf_block()         bcf_utils.cpp:662-942
//   * --depth inf (simulate_record_true_values, vcfgl.cpp:1089-1262): no sampling at all, the true
//     genotype gets GL 0 / GP 1 / PL 0 and every other genotype -inf / 0 / 255; written directly (depth_inf.h), or with
//     --device-inf 1 made on the device (vgl_ctx_true_values) and sent through the device run like simulated tiles
//   * -printTruth 1: the decoded input records (incl. exploded ones) as <prefix>.truth.vcf
// CPU simulation path here.  Input: VCF text, gzip / bgzip'd VCF, BCF (raw or BGZF).
// The units, each a header beside this file: host_util.h (exit, clock, number text), cli_args.h, vcf_input.h, sites.h, gvcf_blocker.h,
// out_header.h, run_plan.h (RunPlan, TileBufs), device_worker.h, tile_writer.h, run_report.h, depth_inf.h, self_test.h, set_alleles.h.
#include "depth_inf.h"
#include "self_test.h"
#include "set_alleles.h"

// ---- the tile ring: produce (decode sites, hand the tile to its device) up to R tiles ahead, write in order.  Returns the number of sites.
// An entry's buffers are page-locked when the entry is first used (about 0.04 s per 250 MB): the second entry of a device is
// prepared while the device already works on the first tile
static size_t run_ring(const Args& a, const RunPlan& P, SiteStream& stream, const std::vector<vgl_ctx*>& ctxs, std::vector<std::unique_ptr<TileBufs>>& ring,
                       const std::vector<std::unique_ptr<DeviceWorker>>& workers, TileWriter& w, const size_t setal_lines) {
    const size_t R = (size_t)P.R, D = (size_t)P.D;
    StageTimer& timer = w.timer;
    size_t n_sites_total = 0, produced = 0, consumed = 0;
    size_t retired = 0;                                         // --device-stream 1: tiles whose members are written (one behind `consumed`); else = consumed
    bool eof = false;
    std::map<std::string, int32_t> contig_ids; const std::string* last_chrom = nullptr; int32_t last_id = 0;
    auto entry = [&](size_t ri) -> TileBufs& {
        if (!ring[ri]) { ring[ri].reset(new TileBufs()); ring[ri]->allocate(a, P, ctxs[ri % D], P.devices[ri % D], (int)(ri / D)); }
        return *ring[ri];
    };
    entry(0);
    timer.lap(StageTimer::TILE_BUFFERS);
    for (;;) {
        while (!eof && produced - retired < R) {
            TileBufs& B = entry(produced % R);
            B.ns = 0; B.t0 = (int64_t)n_sites_total; B.done = false; B.dev = (int)(produced % D); B.bad_pos = -1;
            while (B.ns < P.TS && stream.next(&B.gt[(size_t)B.ns * P.N], B.meta[B.ns])) B.ns++;
            if (B.ns < P.TS) eof = true;
            if (B.ns == 0) break;
            if (P.path == GVCF) for (int i = 0; i < B.ns; i++) {        // contig ids: equal for equal names (the device compares ids)
                const std::string& c = B.meta[i].rec->chrom;
                if (last_chrom == nullptr || *last_chrom != c) {
                    auto ins = contig_ids.emplace(c, (int32_t)contig_ids.size());
                    last_id = ins.first->second; last_chrom = &ins.first->first;
                }
                B.contig[i] = last_id; B.pos0[i] = B.meta[i].pos0;
            }
            n_sites_total += (size_t)B.ns;
            if (P.setal && n_sites_total > setal_lines)
                die("--set-alleles %s has %zu lines but the run has more records: one line per record is needed.", a.set_alleles_fn.c_str(), setal_lines);
            if (P.host_pileup) memset(B.reads.data(), 0xFF, (size_t)P.pile_cap * B.ns * P.N);
            workers[B.dev]->push(&B);
            produced++;
        }
        timer.lap(StageTimer::SITES);
        if (consumed == produced) break;
        TileBufs& B = *ring[consumed % R];
        { std::unique_lock<std::mutex> lk(B.m); B.cv.wait(lk, [&] { return B.done; }); }
        timer.lap(StageTimer::DEVICE_WAIT);
        if (B.bad_pos >= 0) die("--depth inf needs complete A/C/G/T genotypes (position %ld)", B.bad_pos);
        w.write_tile(B);
        timer.lap(StageTimer::WRITE);
        consumed++;
        // --device-stream 1: this tile is being assembled and compressed; meanwhile the one before it is written
        if (P.stream) { while (retired + 1 < consumed) { w.retire_tile(*ring[retired % R]); retired++; } timer.lap(StageTimer::WRITE); }
        else retired = consumed;
    }
    if (P.stream) { timer.restart(); while (retired < consumed) { w.retire_tile(*ring[retired % R]); retired++; } timer.lap(StageTimer::WRITE); }
    for (auto& W : workers) W->finish();
    return n_sites_total;
}

static int device_run(const Args& a, const Vcf& vcf, const int N, const int enc_threads, SiteStream& stream, vsink::Sink& truth_sink, RunLog& runlog,
                      StageTimer& timer, const InputStats& in_stats, const std::vector<int8_t>& setal_table);

// ---------------------------------------------------------------------------------------
int main(int argc, char** argv) {
    const int hook_rc = run_hook(argc, argv);
    if (hook_rc != NOT_A_HOOK) return hook_rc;
    Args a = parse_args(argc, argv);
    if (a.device_input || a.device_bcf_input) {                 // (checked before any file of the run exists, the .arg file included)
        gzFile fp = gzopen(a.in_fn.c_str(), "r"); char magic[3] = {0, 0, 0};
        if (!fp) die("Could not open file: %s", a.in_fn.c_str());
        const int k = gzread(fp, magic, 3); gzclose(fp);
        const bool bcf = k == 3 && !memcmp(magic, "BCF", 3);
        if (a.device_input && bcf) die("--device-input 1 is not supported with BCF input (its genotypes are binary already: there is no text to parse).");
        if (a.device_bcf_input && !bcf) die("--device-bcf-input 1 needs BCF input (the genotype columns of VCF text are what --device-input 1 parses).");
    }
    const std::vector<int8_t> setal_table = a.set_alleles_fn.empty() ? std::vector<int8_t>() : read_set_alleles(a);   // (a bad file: before any file of the run exists)
    RunLog runlog; runlog.open(a);
    StageTimer timer;
    const int enc_threads = encode_threads(a);
    InputStats in_stats;
    const Vcf vcf = read_input(a, enc_threads, in_stats);
    timer.lap(StageTimer::READ);
    const int N = (int)vcf.samples.size();
    if (N <= 0) die("no samples in %s", a.in_fn.c_str());
    if (!a.depths.empty() && (int)a.depths.size() != N) die("--depths-file must hold one depth per sample (%zu given, %d samples)", a.depths.size(), N);
    SiteStream stream(a, vcf, N);
    vsink::Sink truth_sink; truth_sink.text_float = put_float;
    if (a.print_truth) {                                 // written as the sites go by (vcfgl.cpp:1518,1548,1607)
        truth_sink.open(a.out_prefix + ".truth" + output_ext(a), a.output_mode[0], truth_header(a, vcf), vcf.samples, 1, bgzf_device(a));
        stream.truth = &truth_sink;
    }
    if (a.depth_inf && !a.device_inf) { run_depth_inf(a, vcf, stream, truth_sink, runlog); return 0; }
    return device_run(a.device_inf ? true_values_args(a) : a, vcf, N, enc_threads, stream, truth_sink, runlog, timer, in_stats, setal_table);
}

// ---- the device run: plan, contexts, sinks, workers, the ring
static int device_run(const Args& a, const Vcf& vcf, const int N, const int enc_threads, SiteStream& stream, vsink::Sink& truth_sink, RunLog& runlog,
                      StageTimer& timer, const InputStats& in_stats, const std::vector<int8_t>& setal_table) {
    const vgl_params p = make_params(a, N);
    const RunPlan P = make_plan(a, p, N, enc_threads);
    std::vector<vgl_ctx*> ctxs(P.D, nullptr);
    timer.restart();
    for (int d = 0; d < P.D; d++) if (vgl_ctx_create(&p, P.devices[d], P.TS, &ctxs[d]) != VGL_OK) die("%s", vgl_last_error());
    if (a.gt_disc) for (vgl_ctx* ctx : ctxs) if (vgl_ctx_discordance(ctx, 1) != VGL_OK) die("--gt-discordance 1: %s", vgl_last_error());
    if (P.fetch) for (vgl_ctx* ctx : ctxs) if (vgl_ctx_fetchgl(ctx, a.fetch_a, a.fetch_b, a.fetch_mode) != VGL_OK) die("--fetch-gl %s: %s", a.fetch_gl.c_str(), vgl_last_error());
    const size_t setal_lines = setal_table.size() / 8;
    if (P.setal) for (vgl_ctx* ctx : ctxs) if (vgl_ctx_set_alleles(ctx, setal_table.data(), 0, (int64_t)setal_lines) != VGL_OK) die("--set-alleles %s: %s", a.set_alleles_fn.c_str(), vgl_last_error());
    if (P.inf) for (vgl_ctx* ctx : ctxs) if (vgl_ctx_true_values(ctx, 1) != VGL_OK) die("--device-inf 1: %s", vgl_last_error());
    timer.lap(StageTimer::CONTEXT);
    TileWriter w(a, P, vcf, timer);
    w.open(ctxs);
    if (P.stream) w.open_streams(ctxs);
    std::vector<std::unique_ptr<TileBufs>> ring(P.R);
    std::vector<std::unique_ptr<DeviceWorker>> workers(P.D);
    for (int d = 0; d < P.D; d++) workers[d].reset(new DeviceWorker(P, ctxs[d], w.hstream[d], a.gvcf_dps));
    const size_t n_sites_total = run_ring(a, P, stream, ctxs, ring, workers, w, setal_lines);
    if (P.setal && n_sites_total != setal_lines)
        die("--set-alleles %s has %zu lines but the run has %zu records: one line per record is needed.", a.set_alleles_fn.c_str(), setal_lines, n_sites_total);
    w.flush_gvcf();
    timer.restart();
    if (!P.rec0) w.out.close();
    if (a.print_truth) truth_sink.close();
    if (a.gt_disc) write_discordance(a, vcf, ctxs);
    w.close_fetch();
    timer.lap(StageTimer::WRITE);
    if (w.pile_fp) { w.pile.close(); fclose(w.pile_fp); }
    // contexts and page-locked buffers are not torn down one by one (0.06 s): the process ends below with _exit(), after the run
    // log, and the driver releases everything at once
    timer.lap(StageTimer::TEARDOWN);
    if (a.verbose) verbose_report(a, P, ctxs, workers, w, in_stats);
    finish_run(a, P, runlog, n_sites_total, w);
    // a flush that fails here (ENOSPC, EPIPE on stdout's TSV listings) is a failed run; VCFGL_HIP_NORMAL_EXIT=1 leaves through
    // exit() instead of _exit(), so that atexit handlers (profilers, sanitizers) run -- at the price of the piecewise teardown
    const int flush_rc = fflush(NULL);
    if (flush_rc != 0) { fprintf(stderr, "\n[ERROR] could not flush the output streams: %s\n", strerror(errno)); _exit(1); }
    if (getenv("VCFGL_HIP_NORMAL_EXIT")) exit(0);
    _exit(0);
}
