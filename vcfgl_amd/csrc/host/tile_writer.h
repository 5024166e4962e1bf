// tile_writer.h -- everything the writer (the main thread) does with a finished tile, in site order: the TSV lines on stdout, the
// pileup, the gVCF blocks and the records; and the stage timer of --verbose 1, whose stages the writer closes
#pragma once
#include "device_worker.h"
#include "gvcf_blocker.h"
#include "out_header.h"

// --verbose 1: wall-clock seconds per stage on stderr at the end
struct StageTimer {
    enum Stage { READ, SITES, CONTEXT, DEVICE_WAIT, ENCODE, WRITE, TILE_BUFFERS, TEARDOWN, PILEUP, N_STAGES };
    double t[N_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, mark = now_s();
    void restart() { mark = now_s(); }
    void lap(Stage s) { const double now = now_s(); t[s] += now - mark; mark = now; }
    void carve(Stage s, double dt) { t[s] += dt; mark += dt; }          // dt seconds just spent belong to s, not to the stage that laps next
};

struct TileWriter {
    const Args& a; const RunPlan& P; const Vcf& vcf; StageTimer& timer;
    vsink::Sink out;
    FILE* pile_fp = nullptr; vsink::Bgzf pile;            // the reference writes the pileup through htslib's BGZF (vcfgl.cpp:1776-1783)
    GvcfBlocker gv;
    FILE* fetch_fp = nullptr; std::string fetch_buf; long n_fetch_lines = 0, n_fetch_absent = 0;      // --fetch-gl XY: <prefix>.fetchgl.csv
    std::vector<std::string> enc; std::string line, tsv;
    long n_out = 0, n_skipped = 0;
    int n_fmt = 0;                                              // FORMAT fields of a simulated record
    int pre_adjq = -1;                                          // preCalc->adj_qScore
    // --device-stream 1: the devices' stream handles; bytes of heads and offsets sent up and of members brought back, per device (--verbose 1)
    std::vector<vgl_stream_host*> hstream; std::vector<double> stream_up, stream_down;

    TileWriter(const Args& a_, const RunPlan& P_, const Vcf& vcf_, StageTimer& timer_)
        : a(a_), P(P_), vcf(vcf_), timer(timer_), hstream(P_.D, nullptr), stream_up(P_.D, 0.0), stream_down(P_.D, 0.0) { out.text_float = put_float; gv.block_dps = a.gvcf_dps; }

    // the record file, the pileup file and the first lines of the listings on stdout
    void open(const std::vector<vgl_ctx*>& ctxs) {
        // BGZF compression threads: --threads as in the reference; when it is not given, up to 8 (same bytes either way)
        if (!P.rec0) out.open(a.out_prefix + P.ext, P.mode, output_header(a, vcf, P.inf), vcf.samples,
                              a.threads_given ? a.threads : (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())), P.bgzf_dev);
        if (P.bcf) {                                                // dictionary ids of the FORMAT keys: the device writes them as typed keys
            const char* keys[7] = {"DP", "GL", "PL", "GP", "AD", "ADF", "ADR"};
            const int on[7] = {a.add_fmt_dp, a.add_gl, a.add_pl, a.add_gp, a.add_fmt_ad, a.add_fmt_adf, a.add_fmt_adr};
            int32_t ids[7];
            for (int k = 0; k < 7; k++) { ids[k] = on[k] ? out.key_id(keys[k]) : 0; n_fmt += on[k] ? 1 : 0; }
            for (vgl_ctx* ctx : ctxs) if (vgl_ctx_bcf_keys(ctx, ids, 7) != VGL_OK) die("--device-bcf 1: %s", vgl_last_error());
        }
        if (P.fetch) { fetch_fp = fopen((a.out_prefix + ".fetchgl.csv").c_str(), "wb"); if (!fetch_fp) die("Could not open file: %s.fetchgl.csv", a.out_prefix.c_str()); }
        if (a.print_pileup) {
            pile_fp = fopen((a.out_prefix + ".pileup.gz").c_str(), "wb"); if (!pile_fp) die("Could not open pileup output");
            pile.open(pile_fp, 1, P.bgzf_dev);
        }
        // ---- TSV lines on stdout (vcfgl.cpp:430-435, 533-554, 1745-1755)
        int pre_q = -1;                                                             // preCalc->qScore
        if (a.print_bpe && a.error_qs != 1) printf("base_pick_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.error_rate);   // io.cpp:1089-1100
        if (a.error_qs != 2) {
            host_errprob_to_qs(a, a.error_rate, pre_q, pre_adjq);
            if (a.print_gl_err) printf("gl_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.precise_gl ? a.error_rate : host_qs_to_errprob((a.adjust_qs & 1) ? pre_adjq : pre_q));
            if (a.print_qs_err) printf("qs_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.error_rate);
            if (a.print_qscores) printf("qs\tNA\tNA\tNA\tNA\t%d\n", a.adjust_qs ? pre_adjq : pre_q);
        }
    }

    // --device-stream 1: one stream handle per device, created once the contexts know what a tile's bodies can take
    void open_streams(const std::vector<vgl_ctx*>& ctxs) {
        // The largest head of a site, from what build_record writes.  Text: chrom, id, qual, filt and the input's own INFO; POS (at most 20
        // digits); REF and ALT (at most five alleles, the longest "<NON_REF>", with commas: 32); eight tabs; and per INFO tag this run adds
        // ";KEY=" (at most 5) and its numbers with commas, 16 bytes each (an int32 takes 11, kputd's forms and %g of a float 13, the binary
        // placeholder "~%08x" 9): DP 1, QS and the AD tags one per allele (A), I16 16.  BCF (encode_head): 8 bytes of lengths, 24 of fixed
        // fields, and every column typed -- a string or vector costs at most 5 bytes over its text, an added number 4 bytes, and the
        // input's INFO at most twice its text (a one-digit number with its comma becomes a 4-byte float): bounded by the same sum with
        // the INFO doubled and 64 bytes more.  The handle refuses a tile whose heads take more.
        size_t longest = 0;
        for (const Rec& r : vcf.recs) longest = std::max(longest, r.chrom.size() + r.id.size() + r.qual.size() + r.filt.size() + 2 * r.info.size());
        const size_t A = (size_t)P.A;
        const size_t n_added = (a.add_info_dp ? 1 : 0) + (a.add_qs ? A : 0) + (a.add_i16 ? 16 : 0) + A * ((a.add_info_ad ? 1 : 0) + (a.add_info_adf ? 1 : 0) + (a.add_info_adr ? 1 : 0));
        const size_t per_site = longest + 20 + 32 + 8 + 6 * 5 + 16 * n_added + 64 + 64;
        const int64_t max_head = (int64_t)P.TS * (int64_t)per_site;
        for (int d = 0; d < P.D; d++) {
            const int64_t cap = vgl_ctx_text_bound(ctxs[d], P.TS);
            if (cap < 0) die("--device-stream 1: %s", vgl_last_error());
            if (vgl_stream_host_create(P.devices[d], P.R / P.D, P.TS, max_head, std::max<int64_t>(cap, 1), &hstream[d]) != VGL_OK)
                die("--device-stream 1: %s (device %d)", vgl_last_error(), P.devices[d]);
            if (vgl_ctx_text_device(ctxs[d], 1) != VGL_OK) die("--device-stream 1: %s", vgl_last_error());
        }
    }

    // one simulated record of a tile: the eight fixed columns as text, the allele strings and the
    // typed FORMAT arrays (reads the tile buffers only: records of a tile are built on several threads)
    void build_record(const TileBufs& B, int i, std::string& line, std::vector<std::string>& al, std::vector<vsink::FmtDesc>& fmt) const {
        const SiteMeta& S = B.meta[i];
        const int N = P.N, A = P.A, G = P.G;
        const int nA = B.na[i], nG = nA * (nA + 1) / 2;
        char hb[64];
        line += S.rec->chrom; snprintf(hb, sizeof hb, "\t%ld\t", S.pos0 + 1); line += hb;
        line += S.rec->id; line += '\t';
        // alleles (vcfgl.cpp:739-762; no-reads site :250-280)
        al.clear();
        for (int k = 0; k < nA; k++) al.push_back(allele_name(B.a2b[(size_t)i * 5 + k], P.nonref));
        if (al.empty()) al.push_back(".");
        line += al[0]; line += '\t';
        if (al.size() == 1) line += '.';
        else for (size_t k = 1; k < al.size(); k++) { if (k > 1) line += ','; line += al[k]; }
        line += '\t'; line += S.rec->qual; line += '\t'; line += S.rec->filt; line += '\t';
        // INFO in add_tags() order: DP, QS, I16, AD, ADF, ADR (after the input record's own INFO)
        std::string info = (S.rec->info == ".") ? "" : S.rec->info;
        auto add_key = [&](const char* k) { if (!info.empty()) info += ';'; info += k; info += '='; };
        if (a.add_info_dp) { add_key("DP"); put_int(info, B.idp[i]); }
        if (a.add_qs) { add_key("QS"); for (int k = 0; k < nA; k++) { if (k) info += ','; out.put_float(info, B.qs[(size_t)i * A + k]); } }
        if (a.add_i16) { add_key("I16"); for (int k = 0; k < 16; k++) { if (k) info += ','; out.put_float(info, B.i16[(size_t)i * 16 + k]); } }
        if (a.add_info_ad) { add_key("AD"); for (int k = 0; k < nA; k++) { if (k) info += ','; put_int(info, B.iad[(size_t)i * A + k]); } }
        if (a.add_info_adf) { add_key("ADF"); for (int k = 0; k < nA; k++) { if (k) info += ','; put_int(info, B.iadf[(size_t)i * A + k]); } }
        if (a.add_info_adr) { add_key("ADR"); for (int k = 0; k < nA; k++) { if (k) info += ','; put_int(info, B.iadr[(size_t)i * A + k]); } }
        line += info.empty() ? "." : info;
        // FORMAT keys: DP, GL, PL, GP, AD, ADF, ADR.  The library writes the multi-valued tags sample-major (VGL_LAYOUT_SAMPLE_MAJOR):
        // the slab of site i holds the record's array as the reference keeps it for bcf_update_format_*(), element k of sample s
        // at slab[s * n + k] with the site's own n -- the encoders below read (and for BCF copy) it front to back
        fmt.clear();
        if (P.path != ARRAYS) return;                            // the sample columns come from the device
        const size_t sN = (size_t)N, sG = (size_t)nG, sA = (size_t)nA;
        if (a.add_fmt_dp) fmt.push_back({"DP", false, 1, &B.dp[(size_t)i * N], 1, sN});
        if (a.add_gl) fmt.push_back({"GL", true, nG, &B.gl[(size_t)i * G * N], sG, 1});
        if (a.add_gp && P.inf) fmt.push_back({"GP", true, nG, &B.gp[(size_t)i * G * N], sG, 1});     // (true values: GL, GP, PL -- vcfgl.cpp:1243-1259)
        if (a.add_pl) fmt.push_back({"PL", false, nG, &B.pl[(size_t)i * G * N], sG, 1});
        if (a.add_gp && !P.inf) fmt.push_back({"GP", true, nG, &B.gp[(size_t)i * G * N], sG, 1});
        if (a.add_fmt_ad) fmt.push_back({"AD", false, nA, &B.ad[(size_t)i * A * N], sA, 1});
        if (a.add_fmt_adf) fmt.push_back({"ADF", false, nA, &B.adf[(size_t)i * A * N], sA, 1});
        if (a.add_fmt_adr) fmt.push_back({"ADR", false, nA, &B.adr[(size_t)i * A * N], sA, 1});
    }
    // the alleles of site i as a gVCF block names them: "A,<NON_REF>"
    std::string site_alleles(const TileBufs& B, int i) const {
        std::string s;
        for (int k = 0; k < B.na[i]; k++) { if (k) s += ','; s += allele_name(B.a2b[(size_t)i * 5 + k], P.nonref); }
        return s.empty() ? std::string(".") : s;
    }
    void emit_block() { gv.emit(out, P.N); n_out++; }

    // --device-gvcf 1: a tile's items in order.  Records and blocks get their fixed columns here (in parallel) and their sample
    // columns from the device; the tile's last block stays open on the host (GvcfBlocker's state) and takes in the first block of a
    // later tile that continues it (same contig, pos0 <= END + 1, same range): min / lexicographic-min aggregates, founder from the left
    void write_gvcf_tile(const TileBufs& B) {
        const int N = P.N, A = P.A;
        const vgl_gvcf_tile& g = B.g;
        const int ni = g.n_items;
        const vgl_gvcf_item* it = g.items;
        auto pl_count_die = [&](int nA) { die("Unexpected number of PL values: %d", N * nA * (nA + 1) / 2); };
        bool merge = false;
        if (ni > 0 && it[0].kind == VGL_GVCF_BLOCK) {
            const int f = it[0].first;
            merge = gv.continues(B.meta[f].rec->chrom, B.meta[f].pos0, it[0].dpr);
            if (merge && (B.na[f] != 2 || gv.pl.size() != (size_t)N * 3)) pl_count_die(B.na[f]);
        }
        if (g.error_site >= 0) pl_count_die(B.na[g.error_site]);
        enc.resize(std::max(ni, 1));
        vsink::parallel_for(ni, P.enc_threads, [&](int k) {
            enc[k].clear();
            const vgl_gvcf_item& t = it[k];
            std::string sh8; std::string& col = P.bcf ? sh8 : enc[k];    // --device-bcf 1: the fixed columns become the record's shared block
            if (t.kind == VGL_GVCF_RECORD) {
                std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt; build_record(B, t.first, col, al, fmt);
                if (P.bcf) out.encode_head(sh8, (uint32_t)n_fmt, (size_t)(B.toff[t.first + 1] - B.toff[t.first]), enc[k]);
                return;
            }
            if ((k == 0 && merge) || k == ni - 1) return;            // carried on the host
            const int f = t.founder;
            GvcfBlocker::fixed_columns(col, out, B.meta[f].rec->chrom, B.meta[f].pos0, B.meta[t.last].pos0, site_alleles(B, f), t.min_dp,
                                       a.add_qs ? &B.qs[(size_t)f * A] : nullptr, a.add_qs ? (size_t)B.na[f] : 0);
            if (P.bcf) out.encode_head(sh8, 2, (size_t)(B.boff[t.block + 1] - B.boff[t.block]), enc[k]);        // PL, DP
        });
        timer.lap(StageTimer::ENCODE);
        for (int k = 0; k < ni; k++) {
            const vgl_gvcf_item& t = it[k];
            if (t.kind == VGL_GVCF_BLOCK && k == 0 && merge) {
                gv.merge(t.min_dp, B.fdp.data(), B.fpl.data(), N, B.meta[t.last].pos0);
                if (k < ni - 1) emit_block();
                continue;
            }
            if (gv.current_dpr != 0) emit_block();
            if (t.kind == VGL_GVCF_BLOCK && k == ni - 1) {               // the tile's last block: open until a later tile decides
                const int f = t.founder, nA = B.na[f];
                gv.open(B.meta[f].rec->chrom, B.meta[f].pos0, B.meta[t.last].pos0, site_alleles(B, f), t.dpr, t.min_dp, (ni == 1) ? B.fdp.data() : B.ldp.data(),
                        (ni == 1) ? B.fpl.data() : B.lpl.data(), N, nA * (nA + 1) / 2, a.add_qs ? &B.qs[(size_t)f * A] : nullptr, nA);
                continue;
            }
            out.put(enc[k]);
            if (t.kind == VGL_GVCF_BLOCK) out.put(B.text.data() + B.boff[t.block], (size_t)(B.boff[t.block + 1] - B.boff[t.block]));
            else out.put(B.text.data() + B.toff[t.first], (size_t)(B.toff[t.first + 1] - B.toff[t.first]));
            n_out++;
        }
        timer.lap(StageTimer::WRITE);
    }

    // --device-stream 1: the members of a tile whose heads were submitted: to the file, in tile order
    void retire_tile(TileBufs& B) {
        const uint8_t* m; int64_t mn, raw;
        if (vgl_stream_host_wait(hstream[B.dev], B.sticket, &m, &mn, &raw) != VGL_OK) die("--device-stream 1: %s", vgl_last_error());
        if (raw != B.hoff[B.ns] + B.toff[B.ns]) die("--device-stream 1: the device assembled %lld bytes of %lld", (long long)raw, (long long)(B.hoff[B.ns] + B.toff[B.ns]));
        out.put_members(m, (size_t)mn);
        stream_down[B.dev] += (double)mn;
        B.sticket = -1;
    }

    // the per-read / per-site TSV lines of site i on stdout, for the sites that reach the read loop (vcfgl.cpp:396-404)
    void dump_tsv(const TileBufs& B, int i) {
        if (!(P.dump_pick || P.dump_reads) || B.st[i] == VGL_SITE_SKIP_EMPTY || B.idp[i] <= 0) return;
        const SiteMeta& S = B.meta[i];
        const int N = P.N, ns = B.ns;
        tsv.clear();
        char hb[96];
        if (P.dump_pick) for (int s = 0; s < N; s++) {                                   // vcfgl.cpp:430-435
            tsv += "base_pick_error_prob\t"; tsv += vcf.samples[s]; tsv += '\t'; tsv += S.rec->chrom;
            snprintf(hb, sizeof hb, "\t%ld\tNA\t%f\n", S.pos0 + 1, B.pick[i]); tsv += hb;
        }
        if (P.dump_reads) for (int s = 0; s < N; s++) {                                  // vcfgl.cpp:533-554
            const int n = B.dp[(size_t)i * N + s];
            for (int r = 0; r < n; r++) {
                const double ep = B.errp[((size_t)r * ns + i) * N + s];
                int q, aq; host_errprob_to_qs(a, ep, q, aq);
                auto head = [&](const char* type) { tsv += type; tsv += '\t'; tsv += vcf.samples[s]; tsv += '\t'; tsv += S.rec->chrom; snprintf(hb, sizeof hb, "\t%ld\t%d\t", S.pos0 + 1, r); tsv += hb; };
                if (a.print_qs_err) { head("qs_error_prob"); snprintf(hb, sizeof hb, "%f\n", ep); tsv += hb; }
                if (a.print_qscores) { head("qs"); snprintf(hb, sizeof hb, "%d\n", (a.adjust_qs & 8) ? aq : q); tsv += hb; }
                if (a.print_gl_err) { head("gl_error_prob"); snprintf(hb, sizeof hb, "%f\n", a.precise_gl ? ep : host_qs_to_errprob((a.adjust_qs & 16) ? aq : q)); tsv += hb; }
            }
        }
        fwrite(tsv.data(), 1, tsv.size(), stdout);
    }

    // the pileup line of site i: vcfgl.cpp:414-416, 616-634 (printed before skip decisions)
    void pileup_line(const TileBufs& B, int i) {
        if (!pile_fp || B.st[i] == VGL_SITE_SKIP_EMPTY) return;
        const SiteMeta& S = B.meta[i];
        const int N = P.N, ns = B.ns;
        const double t_pile = now_s();
        line.clear();
        char hb[64]; snprintf(hb, sizeof hb, "\t%ld\t%c", S.pos0 + 1, S.ref_char);
        line += S.rec->chrom; line += hb;
        if (P.device_pileup) {                                      // the prefix here, the sample columns and the newline from the device
            pile.write(line.data(), line.size());
            pile.write(B.ptext.data() + B.poff[i], (size_t)(B.poff[i + 1] - B.poff[i]));
        } else {
            for (int s = 0; s < N; s++) {
                const int n = B.dp[(size_t)i * N + s];
                if (n == 0) { line += "\t0\t*\t*"; continue; }
                snprintf(hb, sizeof hb, "\t%d\t", n); line += hb;
                for (int r = 0; r < n; r++) line += "ACGT"[B.reads[((size_t)r * ns + i) * N + s] & 3];
                line += '\t';
                if (!(a.adjust_qs & 4)) for (int r = 0; r < n; r++) line += (char)((B.reads[((size_t)r * ns + i) * N + s] >> 2) + 33);
                else if (a.error_qs != 2) line.append((size_t)n, (char)(pre_adjq + 33));                  // PROGRAM_WILL_ADJUST_QS_FOR_PILEUP
                else for (int r = 0; r < n; r++) { int q, aq; host_errprob_to_qs(a, B.errp[((size_t)r * ns + i) * N + s], q, aq); line += (char)(aq + 33); }
            }
            line += '\n';
            pile.write(line.data(), line.size());
        }
        timer.carve(StageTimer::PILEUP, now_s() - t_pile);          // --verbose 1: the pileup's own stage, out of write/compress
    }

    // --fetch-gl XY: "POS," here, the values and the newline from the device; a record without the genotype has no line
    void fetch_lines(const TileBufs& B) {
        fetch_buf.clear();
        char hb[32];
        for (int i = 0; i < B.ns; i++) {
            const int64_t b = B.foff[i], e = B.foff[i + 1];
            if (e <= b) { if (B.st[i] >= 0) n_fetch_absent++; continue; }
            snprintf(hb, sizeof hb, "%ld,", B.meta[i].pos0 + 1); fetch_buf += hb;
            fetch_buf.append((const char*)B.ftext.data() + b, (size_t)(e - b));
            n_fetch_lines++;
        }
        if (!fetch_buf.empty() && fwrite(fetch_buf.data(), 1, fetch_buf.size(), fetch_fp) != fetch_buf.size()) die("Could not write file: %s.fetchgl.csv", a.out_prefix.c_str());
    }
    void close_fetch() { if (fetch_fp && fclose(fetch_fp) != 0) die("Could not write file: %s.fetchgl.csv", a.out_prefix.c_str()); fetch_fp = nullptr; }

    bool skipped(const TileBufs& B, int i) { if (B.st[i] >= 0) return false; n_skipped++; return true; }

    // -doGVCF 1 on the host: write_record_values (vcfgl.cpp:167-206) carries the open block from record to record (and from tile to
    // tile, whichever device simulated it)
    void host_gvcf_site(const TileBufs& B, int i) {
        const SiteMeta& S = B.meta[i];
        const int N = P.N, A = P.A, G = P.G;
        std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt;
        line.clear();
        build_record(B, i, line, al, fmt);
        SiteView sv;
        sv.chrom = &S.rec->chrom; sv.pos0 = S.pos0; sv.n_obs = B.nobs[i]; sv.n_alleles = B.na[i]; sv.N = N; sv.G = G;
        sv.dp = &B.dp[(size_t)i * N]; sv.pl = &B.pl[(size_t)i * G * N]; sv.qs = a.add_qs ? &B.qs[(size_t)i * A] : nullptr;
        sv.alleles = al[0]; for (size_t k = 1; k < al.size(); k++) { sv.alleles += ','; sv.alleles += al[k]; }
        int ret = gv.prepare(&sv);
        if (ret == GvcfBlocker::FLUSH_BLOCK) { emit_block(); ret = gv.prepare(&sv); }
        if (ret == GvcfBlocker::WRITE_SIMREC) { out.write_rec(line, fmt); n_out++; }
    }

    // the plain records of a tile: encoded on enc_threads threads, then written in site order -- or, --device-stream 1, their heads
    // go up and the device puts the records together and compresses them
    void write_records(TileBufs& B) {
        const int ns = B.ns;
        enc.resize(ns);
        vsink::parallel_for(ns, P.enc_threads, [&](int i) {
            enc[i].clear();
            if (B.st[i] < 0) return;
            std::string sh; std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt;
            build_record(B, i, sh, al, fmt);
            if (P.bcf) { out.encode_head(sh, (uint32_t)n_fmt, (size_t)(B.toff[i + 1] - B.toff[i]), enc[i]); return; }
            if (P.path == TEXT) { enc[i] = std::move(sh); return; }
            out.encode_rec(sh, fmt, enc[i]);
        });
        if (P.stream) {
            B.heads.clear();
            for (int i = 0; i < ns; i++) { B.hoff[i] = (int64_t)B.heads.size(); B.heads += enc[i]; if (B.st[i] >= 0) n_out++; }
            B.hoff[ns] = (int64_t)B.heads.size();
            timer.lap(StageTimer::ENCODE);
            if (vgl_stream_host_submit(hstream[B.dev], B.sbuf, ns, (const uint8_t*)B.heads.data(), B.hoff.data(), B.toff.data(), &B.sticket) != VGL_OK)
                die("--device-stream 1: %s", vgl_last_error());
            stream_up[B.dev] += (double)B.heads.size() + 16.0 * (ns + 1);
            timer.lap(StageTimer::WRITE);
            return;
        }
        timer.lap(StageTimer::ENCODE);
        for (int i = 0; i < ns; i++) if (B.st[i] >= 0) {
            out.put(enc[i]);
            if (P.path == TEXT) out.put(B.text.data() + B.toff[i], (size_t)(B.toff[i + 1] - B.toff[i]));     // tab, FORMAT, the sample columns, newline
            n_out++;
        }
        timer.lap(StageTimer::WRITE);
    }

    // One finished tile.  The per-site jobs run in this order for each site: it decides stdout, the pileup and the gVCF carry.
    void write_tile(TileBufs& B) {
        for (int i = 0; i < B.ns; i++) {
            dump_tsv(B, i);
            pileup_line(B, i);
            if (skipped(B, i)) continue;
            if (a.do_gvcf && P.path != GVCF) host_gvcf_site(B, i);   // (plain records, device gVCF: written below)
        }
        if (P.fetch) fetch_lines(B);
        if (P.rec0) return;                                      // (no listing, no pileup, no record: the sites were counted)
        if (P.path == GVCF) write_gvcf_tile(B);
        if (!a.do_gvcf) write_records(B);
    }

    // the end of the record stream: the block still open
    void flush_gvcf() { if (a.do_gvcf && gv.prepare(nullptr) == GvcfBlocker::FLUSH_BLOCK) emit_block(); }
};
