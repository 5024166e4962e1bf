// device_worker.h -- one worker per device: simulates the tiles handed to it, in order
#pragma once

#include "run_plan.h"

struct DeviceWorker {
    const RunPlan& P; vgl_ctx* const ctx; vgl_stream_host* const hs;          // hs: the device's stream handle (--device-stream 1), else null
    const int32_t* const dps; const int32_t n_dps;                             // --gvcf-dps
    std::thread th; std::mutex m; std::condition_variable cv; std::vector<TileBufs*> q; size_t head = 0; bool stop = false;
    long tiles = 0, sites = 0; double t_first = -1.0, t_last = 0.0; double text_bytes = 0.0;          // --verbose 1: what this device did (written by its own thread, read after the join)

    DeviceWorker(const RunPlan& P_, vgl_ctx* ctx_, vgl_stream_host* hs_, const std::vector<int>& gvcf_dps)
        : P(P_), ctx(ctx_), hs(hs_), dps(gvcf_dps.data()), n_dps((int32_t)gvcf_dps.size()) { th = std::thread([this] { run(); }); }
    void push(TileBufs* B) { { std::lock_guard<std::mutex> lk(m); q.push_back(B); } cv.notify_one(); }
    void finish() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all(); th.join(); }

    void run() {
        // a tile is submitted (vgl_simulate_tile_async) before the previous one is waited for: its kernels run while the
        // previous tile's tags are still on their way to the host
        TileBufs* prev = nullptr; int32_t prev_ticket = 0;
        for (;;) {
            TileBufs* B = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                if (!prev) cv.wait(lk, [&] { return stop || head < q.size(); });
                if (head < q.size()) B = q[head++];
                else if (!prev) return;
            }
            int32_t ticket = 0;
            if (B) {
                if (t_first < 0.0) t_first = now_s();
                if (P.device_pileup && vgl_ctx_pileup_next(ctx, &B->pt) != VGL_OK) die("%s", vgl_last_error());   // (a side channel of the tile call below)
                if (P.fetch && vgl_ctx_fetchgl_next(ctx, &B->ft) != VGL_OK) die("%s", vgl_last_error());               // (likewise)
                int rc = VGL_OK;
                switch (P.path) {
                case ARRAYS: rc = vgl_simulate_tile_async(ctx, B->t0, B->ns, B->gt.data(), &B->o, &ticket); break;
                case GVCF: rc = vgl_simulate_tile_gvcf_async(ctx, B->t0, B->ns, B->gt.data(), B->contig.data(), B->pos0.data(), dps, n_dps, &B->o, &B->g, &ticket); break;
                // (--device-stream 1: the text stays on the device, in the entry's body buffer of the stream handle)
                case TEXT: rc = vgl_simulate_tile_text_async(ctx, B->t0, B->ns, B->gt.data(), &B->o, hs ? vgl_stream_host_body(hs, B->sbuf) : B->text.data(),
                                                             B->text_cap, B->toff.data(), &ticket); break;
                }
                if (rc != VGL_OK) die("%s", vgl_last_error());
            }
            if (prev) {
                int wrc = vgl_tile_wait(ctx, prev_ticket);
                if (wrc == VGL_E_ARG && P.inf) {                         // the library names the site; the writer, in site order, reports its position
                    for (int i = 0; i < prev->ns && prev->bad_pos < 0; i++)
                        for (int s = 0; s < P.N; s++) {
                            const uint8_t b = prev->gt[(size_t)i * P.N + s];
                            if ((b & 0xF) > 3 || (b >> 4) > 3) { prev->bad_pos = prev->meta[i].pos0 + 1; break; }
                        }
                    if (prev->bad_pos >= 0) wrc = VGL_OK;                // (the tile is handed on as done; the writer ends the run when it comes to it)
                }
                if (wrc == VGL_E_SETAL) die("--set-alleles: %s.  Every allele of a line must be one of its record's alleles.", vgl_last_error());
                if (wrc != VGL_OK) die("%s", vgl_last_error());
                if (P.path == TEXT && !hs) text_bytes += (double)prev->toff[prev->ns];
                if (P.path == GVCF) text_bytes += (double)prev->g.text_needed;
                if (P.device_pileup) text_bytes += (double)prev->pt.text_needed;
                if (P.fetch) text_bytes += (double)prev->ft.text_needed;
                tiles += 1; sites += prev->ns; t_last = now_s();
                { std::lock_guard<std::mutex> lk(prev->m); prev->done = true; }
                prev->cv.notify_all();
            }
            prev = B; prev_ticket = ticket;
        }
    }
};
