// The launch plan (vcfgl_amd/csrc/hostlib/plan.h, with the tables of hostlib/tables.h) on the CPU: reads the cases of
// tests/ctx_plan_cases.py, one per line as `name key=value ...` (case_line), runs vgl_plan without hooks and prints for each
// `name field=value ...` with the fields of vgl_ctx_info the plan decides (vgl_plan_info: the library's own derivation), or
// `name code=<return code> error=<text>` for a refusal.  Built with -fsanitize=address,undefined by tests/test_plan_core_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/vcfgl_hip.h"
#include "vgl_device.h"
#include "hostlib/tables.h"
#include "hostlib/plan.h"

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string w; std::getline(ss, w, sep);) out.push_back(w);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: plan_core_main CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    int n_cases = 0;
    for (std::string line; std::getline(in, line);) {
        const std::vector<std::string> words = split(line, ' ');
        if (words.empty()) continue;
        vgl_params p;
        memset(&p, 0, sizeof p);
        std::vector<double> depths; std::vector<int32_t> bins;
        int max_sites = 0;
        for (size_t i = 1; i < words.size(); i++) {
            const size_t eq = words[i].find('=');
            const std::string k = words[i].substr(0, eq), v = words[i].substr(eq + 1);
            const long long iv = strtoll(v.c_str(), nullptr, 10);
            const double dv = strtod(v.c_str(), nullptr);
#define INT_FIELD(f) if (k == #f) { p.f = (int32_t)iv; continue; }
#define DBL_FIELD(f) if (k == #f) { p.f = dv; continue; }
            INT_FIELD(abi_version) INT_FIELD(seed) INT_FIELD(n_samples) INT_FIELD(rng_mode) INT_FIELD(beta_sampler) INT_FIELD(error_qs)
            INT_FIELD(gl_model) INT_FIELD(precise_gl) INT_FIELD(adjust_qs) INT_FIELD(n_qs_bins) INT_FIELD(i16_mapq) INT_FIELD(do_unobserved)
            INT_FIELD(rm_invar_sites) INT_FIELD(rm_empty_sites) INT_FIELD(do_gvcf) INT_FIELD(add_gl) INT_FIELD(add_gp) INT_FIELD(add_pl)
            INT_FIELD(add_i16) INT_FIELD(add_qs) INT_FIELD(add_fmt_dp) INT_FIELD(add_info_dp) INT_FIELD(add_fmt_ad) INT_FIELD(add_info_ad)
            INT_FIELD(add_fmt_adf) INT_FIELD(add_info_adf) INT_FIELD(add_fmt_adr) INT_FIELD(add_info_adr) INT_FIELD(out_layout)
            DBL_FIELD(depth) DBL_FIELD(error_rate) DBL_FIELD(beta_variance) DBL_FIELD(gl1_theta) DBL_FIELD(adjust_by)
            if (k == "max_sites") { max_sites = (int)iv; continue; }
            if (k == "depths") { for (const std::string& w : split(v, ',')) depths.push_back(strtod(w.c_str(), nullptr)); continue; }
            if (k == "qs_bins") { for (const std::string& w : split(v, ',')) bins.push_back((int32_t)strtol(w.c_str(), nullptr, 10)); continue; }
            if (k == "layout") {
                const std::vector<std::string> w = split(v, ',');
                if (w.size() != 6) { fprintf(stderr, "%s: layout takes 6 values\n", words[0].c_str()); return 2; }
                p.layout.block = strtoull(w[0].c_str(), nullptr, 10);
                for (int j = 0; j < 4; j++) p.layout.off[j] = strtoull(w[1 + j].c_str(), nullptr, 10);
                p.layout.qs_read_stride = strtoull(w[5].c_str(), nullptr, 10);
                continue;
            }
            fprintf(stderr, "%s: unknown key %s\n", words[0].c_str(), k.c_str());
            return 2;
        }
        if (!depths.empty()) p.depths = depths.data();
        if (!bins.empty()) p.qs_bins = bins.data();
        VglDevParams D; VglPlanExtra X;
        char err[VGL_PLAN_ERR] = "";
        const int rc = vgl_plan(&p, max_sites, 0, vgl_no_env, &D, &X, err);
        ++n_cases;
        if (rc != VGL_OK) { printf("%s code=%d error=%s\n", words[0].c_str(), rc, err); continue; }
        vgl_ctx_info_t r;
        memset(&r, 0, sizeof r);
        r.size = (int32_t)sizeof r;
        vgl_plan_info(D, p.rng_mode, max_sites, &r);
        printf("%s size=%d abi_version=%d n_samples=%d max_sites_per_tile=%d max_alleles=%d max_genotypes=%d rng_mode=%d depth_mode=%d fused=%d fused_split=%d "
               "sample_lean=%d gl_sort=%d gl_wpb=%d read_cap=%d pool_cap=%d pool_lds_bytes=%d rng_tile_max_sites=%lld\n",
               words[0].c_str(), r.size, r.abi_version, r.n_samples, r.max_sites_per_tile, r.max_alleles, r.max_genotypes, r.rng_mode, r.depth_mode, r.fused,
               r.fused_split, r.sample_lean, r.gl_sort, r.gl_wpb, r.read_cap, r.pool_cap, r.pool_lds_bytes, (long long)r.rng_tile_max_sites);
    }
    return n_cases > 0 ? 0 : 2;
}
