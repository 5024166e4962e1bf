// self_test.h -- the program's self-test hooks: its formatters, encoders and input parser driven from the command line by the tests
#pragma once
#include "sites.h"

static const int NOT_A_HOOK = -1;

// runs the hook argv[1] names and returns its exit code; NOT_A_HOOK when argv[1] names none
static int run_hook(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--format-floats")) {
        // self-test hook of the VCF float formatter: hex float32 bit patterns in, formatted text out
        for (int i = 2; i < argc; i++) { uint32_t b = (uint32_t)strtoul(argv[i], NULL, 16); float f; memcpy(&f, &b, 4); std::string s; put_float(s, f); printf("%s\n", s.c_str()); }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--qs-to-errprob")) {        // test hook: QS_TO_ERRPROB of every argument, 17 digits
        for (int i = 2; i < argc; i++) printf("%.17g\n", host_qs_to_errprob(atoi(argv[i])));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "--encode-ints")) {
        // self-test hook of the BCF writer's integer vectors: --encode-ints <dictionary id> <n> [<int> | . | e ...] prints, in hex, the
        // typed key, the size/type byte(s) and the values ("." missing, "e" vector end) in the type the writer picks for their range
        std::vector<int32_t> v;
        for (int i = 4; i < argc; i++) v.push_back(!strcmp(argv[i], ".") ? VGL_INT32_MISSING : !strcmp(argv[i], "e") ? INT32_MIN + 1 : (int32_t)strtol(argv[i], NULL, 10));
        std::string b;
        vsink::Sink::encode_int_field(b, (int32_t)strtol(argv[2], NULL, 10), atoi(argv[3]), v.data(), v.size());
        for (unsigned char c : b) printf("%02x", c);
        printf("\n");
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "--encode-selftest")) {
        // self-test hook of the BCF writer: --encode-selftest <mode> <out path> <int> [<int> ...] writes one record whose
        // FORMAT/X holds the given integers for sample s1 (and their reverse for s2) and INFO/Y the same list
        vsink::Sink out; out.text_float = put_float;
        std::vector<std::string> hdr = {"##fileformat=VCFv4.2", "##contig=<ID=c1,length=10>",
                                        "##INFO=<ID=Y,Number=.,Type=Integer,Description=\"y\">", "##FORMAT=<ID=X,Number=.,Type=Integer,Description=\"x\">"};
        out.open(argv[3], argv[2][0], hdr, {"s1", "s2"});
        std::vector<int32_t> v; for (int i = 4; i < argc; i++) v.push_back(!strcmp(argv[i], ".") ? VGL_INT32_MISSING : (int32_t)strtol(argv[i], NULL, 10));
        const int n = (int)v.size();
        std::vector<int32_t> plane(2 * (size_t)n);
        for (int k = 0; k < n; k++) { plane[(size_t)k * 2] = v[k]; plane[(size_t)k * 2 + 1] = v[n - 1 - k]; }
        std::string sh = "c1\t5\trs1\tA\tC,<*>\t.\tPASS\tY=";
        for (int k = 0; k < n; k++) { if (k) sh += ','; put_int(sh, v[k]); }
        out.write_rec(sh, {{"X", false, n, plane.data(), 1, 2}});
        out.close();
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "--dump-gt")) {
        // test hook of the input parser: --dump-gt <file> <source 0|1> <mode 0|1|2|3> prints per record line "pos status allelesum row":
        // the row make_site hands to the tile calls in hex, the status of the line (VGL_VCFIN_*: 1 = outside the device parser's plain
        // grammar), through the host parser (0, no GPU needed) or the device parser (1).  For a BCF file: 2 decodes its GT vectors on the
        // device (--device-bcf-input 1), 3 on the host with the status the device would give (VGL_BCFIN_*, from the shared per-sample
        // rule; no GPU needed); with 0 a BCF record has no status (-1)
        Args a; a.source = atoi(argv[3]);
        const int mode = atoi(argv[4]);
        if (a.source < 0 || a.source > 1 || mode < 0 || mode > 3) die("--dump-gt <file> <source 0|1> <mode 0|1|2|3>");
        InputOpt opt; opt.device_input = mode == 1; opt.device_bcf_input = mode == 2; opt.source = a.source; opt.classify = true; opt.classify_bcf = mode == 3; opt.tile_sites = 256;
        Vcf vcf = read_vcf(argv[2], false, 4, opt);
        const int N = (int)vcf.samples.size();
        if (N <= 0) die("no samples in %s", argv[2]);
        std::vector<uint8_t> row((size_t)N); SiteMeta m; std::string line;
        for (const Rec& r : vcf.recs) {
            make_site(a, r, r.pos0, false, N, row.data(), m, nullptr);
            long sum = 0;
            if (r.dev_row) sum = r.dev_sum; else for (int8_t g : r.gt) if (g > 0) sum += g;
            char hb[64]; snprintf(hb, sizeof hb, "%ld %d %ld ", r.pos0 + 1, (int)r.in_status, sum); line = hb;
            for (int s = 0; s < N; s++) { snprintf(hb, sizeof hb, "%02x", row[s]); line += hb; }
            puts(line.c_str());
        }
        return 0;
    }
    return NOT_A_HOOK;
}
